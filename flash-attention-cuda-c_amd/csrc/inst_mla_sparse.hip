// inst_mla_sparse.hip -- the kernels of flash_attention_mla_sparse_decode / _paged (mla_sparse.hip.h): the sparse MLA
// split kernel in its two bf16 cache forms, and its guarded combine at D = 512.  Built as inst_mla_decode.hip is: the MFMAs in VGPR form
// (the Makefile's flag), launch bounds (256, 1).
#include "mla_sparse.hip.h"

namespace fa {

int mla_sparse_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparseParams& p) {
    if (!p.indices || (paged && !p.block_table)) return FA_ERR_NULL_POINTER;   // (what the kernels dereference unconditionally)
    const Kernel k = paged ? kernel_of<mla_sparse_kernel<true>>(MlaCfg::LDS_BYTES) : kernel_of<mla_sparse_kernel<false>>(MlaCfg::LDS_BYTES);
    return (int)launch(k, grid, MlaCfg::THREADS, MlaCfg::LDS_BYTES, st, p);
}

int mla_sparse_combine_launch(unsigned rows, hipStream_t st, const MlaSparseParams& p) {
    return (int)launch(kernel_of<mla_sparse_combine_kernel<MlaCfg::DL>>(0), rows, 256, 0, st, p);
}

}  // namespace fa
