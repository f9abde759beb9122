// inst_mla_sparse_fp8.hip -- the kernels of flash_attention_mla_sparse_decode_fp8 / _paged_fp8 (mla_sparse.hip.h):
// the KV8 form of the sparse MLA split kernel in its two cache forms.  A unit of its own, built as inst_mla_decode_fp8.hip is: the MFMAs
// in VGPR form and no packed fp32 arithmetic (the Makefile's two flags).  The combine is inst_mla_sparse.hip's.
#include "mla_sparse.hip.h"

namespace fa {

int mla_sparse_fp8_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparseParams& p) {
    if (!p.indices || (paged && !p.block_table)) return FA_ERR_NULL_POINTER;   // (what the kernels dereference unconditionally)
    const Kernel k = paged ? kernel_of<mla_sparse_kernel<true, true>>(MlaCfg::LDS_BYTES) : kernel_of<mla_sparse_kernel<false, true>>(MlaCfg::LDS_BYTES);
    return (int)launch(k, grid, MlaCfg::THREADS, MlaCfg::LDS_BYTES, st, p);
}

}  // namespace fa
