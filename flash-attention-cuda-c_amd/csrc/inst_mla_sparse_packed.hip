// inst_mla_sparse_packed.hip -- the kernels of flash_attention_mla_sparse_decode_packed / _paged_packed (mla_sparse.hip.h; DESIGN.md
// section 41): the sparse MLA split kernel on the 656-byte packed fp8 row, in its two cache forms.  A unit of its own, built as
// inst_mla_sparse_fp8.hip is: the MFMAs in VGPR form and no packed fp32 arithmetic (the Makefile's two flags).  The combine is
// inst_mla_sparse.hip's.
#include "mla_sparse.hip.h"

namespace fa {

int mla_sparse_packed_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparseParams& p) {
    if (!p.indices || (paged && !p.block_table)) return FA_ERR_NULL_POINTER;   // (what the kernels dereference unconditionally)
    const Kernel k = paged ? kernel_of<mla_sparse_packed_kernel<true>>(MlaCfg::LDS_BYTES) : kernel_of<mla_sparse_packed_kernel<false>>(MlaCfg::LDS_BYTES);
    return (int)launch(k, grid, MlaCfg::THREADS, MlaCfg::LDS_BYTES, st, p);
}

}  // namespace fa
