// inst_mla_sparse_prefill.hip -- the kernels of flash_attention_mla_sparse_prefill / _paged on a bf16 cache (mla_sparse_prefill.hip.h;
// DESIGN.md section 42): the 128-head sparse MLA prefill kernel in its two bf16 cache forms.  Built as inst_mla_sparse.hip is: the
// MFMAs in VGPR form (the Makefile's flag); launch bounds (512, 1), eight waves of at most 256 registers.
#include "mla_sparse_prefill.hip.h"

namespace fa {

int mla_sparse_prefill_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparsePrefillParams& p) {
    if (!p.indices || !p.cu_q || (paged && !p.block_table)) return FA_ERR_NULL_POINTER;   // (what the kernels dereference unconditionally)
    using F = MlaSparsePrefillCfg;
    const Kernel k = paged ? kernel_of<mla_sparse_prefill_kernel<true>>(F::LDS_BYTES) : kernel_of<mla_sparse_prefill_kernel<false>>(F::LDS_BYTES);
    return (int)launch(k, grid, F::THREADS, F::LDS_BYTES, st, p);
}

}  // namespace fa
