// inst_mla_sparse_prefill_fp8.hip -- the kernels of flash_attention_mla_sparse_prefill / _paged on an fp8 (e4m3fn) cache
// (mla_sparse_prefill.hip.h): the KV8 form of the 128-head sparse MLA prefill kernel in its two cache forms.  A
// unit of its own, built as inst_mla_sparse_fp8.hip is: the MFMAs in VGPR form and no packed fp32 arithmetic (the Makefile's two flags).
#include "mla_sparse_prefill.hip.h"

namespace fa {

int mla_sparse_prefill_fp8_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparsePrefillParams& p) {
    if (!p.indices || !p.cu_q || (paged && !p.block_table)) return FA_ERR_NULL_POINTER;   // (what the kernels dereference unconditionally)
    using F = MlaSparsePrefillCfg;
    const Kernel k = paged ? kernel_of<mla_sparse_prefill_kernel<true, true>>(F::LDS_BYTES)
                           : kernel_of<mla_sparse_prefill_kernel<false, true>>(F::LDS_BYTES);
    return (int)launch(k, grid, F::THREADS, F::LDS_BYTES, st, p);
}

}  // namespace fa
