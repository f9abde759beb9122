// inst_mla_decode_fp8.hip -- the kernels of flash_attention_mla_decode_fp8 / _paged_fp8 (mla_decode.hip.h): the KV8
// form of the MLA split kernel in its two cache forms.  A unit of its own beside inst_mla_decode.hip, so that it can be built without
// packed fp32 arithmetic (the Makefile's second flag, as for the MLA prefill kernel) while the bf16 unit stays the object it was; the
// MFMAs in VGPR form as there.  The combine is inst_mla_decode.hip's.
#include "mla_decode.hip.h"

namespace fa {

int mla_decode_fp8_launch(bool paged, unsigned grid, hipStream_t st, const DecodeParams& p) {
    if (paged && !p.block_table) return FA_ERR_NULL_POINTER;   // (what the paged kernel dereferences unconditionally)
    const Kernel k = paged ? kernel_of<mla_decode_kernel<true, true>>(MlaCfg::LDS_BYTES) : kernel_of<mla_decode_kernel<false, true>>(MlaCfg::LDS_BYTES);
    return (int)launch(k, grid, MlaCfg::THREADS, MlaCfg::LDS_BYTES, st, p);
}

}  // namespace fa
