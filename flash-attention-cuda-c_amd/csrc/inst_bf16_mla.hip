// inst_bf16_mla.hip -- the kernels of flash_attention_mla_prefill (fwd_mla.hip.h): bf16 Q, K, V with 192 score
// and 128 value columns, with and without the top-left mask, O in fp32, bf16 or fp16.  Built with the MFMAs in VGPR form (the Makefile's
// flag): launch bounds (256, 1), and the 128 accumulator registers of O^T are rescaled by the VALU at every key tile.
#include "fwd_mla.hip.h"

namespace fa {

Kernel mla_prefill_kernel(bool causal, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        return by_bool(causal, [&]<bool CAUSAL>() { return kernel_of<fwd_mla_kernel<OutT, CAUSAL>>(MlaPrefillCfg::LDS_BYTES); });
    });
}

}  // namespace fa
