// inst_f32_d128.hip -- fp32 inputs, exact-fp32 MFMA kernel at D = 128 (one translation unit of libflash_attention.so: see launchers.hip.h).
#include "kernel_f32.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel f32_d128_kernel(bool causal, bool pad, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        return by_bool(causal, [&]<bool CAUSAL>() {
            return by_bool(pad, [&]<bool PAD>() {
                using C = F32Cfg<128, CAUSAL, OutT, PAD>;
                return kernel_of<fwd_f32_mfma_kernel<C>>(C::LDS_BYTES);
            });
        });
    });
}

}  // namespace fa
