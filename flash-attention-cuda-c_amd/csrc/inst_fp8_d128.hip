// inst_fp8_d128.hip -- fp8 e4m3fn inputs, MFMA kernel at D = 128 (one translation unit of libflash_attention.so: see launchers.hip.h).
#include "kernel_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

// (the fp8 kernels run the 32x32x16 engine, which sums unrounded weights: no separate LSE instantiation)
Kernel fp8_d128_kernel(bool causal, bool pad, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        return by_bool(causal, [&]<bool CAUSAL>() {
            return by_bool(pad, [&]<bool PAD>() {
                using C = ProdCfg<128, CAUSAL, OutT, 1, false, PAD>;
                return kernel_of<fwd_mfma_kernel<C>>(C::LDS_BYTES);
            });
        });
    });
}

}  // namespace fa
