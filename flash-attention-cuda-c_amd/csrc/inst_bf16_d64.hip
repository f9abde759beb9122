// inst_bf16_d128.hip -- bf16 inputs, MFMA kernel at D = 64 (one translation unit of libflash_attention.so: see launchers.hip.h).
#include "kernel_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel bf16_d64_kernel(bool causal, bool pad, bool lse, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        return by_bool(pad, [&]<bool PAD>() {
            // without the mask (16x16x32 engine) a call that also wants the LSE runs the instantiation that sums the unrounded weights;
            // the causal kernels (32x32x16 engine) sum unrounded weights anyway
            using C = ProdCfg<64, true, OutT, 2, false, PAD>;
            using N = ProdCfg<64, false, OutT, 2, false, PAD>;
            using L = ProdCfg<64, false, OutT, 2, false, PAD, true>;
            if (causal) return kernel_of<fwd_mfma_kernel<C>>(C::LDS_BYTES);
            return lse ? kernel_of<fwd_mfma_kernel<L>>(L::LDS_BYTES) : kernel_of<fwd_mfma_kernel<N>>(N::LDS_BYTES);
        });
    });
}

}  // namespace fa
