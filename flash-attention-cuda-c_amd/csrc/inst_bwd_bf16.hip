// inst_bwd_bf16.hip -- the backward pass's kernels, bf16 Q/K/V at D = 64 / 128 (one translation unit of libflash_attention.so: see
// launchers.hip.h and bwd_bf16.hip.h).
#include "bwd_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

// O / dO type (fp32 or bf16) for a runtime code; `f.template operator()<T>()`
template <class F>
Kernel by_io(int dtype, F f) {
    return dtype == FA_DTYPE_F32 ? f.template operator()<float>() : f.template operator()<__bf16>();
}

Kernel bwd_pre_kernel_of(int d, int o_dtype) {
    return by_io(o_dtype, [&]<class OT>() {
        return d == 128 ? kernel_of<bwd_pre_kernel<128, OT>>(0) : kernel_of<bwd_pre_kernel<64, OT>>(0);
    });
}

Kernel bwd_main_kernel_of(int d, bool causal, int o_dtype, int grad_dtype, bool grouped) {
    return by_io(o_dtype, [&]<class OT>() {
        return by_io(grad_dtype, [&]<class GT>() {
            return by_bool(causal, [&]<bool CAUSAL>() {
                return by_bool(grouped, [&]<bool GROUPED>() {
                    return d == 128 ? kernel_of<bwd_main_kernel<128, CAUSAL, OT, GT, GROUPED>>(BwdCfg<128>::LDS_BYTES)
                                    : kernel_of<bwd_main_kernel<64, CAUSAL, OT, GT, GROUPED>>(BwdCfg<64>::LDS_BYTES);
                });
            });
        });
    });
}

Kernel bwd_post_kernel_of(int d, int grad_dtype) {
    return by_io(grad_dtype, [&]<class GT>() {
        return d == 128 ? kernel_of<bwd_post_kernel<128, GT>>(0) : kernel_of<bwd_post_kernel<64, GT>>(0);
    });
}

}  // namespace fa
