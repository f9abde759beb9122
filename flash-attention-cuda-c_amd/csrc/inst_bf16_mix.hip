// inst_bf16_mix.hip -- bf16 inputs under the causal mask at the library's default precision, D = 128 / 64: the bf16-weights kernel whose
// units of the first Params::hp query blocks of every head (the rows that see fewer than FA_EARLY_KEYS keys) run with fp16 softmax
// weights -- one walk over one (head, query block) list, every unit in the precision of its block (kernel_bf16.hip.h: KernelCfg::MIX,
// MixCfg; one translation unit of libflash_attention.so: see launchers.hip.h).
#include "kernel_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel bf16_causal_mix_kernel(int d, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        using C128 = MixCfg<128, OutT>;
        using C64 = MixCfg<64, OutT>;
        return d == 128 ? kernel_of<fwd_mfma_kernel<C128>>(C128::LDS_BYTES) : kernel_of<fwd_mfma_kernel<C64>>(C64::LDS_BYTES);
    });
}

}  // namespace fa
