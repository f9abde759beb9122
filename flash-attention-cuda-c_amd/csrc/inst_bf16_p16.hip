// inst_bf16_p16.hip -- bf16 inputs WITHOUT the causal mask, fp16 softmax weights on every row (FA_FLAG_F16_WEIGHTS, or seqLenK <
// FA_EARLY_KEYS), D = 128 / 64: the mixed-precision kernel of the 16x16x32 engine with Params::hp = all query blocks -- K by LDS-DMA, V
// as fp16 through registers (MixStage); +1.5 ... +2.4 % over both tiles through registers (profiles/r04_tune_g_*.log).  Under the
// mask the 32x32x16 mixed-precision kernel of inst_bf16_mix.hip serves these calls.
// (one translation unit of libflash_attention.so: see launchers.hip.h).
#include "kernel_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

// fp32 sum of the unrounded weights (the LSE is exact either way), every unit "early"
template <int D, typename OutT>
using F16Cfg = KernelCfg<D, false, OutT, 2, Opt{.sum_mfma = 0, .mix = true}>;

Kernel bf16_p16_kernel(int d, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        using C128 = F16Cfg<128, OutT>;
        using C64 = F16Cfg<64, OutT>;
        return d == 128 ? kernel_of<fwd_mfma_kernel<C128>>(C128::LDS_BYTES) : kernel_of<fwd_mfma_kernel<C64>>(C64::LDS_BYTES);
    });
}

}  // namespace fa
