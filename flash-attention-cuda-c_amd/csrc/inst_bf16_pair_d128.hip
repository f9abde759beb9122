// inst_bf16_pair_d128.hip -- bf16 inputs, D = 128, small problems, with or without the causal mask (at most one 256-row unit per TWO CUs): 128-row units, one per
// workgroup of four waves, ONE workgroup per CU (a d = 128 ring leaves no room for a second): the launch occupies twice the CUs
// (kernel_bf16.hip.h: fwd_mfma_pair_kernel; one translation unit of libflash_attention.so: see launchers.hip.h).
#include "kernel_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

// ONE configuration for both weight precisions: the four-wave form of the persistent kernels' mixed-precision kernel (KernelCfg::MIX) on their
// engine (32x32x16 under the mask, 16x16x32 without) -- K by LDS-DMA, V by LDS-DMA (bf16 weights) or as fp16 through registers (the blocks
// qb < Params::hp), exact fp32 row sums whether or not the call asks for the LSE.  (The register-staged 16x16x32 fp16-weights kernel in
// the fp16 blocks' place spills 31 VGPRs into its tile loop: 32 staging registers at four waves.)  It fills both configuration slots of
// fwd_mfma_pair_kernel.
template <bool CAUSAL, typename OutT>
using PairA = KernelCfg<128, CAUSAL, OutT, 2, Opt{.m16 = CAUSAL ? 0 : -1, .sum_mfma = 0, .waves = 4, .mix = true}>;

// launched with (Params, hp, jpx): p.nQ = 128-row query blocks per head, the first hp of them take fp16 weights
Kernel bf16_pair_d128_kernel(bool causal, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        return by_bool(causal, [&]<bool CAUSAL>() {
            using A = PairA<CAUSAL, OutT>;
            return kernel_of<fwd_mfma_pair_kernel<A, A>>(A::LDS_BYTES);
        });
    });
}

}  // namespace fa
