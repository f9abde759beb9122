// inst_bf16_pair_d64.hip -- bf16 inputs, D = 64, small problems, with or without the causal mask (at most one 256-row unit per CU): 128-row units, one per
// workgroup of four waves, two workgroups per CU paired heaviest + lightest (kernel_bf16.hip.h: fwd_mfma_pair_kernel; one translation
// unit of libflash_attention.so: see launchers.hip.h).  D = 128 (one workgroup per CU): inst_bf16_pair_d128.hip.
#include <algorithm>

#include "kernel_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

// bf16 weights: the engine of the persistent kernels (32x32x16 under the mask, 16x16x32 without; LDS-DMA staging).  Without the mask the row
// sums are the exact fp32 ones (the persistent kernels' LSE instantiation) whether or not the call asks for the LSE: one instantiation
template <bool CAUSAL, typename OutT>
using PairA = KernelCfg<64, CAUSAL, OutT, 2, Opt{.m16 = CAUSAL ? 0 : -1, .sum_mfma = 0, .waves = 4}>;
template <bool CAUSAL, typename OutT>
using PairB = KernelCfg<64, CAUSAL, OutT, 2, Opt{.sum_mfma = 0, .waves = 4, .p_f16 = true}>;      // fp16 weights

template <bool CAUSAL, typename OutT>
constexpr int pair_lds = std::max(PairA<CAUSAL, OutT>::LDS_BYTES, PairB<CAUSAL, OutT>::LDS_BYTES);
static_assert(pair_lds<true, float> <= 80 * 1024 - 256 && pair_lds<true, __bf16> <= 80 * 1024 - 256, "two workgroups per CU");

// launched with (Params, hp, jpx): p.nQ = 128-row query blocks per head, the first hp of them take fp16 weights
Kernel bf16_pair_d64_kernel(bool causal, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        return by_bool(causal, [&]<bool CAUSAL>() {
            return kernel_of<fwd_mfma_pair_kernel<PairA<CAUSAL, OutT>, PairB<CAUSAL, OutT>>>(pair_lds<CAUSAL, OutT>);
        });
    });
}

}  // namespace fa
