// launchers.hip.h -- how the host side names and starts a kernel instantiation, and the per-group selectors that the translation
// units inst_*.hip define.  The kernels are spread over several translation units only so that they compile in parallel (one hipcc
// process per group); FlashAttention.hip holds the C ABI, validation and the routing decision, and calls the selectors below.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/flash_attention.h"
#include "loaders.hip.h"

namespace fa {

// One kernel instantiation as the host sees it.  The MFMA kernels need up to 96 KiB of dynamic LDS: above the 64 KiB default, so
// launch() raises the limit once per (instantiation, device) -- function attributes are per device, and the multi-GPU driver calls
// in from one host thread per device.
struct Kernel {
    const void* fn;              // the __global__ function
    int lds_bytes;               // its dynamic LDS (Cfg::LDS_BYTES); the generic and weights kernels: the most any head dimension takes
    std::atomic<bool>* raised;   // [64]: the LDS limit has been raised on device i
};

template <auto fn>
Kernel kernel_of(int lds_bytes) {
    static std::atomic<bool> raised[64];
    return {(const void*)fn, lds_bytes, raised};
}

// The instantiation for a runtime output type: f.template operator()<OutT>() for O in fp32, bf16 or (any other o_dtype) fp16
template <class F>
Kernel by_out(int o_dtype, F f) {
    if (o_dtype == FA_DTYPE_F32) return f.template operator()<float>();
    if (o_dtype == FA_DTYPE_BF16) return f.template operator()<__bf16>();
    return f.template operator()<_Float16>();
}

// ... and for a runtime flag
template <class F>
Kernel by_bool(bool b, F f) {
    return b ? f.template operator()<true>() : f.template operator()<false>();
}

// Launch k with lds_bytes of dynamic LDS (<= k.lds_bytes); args are the kernel's parameters, in their exact types.  (Raising the
// limit is not a stream operation; a repeated raise is harmless.)
template <class... Args>
hipError_t launch(const Kernel& k, unsigned grid, int threads, int lds_bytes, hipStream_t st, Args... args) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool known = dev >= 0 && dev < 64;
    if (!(known && k.raised[dev].load(std::memory_order_acquire))) {
        e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes);
        if (e != hipSuccess) return e;
        if (known) k.raised[dev].store(true, std::memory_order_release);
    }
    void* argv[] = {&args...};
    (void)hipLaunchKernel(k.fn, dim3(grid), dim3(threads), argv, lds_bytes, st);
    return hipGetLastError();
}

// ---- group selectors (each defined in exactly one inst_*.hip) ----
// (the append and backward selectors are declared beside their kernels: kv_append.hip.h, bwd_bf16.hip.h; the split-KV kernel's forms and
// its combine have launchers in place of selectors -- split_forms.hip.h: one table of the forms, one unit per row built from split_unit.hip)
// Kernels taking (Params):
// bf16 inputs, persistent kernel instantiated at D = 128 / 64; pad: the tensors' head dimension is smaller than D; lse: the call
// wants the LSE (without the mask that selects the instantiation that keeps the fp32 sum of the unrounded weights: computers16.hip.h)
Kernel bf16_d128_kernel(bool causal, bool pad, bool lse, int o_dtype);
Kernel bf16_d64_kernel(bool causal, bool pad, bool lse, int o_dtype);
// fp8 e4m3fn inputs (always the D = 128 instantiation)
Kernel fp8_d128_kernel(bool causal, bool pad, int o_dtype);
// bf16 inputs, causal, d = 128 or 64 exactly: one kernel, one (head, query block) list; the units of the first Params::hp query
// blocks of every head run with fp16 weights, the rest with bf16 weights (inst_bf16_mix.hip)
Kernel bf16_causal_mix_kernel(int d, int o_dtype);
// bf16 inputs without the mask, fp16 weights on every row (d = 128 or 64 exactly)
Kernel bf16_p16_kernel(int d, int o_dtype);
// fp32 inputs, exact-fp32 MFMA kernel at D = 128 / 64
Kernel f32_d128_kernel(bool causal, bool pad, int o_dtype);
Kernel f32_d64_kernel(bool causal, bool pad, int o_dtype);
// Kernels taking (Params, hp, jpx): small problems, 128-row units, one per workgroup of four waves -- causal at D = 64: two
// workgroups per CU, paired; else one per CU (inst_bf16_pair_d64.hip, inst_bf16_pair_d128.hip)
Kernel bf16_pair_d64_kernel(bool causal, int o_dtype);
Kernel bf16_pair_d128_kernel(bool causal, int o_dtype);

}  // namespace fa
