// inst_kv_append.hip -- the K/V cache append kernels: bf16 new rows into bf16 (bit copy) or e4m3fn (quantised) caches, contiguous or
// paged, at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and kv_append.hip.h).
#include "kv_append.hip.h"
#include "launchers.hip.h"

namespace fa {

// (the ragged, token-major form is VARLEN)
template <int D, bool VARLEN>
static Kernel kv_append_of(bool kv8, bool paged) {
    return by_bool(kv8, [&]<bool KV8>() {
        return by_bool(paged, [&]<bool PAGED>() {
            if constexpr (VARLEN) return kernel_of<kv_append_varlen_kernel<D, KV8, PAGED>>(0);
            else return kernel_of<kv_append_kernel<D, KV8, PAGED>>(0);
        });
    });
}

Kernel kv_append_kernel_of(int d, bool kv8, bool paged) {
    return d == 128 ? kv_append_of<128, false>(kv8, paged) : kv_append_of<64, false>(kv8, paged);
}

Kernel kv_append_varlen_kernel_of(int d, bool kv8, bool paged) {
    return d == 128 ? kv_append_of<128, true>(kv8, paged) : kv_append_of<64, true>(kv8, paged);
}

}  // namespace fa
