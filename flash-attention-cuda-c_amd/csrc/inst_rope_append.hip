// inst_rope_append.hip -- the K/V cache append kernels with the rotary embedding fused in: bf16 new K / V rows and Q rows, bf16 or
// e4m3fn caches, contiguous or paged, uniform, uniform with per-row position offsets or ragged, at D = 64 / 128 (one translation unit of libflash_attention.so: see
// launchers.hip.h and rope_append.hip.h).  The pair style and rotDim are runtime arguments of every instantiation.
#include "rope_append.hip.h"
#include "launchers.hip.h"

namespace fa {

// (the ragged, token-major form is VARLEN)
template <int D, bool VARLEN>
static Kernel rope_append_of(bool kv8, bool paged) {
    return by_bool(kv8, [&]<bool KV8>() {
        return by_bool(paged, [&]<bool PAGED>() {
            if constexpr (VARLEN) return kernel_of<rope_append_varlen_kernel<D, KV8, PAGED>>(0);
            else return kernel_of<rope_append_kernel<D, KV8, PAGED>>(0);
        });
    });
}

Kernel rope_append_kernel_of(int d, bool kv8, bool paged) {
    return d == 128 ? rope_append_of<128, false>(kv8, paged) : rope_append_of<64, false>(kv8, paged);
}

Kernel rope_append_pos_kernel_of(int d, bool kv8, bool paged) {
    return by_bool(kv8, [&]<bool KV8>() {
        return by_bool(paged, [&]<bool PAGED>() {
            return d == 128 ? kernel_of<rope_append_kernel<128, KV8, PAGED, true>>(0) : kernel_of<rope_append_kernel<64, KV8, PAGED, true>>(0);
        });
    });
}

Kernel rope_append_varlen_kernel_of(int d, bool kv8, bool paged) {
    return d == 128 ? rope_append_of<128, true>(kv8, paged) : rope_append_of<64, true>(kv8, paged);
}

}  // namespace fa
