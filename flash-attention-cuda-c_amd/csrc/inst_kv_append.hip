// inst_kv_append.hip -- the K/V cache append kernels: bf16 new rows into bf16 (bit copy) or e4m3fn (quantised) caches, contiguous or
// paged, at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and kv_append.hip.h).
#include "kv_append.hip.h"
#include "launchers.hip.h"

namespace fa {

template <int D>
static Kernel kv_append_of(bool kv8, bool paged) {
    if (kv8) return paged ? kernel_of<kv_append_kernel<D, true, true>>(0) : kernel_of<kv_append_kernel<D, true, false>>(0);
    return paged ? kernel_of<kv_append_kernel<D, false, true>>(0) : kernel_of<kv_append_kernel<D, false, false>>(0);
}

Kernel kv_append_kernel_of(int d, bool kv8, bool paged) { return d == 128 ? kv_append_of<128>(kv8, paged) : kv_append_of<64>(kv8, paged); }

// the ragged (token-major) append
template <int D>
static Kernel kv_append_varlen_of(bool kv8, bool paged) {
    if (kv8) return paged ? kernel_of<kv_append_varlen_kernel<D, true, true>>(0) : kernel_of<kv_append_varlen_kernel<D, true, false>>(0);
    return paged ? kernel_of<kv_append_varlen_kernel<D, false, true>>(0) : kernel_of<kv_append_varlen_kernel<D, false, false>>(0);
}

Kernel kv_append_varlen_kernel_of(int d, bool kv8, bool paged) {
    return d == 128 ? kv_append_varlen_of<128>(kv8, paged) : kv_append_varlen_of<64>(kv8, paged);
}

}  // namespace fa
