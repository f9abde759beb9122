// inst_kv_accept.hip -- the in-cache acceptance kernels of a speculative step: bf16 or e4m3fn caches, contiguous or paged, at
// D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and kv_accept.hip.h).
#include "kv_accept.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel kv_accept_kernel_of(int d, bool kv8, bool paged) {
    return by_bool(kv8, [&]<bool KV8>() {
        return by_bool(paged, [&]<bool PAGED>() {
            return d == 128 ? kernel_of<kv_accept_kernel<128, KV8, PAGED>>(0) : kernel_of<kv_accept_kernel<64, KV8, PAGED>>(0);
        });
    });
}

}  // namespace fa
