// inst_mla_append.hip -- the MLA latent-cache append kernels: bf16 latent and rotary rows into one 576-wide bf16 (bit copy) or e4m3fn
// (quantised) cache, contiguous or paged (one translation unit of libflash_attention.so: see launchers.hip.h and mla_append.hip.h).
#include "mla_append.hip.h"

namespace fa {

Kernel mla_append_kernel_of(bool kv8, bool paged) {
    return by_bool(kv8, [&]<bool KV8>() {
        return by_bool(paged, [&]<bool PAGED>() { return kernel_of<mla_append_kernel<KV8, PAGED>>(0); });
    });
}

}  // namespace fa
