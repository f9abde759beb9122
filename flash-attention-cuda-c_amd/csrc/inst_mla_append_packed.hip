// inst_mla_append_packed.hip -- the packed MLA latent-cache append kernels: bf16 latent and rotary rows into 656-byte rows of e4m3fn codes,
// per-128-column fp32 scales and bf16 rotary columns, contiguous or paged (one translation unit of libflash_attention.so: see
// launchers.hip.h and mla_append_packed.hip.h).  Built without packed fp32 arithmetic (the Makefile's flag): its scales are pinned to the bit.
#include "mla_append_packed.hip.h"

namespace fa {

Kernel mla_append_packed_kernel_of(bool paged) {
    return by_bool(paged, [&]<bool PAGED>() { return kernel_of<mla_append_packed_kernel<PAGED>>(0); });
}

}  // namespace fa
