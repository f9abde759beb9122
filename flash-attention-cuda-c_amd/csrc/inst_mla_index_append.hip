// inst_mla_index_append.hip -- the MLA index-cache append kernels: bf16 index keys (and queries) rotated, Hadamard-transformed and
// quantised to e4m3fn under one scale per row, into a contiguous or paged index cache (one translation unit of
// libflash_attention.so: see launchers.hip.h and mla_index_append.hip.h).
#include "mla_index_append.hip.h"

namespace fa {

Kernel mla_index_append_kernel_of(bool paged) {
    return by_bool(paged, [&]<bool PAGED>() { return kernel_of<mla_index_append_kernel<PAGED>>(0); });
}

}  // namespace fa
