// inst_rope_append.hip -- the K/V cache append kernels with the rotary embedding fused in: bf16 new K / V rows and Q rows, bf16 or
// e4m3fn caches, contiguous or paged, uniform or ragged, at D = 64 / 128 (one translation unit of libflash_attention.so: see
// launchers.hip.h and rope_append.hip.h).  The pair style and rotDim are runtime arguments of every instantiation.
#include "rope_append.hip.h"
#include "launchers.hip.h"

namespace fa {

template <int D>
static Kernel rope_append_of(bool kv8, bool paged) {
    if (kv8) return paged ? kernel_of<rope_append_kernel<D, true, true>>(0) : kernel_of<rope_append_kernel<D, true, false>>(0);
    return paged ? kernel_of<rope_append_kernel<D, false, true>>(0) : kernel_of<rope_append_kernel<D, false, false>>(0);
}

Kernel rope_append_kernel_of(int d, bool kv8, bool paged) { return d == 128 ? rope_append_of<128>(kv8, paged) : rope_append_of<64>(kv8, paged); }

// the ragged (token-major) form
template <int D>
static Kernel rope_append_varlen_of(bool kv8, bool paged) {
    if (kv8) return paged ? kernel_of<rope_append_varlen_kernel<D, true, true>>(0) : kernel_of<rope_append_varlen_kernel<D, true, false>>(0);
    return paged ? kernel_of<rope_append_varlen_kernel<D, false, true>>(0) : kernel_of<rope_append_varlen_kernel<D, false, false>>(0);
}

Kernel rope_append_varlen_kernel_of(int d, bool kv8, bool paged) {
    return d == 128 ? rope_append_varlen_of<128>(kv8, paged) : rope_append_varlen_of<64>(kv8, paged);
}

}  // namespace fa
