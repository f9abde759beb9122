// inst_decode_bf16.hip -- the split-KV decode kernels, bf16 Q/K/V at D = 64 / 128 (one translation unit of libflash_attention.so: see
// launchers.hip.h and decode_bf16.hip.h).
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<false, false, true, false, false>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8

Kernel decode_combine_kernel_of(int d) {
    return d == 128 ? kernel_of<decode_combine_kernel<128>>(0) : kernel_of<decode_combine_kernel<64>>(0);
}

}  // namespace fa
