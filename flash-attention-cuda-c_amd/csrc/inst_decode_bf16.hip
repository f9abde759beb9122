// inst_decode_bf16.hip -- the split-KV decode kernels, bf16 Q/K/V at D = 64 / 128 (one translation unit of libflash_attention.so: see
// launchers.hip.h and decode_bf16.hip.h).
#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel decode_split_kernel_of(int d) {
    return d == 128 ? kernel_of<split_kv_kernel<128, 1, false, false, true>>(DecodeCfg<128, 2>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, 1, false, false, true>>(DecodeCfg<64, 2>::LDS_BYTES);
}

Kernel decode_combine_kernel_of(int d) {
    return d == 128 ? kernel_of<decode_combine_kernel<128>>(0) : kernel_of<decode_combine_kernel<64>>(0);
}

}  // namespace fa
