// inst_decode_fp8.hip -- the fp8 K/V form of the split-KV decode kernel (bf16 Q against e4m3fn K/V caches with per-head descales) at
// D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h).  The combine kernel is
// the bf16 path's (inst_decode_bf16.hip).
#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel decode_fp8_split_kernel_of(int d) {
    return d == 128 ? kernel_of<split_kv_kernel<128, 1, false, true, true>>(DecodeCfg<128, 1>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, 1, false, true, true>>(DecodeCfg<64, 1>::LDS_BYTES);
}

}  // namespace fa
