// inst_decode_paged_bf16.hip -- the paged form of the split-KV decode kernel (K/V pools of fixed-size pages behind a block table),
// bf16 Q/K/V at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h).  The
// combine kernel is the contiguous path's (inst_decode_bf16.hip).
#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel decode_paged_split_kernel_of(int d) {
    return d == 128 ? kernel_of<split_kv_kernel<128, 1, true, false, true>>(DecodeCfg<128, 2>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, 1, true, false, true>>(DecodeCfg<64, 2>::LDS_BYTES);
}

}  // namespace fa
