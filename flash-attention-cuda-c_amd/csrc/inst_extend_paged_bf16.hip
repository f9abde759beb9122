// inst_extend_paged_bf16.hip -- the paged bf16 cache form of the chunked-prefill kernel against the decode caches at D = 64 / 128 (one translation
// unit of libflash_attention.so: see launchers.hip.h and extend_bf16.hip.h).  The combine kernel is decode's (inst_decode_bf16.hip).
#include "extend_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel extend_paged_split_kernel_of(int d) {
    return d == 128 ? kernel_of<extend_split_kernel<128, ExtendCfg<128>::RT, true, false>>(DecodeCfg<128, 2>::LDS_BYTES)
                    : kernel_of<extend_split_kernel<64, ExtendCfg<64>::RT, true, false>>(DecodeCfg<64, 2>::LDS_BYTES);
}

}  // namespace fa
