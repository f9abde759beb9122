// inst_extend_fp8.hip -- the contiguous fp8 (e4m3fn) cache form of the chunked-prefill kernel against the decode caches at D = 64 / 128 (one translation
// unit of libflash_attention.so: see launchers.hip.h and extend_bf16.hip.h).  The combine kernel is decode's (inst_decode_bf16.hip).
#include "extend_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel extend_fp8_split_kernel_of(int d) {
    return d == 128 ? kernel_of<extend_split_kernel<128, ExtendCfg<128>::RT, false, true>>(DecodeCfg<128, 1>::LDS_BYTES)
                    : kernel_of<extend_split_kernel<64, ExtendCfg<64>::RT, false, true>>(DecodeCfg<64, 1>::LDS_BYTES);
}

}  // namespace fa
