// inst_extend_paged_bf16.hip -- the paged bf16 cache form of chunked prefill against the decode caches: the split-KV kernel with
// ExtendCfg::RT 16-row tiles per wave and no window, at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and
// decode_bf16.hip.h; built with the MFMAs in VGPR form: Makefile).  The combine kernel is decode's (inst_decode_bf16.hip).
#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel extend_paged_split_kernel_of(int d) {
    return d == 128 ? kernel_of<split_kv_kernel<128, ExtendCfg<128>::RT, true, false, false>>(DecodeCfg<128, 2>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, ExtendCfg<64>::RT, true, false, false>>(DecodeCfg<64, 2>::LDS_BYTES);
}

}  // namespace fa
