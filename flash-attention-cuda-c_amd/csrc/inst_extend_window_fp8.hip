// inst_extend_window_fp8.hip -- the contiguous fp8 (e4m3fn) cache form of chunked prefill with a sliding window
// (flash_attention_extend_window with windowSize > 0): the split-KV kernel with ExtendCfg::RT 16-row tiles per wave and WINDOW = true, at
// D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h; built with the MFMAs in VGPR
// form: Makefile).  windowSize = 0 is served by the un-windowed unit; the combine kernel is the un-windowed family's.
#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel extend_window_fp8_split_kernel_of(int d) {
    return d == 128 ? kernel_of<split_kv_kernel<128, ExtendCfg<128>::RT, false, true, true, false>>(DecodeCfg<128, 1>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, ExtendCfg<64>::RT, false, true, true, false>>(DecodeCfg<64, 1>::LDS_BYTES);
}

}  // namespace fa
