// inst_extend_window_varlen_paged_fp8.hip -- the paged fp8 (e4m3fn) cache form of RAGGED chunked prefill with a sliding window
// (flash_attention_extend_paged_varlen_window with windowSize > 0): the split-KV kernel with ExtendCfg::RT 16-row tiles per wave and
// WINDOW = true, at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h; built with the
// MFMAs in VGPR form: Makefile).  windowSize = 0 is served by the un-windowed unit; the combine kernel is the un-windowed family's.
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<true, true, true, true, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8

}  // namespace fa
