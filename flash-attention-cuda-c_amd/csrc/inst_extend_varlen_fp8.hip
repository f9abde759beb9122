// inst_extend_varlen_fp8.hip -- the contiguous fp8 (e4m3fn) cache form of RAGGED chunked prefill (flash_attention_extend_varlen): the
// split-KV kernel with ExtendCfg::RT 16-row tiles per wave, no window and a per-sequence row count, at D = 64 / 128 (one translation
// unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h; built with the MFMAs in VGPR form: Makefile).  The combine
// kernel is inst_extend_varlen_bf16.hip's.
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<true, true, false, false, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8

}  // namespace fa
