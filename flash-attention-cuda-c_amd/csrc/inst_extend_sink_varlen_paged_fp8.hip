// inst_extend_sink_varlen_paged_fp8.hip -- the paged fp8 (e4m3fn) cache form of RAGGED chunked prefill with attention sinks (flash_attention_sink_extend_paged_varlen under one split):
// the split-KV kernel with SINK = true and WINDOW = true -- windowSize = 0 runs it at window = 0 -- at D = 64 / 128 (one translation unit of
// libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h; built with the
// MFMAs in VGPR form: Makefile).  Under more than one split the call launches the
// SINK = false unit and the SINK combine.
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<true, true, true, true, true, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8, SINK

}  // namespace fa
