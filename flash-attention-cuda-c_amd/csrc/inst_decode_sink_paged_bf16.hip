// inst_decode_sink_paged_bf16.hip -- the paged bf16 cache form of split-KV decode with attention sinks (flash_attention_sink_decode_paged under one split):
// the split-KV kernel with SINK = true and WINDOW = true -- windowSize = 0 runs it at window = 0 -- at D = 64 / 128 (one translation unit of
// libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h).  Under more than one split the call launches the
// SINK = false unit and the SINK combine.
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<false, false, true, true, false, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8, SINK

}  // namespace fa
