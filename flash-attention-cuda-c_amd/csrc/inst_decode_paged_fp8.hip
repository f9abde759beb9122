// inst_decode_paged_fp8.hip -- the paged fp8 K/V form of the split-KV decode kernel (bf16 Q against e4m3fn K/V pools of fixed-size
// pages behind a block table, per-head descales) at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h
// and decode_bf16.hip.h).  The combine kernel is the bf16 path's (inst_decode_bf16.hip).
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<false, false, true, true, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8

}  // namespace fa
