// inst_decode_paged_bf16.hip -- the paged form of the split-KV decode kernel (K/V pools of fixed-size pages behind a block table),
// bf16 Q/K/V at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h).  The
// combine kernel is the contiguous path's (inst_decode_bf16.hip).
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<false, false, true, true, false>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8

}  // namespace fa
