// inst_decode_tree_fp8.hip -- the contiguous fp8 (e4m3fn) cache form of tree-masked verification (flash_attention_tree), split-KV decode form (1 .. FA_DECODE_MAX_Q draft nodes):
// the split-KV kernel with TREE = true, SINK = true and WINDOW = true at D = 64 / 128 (one translation unit of libflash_attention.so: see
// launchers.hip.h and decode_bf16.hip.h).  Launched under any split count: under more than
// one the slabs hold the keys alone and the call's combine is the existing one, sink or not.
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<false, false, true, false, true, true, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8, SINK, TREE

}  // namespace fa
