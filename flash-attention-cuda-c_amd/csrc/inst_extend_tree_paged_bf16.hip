// inst_extend_tree_paged_bf16.hip -- the paged bf16 cache form of tree-masked verification (flash_attention_tree_paged), chunked-prefill form (17 .. FA_TREE_MAX_Q draft nodes):
// the split-KV kernel with TREE = true, SINK = true and WINDOW = true at D = 64 / 128 (one translation unit of libflash_attention.so: see
// launchers.hip.h and decode_bf16.hip.h; built with the MFMAs in VGPR form: Makefile).  Launched under any split count: under more than
// one the slabs hold the keys alone and the call's combine is the existing one, sink or not.
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<true, false, true, true, false, true, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8, SINK, TREE

}  // namespace fa
