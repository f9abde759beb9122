// inst_extend_paged_fp8.hip -- the paged fp8 (e4m3fn) cache form of chunked prefill against the decode caches: the split-KV kernel with
// ExtendCfg::RT 16-row tiles per wave and no window, at D = 64 / 128 (one translation unit of libflash_attention.so: see launchers.hip.h and
// decode_bf16.hip.h; built with the MFMAs in VGPR form: Makefile).  The combine kernel is decode's (inst_decode_bf16.hip).
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<true, false, false, true, true>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8

}  // namespace fa
