// inst_extend_varlen_bf16.hip -- the contiguous bf16 cache form of RAGGED chunked prefill (flash_attention_extend_varlen): the split-KV
// kernel with ExtendCfg::RT 16-row tiles per wave, no window and a per-sequence row count, at D = 64 / 128, and the combine kernel that
// skips the rows no sequence owns (one translation unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h; built with
// the MFMAs in VGPR form: Makefile).
#include "split_kv_inst.hip.h"

namespace fa {

template Kernel split_kernel_of<true, true, false, false, false>(int);   // EXTEND, VARLEN, WINDOW, PAGED, KV8

Kernel extend_varlen_combine_kernel_of(int d) {
    return d == 128 ? kernel_of<decode_combine_kernel<128, true>>(0) : kernel_of<decode_combine_kernel<64, true>>(0);
}

}  // namespace fa
