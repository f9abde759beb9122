// inst_extend_varlen_paged_bf16.hip -- the paged bf16 cache form of RAGGED chunked prefill (flash_attention_extend_paged_varlen): the
// split-KV kernel with ExtendCfg::RT 16-row tiles per wave, no window and a per-sequence row count, at D = 64 / 128 (one translation
// unit of libflash_attention.so: see launchers.hip.h and decode_bf16.hip.h; built with the MFMAs in VGPR form: Makefile).  The combine
// kernel is inst_extend_varlen_bf16.hip's.
#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

Kernel extend_varlen_paged_split_kernel_of(int d) {
    return d == 128 ? kernel_of<split_kv_kernel<128, ExtendCfg<128>::RT, true, false, false, true>>(DecodeCfg<128, 2>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, ExtendCfg<64>::RT, true, false, false, true>>(DecodeCfg<64, 2>::LDS_BYTES);
}

}  // namespace fa
