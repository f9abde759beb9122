// split_kv_inst.hip.h -- the one selector of the split-KV kernel's instantiations (decode_bf16.hip.h: split_kernel_of), for the
// inst_decode_*.hip and inst_extend_*.hip units only: each includes this and instantiates the selector of its call family and cache form
// explicitly, so that the kernels of one unit are compiled by that unit (in parallel with the others, under its own flags: Makefile).
#pragma once

#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

// EXTEND: chunked prefill, ExtendCfg::RT 16-row tiles per wave (decode: one); the LDS size is that of the cache's element size
template <bool EXTEND, bool VARLEN, bool WINDOW, bool PAGED, bool KV8, bool SINK, bool TREE>
Kernel split_kernel_of(int d) {
    constexpr int ES = KV8 ? 1 : 2;
    return d == 128 ? kernel_of<split_kv_kernel<128, EXTEND ? ExtendCfg<128>::RT : 1, PAGED, KV8, WINDOW, VARLEN, SINK, TREE>>(DecodeCfg<128, ES>::LDS_BYTES)
                    : kernel_of<split_kv_kernel<64, EXTEND ? ExtendCfg<64>::RT : 1, PAGED, KV8, WINDOW, VARLEN, SINK, TREE>>(DecodeCfg<64, ES>::LDS_BYTES);
}

}  // namespace fa
