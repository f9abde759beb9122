// mla_append.hip.h -- the WRITE side of the MLA latent cache (flash_attention_mla_append, flash_attention_mla_append_paged; DESIGN.md
// section 37): the last Sq tokens of every sequence, given as TWO bf16 tensors -- the compressed latent Cnew [B, Sq, 512] and the key's
// rotary part Rnew [B, Sq, 64], already rotated -- become rows of the 576-wide cache that mla_decode.hip.h reads: columns [0, 512) and
// [512, 576) of row p, contiguous [B, capacity, 576] or a pool of pages behind a block table; bf16 (a bit copy) or OCP e4m3fn under ONE
// fp32 descale (kv_append.hip.h's kv_store8: divide, saturate, round to nearest even once, a NaN quotient becomes a NaN code).
//
//   * POSITIONS are kv_append_kernel's: L = min(kv_lens[b], capacity) ALREADY counts the new rows; new row i is key position
//     p = L - Sq + i, written when p >= 0; L <= 0 writes nothing.  Lengths, the descale and table entries are read here, never by the host.
//   * WORK.  A workgroup is (sequence, block of 64 key POSITIONS), aligned in position space: block rb covers positions
//     [64 (first / 64 + rb), + 64) cut to [first, L), first = max(L - Sq, 0), so ceil(Sq / 64) + 1 blocks reach every row.  Each of the
//     four waves owns 16 consecutive positions aligned to 16, hence ONE page: the length, the descale and the page entry are
//     wave-uniform scalars, read once.  A wave that holds no position of [first, L) returns before it reads its table entry.
//   * A ROW is 72 chunks of 8 elements, which no power-of-two group of lanes holds (kv_append_kernel maps D / 8 lanes to a row): a wave's
//     16 rows are 16 x 72 = 1152 chunks, 18 per lane, and chunk idx = 64 n + lane is chunk idx % 72 of row idx / 72 -- the lane map of
//     the decode kernel's fetch.  Chunks below 64 come from Cnew, the others from Rnew: one 16-byte load each, all 18 issued before the
//     first store.  The stores of one wave instruction are 64 consecutive chunks: contiguous runs of whole rows.
//   * A table entry outside [0, numPages) is NOT clamped: the wave skips its rows.
//   * Every address is 64-bit arithmetic on the element strides.  No LDS, no scratch, no atomics; every store is a vector store.
#pragma once

#include "kv_append.hip.h"

namespace fa {

struct MlaAppendParams {
    const __bf16* Cnew;           // [B, Sq, 512]
    const __bf16* Rnew;           // [B, Sq, 64]
    void* KV;                     // the cache, or (paged) the pool
    const int32_t* kv_lens;       // optional [B] (device memory); NULL = the capacity
    const int32_t* block_table;   // paged: [B][table_stride] page numbers (device memory)
    const float* descale;         // fp8: optional, ONE fp32 (device memory); NULL = 1
    int64_t cB, cS, rB, rS;       // element strides of the new rows (bf16)
    int64_t kvB, kvS;             // element strides of the cache (paged: kvB the page stride); fp8: bytes
    int64_t table_stride;
    int Sq, cap;                  // cap: the capacity (paged: max_pages * page size)
    int row_blocks;               // position blocks per sequence: ceil(Sq / 64) + 1
    int num_pages, page_shift;    // paged: page size = 1 << page_shift, >= 16
};

struct MlaAppendCfg {
    static constexpr int DL = 512, DR = 64;
    static constexpr int CPR = (DL + DR) / 8;                     // 8-element chunks per row
    static constexpr int CL = DL / 8;                             // ... of which the first come from Cnew
    static constexpr int NCH = KvAppendCfg::WROWS * CPR / 64;     // chunks per lane
    static_assert(KvAppendCfg::WROWS * CPR % 64 == 0, "a wave's rows are whole wave instructions");
};

template <bool KV8, bool PAGED>
__global__ __launch_bounds__(256) void mla_append_kernel(const MlaAppendParams p) {
    using W = KvAppendCfg;
    using C = MlaAppendCfg;
    constexpr int ES = KV8 ? 1 : 2;      // bytes per cache element
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;

    // blockIdx -> (sequence, position block)
    const int rb = blockIdx.x % p.row_blocks;
    const int b = blockIdx.x / p.row_blocks;

    int len = p.cap;
    if (p.kv_lens) len = min(p.kv_lens[b], p.cap);
    len = __builtin_amdgcn_readfirstlane(len);
    if (len <= 0) return;                                  // an inactive slot: nothing is written
    const int first = max(len - p.Sq, 0);                  // the position of the first row written
    // this wave's 16 positions
    const int pw = ((first / W::BLOCK + rb) * W::WAVES + wave) * W::WROWS;
    if (pw + W::WROWS <= first || pw >= len) return;       // (before the table entry is read)

    char* dst = (char*)p.KV;
    int row0 = pw;                                         // the wave's first row within its sequence or page
    if constexpr (PAGED) {
        const int entry = __builtin_amdgcn_readfirstlane(p.block_table[b * p.table_stride + (pw >> p.page_shift)]);
        if (entry < 0 || entry >= p.num_pages) return;     // not clamped: a clamped write would land in another sequence's page
        dst += (int64_t)entry * p.kvB * ES;
        row0 = pw & ((1 << p.page_shift) - 1);
    } else {
        dst += (int64_t)b * p.kvB * ES;
    }
    const __bf16* csrc = p.Cnew + (int64_t)b * p.cB;
    const __bf16* rsrc = p.Rnew + (int64_t)b * p.rB;

    float ds = 1.f;
    if constexpr (KV8) {
        if (p.descale) ds = p.descale[0];
    }

    const int shift = len - p.Sq;                          // position - shift = the new row's index (>= 0 from `first` on)
    u32x4 x[C::NCH];
    bool ok[C::NCH];
#pragma unroll
    for (int n = 0; n < C::NCH; ++n) {
        const int idx = 64 * n + lane;
        const int row = idx / C::CPR, ch = idx - row * C::CPR;
        const int pos = pw + row;
        ok[n] = pos >= first && pos < len;
        x[n] = u32x4{0u, 0u, 0u, 0u};
        if (ok[n]) {
            const __bf16* src = ch < C::CL ? csrc + (int64_t)(pos - shift) * p.cS + ch * 8
                                           : rsrc + (int64_t)(pos - shift) * p.rS + (ch - C::CL) * 8;
            x[n] = *reinterpret_cast<const u32x4*>(src);
        }
    }
#pragma unroll
    for (int n = 0; n < C::NCH; ++n) {
        if (!ok[n]) continue;
        const int idx = 64 * n + lane;
        const int row = idx / C::CPR, ch = idx - row * C::CPR;
        kv_store8<KV8>(dst + ((int64_t)(row0 + row) * p.kvS + ch * 8) * ES, x[n], ds);
    }
}

// the instantiation for (fp8 cache, paged): inst_mla_append.hip
Kernel mla_append_kernel_of(bool kv8, bool paged);

}  // namespace fa
