// mla_append_packed.hip.h -- the WRITE side of the PACKED MLA latent cache (flash_attention_mla_append_packed, _paged_packed; DESIGN.md
// section 41): the last Sq tokens of every sequence, given as mla_append.hip.h's two bf16 tensors Cnew [B, Sq, 512] and Rnew [B, Sq, 64],
// become MlaPackedRow rows of 656 bytes -- 512 e4m3fn codes, one fp32 scale per block of 128 latent columns, the rotary columns as they
// are -- contiguous [B, capacity, 656] or a pool of pages behind a block table.
//
//   * POSITIONS and WORK are mla_append_kernel's: L = min(kv_lens[b], capacity) ALREADY counts the new rows, row i goes to p = L - Sq + i
//     iff p >= 0, L <= 0 writes nothing; a workgroup is (sequence, 64 positions) aligned in position space, a wave 16 positions aligned
//     to 16, hence ONE page; a wave without a position leaves before it reads its table entry; an entry outside [0, numPages) skips its
//     rows and is never clamped.
//   * A ROW's 512 latent columns are ONE wave instruction: lane l loads 16 bytes, the columns [8 l, 8 l + 8) of block l / 16.  Per block,
//     mla_index_append.hip.h's steps 5 .. 7 in plain fp32: amax = max(max |x|, 1e-4) over the sixteen lanes (idx_lane_xor: DPP and
//     ds_swizzle, no LDS memory), s0 = amax * fl32(1 / 448), s = s0 or (pow2) the least power of two >= s0, kv_quantise4 under the
//     descale s.  A lane stores its eight codes as one 8-byte store -- 512 contiguous bytes per row -- and lane 0 of the block the scale.
//     Whether a row is written is wave-uniform: a row that is not costs nothing, and EXEC is full at every exchange.
//   * The sixteen rows' ROPE parts are 128 chunks of 16 bytes, two per lane: chunk 64 n + l is chunk % 8 of row chunk / 8; bit copies.
//   * All loads of a wave's rows (16 + 2 per lane) are issued before its first store.  Every address is 64-bit arithmetic on the strides
//     (the cache's in BYTES).  No LDS, no scratch, no atomics; every byte has one writer; every store is a vector store.
#pragma once

#include "mla_append.hip.h"
#include "mla_decode.hip.h"
#include "mla_index_append.hip.h"

namespace fa {

// mla_append_kernel's parameters (descale unused; kvB, kvS in bytes) and the scale format
struct MlaAppendPackedParams : MlaAppendParams {
    int pow2;
};

template <bool PAGED>
__global__ __launch_bounds__(256) void mla_append_packed_kernel(const MlaAppendPackedParams p) {
#pragma clang fp contract(off)
    using W = KvAppendCfg;
    using R = MlaPackedRow;
    constexpr int NR = 2 * MlaCfg::DR / 16 * W::WROWS / 64;   // rope chunks per lane
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;

    // blockIdx -> (sequence, position block)
    const int rb = blockIdx.x % p.row_blocks;
    const int b = blockIdx.x / p.row_blocks;

    int len = p.cap;
    if (p.kv_lens) len = min(p.kv_lens[b], p.cap);
    len = __builtin_amdgcn_readfirstlane(len);
    if (len <= 0) return;                                  // an inactive slot: nothing is written
    const int first = max(len - p.Sq, 0);                  // the position of the first row written
    const int pw = ((first / W::BLOCK + rb) * W::WAVES + wave) * W::WROWS;   // this wave's 16 positions
    if (pw + W::WROWS <= first || pw >= len) return;       // (before the table entry is read)

    char* dst = (char*)p.KV;
    int row0 = pw;                                         // the wave's first row within its sequence or page
    if constexpr (PAGED) {
        const int entry = __builtin_amdgcn_readfirstlane(p.block_table[b * p.table_stride + (pw >> p.page_shift)]);
        if (entry < 0 || entry >= p.num_pages) return;     // not clamped: a clamped write would land in another sequence's page
        dst += (int64_t)entry * p.kvB;
        row0 = pw & ((1 << p.page_shift) - 1);
    } else {
        dst += (int64_t)b * p.kvB;
    }
    dst += (int64_t)row0 * p.kvS;
    const int shift = len - p.Sq;                          // position - shift = the new row's index (>= 0 from `first` on)
    const __bf16* csrc = p.Cnew + (int64_t)b * p.cB + 8 * lane;
    const __bf16* rsrc = p.Rnew + (int64_t)b * p.rB + 8 * (lane & 7);

    u32x4 x[W::WROWS], rp[NR];
#pragma unroll
    for (int j = 0; j < W::WROWS; ++j) {
        const int pos = pw + j;                            // (wave-uniform, and so is the branch)
        x[j] = u32x4{0u, 0u, 0u, 0u};
        if (pos >= first && pos < len) x[j] = *reinterpret_cast<const u32x4*>(csrc + (int64_t)(pos - shift) * p.cS);
    }
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        const int pos = pw + 8 * n + (lane >> 3);
        rp[n] = u32x4{0u, 0u, 0u, 0u};
        if (pos >= first && pos < len) rp[n] = *reinterpret_cast<const u32x4*>(rsrc + (int64_t)(pos - shift) * p.rS);
    }

    constexpr float C1 = (float)(1.0 / 448.0);
#pragma unroll
    for (int j = 0; j < W::WROWS; ++j) {
        const int pos = pw + j;
        if (pos < first || pos >= len) continue;
        float amax = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(bf16_lo(x[j][w])), __builtin_fabsf(bf16_hi(x[j][w]))));
        amax = __builtin_fmaxf(amax, idx_lane_xor<1>(amax));
        amax = __builtin_fmaxf(amax, idx_lane_xor<2>(amax));
        amax = __builtin_fmaxf(amax, idx_lane_xor<4>(amax));
        amax = __builtin_fmaxf(amax, idx_lane_xor<8>(amax));
        amax = __builtin_fmaxf(amax, 1e-4f);
        float sc = amax * C1;                              // a normal number
        if (p.pow2) {                                      // 2^ceil(log2 s0): the exponent, one more when the mantissa is not zero
            const uint32_t u = __float_as_uint(sc);
            sc = __uint_as_float(((u >> 23) + ((u & 0x7FFFFFu) != 0u)) << 23);
        }
        u32x2 y;
        y[0] = kv_quantise4(x[j][0], x[j][1], sc);
        y[1] = kv_quantise4(x[j][2], x[j][3], sc);
        char* row = dst + (int64_t)j * p.kvS;
        *reinterpret_cast<u32x2*>(row + R::CODES + 8 * lane) = y;
        if ((lane & 15) == 0) *reinterpret_cast<float*>(row + R::SCALES + 4 * (lane >> 4)) = sc;
    }
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        const int r = 8 * n + (lane >> 3), pos = pw + r;
        if (pos >= first && pos < len) *reinterpret_cast<u32x4*>(dst + (int64_t)r * p.kvS + R::ROPE + 16 * (lane & 7)) = rp[n];
    }
}

// the instantiation for (paged): inst_mla_append_packed.hip
Kernel mla_append_packed_kernel_of(bool paged);

}  // namespace fa
