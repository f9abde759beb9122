// mla_index_append.hip.h -- the WRITE side of the MLA index cache (flash_attention_mla_index_append, _paged): one
// launch takes the step's raw bf16 index projections and makes what mla_index.hip.h reads -- the new key rows Knew [B, Sq, 128] become
// e4m3fn rows of the index cache Kidx and one fp32 scale each in kScale (contiguous or paged), and (optionally) the step's index queries
// Qraw [B, Sq, 64, 128] become the dense e4m3fn Qidx, their scales folded into the head weights: W = (Wraw * qscale) * wScale.
//
//   * A ROW is 128 bf16: rotary embedding (optional; rope_append.hip.h's rope_pair, rounded once to bf16), a 128-point Walsh-Hadamard
//     transform in fp32 (Sylvester order, seven stages of strides 1 .. 64, every butterfly one add and one subtract), the product with
//     fl32(2^-3.5) rounded to bf16, amax = max(max |r|, 1e-4), s0 = amax * fl32(1 / 448), the scale s = s0 or (pow2) s0 rounded UP to a
//     power of two, and kv_append.hip.h's kv_quantise4 on the bf16 row under the descale s.  Pinned to the bit (include/flash_attention.h).
//   * LANES.  16 lanes hold a row, lane g its columns [8 g, 8 g + 8): one 16-byte load, so a wave instruction holds four rows and a
//     lane four rows of its wave's sixteen.  Element index = 8 g + e: stages 1, 2, 4 of the transform run over a lane's registers; stages
//     8, 16, 32, 64 exchange with lane g ^ 1, 2, 4, 8 -- DPP quad_perm, quad_perm, ds_swizzle, DPP row_ror:8 -- and so does the amax.
//     No LDS memory.  Half-split (NeoX) pairs (j, j + rot / 2) are rot / 16 lanes apart with the same e: the partner's four words come
//     by ds_bpermute; interleaved (GPT-J) pairs are the two halves of a lane's own words.  A lane's columns are all below rot or none.
//     Eight codes leave as one 8-byte store; lane 0 of the row writes the scale (or W).  EXEC is full through the arithmetic: a row
//     that is not written runs on zeros and only its loads and stores are skipped.
//   * UNITS.  Workgroups [0, k_blocks) are K units with mla_append_kernel's position-aligned split: (sequence, 64 positions), a wave 16
//     positions aligned to 16, hence one page; the length and the page entry are wave-uniform, and a wave without a position to write
//     leaves before it reads its entry.  Row i goes to p = L - Sq + i >= 0, L = min(kv_lens[b], cap); L <= 0 writes nothing; an entry
//     outside [0, num_pages) skips its rows.  A K row is rotated at p.  The others are Q units, one per (b, i): the 64 heads are 64
//     rows, 16 per wave, all rotated at pq = max(clamp(kv_lens[b], 1, cap) - Sq + i, 0) -- one table row per workgroup; always written.
//   * All loads of a wave's rows (data, table rows, Wraw) are issued before its first store.  Every address is 64-bit arithmetic on the
//     strides.  No scratch, no atomics; every output byte has one writer; every store is a vector store.
#pragma once

#include "kv_append.hip.h"

namespace fa {

struct MlaIndexAppendParams {
    const __bf16* Knew;           // [B, Sq, 128], element strides knB, knS
    uint8_t* K;                   // [B, cap, 128] e4m3fn; paged: the pool [P, page, 128]
    float* k_scale;               // [B, cap]; paged: [P, page]
    const __bf16* Qraw;           // [B, Sq, 64, 128], element strides qB, qH, qS; NULL: no Q units
    const float* Wraw;            // [B, Sq, 64]
    uint8_t* Qidx;                // [B, Sq, 64, 128] e4m3fn
    float* W;                     // [B, Sq, 64]
    const float* cos_sin;         // [max_pos][rot] (device memory); NULL: no rotation
    const int32_t* kv_lens;       // optional [B] (device memory); NULL = the capacity
    const int32_t* block_table;   // paged: [B][table_stride] page numbers (device memory)
    int64_t knB, knS, qB, qH, qS, table_stride;
    float w_scale;
    int Sq, cap;
    int row_blocks, k_blocks;     // position blocks per sequence: ceil(Sq / 64) + 1; K units: B * row_blocks
    int num_pages, page_shift;
    int rot, interleaved, pow2;
};

struct MlaIndexAppendCfg {
    static constexpr int HEADS = 64, D = 128;
    static constexpr int LPR = D / 8;                          // lanes per row
    static constexpr int RPI = 64 / LPR;                       // rows per wave instruction
    static constexpr int NR = KvAppendCfg::WROWS / RPI;        // rows per lane
    static_assert(HEADS == KvAppendCfg::BLOCK, "a Q unit's heads are one workgroup's rows");
};

// the value lane ^ M holds, M = 1, 2, 4, 8: inside the 16-lane group of a row.  EXEC must be full
template <int M>
__device__ __forceinline__ float idx_lane_xor(float v) {
    const int u = __float_as_int(v);
    if constexpr (M == 1) return __int_as_float(__builtin_amdgcn_update_dpp(0, u, 0xB1, 0xF, 0xF, true));         // quad_perm:[1,0,3,2]
    else if constexpr (M == 2) return __int_as_float(__builtin_amdgcn_update_dpp(0, u, 0x4E, 0xF, 0xF, true));    // quad_perm:[2,3,0,1]
    else if constexpr (M == 4) return __int_as_float(__builtin_amdgcn_ds_swizzle(u, 0x101F));                     // bit mode: xor 4
    else return __int_as_float(__builtin_amdgcn_update_dpp(0, u, 0x128, 0xF, 0xF, true));                         // row_ror:8
}

// What lane g of a row needs to rotate its eight columns
struct IdxRot {
    bool on;          // the lane's columns are below rot
    bool first;       // half-split: the lane holds first members of its pairs (y1), else second ones (y2)
    int partner;      // half-split: the byte address (ds_bpermute) of the lane that holds the other members
    int c_off;        // the lane's cosines in a table row; its sines are rot / 2 behind them
};

__device__ __forceinline__ IdxRot idx_rot(const MlaIndexAppendParams& p, int lane) {
    const int g = lane & 15, h = p.rot >> 4;     // h: lanes per half of the rotated columns
    IdxRot r;
    r.on = p.cos_sin != nullptr && g < 2 * h;
    r.first = g < h;
    r.partner = 4 * (r.on && !p.interleaved ? (r.first ? lane + h : lane - h) : lane);
    r.c_off = p.interleaved ? 4 * g : 8 * (r.first ? g : g - h);
    return r;
}

// the angles of the lane's eight columns from table row `row`: c[e], s[e] belong to column 8 g + e
__device__ __forceinline__ void idx_angles(const float* row, int rot, bool interleaved, const IdxRot& r, bool ok, float (&c)[8],
                                           float (&s)[8]) {
    f32x4 t[4] = {};
    if (r.on && ok) {
        const float* cp = row + r.c_off;
        const float* sp = cp + (rot >> 1);
        t[0] = *reinterpret_cast<const f32x4*>(cp);
        t[2] = *reinterpret_cast<const f32x4*>(sp);
        if (!interleaved) {
            t[1] = *reinterpret_cast<const f32x4*>(cp + 4);
            t[3] = *reinterpret_cast<const f32x4*>(sp + 4);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        c[e] = interleaved ? t[0][e >> 1] : e < 4 ? t[0][e] : t[1][e - 4];
        s[e] = interleaved ? t[2][e >> 1] : e < 4 ? t[2][e] : t[3][e - 4];
    }
}

// One row, as its sixteen lanes see it: x the lane's eight bf16 -> the lane's eight codes; the row's scale in every lane of the row.
// rope, interleaved, pow2 are wave-uniform
__device__ __forceinline__ u32x2 idx_row(u32x4 x, const float (&c)[8], const float (&s)[8], const IdxRot& r, bool rope, bool interleaved,
                                         bool pow2, int g, float& scale) {
#pragma clang fp contract(off)
    float t[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) { t[2 * w] = bf16_lo(x[w]); t[2 * w + 1] = bf16_hi(x[w]); }

    if (rope) {
        float o[8];                                  // the other member of every pair
        if (interleaved) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = t[e ^ 1];
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t u = (uint32_t)__builtin_amdgcn_ds_bpermute(r.partner, (int)x[w]);
                o[2 * w] = bf16_lo(u); o[2 * w + 1] = bf16_hi(u);
            }
        }
        float y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {                // rope_pair: y1 = fmaf(x1, c, -(x2 s)), y2 = fmaf(x2, c, x1 s)
            const float os = o[e] * s[e];
            const bool y1 = interleaved ? (e & 1) == 0 : r.first;
            y[e] = __builtin_fmaf(t[e], c[e], y1 ? -os : os);
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {                // rounded once to bf16; the columns at or beyond rot untouched
            const uint32_t yw = pack_bf16(y[2 * w], y[2 * w + 1]);
            if (r.on) { t[2 * w] = bf16_lo(yw); t[2 * w + 1] = bf16_hi(yw); }
        }
    }

    // strides 1, 2, 4: the lane's own registers
#pragma unroll
    for (int st = 1; st < 8; st <<= 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e & st) continue;
            const float a = t[e], b = t[e + st];
            t[e] = a + b;
            t[e + st] = a - b;
        }
    }
    // strides 8, 16, 32, 64: lane g ^ 1, 2, 4, 8; the lane with the bit clear holds a
    auto stage = [&]<int M>() {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float o = idx_lane_xor<M>(t[e]);
            t[e] = (g & M) ? o - t[e] : t[e] + o;
        }
    };
    stage.template operator()<1>();
    stage.template operator()<2>();
    stage.template operator()<4>();
    stage.template operator()<8>();

    // r = bf16(t * 2^-3.5); amax over the row
    constexpr float C0 = 0.08838834764831845f, C1 = (float)(1.0 / 448.0);
    uint32_t rw[4];
    float amax = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        rw[w] = pack_bf16(t[2 * w] * C0, t[2 * w + 1] * C0);
        amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(bf16_lo(rw[w])), __builtin_fabsf(bf16_hi(rw[w]))));
    }
    amax = __builtin_fmaxf(amax, idx_lane_xor<1>(amax));
    amax = __builtin_fmaxf(amax, idx_lane_xor<2>(amax));
    amax = __builtin_fmaxf(amax, idx_lane_xor<4>(amax));
    amax = __builtin_fmaxf(amax, idx_lane_xor<8>(amax));
    amax = __builtin_fmaxf(amax, 1e-4f);
    float sc = amax * C1;                            // a normal number
    if (pow2) {                                      // 2^ceil(log2 s0): the exponent, one more when the mantissa is not zero
        const uint32_t u = __float_as_uint(sc);
        sc = __uint_as_float(((u >> 23) + ((u & 0x7FFFFFu) != 0u)) << 23);
    }
    scale = sc;
    u32x2 y;
    y[0] = kv_quantise4(rw[0], rw[1], sc);
    y[1] = kv_quantise4(rw[2], rw[3], sc);
    return y;
}

template <bool PAGED>
__global__ __launch_bounds__(256) void mla_index_append_kernel(const MlaIndexAppendParams p) {
    using W = KvAppendCfg;
    using C = MlaIndexAppendCfg;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int lr = lane >> 4, g = lane & 15;
    const bool rope = p.cos_sin != nullptr, il = p.interleaved != 0, pow2 = p.pow2 != 0;
    const IdxRot rot = idx_rot(p, lane);

    if ((int)blockIdx.x < p.k_blocks) {
        // ---- a K unit: blockIdx -> (sequence, position block)
        const int rb = blockIdx.x % p.row_blocks;
        const int b = blockIdx.x / p.row_blocks;
        int len = p.cap;
        if (p.kv_lens) len = min(p.kv_lens[b], p.cap);
        len = __builtin_amdgcn_readfirstlane(len);
        if (len <= 0) return;                                  // an inactive slot: nothing is written
        const int first = max(len - p.Sq, 0);                  // the position of the first row written
        const int pw = ((first / W::BLOCK + rb) * W::WAVES + wave) * W::WROWS;   // this wave's 16 positions
        if (pw + W::WROWS <= first || pw >= len) return;       // (before the table entry is read)

        int64_t row0;                                          // the wave's first row in the cache or the pool
        if constexpr (PAGED) {
            const int entry = __builtin_amdgcn_readfirstlane(p.block_table[b * p.table_stride + (pw >> p.page_shift)]);
            if (entry < 0 || entry >= p.num_pages) return;     // not clamped: a clamped write would land in another sequence's page
            row0 = ((int64_t)entry << p.page_shift) + (pw & ((1 << p.page_shift) - 1));
        } else {
            row0 = (int64_t)b * p.cap + pw;
        }
        const __bf16* src = p.Knew + (int64_t)b * p.knB + 8 * g;
        const int shift = len - p.Sq;                          // position - shift = the new row's index (>= 0 from `first` on)

        u32x4 x[C::NR];
        bool ok[C::NR];
        float c[C::NR][8], s[C::NR][8];
#pragma unroll
        for (int j = 0; j < C::NR; ++j) {
            const int pos = pw + j * C::RPI + lr;
            ok[j] = pos >= first && pos < len;
            x[j] = u32x4{0u, 0u, 0u, 0u};
            if (ok[j]) x[j] = *reinterpret_cast<const u32x4*>(src + (int64_t)(pos - shift) * p.knS);
            idx_angles(p.cos_sin + (int64_t)pos * p.rot, p.rot, il, rot, ok[j], c[j], s[j]);
        }
#pragma unroll
        for (int j = 0; j < C::NR; ++j) {
            float scale;
            const u32x2 y = idx_row(x[j], c[j], s[j], rot, rope, il, pow2, g, scale);
            if (!ok[j]) continue;
            const int64_t row = row0 + j * C::RPI + lr;
            *reinterpret_cast<u32x2*>(p.K + row * C::D + 8 * g) = y;
            if (g == 0) p.k_scale[row] = scale;
        }
        return;
    }

    // ---- a Q unit: blockIdx -> (sequence, query row); the 64 heads are the workgroup's rows
    const int u = blockIdx.x - p.k_blocks;
    const int b = u / p.Sq, i = u - b * p.Sq;
    int len = p.cap;
    if (p.kv_lens) len = p.kv_lens[b];
    len = __builtin_amdgcn_readfirstlane(len);
    const int pq = max(min(max(len, 1), p.cap) - p.Sq + i, 0); // the row's position: flash_attention_rope_append's
    const int64_t orow = ((int64_t)b * p.Sq + i) * C::HEADS;   // the row's first head in Qidx and W
    const __bf16* src = p.Qraw + (int64_t)b * p.qB + (int64_t)i * p.qS + 8 * g;

    float c[8], s[8];
    idx_angles(p.cos_sin + (int64_t)pq * p.rot, p.rot, il, rot, true, c, s);
    u32x4 x[C::NR];
    float wr[C::NR];
#pragma unroll
    for (int j = 0; j < C::NR; ++j) {
        const int h = wave * W::WROWS + j * C::RPI + lr;
        x[j] = *reinterpret_cast<const u32x4*>(src + (int64_t)h * p.qH);
        wr[j] = 0.f;
        if (g == 0) wr[j] = p.Wraw[orow + h];
    }
#pragma unroll
    for (int j = 0; j < C::NR; ++j) {
        const int h = wave * W::WROWS + j * C::RPI + lr;
        float scale;
        const u32x2 y = idx_row(x[j], c, s, rot, rope, il, pow2, g, scale);
        *reinterpret_cast<u32x2*>(p.Qidx + (orow + h) * C::D + 8 * g) = y;
        if (g == 0) {
#pragma clang fp contract(off)
            const float ws = wr[j] * scale;
            p.W[orow + h] = ws * p.w_scale;
        }
    }
}

// the instantiation for (paged): inst_mla_index_append.hip
Kernel mla_index_append_kernel_of(bool paged);

}  // namespace fa
