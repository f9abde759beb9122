// rope_append.hip.h -- the K/V cache append with the ROTARY EMBEDDING fused in (flash_attention_rope_append, _paged, _varlen,
// _paged_varlen): one launch rotates the new K rows at their cache positions and stores them (bf16 or e4m3fn),
// appends the new V rows exactly as kv_append.hip.h does, and rotates the step's Q rows at the same positions into Qout (bf16).
//
//   * POSITIONS.  Lq = clamp(kv_lens[b], 1, cap) (NULL: cap) ALREADY counts the new rows.  Row i of a sequence has the VIRTUAL position
//     v = Lq - Sq + i, which may be negative.  Q row i is always written, rotated at table row max(v, 0): the position decode's and
//     extend's bottom-right mask gives it ("at least key 0"; an inactive slot clamped to length 1).  K / V row i is written iff
//     kv_lens[b] > 0 and v >= 0, at position v: the twin's rule (for kv_lens[b] > 0, Lq = min(kv_lens[b], cap) is the twin's L).
//   * THE TABLE.  cos_sin is fp32 [max_pos, rot]: row p holds cos(p theta_j), j < rot / 2, then sin(p theta_j).  max_pos >= cap is
//     checked by the host, every row read is below Lq <= cap: nothing is clamped here.  No sine is computed here.
//   * A LANE owns BOTH members of every pair it rotates: D / 16 lanes hold a row, lane k of them two 8-element chunks A and B --
//       half-split (NeoX) pairs (j, j + rot / 2):  A = columns [8k, 8k + 8), B = [rot / 2 + 8k, + 8): element e of A pairs element e of B;
//       interleaved (GPT-J) pairs (2j, 2j + 1):    A = [16k, 16k + 8), B = [16k + 8, 16k + 16): the two halves of every 32-bit word;
//       k >= rot / 16 (columns >= rot):            A = [16k, 16k + 8), B = [16k + 8, 16k + 16), stored as loaded.
//     Either way lane k < rot / 16 needs the angles 8k .. 8k + 7: 32 bytes of cosines and 32 bytes of sines, two 16-byte loads each,
//     ONCE per position -- reused over every head the lane loops on.  Qout == Q (in place) has one reader-writer per element: no LDS.
//   * VALUES (pinned to the bit; rope_pair).  x1, x2 the pair as fp32, c, s from the table: y1 = fmaf(x1, c, -(x2 * s)),
//     y2 = fmaf(x2, c, x1 * s), the lone product rounded to fp32 first; y rounded ONCE to bf16 (nearest even).  That bf16 is Qout's
//     element; for K it goes through kv_append.hip.h's store (kv_store8), so the caches hold what
//     kv_append_kernel stores for the bf16 rotation of K, byte for byte.  V and the columns >= rot never pass through arithmetic.
//   * HEADS.  The units of one K/V head are its K row, its V row and the rows of its G = H / Hkv query heads.  A workgroup takes a
//     SLICE of heads_per_slice consecutive K/V heads and loops over their units; the host makes as many slices as fill the device and
//     no more (FlashAttention.hip: kv_append_run), so a position's table row is read once per slice, not once per head.  Units
//     are taken UB at a time: all their loads are issued, then they are rotated and stored.
//   * UNIFORM kernel: kv_append_kernel's decomposition (KvAppendCfg: blocks of 64, waves of 16 aligned positions, one page each) in
//     the space of v, first = Lq - Sq: a wave's positions are all negative or none.  The length, the descales and the page entry are
//     wave-uniform; a wave reads its page entry only if it writes K / V rows.  An entry outside [0, num_pages) skips the K / V rows,
//     not the Q rows.
//   * RAGGED kernel: kv_append_varlen_kernel's: token-major, D / 16 lanes per token, a binary search in cu_q, per-lane position and
//     page entry; a token no sequence owns is neither read nor written.
//   * POSITION OFFSETS (POS; flash_attention_rope_append_pos, _paged_pos): the uniform kernel with the table row of
//     new row i taken from pos_offsets[b, i] instead of i -- max(first + clamp(pos_offsets[b, i], 0, Sq - 1), 0), for Q and for K: a
//     draft tree's node rotates at base + its depth.  The row's SLOT, its V and everything else are the twin's; the offset i is the twin.
//     A lane loads the offsets of the rows it owns (4 bytes each, only where the Q row exists) before their table rows; the clamp keeps
//     the table row below Lq, so a stale offset gives a wrong angle, never an address outside the table.
//   * Every address is 64-bit arithmetic on element strides.  No LDS, no scratch, no atomics; every store is a vector store of 16
//     bytes (8 into an fp8 cache).
#pragma once

#include <type_traits>

#include "kv_append.hip.h"

namespace fa {

struct RopeAppendParams {
    KvAppendParams a;             // the K / V side: the twin's (Sq; ragged: totalQ)
    const __bf16* Q;
    __bf16* Qout;                 // may be Q itself
    const float* cos_sin;         // [max_pos][rot] (device memory)
    int64_t qB, qH, qS, oB, oH, oS;   // element strides of Q and Qout
    int G;                        // query heads per K/V head
    int rot;                      // rotDim: a multiple of 16 in [16, D]
    int interleaved;              // 0: pairs (j, j + rot / 2); 1: pairs (2j, 2j + 1)
    int head_slices, heads_per_slice;   // ceil(Hkv / heads_per_slice) slices of consecutive K/V heads
};

// the POS kernel's: a type of its own, so that RopeAppendParams keeps its size and layout
struct RopePosParams : RopeAppendParams {
    const int32_t* pos_offsets;   // [B][Sq] (device memory)
};

struct RopeAppendVarlenParams {
    RopeAppendParams r;           // a.knB / a.vnB, qB / oB, a.row_blocks: not read
    const int32_t* cu_q;          // [B + 1] (device memory)
    int B;
    int token_blocks;             // ceil(totalQ / (256 / (D / 16)))
};

// one pair: the products that stand alone are rounded to fp32, the others are fused
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& y1, float& y2) {
#pragma clang fp contract(off)
    const float x2s = x2 * s, x1s = x1 * s;
    y1 = __builtin_fmaf(x1, c, -x2s);
    y2 = __builtin_fmaf(x2, c, x1s);
}

// the eight pairs a lane holds in its chunks A and B, angles 0 .. 7 of c / s, rounded to bf16 in place
__device__ __forceinline__ void rope_rotate(u32x4& a, u32x4& b, const float (&c)[8], const float (&s)[8], bool interleaved) {
    if (interleaved) {   // pair w is the 32-bit word w of (A, B)
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const uint32_t x = w < 4 ? a[w] : b[w - 4];
            float y1, y2;
            rope_pair(bf16_lo(x), bf16_hi(x), c[w], s[w], y1, y2);
            const uint32_t y = pack_bf16(y1, y2);
            if (w < 4) a[w] = y; else b[w - 4] = y;
        }
    } else {             // pair e is element e of A with element e of B
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            float y1l, y2l, y1h, y2h;
            rope_pair(bf16_lo(a[w]), bf16_lo(b[w]), c[2 * w], s[2 * w], y1l, y2l);
            rope_pair(bf16_hi(a[w]), bf16_hi(b[w]), c[2 * w + 1], s[2 * w + 1], y1h, y2h);
            a[w] = pack_bf16(y1l, y1h);
            b[w] = pack_bf16(y2l, y2h);
        }
    }
}

// What one lane does with its NR rows (RSTEP rows apart in the new rows, in Q and in the cache slab) over the K/V heads of `slice`.
// Per row j: q_ok (the Q row exists), kv_ok (its K / V rows are written), pq (its table row).  *_row: element offsets of row 0
// without the head and the column -- Knew, Vnew, Q, Qout, and the K / V caches (batch entry or page included).  k: the lane's index
// among the D / 16 lanes of the row.
template <int D, bool KV8, int NR, int RSTEP>
__device__ __forceinline__ void rope_heads(const RopeAppendParams& r, int slice, const bool (&q_ok)[NR], const bool (&kv_ok)[NR],
                                           const int (&pq)[NR], int64_t kn_row, int64_t vn_row, int64_t q_row, int64_t o_row,
                                           int64_t k_row, int64_t v_row, int k) {
    const KvAppendParams& p = r.a;
    constexpr int ES = KV8 ? 1 : 2;      // bytes per cache element
    constexpr int UB = 4 / NR;           // units per batch of loads: four rows of 32 bytes in flight per lane
    const bool rotates = k < (r.rot >> 4);
    const int col_a = rotates && !r.interleaved ? 8 * k : 16 * k;
    const int col_b = rotates && !r.interleaved ? (r.rot >> 1) + 8 * k : 16 * k + 8;

    // the angles of the lane's pairs, once per row
    float c[NR][8], s[NR][8];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        f32x4 t[4] = {};
        if (rotates && q_ok[j]) {
            const float* row = r.cos_sin + (int64_t)pq[j] * r.rot + 8 * k;
            t[0] = *reinterpret_cast<const f32x4*>(row);
            t[1] = *reinterpret_cast<const f32x4*>(row + 4);
            t[2] = *reinterpret_cast<const f32x4*>(row + (r.rot >> 1));
            t[3] = *reinterpret_cast<const f32x4*>(row + (r.rot >> 1) + 4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { c[j][e] = t[0][e]; c[j][4 + e] = t[1][e]; s[j][e] = t[2][e]; s[j][4 + e] = t[3][e]; }
    }

    const int h0 = slice * r.heads_per_slice, h1 = min(h0 + r.heads_per_slice, p.Hkv);
    const int units = 2 + r.G;           // of one K/V head: K, V, its query heads
    for (int kvh = h0; kvh < h1; ++kvh) {
        float kds = 1.f, vds = 1.f;
        if constexpr (KV8) {
            if (p.k_descale) kds = p.k_descale[kvh];
            if (p.v_descale) vds = p.v_descale[kvh];
        }
        for (int ub = 0; ub < units; ub += UB) {
            u32x4 xa[UB][NR], xb[UB][NR];
#pragma unroll
            for (int t = 0; t < UB; ++t) {
                const int u = ub + t;            // wave-uniform: 0 K, 1 V, 2 + g the g-th query head
                const __bf16* src = u == 0 ? p.Knew + (int64_t)kvh * p.knH : u == 1 ? p.Vnew + (int64_t)kvh * p.vnH
                                                                                    : r.Q + ((int64_t)kvh * r.G + (u - 2)) * r.qH;
                const int64_t row = u == 0 ? kn_row : u == 1 ? vn_row : q_row, step = RSTEP * (u == 0 ? p.knS : u == 1 ? p.vnS : r.qS);
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    xa[t][j] = xb[t][j] = u32x4{0u, 0u, 0u, 0u};
                    if (u < units && (u < 2 ? kv_ok[j] : q_ok[j])) {
                        const __bf16* x = src + row + j * step;
                        xa[t][j] = *reinterpret_cast<const u32x4*>(x + col_a);
                        xb[t][j] = *reinterpret_cast<const u32x4*>(x + col_b);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < UB; ++t) {
                const int u = ub + t;
                if (u >= units) break;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    if (!(u < 2 ? kv_ok[j] : q_ok[j])) continue;
                    if (u != 1 && rotates) rope_rotate(xa[t][j], xb[t][j], c[j], s[j], r.interleaved != 0);
                    if (u < 2) {
                        char* dst = (char*)(u == 0 ? p.K : p.V);
                        const int64_t cH = u == 0 ? p.kH : p.vH, cS = u == 0 ? p.kS : p.vS;
                        dst += ((u == 0 ? k_row : v_row) + (int64_t)kvh * cH + j * (RSTEP * cS)) * ES;
                        kv_store8<KV8>(dst + col_a * ES, xa[t][j], u == 0 ? kds : vds);
                        kv_store8<KV8>(dst + col_b * ES, xb[t][j], u == 0 ? kds : vds);
                    } else {
                        __bf16* dst = r.Qout + ((int64_t)kvh * r.G + (u - 2)) * r.oH + o_row + j * (RSTEP * r.oS);
                        *reinterpret_cast<u32x4*>(dst + col_a) = xa[t][j];
                        *reinterpret_cast<u32x4*>(dst + col_b) = xb[t][j];
                    }
                }
            }
        }
    }
}

template <int D, bool KV8, bool PAGED, bool POS = false>
__global__ __launch_bounds__(256) void rope_append_kernel(const std::conditional_t<POS, RopePosParams, RopeAppendParams> r) {
    using C = KvAppendCfg;             // WROWS, BLOCK: of VIRTUAL positions here
    const KvAppendParams& p = r.a;
    constexpr int LPR = D / 16;          // lanes per row
    constexpr int RPI = 64 / LPR;        // rows per wave instruction
    constexpr int NR = C::WROWS / RPI;   // rows per lane
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;

    // blockIdx -> (sequence, position block, head slice); the slice runs fastest
    int u = blockIdx.x;
    const int slice = u % r.head_slices; u /= r.head_slices;
    const int rb = u % p.row_blocks;
    const int b = u / p.row_blocks;

    int len = p.cap;
    if (p.kv_lens) len = p.kv_lens[b];
    len = __builtin_amdgcn_readfirstlane(len);
    const int lq = min(max(len, 1), p.cap);                // the length the attention calls use
    const int first = lq - p.Sq;                           // the virtual position of row 0: negative when the rows outnumber the length
    // this wave's 16 virtual positions (>> floors: blocks are aligned below zero too)
    const int vw = (((first >> 6) + rb) * C::WAVES + wave) * C::WROWS;
    if (vw + C::WROWS <= first || vw >= lq) return;        // (before the table entry is read)

    bool kv_wave = len > 0 && vw >= 0;                     // the wave's rows that exist are K / V rows
    int64_t k_row = 0, v_row = 0;
    int row0 = vw;                                         // the wave's first row within its cache slab
    if (kv_wave) {
        if constexpr (PAGED) {
            const int entry = __builtin_amdgcn_readfirstlane(p.block_table[b * p.table_stride + (vw >> p.page_shift)]);
            if (entry < 0 || entry >= p.num_pages) kv_wave = false;   // not clamped: K and V are skipped, Q is not
            k_row = (int64_t)entry * p.kB;
            v_row = (int64_t)entry * p.vB;
            row0 = vw & ((1 << p.page_shift) - 1);
        } else {
            k_row = (int64_t)b * p.kB;
            v_row = (int64_t)b * p.vB;
        }
    }

    const int lr = lane / LPR, k = lane % LPR;
    bool q_ok[NR], kv_ok[NR];
    int pq[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int v = vw + j * RPI + lr;
        q_ok[j] = v >= first && v < lq;
        kv_ok[j] = kv_wave && q_ok[j];
        pq[j] = max(v, 0);
        if constexpr (POS) {                               // the row's offset in place of its index v - first
            int off = 0;
            if (q_ok[j]) off = r.pos_offsets[(int64_t)b * p.Sq + (v - first)];
            pq[j] = max(first + min(max(off, 0), p.Sq - 1), 0);
        }
    }
    const int64_t i0 = vw + lr - first;                    // the index of the lane's first row among the new rows
    rope_heads<D, KV8, NR, RPI>(r, slice, q_ok, kv_ok, pq, (int64_t)b * p.knB + i0 * p.knS, (int64_t)b * p.vnB + i0 * p.vnS,
                                (int64_t)b * r.qB + i0 * r.qS, (int64_t)b * r.oB + i0 * r.oS, k_row + (int64_t)(row0 + lr) * p.kS,
                                v_row + (int64_t)(row0 + lr) * p.vS, k);
}

template <int D, bool KV8, bool PAGED>
__global__ __launch_bounds__(256) void rope_append_varlen_kernel(const RopeAppendVarlenParams pv) {
    const RopeAppendParams& r = pv.r;
    const KvAppendParams& p = r.a;
    constexpr int LPR = D / 16;          // lanes per token
    constexpr int TPB = 256 / LPR;       // tokens per workgroup

    // blockIdx -> (token block, head slice); the slice runs fastest
    const int slice = blockIdx.x % r.head_slices, tb = blockIdx.x / r.head_slices;
    const int t = tb * TPB + (int)threadIdx.x / LPR, k = (int)threadIdx.x % LPR;
    if (t >= p.Sq) return;

    // the last sequence whose first token is at or below t
    int lo = 0, hi = pv.B;               // cu_q[lo] <= t (or lo = 0) and cu_q[hi] > t (or hi = B)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pv.cu_q[mid] <= t) lo = mid; else hi = mid;
    }
    const int b = lo;
    const int q0 = min(max(pv.cu_q[b], 0), p.Sq), q1 = min(max(pv.cu_q[b + 1], q0), p.Sq);
    if (t < q0 || t >= q1) return;       // a token no sequence owns

    int len = p.cap;
    if (p.kv_lens) len = p.kv_lens[b];
    const int lq = min(max(len, 1), p.cap);
    const int v = lq - (q1 - q0) + (t - q0);               // < lq <= cap
    bool kv = len > 0 && v >= 0;
    int64_t k_row = 0, v_row = 0;
    int row = v;
    if (kv) {
        if constexpr (PAGED) {
            const int entry = p.block_table[b * p.table_stride + (v >> p.page_shift)];
            if (entry < 0 || entry >= p.num_pages) kv = false;        // not clamped: K and V are skipped, Q is not
            k_row = (int64_t)entry * p.kB;
            v_row = (int64_t)entry * p.vB;
            row = v & ((1 << p.page_shift) - 1);
        } else {
            k_row = (int64_t)b * p.kB;
            v_row = (int64_t)b * p.vB;
        }
    }
    const bool q_ok[1] = {true}, kv_ok[1] = {kv};
    const int pq[1] = {max(v, 0)};
    rope_heads<D, KV8, 1, 0>(r, slice, q_ok, kv_ok, pq, (int64_t)t * p.knS, (int64_t)t * p.vnS, (int64_t)t * r.qS, (int64_t)t * r.oS,
                             k_row + (int64_t)row * p.kS, v_row + (int64_t)row * p.vS, k);
}

// the instantiation for (d, fp8 cache, paged): inst_rope_append.hip
Kernel rope_append_kernel_of(int d, bool kv8, bool paged);
Kernel rope_append_pos_kernel_of(int d, bool kv8, bool paged);
Kernel rope_append_varlen_kernel_of(int d, bool kv8, bool paged);

}  // namespace fa
