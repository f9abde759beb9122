// fwd_mla.hip.h -- the kernel of flash_attention_mla_prefill: the forward pass of multi-head latent attention in
// its UP-PROJECTED (prefill) form.  Ordinary multi-head attention whose score and value widths differ:
//     O = softmax(scale Q K^T [+ top-left causal mask]) V,   Q [B, H, Sq, 192], K [B, H, Sk, 192], V [B, H, Sk, 128], O [B, H, Sq, 128]
// fwd_mfma_kernel (kernel_bf16.hip.h) is built around ONE head dimension: its ring slot, its staging pieces and its d-block loops all
// take D.  This kernel has a geometry of its own:
//   * the work unit is (batch, head, block of 256 query rows), one workgroup of four waves per unit, one workgroup per CU; the grid is
//     one workgroup per unit in unit_of_block's order (loaders.hip.h): an XCD group walks a contiguous range of units, so the query
//     blocks of a head -- which re-read the same K and V -- run close together on one L2, and under the mask a head's blocks start
//     heaviest first; the hardware hands the next unit to the first CU that is free, which balances the unequal units without atomics
//     or a workspace;
//   * a wave owns 64 query rows as two 32-row tiles (RT = 2) on v_mfma_f32_32x32x16_bf16.  Scores are S^T = K Q^T: a query row is a
//     COLUMN of the product, so its 64 scores of a key tile live in the lane pair (l, l ^ 32) and the softmax needs one
//     v_permlane32_swap.  The B fragments of Q^T for all 192 columns stay in registers for the unit: 12 k-steps x 4 VGPRs x RT = 96.
//     Every K fragment and every V^T fragment read from LDS feeds BOTH row tiles: half the LDS reads per MFMA of a 32-row wave;
//   * the rounded weights are the B operand of O^T = V^T P^T as they stand: register 8u + j of a score tile holds key
//     16u + 8(j >> 2) + 4h + (j & 3), and V^T is read by ds_read_b64_tr_b16 in that key order.  O^T covers the 128 value columns only:
//     4 d-blocks x 16 x RT = 128 accumulator VGPRs;
//   * a 64-key tile is staged once per workgroup as TWO row-major images of different row length, both padded (derivation below):
//     K rows of 384 + 16 bytes, V rows of 256 + 64 bytes; 45 KiB per slot, two slots.  The tile in flight lives in REGISTERS, not in
//     a third slot: 6 + 4 buffer_load_dwordx4 per lane are issued right after the barrier that publishes tile t and written to the
//     other slot when tile t's arithmetic is done, so the fetch of tile t + 1 is in flight during all of it and one barrier per
//     tile suffices (the slot written at step t + 1 was last read at step t - 1, which every wave left before the barrier of step t).
//     Three 40-KiB slots filled by LDS-DMA would spare the 40 staging registers, which this kernel -- one wave per SIMD, 512
//     registers -- does not miss, and would need images cut into linear 1-KiB pieces, which a padded row is not;
//   * rows at and beyond Sk are V rows too: the tile is fetched through buffer descriptors that end at the head's last row, so they
//     arrive as zeros; their scores are masked by index;
//   * under the mask a unit fetches the tiles up to its last row's diagonal and no further, a wave computes the tiles up to ITS last
//     row's diagonal, and only a tile that crosses the wave's diagonal or the end of K takes the select (a wave-uniform branch);
//   * precision: fp32 scores, a tracked running max, fp32 sum of the UNROUNDED weights.  A unit whose first row sees fewer than
//     FA_EARLY_KEYS keys (query block < Params::hp) feeds the weights as a bf16 hi + lo pair -- two MFMAs on one V^T fragment, as in
//     decode -- every other unit as single bf16: a workgroup-uniform choice, two instantiations of the tile step.
//
// The LDS images.  LDS has 64 banks of 4 bytes; a wave's ds_read_b128 is served sixteen lanes at a time, a ds_read_b64_tr_b16 thirty-two.
//   K: lane (r = l & 31, h = l >> 5) reads the 16-byte chunk 2 ks + h of key r: sixteen lanes are sixteen keys at ONE chunk.  With rows
//      of W dwords key k starts at bank k W mod 64; W = 96 (no pad) puts keys 0 and 2 on one bank.  The sixteen 4-dword windows are
//      disjoint when k W mod 64 runs through all multiples of 4, i.e. W = 4 x odd: the smallest pad is 16 bytes, W = 100 = 4 x 25
//      (k W mod 64 = 36 k mod 64, a bijection of k mod 16 onto the multiples of 4) -- and any sixteen lanes with distinct k mod 16 do.
//   V: the 32 lanes of a half-wave's transposed read are 4 keys x 64 contiguous bytes (two 16-column groups): four 16-dword windows,
//      disjoint when W mod 64 is 16 or 48.  W = 64 (no pad) puts all four on one; the smallest pad is 64 bytes, W = 80.
#pragma once

#include "launchers.hip.h"

namespace fa {

struct MlaPrefillCfg {
    static constexpr int DQK = 192, DV = 128;                 // score columns (128 nope + 64 rotary), value columns
    static constexpr int WAVES = 4, THREADS = 256;
    static constexpr int RT = 2;                              // 32-row tiles per wave
    static constexpr int WROWS = 32 * RT;                     // query rows per wave
    static constexpr int ROWS = WAVES * WROWS;                // query rows per unit
    static constexpr int KT = 64;                             // keys per tile
    static constexpr int KS = DQK / 16;                       // 16-wide k-steps of the score product
    static constexpr int DB = DV / 32;                        // 32-wide column blocks of O^T
    static constexpr int KROW = DQK * 2 + 16;                 // LDS bytes per row of the K image (100 dwords)
    static constexpr int VROW = DV * 2 + 64;                  // ... of the V image (80 dwords)
    static constexpr int K_IMG = KT * KROW, V_IMG = KT * VROW;
    static constexpr int SLOT = K_IMG + V_IMG;                // one tile: [K image | V image]
    static constexpr int LDS_BYTES = 2 * SLOT;
    static constexpr int KCH = DQK * 2 / 16, VCH = DV * 2 / 16;   // 16-byte chunks per row
    static constexpr int KLD = KT * KCH / THREADS;            // 16-byte loads per lane and tile: K
    static constexpr int VLD = KT * VCH / THREADS;            // ... V
    static_assert(KLD == 2 * (KCH / 8) && VLD == KT / (THREADS / VCH), "the fetch's lane maps (fwd_mla_kernel)");
    static_assert((KROW / 4) % 8 == 4 && (VROW / 4) % 64 == 16, "the bank rule of the two images");
    static_assert(LDS_BYTES <= 160 * 1024, "two slots fit a CU");
};

// O^T of one row: four consecutive value columns
template <class OutT>
__device__ __forceinline__ void mla_store4(OutT* dst, float a, float b, float c, float d) {
    if constexpr (__is_same(OutT, float)) *reinterpret_cast<f32x4*>(dst) = f32x4{a, b, c, d};
    else if constexpr (__is_same(OutT, __bf16)) *reinterpret_cast<u32x2*>(dst) = u32x2{pack_bf16(a, b), pack_bf16(c, d)};
    else *reinterpret_cast<u32x2*>(dst) = u32x2{pack_f16(a, b), pack_f16(c, d)};
}

// Params as run() fills them, with: d not read (the widths are the configuration's), V's strides those of 128-wide rows, nQ the
// 256-row blocks of a head, units = B H nQ in one list (qb0 = 0), hp the leading blocks of every head that take the weight pair.
template <class OutT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void fwd_mla_kernel(const Params p) {
    using C = MlaPrefillCfg;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    int g, qb;
    if (!unit_of_block(p, CAUSAL, g, qb)) return;   // (the whole workgroup: the grid is rounded up to the XCD groups)
    const int b = g / p.H, hd = g - b * p.H;
    const int S = p.S, Sk = p.Sk;
    const int q0 = qb * C::ROWS, qw0 = q0 + wv * C::WROWS;
    const bool pair = qb < p.hp;
    // tiles the unit fetches: up to its last row's diagonal; tiles this wave computes: up to ITS last row's (none: it holds no row)
    const int nt = ((CAUSAL ? min(Sk, min(q0 + C::ROWS, S)) : Sk) + C::KT - 1) / C::KT;
    const int ntw = qw0 >= S ? 0 : CAUSAL ? (min(Sk, min(qw0 + C::WROWS, S)) + C::KT - 1) / C::KT : nt;

    // B fragments of Q^T: row qw0 + 32 rt + r, columns 16 ks + 8 h .. + 7; a row beyond Sq is zeros (and is not written)
    bf16x8 qf[C::RT][C::KS];
    int lim[C::RT];   // the row sees the keys below lim
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
        const int q = qw0 + 32 * rt + r;
        const bool ok = q < S;
        const __bf16* qp = (const __bf16*)p.Q + b * p.qB + hd * p.qH + (ok ? q : 0) * p.qS + 8 * h;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            const u32x4 v = *reinterpret_cast<const u32x4*>(qp + 16 * ks);
            qf[rt][ks] = __builtin_bit_cast(bf16x8, ok ? v : z);
        }
        lim[rt] = CAUSAL ? min(Sk, q + 1) : Sk;
    }

    // the fetch.  K: lane tid takes, of rows (tid >> 3) + 32 i, the chunks (tid & 7) + 8 j -- 2 x 3 loads, each wave-instruction eight
    // rows x 128 contiguous bytes; V: of rows (tid >> 4) + 16 i the chunk tid & 15 -- 4 loads of four rows x 256 bytes.  One per-lane
    // offset per tensor and side, everything else scalars and immediates.  One descriptor per tensor over the head's rows: a row at or
    // beyond Sk fails the range check (which covers the VGPR offset: the tile's goes there) and reads as zeros
    const int ksb = (int)(p.kS * 2), vsb = (int)(p.vS * 2);
    const char* Kh = (const char*)p.K + (b * p.kB + hd * p.kH) * 2;
    const char* Vh = (const char*)p.V + (b * p.vB + hd * p.vH) * 2;
    const __amdgpu_buffer_rsrc_t krsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Kh, 0, (Sk - 1) * ksb + C::DQK * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Vh, 0, (Sk - 1) * vsb + C::DV * 2, 0x00020000);
    const int kgo = (tid >> 3) * ksb + (tid & 7) * 16, klo = (tid >> 3) * C::KROW + (tid & 7) * 16;
    const int vgo = (tid >> 4) * vsb + (tid & 15) * 16, vlo = C::K_IMG + (tid >> 4) * C::VROW + (tid & 15) * 16;
    u32x4 kn[C::KLD], vn[C::VLD];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int n = 0; n < C::KLD; ++n)
            kn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krsrc, kgo + (t * C::KT + 32 * (n / 3)) * ksb + (n % 3) * 128, 0, 0));
#pragma unroll
        for (int n = 0; n < C::VLD; ++n)
            vn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vrsrc, vgo + (t * C::KT + 16 * n) * vsb, 0, 0));
    };

    // K row read (kt, ks): key 32 kt + r, chunk 2 ks + h.  V transposed read (u4, jj, db): lane 4 q + pp of the 16-lane group gg of
    // half h supplies key 16 u4 + 8 jj + 4 h + q, columns 32 db + 16 gg + 4 pp .. + 3
    const int krd = r * C::KROW + h * 16;
    const int vrd = C::K_IMG + (4 * h + ((lane & 15) >> 2)) * C::VROW + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;

    const float NEG_INF = -__builtin_inff();
    float m[C::RT], l[C::RT];   // of the lane's rows: running max (log2 domain, shared by the lane pair), this lane's share of the sum
    f32x16 o[C::RT][C::DB];     // O^T: column 32 db + acc_row(reg, h), row qw0 + 32 rt + r
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
        m[rt] = NEG_INF;
        l[rt] = 0.f;
#pragma unroll
        for (int db = 0; db < C::DB; ++db)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[rt][db][e] = 0.f;
    }

    // one tile of this wave.  Every row sees key 0, so the running max is finite from tile 0 on and no difference is inf - inf
    auto tile_step = [&]<bool PAIR>(lds_ptr slot, int t) {
        f32x16 s[C::RT][2];   // S^T: s[rt][kt][reg] = key 64 t + 32 kt + acc_row(reg, h), row qw0 + 32 rt + r
#pragma unroll
        for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int e = 0; e < 16; ++e) s[rt][kt][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const bf16x8 a = lds_read_b128(slot, krd + kt * 32 * C::KROW + ks * 32);
#pragma unroll
                for (int rt = 0; rt < C::RT; ++rt) s[rt][kt] = mfma_32x32x16(a, qf[rt][ks], s[rt][kt]);
            }
        // the select: only where the tile crosses the wave's diagonal or the end of K (wave-uniform)
        const int k0 = t * C::KT;
        const bool crosses = k0 + C::KT > Sk || (CAUSAL && k0 + C::KT - 1 > qw0);
        uint32_t whi[C::RT][16], wlo[C::RT][16];
#pragma unroll
        for (int rt = 0; rt < C::RT; ++rt) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int e = 0; e < 16; ++e) s[rt][kt][e] *= p.scale_log2;
            if (crosses) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        s[rt][kt][e] = k0 + 32 * kt + 4 * h + acc_row(e, 0) < lim[rt] ? s[rt][kt][e] : NEG_INF;
            }
            float mx = NEG_INF;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[rt][kt][e]);
            mx = max_both_halves(mx);
            const float m_new = fmaxf(m[rt], mx);
            const float alpha = fast_exp2(m[rt] - m_new);
            m[rt] = m_new;
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    const float p0 = fast_exp2(s[rt][kt][e] - m_new), p1 = fast_exp2(s[rt][kt][e + 1] - m_new);
                    sum += p0 + p1;
                    const uint32_t hi = pack_bf16(p0, p1);
                    whi[rt][8 * kt + (e >> 1)] = hi;
                    // weights as a bf16 pair: hi = bf16(p), lo = bf16(p - hi) -- 16 significant bits between them
                    if constexpr (PAIR) wlo[rt][8 * kt + (e >> 1)] = pack_bf16(p0 - bf16_lo(hi), p1 - bf16_hi(hi));
                }
            l[rt] = l[rt] * alpha + sum;
#pragma unroll
            for (int db = 0; db < C::DB; ++db) o[rt][db] *= alpha;
        }
        // O^T += V^T P^T: 16-key step u4 = registers 8 (u4 & 1) .. + 7 of score tile u4 >> 1
#pragma unroll
        for (int u4 = 0; u4 < 4; ++u4)
#pragma unroll
            for (int db = 0; db < C::DB; ++db) {
                const s16x4 a0 = lds_read_tr16_b64(slot, vrd + (16 * u4) * C::VROW + db * 64);
                const s16x4 a1 = lds_read_tr16_b64(slot, vrd + (16 * u4 + 8) * C::VROW + db * 64);
                typedef __attribute__((ext_vector_type(8))) short s16x8;
                const bf16x8 a = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                for (int rt = 0; rt < C::RT; ++rt) {
                    const uint32_t* w = &whi[rt][4 * u4];
                    o[rt][db] = mfma_32x32x16(a, __builtin_bit_cast(bf16x8, u32x4{w[0], w[1], w[2], w[3]}), o[rt][db]);
                    if constexpr (PAIR) {
                        const uint32_t* v = &wlo[rt][4 * u4];
                        o[rt][db] = mfma_32x32x16(a, __builtin_bit_cast(bf16x8, u32x4{v[0], v[1], v[2], v[3]}), o[rt][db]);
                    }
                }
            }
    };

    load_tile(0);
    for (int t = 0; t < nt; ++t) {
        // this tile: registers -> its slot, published by the barrier; then the next tile's loads, in flight under the arithmetic
        const lds_ptr slot = smem + (t & 1) * C::SLOT;
#pragma unroll
        for (int n = 0; n < C::KLD; ++n) lds_write_b128(slot, klo + 32 * (n / 3) * C::KROW + (n % 3) * 128, kn[n]);
#pragma unroll
        for (int n = 0; n < C::VLD; ++n) lds_write_b128(slot, vlo + 16 * n * C::VROW, vn[n]);
        __syncthreads();
        if (t + 1 < nt) load_tile(t + 1);
        if (t < ntw) {   // (wave-uniform: EXEC is all ones at every transposed read)
            if (pair) tile_step.template operator()<true>(slot, t);
            else tile_step.template operator()<false>(slot, t);
        }
    }

    // ---- normalise and write: a lane holds, of its row, the columns 32 db + 8 g4 + 4 h .. + 3 ----
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
        const int q = qw0 + 32 * rt + r;
        const float L = sum_both_halves(l[rt]);
        if (q < S) {
            const float inv = 1.0f / L;
            OutT* dst = (OutT*)p.O + b * p.oB + hd * p.oH + q * p.oS + 4 * h;
#pragma unroll
            for (int db = 0; db < C::DB; ++db)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    mla_store4<OutT>(dst + 32 * db + 8 * g4, o[rt][db][4 * g4] * inv, o[rt][db][4 * g4 + 1] * inv,
                                     o[rt][db][4 * g4 + 2] * inv, o[rt][db][4 * g4 + 3] * inv);
            if (p.lse && h == 0) p.lse[((int64_t)b * p.H + hd) * S + q] = (m[rt] + __log2f(L)) * 0.6931471805599453f;
        }
    }
}

}  // namespace fa
