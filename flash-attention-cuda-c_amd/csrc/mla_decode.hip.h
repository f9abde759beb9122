// mla_decode.hip.h -- the kernel of flash_attention_mla_decode / _paged: decode for multi-head latent attention in its absorbed form
// (DESIGN.md section 35).  Every query head attends ONE shared cache row per token, DL = 512 latent columns + DR = 64 rotary columns:
//     O = softmax(scale Q KV^T) KV[:, :512],   Q [B, H, Sq, 576], KV [B, Sk, 576], O [B, H, Sq, 512]
// so there is one K/V "head" for up to 128 query heads, the head dimension is 4.5 times the split-KV kernel's largest, and K and V are
// the same bytes.  split_kv_kernel (decode_bf16.hip.h) keeps a wave's O^T for the whole head dimension in registers (D/16 RT 4: 512 at
// D = 512, RT = 4) and fetches K and V as two streams; this kernel is built the other way round:
//   * the work unit is (batch, row block of 64 packed rows, key split): packed row = h * Sq + i, as in decode with G = H; four waves,
//     one per SIMD, one workgroup per CU; the keys of a sequence are divided over the splits in whole tiles of KT = 32 keys;
//   * a key tile is fetched from memory ONCE and serves both products: 32 rows x 1152 bytes go global -> registers -> one row-major LDS
//     image (two buffers), which is read by rows (ds_read_b128: the A operand of S^T = KV Q^T) and by columns (ds_read_b64_tr_b16: the
//     A operand of O^T = V^T P^T, columns below 512 only).  The image's rows are 1152 + 32 bytes apart (296 dwords = 40 mod 64): the
//     eight rows of a half-wave's transposed read fall on eight different 8-dword bank groups, and the sixteen rows of a ds_read_b128
//     lane group ({0-3, 12-15} at one 16-byte chunk, {4-11} at the next) on sixteen different 4-dword groups -- both reads are
//     conflict-free without an XOR, which a 1152-byte row has no power-of-two chunk count for;
//   * wave w computes the scores of row tile w (16 rows) against the whole tile -- its Q fragments stay in registers, 18 k-steps x 4 =
//     72 VGPRs -- and runs the online softmax of those 16 rows only; products are swapped as in decode (a softmax row lives in the four
//     lanes l, l^16, l^32, l^48); it writes the weights, as a bf16 hi + lo pair, and the rows' rescale factors to LDS;
//   * after a barrier wave w owns the output columns [128 w, 128 w + 128) of ALL 64 rows: 8 column groups x 4 row tiles x 4 = 128
//     accumulator VGPRs.  It reads every row tile's P^T fragment from LDS (16 bytes per lane: the MFMA's k index stands for key
//     16 (j >> 2) + 4 h4 + (j & 3), the order in which the score registers hold them and in which V^T is read) and V^T from the tile's
//     image, only its own columns.  Nothing is read twice from memory, the four waves share one image;
//   * a row tile without a row (H Sq <= 48 in the last block) is skipped, in the scores and in the P.V product: workgroup-uniform
//     branches, so EXEC is all ones at every transposed read;
//   * rows at and beyond kvLens[b] are V rows too and must arrive in LDS as zeros (0 x NaN would reach the accumulators): the tile is
//     fetched through buffer descriptors whose record count is THIS SEQUENCE's length, as in decode; their scores are masked by index;
//   * PAGED: a 16-key group lies in one page.  Waves 0, 1 fetch the tile's first group, waves 2, 3 its second, so a wave builds ONE
//     descriptor per tile, based at the group's first row (64-bit: the pool may exceed 4 GiB) and holding the group's rows below the
//     length.  The table entry is a scalar load issued one tile before the fetch that uses it; index and entry are clamped as in decode;
//   * precision is decode's: fp32 scores and softmax, hi + lo weights (FA_MLA_SINGLE_WEIGHTS, a build-time switch that is OFF in the
//     library, drops the lo product to measure its cost: tools/bench_decode.py --mla);
//   * ns = 1: the kernel normalises and writes O and the LSE.  ns > 1: normalised fp32 slabs and partial LSEs, summed by
//     decode_combine_kernel<512> in a fixed order.  An empty split writes O = 0, LSE = -inf.
// The parameters are a DecodeParams filled as decode_run fills one (K = the latent cache, V not read, Hkv = 1, G = H, kH not read).
#pragma once

#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

struct MlaCfg {
    static constexpr int DL = 512, DR = 64, D = DL + DR;     // latent (the V columns), rotary, score columns
    static constexpr int WAVES = 4, THREADS = 256;
    static constexpr int ROWS = 64;                           // packed rows per workgroup: one 16-row tile per wave
    static constexpr int KT = 32;                             // keys per tile: K of the P.V MFMA
    static constexpr int KS = D / 32;                         // 32-wide k-steps of the score product
    static constexpr int DG = DL / 16 / WAVES;                // 16-wide column groups of O^T per wave
    static constexpr int ROWB = D * 2;                        // bytes of a cache row
    static constexpr int CPR = ROWB / 16;                     // 16-byte chunks per row
    static constexpr int LROW = ROWB + 32;                    // LDS bytes per row of the image
    static constexpr int IMG = KT * LROW;                     // one tile's image
    static constexpr int NLD = 16 * CPR / 64 / 2;             // 16-byte loads per lane and tile: half a 16-key group per wave
    static constexpr int P_OFF = 2 * IMG;                     // [hi, lo][row 64][quarter 4] 16-byte fragments of P^T
    static constexpr int P_HALF = ROWS * 64;
    static constexpr int AL_OFF = P_OFF + 2 * P_HALF;         // [row 64] rescale factor of the tile; at the end M
    static constexpr int L_OFF = AL_OFF + ROWS * 4;           // at the end: [row 64] L
    static constexpr int LDS_BYTES = L_OFF + ROWS * 4;
    static_assert(16 * CPR % 128 == 0, "a wave loads half a 16-key group in whole instructions");
    static_assert(IMG % 16 == 0 && LROW % 16 == 0, "16-byte aligned rows");
};

// the two launchers of inst_mla_decode.hip: the split kernel (contiguous or paged) and decode_combine_kernel<512>
int mla_decode_launch(bool paged, unsigned grid, hipStream_t st, const DecodeParams& p);
int mla_combine_launch(unsigned rows, hipStream_t st, const DecodeParams& p);

template <bool PAGED>
__global__ __launch_bounds__(256, 1) void mla_decode_kernel(const DecodeParams p) {
    using C = MlaCfg;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h4 = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(wave);

    // blockIdx -> (batch, row block, split); the split index runs fastest
    int u = blockIdx.x;
    const int split = u % p.ns; u /= p.ns;
    const int rb = u % p.row_blocks;
    const int b = u / p.row_blocks;

    int len = p.Sk;
    if (p.kv_lens) len = min(max(p.kv_lens[b], 1), p.Sk);
    len = __builtin_amdgcn_readfirstlane(len);
    const int Sq = p.Sq, nrows = p.H * Sq;
    const int pr0 = rb * C::ROWS;
    // the row tiles of this block that hold a row (1 .. 4; the same in every wave)
    const int nrt = __builtin_amdgcn_readfirstlane((min(nrows - pr0, C::ROWS) + 15) >> 4);
    // Sq <= FA_DECODE_MAX_Q: the block holds the last row of a head or the last row of all, whose limit is len -- every tile below len
    const int nt = (len + C::KT - 1) / C::KT;
    const int t0 = (int)(((int64_t)nt * split) / p.ns), t1 = (int)(((int64_t)nt * (split + 1)) / p.ns);

    // this lane's row of the wave's row tile (column r of the swapped score product): head g, query row qi, which sees the keys below
    // lim.  Bottom-right aligned mask: the Sq rows are the LAST rows of the sequence; at least key 0
    const int pr = pr0 + wv * 16 + r;
    const bool row_ok = pr < nrows;
    const int g = row_ok ? pr / Sq : 0, qi = row_ok ? pr - g * Sq : 0;
    const int lim = p.causal ? max(len - Sq + qi + 1, 1) : len;
    // B fragments of Q^T: Q[row][32 ks + 8 h4 .. + 7]
    bf16x8 qf[C::KS];
    {
        const __bf16* q = p.Q + b * p.qB + g * p.qH + qi * p.qS + 8 * h4;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            qf[ks] = __builtin_bit_cast(bf16x8, row_ok ? *reinterpret_cast<const u32x4*>(q + 32 * ks) : z);
        }
    }

    // the fetch: waves 0, 1 take the tile's first 16-key group, waves 2, 3 its second; load n of a wave is the 16-byte chunk
    // (64 (NLD (wave & 1) + n) + lane) of the group's 16 x CPR chunks, row-major
    const int grp = wv >> 1;
    const int ksb = (int)(p.kS * 2);
    int goff[C::NLD], loff[C::NLD];
#pragma unroll
    for (int n = 0; n < C::NLD; ++n) {
        const int idx = 64 * (C::NLD * (wave & 1) + n) + lane;
        const int row = idx / C::CPR, ch = idx - row * C::CPR;
        goff[n] = row * ksb + ch * 16;
        loff[n] = (16 * grp + row) * C::LROW + ch * 16;
    }
    // contiguous: one descriptor over the VISIBLE rows of this sequence -- rows >= len read as 0
    const char* Kb = (const char*)(p.K + (PAGED ? 0 : b * p.kB));
    const __amdgpu_buffer_rsrc_t krsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, (len - 1) * ksb + C::ROWB, 0x00020000);
    // paged: this sequence's row of the table, the last page that holds a visible key, the entry of the wave's group of a tile
    const int32_t* tb = p.block_table + (PAGED ? b * p.table_stride : 0);
    const int last_page = PAGED ? (len - 1) >> p.page_shift : 0;
    auto table_entry = [&](int t) {
        const int key = t * C::KT + 16 * grp;
        return tb[min(key >> p.page_shift, last_page)];
    };
    u32x4 kn[C::NLD];
    auto load_tile = [&](int t, int entry) {
        if constexpr (!PAGED) {
            const int base = (t * C::KT + 16 * grp) * ksb;
#pragma unroll
            for (int n = 0; n < C::NLD; ++n)
                kn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krsrc, base + goff[n], 0, 0));
        } else {
            // the group's descriptor: at its first row, holding its rows below len (none: zero bytes, everything reads as 0)
            const int key = t * C::KT + 16 * grp;
            const int page = min(max(entry, 0), p.num_pages - 1);
            const __bf16* base = p.K + page * p.kB + (key & ((1 << p.page_shift) - 1)) * p.kS;
            const int rows = min(len - key, 16);
            const int bytes = rows > 0 ? (rows - 1) * ksb + C::ROWB : 0;
            const uint64_t a = (uint64_t)base;
            const uint64_t au = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
            const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc((void*)au, 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
#pragma unroll
            for (int n = 0; n < C::NLD; ++n)
                kn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(gr, goff[n], 0, 0));
        }
    };

    // row read (kg, ks): key 16 kg + r of the tile, chunk 4 ks + h4.  Transposed read (dg, jj): lane 4 q + pp of quarter h4 supplies
    // row 16 jj + 4 h4 + q, columns 128 wave + 16 dg + 4 pp .. + 3
    const int krd = r * C::LROW + h4 * 16;
    const int vrd = (4 * h4 + (r >> 2)) * C::LROW + wave * 256 + (lane & 3) * 8;
    // P^T fragment of row `row`, quarter h4 (written by the row's wave, read by all four); the row's rescale factor
    const int pwr = C::P_OFF + (wave * 16 + r) * 64 + h4 * 16;
    const int prd = C::P_OFF + r * 64 + h4 * 16;
    FA_LDS float* al = reinterpret_cast<FA_LDS float*>(smem + C::AL_OFF);
    FA_LDS float* ll = reinterpret_cast<FA_LDS float*>(smem + C::L_OFF);

    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, l = 0.f;   // of this lane's row: running max (log2 domain, shared by the row's four lanes), this lane's share of the sum
    f32x4 o[4][C::DG];            // O^T: column 128 wave + 16 dg + 4 h4 + reg, packed row 16 rt + r
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg) o[rt][dg] = f32x4{0.f, 0.f, 0.f, 0.f};

    int e_next = 0;
    if (t0 < t1) {
        int e0 = 0;
        if constexpr (PAGED) {
            e0 = table_entry(t0);
            e_next = table_entry(t0 + 1);
        }
        load_tile(t0, e0);
    }
    for (int t = t0; t < t1; ++t) {
        // this tile: registers -> its buffer of the image.  (The buffer's last readers are the P.V products of tile t - 2, which every
        // wave left before the first barrier of tile t - 1)
        const lds_ptr img = smem + ((t - t0) & 1) * C::IMG;
#pragma unroll
        for (int n = 0; n < C::NLD; ++n) lds_write_b128(img, loff[n], kn[n]);
        __syncthreads();
        if (t + 1 < t1) {   // (uniform) the next tile, in flight under both products; paged: its entry arrived a tile ago
            load_tile(t + 1, e_next);
            if constexpr (PAGED) e_next = table_entry(t + 2);
        }

        if (wv < nrt) {
            // S^T of the wave's row tile: s[kg][reg] = key 32 t + 16 kg + 4 h4 + reg, packed row r
            f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
                for (int kg = 0; kg < 2; ++kg)
                    s[kg] = mfma_16x16x32(lds_read_b128(img, krd + kg * 16 * C::LROW + ks * 64), qf[ks], s[kg]);
            const int kb = t * C::KT + 4 * h4;
            float x[8];
            float mx = NEG_INF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[j] = kb + 16 * (j >> 2) + (j & 3) < lim ? s[j >> 2][j & 3] * p.scale_log2 : NEG_INF;
                mx = fmaxf(mx, x[j]);
            }
            mx = max_all_quarters(mx);
            const float m_new = fmaxf(m, mx);
            const float m_use = m_new == NEG_INF ? 0.f : m_new;   // nothing visible yet: exp2(-inf - 0) = 0, never inf - inf
            const float alpha = fast_exp2(m - m_use);
            m = m_new;
            float sum = 0.f;
            uint32_t whi[4], wlo[4];
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const float p0 = fast_exp2(x[j] - m_use), p1 = fast_exp2(x[j + 1] - m_use);
                sum += p0 + p1;
                // weights as a bf16 pair: hi = bf16(p), lo = bf16(p - hi) -- 16 significant bits between them
                whi[j >> 1] = pack_bf16(p0, p1);
                wlo[j >> 1] = pack_bf16(p0 - bf16_lo(whi[j >> 1]), p1 - bf16_hi(whi[j >> 1]));
            }
            l = l * alpha + sum;
            lds_write_b128(smem, pwr, u32x4{whi[0], whi[1], whi[2], whi[3]});
#ifndef FA_MLA_SINGLE_WEIGHTS
            lds_write_b128(smem, pwr + C::P_HALF, u32x4{wlo[0], wlo[1], wlo[2], wlo[3]});
#endif
            if (h4 == 0) al[wave * 16 + r] = alpha;
        }
        __syncthreads();

        // O^T += V^T P^T over the row tiles that hold a row, the wave's 128 columns
        bf16x8 phi[4], plo[4];
        float alpha[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            if (rt < nrt) {
                phi[rt] = lds_read_b128(smem, prd + rt * 1024);
#ifndef FA_MLA_SINGLE_WEIGHTS
                plo[rt] = lds_read_b128(smem, prd + rt * 1024 + C::P_HALF);
#endif
                alpha[rt] = al[rt * 16 + r];
            }
        }
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg) {
            // A fragment of V^T in the weights' key order: rows 4 h4 .. + 3 (j < 4), rows 16 + 4 h4 .. + 3 (j >= 4)
            const s16x4 a0 = lds_read_tr16_b64(img, vrd + dg * 32);
            const s16x4 a1 = lds_read_tr16_b64(img, vrd + 16 * C::LROW + dg * 32);
            typedef __attribute__((ext_vector_type(8))) short s16x8;
            const bf16x8 a = __builtin_bit_cast(bf16x8, s16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]});
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                if (rt < nrt) {
                    o[rt][dg] *= alpha[rt];
                    o[rt][dg] = mfma_16x16x32(a, phi[rt], o[rt][dg]);
#ifndef FA_MLA_SINGLE_WEIGHTS
                    o[rt][dg] = mfma_16x16x32(a, plo[rt], o[rt][dg]);
#endif
                }
            }
        }
    }

    // ---- every row's (M, L) to LDS (the last tile's readers of the rescale factors must be through: one barrier), then each wave
    // normalises and writes its 128 columns of the rows that exist ----
    __syncthreads();
    const float lr = sum_all_quarters(l);
    if (h4 == 0) {
        al[wave * 16 + r] = m;
        ll[wave * 16 + r] = lr;
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int opr = pr0 + rt * 16 + r;
        if (rt < nrt && opr < nrows) {
            const float M = al[rt * 16 + r], L = ll[rt * 16 + r];
            const int oh = opr / Sq, oi = opr - oh * Sq;
            const float inv = M != NEG_INF ? 1.0f / L : 0.f;                                      // empty split: O = 0
            const float lse = M != NEG_INF ? (M + __log2f(L)) * 0.6931471805599453f : NEG_INF;    // ... LSE = -inf
            const int64_t row = ((int64_t)b * p.H + oh) * Sq + oi;
            const int col = wave * 128 + 4 * h4;
            if (p.ns == 1) {
                const int64_t base = b * p.oB + oh * p.oH + oi * p.oS + col;
#pragma unroll
                for (int dg = 0; dg < C::DG; ++dg)
#pragma unroll
                    for (int j = 0; j < 4; ++j) store_out(p.O, p.o_dtype, base + 16 * dg + j, o[rt][dg][j] * inv);
                if (p.lse && wave == 0 && h4 == 0) p.lse[row] = lse;
            } else {
                float* dst = p.part_o + ((int64_t)split * p.rows + row) * C::DL + col;
#pragma unroll
                for (int dg = 0; dg < C::DG; ++dg) *reinterpret_cast<f32x4*>(dst + 16 * dg) = o[rt][dg] * inv;
                if (wave == 0 && h4 == 0) p.part_lse[(int64_t)split * p.rows + row] = lse;
            }
        }
    }
}

}  // namespace fa
