// mla_sparse.hip.h -- the kernel of flash_attention_mla_sparse_decode*: MLA decode in which every query row (b, i) attends the cache rows a
// device-side index list names (DeepSeek-V3.2's sparse attention after its indexer):
//     O[b, h, i] = softmax over the row's keys of (scale q . KV[p, :576]) KV[p, :512],   p = indices[b, i, t], 0 <= p < lim
// The kernel is mla_decode.hip.h's from the LDS image on -- one padded row-major image per tile of KT = 32 rows, read by rows for the
// scores and through ds_read_b64_tr_b16 for P.V; four waves, each owning 16 rows of the softmax and 128 columns of O^T; the next tile in
// flight in registers; the per-tile arithmetic and its order, statement for statement -- and differs in two things:
//   * the work unit is (sequence, query row i, block of 64 HEADS, split of the slot range): rows that share a tile must share an index
//     list, so the packed row is h and not h Sq + i, and lim -- len, or under the mask max(len - Sq + i + 1, 1) -- is uniform in the
//     workgroup.  The slots [0, topk) are cut into tiles of 32 and those into splits as the dense kernel cuts its keys;
//   * a tile is 32 GATHERED rows, each at its own 64-bit address (no buffer descriptor spans a pool above 4 GiB).  The lane map is the
//     dense one: wave w fetches the slots [8 w, 8 w + 8) of the tile, NLD chunks per lane; load n of lane l belongs to slot
//     8 w + (64 n + l) / CPR.  A tile's indices travel through three stages, one tile apart, in the lanes s and s + 32 of EVERY wave:
//         raw      tile t + 3:  indices[b, i, 32 t + s], or -1 at and beyond topk (never read);
//         checked  tile t + 2:  the position if 0 <= p < lim, else -1; PAGED: its table entry, in flight (an invalid slot reads none);
//         placed   tile t + 1:  the row's 64-bit byte offset (paged: the entry clamped into [0, P)) and, by ballot, the tile's 32-bit
//                               validity word -- uniform in the workgroup, every wave computes the same one;
//     so the indices are loaded two tiles ahead of the rows and the table entry one.  A lane gets the offsets of its NLD loads by
//     ds_bpermute from the lanes that placed them (two dwords per load), not by loads of its own, and fetches with per-lane addresses
//     (global_load).  A slot that is not a key -- -1, a position at or beyond lim, a slot at or beyond topk -- is NOT fetched: its
//     chunks are zeros selected in registers, because the image's rows are V rows too (0 x NaN would reach the accumulators);
//   * the score mask is the validity word (bit 16 kg + 4 h4 + reg of the tile) where the dense kernel compares key < lim.  A tile
//     without a key leaves m, l and O as they were (m_use, as there); a row without any key ends with m = -inf: O = 0, LSE = -inf.
// ns > 1: slabs as the dense kernel writes them, summed by mla_sparse_combine_kernel -- decode_combine_kernel<512> with the one guard a
// row without a key in ANY split needs (M = -inf: weights exp(-inf - 0) = 0, O = 0, LSE = -inf; with a key every bit is the dense
// combine's).
#pragma once

#include "mla_decode.hip.h"

namespace fa {

// the parameters: a type of its own beside DecodeParams, which keeps its size and layout (as SinkDecodeParams).  row_blocks counts the
// blocks of 64 HEADS; Sk the capacity; the rest as mla_run fills it
struct MlaSparseParams : DecodeParams {
    const int32_t* indices;       // [B, Sq, topk] (device memory), element strides isB, isQ
    int64_t isB, isQ;
    int topk;
};

int mla_sparse_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparseParams& p);       // inst_mla_sparse.hip
int mla_sparse_fp8_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparseParams& p);   // inst_mla_sparse_fp8.hip
int mla_sparse_combine_launch(unsigned rows, hipStream_t st, const MlaSparseParams& p);           // inst_mla_sparse.hip
int mla_sparse_packed_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparseParams& p);   // inst_mla_sparse_packed.hip

// (mla_sparse_packed_kernel below repeats this kernel's text from the LDS image on -- Q fragments, index pipeline, scores, softmax, P.V,
// epilogue: mirror any edit of those there.)
template <bool PAGED, bool KV8 = false>
__global__ __launch_bounds__(256, 1) void mla_sparse_kernel(const MlaSparseParams p) {
    using C = MlaCfg;
    constexpr int ES = KV8 ? 1 : 2;                           // bytes per cache element
    constexpr int CB = 8 * ES;                                // bytes of a fetched chunk: 8 elements
    typedef std::conditional_t<KV8, u32x2, u32x4> chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h4 = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(wave);

    // blockIdx -> (batch, query row, head block, split); the split index runs fastest
    int u = blockIdx.x;
    const int split = u % p.ns; u /= p.ns;
    const int hb = u % p.row_blocks; u /= p.row_blocks;
    const int Sq = p.Sq;
    const int qi = u % Sq;
    const int b = u / Sq;

    int len = p.Sk;
    if (p.kv_lens) len = min(max(p.kv_lens[b], 1), p.Sk);
    len = __builtin_amdgcn_readfirstlane(len);
    // the keys this query row sees are the positions below lim (bottom-right aligned mask, at least key 0): uniform
    const int lim = p.causal ? max(len - Sq + qi + 1, 1) : len;
    const int pr0 = hb * C::ROWS;
    const int nrt = __builtin_amdgcn_readfirstlane((min(p.H - pr0, C::ROWS) + 15) >> 4);   // the row tiles that hold a head (1 .. 4)
    const int topk = p.topk;
    const int nt = (topk + C::KT - 1) / C::KT;
    const int t0 = (int)(((int64_t)nt * split) / p.ns), t1 = (int)(((int64_t)nt * (split + 1)) / p.ns);

    // this lane's row of the wave's row tile (column r of the swapped score product): head g of query row qi
    const int g0 = pr0 + wv * 16 + r;
    const bool row_ok = g0 < p.H;
    const int g = row_ok ? g0 : 0;
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

    // the fetch: wave w takes the slots [8 w, 8 w + 8) of the tile (waves 0, 1 its first 16-row group, waves 2, 3 its second: the
    // dense map); load n is chunk ch of the wave's row (64 n + lane) / CPR
    const int grp = wv >> 1;
    const int ksb = (int)(p.kS * ES);
    int coff[C::NLD], loff[C::NLD], src[C::NLD];
#pragma unroll
    for (int n = 0; n < C::NLD; ++n) {
        const int idx = 64 * (C::NLD * (wave & 1) + n) + lane;
        const int row = idx / C::CPR, ch = idx - row * C::CPR;   // row 0 .. 15 of the group
        coff[n] = ch * CB;
        loff[n] = (16 * grp + row) * C::LROW + ch * 16;
        src[n] = 16 * grp + row;                                 // the slot of the tile, and the lane that placed it
    }
    const char* const Kb = (const char*)p.K + (PAGED ? (int64_t)0 : b * p.kB * ES);
    const int32_t* const ind = p.indices + b * p.isB + qi * p.isQ;
    const int32_t* const tb = p.block_table + (PAGED ? b * p.table_stride : 0);
    const int sl = lane & 31;   // the slot this lane carries through the stages (lanes s and s + 32 alike)

    // stage 1: the raw index of slot sl of tile t; -1 where there is no slot
    auto load_index = [&](int t) {
        const int s = t * C::KT + sl;
        return t < t1 && s < topk ? ind[s] : -1;
    };
    // stage 2: the position if it is a key, else -1; paged: the key's table entry (nothing is read for a slot that is no key)
    auto check = [&](int raw, int& pos, int& entry) {
        pos = raw >= 0 && raw < lim ? raw : -1;
        entry = 0;
        if constexpr (PAGED) {
            if (pos >= 0) entry = tb[pos >> p.page_shift];
        }
    };
    // stage 3: the row's byte offset from Kb and the tile's validity word
    auto place = [&](int pos, int entry, uint32_t& olo, uint32_t& ohi) {
        int64_t off;
        if constexpr (PAGED) {
            const int page = min(max(entry, 0), p.num_pages - 1);
            off = (int64_t)page * p.kB * ES + (int64_t)(pos & ((1 << p.page_shift) - 1)) * ksb;
        } else {
            off = (int64_t)pos * ksb;
        }
        if (pos < 0) off = 0;
        olo = (uint32_t)off; ohi = (uint32_t)((uint64_t)off >> 32);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)__ballot(pos >= 0));   // lanes 0 .. 31: one bit per slot
    };
    chunk_t kn[C::NLD];
    // the rows of a placed tile: every lane asks the placing lanes for the offsets of its loads
    auto load_tile = [&](uint32_t olo, uint32_t ohi, uint32_t valid) {
#pragma unroll
        for (int n = 0; n < C::NLD; ++n) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src[n] * 4, (int)olo);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src[n] * 4, (int)ohi);
            const char* a = Kb + (int64_t)(((uint64_t)hi << 32) | lo) + coff[n];
            chunk_t v;
            if constexpr (KV8) v = u32x2{0u, 0u};
            else v = u32x4{0u, 0u, 0u, 0u};
            if ((valid >> src[n]) & 1u) v = *reinterpret_cast<const chunk_t*>(a);
            kn[n] = v;
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
    // KV8: the logical cache is KV8 * ds -- in the scores (here) and in the values (the normaliser, below)
    float ds = 1.f;
    if constexpr (KV8) ds = p.k_descale ? p.k_descale[0] : 1.f;
    const float sl2_ds = p.scale_log2 * ds;
    float m = NEG_INF, l = 0.f;   // of this lane's row: running max (log2 domain, shared by the row's four lanes), this lane's share of the sum
    f32x4 o[4][C::DG];            // O^T: column 128 wave + 16 dg + 4 h4 + reg, head 16 rt + r of the block
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg) o[rt][dg] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the pipeline's state: the validity word of the tile in LDS and of the tile in flight; the checked tile; the raw tile
    uint32_t valid = 0u, valid_next = 0u;
    int pos1 = -1, ent1 = 0, raw2 = -1;
    if (t0 < t1) {
        int pos0, ent0;
        uint32_t olo, ohi;
        check(load_index(t0), pos0, ent0);
        valid_next = place(pos0, ent0, olo, ohi);
        load_tile(olo, ohi, valid_next);
        check(load_index(t0 + 1), pos1, ent1);
        raw2 = load_index(t0 + 2);
    }
    for (int t = t0; t < t1; ++t) {
        // this tile: registers -> its buffer of the image.  (The buffer's last readers are the P.V products of tile t - 2, which every
        // wave left before the first barrier of tile t - 1)
        const lds_ptr img = smem + ((t - t0) & 1) * C::IMG;
#pragma unroll
        for (int n = 0; n < C::NLD; ++n) {
            if constexpr (KV8) lds_write_b128(img, loff[n], fp8x8_to_bf16x8(kn[n][0], kn[n][1]));
            else lds_write_b128(img, loff[n], kn[n]);
        }
        valid = valid_next;
        __syncthreads();
        if (t + 1 < t1) {   // (uniform) the next tile's rows, in flight under both products; its offsets were checked a tile ago
            uint32_t olo, ohi;
            valid_next = place(pos1, ent1, olo, ohi);
            load_tile(olo, ohi, valid_next);
            check(raw2, pos1, ent1);        // tile t + 2 (paged: its table entries leave now)
            raw2 = load_index(t + 3);
        }

        if (wv < nrt) {
            // S^T of the wave's row tile: s[kg][reg] = slot 32 t + 16 kg + 4 h4 + reg, head r
            f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
                for (int kg = 0; kg < 2; ++kg)
                    s[kg] = mfma_16x16x32(lds_read_b128(img, krd + kg * 16 * C::LROW + ks * 64), qf[ks], s[kg]);
            const uint32_t vq = valid >> (4 * h4);   // bit 16 kg + reg: this lane's eight slots
            float x[8];
            float mx = NEG_INF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[j] = (vq >> (16 * (j >> 2) + (j & 3))) & 1u ? s[j >> 2][j & 3] * (KV8 ? sl2_ds : p.scale_log2) : NEG_INF;
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
            lds_write_b128(smem, pwr + C::P_HALF, u32x4{wlo[0], wlo[1], wlo[2], wlo[3]});
            if (h4 == 0) al[wave * 16 + r] = alpha;
        }
        __syncthreads();

        // O^T += V^T P^T over the row tiles that hold a head, the wave's 128 columns
        bf16x8 phi[4], plo[4];
        float alpha[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            if (rt < nrt) {
                phi[rt] = lds_read_b128(smem, prd + rt * 1024);
                plo[rt] = lds_read_b128(smem, prd + rt * 1024 + C::P_HALF);
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
                    o[rt][dg] = mfma_16x16x32(a, plo[rt], o[rt][dg]);
                }
            }
        }
    }

    // ---- every row's (M, L) to LDS (the last tile's readers of the rescale factors must be through: one barrier), then each wave
    // normalises and writes its 128 columns of the heads that exist ----
    __syncthreads();
    const float lr = sum_all_quarters(l);
    if (h4 == 0) {
        al[wave * 16 + r] = m;
        ll[wave * 16 + r] = lr;
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int oh = pr0 + rt * 16 + r;
        if (rt < nrt && oh < p.H) {
            const float M = al[rt * 16 + r], L = ll[rt * 16 + r];
            float inv = M != NEG_INF ? 1.0f / L : 0.f;                                            // no key: O = 0
            if constexpr (KV8) inv *= ds;                                                         // (the slabs are normalised: both branches)
            const float lse = M != NEG_INF ? (M + __log2f(L)) * 0.6931471805599453f : NEG_INF;    // ... LSE = -inf
            const int64_t row = ((int64_t)b * p.H + oh) * Sq + qi;
            const int col = wave * 128 + 4 * h4;
            if (p.ns == 1) {
                const int64_t base = b * p.oB + oh * p.oH + qi * p.oS + col;
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

// 8 e4m3fn codes (two dwords) under one fp32 scale -> 8 bf16: bf16_rne(fl32(float(code) * scale)), the logical value of a packed row
__device__ __forceinline__ u32x4 fp8x8_scaled_to_bf16x8(uint32_t lo, uint32_t hi, float sc) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    return u32x4{pack_bf16(a[0] * sc, a[1] * sc), pack_bf16(b[0] * sc, b[1] * sc), pack_bf16(c[0] * sc, c[1] * sc),
                 pack_bf16(d[0] * sc, d[1] * sc)};
}

// PACKED (flash_attention_mla_sparse_decode_packed / _paged_packed): mla_sparse_kernel on MlaPackedRow's 656-byte
// rows -- 512 e4m3fn codes, four fp32 scales (one per 128 columns), 64 bf16 rotary columns; p.kB and p.kS are BYTES.  A sibling and not
// a third template form, so that the two existing forms keep their symbols and their device code to the byte.  Units, the index
// pipeline, the image and everything after it are that kernel's, statement for statement (the score scale and the normaliser are the
// bf16 form's: the scales are applied on the way INTO the image and nowhere else).  The fetch is its own -- 41 chunks of 16 bytes per row
// do not divide over the dense lane map:
//   * codes: load n of a lane is the 8 bytes [8 lane, 8 lane + 8) of slot 8 w + n -- a wave instruction is one row's 512 contiguous
//     bytes -- and becomes ONE ds_write_b128 at column 8 lane of that row: v_cvt_pk_f32_fp8, one fp32 product with the block's scale, one
//     rounding to bf16.  The slot of load n is wave-uniform, so its offset comes by v_readlane from the placing lane (no LDS traffic) and
//     the row's base is scalar;
//   * scales: one dword load beside every code load, scale lane / 16 of the same row (sixteen lanes share an address);
//   * rope: ONE 16-byte load per lane, chunk lane % 8 of slot 8 w + lane / 8 (its offset by ds_bpermute, as the other forms'), written
//     unconverted to column 512 + 8 (lane % 8).
// 17 loads per lane and tile for 8 x 656 bytes, 28 registers in flight (the bf16 form: 9 loads, 36 registers; 18 ds_bpermute where this
// form has 2).  A slot that is not a key is not fetched: zero codes under a zero scale, a zero rope chunk.
template <bool PAGED>
__global__ __launch_bounds__(256, 1) void mla_sparse_packed_kernel(const MlaSparseParams p) {
    using C = MlaCfg;
    using R = MlaPackedRow;
    constexpr int PS = C::KT / C::WAVES;                      // slots of a tile per wave
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h4 = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(wave);

    // blockIdx -> (batch, query row, head block, split); the split index runs fastest
    int u = blockIdx.x;
    const int split = u % p.ns; u /= p.ns;
    const int hb = u % p.row_blocks; u /= p.row_blocks;
    const int Sq = p.Sq;
    const int qi = u % Sq;
    const int b = u / Sq;

    int len = p.Sk;
    if (p.kv_lens) len = min(max(p.kv_lens[b], 1), p.Sk);
    len = __builtin_amdgcn_readfirstlane(len);
    const int lim = p.causal ? max(len - Sq + qi + 1, 1) : len;
    const int pr0 = hb * C::ROWS;
    const int nrt = __builtin_amdgcn_readfirstlane((min(p.H - pr0, C::ROWS) + 15) >> 4);   // the row tiles that hold a head (1 .. 4)
    const int topk = p.topk;
    const int nt = (topk + C::KT - 1) / C::KT;
    const int t0 = (int)(((int64_t)nt * split) / p.ns), t1 = (int)(((int64_t)nt * (split + 1)) / p.ns);

    const int g0 = pr0 + wv * 16 + r;
    const bool row_ok = g0 < p.H;
    const int g = row_ok ? g0 : 0;
    bf16x8 qf[C::KS];
    {
        const __bf16* q = p.Q + b * p.qB + g * p.qH + qi * p.qS + 8 * h4;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            qf[ks] = __builtin_bit_cast(bf16x8, row_ok ? *reinterpret_cast<const u32x4*>(q + 32 * ks) : z);
        }
    }

    const char* const Kb = (const char*)p.K + (PAGED ? (int64_t)0 : b * p.kB);
    const int32_t* const ind = p.indices + b * p.isB + qi * p.isQ;
    const int32_t* const tb = p.block_table + (PAGED ? b * p.table_stride : 0);
    const int sl = lane & 31;   // the slot this lane carries through the stages (lanes s and s + 32 alike)
    const int rsl = PS * wv + (lane >> 3);   // the slot of this lane's rope chunk

    // the three stages of mla_sparse_kernel
    auto load_index = [&](int t) {
        const int s = t * C::KT + sl;
        return t < t1 && s < topk ? ind[s] : -1;
    };
    auto check = [&](int raw, int& pos, int& entry) {
        pos = raw >= 0 && raw < lim ? raw : -1;
        entry = 0;
        if constexpr (PAGED) {
            if (pos >= 0) entry = tb[pos >> p.page_shift];
        }
    };
    auto place = [&](int pos, int entry, uint32_t& olo, uint32_t& ohi) {
        int64_t off;
        if constexpr (PAGED) {
            const int page = min(max(entry, 0), p.num_pages - 1);
            off = (int64_t)page * p.kB + (int64_t)(pos & ((1 << p.page_shift) - 1)) * p.kS;
        } else {
            off = (int64_t)pos * p.kS;
        }
        if (pos < 0) off = 0;
        olo = (uint32_t)off; ohi = (uint32_t)((uint64_t)off >> 32);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)__ballot(pos >= 0));   // lanes 0 .. 31: one bit per slot
    };
    // the rows of a placed tile: the codes and the scale of load n (slot PS wave + n), the lane's rope chunk
    u32x2 kc[PS];
    float ksc[PS];
    u32x4 kr;
    auto load_tile = [&](uint32_t olo, uint32_t ohi, uint32_t valid) {
#pragma unroll
        for (int n = 0; n < PS; ++n) {
            const int s = PS * wv + n;                        // (wave-uniform: a scalar row base, a scalar branch)
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)olo, s), hi = (uint32_t)__builtin_amdgcn_readlane((int)ohi, s);
            const char* a = Kb + (int64_t)(((uint64_t)hi << 32) | lo);
            kc[n] = u32x2{0u, 0u};
            ksc[n] = 0.f;
            if ((valid >> s) & 1u) {
                kc[n] = *reinterpret_cast<const u32x2*>(a + R::CODES + 8 * lane);
                ksc[n] = *reinterpret_cast<const float*>(a + R::SCALES + 4 * h4);
            }
        }
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(rsl * 4, (int)olo);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(rsl * 4, (int)ohi);
        kr = u32x4{0u, 0u, 0u, 0u};
        if ((valid >> rsl) & 1u) kr = *reinterpret_cast<const u32x4*>(Kb + (int64_t)(((uint64_t)hi << 32) | lo) + R::ROPE + 16 * (lane & 7));
    };

    const int krd = r * C::LROW + h4 * 16;
    const int vrd = (4 * h4 + (r >> 2)) * C::LROW + wave * 256 + (lane & 3) * 8;
    const int pwr = C::P_OFF + (wave * 16 + r) * 64 + h4 * 16;
    const int prd = C::P_OFF + r * 64 + h4 * 16;
    FA_LDS float* al = reinterpret_cast<FA_LDS float*>(smem + C::AL_OFF);
    FA_LDS float* ll = reinterpret_cast<FA_LDS float*>(smem + C::L_OFF);

    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, l = 0.f;
    f32x4 o[4][C::DG];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg) o[rt][dg] = f32x4{0.f, 0.f, 0.f, 0.f};

    uint32_t valid = 0u, valid_next = 0u;
    int pos1 = -1, ent1 = 0, raw2 = -1;
    if (t0 < t1) {
        int pos0, ent0;
        uint32_t olo, ohi;
        check(load_index(t0), pos0, ent0);
        valid_next = place(pos0, ent0, olo, ohi);
        load_tile(olo, ohi, valid_next);
        check(load_index(t0 + 1), pos1, ent1);
        raw2 = load_index(t0 + 2);
    }
    for (int t = t0; t < t1; ++t) {
        // this tile: registers -> its buffer of the image, the scales applied here
        const lds_ptr img = smem + ((t - t0) & 1) * C::IMG;
#pragma unroll
        for (int n = 0; n < PS; ++n)
            lds_write_b128(img, (PS * wv + n) * C::LROW + 16 * lane, fp8x8_scaled_to_bf16x8(kc[n][0], kc[n][1], ksc[n]));
        lds_write_b128(img, rsl * C::LROW + 2 * C::DL + 16 * (lane & 7), kr);
        valid = valid_next;
        __syncthreads();
        if (t + 1 < t1) {
            uint32_t olo, ohi;
            valid_next = place(pos1, ent1, olo, ohi);
            load_tile(olo, ohi, valid_next);
            check(raw2, pos1, ent1);
            raw2 = load_index(t + 3);
        }

        if (wv < nrt) {
            f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
                for (int kg = 0; kg < 2; ++kg)
                    s[kg] = mfma_16x16x32(lds_read_b128(img, krd + kg * 16 * C::LROW + ks * 64), qf[ks], s[kg]);
            const uint32_t vq = valid >> (4 * h4);
            float x[8];
            float mx = NEG_INF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[j] = (vq >> (16 * (j >> 2) + (j & 3))) & 1u ? s[j >> 2][j & 3] * p.scale_log2 : NEG_INF;
                mx = fmaxf(mx, x[j]);
            }
            mx = max_all_quarters(mx);
            const float m_new = fmaxf(m, mx);
            const float m_use = m_new == NEG_INF ? 0.f : m_new;
            const float alpha = fast_exp2(m - m_use);
            m = m_new;
            float sum = 0.f;
            uint32_t whi[4], wlo[4];
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const float p0 = fast_exp2(x[j] - m_use), p1 = fast_exp2(x[j + 1] - m_use);
                sum += p0 + p1;
                whi[j >> 1] = pack_bf16(p0, p1);
                wlo[j >> 1] = pack_bf16(p0 - bf16_lo(whi[j >> 1]), p1 - bf16_hi(whi[j >> 1]));
            }
            l = l * alpha + sum;
            lds_write_b128(smem, pwr, u32x4{whi[0], whi[1], whi[2], whi[3]});
            lds_write_b128(smem, pwr + C::P_HALF, u32x4{wlo[0], wlo[1], wlo[2], wlo[3]});
            if (h4 == 0) al[wave * 16 + r] = alpha;
        }
        __syncthreads();

        bf16x8 phi[4], plo[4];
        float alpha[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            if (rt < nrt) {
                phi[rt] = lds_read_b128(smem, prd + rt * 1024);
                plo[rt] = lds_read_b128(smem, prd + rt * 1024 + C::P_HALF);
                alpha[rt] = al[rt * 16 + r];
            }
        }
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg) {
            const s16x4 a0 = lds_read_tr16_b64(img, vrd + dg * 32);
            const s16x4 a1 = lds_read_tr16_b64(img, vrd + 16 * C::LROW + dg * 32);
            typedef __attribute__((ext_vector_type(8))) short s16x8;
            const bf16x8 a = __builtin_bit_cast(bf16x8, s16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]});
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                if (rt < nrt) {
                    o[rt][dg] *= alpha[rt];
                    o[rt][dg] = mfma_16x16x32(a, phi[rt], o[rt][dg]);
                    o[rt][dg] = mfma_16x16x32(a, plo[rt], o[rt][dg]);
                }
            }
        }
    }

    __syncthreads();
    const float lr = sum_all_quarters(l);
    if (h4 == 0) {
        al[wave * 16 + r] = m;
        ll[wave * 16 + r] = lr;
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int oh = pr0 + rt * 16 + r;
        if (rt < nrt && oh < p.H) {
            const float M = al[rt * 16 + r], L = ll[rt * 16 + r];
            const float inv = M != NEG_INF ? 1.0f / L : 0.f;                                      // no key: O = 0
            const float lse = M != NEG_INF ? (M + __log2f(L)) * 0.6931471805599453f : NEG_INF;    // ... LSE = -inf
            const int64_t row = ((int64_t)b * p.H + oh) * Sq + qi;
            const int col = wave * 128 + 4 * h4;
            if (p.ns == 1) {
                const int64_t base = b * p.oB + oh * p.oH + qi * p.oS + col;
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

// decode_combine_kernel<512> (decode_bf16.hip.h) for rows that may have no key in any split: then every partial LSE is -inf, and the
// maximum is replaced by 0 in the weights' exponent -- exp(-inf - 0) = 0, never inf - inf -- so that O = 0 and LSE = -inf + ln 0 = -inf
// come out.  A row with a key takes the same steps in the same order as there.  (A template, so that only inst_mla_sparse.hip holds it)
template <int D>
__global__ __launch_bounds__(256) void mla_sparse_combine_kernel(const MlaSparseParams p) {
    constexpr int TPR = D / 4, SLOTS = 256 / TPR;
    __shared__ float wgt[WAVE];
    __shared__ f32x4 part[SLOTS][TPR];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float mine = lane < p.ns ? p.part_lse[(int64_t)lane * p.rows + row] : -__builtin_inff();
    float M = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
    const bool none = M == -__builtin_inff();
    const float w = __expf(mine - (none ? 0.f : M));
    float W = w;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) W += __shfl_xor(W, o);   // (a butterfly: the same sum, bit for bit, in every lane and wave)
    if (tid < WAVE) wgt[tid] = w;
    __syncthreads();
    const int c = tid % TPR, slot = tid / TPR;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = slot; s < p.ns; s += SLOTS)
        acc += wgt[s] * *reinterpret_cast<const f32x4*>(p.part_o + ((int64_t)s * p.rows + row) * D + 4 * c);
    part[slot][c] = acc;
    __syncthreads();
    if (tid >= TPR) return;
    f32x4 sum = part[0][c];
#pragma unroll
    for (int j = 1; j < SLOTS; ++j) sum += part[j][c];
    const float inv = none ? 0.f : 1.0f / W;
    const int oi = row % p.Sq, bh = row / p.Sq, oh = bh % p.H, b = bh / p.H;
    const int64_t base = b * p.oB + oh * p.oH + oi * p.oS + 4 * c;
#pragma unroll
    for (int j = 0; j < 4; ++j) store_out(p.O, p.o_dtype, base + j, sum[j] * inv);
    if (p.lse && c == 0) p.lse[row] = none ? -__builtin_inff() : M + __logf(W);
}

}  // namespace fa
