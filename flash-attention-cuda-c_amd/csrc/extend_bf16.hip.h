// extend_bf16.hip.h -- chunked prefill against the decode K/V caches: seqLenQ new query rows per sequence, 1 .. the capacity, against
// the caches flash_attention_decode* reads, all four forms (flash_attention_extend, flash_attention_extend_paged; DESIGN.md
// section 19).
//
// The decode kernel (decode_bf16.hip.h) with RT 16-row tiles per wave where it has one.  Everything there holds here: the unit is
// (batch, K/V head, row block, key split) with packed row = g * seqLenQ + i; four waves take 32 keys each of a 128-key tile; the
// products are swapped, so the score registers are the B operand of P.V; K goes straight to its A fragment, V through the wave-private
// padded LDS image and ds_read_b64_tr_b16; descriptors hold this sequence's visible rows; the weights are a bf16 hi + lo pair; the
// paged form builds one descriptor per 16-key group and fetches its table entries two tiles ahead; fp8 is converted exactly in
// registers with k_descale on the score scale and v_descale on the final 1 / l.  What differs:
//   * a row block is 16 RT packed rows.  One K fragment and one transposed V read per d group feed RT MFMAs where they fed one: the
//     cache is read once per 16 RT rows, which is the point of the call.  The per-row state (Q fragments, m, l, O^T, the mask limit,
//     the weights and alpha) is an array over rt; every row's arithmetic is decode's, expression for expression, and a row of an MFMA
//     column depends on no other column, so for seqLenQ <= 16 the result is flash_attention_decode's bit for bit;
//   * a row block walks only the tiles one of its rows can see: ntb = ceil(max over its rows of lim / 128) tiles, divided over the
//     splits in whole tiles by decode's formula.  Under the causal mask the lower blocks of a long chunk read less.  A block of
//     seqLenQ <= 16 always holds a row with lim = len (its last row, or the last query row of a head), so ntb = nt there;
//   * the end-of-loop merge of the four waves runs once per rt through the same 16-row buffer (the wave's V image), two barriers
//     per rt: LDS stays at decode's size.
// No sliding window: DecodeParams::window is not read.
#pragma once

#include "decode_bf16.hip.h"

namespace fa {

// 16-row tiles per wave.  RT = 2 runs two workgroups per CU, RT = 4 one (its accumulators fill the register file); RT = 8 spills.
// Measured (profiles/extend_rt_sweep.log): at d = 128 RT = 4 with the MFMAs in VGPR form (the Makefile's flag on
// the inst_extend units) is 4 ... 17 % faster than RT = 2 behind a cached prefix and 16 % slower on a chunk with no prefix; at
// d = 64 the two are equal and RT = 2 keeps the occupancy.  FA_EXTEND_RT: a build-time override for such a comparison
template <int D>
struct ExtendCfg {
#ifdef FA_EXTEND_RT
    static constexpr int RT = FA_EXTEND_RT;
#else
    static constexpr int RT = D == 128 ? 4 : 2;
#endif
    static constexpr int ROWS = RT * DecodeCfg<D>::ROWS;   // packed rows per workgroup
    static constexpr int WGS_PER_CU = RT >= 4 ? 1 : 2;     // resident workgroups per CU: what the split rule fills
};

template <int D, int RT, bool PAGED, bool KV8 = false>
__global__ __launch_bounds__(256, RT <= 2 ? 2 : 1) void extend_split_kernel(const DecodeParams p) {
    constexpr int ES = KV8 ? 1 : 2;   // bytes per K/V element
    using KV = __attribute__((may_alias)) typename std::conditional<KV8, uint8_t, __bf16>::type;
    using C = DecodeCfg<D, ES>;
    constexpr int RPB = RT * C::ROWS;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h4 = lane >> 4;

    // blockIdx -> (batch, K/V head, row block, split); the split index runs fastest
    int u = blockIdx.x;
    const int split = u % p.ns; u /= p.ns;
    const int rb = u % p.row_blocks; u /= p.row_blocks;
    const int kvh = u % p.Hkv;
    const int b = u / p.Hkv;

    int len = p.Sk;
    if (p.kv_lens) len = min(max(p.kv_lens[b], 1), p.Sk);
    len = __builtin_amdgcn_readfirstlane(len);
    // the tiles this row block can see: below the largest limit of its rows.  Causal: the limit grows with the query row, and the
    // largest query row of the block is the last one -- unless the block reaches into the next head, then it holds a row Sq - 1
    const int nrows = p.G * p.Sq, pr0 = rb * RPB, prl = min(pr0 + RPB, nrows) - 1;
    const int gl = prl / p.Sq, qmax = pr0 / p.Sq != gl ? p.Sq - 1 : prl - gl * p.Sq;
    const int limb = p.causal ? max(len - p.Sq + qmax + 1, 1) : len;
    const int ntb = (limb + C::TILE - 1) / C::TILE;
    const int t0 = (int)(((int64_t)ntb * split) / p.ns), t1 = (int)(((int64_t)ntb * (split + 1)) / p.ns);

    // this lane's packed rows (column r of the swapped products, tile rt): query head g of the group, query row i; the keys the row
    // sees are [0, lim).  Bottom-right aligned mask: the Sq rows are the LAST rows of the sequence; at least key 0
    unsigned span[RT];
    // B fragments of Q^T: Q[row][32 ks + 8 h4 .. + 7].  KV8: Q[row][64 (ks / 2) + 16 h4 + 8 (ks % 2) .. + 7] (decode_bf16.hip.h)
    bf16x8 qf[RT][C::KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int pr = pr0 + rt * C::ROWS + r;
        const bool row_ok = pr < nrows;
        const int g = row_ok ? pr / p.Sq : 0, qi = row_ok ? pr - g * p.Sq : 0;
        const int h = kvh * p.G + g;
        const int limc = max(len - p.Sq + qi + 1, 1);
        span[rt] = (unsigned)(p.causal ? limc : len);
        const __bf16* q = p.Q + b * p.qB + h * p.qH + qi * p.qS + (KV8 ? 16 : 8) * h4;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            qf[rt][ks] = __builtin_bit_cast(bf16x8, row_ok ? *reinterpret_cast<const u32x4*>(q + (KV8 ? 64 * (ks >> 1) + 8 * (ks & 1) : 32 * ks)) : z);
        }
    }
    float scale_log2_kd = 0.f;
    if constexpr (KV8) scale_log2_kd = p.scale_log2 * (p.k_descale ? p.k_descale[kvh] : 1.f);

    // descriptors over the VISIBLE part of this (batch, K/V head): rows >= len read as 0 (contiguous form)
    const char* Kh = (const char*)((const KV*)p.K + b * p.kB + kvh * p.kH);
    const char* Vh = (const char*)((const KV*)p.V + b * p.vB + kvh * p.vH);
    const int ksb = (int)(p.kS * ES), vsb = (int)(p.vS * ES);
    const __amdgpu_buffer_rsrc_t krsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Kh, 0, (len - 1) * ksb + D * ES, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Vh, 0, (len - 1) * vsb + D * ES, 0x00020000);
    const int koff = (wave * C::WKEYS + r) * ksb + h4 * 16;
    const int vkey = lane / C::CPR, vch = lane % C::CPR;
    const int voff = (wave * C::WKEYS + vkey) * vsb + vch * 16;
    const lds_ptr vimg = smem + wave * C::VIMG;
    const int vwr = vkey * C::VROW + vch * (32 / ES);
    const int vrd = (4 * h4 + ((lane & 15) >> 2)) * C::VROW + (lane & 3) * 8;

    // paged form: decode's per-group descriptors and its table prefetch two tiles ahead (e0, e1: the entries of the tile whose loads
    // are issued next; ev, lane parity = group: in flight for the tile after it)
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int32_t* tb = p.block_table + b * p.table_stride;
    const int last_page = (len - 1) >> p.page_shift;
    const int gkoff = r * ksb + h4 * 16, gvoff = vkey * vsb + vch * 16;
    int ev = 0, e0 = 0, e1 = 0;
    // only pages that hold a key below the length are looked up (a tile past the end repeats the last one)
    auto table_entries = [&](int t) {
        const int key = t * C::TILE + wv * C::WKEYS + 16 * (lane & 1);
        return tb[min(key >> p.page_shift, last_page)];
    };
    auto next_entries = [&](int t) {
        e0 = __builtin_amdgcn_readlane(ev, 0);
        e1 = __builtin_amdgcn_readlane(ev, 1);
        ev = table_entries(t);
    };
    // one 16-key group of one pool: a descriptor at its first row, holding its rows below len
    auto group_rsrc = [&](const __bf16* pool, int64_t page_stride, int64_t head_stride, int64_t row_stride, int entry, int key) {
        const int page = min(max(entry, 0), p.num_pages - 1);
        const KV* base = (const KV*)pool + page * page_stride + kvh * head_stride + (key & ((1 << p.page_shift) - 1)) * row_stride;
        const int rows = min(len - key, 16);
        const int bytes = rows > 0 ? (rows - 1) * (int)(row_stride * ES) + D * ES : 0;
        const uint64_t a = (uint64_t)base;
        const uint64_t au = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
        return __builtin_amdgcn_make_buffer_rsrc((void*)au, 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
    };
    u32x4 kn[2][C::KL], vn[C::NV];
    auto load_tile = [&](int t) {
        if constexpr (!PAGED) {
            const int kt = t * C::TILE * ksb, vt = t * C::TILE * vsb;
#pragma unroll
            for (int kg = 0; kg < 2; ++kg)
#pragma unroll
                for (int ks = 0; ks < C::KL; ++ks)
                    kn[kg][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krsrc, koff + kt + kg * 16 * ksb + ks * 64, 0, 0));
#pragma unroll
            for (int n = 0; n < C::NV; ++n)
                vn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vrsrc, voff + vt + n * C::KPI * vsb, 0, 0));
        } else {
            __amdgpu_buffer_rsrc_t kr[2], vr[2];
#pragma unroll
            for (int kg = 0; kg < 2; ++kg) {
                const int entry = kg ? e1 : e0, key = t * C::TILE + wv * C::WKEYS + 16 * kg;
                kr[kg] = group_rsrc(p.K, p.kB, p.kH, p.kS, entry, key);
                vr[kg] = group_rsrc(p.V, p.vB, p.vH, p.vS, entry, key);
            }
#pragma unroll
            for (int kg = 0; kg < 2; ++kg)
#pragma unroll
                for (int ks = 0; ks < C::KL; ++ks)
                    kn[kg][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(kr[kg], gkoff + ks * 64, 0, 0));
#pragma unroll
            for (int n = 0; n < C::NV; ++n)   // (V load n covers the keys KPI n .. KPI n + KPI - 1 of the wave's 32: one group)
                vn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vr[n * C::KPI / 16], gvoff + (n * C::KPI % 16) * vsb, 0, 0));
        }
    };

    const float NEG_INF = -__builtin_inff();
    float m[RT], l[RT];   // per tile rt: running max (log2 domain, shared by the row's four lanes), this lane's share of the sum
    f32x4 o[RT][C::DG];   // O^T: d = 16 dg + 4 h4 + reg, packed row r of tile rt
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        m[rt] = NEG_INF;
        l[rt] = 0.f;
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg) o[rt][dg] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    if (t0 < t1) {
        if constexpr (PAGED) {
            ev = table_entries(t0);
            next_entries(t0 + 1);
        }
        load_tile(t0);
    }
    for (int t = t0; t < t1; ++t) {
        // V of this tile: registers -> the wave's LDS image (the previous tile's reads are done: same wave, program order)
#pragma unroll
        for (int n = 0; n < C::NV; ++n) {
            if constexpr (!KV8) lds_write_b128(vimg, vwr + n * C::KPI * C::VROW, vn[n]);
            else {   // 16 e4m3fn bytes -> 16 bf16, exactly: the image is the bf16 form's
                lds_write_b128(vimg, vwr + n * C::KPI * C::VROW, fp8x8_to_bf16x8(vn[n][0], vn[n][1]));
                lds_write_b128(vimg, vwr + n * C::KPI * C::VROW + 16, fp8x8_to_bf16x8(vn[n][2], vn[n][3]));
            }
        }
        // one K fragment feeds the RT row tiles
        f32x4 s[RT][2];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) s[rt][0] = s[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
            if constexpr (!KV8) {
#pragma unroll
                for (int ks = 0; ks < C::KS; ++ks) {
                    const bf16x8 a = __builtin_bit_cast(bf16x8, kn[kg][ks]);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) s[rt][kg] = mfma_16x16x32(a, qf[rt][ks], s[rt][kg]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < C::KL; ++c) {   // a 16-byte load = the A fragments of two k-groups, in the d order of qf
                    const bf16x8 a0 = __builtin_bit_cast(bf16x8, fp8x8_to_bf16x8(kn[kg][c][0], kn[kg][c][1]));
                    const bf16x8 a1 = __builtin_bit_cast(bf16x8, fp8x8_to_bf16x8(kn[kg][c][2], kn[kg][c][3]));
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        s[rt][kg] = mfma_16x16x32(a0, qf[rt][2 * c], s[rt][kg]);
                        s[rt][kg] = mfma_16x16x32(a1, qf[rt][2 * c + 1], s[rt][kg]);
                    }
                }
            }
        }
        if (t + 1 < t1) {   // (wave-uniform) next tile's K and V: in flight under the softmax and the P.V product
            if constexpr (PAGED) next_entries(t + 2);   // tile t + 1's entries arrived with the K/V of tile t: issued before them
            load_tile(t + 1);
        }

        // s[rt][kg][reg]: key kb + 16 kg + reg, packed row r of tile rt
        const int kb = t * C::TILE + wave * C::WKEYS + 4 * h4;
        bf16x8 phi[RT], plo[RT];
        float alpha[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float x[8];
            float mx = NEG_INF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned rel = (unsigned)(kb + 16 * (j >> 2) + (j & 3));
                x[j] = rel < span[rt] ? s[rt][j >> 2][j & 3] * (KV8 ? scale_log2_kd : p.scale_log2) : NEG_INF;
                mx = fmaxf(mx, x[j]);
            }
            mx = max_all_quarters(mx);
            const float m_new = fmaxf(m[rt], mx);
            const float m_use = m_new == NEG_INF ? 0.f : m_new;   // nothing visible yet: exp2(-inf - 0) = 0, never inf - inf
            alpha[rt] = fast_exp2(m[rt] - m_use);
            m[rt] = m_new;
            float sum = 0.f;
            uint32_t hi[4], lo[4];
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const float p0 = fast_exp2(x[j] - m_use), p1 = fast_exp2(x[j + 1] - m_use);
                sum += p0 + p1;
                // weights as a bf16 pair: hi = bf16(p), lo = bf16(p - hi) -- 16 significant bits between them
                hi[j >> 1] = pack_bf16(p0, p1);
                lo[j >> 1] = pack_bf16(p0 - bf16_lo(hi[j >> 1]), p1 - bf16_hi(hi[j >> 1]));
            }
            l[rt] = l[rt] * alpha[rt] + sum;
            // B fragment of P^T: element j of quarter h4 = the MFMA's k index 8 h4 + j = key 16 (j >> 2) + 4 h4 + (j & 3)
            phi[rt] = __builtin_bit_cast(bf16x8, u32x4{hi[0], hi[1], hi[2], hi[3]});
            plo[rt] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], lo[2], lo[3]});
        }
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg) {
            // A fragment of V^T in that key order, read once for the RT tiles: rows 4 h4 .. + 3 (j < 4), rows 16 + 4 h4 .. + 3 (j >= 4)
            const s16x4 a0 = lds_read_tr16_b64(vimg, vrd + dg * 32);
            const s16x4 a1 = lds_read_tr16_b64(vimg, vrd + 16 * C::VROW + dg * 32);
            typedef __attribute__((ext_vector_type(8))) short s16x8;
            const bf16x8 a = __builtin_bit_cast(bf16x8, s16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]});
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                o[rt][dg] *= alpha[rt];
                o[rt][dg] = mfma_16x16x32(a, phi[rt], o[rt][dg]);
                o[rt][dg] = mfma_16x16x32(a, plo[rt], o[rt][dg]);
            }
        }
    }

    // ---- merge the four waves' (m, l, O^T) through LDS, one 16-row tile at a time: each wave writes the tile into its own V image,
    // every thread sums one row's share over the waves; the second barrier keeps the next tile's writes behind these reads ----
    FA_LDS float* ml = reinterpret_cast<FA_LDS float*>(smem + C::ML_OFF);
    constexpr int DPT = D / 16;   // thread -> packed row tid / 16 of the tile, DPT consecutive d
    const int orow = tid >> 4, d0 = (tid & 15) * DPT;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        if (rt > 0) __syncthreads();
        const float lr = sum_all_quarters(l[rt]);
        if (h4 == 0) {
            ml[wave * C::ROWS + r] = m[rt];
            ml[(C::WAVES + wave) * C::ROWS + r] = lr;
        }
#pragma unroll
        for (int dg = 0; dg < C::DG; ++dg)
            *reinterpret_cast<FA_LDS f32x4*>(vimg + r * C::OROW + (16 * dg + 4 * h4) * 4) = o[rt][dg];
        __syncthreads();

        float M = NEG_INF;
#pragma unroll
        for (int w = 0; w < C::WAVES; ++w) M = fmaxf(M, ml[w * C::ROWS + orow]);
        float L = 0.f, acc[DPT];
#pragma unroll
        for (int j = 0; j < DPT; ++j) acc[j] = 0.f;
        if (M != NEG_INF) {
#pragma unroll
            for (int w = 0; w < C::WAVES; ++w) {
                const float wgt = fast_exp2(ml[w * C::ROWS + orow] - M);   // a wave that saw nothing: exp2(-inf) = 0
                L += wgt * ml[(C::WAVES + w) * C::ROWS + orow];
                FA_LDS const float* src = reinterpret_cast<FA_LDS const float*>(smem + w * C::VIMG + orow * C::OROW) + d0;
#pragma unroll
                for (int j = 0; j < DPT; ++j) acc[j] += wgt * src[j];
            }
        }
        const int opr = pr0 + rt * C::ROWS + orow;
        if (opr < nrows) {   // (no early exit: the barriers of the tiles to come are the whole workgroup's)
            const int og = opr / p.Sq, oi = opr - og * p.Sq, oh = kvh * p.G + og;
            float inv = M != NEG_INF ? 1.0f / L : 0.f;                                         // empty split: O = 0
            if constexpr (KV8) inv *= p.v_descale ? p.v_descale[kvh] : 1.f;                    // V = V8 * v_descale: once, on the normalised sum
            const float lse = M != NEG_INF ? (M + __log2f(L)) * 0.6931471805599453f : NEG_INF;   // ... LSE = -inf
            const int64_t row = ((int64_t)b * p.H + oh) * p.Sq + oi;
            if (p.ns == 1) {
                const int64_t base = b * p.oB + oh * p.oH + oi * p.oS + d0;
#pragma unroll
                for (int j = 0; j < DPT; ++j) store_out(p.O, p.o_dtype, base + j, acc[j] * inv);
                if (p.lse && (tid & 15) == 0) p.lse[row] = lse;
            } else {
                float* dst = p.part_o + ((int64_t)split * p.rows + row) * D + d0;
#pragma unroll
                for (int j = 0; j < DPT; ++j) dst[j] = acc[j] * inv;
                if ((tid & 15) == 0) p.part_lse[(int64_t)split * p.rows + row] = lse;
            }
        }
    }
}

// ---- selectors (inst_extend_bf16.hip, inst_extend_paged_bf16.hip, inst_extend_fp8.hip, inst_extend_paged_fp8.hip) ----
struct Kernel;
Kernel extend_split_kernel_of(int d);
Kernel extend_paged_split_kernel_of(int d);
Kernel extend_fp8_split_kernel_of(int d);
Kernel extend_paged_fp8_split_kernel_of(int d);

}  // namespace fa
