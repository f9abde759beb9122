// mla_sparse_prefill.hip.h -- the kernel of flash_attention_mla_sparse_prefill / _paged: sparse MLA attention for
// a RAGGED, token-major batch of any number of query tokens -- a prompt, a chunk of a chunked prefill, a mixed continuous-batching step.
// Per token the rule is flash_attention_mla_sparse_decode's (mla_sparse.hip.h) with the sequence's own row count:
//     O[tok, h] = softmax over the token's keys of (scale q . KV[p, :576]) KV[p, :512],   p = indices[tok, t], 0 <= p < lim
// From the LDS image on, a row tile of 16 heads is treated as mla_sparse_kernel treats it, statement for statement: the 32-slot tile, the
// padded 1184-byte row-major image read by rows for the scores and through ds_read_b64_tr_b16 for P.V, the three-stage index pipeline
// (raw, checked, placed) with the 32-bit validity word as the score mask, zeroed rows for the slots that are no key, hi + lo bf16
// weights, and the order of every accumulator's updates (o *= alpha; += V^T P_hi; += V^T P_lo, tile by tile) -- so a token's O and LSE
// are, bit for bit, what the decode call under one split returns for that token alone.  What differs is the work split:
//   * the work unit is (token, block of 128 HEADS), blockIdx = token * row_blocks + head block.  Every wave finds the token's sequence
//     by itself from cu_q, 64 sequences per step (lane i clamps the pair of sequence base + i as varlen_unit_of does; a ballot names the
//     owner).  A token no sequence owns -- every token at or beyond cu_q[B] -- leaves at once, the whole workgroup alike and before any
//     barrier: nothing of it is read or written.  The unit walks all ceil(topk / 32) slot tiles itself: no split, no slab, no combine;
//   * ONE image serves EIGHT row tiles: eight waves, two per SIMD, at most 256 registers each.  Wave w computes the scores and the
//     softmax of row tile w (72 registers of Q) and owns the columns [64 w, 64 w + 64) of O^T for all 128 heads (8 row tiles x 4 column
//     groups x 4 = 128 accumulators, in VGPR form as in the decode kernels).  A gathered row is fetched once per 128 heads where the
//     decode kernel fetches it once per 64, and the index pipeline and the image writes are paid once per 128 heads too;
//   * the fetch has a lane map of its own: a tile is 32 x 72 = 2304 chunks over 512 lanes -- load n of thread t is chunk 512 n + t,
//     n = 0 .. 3, and a fifth load, chunk 2048 + t, that the waves 0 .. 3 issue alone.  Chunk c is chunk c % 72 of slot c / 72, so a
//     wave instruction reads 1024 contiguous bytes of at most two rows.  Every wave holds the placed offsets of all 32 slots (lanes s
//     and s + 32), so the offsets come by ds_bpermute as there;
//   * the register budget (Q 72 + O 128 + the tile in flight 20 of 256) is closed by three things: the next tile is in flight under
//     the P.V product only -- gathered after the second barrier, written to the other image at the end of the step; the P.V product
//     holds two V^T fragments (8 registers) and reads the P^T fragments one row tile at a time (9 registers), not all at once (72);
//     and the first QL = 8 k-steps of Q live in LDS, a 16-byte slot per thread and k-step that only its thread touches (one
//     workgroup per CU has 64 KB to spare), the other 10 in registers.  No scratch in any form.
// Row tiles without a head are skipped by workgroup-uniform branches (nrt 1 .. 8), so one kernel serves every H.
#pragma once

#include "mla_sparse.hip.h"

namespace fa {

struct MlaSparsePrefillCfg {
    using C = MlaCfg;
    static constexpr int WAVES = 8, THREADS = 512;
    static constexpr int ROWS = 128;                          // heads per workgroup: one 16-row tile per wave
    static constexpr int DG = C::DL / 16 / WAVES;             // 16-wide column groups of O^T per wave
    static constexpr int CHUNKS = C::KT * C::CPR;             // chunks of a tile
    static constexpr int NLD = (CHUNKS + THREADS - 1) / THREADS;       // loads per lane and tile; the last by a part of the waves
    static constexpr int LAST_WAVES = (CHUNKS - (NLD - 1) * THREADS) / WAVE;
    static constexpr int P_OFF = 2 * C::IMG;                  // [hi, lo][row 128][quarter 4] 16-byte fragments of P^T
    static constexpr int P_HALF = ROWS * 64;
    static constexpr int AL_OFF = P_OFF + 2 * P_HALF;         // [row 128] rescale factor of the tile; at the end M
    static constexpr int L_OFF = AL_OFF + ROWS * 4;           // at the end: [row 128] L
    static constexpr int Q_OFF = L_OFF + ROWS * 4;            // [k-step QL][thread 512] 16-byte B fragments of Q^T: the thread's own
#ifdef FA_MLA_PREFILL_QL
    static constexpr int QL = FA_MLA_PREFILL_QL;
#else
    static constexpr int QL = 8;                              // k-steps of Q kept in LDS; the other C::KS - QL stay in registers
#endif
    static constexpr int LDS_BYTES = Q_OFF + QL * THREADS * 16;
    static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU: the CU's 160 KB of LDS");
    static_assert((CHUNKS - (NLD - 1) * THREADS) % WAVE == 0 && LAST_WAVES >= 1 && LAST_WAVES <= WAVES, "the last load is whole waves");
};

// MlaSparseParams filled as mla_run fills it for one split, the tensors packed by token: Sq holds totalQ, qS / oS are the token strides
// (qB / oB are not read), isQ the token stride of indices (isB is not read), rows = H * totalQ, row_blocks counts the blocks of 128
// heads, ns = 1
struct MlaSparsePrefillParams : MlaSparseParams {
    const int32_t* cu_q;          // [B + 1] (device memory): sequence b owns the tokens [cu_q[b], cu_q[b + 1]), clamped into [0, Sq]
    int B;
};

int mla_sparse_prefill_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparsePrefillParams& p);       // inst_mla_sparse_prefill.hip
int mla_sparse_prefill_fp8_launch(bool paged, unsigned grid, hipStream_t st, const MlaSparsePrefillParams& p);   // inst_mla_sparse_prefill_fp8.hip

template <bool PAGED, bool KV8 = false>
__global__ __launch_bounds__(512, 1) void mla_sparse_prefill_kernel(const MlaSparsePrefillParams p) {
    using C = MlaCfg;
    using F = MlaSparsePrefillCfg;
    constexpr int ES = KV8 ? 1 : 2;                           // bytes per cache element
    constexpr int CB = 8 * ES;                                // bytes of a fetched chunk: 8 elements
    typedef std::conditional_t<KV8, u32x2, u32x4> chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h4 = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(wave);

    // blockIdx -> (token, head block); the token's sequence b, its row qj of the sequence's sq rows
    const int hb = blockIdx.x % p.row_blocks;
    const int tok = blockIdx.x / p.row_blocks;
    int b = -1, qj = 0, sq = 0;
    for (int base = 0; base < p.B; base += WAVE) {
        const int s = min(base + lane, p.B - 1);
        const int q0 = min(max(p.cu_q[s], 0), p.Sq), q1 = min(max(p.cu_q[s + 1], q0), p.Sq);
        const unsigned long long hit = __ballot(base + lane < p.B && q0 <= tok && tok < q1);
        if (hit != 0) {
            const int l = __builtin_ctzll(hit);
            b = base + l;
            qj = tok - __builtin_amdgcn_readlane(q0, l);
            sq = __builtin_amdgcn_readlane(q1 - q0, l);
            break;
        }
    }
    if (b < 0) return;   // (uniform in the workgroup: every wave scans the same offsets)

    int len = p.Sk;
    if (p.kv_lens) len = min(max(p.kv_lens[b], 1), p.Sk);
    len = __builtin_amdgcn_readfirstlane(len);
    // the keys this token sees are the positions below lim (bottom-right aligned mask over the sequence's own rows, at least key 0)
    const int lim = p.causal ? max(len - sq + qj + 1, 1) : len;
    const int pr0 = hb * F::ROWS;
    const int nrt = __builtin_amdgcn_readfirstlane((min(p.H - pr0, F::ROWS) + 15) >> 4);   // the row tiles that hold a head (1 .. 8)
    const int topk = p.topk;
    const int nt = (topk + C::KT - 1) / C::KT;

    // this lane's row of the wave's row tile (column r of the swapped score product): head g of the token
    const int g0 = pr0 + wv * 16 + r;
    const bool row_ok = g0 < p.H;
    const int g = row_ok ? g0 : 0;
    // B fragments of Q^T: Q[row][32 ks + 8 h4 .. + 7]
    // The first QL k-steps live in LDS, each thread's fragments in a slot of its own (written and read by the same thread: no barrier),
    // the others in registers: 72 registers of Q beside 128 of O^T leave too few for the rest of the tile step
    bf16x8 qf[C::KS - F::QL];
    const int qoff = F::Q_OFF + tid * 16;
    {
        const __bf16* q = p.Q + tok * p.qS + g * p.qH + 8 * h4;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            const u32x4 v = row_ok ? *reinterpret_cast<const u32x4*>(q + 32 * ks) : z;
            if (ks < F::QL) lds_write_b128(smem, qoff + ks * F::THREADS * 16, v);
            else qf[ks - F::QL] = __builtin_bit_cast(bf16x8, v);
        }
    }

    // the fetch: load n of this thread is chunk 512 n + tid of the tile -- chunk ch of slot src; the last load by the first waves only
    // (the slot and the chunk are recomputed where they are used, from a thread index the compiler cannot see through: fifteen
    // registers less across the tile step)
    const int ksb = (int)(p.kS * ES);
    auto chunk_of = [&](int n, int& row, int& ch) {
        int tt = tid;
        asm volatile("" : "+v"(tt));
        const int c = F::THREADS * n + tt;
        row = c / C::CPR;                                         // the slot of the tile, and the lane that placed it
        ch = c - row * C::CPR;
    };
    const bool last_load = wv < F::LAST_WAVES;                    // (wave-uniform)
    const char* const Kb = (const char*)p.K + (PAGED ? (int64_t)0 : b * p.kB * ES);
    const int32_t* const ind = p.indices + tok * p.isQ;
    const int32_t* const tb = p.block_table + (PAGED ? b * p.table_stride : 0);
    const int sl = lane & 31;   // the slot this lane carries through the stages (lanes s and s + 32 alike)

    // stage 1: the raw index of slot sl of tile t; -1 where there is no slot
    auto load_index = [&](int t) {
        const int s = t * C::KT + sl;
        return t < nt && s < topk ? ind[s] : -1;
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
    chunk_t kn[F::NLD];
    // registers -> a buffer of the image
    auto store_tile = [&](lds_ptr img) {
#pragma unroll
        for (int n = 0; n < F::NLD; ++n) {
            if (n == F::NLD - 1 && !last_load) break;
            int row, ch;
            chunk_of(n, row, ch);
            const int loff = row * C::LROW + ch * 16;
            if constexpr (KV8) lds_write_b128(img, loff, fp8x8_to_bf16x8(kn[n][0], kn[n][1]));
            else lds_write_b128(img, loff, kn[n]);
        }
    };
    // the rows of a placed tile: every lane asks the placing lanes for the offsets of its loads
    auto load_tile = [&](uint32_t olo, uint32_t ohi, uint32_t valid) {
#pragma unroll
        for (int n = 0; n < F::NLD; ++n) {
            if (n == F::NLD - 1 && !last_load) break;
            int src, ch;
            chunk_of(n, src, ch);
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src * 4, (int)olo);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src * 4, (int)ohi);
            const char* a = Kb + (int64_t)(((uint64_t)hi << 32) | lo) + ch * CB;
            chunk_t v;
            if constexpr (KV8) v = u32x2{0u, 0u};
            else v = u32x4{0u, 0u, 0u, 0u};
            if ((valid >> src) & 1u) v = *reinterpret_cast<const chunk_t*>(a);
            kn[n] = v;
        }
    };

    // row read (kg, ks): key 16 kg + r of the tile, chunk 4 ks + h4.  Transposed read (dg, jj): lane 4 q + pp of quarter h4 supplies
    // row 16 jj + 4 h4 + q, columns 64 wave + 16 dg + 4 pp .. + 3
    const int krd = r * C::LROW + h4 * 16;
    const int vrd = (4 * h4 + (r >> 2)) * C::LROW + wave * 128 + (lane & 3) * 8;
    // P^T fragment of row `row`, quarter h4 (written by the row's wave, read by all eight); the row's rescale factor
    const int pwr = F::P_OFF + (wave * 16 + r) * 64 + h4 * 16;
    const int prd = F::P_OFF + r * 64 + h4 * 16;
    FA_LDS float* al = reinterpret_cast<FA_LDS float*>(smem + F::AL_OFF);
    FA_LDS float* ll = reinterpret_cast<FA_LDS float*>(smem + F::L_OFF);

    const float NEG_INF = -__builtin_inff();
    // KV8: the logical cache is KV8 * ds -- in the scores (here) and in the values (the normaliser, below)
    float ds = 1.f;
    if constexpr (KV8) ds = p.k_descale ? p.k_descale[0] : 1.f;
    const float sl2_ds = p.scale_log2 * ds;
    float m = NEG_INF, l = 0.f;   // of this lane's row: running max (log2 domain, shared by the row's four lanes), this lane's share of the sum
    f32x4 o[F::WAVES][F::DG];     // O^T: column 64 wave + 16 dg + 4 h4 + reg, head 16 rt + r of the block
#pragma unroll
    for (int rt = 0; rt < F::WAVES; ++rt)
#pragma unroll
        for (int dg = 0; dg < F::DG; ++dg) o[rt][dg] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the pipeline's state: the validity word of the tile in LDS and of the tile in flight; the checked tile; the raw tile
    uint32_t valid = 0u, valid_next = 0u;
    int pos1 = -1, ent1 = 0, raw2 = -1;
    {
        int pos0, ent0;
        uint32_t olo, ohi;
        check(load_index(0), pos0, ent0);
        valid_next = place(pos0, ent0, olo, ohi);
        load_tile(olo, ohi, valid_next);
        check(load_index(1), pos1, ent1);
        raw2 = load_index(2);
        store_tile(smem);
    }
    for (int t = 0; t < nt; ++t) {
        // this tile's buffer of the image was written at the end of the step before (tile 0: above)
        const lds_ptr img = smem + (t & 1) * C::IMG;
        valid = valid_next;
        __syncthreads();

        if (wv < nrt) {
            // S^T of the wave's row tile: s[kg][reg] = slot 32 t + 16 kg + 4 h4 + reg, head r
            f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks) {
                bf16x8 qk;
                if (ks < F::QL) qk = lds_read_b128(smem, qoff + ks * F::THREADS * 16);
                else qk = qf[ks - F::QL];
#pragma unroll
                for (int kg = 0; kg < 2; ++kg) s[kg] = mfma_16x16x32(lds_read_b128(img, krd + kg * 16 * C::LROW + ks * 64), qk, s[kg]);
            }
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
            lds_write_b128(smem, pwr + F::P_HALF, u32x4{wlo[0], wlo[1], wlo[2], wlo[3]});
            if (h4 == 0) al[wave * 16 + r] = alpha;
        }
        __syncthreads();
        // the next tile's rows: in flight under the P.V product only -- the score product has no registers left for them -- and its
        // offsets were checked a tile ago
        const bool more = t + 1 < nt;   // (uniform)
        if (more) {
            uint32_t olo, ohi;
            valid_next = place(pos1, ent1, olo, ohi);
            load_tile(olo, ohi, valid_next);
            check(raw2, pos1, ent1);        // tile t + 2 (paged: its table entries leave now)
            raw2 = load_index(t + 3);
        }

        // O^T += V^T P^T over the row tiles that hold a head, the wave's 64 columns, two column groups at a time.  A fragments of V^T
        // in the weights' key order: rows 4 h4 .. + 3 (j < 4), rows 16 + 4 h4 .. + 3 (j >= 4)
#pragma unroll
        for (int d0 = 0; d0 < F::DG; d0 += 2) {
            bf16x8 a[2];
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const s16x4 a0 = lds_read_tr16_b64(img, vrd + (d0 + d) * 32);
                const s16x4 a1 = lds_read_tr16_b64(img, vrd + 16 * C::LROW + (d0 + d) * 32);
                typedef __attribute__((ext_vector_type(8))) short s16x8;
                a[d] = __builtin_bit_cast(bf16x8, s16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]});
            }
#pragma unroll
            for (int rt = 0; rt < F::WAVES; ++rt) {
                if (rt < nrt) {
                    const bf16x8 phi = lds_read_b128(smem, prd + rt * 1024);
                    const bf16x8 plo = lds_read_b128(smem, prd + rt * 1024 + F::P_HALF);
                    const float alpha = al[rt * 16 + r];
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        o[rt][d0 + d] *= alpha;
                        o[rt][d0 + d] = mfma_16x16x32(a[d], phi, o[rt][d0 + d]);
                        o[rt][d0 + d] = mfma_16x16x32(a[d], plo, o[rt][d0 + d]);
                    }
                }
            }
        }
        // the next tile: registers -> the other buffer of the image, whose last readers are the P.V products of tile t - 1: every wave
        // left them before this step's first barrier
        if (more) store_tile(smem + ((t + 1) & 1) * C::IMG);
    }

    // ---- every row's (M, L) to LDS (the last tile's readers of the rescale factors must be through: one barrier), then each wave
    // normalises and writes its 64 columns of the heads that exist ----
    __syncthreads();
    const float lr = sum_all_quarters(l);
    if (h4 == 0) {
        al[wave * 16 + r] = m;
        ll[wave * 16 + r] = lr;
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < F::WAVES; ++rt) {
        const int oh = pr0 + rt * 16 + r;
        if (rt < nrt && oh < p.H) {
            const float M = al[rt * 16 + r], L = ll[rt * 16 + r];
            float inv = M != NEG_INF ? 1.0f / L : 0.f;                                            // no key: O = 0
            if constexpr (KV8) inv *= ds;
            const float lse = M != NEG_INF ? (M + __log2f(L)) * 0.6931471805599453f : NEG_INF;    // ... LSE = -inf
            const int64_t base = tok * p.oS + oh * p.oH + wave * 64 + 4 * h4;
#pragma unroll
            for (int dg = 0; dg < F::DG; ++dg)
#pragma unroll
                for (int j = 0; j < 4; ++j) store_out(p.O, p.o_dtype, base + 16 * dg + j, o[rt][dg][j] * inv);
            if (p.lse && wave == 0 && h4 == 0) p.lse[(int64_t)oh * p.Sq + tok] = lse;
        }
    }
}

}  // namespace fa
