// mla_index.hip.h -- the two kernels of flash_attention_mla_index_topk / _paged: the sparse-attention INDEXER of
// DeepSeek-V3.2 in the model's own fp8 form, the producer of the `indices` flash_attention_mla_sparse_decode* consumes.
//     logit[b, i, k] = kScale[b, k] * sum_{h < 64} W[b, i, h] * max(0, sum_{d < 128} Qidx[b, i, h, d] * Kidx[b, k, d]),   k < lim_i
//     indices[b, i, :] = the min(topk, lim_i) positions of the largest logits, ties to the lower position, ascending, then -1
// lim_i is the sparse call's: len_b (kvLens clamped into [1, capacity]) or, under the mask, max(len_b - Sq + i + 1, 1).
//
// Kernel 1, mla_index_logits_kernel: memory-bound (132 bytes per token), built to read the index cache ONCE per sequence whatever Sq is.
//   * a workgroup of four waves owns KB = 256 consecutive keys of one sequence, a wave 64 of them as NT = 2 tiles of 32.  A workgroup
//     whose first key is at or beyond len_b -- the largest lim_i -- leaves before any load; a key at or beyond len_b is not read at all
//     (its lane re-reads key len_b - 1), so neither rows nor scales nor, paged, table entries beyond the length are touched;
//   * a tile's K rows go from global memory straight into registers as the B operand of the block-scaled
//     v_mfma_scale_f32_32x32x64_f8f6f4 (unit scales; twice the rate of the 32x32x16 fp8 form, which at Sq >= 3 would bound the kernel):
//     keys are the accumulator's columns.  The instruction pairs byte j of lane half h of A with byte j of lane half h of B, so the
//     contraction order is free: lane (r, h) takes bytes [64 h, 64 h + 64) of key r's row -- four 16-byte loads, 16 VGPRs per tile, no
//     LDS -- and product s = 0, 1 contracts its bytes [32 s, 32 s + 32);
//   * the 64 heads of a query row are two A tiles, heads the accumulator's rows: Qidx of up to QC = 4 query rows and their W are staged
//     in LDS once per workgroup (head rows padded to 144 bytes: the 16-byte reads of 16 lanes fall into distinct banks), lane (r, h)
//     reading bytes [64 h, 64 h + 64) of head 32 t + r.  The wave loops over the query rows with K held in registers;
//   * ReLU, the multiply by W[h] and the sum over heads run over a lane's 16 accumulator registers (rows 8 g + 4 h + j of the tile, W
//     read as four 16-byte LDS words), then one exchange between the lane halves; no reduction across keys.  Every sum is a chain of
//     fmaf in one fixed order, so the paged form equals the contiguous one bit for bit.  -0 is stored as +0.
// Kernel 2, mla_index_topk_kernel: one workgroup of 1024 threads per (b, i) row, a radix select on the order-preserving 32-bit image of
//   the fp32 logit -- 11 + 11 + 10 bits, LDS histograms (LDS atomics only), a suffix scan over the bins -- that finds the threshold value T
//   and how many entries equal to T are admitted; then ONE ordered emit pass: chunks of 1024 positions in position order, a ballot and
//   a prefix count over the workgroup give every admitted position its slot, which makes the ascending order and the lower-position tie
//   rule hold without sorting anything.  lim_i <= topk: no passes, the row is 0 .. lim_i - 1 and the -1 tail.  No global atomics.
#pragma once

#include "launchers.hip.h"
#include "utils.hip.h"

namespace fa {

struct MlaIndexCfg {
    static constexpr int HEADS = 64, D = 128;
    static constexpr int THREADS = 256, NT = 2, KB = 4 * NT * 32;     // kernel 1: keys per workgroup
    static constexpr int QC = 4;                                       // query rows staged at a time
    static constexpr int HROW = D + 16;                                // bytes of a padded head row in LDS
    static constexpr int QROW = HEADS * HROW;                          // ... of a query row
    static constexpr int W_OFF = QC * QROW;
    static constexpr int LDS_BYTES = W_OFF + QC * HEADS * 4;           // 37 888
    static constexpr int SEL_THREADS = 1024, BINS = 2048;              // kernel 2
};

struct MlaIndexParams {
    const uint8_t* Q;             // [B, Sq, 64, 128] e4m3fn
    const float* W;               // [B, Sq, 64]
    const uint8_t* K;             // [B, capacity, 128] e4m3fn; paged: the pool [P, page, 128]
    const float* k_scale;         // [B, capacity]; paged: [P, page]
    const int32_t* kv_lens;       // [B] or NULL
    const int32_t* block_table;   // paged: [B, table_stride]
    float* logits;                // [B, Sq, ls]
    int32_t* indices;             // [B, Sq, topk], element strides isB, isQ
    int64_t table_stride, ls, isB, isQ;
    int Sq, cap, topk, num_pages, page_shift, causal, key_blocks;
};

int mla_index_launch(bool paged, unsigned grid, unsigned rows, hipStream_t st, const MlaIndexParams& p);   // inst_mla_index.hip

__device__ __forceinline__ int mla_index_len(const MlaIndexParams& p, int b) {
    int len = p.cap;
    if (p.kv_lens) len = min(max(p.kv_lens[b], 1), p.cap);
    return __builtin_amdgcn_readfirstlane(len);
}

template <bool PAGED>
__global__ __launch_bounds__(256) void mla_index_logits_kernel(const MlaIndexParams p) {
    using C = MlaIndexCfg;
    __shared__ __attribute__((aligned(16))) char smem_raw[C::LDS_BYTES];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / p.key_blocks;
    const int k0 = (blockIdx.x - b * p.key_blocks) * C::KB;
    const int len = mla_index_len(p, b);
    if (k0 >= len) return;   // (uniform) no query row of the sequence sees a key of this block
    const int Sq = p.Sq;

    // the wave's keys: tile n holds key kw + 32 n + r in column r.  A key at or beyond len is replaced by len - 1 in every address
    const int kw = k0 + wv * (C::NT * 32);
    const bool active = kw < len;
    u32x4 kf[C::NT][4];
    float ks[C::NT];
    if (active) {
#pragma unroll
        for (int n = 0; n < C::NT; ++n) {
            const int kk = min(kw + 32 * n + r, len - 1);
            int64_t row;
            if constexpr (PAGED) {
                const int entry = p.block_table[b * p.table_stride + (kk >> p.page_shift)];
                const int page = min(max(entry, 0), p.num_pages - 1);
                row = ((int64_t)page << p.page_shift) + (kk & ((1 << p.page_shift) - 1));
            } else {
                row = (int64_t)b * p.cap + kk;
            }
            const u32x4* src = reinterpret_cast<const u32x4*>(p.K + row * C::D + 64 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) kf[n][c] = __builtin_nontemporal_load(src + c);
            ks[n] = p.k_scale[row];
        }
    }

    for (int c0 = 0; c0 < Sq; c0 += C::QC) {
        const int nq = min(C::QC, Sq - c0);
        if (c0) __syncthreads();   // the previous rows' readers are through
        // Qidx of rows c0 .. c0 + nq - 1: 512 chunks of 16 bytes per row, chunk c = 8 head + part; their W
        const u32x4* qsrc = reinterpret_cast<const u32x4*>(p.Q + ((int64_t)b * Sq + c0) * (C::HEADS * C::D));
        for (int c = tid; c < nq * 512; c += C::THREADS) {
            const int qi = c >> 9, cc = c & 511;
            *reinterpret_cast<FA_LDS u32x4*>(smem + qi * C::QROW + (cc >> 3) * C::HROW + (cc & 7) * 16) = qsrc[c];
        }
        const float* wsrc = p.W + ((int64_t)b * Sq + c0) * C::HEADS;
        for (int c = tid; c < nq * C::HEADS; c += C::THREADS) reinterpret_cast<FA_LDS float*>(smem + C::W_OFF)[c] = wsrc[c];
        __syncthreads();
        if (!active) continue;
        for (int qi = 0; qi < nq; ++qi) {
            const int i = c0 + qi;
            const int lim = p.causal ? max(len - Sq + i + 1, 1) : len;
            if (kw >= lim) continue;   // (uniform in the wave)
            float part[C::NT];
#pragma unroll
            for (int n = 0; n < C::NT; ++n) part[n] = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int qa = qi * C::QROW + (32 * t + r) * C::HROW + 64 * h;
                u32x4 a[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) a[c] = *reinterpret_cast<FA_LDS const u32x4*>(smem + qa + 16 * c);
                // W of the rows this lane's accumulator registers hold: heads 32 t + 8 g + 4 h + (0 .. 3)
                f32x4 w[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    w[g] = *reinterpret_cast<FA_LDS const f32x4*>(smem + C::W_OFF + (qi * C::HEADS + 32 * t + 8 * g + 4 * h) * 4);
#pragma unroll
                for (int n = 0; n < C::NT; ++n) {
                    f32x16 acc;
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
                    acc = mfma_32x32x64_fp8_unit_scale(a[0], a[1], kf[n][0], kf[n][1], acc);
                    acc = mfma_32x32x64_fp8_unit_scale(a[2], a[3], kf[n][2], kf[n][3], acc);
#pragma unroll
                    for (int j = 0; j < 16; ++j) part[n] = __builtin_fmaf(fmaxf(acc[j], 0.f), w[j >> 2][j & 3], part[n]);
                }
            }
            float* out = p.logits + ((int64_t)b * Sq + i) * p.ls;
#pragma unroll
            for (int n = 0; n < C::NT; ++n) {
                const float x = (part[n] + other_half(part[n])) * ks[n];
                const int key = kw + 32 * n + r;
                if (h == 0 && key < lim) out[key] = x == 0.f ? 0.f : x;   // (-0 -> +0)
            }
        }
    }
}

// the order-preserving image of an fp32: a > b (as numbers) <=> image(a) > image(b); +0 above -0, NaNs at the two ends
__device__ __forceinline__ uint32_t mla_index_image(float x) {
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// (a template, so that only inst_mla_index.hip holds it)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void mla_index_topk_kernel(const MlaIndexParams p) {
    using C = MlaIndexCfg;
    static_assert(THREADS == C::SEL_THREADS && C::BINS == 2 * THREADS && THREADS == 16 * WAVE, "two bins per thread, sixteen waves");
    __shared__ int hist[C::BINS];
    __shared__ int wsum[2][16];
    __shared__ int sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / p.Sq, i = blockIdx.x - b * p.Sq;
    const int len = mla_index_len(p, b);
    const int lim = p.causal ? max(len - p.Sq + i + 1, 1) : len;
    const int topk = p.topk;
    const float* row = p.logits + (int64_t)blockIdx.x * p.ls;
    int32_t* out = p.indices + b * p.isB + i * p.isQ;

    if (lim <= topk) {   // (uniform) every visible position, then the tail
        for (int s = tid; s < topk; s += C::SEL_THREADS) out[s] = s < lim ? s : -1;
        return;
    }

    // ---- the threshold: after the three passes `prefix` is the image T of the topk-th largest logit and `need` (>= 1) the number of
    // entries equal to T that are admitted; every entry above T is ----
    uint32_t prefix = 0;
    int need = topk;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int sh = pass == 0 ? 21 : pass == 1 ? 10 : 0;         // the pass's digit: bits [sh, top)
        const int top = pass == 0 ? 32 : pass == 1 ? 21 : 10;
        const uint32_t mask = (1u << (top - sh)) - 1u;
        hist[2 * tid] = 0; hist[2 * tid + 1] = 0;
        __syncthreads();
#pragma unroll 4
        for (int k = tid; k < lim; k += C::SEL_THREADS) {
            const uint32_t u = mla_index_image(row[k]);
            if (pass == 0 || (u >> top) == (prefix >> top)) atomicAdd(&hist[(u >> sh) & mask], 1);   // (an LDS atomic)
        }
        __syncthreads();
        // suffix sums over the bins: this thread owns bins 2 tid and 2 tid + 1; `above` = the count in the bins above both
        const int h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
        int v = h0 + h1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(v, o);
            if (lane + o < 64) v += t;
        }
        if (lane == 0) wsum[0][wave] = v;
        __syncthreads();
        int above = v - (h0 + h1);
        for (int w = wave + 1; w < 16; ++w) above += wsum[0][w];
        // the one bin d with count(bins > d) < need <= count(bins >= d)
        if (above < need && need <= above + h1) { sel[0] = 2 * tid + 1; sel[1] = need - above; }
        else if (above + h1 < need && need <= above + h1 + h0) { sel[0] = 2 * tid; sel[1] = need - above - h1; }
        __syncthreads();
        prefix |= (uint32_t)sel[0] << sh;
        need = sel[1];
    }

    // ---- the ordered emit: chunks of 1024 positions in position order.  g / e: the entry is above / equal to T; one packed count
    // (g in the high half, e in the low: a chunk holds at most 1024 of either) is scanned over the workgroup, and the e-th equal entry
    // of the row is admitted iff e < need ----
    int out_base = 0, eq_base = 0;   // admitted entries / entries equal to T before this chunk
    for (int k0 = 0, it = 0; k0 < lim && out_base < topk; k0 += C::SEL_THREADS, ++it) {
        const int k = k0 + tid;
        uint32_t u = 0;
        if (k < lim) u = mla_index_image(row[k]);
        const bool g = k < lim && u > prefix, e = k < lim && u == prefix;
        const uint64_t bg = __ballot(g), be = __ballot(e);
        const uint64_t below = ((uint64_t)1 << lane) - 1;
        int g_before = __popcll(bg & below), e_before = __popcll(be & below);
        if (lane == 0) wsum[it & 1][wave] = (__popcll(bg) << 16) | __popcll(be);
        __syncthreads();
        int g_all = 0, e_all = 0;
        for (int w = 0; w < 16; ++w) {
            const int c = wsum[it & 1][w];
            if (w < wave) { g_before += c >> 16; e_before += c & 0xffff; }
            g_all += c >> 16; e_all += c & 0xffff;
        }
        const int e_rank = eq_base + e_before;                              // equal entries of the row before this one
        const int slot = out_base + g_before + min(e_rank, need) - min(eq_base, need);
        if (g || (e && e_rank < need)) out[slot] = k;
        out_base += g_all + min(eq_base + e_all, need) - min(eq_base, need);
        eq_base += e_all;
    }
}

}  // namespace fa
