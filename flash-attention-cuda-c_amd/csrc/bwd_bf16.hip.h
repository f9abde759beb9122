// bwd_bf16.hip.h -- the attention backward pass (dQ, dK, dV) for bf16 Q, K, V at D = 64 / 128 (include/flash_attention.h:
// flash_attention_backward).  P is recomputed from Q, K and the forward's LSE; three launches:
//
//   1. bwd_pre_kernel   one pass over the query rows: delta = rowsum(dO * O) (fp32, workspace) and the fp32 dQ accumulator
//                       (workspace) zeroed -- it stands where a memset node would, so a captured graph stays one chain of kernels.
//   2. bwd_main_kernel  one workgroup = 4 waves = one block of 256 keys of one (b, K/V head); wave w owns keys 64w .. 64w+63 of the
//                       block and keeps dV^T and dK^T of those keys in registers for the whole sweep over the query rows, in 32-row
//                       slices (under the causal mask from the first slice that sees the block), of the G query heads that share the
//                       K/V head, one head after the other (grouped-query attention; G = 1: the head itself) -- so dK and dV are
//                       the group's sum, written once, by one workgroup: no cross-workgroup sum, bitwise reproducible.  Per slice,
//                       five 32x32x16 MFMA products:
//                         S'  = Q K^T  - LSE/scale     (accumulator seeded with the row constant: p = exp2(c S'), c = scale log2 e,
//                         dP' = dO V^T - delta          needs no subtraction and no row maximum)
//                         dV^T += dO^T P,   dK^T += Q^T dS   (dS = P * dP')
//                         dQ   += dS K
//                       S and dP are computed with the KEY on the MFMA lane, so their accumulators, packed to bf16, are already the B
//                       operands of the dV^T / dK^T products (cdna_hip_programming section 3, "An accumulator tile as the next MFMA's
//                       operand"); dO^T and Q^T come from the same LDS images by hardware-transposed reads (ds_read_b64_tr_b16).
//                       dS crosses LDS once, as a [key][query] image; each wave then computes dQ for a quarter of the head columns
//                       over all 256 keys and adds it with no-return fp32 atomics into the accumulator (a quarter of the atomic
//                       bytes of four 64-key partial sums).
//   3. bwd_post_kernel  dQ = scale * accumulator, converted to the gradient type, written through the caller's strides.
//
// LDS images (rows padded by 16 bytes): K [256 keys][D] (rows for S, columns for dQ), Q and dO [32 rows][D] (rows for S / dP,
// columns for dK^T / dV^T), dS^T [256 keys][32 rows], the slice's two row constants.  V lives in registers (the wave's 64 keys).
#pragma once

#include "utils.hip.h"

namespace fa {

// Kernel arguments.  Strides in elements (last dimension contiguous); the workspace arrays are dense.
struct BwdParams {
    const __bf16* Q;
    const __bf16* K;
    const __bf16* V;
    const void* O;        // o_dtype
    const void* dO;       // o_dtype
    const float* lse;     // dense [B, H, Sq], natural log
    void* dQ;             // grad_dtype
    void* dK;
    void* dV;
    float* delta;         // workspace: [B*H*Sq]
    float* dq_acc;        // workspace: [B*H*Sq][D]
    int64_t qB, qH, qS, kB, kH, kS, vB, vH, vS, oB, oH, oS, doB, doH, doS;
    int64_t dqB, dqH, dqS, dkB, dkH, dkS, dvB, dvH, dvS;
    int H, Sq, Sk;        // H: query heads
    int heads;            // B * H
    int Hkv, group;       // K/V heads; group = H / Hkv query heads share each: query head h reads K/V head h / group
    int kv_heads;         // B * Hkv
    int nK;               // 256-key blocks per head
    float scale;
    float inv_scale;      // 1 / scale: the S accumulator is seeded with -LSE / scale
    float c;              // scale * log2(e)
};

// Under the causal mask the key blocks are launched heaviest first (block 0 of every K/V head, then block 1, ...): 3.53 ms against 5.9 ms
// with a head's blocks adjacent at B 8 H 16 S 4096 d 128 (profiles/r05_backward_causal_order_ab.log; head-major ends on the heavy
// blocks of the last heads).  Without the mask a head's blocks are adjacent, so they share the head's Q and dO in L2.
#ifndef FA_BWD_HEAVY_FIRST
#define FA_BWD_HEAVY_FIRST 1
#endif

template <int D>
struct BwdCfg {
    static constexpr int ROW = D * 2 + 16;           // Q / dO / K image row (bytes)
    static constexpr int SROW = 32 * 2 + 16;         // dS^T image row: the 32 query rows of one key
    static constexpr int K_OFF = 0;
    static constexpr int Q_OFF = K_OFF + 256 * ROW;
    static constexpr int DO_OFF = Q_OFF + 32 * ROW;
    static constexpr int DS_OFF = DO_OFF + 32 * ROW;
    static constexpr int SEED_OFF = DS_OFF + 256 * SROW;   // 32 floats -LSE/scale, 32 floats -delta
    static constexpr int LDS_BYTES = SEED_OFF + 64 * 4;
};

template <class T> struct BwdIO;
template <> struct BwdIO<float> {
    // 8 consecutive elements as fp32
    __device__ static void load8(const float* p, float* x) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
        for (int i = 0; i < 4; ++i) { x[i] = a[i]; x[4 + i] = b[i]; }
    }
    __device__ static void store4(float* p, float a, float b, float c, float d) { *reinterpret_cast<f32x4*>(p) = f32x4{a, b, c, d}; }
};
template <> struct BwdIO<__bf16> {
    __device__ static void load8(const __bf16* p, float* x) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p);
        for (int i = 0; i < 4; ++i) { x[2 * i] = bf16_lo(v[i]); x[2 * i + 1] = bf16_hi(v[i]); }
    }
    __device__ static void store4(__bf16* p, float a, float b, float c, float d) {
        *reinterpret_cast<u32x2*>(p) = u32x2{pack_bf16(a, b), pack_bf16(c, d)};
    }
};

// ---- 1. pre-pass: delta and the zeroed dQ accumulator -----------------------------------------------------------------------
// D/8 lanes per query row, 8 elements each
template <int D, class OT>
__global__ __launch_bounds__(256) void bwd_pre_kernel(const BwdParams p) {
    constexpr int LPR = D / 8, RPB = 256 / LPR;
    const int64_t rows = (int64_t)p.heads * p.Sq;
    const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
    const int c0 = (threadIdx.x % LPR) * 8;
    float sum = 0.f;
    if (row < rows) {
        const int64_t bh = row / p.Sq;
        const int q = (int)(row - bh * p.Sq);
        const int b = (int)(bh / p.H), h = (int)(bh - (int64_t)b * p.H);
        float o[8], g[8];
        BwdIO<OT>::load8((const OT*)p.O + b * p.oB + h * p.oH + q * p.oS + c0, o);
        BwdIO<OT>::load8((const OT*)p.dO + b * p.doB + h * p.doH + q * p.doS + c0, g);
        for (int i = 0; i < 8; ++i) sum = fmaf(o[i], g[i], sum);
        float* acc = p.dq_acc + row * D + c0;
        *reinterpret_cast<f32x4*>(acc) = f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(acc + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int m = LPR / 2; m > 0; m >>= 1) sum += __shfl_xor(sum, m, LPR);
    if (row < rows && threadIdx.x % LPR == 0) p.delta[row] = sum;
}

// ---- 3. post-pass: dQ = scale * accumulator -----------------------------------------------------------------------------------
template <int D, class GT>
__global__ __launch_bounds__(256) void bwd_post_kernel(const BwdParams p) {
    constexpr int QPR = D / 4;   // 4-float quads per row
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx / QPR;
    if (row >= (int64_t)p.heads * p.Sq) return;
    const int c0 = (int)(idx - row * QPR) * 4;
    const int64_t bh = row / p.Sq;
    const int q = (int)(row - bh * p.Sq);
    const int b = (int)(bh / p.H), h = (int)(bh - (int64_t)b * p.H);
    const f32x4 a = *reinterpret_cast<const f32x4*>(p.dq_acc + row * D + c0);
    const float s = p.scale;
    BwdIO<GT>::store4((GT*)p.dQ + b * p.dqB + h * p.dqH + q * p.dqS + c0, s * a[0], s * a[1], s * a[2], s * a[3]);
}

// ---- 2. main kernel --------------------------------------------------------------------------------------------------------
// 8 bf16 of one column of a row-major LDS image by two hardware-transposed reads: per 16-lane group, lane i gets column col + i,
// rows row_lo .. row_lo+3 (elements 0..3) and row_hi .. row_hi+3 (elements 4..7); lane i addresses row (i >> 2), columns 4(i & 3).
__device__ __forceinline__ bf16x8 tr8(lds_ptr img, int row_bytes, int row_lo, int row_hi, int col, int lane) {
    const int i = lane & 15;
    const int off = (i >> 2) * row_bytes + (col + 4 * (i & 3)) * 2;
    const s16x4 lo = lds_read_tr16_b64(img, row_lo * row_bytes + off);
    const s16x4 hi = lds_read_tr16_b64(img, row_hi * row_bytes + off);
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

__device__ __forceinline__ f32x4 lds_read_f32x4(lds_ptr base, int byte_off) {
    return *reinterpret_cast<FA_LDS const f32x4*>(base + byte_off);
}

// GROUPED: more than one query head per K/V head (p.group > 1).  The instantiation without it is the sweep over ONE head: the
// head switch below costs the d = 128 kernel, which has no register to spare, ~1 % when it is compiled in.
template <int D, bool CAUSAL, class OT, class GT, bool GROUPED>
__global__ __launch_bounds__(256, 1) void bwd_main_kernel(const BwdParams p) {
    using C = BwdCfg<D>;
    constexpr int ROW = C::ROW, SROW = C::SROW;
    constexpr int NT = D / 32;                              // 32-row d tiles of dV^T / dK^T
    constexpr int KS = D / 16;                              // 16-element k-steps of S / dP over d
    constexpr int CPR = D / 8;                              // 16-byte chunks per bf16 row
    constexpr int NQC = 32 * CPR / 256;                     // Q chunks per thread and slice
    constexpr int EPC = 16 / (int)sizeof(OT);               // dO elements per 16-byte chunk
    constexpr int DCPR = D / EPC;                           // dO chunks per row
    constexpr int NDC = 32 * DCPR / 256;                    // dO chunks per thread and slice
    static_assert(NQC >= 1 && NDC >= 1, "at least one chunk per thread");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const lds_ptr kimg = smem + C::K_OFF, qimg = smem + C::Q_OFF, doimg = smem + C::DO_OFF, dsimg = smem + C::DS_OFF;
    const lds_ptr seeds = smem + C::SEED_OFF;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, hh = lane >> 5, G = lane >> 4;
    int bh, kb;   // bh: (batch, K/V head)
    if (CAUSAL && FA_BWD_HEAVY_FIRST) { kb = blockIdx.x / p.kv_heads; bh = blockIdx.x - kb * p.kv_heads; }
    else { bh = blockIdx.x / p.nK; kb = blockIdx.x - bh * p.nK; }
    const int b = bh / p.Hkv, h = bh - b * p.Hkv;
    const int k0 = kb * 256;
    const __bf16* Kh = p.K + b * p.kB + h * p.kH;
    const __bf16* Vh = p.V + b * p.vB + h * p.vH;
    // the group's query heads h * group .. h * group + group - 1 are swept in turn: the head the NEXT slice is loaded from ...
    const int group = GROUPED ? p.group : 1;
    const int hq0 = h * group;
    const int64_t bhq0 = (int64_t)b * p.H + hq0;
    const __bf16* Qh = p.Q + b * p.qB + hq0 * p.qH;
    const OT* dOh = (const OT*)p.dO + b * p.doB + hq0 * p.doH;
    const float* lse_h = p.lse + bhq0 * p.Sq;
    const float* delta_h = p.delta + bhq0 * p.Sq;
    float* acc_h = p.dq_acc + bhq0 * p.Sq * D;   // ... and the dQ accumulator of the head being swept

    // K block -> LDS (rows past Sk are zeros)
    for (int c = tid; c < 256 * CPR; c += 256) {
        const int row = c / CPR, cc = c - row * CPR;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (k0 + row < p.Sk) v = *reinterpret_cast<const u32x4*>(Kh + (int64_t)(k0 + row) * p.kS + cc * 8);
        lds_write_b128(kimg, row * ROW + cc * 16, v);
    }
    // the wave's V as the B fragments of dP = dO V^T: lane (r, hh) holds V[key 32t + r][16s + 8hh .. +7]
    const int kw = k0 + 64 * w;
    bf16x8 vf[2][KS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int key = kw + 32 * t + r;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (key < p.Sk) v = *reinterpret_cast<const u32x4*>(Vh + (int64_t)key * p.vS + 16 * s + 8 * hh);
            vf[t][s] = __builtin_bit_cast(bf16x8, v);
        }
    }
    f32x16 dv[NT][2], dk[NT][2];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) { dv[n][t][i] = 0.f; dk[n][t][i] = 0.f; }

    const int nsl = (p.Sq + 31) / 32;
    const int sl0 = CAUSAL ? min(k0 / 32, nsl) : 0;   // the first slice with a row q >= k0
    // the next slice's rows, staged in registers while the current one computes
    u32x4 qr[NQC], dor[NDC];
    float sd = 0.f;
    auto load_slice = [&](int q0) {
#pragma unroll
        for (int m = 0; m < NQC; ++m) {
            const int c = tid + 256 * m, row = c / CPR, cc = c - row * CPR;
            qr[m] = u32x4{0u, 0u, 0u, 0u};
            if (q0 + row < p.Sq) qr[m] = *reinterpret_cast<const u32x4*>(Qh + (int64_t)(q0 + row) * p.qS + cc * 8);
        }
#pragma unroll
        for (int m = 0; m < NDC; ++m) {
            const int c = tid + 256 * m, row = c / DCPR, cc = c - row * DCPR;
            dor[m] = u32x4{0u, 0u, 0u, 0u};
            if (q0 + row < p.Sq) dor[m] = *reinterpret_cast<const u32x4*>(dOh + (int64_t)(q0 + row) * p.doS + cc * EPC);
        }
        // rows past Sq: S' = -inf (p = 0), dP' = 0
        if (tid < 32) sd = q0 + tid < p.Sq ? -lse_h[q0 + tid] * p.inv_scale : -INFINITY;
        else if (tid < 64) sd = q0 + tid - 32 < p.Sq ? -delta_h[q0 + tid - 32] : 0.f;
    };
    auto write_slice = [&]() {
#pragma unroll
        for (int m = 0; m < NQC; ++m) {
            const int c = tid + 256 * m, row = c / CPR, cc = c - row * CPR;
            lds_write_b128(qimg, row * ROW + cc * 16, qr[m]);
        }
#pragma unroll
        for (int m = 0; m < NDC; ++m) {
            const int c = tid + 256 * m, row = c / DCPR, cc = c - row * DCPR;
            if constexpr (sizeof(OT) == 2) {
                lds_write_b128(doimg, row * ROW + cc * 16, dor[m]);
            } else {   // fp32 dO rounded to bf16 for the MFMA products
                const f32x4 x = __builtin_bit_cast(f32x4, dor[m]);
                *reinterpret_cast<FA_LDS u32x2*>(doimg + row * ROW + cc * 8) = u32x2{pack_bf16(x[0], x[1]), pack_bf16(x[2], x[3])};
            }
        }
        if (tid < 64) *reinterpret_cast<FA_LDS float*>(seeds + tid * 4) = sd;
    };

    if (sl0 < nsl) load_slice(sl0 * 32);
    // ONE loop over the slices of all the group's heads (sl wraps from the last slice of a head to the first of the next)
    for (int sl = sl0, left = (nsl - sl0) * group; left > 0; --left) {
        const int q0 = sl * 32;
        __syncthreads();                     // every wave is done with the previous slice's images
        write_slice();
        __syncthreads();

        // ---- S', dP', P, dS and the dV^T / dK^T products of this wave's 64 keys ----
        const bool hidden = kw >= p.Sk || (CAUSAL && kw > q0 + 31);
        if (hidden) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<FA_LDS u32x2*>(dsimg + (64 * w + 32 * t + r) * SROW + (8 * g + 4 * hh) * 2) = u32x2{0u, 0u};
        } else {
            f32x16 sa[2], pa[2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // accumulator registers 4g .. 4g+3 hold rows 8g + 4hh .. +3
                const f32x4 ls = lds_read_f32x4(seeds, (8 * g + 4 * hh) * 4);
                const f32x4 dl = lds_read_f32x4(seeds, 128 + (8 * g + 4 * hh) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sa[0][4 * g + j] = sa[1][4 * g + j] = ls[j];
                    pa[0][4 * g + j] = pa[1][4 * g + j] = dl[j];
                }
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int col = (16 * s + 8 * hh) * 2;
                const bf16x8 qa = lds_read_b128(qimg, r * ROW + col);
                const bf16x8 ga = lds_read_b128(doimg, r * ROW + col);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bf16x8 kf = lds_read_b128(kimg, (64 * w + 32 * t + r) * ROW + col);
                    sa[t] = mfma_32x32x16(qa, kf, sa[t]);
                    pa[t] = mfma_32x32x16(ga, vf[t][s], pa[t]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // p = exp2(c S'), dS = p dP'; the keys the mask (or the end of the sequence) cuts get the per-element test
            const bool edge = kw + 63 >= p.Sk || (CAUSAL && kw + 63 > q0);
            bf16x8 pb[2][2], sb[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int key = kw + 32 * t + r;
                float pv[16], dsv[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float e = fast_exp2(p.c * sa[t][i]);
                    if (edge && (key >= p.Sk || (CAUSAL && key > q0 + acc_row(i, hh)))) e = 0.f;
                    pv[i] = e;
                    dsv[i] = e * pa[t][i];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const u32x4 a = {pack_bf16(pv[8 * u], pv[8 * u + 1]), pack_bf16(pv[8 * u + 2], pv[8 * u + 3]),
                                     pack_bf16(pv[8 * u + 4], pv[8 * u + 5]), pack_bf16(pv[8 * u + 6], pv[8 * u + 7])};
                    const u32x4 d = {pack_bf16(dsv[8 * u], dsv[8 * u + 1]), pack_bf16(dsv[8 * u + 2], dsv[8 * u + 3]),
                                     pack_bf16(dsv[8 * u + 4], dsv[8 * u + 5]), pack_bf16(dsv[8 * u + 6], dsv[8 * u + 7])};
                    pb[t][u] = __builtin_bit_cast(bf16x8, a);
                    sb[t][u] = __builtin_bit_cast(bf16x8, d);
                    // dS^T -> LDS: registers 4g .. 4g+3 (g = 2u, 2u+1) are rows 8g + 4hh .. +3 of key column `key`
                    FA_LDS u32x2* dst = reinterpret_cast<FA_LDS u32x2*>(dsimg + (64 * w + 32 * t + r) * SROW + (16 * u + 4 * hh) * 2);
                    dst[0] = u32x2{d[0], d[1]};
                    *reinterpret_cast<FA_LDS u32x2*>(dsimg + (64 * w + 32 * t + r) * SROW + (16 * u + 8 + 4 * hh) * 2) = u32x2{d[2], d[3]};
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // dV^T += dO^T P, dK^T += Q^T dS: A fragments by transposed reads; element j of lane half hh is row
            // 16u + 8(j >> 2) + 4hh + (j & 3) of the slice -- the row order of the packed accumulator fragments
#pragma unroll
            for (int n = 0; n < NT; ++n) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int rl = 16 * u + 4 * hh, col = 32 * n + 16 * (G & 1);
                    const bf16x8 gt = tr8(doimg, ROW, rl, rl + 8, col, lane);
                    const bf16x8 qt = tr8(qimg, ROW, rl, rl + 8, col, lane);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        dv[n][t] = mfma_32x32x16(gt, pb[t][u], dv[n][t]);
                        dk[n][t] = mfma_32x32x16(qt, sb[t][u], dk[n][t]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();                     // dS^T of all 256 keys is in LDS
        // (issued here, where the S / dP / P / dS registers are dead)
        if (left > 1) {
            int qn = q0 + 32;
            if (GROUPED && sl + 1 == nsl) {      // the group's next head, from its first slice
                Qh += p.qH; dOh += p.doH; lse_h += p.Sq; delta_h += p.Sq;
                qn = sl0 * 32;
            }
            load_slice(qn);
        }

        // ---- dQ += dS K over the block's keys: wave w takes head columns [D/4 w, D/4 (w+1)) ----
        int kend = 256;                      // keys past this are hidden from every row of the slice (their dS is 0)
        if (CAUSAL) kend = min(kend, q0 + 32 - k0);
        kend = min(kend, p.Sk - k0);
        if constexpr (D == 128) {
            f32x16 dq;
            for (int i = 0; i < 16; ++i) dq[i] = 0.f;
            const int steps = (kend + 15) / 16;
            for (int s = 0; s < steps; ++s) {
                const int rl = 16 * s + 8 * hh;
                const bf16x8 a = tr8(dsimg, SROW, rl, rl + 4, 16 * (G & 1), lane);          // dS[q = r][key 16s + 8hh + j]
                const bf16x8 kk = tr8(kimg, ROW, rl, rl + 4, 32 * w + 16 * (G & 1), lane);  // K[key 16s + 8hh + j][d = 32w + r]
                dq = mfma_32x32x16(a, kk, dq);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = q0 + acc_row(i, hh);
                if (q < p.Sq) unsafeAtomicAdd(acc_h + (int64_t)q * D + 32 * w + r, dq[i]);
            }
        } else {
            f32x4 dq[2];
            for (int i = 0; i < 4; ++i) dq[0][i] = dq[1][i] = 0.f;
            const int steps = (kend + 31) / 32;
            for (int s = 0; s < steps; ++s) {
                const int rl = 32 * s + 8 * G;
                const bf16x8 kk = tr8(kimg, ROW, rl, rl + 4, 16 * w, lane);                 // K[key 32s + 8G + j][d = 16w + i]
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) {
                    const bf16x8 a = tr8(dsimg, SROW, rl, rl + 4, 16 * qt, lane);           // dS[q = 16qt + i][key 32s + 8G + j]
                    dq[qt] = mfma_16x16x32(a, kk, dq[qt]);
                }
            }
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int q = q0 + 16 * qt + 4 * G + i;
                    if (q < p.Sq) unsafeAtomicAdd(acc_h + (int64_t)q * D + 16 * w + (lane & 15), dq[qt][i]);
                }
        }
        if (++sl == nsl && GROUPED) { sl = sl0; acc_h += (int64_t)p.Sq * D; }
    }

    // ---- dK = scale dS^T Q, dV = P^T dO: lane holds key kw + 32t + r, registers 4g .. 4g+3 = d rows 32n + 8g + 4hh .. +3 ----
    GT* dKh = (GT*)p.dK + b * p.dkB + h * p.dkH;
    GT* dVh = (GT*)p.dV + b * p.dvB + h * p.dvH;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int key = kw + 32 * t + r;
        if (key >= p.Sk) continue;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * n + 8 * g + 4 * hh;
                const float s = p.scale;
                BwdIO<GT>::store4(dVh + (int64_t)key * p.dvS + d, dv[n][t][4 * g], dv[n][t][4 * g + 1], dv[n][t][4 * g + 2],
                                  dv[n][t][4 * g + 3]);
                BwdIO<GT>::store4(dKh + (int64_t)key * p.dkS + d, s * dk[n][t][4 * g], s * dk[n][t][4 * g + 1],
                                  s * dk[n][t][4 * g + 2], s * dk[n][t][4 * g + 3]);
            }
    }
}

// ---- selectors (inst_bwd_bf16.hip) ----
struct Kernel;
Kernel bwd_pre_kernel_of(int d, int o_dtype);
Kernel bwd_main_kernel_of(int d, bool causal, int o_dtype, int grad_dtype, bool grouped);
Kernel bwd_post_kernel_of(int d, int grad_dtype);

}  // namespace fa
