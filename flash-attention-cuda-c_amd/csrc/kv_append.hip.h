// kv_append.hip.h -- the WRITE side of the decode caches (flash_attention_kv_append, flash_attention_kv_append_paged; DESIGN.md
// section 18): the last Sq rows of every sequence, given as bf16 [B, Hkv, Sq, d], go into the cache that the split-KV kernel
// (decode_bf16.hip.h: decode and chunked prefill) reads -- contiguous [B, Hkv, capacity, d] or pools of pages behind a block table; bf16 (a bit copy) or OCP
// e4m3fn with one fp32 descale per K/V head (divide, saturate, round to nearest even once).
//
//   * POSITIONS.  L = min(kv_lens[b], capacity) ALREADY counts the new rows: new row i is key position p = L - Sq + i, written when
//     p >= 0; L <= 0 writes nothing.  Lengths, descales and table entries are read here, never by the host.
//   * WORK.  One launch does K and V.  A workgroup is (sequence, K/V head, block of 64 key POSITIONS, K or V).  Blocks are aligned
//     in position space, not in the new rows' index: block rb covers positions [64 (first / 64 + rb), + 64) cut to [first, L),
//     first = max(L - Sq, 0), so ceil(Sq / 64) + 1 blocks reach every row wherever first falls.  Each of the four waves owns 16
//     consecutive positions aligned to 16; a page is a power of two >= 16 rows, so a wave's rows lie in ONE page: the length, the
//     descale and the page entry are wave-uniform scalars, read once per wave.  A wave that holds no position of [first, L) returns
//     before it reads its table entry: only the entries of pages that receive a row are read.
//   * A LANE owns 8 consecutive d of one row: one 16-byte load of the new row; fp8: 8 correctly rounded divisions, the clamp to
//     +-448 in fp32, 4 v_cvt_pk_fp8_f32, one 8-byte store; bf16: the 16 bytes stored as loaded.  D / 8 lanes hold a row and 512 / D
//     rows share a wave instruction: the stores of a wave are whole rows, contiguous runs in one page.
//   * A table entry outside [0, numPages) is NOT clamped (decode may clamp: it only reads): the wave skips its rows.
//   * Every address is 64-bit arithmetic on the element strides.  No LDS, no scratch, no atomics; every store is a vector store.
//   * NaN.  The clamp would lose a NaN (max / min return the other operand), and what the conversion instruction does with one by
//     itself is not relied on: 0x7F is OR-ed into the byte of every element whose quotient is NaN (0x7F or 0xFF: a NaN code).
// The ragged form (new rows packed by token, a per-sequence row count) is a second, token-major kernel below.
#pragma once

#include "../../include/flash_attention.h"
#include "launchers.hip.h"
#include "utils.hip.h"

namespace fa {

struct KvAppendParams {
    const __bf16* Knew;
    const __bf16* Vnew;
    void* K;                      // the cache, or (paged) the pool
    void* V;
    const int32_t* kv_lens;       // optional [B] (device memory); NULL = the capacity
    const int32_t* block_table;   // paged: [B][table_stride] page numbers (device memory)
    const float* k_descale;       // fp8: optional [Hkv] (device memory); NULL = 1
    const float* v_descale;
    int64_t knB, knH, knS, vnB, vnH, vnS;   // element strides of the new rows (bf16)
    int64_t kB, kH, kS, vB, vH, vS;         // element strides of the caches (paged: kB / vB the page strides); fp8: bytes
    int64_t table_stride;
    int Hkv, Sq, cap;             // cap: the capacity (paged: max_pages * page size)
    int row_blocks;               // position blocks per (sequence, K/V head): ceil(Sq / 64) + 1
    int num_pages, page_shift;    // paged: page size = 1 << page_shift, >= 16
};

struct KvAppendCfg {
    static constexpr int THREADS = 256, WAVES = 4;
    static constexpr int WROWS = 16;               // positions per wave: one page holds them all (page sizes are powers of two >= 16)
    static constexpr int BLOCK = WAVES * WROWS;    // positions per workgroup
};

// the quotient saturated to +-448 in fp32: the conversion never sees an overflow (a NaN does not survive this: see above)
__device__ __forceinline__ float kv_saturate(float q) { return __builtin_fminf(__builtin_fmaxf(q, -448.f), 448.f); }

// four bf16 (two words) -> four e4m3fn bytes, the lowest d in the lowest byte
__device__ __forceinline__ uint32_t kv_quantise4(uint32_t w0, uint32_t w1, float ds) {
    const float q0 = bf16_lo(w0) / ds, q1 = bf16_hi(w0) / ds, q2 = bf16_lo(w1) / ds, q3 = bf16_hi(w1) / ds;   // correctly rounded
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(kv_saturate(q0), kv_saturate(q1), 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(kv_saturate(q2), kv_saturate(q3), r, true);
    const uint32_t nan = (q0 != q0 ? 0x7Fu : 0u) | (q1 != q1 ? 0x7F00u : 0u) | (q2 != q2 ? 0x7F0000u : 0u) | (q3 != q3 ? 0x7F000000u : 0u);
    return (uint32_t)r | nan;
}

// 8 bf16 into a cache row: a bit copy, or kv_quantise4 twice and one 8-byte store
template <bool KV8>
__device__ __forceinline__ void kv_store8(char* out, u32x4 x, float ds) {
    if constexpr (KV8) {
        u32x2 y;
        y[0] = kv_quantise4(x[0], x[1], ds);
        y[1] = kv_quantise4(x[2], x[3], ds);
        *reinterpret_cast<u32x2*>(out) = y;
    } else {
        *reinterpret_cast<u32x4*>(out) = x;
    }
}

template <int D, bool KV8, bool PAGED>
__global__ __launch_bounds__(256) void kv_append_kernel(const KvAppendParams p) {
    using C = KvAppendCfg;
    constexpr int LPR = D / 8;           // lanes per row
    constexpr int RPI = 64 / LPR;        // rows per wave instruction
    constexpr int PASSES = C::WROWS / RPI;
    constexpr int ES = KV8 ? 1 : 2;      // bytes per cache element
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;

    // blockIdx -> (sequence, K/V head, position block, K or V); K / V runs fastest
    int u = blockIdx.x;
    const int isV = u & 1; u >>= 1;
    const int rb = u % p.row_blocks; u /= p.row_blocks;
    const int kvh = u % p.Hkv;
    const int b = u / p.Hkv;

    int len = p.cap;
    if (p.kv_lens) len = min(p.kv_lens[b], p.cap);
    len = __builtin_amdgcn_readfirstlane(len);
    if (len <= 0) return;                                  // an inactive slot: nothing is written
    const int first = max(len - p.Sq, 0);                  // the position of the first row written
    // this wave's 16 positions
    const int pw = ((first / C::BLOCK + rb) * C::WAVES + wave) * C::WROWS;
    if (pw + C::WROWS <= first || pw >= len) return;       // (before the table entry is read)

    const __bf16* src = isV ? p.Vnew : p.Knew;
    const int64_t nB = isV ? p.vnB : p.knB, nH = isV ? p.vnH : p.knH, nS = isV ? p.vnS : p.knS;
    const int64_t cB = isV ? p.vB : p.kB, cH = isV ? p.vH : p.kH, cS = isV ? p.vS : p.kS;
    char* dst = (char*)(isV ? p.V : p.K);

    int row0 = pw;                                         // the wave's first row within its cache slab
    if constexpr (PAGED) {
        const int entry = __builtin_amdgcn_readfirstlane(p.block_table[b * p.table_stride + (pw >> p.page_shift)]);
        if (entry < 0 || entry >= p.num_pages) return;     // not clamped: a clamped write would land in another sequence's page
        dst += (int64_t)entry * cB * ES;
        row0 = pw & ((1 << p.page_shift) - 1);
    } else {
        dst += (int64_t)b * cB * ES;
    }
    dst += (int64_t)kvh * cH * ES;
    src += (int64_t)b * nB + (int64_t)kvh * nH;

    float ds = 1.f;
    if constexpr (KV8) {
        const float* dp = isV ? p.v_descale : p.k_descale;
        if (dp) ds = dp[kvh];
    }

    const int lr = lane / LPR, col = (lane % LPR) * 8;
    const int shift = len - p.Sq;                          // position - shift = the new row's index (>= 0 from `first` on)
    u32x4 x[PASSES];
    bool ok[PASSES];
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
        const int pos = pw + j * RPI + lr;
        ok[j] = pos >= first && pos < len;
        x[j] = u32x4{0u, 0u, 0u, 0u};
        if (ok[j]) x[j] = *reinterpret_cast<const u32x4*>(src + (int64_t)(pos - shift) * nS + col);
    }
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
        if (!ok[j]) continue;
        kv_store8<KV8>(dst + ((int64_t)(row0 + j * RPI + lr) * cS + col) * ES, x[j], ds);
    }
}

// The RAGGED append (flash_attention_kv_append_varlen, flash_attention_kv_append_paged_varlen): the new rows are
// packed by token, [totalQ, Hkv, d], and sequence b owns the tokens [cu_q[b], cu_q[b + 1]) (each pair clamped into [0, totalQ] as the
// ragged attention clamps it).  TOKEN-major: a group of D / 8 lanes owns one token row of one K/V head of K or V; it finds its
// sequence by a binary search in cu_q (the LAST b with cu_q[b] <= t: sequences without rows share their offset with the one behind
// them and are passed over), then does what the uniform kernel does for one row -- L = min(kv_lens[b], cap), position
// L - sq_b + (t - cu_q[b]), written if >= 0; its own table entry, skipped outside [0, num_pages); the same load and kv_store8,
// so the bytes are the uniform kernel's for that sequence alone.  A token no sequence owns writes nothing.  The waves are not
// aligned in position space (a wave's rows may lie in several sequences and pages: the length, the entry and the position are
// per-lane values), which costs the uniform kernel's scalar loads but needs no unit lookup and no second launch.
struct KvAppendVarlenParams {
    KvAppendParams a;             // Sq: totalQ; knB / vnB, row_blocks: not read
    const int32_t* cu_q;          // [B + 1] (device memory)
    int B;
    int token_blocks;             // ceil(totalQ / (256 / (D / 8)))
};

template <int D, bool KV8, bool PAGED>
__global__ __launch_bounds__(256) void kv_append_varlen_kernel(const KvAppendVarlenParams pv) {
    const KvAppendParams& p = pv.a;
    constexpr int LPR = D / 8;           // lanes per row
    constexpr int TPB = 256 / LPR;       // tokens per workgroup
    constexpr int ES = KV8 ? 1 : 2;      // bytes per cache element

    // blockIdx -> (K/V head, token block, K or V); K / V runs fastest
    int u = blockIdx.x;
    const int isV = u & 1; u >>= 1;
    const int tb = u % pv.token_blocks;
    const int kvh = u / pv.token_blocks;
    const int t = tb * TPB + (int)threadIdx.x / LPR, col = ((int)threadIdx.x % LPR) * 8;
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
    if (p.kv_lens) len = min(p.kv_lens[b], p.cap);
    if (len <= 0) return;                                  // an inactive slot: nothing is written
    const int pos = len - (q1 - q0) + (t - q0);            // < len <= cap
    if (pos < 0) return;                                   // more new rows than the length: the leading ones are dropped

    const __bf16* src = isV ? p.Vnew : p.Knew;
    const int64_t nH = isV ? p.vnH : p.knH, nS = isV ? p.vnS : p.knS;
    const int64_t cB = isV ? p.vB : p.kB, cH = isV ? p.vH : p.kH, cS = isV ? p.vS : p.kS;
    char* dst = (char*)(isV ? p.V : p.K);

    int row = pos;
    if constexpr (PAGED) {
        const int entry = p.block_table[b * p.table_stride + (pos >> p.page_shift)];
        if (entry < 0 || entry >= p.num_pages) return;     // not clamped: a clamped write would land in another sequence's page
        dst += (int64_t)entry * cB * ES;
        row = pos & ((1 << p.page_shift) - 1);
    } else {
        dst += (int64_t)b * cB * ES;
    }
    dst += ((int64_t)kvh * cH + (int64_t)row * cS + col) * ES;

    float ds = 1.f;
    if constexpr (KV8) {
        const float* dp = isV ? p.v_descale : p.k_descale;
        if (dp) ds = dp[kvh];
    }
    const u32x4 x = *reinterpret_cast<const u32x4*>(src + (int64_t)t * nS + (int64_t)kvh * nH + col);
    kv_store8<KV8>(dst, x, ds);
}

// the instantiation for (d, fp8 cache, paged): inst_kv_append.hip
Kernel kv_append_kernel_of(int d, bool kv8, bool paged);
Kernel kv_append_varlen_kernel_of(int d, bool kv8, bool paged);

}  // namespace fa
