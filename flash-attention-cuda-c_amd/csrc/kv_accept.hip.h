// kv_accept.hip.h -- IN-CACHE ACCEPTANCE of a speculative step (flash_attention_kv_accept, flash_attention_kv_accept_paged; DESIGN.md
// section 33): after a draft tree of Sq nodes was appended at the cache positions base + 0 .. base + Sq - 1 and verified
// (flash_attention_tree*), the accepted root-to-leaf path j_0 < j_1 < ... < j_(n-1) is moved to base + 0 .. base + n - 1, where a
// linear append of the accepted tokens would have put it.  A row appended with flash_attention_rope_append_pos at its depth is
// already rotated (and, in an fp8 cache, quantised) for the position it moves to: the move is a copy of bits.
//
//   * THE RULE.  L = min(kv_lens[b], cap) (NULL: cap) still counts the draft; L <= 0: nothing.  base = L - Sq,
//     n = clamp(accept_lens[b], 0, Sq), j_t = clamp(accept_idx[b, t], 0, Sq - 1).  For t = 0 .. n - 1 IN ASCENDING ORDER, K and V of
//     every K/V head at position base + j_t are copied to position base + t.  A move with a negative source or destination position
//     is skipped; (paged) a move whose source or destination page entry is outside [0, num_pages) is skipped, never clamped; the move
//     j_t == t writes nothing.  Nothing else is written, kv_lens included.
//   * ONE LANE PER BYTE COLUMN, NOT PER MOVE.  The moves overlap in place: on the chain accept_idx = 1, 2, 3, ... every destination
//     is the previous move's source.  A lane (or a wave) per move would run the moves in an order the hardware picks: move t + 1 may
//     store to base + t + 1 before move t has read it, and row t then holds the draft's row t + 2.  No barrier below a second buffer
//     mends that across workgroups.  Here every (sequence, K/V head, K or V, 16-byte column chunk) is owned by ONE lane that walks t
//     upwards: its loads and stores of one address are program-ordered, and no other lane touches its bytes.  For a path of a
//     topologically ordered tree (j_t strictly increasing, so j_t >= t) no source is overwritten before it is read, and row t ends
//     as the draft's row j_t.
//   * BATCHES.  The lane issues the loads of NB consecutive moves before their stores.  The one way a batch could differ from the
//     sequential rule is a source that an EARLIER move of the same batch writes (j_(t+i) == t + k, k < i; never on an increasing
//     path): that value is forwarded from the earlier move's register, so every index list gives the sequential rule's bytes.
//   * UNIFORM.  A wave holds 64 consecutive (K/V head, chunk) pairs of one sequence and one of K / V: the length, n, the indices and
//     the page entries are wave-uniform scalars, and so is every branch but "the lane has a head".
//   * Every address is 64-bit arithmetic on element strides; a row start is 16-byte aligned (the host's stride checks).  No LDS, no
//     scratch, no atomics; every store is a vector store of 16 bytes.
#pragma once

#include "../../include/flash_attention.h"
#include "launchers.hip.h"
#include "utils.hip.h"

namespace fa {

struct KvAcceptParams {
    void* K;                      // the cache, or (paged) the pool
    void* V;
    const int32_t* kv_lens;       // optional [B] (device memory); NULL = the capacity
    const int32_t* block_table;   // paged: [B][table_stride] page numbers (device memory)
    const int32_t* accept_idx;    // [B][Sq] (device memory)
    const int32_t* accept_lens;   // [B] (device memory)
    int64_t kB, kH, kS, vB, vH, vS;   // element strides of the caches (paged: kB / vB the page strides); fp8: bytes
    int64_t table_stride;
    int B, Hkv, Sq, cap;          // Sq: the draft's nodes; cap: the capacity (paged: max_pages * page size)
    int head_groups;              // waves per (sequence, K or V): ceil(Hkv * chunks per row / 64)
    int num_pages, page_shift;    // paged: page size = 1 << page_shift, >= 16
};

struct KvAcceptCfg {
    static constexpr int THREADS = 256, WAVES = 4;
    static constexpr int NB = 4;                   // moves whose loads are in flight together
};

template <int D, bool KV8, bool PAGED>
__global__ __launch_bounds__(256) void kv_accept_kernel(const KvAcceptParams p) {
    using C = KvAcceptCfg;
    constexpr int ES = KV8 ? 1 : 2;      // bytes per cache element
    constexpr int CPR = D * ES / 16;     // 16-byte chunks per row
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;

    // (blockIdx, wave) -> (sequence, head group, K or V); K / V runs fastest
    int u = blockIdx.x * C::WAVES + wave;
    const int isV = u & 1; u >>= 1;
    const int hg = u % p.head_groups;
    const int b = u / p.head_groups;
    if (b >= p.B) return;

    int len = p.cap;
    if (p.kv_lens) len = min(p.kv_lens[b], p.cap);
    len = __builtin_amdgcn_readfirstlane(len);
    if (len <= 0) return;                                  // an inactive slot: nothing is moved
    const int base = len - p.Sq;                           // the position of the draft's node 0: negative when the draft outnumbers the length
    const int n = __builtin_amdgcn_readfirstlane(min(max(p.accept_lens[b], 0), p.Sq));

    const int w = hg * 64 + lane;                          // the lane's (K/V head, chunk)
    const int kvh = w / CPR, chunk = w % CPR;
    const bool has_head = kvh < p.Hkv;
    const int64_t cB = isV ? p.vB : p.kB, cH = isV ? p.vH : p.kH, cS = isV ? p.vS : p.kS;
    char* cache = (char*)(isV ? p.V : p.K) + ((int64_t)kvh * cH * ES + chunk * 16);
    if constexpr (!PAGED) cache += (int64_t)b * cB * ES;
    const int32_t* idx = p.accept_idx + (int64_t)b * p.Sq;
    const int32_t* table = PAGED ? p.block_table + (int64_t)b * p.table_stride : nullptr;

    // the byte offset of position `pos` (>= 0, < cap) from `cache`; false: its page entry is out of range
    auto locate = [&](int pos, int64_t& at) {
        if constexpr (PAGED) {
            const int entry = __builtin_amdgcn_readfirstlane(table[pos >> p.page_shift]);
            if (entry < 0 || entry >= p.num_pages) return false;      // not clamped
            at = ((int64_t)entry * cB + (int64_t)(pos & ((1 << p.page_shift) - 1)) * cS) * ES;
        } else {
            at = (int64_t)pos * cS * ES;
        }
        return true;
    };

    for (int t0 = 0; t0 < n; t0 += C::NB) {
        u32x4 x[C::NB];
        bool ok[C::NB];
        int j[C::NB];
        int64_t dst[C::NB];
#pragma unroll
        for (int i = 0; i < C::NB; ++i) {
            const int t = t0 + i;
            ok[i] = false;
            j[i] = -1;
            dst[i] = 0;
            x[i] = u32x4{0u, 0u, 0u, 0u};
            if (t >= n) continue;
            j[i] = __builtin_amdgcn_readfirstlane(min(max(idx[t], 0), p.Sq - 1));
            int64_t src = 0;
            ok[i] = j[i] != t && base + j[i] >= 0 && base + t >= 0 && locate(base + j[i], src) && locate(base + t, dst[i]);
            if (ok[i] && has_head) x[i] = *reinterpret_cast<const u32x4*>(cache + src);
        }
        // a source that an earlier move of this batch writes holds that move's value by the time the sequential rule reads it
#pragma unroll
        for (int i = 1; i < C::NB; ++i) {
#pragma unroll
            for (int k = 0; k < i; ++k)
                if (ok[i] && ok[k] && j[i] == t0 + k) x[i] = x[k];
        }
#pragma unroll
        for (int i = 0; i < C::NB; ++i)
            if (ok[i] && has_head) *reinterpret_cast<u32x4*>(cache + dst[i]) = x[i];
    }
}

// the instantiation for (d, fp8 cache, paged): inst_kv_accept.hip
Kernel kv_accept_kernel_of(int d, bool kv8, bool paged);

}  // namespace fa
