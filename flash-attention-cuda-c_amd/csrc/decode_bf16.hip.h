// decode_bf16.hip.h -- the split-KV kernel of the cache-reading calls.  Decode: 1 .. FA_DECODE_MAX_Q new query rows per sequence against a
// long K/V cache, every sequence of the batch at its own length (flash_attention_decode).  Chunked prefill: the
// same kernel with RT > 1, seqLenQ up to the capacity (flash_attention_extend; the RT bullet below).
//
// The prefill kernels (kernel_bf16.hip.h) are built around 256 query rows per workgroup and one workgroup per (head, query block)
// walking all keys.  Decode is the opposite shape: a handful of rows, and the K/V read IS the cost.  So here
//   * the work unit is (batch, K/V head, row block, key split): the G * seqLenQ rows that share a K/V head are PACKED into the
//     16-row M dimension of one MFMA tile (packed row = g * seqLenQ + i: query head g of the group, query row i), so a K/V tile
//     is fetched once for the whole group, and the key range of every sequence is divided over `ns` splits in whole 128-key tiles;
//   * a workgroup is four waves; per 128-key tile each wave takes 32 keys of its own, and the waves' (m, l, O) are merged
//     through LDS once, at the end;
//   * the products are swapped (S^T = K Q^T, O^T = V^T P^T; 16x16x32 MFMA): a softmax row then lives in the four lanes
//     l, l^16, l^32, l^48, and the score registers ARE the B operand of the P.V product -- the MFMA's k index is free to stand
//     for any key as long as both operands agree, and V^T is read with that same key order;
//   * K goes straight from global memory to the registers of its A fragment (16 keys x 64 contiguous bytes per wave instruction),
//     one tile ahead; V needs a k-major fragment: it is loaded in whole 256-byte rows one tile ahead, written row-major into a
//     wave-private LDS image (row stride +32 bytes: the eight rows of a half-wave's transposed read fall on different banks) and
//     read back with ds_read_b64_tr_b16.  Wave-private: no barrier in the loop;
//   * K and V are fetched through buffer descriptors whose record count is THIS SEQUENCE's length: rows at and beyond kvLens[b]
//     arrive as 0 whatever the memory holds, their scores are masked to -inf by key index, P = 0 there;
//   * the kernel is bandwidth-bound with MFMA to spare, which is spent on precision: the softmax weights enter the P.V product
//     as a bf16 hi + lo pair (two MFMAs against the bf16 V as it lies in memory), ~16 significant bits, so the stated tolerance
//     holds for short caches too (where plain bf16 weights miss it: flash_attention.h, FA_EARLY_KEYS) with no fp16 range caveat;
//   * ns = 1: the split kernel normalises and writes O (and the LSE) itself.  ns > 1: it writes normalised fp32 partial outputs
//     and partial log-sum-exps into slabs, and decode_combine_kernel -- a second launch on the same stream -- sums them in a fixed
//     order: no atomics, the same bits run to run.  An empty split (a short sequence under many splits) writes O = 0, LSE = -inf
//     and gets weight 0;
//   * PAGED (flash_attention_decode_paged): K and V are pools of fixed-size pages [page][K/V head][row][d] and
//     key k of sequence b is row k % page_size of page block_table[b][k / page_size].  Same loop body; the one difference is where a
//     16-key group comes from.  A page holds a whole number of 16-key groups, so each of a wave's two groups per tile lies in one
//     page: the wave builds one descriptor per group and tensor, based AT the group's first row (64-bit: the pool may exceed 4 GiB)
//     and holding the group's rows below the length (none: zero bytes, everything reads as 0), and the per-lane offsets stay within
//     16 rows.  The two table entries a wave needs per tile are fetched by one vector load (lane parity = group) two tiles ahead --
//     in program order BEFORE the K/V loads of the tile in between, whose wait covers it -- so the table is never in the latency
//     chain of the K/V prefetch; the index is clamped to the last page that holds a visible key and the entry into [0, num_pages).
//   * KV8 (flash_attention_decode_fp8, flash_attention_decode_paged_fp8): the K/V elements are one byte, OCP
//     e4m3fn, with an fp32 descale per K/V head: K = K8 * k_descale[kvh], V = V8 * v_descale[kvh].  Only the K/V stream changes: a
//     lane's 16 bytes of K are 16 consecutive d of one key -- TWO 8-wide MFMA k-groups -- so the Q fragments are loaded in that d
//     order (the MFMA's k index may stand for any d as long as both operands agree) and K needs no cross-lane move; a lane's 16
//     bytes of V become 32 bytes of the same bf16 LDS image.  fp8 -> bf16 is exact (3 mantissa bits), in registers; from there
//     on the MFMAs, the softmax and the P.V product are the bf16 kernel's.  k_descale is folded into the score scale, v_descale
//     into the final 1 / l: the loop body carries neither.
//   * WINDOW (flash_attention_decode_window, flash_attention_decode_paged_window): window = W > 0 gives every
//     row a LOWER bound next to the upper one: row i sees lo_i <= key < lim with lo_i = max(limC_i - W, 0), limC_i the row's
//     bottom-right causal limit (whether or not is_causal cuts the top).  first = lo_0 is the lowest key any row sees: the
//     sequence's tiles are [first / TILE, nt), divided over the splits as before, so nothing below the first tile is fetched -- in
//     the paged form not even its table entry (look-ups are clamped to [page of first, last page]).  Keys below `first` may hold
//     anything.  In K that is harmless (the masked score is a select); V rows below `first` must arrive as 0 (0 x NaN would reach
//     the accumulator), and they can only lie in the sequence's first tile, which is only ever loaded by the prologue: there a lane
//     whose V row is below `first` uses an offset beyond any record count, and a paged 16-key group wholly below it a zero-byte
//     descriptor.  The loop's own loads carry none of this.  window = 0: first = lo_i = 0.  The decode instantiations are
//     WINDOW = true; with WINDOW = false (un-windowed chunked prefill: DecodeParams::window is not read) every term of this bullet
//     folds away.
//   * WINDOW at RT > 1 (flash_attention_extend*_window), uniform or VARLEN: the per-row bounds lo / span are
//     the same text over rt, with Sq the sequence's row count.  The tile range follows the window PER ROW BLOCK: a block whose
//     smallest query row is qmin (0 if the block reaches into the next head, else its first row's) starts at
//     firstb = max(max(len - Sq + qmin + 1, 1) - W, 0), tile tlo_b = firstb / TILE, and its tiles [tlo_b, ntb) are divided over the
//     splits as before: a long windowed chunk reads about W + rows keys per block, not the whole prefix.  Sq <= FA_DECODE_MAX_Q:
//     firstb = first, so the range -- and with it every bit -- is decode's.  The "V below first" logic stays keyed on the
//     sequence-wide `first`: firstb >= first, keys in [first, firstb) are data (another block reads them; here they are masked
//     with P = 0 against finite V), and the tile that holds `first` is tile tlo = first / TILE <= tlo_b <= t0 of every split, which a
//     block can only load as its own t0, i.e. by the prologue -- the loop loads tiles above t0 only.  Known cost: row blocks are
//     not head-aligned, and a block that straddles two heads of a long windowed chunk walks from lo_0 to len (only when
//     G Sq is no multiple of the row block).  At RT = 1 and at WINDOW = false the per-block term is not compiled.
//   * RT (flash_attention_extend, flash_attention_extend_paged): a row block is 16 RT packed rows -- RT 16-row
//     tiles per wave; decode is RT = 1.  One K fragment and one transposed V read per d group feed RT MFMAs: the cache is read once
//     per 16 RT rows, which is the point of the chunked-prefill call.  The per-row state (Q fragments, m, l, O^T, the mask limits,
//     the weights and alpha) is an array over rt, and a row of an MFMA column depends on no other column: for seqLenQ <= 16 the
//     chunked-prefill result is flash_attention_decode's bit for bit, being the same text.  A row block walks only the tiles one of
//     its rows can see: ntb = ceil(max over its rows of lim / 128), divided over the splits in whole tiles; under the causal mask
//     the lower blocks of a long chunk read less.  The end-of-loop merge of the four waves runs once per rt through the same 16-row
//     buffer (the wave's V image), with a second barrier between two tiles: LDS stays at the RT = 1 size.
//   * VARLEN (flash_attention_extend_varlen, flash_attention_extend_paged_varlen): the row count is a
//     per-sequence DEVICE value, sq_b = cu_q[b + 1] - cu_q[b] (both clamped into [0, totalQ]), and Q, O, the LSE and the slabs are
//     packed by token: row i of sequence b is packed row cu_q[b] + i.  Everything above derives its mask limits, tile counts and split
//     ranges from (len, Sq) of the ONE sequence a workgroup works on, so only two things change.  The unit decoding: the grid holds
//     Hkv * NB * ns workgroups, NB a host-side bound on sum_b ceil(G sq_b / RPB); every wave finds the sequence and the row block of
//     its block index by a wave-wide scan of the per-sequence block counts, 64 sequences per step (unit_of), and a workgroup whose
//     index lies beyond the real total returns before any barrier.  No extra launch, no workspace.  And the addressing: Sq becomes
//     the scalar sq_b, a Q / O row is token cu_q[b] + i on the token strides, a slab / LSE row is h * totalQ + cu_q[b] + i.  The
//     per-row text is untouched: sequence b's bits are those of the RT > 1 kernel on that sequence alone.  With VARLEN = false every
//     term of this bullet folds away.
//   * SINK (flash_attention_sink_*): an attention sink is a logit per QUERY head (sinks[h], natural log, not scaled)
//     that joins every row's softmax as one more key with value 0, whatever the mask, the window and the length, once per row.  The loop
//     knows nothing of it: it is added to (M, L) in the epilogue of the kernel that writes O -- under one split this kernel (the p.ns == 1
//     branch), under more the combine kernel, which takes it as one more partial result with O = 0; the slabs hold the keys alone either
//     way.  The SINK forms take parameter types of their own (SinkDecodeParams, SinkVarlenDecodeParams: the struct + the pointer), so the
//     SINK = false kernels' arguments are what they were; sinks = -inf reproduces their bits.  With SINK = false every term folds away.
//   * TREE (flash_attention_tree, flash_attention_tree_paged): the Sq rows are the nodes of a speculative draft
//     TREE, already in the cache as its last Sq keys -- node j is key base + j, base = len - Sq -- and row i sees, of those, only the
//     nodes whose bit is set in its 64-bit word tree_mask[b * Sq + i] and, always, its own key; below `base` the mask is the causal
//     one (p.causal is set), the window and the sinks are the twin's.  The one change to the arithmetic is the select of a score:
//     `rel < span` gains "and (key < base or bit key - base of the row's word)".  A tile wholly below `base` (t TILE + TILE <= base,
//     wave-uniform) takes the select as it was; only the one or two tiles that reach into [base, len) fetch the rows' words (an L2
//     hit; they are not held across the loop: the RT = 4, d = 128 form has no registers to spare) and take the masked select -- the
//     tree term is a branch of its own behind the select, which sets the scores it refuses to -inf and takes the maximum again:
//     written into the select itself it was if-converted and every tile of the cache paid its 64-bit shifts (+30 ... 60 % at RT = 4).  The
//     row's own bit is set in the fetched word, and its index, max(i, -base), is recovered from lo + span, so the row index is not
//     kept either; a row clamped to key 0 (len < Sq) fetches a word whose other bits no visible key reads.  Everything after the
//     select is the same text: a chain or an all-ones word gives the causal twin's bits.  The TREE forms are WINDOW = true, SINK =
//     true, VARLEN = false with a parameter type of their own (TreeDecodeParams); their epilogue reads sinks where the SINK form
//     does -- under ns = 1, a NULL pointer there being -inf -- and under more splits the slabs hold the keys alone and the combine
//     kernels, sink or not, are launched unchanged.  With TREE = false every term folds away.
//   * SHARED (flash_attention_cascade_decode*): the cache is ONE prefix that every sequence of the batch sees in
//     full, so the unit is (K/V head, row block, split) with no batch index and the packed rows of a K/V head run ACROSS the batch:
//     packed row = (b G + g) Sq + i, B G Sq of them, and a row block of 16 RT rows holds rows of several sequences -- a K/V tile of the
//     prefix is fetched once for all of them.  K and V are head kvh of the one shared cache (paged: the pool through the one-row
//     table), len is the shared length (kv_lens[0] clamped into [1, Sk]), and every row has lo = 0, span = len: no mask, p.causal is
//     not read.  The epilogue writes slabs under every split count, ns = 1 included, at decode's slab row (b H + h) Sq + i, and never
//     O: the sequences' own suffixes are decode's kernel into further slabs and the one combine merges both.  The loop body, the
//     fetch, the fp8 path and the four-wave merge are the same text.  The form is RT = ExtendCfg<D>::RT, WINDOW = VARLEN = SINK = TREE =
//     false, with a parameter type of its own (SharedDecodeParams: the struct + B).  With SHARED = false every term folds away.
#pragma once

#include "../../include/flash_attention.h"
#include "utils.hip.h"

namespace fa {

struct DecodeParams {
    const __bf16* Q;
    const __bf16* K;
    const __bf16* V;
    void* O;
    float* lse;              // optional [B, H, Sq]
    const int32_t* kv_lens;  // optional [B] (device memory)
    float* part_o;           // ns > 1: [ns][B*H*Sq][D] normalised partial outputs
    float* part_lse;         // ns > 1: [ns][B*H*Sq] partial log-sum-exps (natural log; -inf: empty split)
    int64_t qB, qH, qS, kB, kH, kS, vB, vH, vS, oB, oH, oS;   // element strides
    int H, Hkv, G, Sq, Sk;
    int row_blocks, ns;
    int rows;                // B * H * Sq
    int o_dtype;
    int causal;
    float scale_log2;        // scale * log2(e)
    // paged form only: K / V are the pools, kB / vB the page strides, Sk the capacity max_pages * page size
    const int32_t* block_table;   // [B][table_stride] page numbers (device memory)
    int64_t table_stride;
    int num_pages, page_shift;    // page size = 1 << page_shift, >= 16
    // fp8 (KV8) form only: K / V hold e4m3fn bytes (strides in elements = bytes); the logical cache is K8 * k_descale[K/V head],
    // V8 * v_descale[K/V head]
    const float* k_descale;       // optional [Hkv] (device memory); NULL = 1
    const float* v_descale;       // optional [Hkv] (device memory); NULL = 1
    int window;                   // 0: none; W > 0: row i sees at most the last W keys up to and including its own position
};

// The ragged (VARLEN) kernels' argument: Q / O / LSE are packed by token, Sq holds totalQ (the bound on the packed rows),
// rows = H * totalQ, row_blocks the bound NB on the row blocks of one K/V head over the whole batch, qB / oB are not read.  A type of
// its own: DecodeParams is 256 bytes, and one field more changes how the compiler fetches the arguments of -- and allocates the
// registers of -- the paged instantiations that never read it
struct VarlenDecodeParams : DecodeParams {
    const int32_t* cu_q;          // [B + 1] (device memory): sequence b owns the packed rows [cu_q[b], cu_q[b + 1]), clamped into [0, Sq]
    int B;
};
// The attention-sink (SINK) kernels' arguments (flash_attention_sink_*): types of their own for the same reason --
// DecodeParams and VarlenDecodeParams keep their size and layout, so the kernels that take them stay what they were
struct SinkDecodeParams : DecodeParams {
    const float* sinks;           // [H] (device memory): one logit per QUERY head, natural-log units, not multiplied by the scale
};
struct SinkVarlenDecodeParams : VarlenDecodeParams {
    const float* sinks;
};
// The tree-masked (TREE) kernels' argument (flash_attention_tree*), again a type of its own: sinks may be NULL here
struct TreeDecodeParams : SinkDecodeParams {
    const uint64_t* tree_mask;    // [B][Sq] (device memory): bit j of word (b, i) set = query row i sees draft node j = key len - Sq + j
};
// The shared-prefix (SHARED) kernels' argument (flash_attention_cascade_decode*), again a type of its own: K / V,
// kv_lens (one entry), Sk and the table describe the ONE shared cache; row_blocks counts the blocks of the B * G * Sq packed rows
struct SharedDecodeParams : DecodeParams {
    int B;
};
template <bool VARLEN, bool SINK = false, bool TREE = false, bool SHARED = false>
struct SplitParamsOf {
    using type = DecodeParams;
};
template <>
struct SplitParamsOf<false, false, false, true> {
    using type = SharedDecodeParams;
};
template <>
struct SplitParamsOf<false, true, true> {
    using type = TreeDecodeParams;
};
template <>
struct SplitParamsOf<true, false> {
    using type = VarlenDecodeParams;
};
template <>
struct SplitParamsOf<false, true> {
    using type = SinkDecodeParams;
};
template <>
struct SplitParamsOf<true, true> {
    using type = SinkVarlenDecodeParams;
};

template <int D, int ES = 2>   // ES: bytes per K/V element in memory (2: bf16, 1: e4m3fn); the LDS image of V is bf16 either way
struct DecodeCfg {
    static constexpr int WAVES = 4, THREADS = 256;
    static constexpr int ROWS = 16;                    // packed rows per 16-row tile: M of the 16x16x32 MFMA
    static constexpr int WKEYS = 32;                   // keys per wave per tile: K of the P.V MFMA
    static constexpr int TILE = WAVES * WKEYS;         // keys per workgroup per inner-loop tile
    static constexpr int KS = D / 32;                  // 32-wide k-steps of the Q K^T product
    static constexpr int DG = D / 16;                  // 16-wide d groups of O^T
    static constexpr int KL = KS * ES / 2;             // 16-byte K loads per lane and 16-key group: 64 bytes of a row per wave load
    static constexpr int CPR = D * ES / 16;            // 16-byte chunks per K / V row
    static constexpr int KPI = 64 / CPR;               // V rows one wave instruction loads
    static constexpr int NV = WKEYS / KPI;             // V loads per lane per tile
    static constexpr int VROW = D * 2 + 32;            // LDS bytes per V row
    static constexpr int VIMG = WKEYS * VROW;          // a wave's V image; later its (O^T) merge buffer
    static constexpr int OROW = (D + 4) * 4;           // merge buffer: bytes per packed row of fp32 O
    static constexpr int ML_OFF = WAVES * VIMG;        // [wave][row] m, then l
    static constexpr int LDS_BYTES = ML_OFF + 2 * WAVES * ROWS * 4;
    static_assert(ROWS * OROW <= VIMG, "the merge buffer reuses the V image");
};

// Chunked prefill: 16-row tiles per wave.  RT = 2 runs two workgroups per CU, RT = 4 one (its accumulators fill the register file);
// RT = 8 spills.  Measured (profiles/extend_rt_sweep.log): at d = 128 RT = 4 with the MFMAs in VGPR form (the
// Makefile's flag on the inst_extend units) is 4 ... 17 % faster than RT = 2 behind a cached prefix and 16 % slower on a chunk with no
// prefix; at d = 64 the two are equal and RT = 2 keeps the occupancy.  FA_EXTEND_RT: a build-time override for such a comparison
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

__device__ __forceinline__ void store_out(void* O, int o_dtype, int64_t idx, float v) {
    if (o_dtype == FA_DTYPE_F32) ((float*)O)[idx] = v;
    else if (o_dtype == FA_DTYPE_BF16) ((__bf16*)O)[idx] = (__bf16)v;
    else ((_Float16*)O)[idx] = (_Float16)v;
}

// VARLEN: what a block index of one K/V head works on -- sequence b, its row block rb, its first packed row q0 and its row count sq
struct VarlenUnit {
    int b, rb, q0, sq;
};

// Block index j in [0, NB) -> the unit, or false beyond the real total sum_b ceil(G sq_b / RPB).  Every wave runs this by itself (no
// LDS, no barrier) and arrives at the same scalars: per step, lane i takes sequence base + i -- its two clamped offsets, its block
// count -- an inclusive scan over the wave gives the running totals, and the first lane whose total exceeds j names the sequence.
// A sequence without rows has no blocks and is never named.  Offsets that are not non-decreasing still give b < B and rows inside
// [0, totalQ): each sequence's pair is clamped by itself
template <int RPB>
__device__ __forceinline__ bool varlen_unit_of(const VarlenDecodeParams& p, int j, int lane, VarlenUnit& u) {
    int done = 0;   // the row blocks of the sequences before this step
    for (int base = 0; base < p.B; base += WAVE) {
        const int s = min(base + lane, p.B - 1);
        const int q0 = min(max(p.cu_q[s], 0), p.Sq), q1 = min(max(p.cu_q[s + 1], q0), p.Sq);
        const int sq = base + lane < p.B ? q1 - q0 : 0;
        const int cnt = (int)(((unsigned)(p.G * sq) + RPB - 1) / RPB);   // (G sq <= H totalQ < 2^31: the host's limit)
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        const int total = __builtin_amdgcn_readlane(incl, WAVE - 1);
        if (j < done + total) {
            const unsigned long long hit = __ballot(done + incl > j);
            if (hit == 0) return false;   // (only totals that overflowed: offsets far from non-decreasing)
            const int l = __builtin_ctzll(hit);
            u.b = base + l;
            u.rb = j - done - __builtin_amdgcn_readlane(incl - cnt, l);
            u.q0 = __builtin_amdgcn_readlane(q0, l);
            u.sq = __builtin_amdgcn_readlane(sq, l);
            return u.sq > 0 && u.rb >= 0;
        }
        done += total;
    }
    return false;
}

// Decode: RT = 1, WINDOW = true.  Chunked prefill: RT = ExtendCfg<D>::RT, WINDOW = false (windowSize = 0) or true (the _window calls);
// ragged chunked prefill: those with VARLEN.  SINK (WINDOW = true only; launched with ns = 1 only -- under more splits the sink is the
// combine's): the epilogue adds the row's head's sink, a key with value 0, to (M, L) before it normalises; the loop is the same text.
// TREE (SINK = true, VARLEN = false only; launched under any ns): the masked select in the tiles that reach into the draft's keys.
// SHARED (RT = ExtendCfg<D>::RT, every other flag false; launched under any ns): one cache for the whole batch, packed rows across it,
// slabs only.
template <int D, int RT, bool PAGED, bool KV8, bool WINDOW, bool VARLEN = false, bool SINK = false, bool TREE = false, bool SHARED = false>
__global__ __launch_bounds__(256, RT <= 2 ? 2 : 1) void split_kv_kernel(const typename SplitParamsOf<VARLEN, SINK, TREE, SHARED>::type p) {
    static_assert(!SINK || WINDOW, "the SINK forms are WINDOW = true: a sinks call without a window runs them at window = 0");
    static_assert(!TREE || (SINK && !VARLEN), "the TREE forms are WINDOW = true, SINK = true, VARLEN = false");
    static_assert(!SHARED || !(WINDOW || VARLEN || SINK || TREE), "the SHARED forms are WINDOW = VARLEN = SINK = TREE = false");
    constexpr int ES = KV8 ? 1 : 2;   // bytes per K/V element
    using KV = __attribute__((may_alias)) typename std::conditional<KV8, uint8_t, __bf16>::type;
    using C = DecodeCfg<D, ES>;
    constexpr int RPB = RT * C::ROWS;   // packed rows per row block
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const lds_ptr smem = (lds_ptr)smem_raw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h4 = lane >> 4;

    // blockIdx -> (batch, K/V head, row block, split); the split index runs fastest
    int u = blockIdx.x;
    const int split = u % p.ns; u /= p.ns;
    // VARLEN: (K/V head, block index over the whole batch, split); the sequence and its row block are looked up, and a block index
    // beyond the real total leaves here, the whole workgroup alike and before any barrier
    VarlenUnit vu{};
    if constexpr (VARLEN) {
        if (!varlen_unit_of<RPB>(p, u % p.row_blocks, lane, vu)) return;
    }
    const int rb = VARLEN ? vu.rb : u % p.row_blocks; u /= p.row_blocks;
    const int kvh = VARLEN ? u : u % p.Hkv;
    // SHARED: (K/V head, row block, split) -- there is one cache, entry 0 of kv_lens and row 0 of the table; the batch index is a row's
    const int b = VARLEN ? vu.b : SHARED ? 0 : u / p.Hkv;

    int len = p.Sk;
    if (p.kv_lens) len = min(max(p.kv_lens[b], 1), p.Sk);
    len = __builtin_amdgcn_readfirstlane(len);
    const int Sq = VARLEN ? vu.sq : p.Sq;   // the rows of this sequence
    const int q0 = VARLEN ? vu.q0 : 0;      // ... and the first of them among the packed rows of Q, O, the LSE and the slabs
    // the lowest key any row sees: row 0's lower bound (0 without a window).  Keys below it are never part of the result
    const int first = WINDOW && p.window > 0 ? max(max(len - Sq + 1, 1) - p.window, 0) : 0;
    // the tiles this row block can see: below the largest limit of its rows.  Causal: the limit grows with the query row, and the
    // largest query row of the block is the last one -- unless the block reaches into the next head, then it holds a row Sq - 1.
    // RT = 1: the host caps Sq at FA_DECODE_MAX_Q = 16, so a 16-row block always holds a row with lim = len (its last row is the last
    // of all, or it holds the last query row of a head): limb = len without the arithmetic
    // SHARED: the packed rows are those of the whole batch, (b G + g) Sq + i, and every row sees the whole prefix
    int nrows = p.G * Sq;
    if constexpr (SHARED) nrows *= p.B;
    const int pr0 = rb * RPB, prl = min(pr0 + RPB, nrows) - 1;
    const int gl = prl / Sq, qmax = pr0 / Sq != gl ? Sq - 1 : prl - gl * Sq;
    const int limb = !SHARED && RT > 1 && p.causal ? max(len - Sq + qmax + 1, 1) : len;
    // the lowest key a row of THIS BLOCK sees: the lower bound of its smallest query row -- row 0 if the block reaches into the next
    // head, else its first row's.  RT = 1, no window, or Sq <= FA_DECODE_MAX_Q (the decode seam: the range stays decode's): `first`
    int firstb = first;
    if constexpr (RT > 1 && WINDOW) {
        if (p.window > 0 && Sq > FA_DECODE_MAX_Q) {
            const int g0 = pr0 / Sq, qmin = g0 != gl ? 0 : pr0 - g0 * Sq;
            firstb = max(max(len - Sq + qmin + 1, 1) - p.window, 0);
        }
    }
    // this block's tiles [tlo, ntb), divided over the splits in whole tiles
    const int ntb = (limb + C::TILE - 1) / C::TILE, tlo = firstb / C::TILE;
    const int t0 = tlo + (int)(((int64_t)(ntb - tlo) * split) / p.ns), t1 = tlo + (int)(((int64_t)(ntb - tlo) * (split + 1)) / p.ns);

    // this lane's packed rows (column r of the swapped products, tile rt): query head g of the group, query row i.  The keys the row
    // sees are [lo, lim).  Bottom-right aligned mask: the Sq rows are the LAST rows of the sequence; at least key 0.  The window's
    // left edge follows the row's own position, causal or not; lo < limc <= lim: every row sees a key
    int lo[RT];
    unsigned span[RT];   // lo <= key < lim  <=>  (unsigned)(key - lo) < span: one compare per score
    // B fragments of Q^T: Q[row][32 ks + 8 h4 .. + 7].  KV8: Q[row][64 (ks / 2) + 16 h4 + 8 (ks % 2) .. + 7] -- the d order in which
    // a lane's 16-byte K loads hold two k-groups each
    bf16x8 qf[RT][C::KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int pr = pr0 + rt * C::ROWS + r;
        const bool row_ok = pr < nrows;
        int g = row_ok ? pr / Sq : 0;
        const int qi = row_ok ? pr - g * Sq : 0;
        int qb = b;   // the sequence of the row.  SHARED: g is b G + g so far
        if constexpr (SHARED) {
            qb = g / p.G;
            g -= qb * p.G;
        }
        const int h = kvh * p.G + g;
        const int limc = max(len - Sq + qi + 1, 1);
        const int lim = !SHARED && p.causal ? limc : len;
        lo[rt] = WINDOW && p.window > 0 ? max(limc - p.window, 0) : 0;
        span[rt] = (unsigned)(lim - lo[rt]);
        const __bf16* q = p.Q + (VARLEN ? 0 : qb * p.qB) + h * p.qH + (q0 + qi) * p.qS + (KV8 ? 16 : 8) * h4;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            qf[rt][ks] = __builtin_bit_cast(bf16x8, row_ok ? *reinterpret_cast<const u32x4*>(q + (KV8 ? 64 * (ks >> 1) + 8 * (ks & 1) : 32 * ks)) : z);
        }
    }
    // the K descale rides on the score scale (one scalar load per workgroup, like kv_lens: a replayed graph sees the value of the moment)
    float scale_log2_kd = 0.f;
    if constexpr (KV8) scale_log2_kd = p.scale_log2 * (p.k_descale ? p.k_descale[kvh] : 1.f);

    // descriptors over the VISIBLE part of this (batch, K/V head): rows >= len read as 0 (contiguous form; the paged form builds
    // its descriptors per tile, below)
    const char* Kh = (const char*)((const KV*)p.K + b * p.kB + kvh * p.kH);
    const char* Vh = (const char*)((const KV*)p.V + b * p.vB + kvh * p.vH);
    const int ksb = (int)(p.kS * ES), vsb = (int)(p.vS * ES);
    const __amdgpu_buffer_rsrc_t krsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Kh, 0, (len - 1) * ksb + D * ES, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Vh, 0, (len - 1) * vsb + D * ES, 0x00020000);
    // K A fragment (kg, ks): key 16 kg + r of the wave's 32, 16-byte chunk 4 ks + h4 (KV8: load c = the fragments 2 c and 2 c + 1)
    const int koff = (wave * C::WKEYS + r) * ksb + h4 * 16;
    // V load n: key KPI n + lane / CPR of the wave's 32, chunk lane % CPR
    const int vkey = lane / C::CPR, vch = lane % C::CPR;
    const int voff = (wave * C::WKEYS + vkey) * vsb + vch * 16;
    const lds_ptr vimg = smem + wave * C::VIMG;
    const int vwr = vkey * C::VROW + vch * (32 / ES);   // (16 bytes of memory are 16 / ES elements: 32 / ES bytes of the bf16 image)
    // transposed read (dg, jj): lane 4q + pp of quarter h4 supplies row 16 jj + 4 h4 + q, columns 16 dg + 4 pp .. + 3
    const int vrd = (4 * h4 + ((lane & 15) >> 2)) * C::VROW + (lane & 3) * 8;

    // paged form: the wave index as the scalar it is (everything the descriptors are built from is then provably wave-uniform), this
    // sequence's row of the table, the last page that holds a visible key, the lane's offsets within a 16-key group, and the table
    // entries of the wave's two 16-key groups: e0, e1 for the tile whose loads are issued next, ev (lane parity = group) in flight
    // for the tile after it
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int32_t* tb = p.block_table + b * p.table_stride;
    const int last_page = (len - 1) >> p.page_shift, first_page = first >> p.page_shift;
    const int gkoff = r * ksb + h4 * 16, gvoff = vkey * vsb + vch * 16;
    int ev = 0, e0 = 0, e1 = 0;
    // the table entries of tile t: only pages that hold a key in [first, len) are looked up (a tile past the end repeats the last
    // one, a group below `first` in the first tile takes the page of `first`: its descriptor holds no bytes)
    auto table_entries = [&](int t) {
        const int key = t * C::TILE + wv * C::WKEYS + 16 * (lane & 1);
        const int page = min(key >> p.page_shift, last_page);
        return tb[WINDOW ? max(page, first_page) : page];
    };
    // take the entries that have arrived into scalars for the next load_tile, THEN fetch tile t's into the register they leave
    auto next_entries = [&](int t) {
        e0 = __builtin_amdgcn_readlane(ev, 0);
        e1 = __builtin_amdgcn_readlane(ev, 1);
        ev = table_entries(t);
    };
    // one 16-key group of one pool: a descriptor at its first row, holding its rows below len (cut: none if all are below `first`)
    auto group_rsrc = [&](const __bf16* pool, int64_t page_stride, int64_t head_stride, int64_t row_stride, int entry, int key, bool cut) {
        const int page = min(max(entry, 0), p.num_pages - 1);
        const KV* base = (const KV*)pool + page * page_stride + kvh * head_stride + (key & ((1 << p.page_shift) - 1)) * row_stride;
        const int rows = WINDOW && cut && key + 16 <= first ? 0 : min(len - key, 16);
        const int bytes = rows > 0 ? (rows - 1) * (int)(row_stride * ES) + D * ES : 0;
        const uint64_t a = (uint64_t)base;
        const uint64_t au = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
        return __builtin_amdgcn_make_buffer_rsrc((void*)au, 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
    };
    // cut (the prologue's load only: the one that can be of the sequence's first tile): V rows below `first` arrive as 0 -- the
    // lane's offset lies beyond any record count (one head's extent is below 2^31 bytes), as rows >= len lie beyond this one's
    constexpr int BEYOND = (int)0x80000000u;
    u32x4 kn[2][C::KL], vn[C::NV];
    auto load_tile = [&](int t, bool cut) {
        const int vkey0 = t * C::TILE + wave * C::WKEYS + vkey;   // the key of this lane's V load 0
        auto below_first = [&](int n) { return WINDOW && cut && vkey0 + n * C::KPI < first; };
        if constexpr (!PAGED) {
            const int kt = t * C::TILE * ksb, vt = t * C::TILE * vsb;
#pragma unroll
            for (int kg = 0; kg < 2; ++kg)
#pragma unroll
                for (int ks = 0; ks < C::KL; ++ks)
                    kn[kg][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krsrc, koff + kt + kg * 16 * ksb + ks * 64, 0, 0));
#pragma unroll
            for (int n = 0; n < C::NV; ++n)
                vn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                    vrsrc, below_first(n) ? BEYOND : voff + vt + n * C::KPI * vsb, 0, 0));
        } else {
            __amdgpu_buffer_rsrc_t kr[2], vr[2];
#pragma unroll
            for (int kg = 0; kg < 2; ++kg) {
                const int entry = kg ? e1 : e0, key = t * C::TILE + wv * C::WKEYS + 16 * kg;
                kr[kg] = group_rsrc(p.K, p.kB, p.kH, p.kS, entry, key, cut);
                vr[kg] = group_rsrc(p.V, p.vB, p.vH, p.vS, entry, key, cut);
            }
#pragma unroll
            for (int kg = 0; kg < 2; ++kg)
#pragma unroll
                for (int ks = 0; ks < C::KL; ++ks)
                    kn[kg][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(kr[kg], gkoff + ks * 64, 0, 0));
#pragma unroll
            for (int n = 0; n < C::NV; ++n)   // (V load n covers the keys KPI n .. KPI n + KPI - 1 of the wave's 32: one group)
                vn[n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                    vr[n * C::KPI / 16], below_first(n) ? BEYOND : gvoff + (n * C::KPI % 16) * vsb, 0, 0));
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
        load_tile(t0, true);
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
            load_tile(t + 1, false);
        }

        // s[rt][kg][reg]: key kb + 16 kg + reg, packed row r of tile rt
        const int kb = t * C::TILE + wave * C::WKEYS + 4 * h4;
        // TREE: does this tile reach into the draft's keys [base, len)?  Wave-uniform (t, len and Sq are scalars); a tile wholly below
        // `base` takes the select as it was
        const int base = len - Sq;
        const bool drafts = TREE && t * C::TILE + C::TILE > base;
        bf16x8 phi[RT], plo[RT];
        float alpha[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int kbl = kb - lo[rt];
            float x[8];
            float mx = NEG_INF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned rel = (unsigned)(kbl + 16 * (j >> 2) + (j & 3));   // key - lo
                x[j] = rel < span[rt] ? s[rt][j >> 2][j & 3] * (KV8 ? scale_log2_kd : p.scale_log2) : NEG_INF;
                mx = fmaxf(mx, x[j]);
            }
            if constexpr (TREE) {
                // the tree term of the select, as a branch of its own (the load keeps it one: none of it is computed in the tiles below
                // `base`): the scores of the nodes the row's word does not name become -inf and the maximum is taken again.  The word is
                // fetched here and not kept: that of query row `own` = lim - 1 - base = max(i, -base) in [0, Sq), with the own bit set.
                // (A row clamped to key 0 reads the word of another row: key 0 is its own key and its only one.)  node = key - base:
                // below 0 the cached prefix; a key the select above kept has a node below Sq <= 64
                if (drafts) {
                    const int own = lo[rt] + (int)span[rt] - 1 - base;
                    const uint64_t word = p.tree_mask[(int64_t)b * Sq + own] | (1ull << own);
                    mx = NEG_INF;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int node = kb - base + 16 * (j >> 2) + (j & 3);
                        if (node >= 0 && !((word >> (node & 63)) & 1)) x[j] = NEG_INF;
                        mx = fmaxf(mx, x[j]);
                    }
                }
            }
            mx = max_all_quarters(mx);
            const float m_new = fmaxf(m[rt], mx);
            const float m_use = m_new == NEG_INF ? 0.f : m_new;   // nothing visible yet: exp2(-inf - 0) = 0, never inf - inf
            alpha[rt] = fast_exp2(m[rt] - m_use);
            m[rt] = m_new;
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
            l[rt] = l[rt] * alpha[rt] + sum;
            // B fragment of P^T: element j of quarter h4 = the MFMA's k index 8 h4 + j = key 16 (j >> 2) + 4 h4 + (j & 3)
            phi[rt] = __builtin_bit_cast(bf16x8, u32x4{whi[0], whi[1], whi[2], whi[3]});
            plo[rt] = __builtin_bit_cast(bf16x8, u32x4{wlo[0], wlo[1], wlo[2], wlo[3]});
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
    // one barrier, every thread sums one row's share over the waves; RT > 1: a second barrier keeps the next tile's writes behind
    // these reads ----
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
            int og = opr / Sq, ob = b;
            const int oi = opr - og * Sq;
            if constexpr (SHARED) {   // (og is b G + g so far)
                ob = og / p.G;
                og -= ob * p.G;
            }
            const int oh = kvh * p.G + og;
            float inv = M != NEG_INF ? 1.0f / L : 0.f;                                         // empty split: O = 0
            if constexpr (KV8) inv *= p.v_descale ? p.v_descale[kvh] : 1.f;                    // V = V8 * v_descale: once, on the normalised sum
            float lse = M != NEG_INF ? (M + __log2f(L)) * 0.6931471805599453f : NEG_INF;         // ... LSE = -inf
            if constexpr (SINK) {
                // one more key of score sinks[head] (natural log, no scale) and value 0, once per row: with sk its log2-domain score,
                //   M' = max(M, sk),  L' = L exp2(M - M') + exp2(sk - M'),  O = acc exp2(M - M') / L',  LSE = (M' + log2 L') ln 2
                // -- every exponent is <= 0, so a sink of any finite size gives finite O and LSE.  sinks = -inf: M' = M, exp2(0) = 1,
                // exp2(-inf) = 0 and every bit is the SINK = false form's.  (ns > 1: the slabs hold the keys alone)
                if (p.ns == 1) {
                    float sink = NEG_INF;   // (TREE: the call may come without sinks, and -inf is no sink)
                    if (!TREE || p.sinks) sink = p.sinks[oh];
                    const float sk = sink * 1.4426950408889634f;
                    const float M2 = fmaxf(M, sk);
                    if (M2 != NEG_INF) {
                        const float e = fast_exp2(M - M2);
                        const float L2 = L * e + fast_exp2(sk - M2);
                        inv = 1.0f / L2 * e;
                        if constexpr (KV8) inv *= p.v_descale ? p.v_descale[kvh] : 1.f;
                        lse = (M2 + __log2f(L2)) * 0.6931471805599453f;
                    }
                }
            }
            const int64_t row = VARLEN ? (int64_t)oh * p.Sq + q0 + oi : ((int64_t)ob * p.H + oh) * Sq + oi;
            if (!SHARED && p.ns == 1) {   // (SHARED: slabs under every split count, never O)
                const int64_t base = (VARLEN ? 0 : ob * p.oB) + oh * p.oH + (q0 + oi) * p.oS + d0;
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

// Sum of the splits' partial results, in a fixed order: per (b, h, row)
//     m = max_s lse_s,   O = sum_s exp(lse_s - m) O_s / sum_s exp(lse_s - m),   LSE = m + ln sum_s exp(lse_s - m)
// rounded once, to the output type.  One workgroup per row, so that the reads of the up to 64 slabs are in flight together (a thread
// that walks the splits one after the other pays one memory latency per split: 30 us at 64 splits): every wave loads the row's
// partial LSEs, one split per lane, and reduces max and sum across its lanes; thread t then sums four consecutive d over the splits
// t / (D/4), + 256 / (D/4), ..., and the 256 / (D/4) partial sums are added through LDS in slot order.  At least one split of a row is
// not empty (every sequence has a key), so m is finite and an empty split's weight is exp(-inf) = 0.
// VARLEN (the ragged form: B = 1 to this kernel, Sq = totalQ, oB not read): a row is (head, token), and the tokens no sequence owns --
// below cu_q[0], at and beyond cu_q[B] -- have no partial results and are not written: their workgroups leave before the first barrier.
// SINK (flash_attention_sink_* under more than one split): the row's head's sink is one more partial result with
// O = 0 and LSE = sinks[head]: m = max(m, sink), one term exp(sink - m) more in the sum of the weights.  sinks = -inf: that term is
// exp(-inf) = 0, m is the splits' and every bit is the SINK = false form's.
template <int D, bool VARLEN = false, bool SINK = false>
__global__ __launch_bounds__(256) void decode_combine_kernel(const typename SplitParamsOf<VARLEN, SINK>::type p) {
    static_assert(FA_DECODE_MAX_SPLITS <= WAVE, "one split per lane");
    constexpr int TPR = D / 4, SLOTS = 256 / TPR;
    __shared__ float wgt[WAVE];
    __shared__ f32x4 part[SLOTS][TPR];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if constexpr (VARLEN) {
        const int t = row % p.Sq;
        if (t < min(max(p.cu_q[0], 0), p.Sq) || t >= min(max(p.cu_q[p.B], 0), p.Sq)) return;
    }
    const float mine = lane < p.ns ? p.part_lse[(int64_t)lane * p.rows + row] : -__builtin_inff();
    float M = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
    float sink = 0.f;
    if constexpr (SINK) {
        sink = p.sinks[row / p.Sq % p.H];
        M = fmaxf(M, sink);
    }
    const float w = __expf(mine - M);
    float W = w;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) W += __shfl_xor(W, o);   // (a butterfly: the same sum, bit for bit, in every lane and wave)
    if constexpr (SINK) W += __expf(sink - M);
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
    const float inv = 1.0f / W;
    const int oi = row % p.Sq, bh = row / p.Sq, oh = bh % p.H, b = bh / p.H;
    const int64_t base = (VARLEN ? 0 : b * p.oB) + oh * p.oH + oi * p.oS + 4 * c;
#pragma unroll
    for (int j = 0; j < 4; ++j) store_out(p.O, p.o_dtype, base + j, sum[j] * inv);
    if (p.lse && c == 0) p.lse[row] = M + __logf(W);
}

// ---- which instantiations exist, which one a call launches and how the host reaches it: split_forms.hip.h (the one table; one
// translation unit per row, all from split_unit.hip) and, for the four combine kernels, inst_split_combine.hip ----

}  // namespace fa
