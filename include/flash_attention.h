/*
 * flash_attention.h -- C ABI of the MI355X-native FlashAttention forward path (its backward pass: flash_attention_backward; its
 * split-KV decode path: flash_attention_decode).
 *
 * Drop-in boundary for the ONE hot path of GMichailov/Flash-Attention-CUDA-C: the fused
 * QK^T -> online softmax -> PV forward kernel
 *
 *     template<int D_HEAD,int Q_TILE_ROWS,int KV_TILE_ROWS> __global__
 *     void twoLoaderMhaFlashAttentionKernel(const float* Q, const float* K, const float* V,
 *                                           float* O, int batchSize, int numHeads, int seqLen,
 *                                           float scale, bool is_causal)
 *                                                   (reference kernels/FlashAttention.cuh:59-63)
 *
 * and its only host-side launcher test_flash_attention<...>() (reference tests/main.cu:21-103).
 * The reference has no symbol literally named flash_attention; BASELINE.json's north_star gives
 * that name to the launch signature above, so this library exports it with the kernel's
 * parameters in the kernel's order (Q,K,V,O,batchSize,numHeads,seqLen,...,scale,is_causal).
 * D_HEAD becomes a runtime argument; tile sizes are an internal policy (helpers.hpp), not ABI.
 *
 * Contract (same as the reference, tests/main.cu:39-48,60-64,99-102):
 *   - Q,K,V,O are DEVICE pointers to dense row-major [batchSize, numHeads, seqLen, dHead]
 *     tensors, element (b,h,s,j) at ((b*numHeads+h)*seqLen+s)*dHead+j
 *     (reference kernels/loaders.cuh:57,92).  Base pointers 16-byte aligned.
 *   - The caller owns all four buffers.  The library allocates nothing, frees nothing, keeps no
 *     global state, never synchronises the host and never prints: the call enqueues work on
 *     `stream` and returns (graph-capturable, re-entrant).  O is fully overwritten.
 *   - is_causal masks key k > query q (reference kernels/utils.cuh:43, tests/main.cu:81).
 *     Every query row keeps at least key 0, so no row is fully masked (the reference's NaN on
 *     fully-masked tiles, SURVEY.md defect D3, is not reproduced).
 *   - Each (b,h) pair is an independent problem (the reference mixes them: defect D2).
 *
 * Return value: 0 on success; > 0 a hipError_t from the launch; < 0 one of FA_ERR_* below.
 * The library never calls exit() (the reference's CUDA_CHECK does, tests/main.cu:12-19).
 *
 * There is NO CPU fallback: on a machine without a gfx950 device the call fails with a HIP error.
 */
#ifndef FLASH_ATTENTION_H
#define FLASH_ATTENTION_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Element types of Q/K/V (`dtype`) and of O (`o_dtype`). */
enum {
    FA_DTYPE_F32 = 0,      /* IEEE fp32 -- the reference's own type (const float*) */
    FA_DTYPE_BF16 = 1,     /* bfloat16, fp32 accumulation on MFMA */
    FA_DTYPE_FP8_E4M3 = 2, /* OCP e4m3fn (not fnuz); inputs only */
    FA_DTYPE_F16 = 3       /* IEEE fp16; output only */
};

/* Argument-validation errors (negative so they cannot collide with hipError_t). */
enum {
    FA_OK = 0,
    FA_ERR_NULL_POINTER = -1,
    FA_ERR_MISALIGNED = -2,       /* a base pointer is not 16-byte aligned */
    FA_ERR_BAD_SHAPE = -3,        /* batchSize/numHeads/seqLen/dHead <= 0 or too large */
    FA_ERR_UNSUPPORTED_DHEAD = -4,/* dHead not supported for this dtype */
    FA_ERR_UNSUPPORTED_DTYPE = -5,
    FA_ERR_BAD_SCALE = -6,        /* scale is NaN or infinite (fp8 inputs: or not positive) */
    FA_ERR_BAD_STRIDE = -7,
    FA_ERR_BAD_FLAGS = -8         /* flash_attention_ex: unknown flag, contradictory flags, or one that does not apply to this dtype / dHead */
};

/*
 * Precision of the softmax weights on the bf16 path (bf16 inputs, dHead 64 or 128).
 *
 * The weights P = exp(scale*S - max) are rounded before the P.V product: to bf16 (8 significant bits), or to fp16 (11 bits) with V
 * converted bf16 -> fp16 on its way into LDS.  The rounding errors of a row's weights average out over the keys that carry its
 * mass, so how close O comes to check.py (reference check.py:19-21) depends on the DATA, not only on the kernel:
 *
 *   tolerance stated by BASELINE.json: |O - ref| <= 1e-3 + 1e-3 |ref|, fp32 output, fraction of elements inside it
 *                                               bf16 weights   fp16 weights   default (flags = 0)
 *   N(0,1) Q, K, V, S = 4096, d = 128, no mask      100 %          100 %          100 %   (= bf16 weights: every row sees 4096 keys)
 *   same, causal                                   99.994 %        100 %          100 %   (the misses of bf16: rows that see few keys)
 *   Q, K x 3 (scores ~ N(0, 9^2): a SHARP softmax, a row's mass on a handful of keys), S = 4096, d = 128:
 *        no mask                                    97.9 %         100 %          97.9 %
 *        causal                                     88.3 %         100 %          90.9 %
 *   (measured: tests/test_flash_attention.py::test_parity_at_stated_tolerance_*, test_sharp_softmax_parity_is_what_it_measures;
 *    a float64 emulation of the bf16-weights arithmetic over 600 N(0,1) heads -- tests/micro/bf16_weight_error_by_row.py,
 *    profiles/r04_bf16_weight_error_by_row.txt -- puts the worst element of the rows that see 1024-1280 keys at 0.70-0.98 of the
 *    tolerance (two draws), of the rows that see 512-1024 keys at 1.07-1.31 x: hence FA_EARLY_KEYS, and its thin margin.)
 *
 *   default (flags = 0)    rows that can see fewer than FA_EARLY_KEYS keys take fp16 weights, all others bf16 weights: under the
 *                          causal mask the query rows q < FA_EARLY_KEYS of every head (whole query blocks; ONE kernel walks all
 *                          query blocks and runs each in the precision of its rows), and every row when seqLenK < FA_EARLY_KEYS.
 *                          Meets the stated tolerance on every element on N(0,1)-like data (the benchmark's); on data whose
 *                          softmax is sharp it is as accurate as bf16 weights are there (table above).  Costs ~0.5 % at seqLen 4096.
 *   FA_FLAG_F16_WEIGHTS    fp16 weights on every row (-7 % throughput; 8-13 x smaller errors): the choice for data with a sharp
 *                          softmax, or whenever the stated tolerance must hold whatever the data.
 *   FA_FLAG_BF16_WEIGHTS   bf16 weights on every row: the fastest form.
 *
 * Range of V.  Any finite bf16 V is valid input for every form (the reference's V is float: kernels/FlashAttention.cuh:60).  fp16
 * holds |v| <= 65504; a unit whose fp16-weights passes come out non-finite (a larger |v| is inf in fp16, and 0 * inf = NaN would
 * even reach rows that do not see that key) is repeated with bf16 weights and bf16 V -- so beyond 65504 the fp16 forms are as
 * accurate as FA_FLAG_BF16_WEIGHTS, never inf / NaN where the exact result is finite.  All forms accumulate un-normalised sums of
 * up to 2^8 x |v| per key in fp32: |V| up to 2^95 (4e28) is safe for any seqLen.
 * Zero-padded head dimensions (dHead not 64 / 128) have no fp16-weights kernel: their rows that see few keys keep bf16 weights.
 * Other dHead, fp8 and fp32 inputs have one form each: the two flags are rejected (FA_ERR_BAD_FLAGS) where they cannot apply,
 * except FA_FLAG_BF16_WEIGHTS on any bf16 problem.
 */
#define FA_EARLY_KEYS 1024
enum {
    FA_FLAG_F16_WEIGHTS = 1,
    FA_FLAG_BF16_WEIGHTS = 2
};

/*
 * flash_attention -- replaces the <<<grid,block,smem>>> launch of
 * twoLoaderMhaFlashAttentionKernel at reference tests/main.cu:60-61.
 *
 *   Q,K,V,O     device pointers, dense [batchSize,numHeads,seqLen,dHead]
 *   dHead       reference template parameter D_HEAD (kernels/FlashAttention.cuh:59)
 *   scale       multiplies QK^T before the softmax; the reference passes 1/sqrt(dHead)
 *               (tests/main.cu:27, check.py:19)
 *   dtype       element type of Q,K,V (FA_DTYPE_*)
 *   o_dtype     element type of O; FA_DTYPE_F32 matches the reference's float* O
 *   stream      hipStream_t (passed as void* so this header needs no HIP include); NULL = the
 *               default stream
 *
 * Supported: f32 inputs, any dHead <= 256 with 16-byte rows, any seqLen (exact fp32: dHead <= 128 on the
 *            f32-input MFMA -- 64 and 128 natively, other multiples of 4 zero-padded on the fly -- larger dHead on
 *            the generic VALU kernel);
 *            bf16 inputs, any dHead <= 128 that is a multiple of 8 on the MFMA path (64 and 128 natively, the
 *            others on the next larger instantiation with rows zero-padded on the fly; any seqLen >= 1), larger
 *            dHead <= 256 on the generic path; fp8 e4m3fn inputs, dHead <= 128 in multiples of 16 (QK^T on the
 *            block-scaled MFMA; dHead < 128 zero-padded on the fly).
 *            One head's K/V extent (seqLen x row stride) must stay below 2^31 bytes on the MFMA paths.
 */
int flash_attention(const void* Q, const void* K, const void* V, void* O,
                    int batchSize, int numHeads, int seqLen, int dHead,
                    float scale, bool is_causal,
                    int dtype, int o_dtype, void* stream);

/*
 * flash_attention_strided -- same path for tensors that are views of a (B,S,H*d_k) model-layout
 * buffer (reference check.py:14-16,24) or any other layout whose last dimension is contiguous.
 * Strides are in ELEMENTS: element (b,h,s,j) of X lives at b*strideB + h*strideH + s*strideS + j.
 * This is the strided API the reference sketched and left commented out
 * (kernels/FlashAttention.cuh:22-27: strideBatch / strideHead per tensor).
 * Row starts must stay 16-byte aligned (strides multiples of 16 bytes).
 */
typedef struct fa_strides {
    int64_t strideB, strideH, strideS;
} fa_strides;

int flash_attention_strided(const void* Q, const void* K, const void* V, void* O,
                            int batchSize, int numHeads, int seqLen, int dHead,
                            float scale, bool is_causal, int dtype, int o_dtype,
                            const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                            const fa_strides* sO, void* stream);

/*
 * flash_attention_lse -- flash_attention() that also returns the log-sum-exp of every softmax row:
 *     LSE[b,h,q] = ln( sum over visible keys k of exp(scale * <Q[b,h,q], K[b,h,k]>) )      (natural log)
 * in a dense fp32 [batchSize, numHeads, seqLen] device buffer (16-byte aligned).  This is the L / M
 * statistic of the reference's commented-out first API (kernels/FlashAttention.cuh:21,
 * archive/archive.cu:34-42,201-204) and what a backward pass, split-KV or ring composition needs.
 * LSE may be NULL (then identical to flash_attention()).
 * O with and without an LSE request: the kernels that return the LSE normalise by the fp32 sum of the UNROUNDED softmax weights
 * (so that the LSE is exact to fp32 rounding); bf16 inputs without the causal mask and without an LSE request normalise by the
 * sum of the ROUNDED weights instead (it comes out of the matrix cores with the P.V product).  The two differ by the weights'
 * rounding averaged over a row: at most one ulp of a bf16 output, <= 2^-9 relative in fp32.  A caller that compares a sharded
 * run with a whole one bit for bit asks for the LSE on BOTH sides: a shard small enough for the 128-row pair kernel always takes
 * the fp32-sum normaliser, which the whole problem's persistent kernel takes only with an LSE request
 * (tests/test_flash_attention.py::test_small_noncausal_shard_against_the_whole_problem; under the causal mask both sides always
 * sum in fp32, and shards of equal kernel choice -- BASELINE cfg4's 256-head slabs -- are bit for bit either way).
 */
int flash_attention_lse(const void* Q, const void* K, const void* V, void* O, float* LSE,
                        int batchSize, int numHeads, int seqLen, int dHead,
                        float scale, bool is_causal, int dtype, int o_dtype, void* stream);

/*
 * flash_attention_cross -- the full argument list of the reference's first (commented-out) API,
 * kernels/FlashAttention.cuh:18-28: separate seqLenQ / seqLenK, the L/M statistic, per-tensor strides.
 *   Q, O   [batchSize, numHeads, seqLenQ, dHead]      K, V   [batchSize, numHeads, seqLenK, dHead]
 *   LSE    fp32 [batchSize, numHeads, seqLenQ] or NULL;   sQ..sO  element strides or NULL (dense)
 * Cross-attention, decode against a longer key/value cache (seqLenQ < seqLenK) and chunked prefill all
 * go through here.  is_causal keeps the reference's predicate on ABSOLUTE row indices -- key k is masked
 * when k > q (kernels/utils.cuh:43) -- i.e. the mask is top-left aligned; query q sees keys
 * 0..min(q, seqLenK-1).  (A caller that wants the last query aligned with the last key offsets its K/V
 * view or runs non-causal over the prefix it may see.)
 * flash_attention_decode() below has the OTHER alignment: its is_causal is bottom-right aligned (the query rows are the LAST rows
 * of the sequence).  Top-left is right when the queries are the FIRST rows of the keys (self-attention, prefill from position 0);
 * bottom-right when new tokens are appended to a cache (decode, speculative decoding).  The two agree when seqLenQ = seqLenK.
 */
int flash_attention_cross(const void* Q, const void* K, const void* V, void* O, float* LSE,
                          int batchSize, int numHeads, int seqLenQ, int seqLenK, int dHead,
                          float scale, bool is_causal, int dtype, int o_dtype,
                          const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                          const fa_strides* sO, void* stream);

/*
 * flash_attention_ex -- flash_attention_cross() plus option flags (FA_FLAG_*); flags = 0 is flash_attention_cross().
 * flash_attention(), _lse(), _strided(), _cross() and _sharded() all run with flags = 0.  It is flash_attention_gqa() with
 * numHeadsKV = numHeads.
 */
int flash_attention_ex(const void* Q, const void* K, const void* V, void* O, float* LSE,
                       int batchSize, int numHeads, int seqLenQ, int seqLenK, int dHead,
                       float scale, bool is_causal, int dtype, int o_dtype,
                       const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                       const fa_strides* sO, unsigned flags, void* stream);

/*
 * flash_attention_gqa -- flash_attention_ex() for grouped-query attention: K and V hold numHeadsKV heads, each shared by a group of
 * G = numHeads / numHeadsKV CONSECUTIVE query heads: query head h attends K/V head h / G (integer division), the convention of
 * repeat_interleave(G, dim 1) on K and V.  numHeadsKV = 1 is multi-query attention; numHeadsKV = numHeads is flash_attention_ex()
 * itself: the same route, the same launch, the same bits.
 *   Q, O   [batchSize, numHeads, seqLenQ, dHead]      K, V   [batchSize, numHeadsKV, seqLenK, dHead]
 *   LSE    fp32 [batchSize, numHeads, seqLenQ] or NULL;   sK, sV = NULL: dense with numHeadsKV heads
 * The result is what flash_attention_ex() returns on K and V expanded G times, bit for bit (the same kernels run the same
 * arithmetic; only the K/V head a work unit reads differs), without the copy: K/V memory and traffic are 1/G of the expanded form,
 * and since the query heads of a group are neighbours in the kernels' unit list, they stream the shared head through one XCD's L2.
 * Every dtype, dHead, mask, flag and stride flash_attention_ex() accepts is accepted, with the same error codes; in addition
 * numHeadsKV <= 0, numHeads % numHeadsKV != 0 or numHeads * G >= 2^31 give FA_ERR_BAD_SHAPE (before any launch).
 * flash_attention_plan() / _plan_ex() describe a grouped-query call when given numHeads = the QUERY heads: the work units are
 * (query head, query block), which numHeadsKV does not alter.
 * flash_attention_weights() and flash_attention_sharded() take one K/V head per query head only.
 */
int flash_attention_gqa(const void* Q, const void* K, const void* V, void* O, float* LSE,
                        int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                        float scale, bool is_causal, int dtype, int o_dtype,
                        const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                        const fa_strides* sO, unsigned flags, void* stream);

/*
 * flash_attention_weights -- the attention matrix the reference's oracle returns next to its output
 * (check.py:20,25 `attn`, printed by its demo at :42).  The fused kernel never stores it; this call
 * rebuilds it from Q, K and the LSE a flash_attention_lse / flash_attention_cross call produced:
 *     P[b,h,q,k] = exp(scale * <Q[b,h,q], K[b,h,k]> - LSE[b,h,q]),   0 where is_causal hides k > q
 * P is a dense fp32 [batchSize, numHeads, seqLenQ, seqLenK] device buffer (mind its size: this is an
 * inspection path for small seqLen).  Any dHead <= 256 with 16-byte rows; sQ / sK as above or NULL.
 * One K head per query head (not grouped-query: for such a model pass K expanded to numHeads heads).
 */
int flash_attention_weights(const void* Q, const void* K, const float* LSE, float* P,
                            int batchSize, int numHeads, int seqLenQ, int seqLenK, int dHead,
                            float scale, bool is_causal, int dtype,
                            const fa_strides* sQ, const fa_strides* sK, void* stream);

/*
 * Multi-GPU: every (b,h) pair is an independent problem, so the forward pass shards
 * over the flattened head index g = b*numHeads + h with no data-path collective.
 *
 * flash_attention_shard_range -- rank `rank` of `nRanks` owns heads [*lo, *hi): contiguous ranges that tile
 * [0, totalHeads) exactly, sizes differing by at most one.  Returns 0 or FA_ERR_BAD_SHAPE.
 *
 * flash_attention_sharded -- one host thread drives nDevices devices: device deviceIds[r] holds, as its own
 * dense [hi-lo, seqLen, dHead] slabs Q[r], K[r], V[r], O[r], the head range of rank r, and gets the same
 * kernel enqueued on streams[r] (NULL array or NULL entry = that device's default stream).  Asynchronous
 * like flash_attention(); the caller's current device is restored.  Returns the first error, else 0.
 * One K/V head per query head (a grouped-query model shards over its K/V heads with flash_attention_gqa on each rank's slab).
 * (One process per GPU -- bench.py under torchrun -- just calls flash_attention() on its own slab.)
 */
int flash_attention_shard_range(int totalHeads, int rank, int nRanks, int* lo, int* hi);

int flash_attention_sharded(int nDevices, const int* deviceIds,
                            const void* const* Q, const void* const* K, const void* const* V, void* const* O,
                            int batchSize, int numHeads, int seqLen, int dHead,
                            float scale, bool is_causal, int dtype, int o_dtype, void* const* streams);

/*
 * Launch-geometry policy -- the counterpart of the reference's helpers.hpp:8-36
 * (calculateSizeBlockQ / calculateSizeBlockKV / getNumCta, which return constants there).
 * Fills the tile sizes and grid the library will use for this problem; returns 0 or FA_ERR_*.
 */
typedef struct fa_launch_plan {
    int q_block_rows;    /* Br: query rows per workgroup          (helpers.hpp:8-19); 256 on the MFMA paths' persistent kernels, 128 (and
                            threads = 256) for small bf16 problems at dHead 64 / 128: the pair kernel */
    int kv_block_rows;   /* Bc: keys per inner-loop tile           (helpers.hpp:21-30) */
    int threads;         /* threads per workgroup                  (tests/main.cu:52)  */
    int grid;            /* number of workgroups                   (helpers.hpp:33-36) */
    int lds_bytes;       /* dynamic LDS per workgroup              (tests/main.cu:55)  */
    int kernel_id;       /* which internal kernel: 0 generic fp32 VALU, 1 bf16 MFMA, 2 fp8 MFMA, 3 exact-fp32 MFMA */
} fa_launch_plan;

int flash_attention_plan(int batchSize, int numHeads, int seqLen, int dHead, bool is_causal,
                         int dtype, int o_dtype, fa_launch_plan* plan);

/*
 * flash_attention_plan_ex -- what a flash_attention_ex() call with these arguments launches.  A bf16 problem may be split in two
 * ranges of query blocks (see "Precision of the softmax weights"): `early` describes the fp16-weights kernel over the first
 * early->q_blocks query blocks of every head, `main` the bf16-weights kernel over the remaining main->q_blocks; a range that
 * does not exist has q_blocks = 0 and grid = 0.  When both exist they run in ONE launch of one kernel (every workgroup walks its
 * share of the list of all query blocks; a unit runs in the precision of its block): both descriptions then carry that launch's
 * grid and LDS size.  lds_bytes is the launched
 * instantiation's own figure (it depends on the engine, the staging form and the output type).  flash_attention_plan() is
 * this call with seqLenK = seqLen, flags = FA_FLAG_BF16_WEIGHTS (one range) and only `main` returned.  Either pointer may be NULL.
 */
typedef struct fa_launch_plan_ex {
    fa_launch_plan launch;
    int q_blocks;        /* query blocks of every head this range covers */
    int first_q_block;   /* ... starting at this one */
    int unit_lists;      /* 1 = both ranges run in ONE launch of one kernel that walks ONE (head, query block) list over all query blocks,
                            every unit in the precision of its range; 0 = this is the only range (or the pair kernel's launch) */
} fa_launch_plan_ex;

int flash_attention_plan_ex(int batchSize, int numHeads, int seqLenQ, int seqLenK, int dHead, bool is_causal,
                            int dtype, int o_dtype, unsigned flags, fa_launch_plan_ex* early, fa_launch_plan_ex* main);

/*
 * flash_attention_backward -- the gradients of O = softmax(scale * Q K^T [+ causal mask]) V with respect to Q, K and V, P recomputed
 * from Q, K and the forward's LSE (no N x N matrix is stored):
 *     P  = exp(scale * Q K^T - LSE)          delta = rowsum(dO * O)
 *     dV = P^T dO                            dS    = P * (dO V^T - delta)
 *     dQ = scale * dS K                      dK    = scale * dS^T Q
 *   Q, O, dO, dQ   [batchSize, numHeads, seqLenQ, dHead]      K, V, dK, dV   [batchSize, numHeads, seqLenK, dHead]
 *   LSE            dense fp32 [batchSize, numHeads, seqLenQ], as flash_attention_lse / _cross / _ex return it
 *   workspace      caller-owned device scratch of flash_attention_backward_workspace_size(batchSize, numHeads, seqLenQ, dHead)
 *                  bytes, 16-byte aligned; its contents on entry are ignored (fp32 delta, then the fp32 dQ accumulator)
 *   sQ .. sdV      element strides as for flash_attention_cross, or NULL (dense)
 * The conventions are the forward's: arguments are validated before any launch, nothing is allocated, the host is never
 * synchronised, the work is enqueued on `stream` (three kernels in one chain: graph-capturable).
 *
 * Mask.  is_causal is the forward's top-left mask on absolute indices (key k hidden when k > q); any seqLenQ, seqLenK >= 1.
 * Every element of dQ, dK and dV is written; keys that no query sees (under the mask: k >= seqLenQ) get dK = dV = 0.
 *
 * Supported: dtype = FA_DTYPE_BF16 (Q, K, V); o_dtype in {F32, BF16}, the type of both O and dO; grad_dtype in {F32, BF16}, the type
 * of dQ, dK and dV; dHead 64 or 128; scale finite and > 0.  One head's K / V extent (seqLenK x row stride) below 2^31 bytes, as on
 * the forward's MFMA paths.  Other inputs are rejected before any launch with the forward's codes: fp32 / fp8 inputs and F16 O or
 * gradients FA_ERR_UNSUPPORTED_DTYPE, any other dHead FA_ERR_UNSUPPORTED_DHEAD, a non-finite or non-positive scale FA_ERR_BAD_SCALE,
 * null pointers, misalignment, bad strides and shapes FA_ERR_NULL_POINTER / _MISALIGNED / _BAD_STRIDE / _BAD_SHAPE.
 *
 * Precision.  P is recomputed in fp32 and rounded to bf16 before dV^T += dO^T P; dS is rounded to bf16 before dK^T += Q^T dS and
 * dQ += dS K; an fp32 dO is rounded to bf16 for the MFMA products (delta is summed from the given O and dO in fp32); every product
 * is accumulated in fp32, and gradients are rounded once, to grad_dtype, when they are written.
 *
 * Determinism.  dK and dV are summed by one workgroup each, in a fixed order: bitwise reproducible from run to run.  dQ is summed
 * across the key blocks of a head with fp32 atomics, so its last bits may vary from run to run.
 *
 * flash_attention_backward_gqa -- the same for grouped-query attention (flash_attention_gqa: query head h attends K/V head h / G,
 * G = numHeads / numHeadsKV):
 *   Q, O, dO, dQ   [batchSize, numHeads, seqLenQ, dHead]      K, V, dK, dV   [batchSize, numHeadsKV, seqLenK, dHead]
 *   LSE            dense fp32 [batchSize, numHeads, seqLenQ];   sK, sV, sdK, sdV = NULL: dense with numHeadsKV heads
 *   workspace      flash_attention_backward_workspace_size(batchSize, numHeads, seqLenQ, dHead) bytes: it depends on the QUERY heads only
 * dK and dV of a K/V head are the sums over its G query heads.  One workgroup owns 256 keys of one (batch, K/V head) and sweeps
 * the query rows of the group's heads one head after the other with the same accumulators, so the determinism paragraph above
 * holds for any G: dK and dV are summed by one workgroup each, in a fixed order; dQ with atomics.  (The grid is
 * batchSize * numHeadsKV * ceil(seqLenK / 256) workgroups: few K/V heads on short sequences leave compute units idle.)
 * Arguments are checked as flash_attention_backward checks them, and numHeadsKV as flash_attention_gqa does (FA_ERR_BAD_SHAPE).
 * flash_attention_backward() is this call with numHeadsKV = numHeads: the same launches, the same bits.
 */
size_t flash_attention_backward_workspace_size(int batchSize, int numHeads, int seqLenQ, int dHead);

int flash_attention_backward(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE,
                             void* dQ, void* dK, void* dV, void* workspace,
                             int batchSize, int numHeads, int seqLenQ, int seqLenK, int dHead,
                             float scale, bool is_causal, int dtype, int o_dtype, int grad_dtype,
                             const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                             const fa_strides* sdO, const fa_strides* sdQ, const fa_strides* sdK, const fa_strides* sdV,
                             void* stream);

int flash_attention_backward_gqa(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE,
                                 void* dQ, void* dK, void* dV, void* workspace,
                                 int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                 float scale, bool is_causal, int dtype, int o_dtype, int grad_dtype,
                                 const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                 const fa_strides* sdO, const fa_strides* sdQ, const fa_strides* sdK, const fa_strides* sdV,
                                 void* stream);

/*
 * flash_attention_decode -- split-KV decode: 1 .. FA_DECODE_MAX_Q new query rows per sequence against a long K/V cache, each sequence
 * of the batch at its own length.  The G = numHeads / numHeadsKV query heads of a group times the seqLenQ rows are packed into one
 * MFMA tile, so the K/V cache -- whose read IS the cost of decode -- is read once per group; and the key range of every sequence is
 * divided over `numSplits` workgroups, whose partial results a second small kernel combines, so that a single sequence fills the chip.
 *   Q, O     [batchSize, numHeads, seqLenQ, dHead]      K, V   [batchSize, numHeadsKV, seqLenK, dHead]; seqLenK is the cache CAPACITY
 *   sQ .. sO element strides as for flash_attention_cross, or NULL (dense): a [B, S, Hkv, d] cache is a view.  Query head h reads
 *            K/V head h / G (flash_attention_gqa's convention)
 *   kvLens   DEVICE pointer to int32[batchSize], the number of valid keys of each sequence, read BY THE KERNEL -- never by the host: the
 *            call stays asynchronous and graph-capturable, and a replayed graph sees the lengths of the moment.  NULL = seqLenK for
 *            every sequence.  A value is clamped on the device into [1, seqLenK].  Keys at and beyond kvLens[b] never enter the result:
 *            they may hold NaN, inf or stale data
 *   LSE      optional dense fp32 [batchSize, numHeads, seqLenQ], natural log, over the visible keys (as flash_attention_lse returns it:
 *            decode results of several devices or cache pages can be merged with it); NULL = not wanted.  O is the same bits either way
 *   workspace caller-owned device scratch of flash_attention_decode_workspace_size(batchSize, numHeads, seqLenQ, dHead, num_splits)
 *            bytes, 16-byte aligned; contents on entry ignored (fp32 partial outputs, then partial log-sum-exps, one slab per split).
 *            Not needed (may be NULL) when the plan says num_splits == 1
 *   numSplits 0 = the library chooses, on the HOST and from the shapes only (seqLenK, not kvLens); > 0 = forced (tests, tuning);
 *            < 0 or > FA_DECODE_MAX_SPLITS: FA_ERR_BAD_SHAPE.  flash_attention_decode_plan() reports the choice and the launches
 * The conventions are the forward's: arguments are validated before any launch, nothing is allocated, the host is never synchronised,
 * no global state, nothing printed; the work is enqueued on `stream` (one kernel, or two in a chain when num_splits > 1).
 *
 * Mask.  is_causal here is BOTTOM-RIGHT aligned: the seqLenQ rows are the LAST rows of the sequence; row i of batch b sees the keys
 * k <= kvLens[b] - seqLenQ + i and -- the library's rule -- at least key 0.  is_causal = false: every row sees keys [0, kvLens[b]).
 * (flash_attention_cross's mask is top-left aligned: see there which applies where.  The prefill kernels have no bottom-right mask.)
 *
 * Supported: dtype = FA_DTYPE_BF16; dHead 64 or 128; o_dtype F32, BF16 or F16; 1 <= seqLenQ <= FA_DECODE_MAX_Q (more new rows is chunked
 * prefill: flash_attention_gqa); any numHeadsKV dividing numHeads; scale finite and > 0; one head's K / V extent (seqLenK x row stride)
 * below 2^31 bytes, as on the prefill MFMA paths.  Everything else is rejected before any launch with the forward's codes: other
 * inputs or outputs FA_ERR_UNSUPPORTED_DTYPE, other dHead FA_ERR_UNSUPPORTED_DHEAD, a non-finite or non-positive scale FA_ERR_BAD_SCALE,
 * seqLenQ out of range, bad head counts, shapes and split counts FA_ERR_BAD_SHAPE, null pointers (a NULL workspace the plan needs
 * included), misalignment (kvLens: 4 bytes) and bad strides FA_ERR_NULL_POINTER / _MISALIGNED / _BAD_STRIDE.
 *
 * Precision.  Scores and the softmax are fp32; the weights enter the P.V product as a bf16 hi + lo pair (two MFMAs against the bf16 V
 * as it lies in memory: ~16 significant bits), accumulated in fp32.  The stated tolerance 1e-3 + 1e-3 |ref| holds on every element for
 * short caches as for long ones, and any finite bf16 V is valid (nothing is converted to fp16: no "Range of V" caveat).
 *
 * Determinism.  Partial results are combined from slabs in a fixed order, without atomics: the same call gives the same bits from run
 * to run.  With o_dtype BF16 / F16 the result is the F32 result of the same call rounded once, at the store.
 *
 * flash_attention_decode_plan -- what a flash_attention_decode() call with these arguments (and this numSplits) launches.
 * flash_attention_decode_workspace_size -- bytes for `numSplits` splits AS PLANNED (pass plan.num_splits, not 0); 0 for one split.
 */
#define FA_DECODE_MAX_Q 16          /* more new rows than this: that is chunked prefill, use flash_attention_gqa */
#define FA_DECODE_MAX_SPLITS 64     /* cap of numSplits */
/* Launch limit of every flash_attention_decode* / flash_attention_extend* call and plan: one launch holds fewer than 2^32 threads, in
 * workgroups of 256.  plan.grid must stay below this, and so must the rows of O (batchSize * numHeads * seqLenQ; ragged: numHeads *
 * totalQ) whenever num_splits > 1 -- the combine kernel runs one workgroup per row.  At or above it: FA_ERR_BAD_SHAPE, from the plan
 * and from the call, before any launch.  numSplits = 0 never asks for a second split at such a row count (the units alone fill the
 * chip), so only a FORCED numSplits > 1 meets the row limit */
#define FA_DECODE_MAX_WORKGROUPS (1 << 24)

typedef struct fa_decode_plan {
    int num_splits;      /* key-range splits per (batch, K/V head, row block) the call will use */
    int row_blocks;      /* blocks of packed (query head of the group, query row) rows per K/V head; 1 = K/V read once per group */
    int rows_per_block;  /* packed rows one workgroup holds */
    int kv_block_rows;   /* keys per inner-loop tile */
    int threads, grid, lds_bytes;          /* of the split kernel */
    int combine_grid, combine_threads;     /* 0 when num_splits == 1: the split kernel writes O itself, one launch */
} fa_decode_plan;

int    flash_attention_decode_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                   int o_dtype, int numSplits /* 0 = the library chooses */, fa_decode_plan* plan);
size_t flash_attention_decode_workspace_size(int batchSize, int numHeads, int seqLenQ, int dHead, int numSplits /* as planned */);

int flash_attention_decode(const void* Q, const void* K, const void* V, void* O, float* LSE,
                           const int32_t* kvLens, void* workspace,
                           int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                           float scale, bool is_causal, int dtype, int o_dtype, int numSplits,
                           const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                           void* stream);

/*
 * flash_attention_decode_paged -- flash_attention_decode against PAGED K/V caches: K and V live in pools of fixed-size pages and every
 * sequence names its pages in a block table, as serving engines store them (no gather into a contiguous copy before the call).
 *   Kpool, Vpool [numPages, numHeadsKV, pageSize, dHead] bf16.  In sK / sV strideB is the PAGE stride (strideH the head stride, strideS
 *            the row stride); NULL = dense.  A [numPages, pageSize, numHeadsKV, dHead] pool is therefore a view
 *   blockTable DEVICE pointer to int32, 4-byte aligned: key k of sequence b is row k % pageSize of page
 *            blockTable[b * tableStride + k / pageSize].  tableStride is in elements, >= maxPagesPerSeq (a row slice of a wider table
 *            is fine).  Entries are read BY THE KERNEL, like kvLens -- the host never synchronises, a replayed graph sees the table of
 *            the moment -- and only the entries of pages that hold at least one key < kvLens[b]; each entry read is clamped on the
 *            device into [0, numPages - 1]: a stale entry can give a wrong answer, never an unmapped address.  Several sequences may
 *            name the same page (a shared prefix); the call only reads the pools
 *   capacity maxPagesPerSeq * pageSize plays the part of flash_attention_decode's seqLenK: kvLens[b] is clamped on the device into
 *            [1, capacity], NULL = the capacity, and the split count is chosen on the host from the capacity.
 *            flash_attention_decode_plan(..., seqLenK = maxPagesPerSeq * pageSize, ...) and flash_attention_decode_workspace_size
 *            describe a paged call as well (there is no second plan function)
 *   Rows at and beyond kvLens[b] in the last page, and every page not read, may hold NaN, inf or stale data: they never enter the result.
 *   pageSize a power of two >= 16 (16 keys are one K fragment load: no load straddles pages); one page's head extent (pageSize x row
 *            stride) below 2^31 bytes.  The pool as a whole may exceed 2^32 bytes: page bases are 64-bit.
 * Q, O, LSE, workspace, numSplits, the bottom-right mask, the precision (hi + lo bf16 weights), the supported types, dHead 64 / 128,
 * seqLenQ <= FA_DECODE_MAX_Q, determinism and the conventions (validated before any launch; never allocates, synchronises or prints)
 * are flash_attention_decode's.  Tiles and splits are divided as there, so the result equals, bit for bit, flash_attention_decode on a
 * contiguous copy of the same pages with seqLenK = the capacity and the same numSplits.
 * Rejected before any launch: everything flash_attention_decode rejects, with the same codes; numPages <= 0, maxPagesPerSeq <= 0,
 * pageSize < 16 or not a power of two, a capacity above 2^24, tableStride < maxPagesPerSeq, a page extent >= 2^31 bytes
 * FA_ERR_BAD_SHAPE; a NULL blockTable FA_ERR_NULL_POINTER; a blockTable not aligned to 4 bytes FA_ERR_MISALIGNED.
 */
int flash_attention_decode_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                 const int32_t* kvLens, const int32_t* blockTable, void* workspace,
                                 int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                 int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                 float scale, bool is_causal, int dtype, int o_dtype, int numSplits,
                                 const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                 void* stream);

/*
 * flash_attention_decode_fp8, flash_attention_decode_paged_fp8 -- flash_attention_decode / flash_attention_decode_paged against fp8
 * K/V caches: bf16 Q, K and V stored as OCP e4m3fn bytes (not fnuz) with one fp32 descale per K/V head.  The K/V read is the cost of
 * decode; an fp8 cache halves it and doubles the context that fits in memory.
 *   K, V / Kpool, Vpool  the siblings' layouts with ONE-BYTE elements: rows of dHead bytes; sK / sV are element strides, which here
 *            are bytes, each a multiple of 16 (row starts stay 16-byte aligned); NULL = dense
 *   kDescale, vDescale   DEVICE pointers to fp32[numHeadsKV], 4-byte aligned, NULL = 1.0 for every head.  The logical cache is
 *            K = K8 * kDescale[kvh], V = V8 * vDescale[kvh].  Read BY THE KERNEL, like kvLens: a replayed graph sees the values of the
 *            moment.  The LSE is over the scores of the logical (descaled) K.  A descale that is not finite and positive gives an
 *            unspecified numeric result, never a bad address
 *   dtype    of Q: FA_DTYPE_BF16.  kv_dtype: FA_DTYPE_FP8_E4M3.  o_dtype as for the siblings
 * Everything else -- kvLens, blockTable, LSE, workspace, numSplits, the bottom-right mask, determinism, the conventions -- is the
 * sibling's.  flash_attention_decode_plan and flash_attention_decode_workspace_size describe these calls unchanged: the plan does not
 * depend on the type of the cache.
 *
 * Conversion and precision.  e4m3fn -> bf16 is exact (3 mantissa bits, and every e4m3fn value, subnormals included, is a bf16
 * value); it happens in registers, and from there on the arithmetic is flash_attention_decode's: bf16 MFMAs, fp32 scores and softmax,
 * bf16 hi + lo weights.  kDescale multiplies the score scale and vDescale the normalised output, once each, in fp32; with power-of-two
 * descales the result is exactly that of the bf16 kernel on the descaled cache.  The stated tolerance 1e-3 + 1e-3 |ref| holds against a
 * reference computed from the DEQUANTISED values; the error of quantising a cache to fp8 is the caller's.  Range of V: |v| <= 448 *
 * vDescale[kvh], the e4m3fn range.  Bytes at and beyond kvLens[b] and pages not read may hold any pattern, 0x7F / 0xFF (NaN) included.
 * A NaN byte BELOW the length is data: it propagates.
 *
 * Paged and contiguous.  Tiles and splits are divided as in the siblings, so flash_attention_decode_paged_fp8 equals, bit for bit,
 * flash_attention_decode_fp8 on a contiguous copy of the same pages with seqLenK = the capacity, the same descales and numSplits.
 *
 * Rejected before any launch: everything the sibling rejects, with the same codes; kv_dtype other than FA_DTYPE_FP8_E4M3 or dtype other
 * than FA_DTYPE_BF16 FA_ERR_UNSUPPORTED_DTYPE; a descale pointer not aligned to 4 bytes FA_ERR_MISALIGNED; a K / V stride that is not a
 * multiple of 16 elements FA_ERR_BAD_STRIDE.  The extent limit -- one head's K / V extent ((seqLenK + 192) x row stride), or one page's
 * (pageSize x row stride), below 2^31 BYTES -- is counted at one byte per element: twice the rows per stride of the bf16 calls.  The
 * capacity cap of 2^24 keys stays.
 */
int flash_attention_decode_fp8(const void* Q, const void* K, const void* V, void* O, float* LSE,
                               const int32_t* kvLens, const float* kDescale, const float* vDescale, void* workspace,
                               int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                               float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                               const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                               void* stream);

int flash_attention_decode_paged_fp8(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                     const int32_t* kvLens, const int32_t* blockTable,
                                     const float* kDescale, const float* vDescale, void* workspace,
                                     int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                     int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                     float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                     const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                     void* stream);

/*
 * flash_attention_decode_window, flash_attention_decode_paged_window -- split-KV decode with a SLIDING WINDOW: every query row sees at
 * most the last windowSize keys up to and including its own position (Mistral, Gemma, the local layers of gpt-oss).  The argument
 * lists are flash_attention_decode_fp8's / flash_attention_decode_paged_fp8's with windowSize after numSplits, and serve all four
 * cache forms: kv_dtype = FA_DTYPE_BF16 (kDescale and vDescale must be NULL) or FA_DTYPE_FP8_E4M3 (the _fp8 siblings' caches and
 * descales), contiguous or paged.  Everything not named here is the sibling's.
 *
 * Mask.  With len = kvLens[b] clamped into [1, capacity], limC_i = max(len - seqLenQ + i + 1, 1) (the bottom-right causal limit of row
 * i, the "at least key 0" rule included) and lo_i = max(limC_i - windowSize, 0):
 *   is_causal = true    row i sees the keys lo_i <= k < limC_i      (flash-attn's window_size = (windowSize - 1, 0))
 *   is_causal = false   row i sees the keys lo_i <= k < len         (window_size = (windowSize - 1, -1): the left edge still follows
 *                       the row's own position)
 * Every row sees at least one key: no NaN rows.  windowSize = 0: no window -- the call is the sibling's (flash_attention_decode,
 * _paged, _fp8, _paged_fp8 by kv_dtype and form): the same launches, the same bits.  There is no right window and no per-head window (attention
 * sinks: flash_attention_sink_decode*, below).
 *
 * Below the window.  first(b) = lo_0 is the lowest key any row of sequence b sees.  The contract mirrors the one for keys at and
 * beyond kvLens[b]: keys below first(b) never enter the result; their K and V may hold NaN, inf, stale data or any fp8 byte (0x7F /
 * 0xFF included).  Only the 128-key tiles from first(b) / 128 on are fetched, so the K/V bytes read follow the window, not the
 * length.  Paged: a page whose keys ALL lie below first(b) is never read and neither is its blockTable entry, which may be any int32:
 * a serving engine may free or reuse the page.  (Look-ups are clamped into [page of first(b), last page with a key < kvLens[b]].)
 * A key in [first(b), kvLens[b]) that one row does not see is still data another row reads: it must be valid.
 *
 * Plan.  A windowed sequence spans at most windowSize + seqLenQ - 1 keys: at most ceil((windowSize + seqLenQ - 1) / 128) + 1 tiles.
 * flash_attention_decode_plan_window chooses the split count from the smaller of that and the capacity's tiles, by the rule of
 * flash_attention_decode_plan -- which is this function with windowSize = 0; windowSize >= seqLenK plans as no window does.  A forced
 * numSplits is used as given; splits beyond the window's tiles come out empty (weight 0).  flash_attention_decode_workspace_size is
 * unchanged: pass the planned num_splits.  Paged: seqLenK = maxPagesPerSeq * pageSize.
 *
 * Tiles and splits are divided alike in both forms: flash_attention_decode_paged_window equals, bit for bit,
 * flash_attention_decode_window on a contiguous copy of the same pages with seqLenK = the capacity and the same numSplits, windowSize
 * and descales.  Precision, determinism and the conventions (validated before any launch; never allocates, synchronises or prints)
 * are the siblings'.
 *
 * Rejected before any launch: everything the sibling of the same kv_dtype and form rejects, with the same codes; windowSize < 0
 * FA_ERR_BAD_SHAPE; kv_dtype other than FA_DTYPE_BF16 / FA_DTYPE_FP8_E4M3, or a non-NULL kDescale / vDescale with
 * kv_dtype = FA_DTYPE_BF16, FA_ERR_UNSUPPORTED_DTYPE.
 */
int flash_attention_decode_plan_window(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                       int o_dtype, int numSplits /* 0 = the library chooses */, int windowSize,
                                       fa_decode_plan* plan);

int flash_attention_decode_window(const void* Q, const void* K, const void* V, void* O, float* LSE,
                                  const int32_t* kvLens, const float* kDescale, const float* vDescale, void* workspace,
                                  int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                  float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                  int windowSize,
                                  const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                  void* stream);

int flash_attention_decode_paged_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                        const int32_t* kvLens, const int32_t* blockTable,
                                        const float* kDescale, const float* vDescale, void* workspace,
                                        int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                        int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                        float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                        int windowSize,
                                        const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                        void* stream);

/*
 * flash_attention_kv_append, flash_attention_kv_append_paged -- the WRITE side of the decode caches: the new rows of every sequence go
 * into the cache that flash_attention_decode* reads -- a bit copy into a bf16 cache, or quantised to OCP e4m3fn with one fp32 descale
 * per K/V head into an fp8 cache.  One launch writes K and V; a decode step is `kv_lens += Sq; append; decode`, one graph.
 *   Knew, Vnew [batchSize, numHeadsKV, seqLenNew, dHead] bf16 (dtype = FA_DTYPE_BF16).  sKnew / sVnew: element strides or NULL (dense);
 *            the last dimension is contiguous, so the K and V slices of a fused [B, S, (H + 2 Hkv) d] projection pass without a copy
 *   K, V / Kpool, Vpool  the caches of the decode call of the same kv_dtype and form: [batchSize, numHeadsKV, seqLenK, dHead], seqLenK
 *            the CAPACITY, or pools [numPages, numHeadsKV, pageSize, dHead] (strideB = the page stride) behind blockTable; bf16
 *            (kv_dtype = FA_DTYPE_BF16; kDescale and vDescale must be NULL) or one-byte e4m3fn elements (FA_DTYPE_FP8_E4M3; strides in
 *            bytes).  The layouts, stride rules and extent limits are the decode calls': what this call accepts, decode accepts
 *   dHead    64 or 128.  1 <= seqLenNew <= capacity: NOT capped at FA_DECODE_MAX_Q -- the same call fills the cache after a prefill
 *
 * Positions.  The rows appended are the rows decode's bottom-right mask treats as the query rows' own: the LAST seqLenNew rows of the
 * sequence, and kvLens[b] ALREADY counts them.  With L = min(kvLens[b], capacity), new row i goes to key position p = L - seqLenNew + i
 * and is written only if p >= 0.  kvLens[b] <= 0 writes nothing for that sequence (an inactive slot of a fixed-batch graph); NULL
 * kvLens = the capacity.  This differs from decode's clamp of the length into [1, capacity] only for kvLens[b] <= 0, where decode
 * reads key 0 and this call writes nothing.  One device tensor of lengths serves both calls of a step; this call writes no length.
 * kvLens, the descales and the table entries are DEVICE memory read BY THE KERNEL: the host never synchronises, and a replayed graph
 * sees the values of the moment.
 *
 * Paged.  Position p is row p % pageSize of page blockTable[b * tableStride + p / pageSize].  Only the entries of pages that receive
 * a row are read.  An entry outside [0, numPages) is NOT clamped (decode may clamp because it only reads; a clamped write would land
 * in another sequence's page): the rows that would go to such a page are skipped and nothing else is touched.  Two sequences that
 * write the same row of the same page: the winner is unspecified, the address never bad.  Page bases are 64-bit: pools above 2^32
 * bytes work.
 *
 * Values.  kv_dtype = FA_DTYPE_BF16: the 2-byte pattern is copied unchanged, NaN payloads and -0 included.
 * kv_dtype = FA_DTYPE_FP8_E4M3: the stored byte is the e4m3fn code of clamp(fp32(x) / descale[kvh], -448, 448): the correctly rounded
 * fp32 quotient, then ONE rounding to nearest even to e4m3fn, subnormals included.  The sign is kept on values that round to zero (-0
 * and negative underflow store 0x80); +-inf stores +-448 (0x7E / 0xFE); NaN stores a NaN code (0x7F or 0xFF).  A NULL descale is
 * 1.0; a descale that is not finite and positive gives unspecified bytes, never a bad address.  The reader's logical cache is then
 * K8 * kDescale[kvh], V8 * vDescale[kvh] (flash_attention_decode_fp8).
 *
 * Conventions.  Everything is validated before the launch; the calls never allocate, synchronise or print; the same inputs give the
 * same bytes (no atomics; every cache byte has one writer).  Rejected with the decode calls' codes for the same mistake: null pointers
 * (a NULL blockTable included) FA_ERR_NULL_POINTER; a base not aligned to 16 bytes, kvLens / blockTable / a descale not aligned to 4
 * FA_ERR_MISALIGNED; a stride that is not a multiple of 16 bytes or a row stride below dHead FA_ERR_BAD_STRIDE; batchSize, numHeadsKV
 * or seqLenK <= 0, seqLenNew < 1 or above the capacity, a capacity above 2^24, numPages <= 0, maxPagesPerSeq <= 0, pageSize < 16 or
 * not a power of two, tableStride < maxPagesPerSeq, one head's extent ((seqLenK + 192) x row stride; paged: pageSize x row stride)
 * of 2^31 bytes or more FA_ERR_BAD_SHAPE; dtype other than FA_DTYPE_BF16, kv_dtype other than FA_DTYPE_BF16 / FA_DTYPE_FP8_E4M3, or
 * a non-NULL descale with a bf16 cache FA_ERR_UNSUPPORTED_DTYPE; any other dHead FA_ERR_UNSUPPORTED_DHEAD.
 * Rotary embedding: flash_attention_rope_append* (below) are these calls with the rotation of K and of the step's Q fused in.
 * Not done here: fp8 new rows, per-token or per-block descales, writing kvLens.
 */
int flash_attention_kv_append(const void* Knew, const void* Vnew, void* K, void* V,
                              const int32_t* kvLens, const float* kDescale, const float* vDescale,
                              int batchSize, int numHeadsKV, int seqLenNew, int seqLenK, int dHead,
                              int dtype /* of Knew, Vnew: FA_DTYPE_BF16 */, int kv_dtype /* FA_DTYPE_BF16 | FA_DTYPE_FP8_E4M3 */,
                              const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sK, const fa_strides* sV,
                              void* stream);

int flash_attention_kv_append_paged(const void* Knew, const void* Vnew, void* Kpool, void* Vpool,
                                    const int32_t* kvLens, const int32_t* blockTable,
                                    const float* kDescale, const float* vDescale,
                                    int batchSize, int numHeadsKV, int seqLenNew,
                                    int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                    int dtype, int kv_dtype,
                                    const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sK, const fa_strides* sV,
                                    void* stream);

/*
 * flash_attention_extend, flash_attention_extend_paged -- CHUNKED PREFILL against the decode caches: seqLenQ new query rows per
 * sequence, 1 .. the capacity, against the caches flash_attention_decode* reads and flash_attention_kv_append* writes.  A chunk of a
 * chunked prefill, a prompt behind a cached prefix, a speculative draft longer than FA_DECODE_MAX_Q rows.  The argument lists are
 * flash_attention_decode_fp8's / flash_attention_decode_paged_fp8's, word for word, and like the _window calls the two entry points
 * serve all four cache forms: kv_dtype = FA_DTYPE_BF16 (kDescale and vDescale must be NULL) or FA_DTYPE_FP8_E4M3 (optional per-head
 * descales).
 *
 * Contract.  Everything not named below is the decode sibling's of the same form and kv_dtype: layouts, strides and the 2^31-byte
 * extent rules; kvLens, the descales and the table entries read by the kernel and clamped as decode clamps them; keys at and beyond the
 * length may hold anything; a pool may exceed 2^32 bytes; o_dtype F32, BF16 or F16, rounded once at the store; the optional LSE (the
 * same bits of O with or without it); the caller-owned workspace of flash_attention_decode_workspace_size(batchSize, numHeads,
 * seqLenQ, dHead, plan.num_splits) bytes (that function has no cap on seqLenQ and serves unchanged); the same bits run to run, no
 * atomics; validation before any launch; no allocation, no host synchronisation, nothing printed, graph-capturable.
 *
 * What differs from decode.
 *   seqLenQ  1 <= seqLenQ <= capacity (seqLenK, or maxPagesPerSeq * pageSize), not capped at FA_DECODE_MAX_Q.  batchSize * numHeads *
 *            seqLenQ and the grid must fit in an int32, and stay below FA_DECODE_MAX_WORKGROUPS as said there (2^24 rows of O under
 *            two forced splits are refused; under numSplits = 0 they run unsplit).  seqLenQ <= FA_DECODE_MAX_Q is legal and means what decode means: the result
 *            is then flash_attention_decode*'s of the same arguments and the same forced numSplits, bit for bit (O and LSE), so a
 *            serving engine may cross 16 rows from one step to the next
 *   mask     decode's, unchanged: kvLens[b] ALREADY counts the new rows (`kv_lens += Sq; append; extend` is one graph).  With
 *            len = clamp(kvLens[b], 1, capacity), row i sees k < max(len - seqLenQ + i + 1, 1) with is_causal and k < len without;
 *            "at least key 0" covers len < seqLenQ.  No NaN rows
 *   tiles    a row block (plan.rows_per_block packed rows g * seqLenQ + i of one K/V head; blocks are NOT head-aligned: row_blocks =
 *            ceil(G * seqLenQ / rows_per_block)) walks only the 128-key tiles one of its rows can see: ntb = ceil(max over the
 *            block's rows of the row's limit / 128); the tiles [0, ntb) are divided over numSplits in whole tiles by decode's formula
 *            (split s takes [ntb s / ns, ntb (s + 1) / ns)).  Under the causal mask the lower row blocks of a long chunk read less.
 *            A split past the end comes out empty (O = 0, LSE = -inf, weight 0), as in decode.  Paged and contiguous divide alike:
 *            flash_attention_extend_paged equals flash_attention_extend on a contiguous copy of the same pages with seqLenK = the
 *            capacity and the same numSplits, bit for bit
 *   plan     flash_attention_extend_plan: fa_decode_plan for these calls (seqLenK = the capacity).  grid = batchSize * numHeadsKV *
 *            row_blocks * num_splits.  numSplits = 0: decode's rule with units = batchSize * numHeadsKV * row_blocks -- a long chunk
 *            fills the chip by its units alone and runs unsplit
 *   precision  decode's: fp32 scores and softmax, weights as a bf16 hi + lo pair, fp32 accumulation, no fp16 anywhere and no range
 *            caveat on V; e4m3fn -> bf16 exactly, in registers, kDescale folded into the score scale and vDescale into the final 1 / l
 * Rejected before any launch: everything the decode sibling of the same form and kv_dtype rejects, with the same codes, except the
 * FA_DECODE_MAX_Q cap; seqLenQ > capacity FA_ERR_BAD_SHAPE; a non-NULL descale with a bf16 cache FA_ERR_UNSUPPORTED_DTYPE.
 * Not done here: fp8 Q, a backward, automatic routing from or to any existing call.  A per-sequence count of new rows
 * is flash_attention_extend_varlen's (below): here every sequence brings seqLenQ rows.  A sliding window is the _window calls' (below).
 */
int flash_attention_extend_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                int o_dtype, int numSplits /* 0 = the library chooses */, fa_decode_plan* plan);

int flash_attention_extend(const void* Q, const void* K, const void* V, void* O, float* LSE,
                           const int32_t* kvLens, const float* kDescale, const float* vDescale, void* workspace,
                           int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                           float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                           const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                           void* stream);

int flash_attention_extend_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                 const int32_t* kvLens, const int32_t* blockTable,
                                 const float* kDescale, const float* vDescale, void* workspace,
                                 int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                 int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                 float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                 const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                 void* stream);

/*
 * flash_attention_extend_varlen, flash_attention_extend_paged_varlen -- RAGGED chunked prefill against the decode caches: every
 * sequence of the batch brings its OWN number of new query rows, 0 .. totalQ, given in device memory.  One step of a continuous-batching
 * engine -- some sequences decoding (1 row, or a short draft), some in the middle of a chunked prefill, some idle -- is one call on the
 * token-major tensors the engine holds, with no regrouping and no padding.  The argument lists are flash_attention_extend's /
 * flash_attention_extend_paged's with seqLenQ replaced by totalQ and cuSeqlensQ added directly before kvLens; both calls serve bf16 and
 * e4m3fn caches through kv_dtype.
 *
 * Contract.  Everything not named below is flash_attention_extend*'s of the same form and kv_dtype: cache layouts, strides and extent
 * rules; kvLens, the descales and the table entries read by the kernel and clamped as there; keys at and beyond the length may hold
 * anything; pools may exceed 2^32 bytes; o_dtype F32, BF16 or F16, rounded once; the optional LSE (the same bits of O with or without
 * it); no atomics, the same bits run to run; validation before any launch; no allocation, no host synchronisation, nothing printed,
 * graph-capturable.
 *   Q, O     PACKED BY TOKEN: row t of totalQ rows, head h, is at t * strideS + h * strideH elements (strideB is ignored, whatever it
 *            holds).  NULL strides = the token-major [totalQ, numHeads, dHead] an engine holds: strideS = numHeads * dHead, strideH = dHead
 *   LSE      optional dense fp32 [numHeads, totalQ]
 *   totalQ   a HOST-side BOUND on the packed rows (the allocation; fixed under a captured graph), >= 1 and NOT capped at the capacity.
 *            The rows in use are given by cuSeqlensQ
 *   cuSeqlensQ  DEVICE pointer to int32[batchSize + 1], 4-byte aligned, required; read by the kernels, never by the host.  With
 *            q0 = clamp(cuSeqlensQ[b], 0, totalQ) and q1 = clamp(cuSeqlensQ[b + 1], q0, totalQ), sequence b owns the rows [q0, q1):
 *            sq_b = q1 - q0 new rows.  sq_b = 0 is legal (an idle slot): nothing of that sequence is computed, and its kvLens entry and
 *            table row are not read.  Rows owned by no sequence -- in particular [cuSeqlensQ[batchSize], totalQ) -- are NOT written:
 *            not O, not the LSE.  Entries that are not non-decreasing give an unspecified result, but every access stays inside the
 *            totalQ rows
 *   mask, tiles, arithmetic  flash_attention_extend's PER SEQUENCE, with sq_b where it has seqLenQ.  kvLens[b] ALREADY counts the new
 *            rows (`kv_lens += q_lens; append; attend` is one graph); with len = clamp(kvLens[b], 1, capacity) row i of sequence b sees
 *            k < max(len - sq_b + i + 1, 1) with is_causal and k < len without; sq_b > len keeps key 0.  The packed rows of a K/V head
 *            are g * sq_b + i, in ceil(G * sq_b / rows_per_block) row blocks; a row block walks only the ntb tiles one of its rows can
 *            see, divided over numSplits by decode's formula
 *   seam     the O and LSE of sequence b are, BIT FOR BIT, what flash_attention_extend* returns for that sequence alone: batchSize = 1,
 *            seqLenQ = sq_b, the same cache form and the same FORCED numSplits -- and for sq_b <= FA_DECODE_MAX_Q therefore
 *            flash_attention_decode*'s as well.  (The per-row text of the kernel is the same; only the unit decoding and the addresses
 *            differ.)  flash_attention_extend_paged_varlen equals flash_attention_extend_varlen on a contiguous copy of the same pages
 *   workspace  flash_attention_decode_workspace_size(1, numHeads, totalQ, dHead, plan.num_splits) bytes -- that function, unchanged:
 *            the slabs are [numSplits][numHeads * totalQ] rows.  Not needed (may be NULL) when the plan says num_splits == 1
 *   plan     flash_attention_extend_varlen_plan: fa_decode_plan for these calls (seqLenK = the capacity).  rows_per_block is
 *            flash_attention_extend_plan's.  row_blocks is a BOUND over the whole batch, which the host can compute without the offsets:
 *            NB = floor((G * totalQ + batchSize * (rows_per_block - 1)) / rows_per_block) >= sum_b ceil(G * sq_b / rows_per_block).
 *            grid = numHeadsKV * NB * num_splits; a workgroup finds its sequence and row block from cuSeqlensQ by itself (no extra
 *            launch, no workspace at num_splits == 1) and one beyond the real total returns at once.  combine_grid = numHeads * totalQ.
 *            numSplits = 0: flash_attention_extend_plan's rule and constants with units = numHeadsKV * NB; that rule is not measured
 *            for mixed batches
 * Limits.  numHeads * totalQ and the grid must fit in an int32 and respect FA_DECODE_MAX_WORKGROUPS; batchSize <= FA_VARLEN_MAX_BATCH;
 *            totalQ >= 1.
 * Rejected before any launch: everything flash_attention_extend* of the same form rejects, with the same codes and in the same order,
 * except its seqLenQ > capacity; a NULL cuSeqlensQ FA_ERR_NULL_POINTER; one not aligned to 4 bytes FA_ERR_MISALIGNED; totalQ < 1,
 * batchSize > FA_VARLEN_MAX_BATCH and the int32 limits FA_ERR_BAD_SHAPE.
 * Not done here: a per-unit choice of rows_per_block, reordering units by length, fp8 Q, routing.  A sliding window
 * is the _window calls' (below).
 */
#define FA_VARLEN_MAX_BATCH 1024    /* sequences per ragged call: the unit lookup scans them 64 at a time, 16 steps at the most */

int flash_attention_extend_varlen_plan(int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                       int o_dtype, int numSplits /* 0 = the library chooses */, fa_decode_plan* plan);

int flash_attention_extend_varlen(const void* Q, const void* K, const void* V, void* O, float* LSE,
                                  const int32_t* cuSeqlensQ, const int32_t* kvLens,
                                  const float* kDescale, const float* vDescale, void* workspace,
                                  int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                  float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                  const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                  void* stream);

int flash_attention_extend_paged_varlen(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                        const int32_t* cuSeqlensQ, const int32_t* kvLens, const int32_t* blockTable,
                                        const float* kDescale, const float* vDescale, void* workspace,
                                        int batchSize, int numHeads, int numHeadsKV, int totalQ,
                                        int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                        float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                        const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                        void* stream);

/*
 * flash_attention_extend_window, flash_attention_extend_paged_window, flash_attention_extend_varlen_window,
 * flash_attention_extend_paged_varlen_window -- chunked prefill and the ragged call with a SLIDING WINDOW: the window of
 * flash_attention_decode_window on every member of the split-KV family, so that a sliding-window model (Mistral, Gemma, the local
 * layers of gpt-oss) prefills a chunk against the cache and runs the mixed decode + prefill step with this library.  Each call takes
 * its sibling's argument list (flash_attention_extend, _extend_paged, _extend_varlen, _extend_paged_varlen) with windowSize directly
 * after numSplits, as the decode _window calls do, and serves all four cache forms.  Everything not named here is the sibling's.
 *
 * Mask (decode's, unchanged).  Per sequence, with len = clamp(kvLens[b], 1, capacity) and Sq the sequence's row count (seqLenQ, or
 * sq_b from cuSeqlensQ): limC_i = max(len - Sq + i + 1, 1), lo_i = max(limC_i - windowSize, 0); row i sees lo_i <= k < limC_i with
 * is_causal and lo_i <= k < len without.  Every row sees a key.  windowSize = 0 IS the sibling call: the same launches (the sibling's
 * kernels) and the same bits.  windowSize >= capacity masks nothing and gives the sibling's bits as well.
 *
 * Below the window.  first(b) = lo_0.  Keys below first(b) never enter the result and may hold NaN, inf, stale data or any fp8 byte;
 * paged: a page wholly below first(b) is never read and neither is its blockTable entry, which may be any int32.  Keys in
 * [first(b), len) are data: a key one row block does not see is one another reads.
 *
 * Tiles: a range PER ROW BLOCK.  A row block (plan.rows_per_block packed rows g * Sq + i of one K/V head, not head-aligned) whose
 * rows are the query rows qmin .. qmax of the chunk walks the 128-key tiles [tlo_b, ntb): ntb as in the sibling (the block's largest
 * limit), tlo_b = firstb / 128 with firstb = max(max(len - Sq + qmin + 1, 1) - windowSize, 0), and qmin = 0 when the block reaches
 * into the next head, else the query row of its first packed row.  For Sq > FA_DECODE_MAX_Q that is exactly the hull of the tiles
 * that hold a key some row of the block sees: a long windowed chunk reads about windowSize + rows_per_block keys per block, not the
 * whole prefix.  The block's tiles are divided over numSplits by decode's formula (split s takes
 * [tlo_b + (ntb - tlo_b) s / ns, tlo_b + (ntb - tlo_b) (s + 1) / ns)); a split past the end comes out empty.
 *   Sq <= FA_DECODE_MAX_Q: qmin = 0 for every block -- the range is decode's [first(b) / 128, ntb), so flash_attention_extend_window is
 *   flash_attention_decode_window of the same arguments and the same forced numSplits, bit for bit (O and LSE).
 * Known cost: row blocks are not head-aligned.  A block that straddles two heads of a long windowed chunk holds rows 0 and Sq - 1 and
 * walks from lo_0 to len, the whole chunk's span.  That happens only when G * Sq is no multiple of rows_per_block (for a chunk longer
 * than a block: when Sq is none).
 *
 * Seams, bit for bit (O and LSE, under the same forced numSplits): the paged calls equal the contiguous ones on a contiguous copy of
 * the same pages; sequence b of a ragged call equals flash_attention_extend*_window on that sequence alone (batchSize = 1, seqLenQ =
 * sq_b), and for sq_b <= FA_DECODE_MAX_Q flash_attention_decode*_window; rows no sequence owns are not written.
 *
 * Plan.  flash_attention_extend_plan_window / flash_attention_extend_varlen_plan_window: the sibling's plan with tiles = min(the
 * capacity's tiles, ceil((windowSize + Sq - 1) / 128) + 1), Sq = seqLenQ or totalQ, as in flash_attention_decode_plan_window; the
 * split count follows by flash_attention_extend_plan's unchanged rule and constants.  That rule is NOT measured for windowed chunks
 * (DESIGN.md section 22).  flash_attention_extend_plan and flash_attention_extend_varlen_plan are these with windowSize = 0;
 * windowSize >= seqLenK plans as no window does.  rows_per_block is the sibling's.  The workspace functions are unchanged.
 *
 * Rejected before any launch: everything the sibling rejects, with the same codes and in the same order; windowSize < 0
 * FA_ERR_BAD_SHAPE.
 * Not done here: a right window, per-head windows, ring-buffer caches, windows and attention sinks in the prefill / backward kernels.
 */
int flash_attention_extend_plan_window(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                       int o_dtype, int numSplits /* 0 = the library chooses */, int windowSize,
                                       fa_decode_plan* plan);

int flash_attention_extend_varlen_plan_window(int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                              int o_dtype, int numSplits /* 0 = the library chooses */, int windowSize,
                                              fa_decode_plan* plan);

int flash_attention_extend_window(const void* Q, const void* K, const void* V, void* O, float* LSE,
                                  const int32_t* kvLens, const float* kDescale, const float* vDescale, void* workspace,
                                  int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                  float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                  int windowSize,
                                  const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                  void* stream);

int flash_attention_extend_paged_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                        const int32_t* kvLens, const int32_t* blockTable,
                                        const float* kDescale, const float* vDescale, void* workspace,
                                        int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                        int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                        float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                        int windowSize,
                                        const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                        void* stream);

int flash_attention_extend_varlen_window(const void* Q, const void* K, const void* V, void* O, float* LSE,
                                         const int32_t* cuSeqlensQ, const int32_t* kvLens,
                                         const float* kDescale, const float* vDescale, void* workspace,
                                         int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                         float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                         int windowSize,
                                         const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                         void* stream);

int flash_attention_extend_paged_varlen_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                               const int32_t* cuSeqlensQ, const int32_t* kvLens, const int32_t* blockTable,
                                               const float* kDescale, const float* vDescale, void* workspace,
                                               int batchSize, int numHeads, int numHeadsKV, int totalQ,
                                               int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                               float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype,
                                               int numSplits, int windowSize,
                                               const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                               void* stream);

/*
 * flash_attention_sink_decode, _decode_paged, _extend, _extend_paged, _extend_varlen, _extend_paged_varlen -- ATTENTION SINKS in the
 * K/V-cache calls: a learned logit per query head that takes part in every row's softmax as one more key whose value is 0 (the
 * sink-trained GQA models: alternating full and windowed layers).  Each call is its _window twin -- flash_attention_decode_window,
 * flash_attention_decode_paged_window, flash_attention_extend_window, flash_attention_extend_paged_window,
 * flash_attention_extend_varlen_window, flash_attention_extend_paged_varlen_window -- with one argument more, directly after vDescale:
 *   sinks    [numHeads] fp32 (device memory), or NULL.  One logit per QUERY head: packed row g * Sq + i of K/V head kvh uses
 *            sinks[kvh * (numHeads / numHeadsKV) + g].  Natural-log units, NOT multiplied by scale.  Read by the kernel, like kvLens
 *            and the descales: no host synchronisation, and a replayed graph sees the values of the moment
 * For a row with the visible scores s_k = scale q.k:
 *   O   = sum_k exp(s_k) v_k / (sum_k exp(s_k) + exp(sink_h))
 *   LSE = ln(sum_k exp(s_k) + exp(sink_h))                              (the returned LSE includes the sink)
 * The sink is visible to every row whatever the mask, the window and the length, and it is counted once per row, not once per split.
 * sink = -inf is "no sink": O and LSE are, bit for bit, those of the call without sinks.  A finite value of any size gives finite O
 * and LSE (a sink far above every score: O = 0, LSE = sink).  +inf and NaN are the caller's error: the row's O and LSE are then NaN.
 *
 * sinks = NULL is the _window twin itself: the same launches, the same bits.  windowSize = 0: no window.  Plans and workspace sizes
 * do not depend on sinks: flash_attention_decode_plan_window / flash_attention_extend_plan_window /
 * flash_attention_extend_varlen_plan_window and flash_attention_decode_workspace_size describe these calls.  The launches are the
 * twin's in number, grids and LDS: under one split the split kernel's SINK form, under more the twin's split kernel (the slabs hold
 * the keys alone) and the combine kernel's SINK form.  Every equality of the twins holds with sinks too: paged = contiguous on a copy
 * of the same pages, seqLenQ <= FA_DECODE_MAX_Q chunked prefill = decode, a ragged sequence = the uniform call on it alone, and
 * nothing beyond the length or below the window is read.
 *
 * Rejected before any launch: everything the twin rejects, with the same codes and in the same order; a sinks pointer not aligned
 * to 4 bytes FA_ERR_MISALIGNED, directly after the twin's alignment checks of kvLens, cuSeqlensQ, blockTable and the descales.
 * Not done here: sinks in flash_attention / flash_attention_ex and in the backward, per-row or per-token sinks, bf16 sink arrays.
 */
int flash_attention_sink_decode(const void* Q, const void* K, const void* V, void* O, float* LSE,
                                const int32_t* kvLens, const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                int windowSize,
                                const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                void* stream);

int flash_attention_sink_decode_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                      const int32_t* kvLens, const int32_t* blockTable,
                                      const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                      int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                      int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                      float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                      int windowSize,
                                      const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                      void* stream);

int flash_attention_sink_extend(const void* Q, const void* K, const void* V, void* O, float* LSE,
                                const int32_t* kvLens, const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                                float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                int windowSize,
                                const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                void* stream);

int flash_attention_sink_extend_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                      const int32_t* kvLens, const int32_t* blockTable,
                                      const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                      int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                      int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                      float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                      int windowSize,
                                      const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                      void* stream);

int flash_attention_sink_extend_varlen(const void* Q, const void* K, const void* V, void* O, float* LSE,
                                       const int32_t* cuSeqlensQ, const int32_t* kvLens,
                                       const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                       int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                       float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                                       int windowSize,
                                       const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                       void* stream);

int flash_attention_sink_extend_paged_varlen(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                             const int32_t* cuSeqlensQ, const int32_t* kvLens, const int32_t* blockTable,
                                             const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                             int batchSize, int numHeads, int numHeadsKV, int totalQ,
                                             int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                             float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype,
                                             int numSplits, int windowSize,
                                             const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                             void* stream);

/*
 * flash_attention_tree, flash_attention_tree_paged -- TREE-MASKED VERIFICATION for speculative decoding (Medusa, EAGLE, SpecInfer and
 * the tree modes of the serving engines): one step verifies a TREE of draft tokens, each node attending to the cached prefix and to its
 * own ancestors only.  Each call is flash_attention_sink_decode / flash_attention_sink_decode_paged without is_causal and with one
 * argument more, directly after sinks:
 *   treeMask [batchSize, seqLenQ] uint64 (device memory), dense: word (b, i) is treeMask[b * seqLenQ + i].  Read by the kernel, like
 *            kvLens: no host synchronisation, and a replayed graph sees the words of the moment (dynamic trees change every step).
 *   seqLenQ  1 <= seqLenQ <= FA_TREE_MAX_Q draft nodes per sequence.  kv_dtype selects a bf16 or an e4m3fn cache: all four cache forms.
 * The seqLenQ rows are the draft nodes of the step.  The caller HAS ALREADY APPENDED them (flash_attention_kv_append*) and kvLens counts
 * them: with len = kvLens[b] and base = len - seqLenQ, node j is key base + j, and node i is query row i of every query head.  Bit j of
 * word (b, i) set means: row i sees node j.  The rule, per row i and key k, with lim_i = max(len - seqLenQ + i + 1, 1) and
 * lo_i = max(lim_i - windowSize, 0) (windowSize = 0: lo_i = 0) exactly as the twin computes them under is_causal = true: k is visible iff
 *   lo_i <= k < lim_i                                                        (k is visible to the causal twin), and
 *   k < base, or bit k - base of the row's word is set, or k == lim_i - 1    (the prefix, a marked node, or the row's own key).
 * So: the own key is always visible and no row is empty; the len < seqLenQ clamp still holds (a row clamped to key 0 sees key 0 alone);
 * bits j > i and bits >= seqLenQ are ignored; an all-ones word, or a chain (bits 0 .. i), is the causal twin.  The window rule stays
 * INDEX-based: it counts positions in the cache, not tree depth (a node's window reaches windowSize keys back from its own slot base + i,
 * siblings' slots included in the count though not in the sum).  sinks apply as in the twin; sinks = NULL means no sinks.  Draft K/V rows
 * are data -- other rows may see them -- and must be finite, as any visible key must be.
 *
 * Equalities (bit for bit, O and LSE, at the same windowSize, sinks and forced numSplits): a chain or all-ones mask is
 * flash_attention_sink_decode* (seqLenQ <= FA_DECODE_MAX_Q) or flash_attention_sink_extend* (above) with is_causal = true; the paged call is the
 * contiguous call on a copy of the same pages; garbage in the ignored bits changes nothing; sinks = NULL is a vector of -inf.  The
 * launches are the twin's in number, grids and LDS -- seqLenQ <= FA_DECODE_MAX_Q decode's, 17 .. FA_TREE_MAX_Q chunked prefill's:
 * flash_attention_tree_plan forwards to flash_attention_decode_plan_window or flash_attention_extend_plan_window by that rule, and
 * flash_attention_decode_workspace_size serves unchanged.  The split kernel is the TREE form under any split count (only the key tiles that
 * reach into [base, len) take the masked select); the combine kernel is the twin's.
 *
 * Rejected before any launch: everything the sink twin rejects, with the same codes and in the same order; a NULL treeMask
 * FA_ERR_NULL_POINTER (with the other pointers); a treeMask not aligned to 8 bytes FA_ERR_MISALIGNED, directly after the sinks check;
 * seqLenQ > FA_TREE_MAX_Q FA_ERR_BAD_SHAPE (with the other shape checks; flash_attention_tree_plan likewise).
 * Not done here: the ragged form (a tree size per sequence); trees above 64 nodes; masks in the prefill forward and in the backward.
 * (Rotary positions by tree depth and the acceptance of the verified path: flash_attention_rope_append_pos and
 * flash_attention_kv_accept, below.)
 */
#define FA_TREE_MAX_Q 64            /* draft nodes per sequence: one uint64 mask word per node */

int flash_attention_tree(const void* Q, const void* K, const void* V, void* O, float* LSE,
                         const int32_t* kvLens, const float* kDescale, const float* vDescale, const float* sinks,
                         const uint64_t* treeMask, void* workspace,
                         int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead,
                         float scale, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                         int windowSize,
                         const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                         void* stream);

int flash_attention_tree_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                               const int32_t* kvLens, const int32_t* blockTable,
                               const float* kDescale, const float* vDescale, const float* sinks,
                               const uint64_t* treeMask, void* workspace,
                               int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                               int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                               float scale, int dtype /* of Q */, int kv_dtype, int o_dtype, int numSplits,
                               int windowSize,
                               const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                               void* stream);

int flash_attention_tree_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, int o_dtype,
                              int numSplits, int windowSize, fa_decode_plan* plan);

/*
 * flash_attention_cascade_decode, flash_attention_cascade_decode_paged -- SHARED-PREFIX (cascade) decode: the sequences of the batch share
 * one prefix (a system prompt, n samples of one prompt, beams, best-of-n candidates), and the call reads that prefix ONCE per row block
 * of the whole batch instead of once per sequence.  The logical cache of sequence b is [ shared[0 : ls) ; unique_b[0 : len_b) ]:
 *   Kshared, Vshared  [numHeadsKV, seqLenShared, dHead], the cache's type; strides sKshared / sVshared (strideB is not read).  Paged: one
 *            pool serves both parts; sharedTable is int32[maxSharedPages] (device memory), the shared part's pages in order, and
 *            blockTable holds the SUFFIX pages (an engine passes its table offset by the shared pages: the shared part is whole pages,
 *            the tail of a prompt that does not fill a page lives in the suffix).  Entries are read and clamped by the kernel as in
 *            flash_attention_decode_paged: only those of pages that hold a key below the length, each into [0, numPages)
 *   sharedLen  int32[1] (device memory): ls = sharedLen[0] clamped into [1, seqLenShared] (paged: maxSharedPages * pageSize) on the
 *            device; NULL = the capacity.  Read by the kernel like kvLens: a replayed graph sees the value of the moment
 *   K, V, kvLens, blockTable  the sequences' own suffixes, as in flash_attention_decode*: len_b = kvLens[b] clamped into [1, seqLenK]
 *   mask     the seqLenQ (1 .. FA_DECODE_MAX_Q) query rows are the last rows of the logical sequence.  Every row sees ALL ls shared
 *            keys -- there is no mask on the shared part -- and of its own suffix what flash_attention_decode shows it on that suffix
 *            alone: the bottom-right is_causal rule, "at least key 0" included.  So whenever len_b >= seqLenQ the result is
 *            flash_attention_decode with is_causal on the concatenated cache of length ls + len_b.  The LSE is over all visible keys
 *            of both parts.  Keys at and beyond ls in the shared cache, keys beyond len_b in the suffixes and pages not read may hold
 *            anything
 *   kv_dtype FA_DTYPE_BF16, or FA_DTYPE_FP8_E4M3 with kDescale / vDescale [numHeadsKV] (NULL = 1): ONE pair for both parts.  A
 *            non-NULL descale with a bf16 cache is FA_ERR_UNSUPPORTED_DTYPE
 *   sinks    NULL, or [numHeads] fp32 attention sinks; they join once per row, as in flash_attention_sink_decode
 *   numSplitsShared, numSplitsUnique  0 = the library chooses, from shapes only (shared: flash_attention_extend's rule with
 *            numHeadsKV * ceil(batchSize * G * seqLenQ / rows_per_block) units and the tiles of seqLenShared; unique:
 *            flash_attention_decode's, clamped into [2, 32]; the shared count is then capped at FA_DECODE_MAX_SPLITS - unique).  Forced
 *            values are taken as given: numSplitsUnique >= 2 (the suffix kernel writes partial results under more than one split only)
 *            and the sum at most FA_DECODE_MAX_SPLITS
 *   plan     flash_attention_cascade_plan (seqLenShared, seqLenK: the capacities): `shared` and `unique` describe the two split
 *            launches (shared.grid = numHeadsKV * row_blocks * num_splits, no batch factor), num_splits is their sum
 *   workspace  flash_attention_decode_workspace_size(batchSize, numHeads, seqLenQ, dHead, plan.num_splits) bytes, ALWAYS required
 * Three launches on the stream, no host synchronisation, graph-capturable: the shared-prefix form of the split-KV kernel (packed rows
 * (b * G + g) * seqLenQ + i across the batch, rows_per_block of them per workgroup) into partial results [0, ns_s); decode's own kernel
 * on the suffixes into [ns_s, ns_s + ns_u); the combine kernel of flash_attention_decode over all of them, in a fixed order: the same
 * bits run to run.  The paged call is the contiguous call on gathered copies under the same split counts, bit for bit.
 *
 * Rejected before any launch: everything flash_attention_decode_window / _paged_window of the same kv_dtype rejects, with the same
 * codes and in the same order, the new arguments at their kind's place: NULL Kshared / Vshared / sharedTable FA_ERR_NULL_POINTER with
 * the other pointers and a NULL workspace where decode asks for its own; sharedLen or sinks not 4-byte aligned FA_ERR_MISALIGNED with
 * the other arrays; seqLenShared <= 0 or > 2^24, maxSharedPages <= 0, numSplitsUnique == 1, a negative count, a sum above
 * FA_DECODE_MAX_SPLITS (a count left to the library needs room for 1 shared and 2 unique) or a shared grid at or above
 * FA_DECODE_MAX_WORKGROUPS FA_ERR_BAD_SHAPE; the strides and extents of the shared tensors are checked as those of K / V.
 * Not done here: several prefix groups in one call and multi-level cascades (call once per group), windows, tree masks,
 * seqLenQ > FA_DECODE_MAX_Q, a ragged form, a stand-alone merge of (O, LSE) pairs.
 */
typedef struct fa_cascade_plan {
    fa_decode_plan shared;   /* the shared-prefix launch */
    fa_decode_plan unique;   /* decode's launch on the suffixes */
    int num_splits;          /* shared.num_splits + unique.num_splits: what the workspace and the combine are sized by */
} fa_cascade_plan;

int flash_attention_cascade_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenShared, int seqLenK, int dHead,
                                 int o_dtype, int numSplitsShared, int numSplitsUnique, fa_cascade_plan* plan);

int flash_attention_cascade_decode(const void* Q, const void* Kshared, const void* Vshared, const void* K, const void* V, void* O,
                                   float* LSE, const int32_t* sharedLen, const int32_t* kvLens,
                                   const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                   int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenShared, int seqLenK, int dHead,
                                   float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype,
                                   int numSplitsShared, int numSplitsUnique,
                                   const fa_strides* sQ, const fa_strides* sKshared, const fa_strides* sVshared,
                                   const fa_strides* sK, const fa_strides* sV, const fa_strides* sO, void* stream);

int flash_attention_cascade_decode_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                         const int32_t* sharedLen, const int32_t* kvLens,
                                         const int32_t* sharedTable, const int32_t* blockTable,
                                         const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                         int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                         int numPages, int pageSize, int maxSharedPages, int maxPagesPerSeq, int64_t tableStride,
                                         int dHead, float scale, bool is_causal, int dtype /* of Q */, int kv_dtype, int o_dtype,
                                         int numSplitsShared, int numSplitsUnique,
                                         const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                         void* stream);

/*
 * flash_attention_kv_append_varlen, flash_attention_kv_append_paged_varlen -- the RAGGED cache append: flash_attention_kv_append /
 * _paged with Knew / Vnew packed by token -- [totalQ, numHeadsKV, dHead] bf16 on the stride rule of flash_attention_extend_varlen's Q
 * (row t, K/V head h at t * strideS + h * strideH; strideB ignored; NULL = dense token-major) -- seqLenNew replaced by totalQ and
 * cuSeqlensQ (that call's: the same device tensor serves both) added directly before kvLens.  Everything not named here is the
 * uniform call's of the same form and kv_dtype.
 *   positions  per sequence, with L = min(kvLens[b], capacity) and sq_b from cuSeqlensQ: new row i goes to position L - sq_b + i when
 *            that is >= 0 (sq_b > L: the leading rows are dropped); L <= 0 or sq_b = 0 writes nothing; tokens owned by no sequence are
 *            not read.  Table entries outside [0, numPages) are skipped, never clamped
 *   values   the uniform call's: a bit copy, or / descale, saturation at +-448, one rounding to nearest even and the NaN rule
 *   seam     the bytes written for sequence b are exactly those of flash_attention_kv_append* called for that sequence alone with
 *            seqLenNew = sq_b; every other byte of the cache keeps its value.  One launch writes K and V, with vector stores only
 * totalQ >= 1 is not capped at the capacity; batchSize <= FA_VARLEN_MAX_BATCH.  Rejected before any launch: everything the uniform
 * call rejects, with the same codes, except its seqLenNew > capacity; a NULL cuSeqlensQ FA_ERR_NULL_POINTER, one not aligned to 4
 * bytes FA_ERR_MISALIGNED, batchSize > FA_VARLEN_MAX_BATCH FA_ERR_BAD_SHAPE.
 */
int flash_attention_kv_append_varlen(const void* Knew, const void* Vnew, void* K, void* V,
                                     const int32_t* cuSeqlensQ, const int32_t* kvLens, const float* kDescale, const float* vDescale,
                                     int batchSize, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                     int dtype /* of Knew, Vnew: FA_DTYPE_BF16 */, int kv_dtype /* FA_DTYPE_BF16 | FA_DTYPE_FP8_E4M3 */,
                                     const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sK, const fa_strides* sV,
                                     void* stream);

int flash_attention_kv_append_paged_varlen(const void* Knew, const void* Vnew, void* Kpool, void* Vpool,
                                           const int32_t* cuSeqlensQ, const int32_t* kvLens, const int32_t* blockTable,
                                           const float* kDescale, const float* vDescale,
                                           int batchSize, int numHeadsKV, int totalQ,
                                           int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                           int dtype, int kv_dtype,
                                           const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sK, const fa_strides* sV,
                                           void* stream);

/*
 * flash_attention_rope_append, _paged, _varlen, _paged_varlen -- the cache append with the ROTARY EMBEDDING fused in: each is its
 * flash_attention_kv_append* twin plus the step's query rows and a cos / sin table.  One launch rotates the new K rows at their cache
 * positions and stores them into the K cache, appends the new V rows exactly as the twin does, and rotates the Q rows at the same
 * positions into Qout.  A step is `kv_lens += Sq; rope_append; decode | extend` (ragged: `kv_lens += q_lens; rope_append_varlen;
 * extend_varlen`) on one device tensor of lengths: one graph, no host synchronisation, no rotated K in memory besides the cache.
 * Everything not named here -- Knew, Vnew, the caches, kvLens, the table, the descales, their strides and limits -- is the twin's.
 *   Q, Qout  bf16 [batchSize, numHeads, seqLenNew, dHead]; ragged: packed by token, [totalQ, numHeads, dHead], on the stride rule of
 *            flash_attention_extend_varlen's Q.  sQ / sQout: element strides or NULL (dense); the last dimension is contiguous, so
 *            the Q slice of a fused QKV projection passes without a copy.  Qout may be the very same view as Q (in place: same
 *            base, same strides); any other overlap is unspecified.  numHeads is a multiple of numHeadsKV
 *   cosSin   fp32 [maxPos, rotDim], device memory, dense, base aligned to 16 bytes: row p holds cos(p theta_j) for j < rotDim / 2,
 *            then sin(p theta_j) -- the common cos_sin_cache layout.  The call never computes a sine: frequency scaling (NTK, YaRN,
 *            ...) is whatever the caller put into the table.  Read BY THE KERNEL
 *   rotDim   a multiple of 16, 16 <= rotDim <= dHead (partial rotary): the columns >= rotDim pass through unrotated
 *   maxPos   >= the capacity (seqLenK; paged: maxPagesPerSeq * pageSize): every position the kernel can form is then inside the
 *            table, and nothing is clamped on the device
 *   interleaved  0: NeoX / half-split pairs (j, j + rotDim / 2); 1: GPT-J pairs (2j, 2j + 1).  Both with angle index j
 *
 * Positions.  K and V: the twin's rule unchanged -- L = min(kvLens[b], capacity), row i goes to p = L - seqLenNew + i, written iff
 * p >= 0; L <= 0 writes nothing; a table entry outside [0, numPages) skips the K / V rows of its page (their Q rows are still
 * written).  Q: EVERY row of every sequence is written (ragged: every token a sequence owns; tokens nobody owns are neither read nor
 * written), rotated at pq = max(clamp(kvLens[b], 1, capacity) - seqLenNew + i, 0): the position decode's and extend's bottom-right mask
 * gives the row, their "at least key 0" rule for kvLens[b] < seqLenNew and their clamp of an inactive slot included.  For every row
 * whose K is written pq = p.  NULL kvLens = the capacity.
 *
 * Values, to the bit.  x1, x2: the pair as fp32 (exact from bf16); c, s: the table's cos and sin of (position, j).
 *     y1 = fmaf(x1, c, -(x2 * s)),  y2 = fmaf(x2, c, x1 * s)      the lone product rounded to fp32 first, the other fused
 * then y is rounded ONCE to bf16, to nearest even.  That bf16 value is Qout's element.  For K it goes through exactly the twin's
 * value rule: a bit copy into a bf16 cache; divided by the descale, saturated at +-448, rounded once, with the twin's NaN rule, into
 * an e4m3fn cache.  So flash_attention_rope_append* == flash_attention_kv_append* applied to the bf16 rotation of Knew, byte for byte.
 * The columns >= rotDim of K and all of V have the twin's bits (NaN payloads, -0); the columns >= rotDim of Q are a bit copy.  NaN in
 * gives NaN out, the pattern unspecified.  With cos = 1, sin = 0 a finite x comes back with its value; -0 may lose its sign (-0 + +0).
 *
 * Conventions: the twin's -- validated before the launch; no allocation, no synchronisation, nothing printed; one writer per byte.
 * Rejected with the twin's codes for the twin's mistakes, in the twin's order, the new checks beside the twin's of the same kind:
 * a NULL Q, Qout or cosSin FA_ERR_NULL_POINTER; one of them not aligned to 16 bytes FA_ERR_MISALIGNED; numHeads <= 0, not a multiple
 * of numHeadsKV, numHeads * (numHeads / numHeadsKV) >= 2^31 or batchSize * numHeads > INT32_MAX / 2 FA_ERR_BAD_SHAPE (with the
 * twin's shape checks); then, after the dHead check, rotDim not a multiple of 16 or outside [16, dHead] FA_ERR_BAD_SHAPE, maxPos
 * below the capacity FA_ERR_BAD_SHAPE, interleaved neither 0 nor 1 FA_ERR_BAD_FLAGS; a stride of Q or Qout that is not a multiple of
 * 16 bytes, or a row stride below dHead, FA_ERR_BAD_STRIDE (after the twin's strides).  The grid limit is the twin's.
 * Not done here: absolute position ids (per-row offsets: flash_attention_rope_append_pos, below), sines computed on the device, fp8 or
 * fp32 new rows, per-token descales, writing kvLens, rotary embedding in flash_attention() or the backward, dHead other than 64 / 128.
 */
int flash_attention_rope_append(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* K, void* V,
                                const float* cosSin, const int32_t* kvLens, const float* kDescale, const float* vDescale,
                                int batchSize, int numHeads, int numHeadsKV, int seqLenNew, int seqLenK, int dHead,
                                int rotDim, int maxPos, int interleaved /* 0 half-split pairs | 1 adjacent pairs */,
                                int dtype /* of Q, Knew, Vnew, Qout: FA_DTYPE_BF16 */, int kv_dtype /* FA_DTYPE_BF16 | FA_DTYPE_FP8_E4M3 */,
                                const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sQout,
                                const fa_strides* sK, const fa_strides* sV, void* stream);

int flash_attention_rope_append_paged(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                      const float* cosSin, const int32_t* kvLens, const int32_t* blockTable,
                                      const float* kDescale, const float* vDescale,
                                      int batchSize, int numHeads, int numHeadsKV, int seqLenNew,
                                      int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                      int rotDim, int maxPos, int interleaved, int dtype, int kv_dtype,
                                      const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sQout,
                                      const fa_strides* sK, const fa_strides* sV, void* stream);

int flash_attention_rope_append_varlen(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* K, void* V,
                                       const float* cosSin, const int32_t* cuSeqlensQ, const int32_t* kvLens,
                                       const float* kDescale, const float* vDescale,
                                       int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                       int rotDim, int maxPos, int interleaved, int dtype, int kv_dtype,
                                       const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sQout,
                                       const fa_strides* sK, const fa_strides* sV, void* stream);

int flash_attention_rope_append_paged_varlen(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                             const float* cosSin, const int32_t* cuSeqlensQ, const int32_t* kvLens,
                                             const int32_t* blockTable, const float* kDescale, const float* vDescale,
                                             int batchSize, int numHeads, int numHeadsKV, int totalQ,
                                             int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                             int rotDim, int maxPos, int interleaved, int dtype, int kv_dtype,
                                             const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew,
                                             const fa_strides* sQout, const fa_strides* sK, const fa_strides* sV, void* stream);

/*
 * flash_attention_rope_append_pos, flash_attention_rope_append_paged_pos -- the fused rotary append with PER-ROW POSITION OFFSETS: each
 * is flash_attention_rope_append / _paged with one argument more, directly after cosSin:
 *   posOffsets [batchSize, seqLenNew] int32 (device memory), dense, base aligned to 4 bytes: entry (b, i) is posOffsets[b * seqLenNew + i].
 *            Read BY THE KERNEL, like kvLens: no host synchronisation, and a replayed graph sees the values of the moment.
 * With first = clamp(kvLens[b], 1, capacity) - seqLenNew as in the twin, row i is rotated -- Q and K alike -- at table row
 *     max(first + off, 0),   off = clamp(posOffsets[b, i], 0, seqLenNew - 1)
 * in place of the twin's max(first + i, 0).  The row is below clamp(kvLens[b], 1, capacity) <= capacity <= maxPos: a stale offset gives
 * a wrong angle, never an address outside the table.  SLOTS DO NOT MOVE: K and V row i go to cache position L - seqLenNew + i under
 * the twin's rule exactly (written iff that is >= 0; a table entry outside [0, numPages) skips K / V and not Q), V and the columns
 * >= rotDim keep the twin's bits, and the values follow the twin's rule to the bit.  posOffsets[b, i] = i IS the twin, byte for byte.
 * The use: a draft tree for flash_attention_tree*, node i at depth t of its sequence, is rotated at base + t (siblings share a
 * position) while it is stored at slot base + i: posOffsets = the nodes' depths.
 * Rejected before any launch: everything the twin rejects, with the same codes and in the same order; a NULL posOffsets
 * FA_ERR_NULL_POINTER (with the other pointers); a posOffsets not aligned to 4 bytes FA_ERR_MISALIGNED (with the other 4-byte arrays).
 * Not done here: the ragged (_varlen) forms (there is no ragged tree call), absolute position ids, writing kvLens, drafts above
 * FA_TREE_MAX_Q in the calls that consume the result (this call itself takes any seqLenNew the twin takes).
 */
int flash_attention_rope_append_pos(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* K, void* V,
                                    const float* cosSin, const int32_t* posOffsets, const int32_t* kvLens,
                                    const float* kDescale, const float* vDescale,
                                    int batchSize, int numHeads, int numHeadsKV, int seqLenNew, int seqLenK, int dHead,
                                    int rotDim, int maxPos, int interleaved, int dtype, int kv_dtype,
                                    const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sQout,
                                    const fa_strides* sK, const fa_strides* sV, void* stream);

int flash_attention_rope_append_paged_pos(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                          const float* cosSin, const int32_t* posOffsets, const int32_t* kvLens,
                                          const int32_t* blockTable, const float* kDescale, const float* vDescale,
                                          int batchSize, int numHeads, int numHeadsKV, int seqLenNew,
                                          int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead,
                                          int rotDim, int maxPos, int interleaved, int dtype, int kv_dtype,
                                          const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew,
                                          const fa_strides* sQout, const fa_strides* sK, const fa_strides* sV, void* stream);

/*
 * flash_attention_kv_accept, flash_attention_kv_accept_paged -- IN-CACHE ACCEPTANCE of a speculative step.  The draft's seqLenDraft
 * nodes lie at the cache positions base + 0 .. base + seqLenDraft - 1 (appended, counted by kvLens, verified by flash_attention_tree*);
 * the call moves the accepted root-to-leaf path to base + 0 .. base + n - 1, where a linear append of the accepted tokens would have
 * put it.  The argument lists are flash_attention_kv_append / _paged without Knew, Vnew, their strides, the descales and dtype, with
 * seqLenNew named seqLenDraft, and with two arrays after kvLens (paged: after blockTable):
 *   acceptIdx  [batchSize, seqLenDraft] int32, acceptLens [batchSize] int32: device memory, dense, bases aligned to 4 bytes, read BY
 *            THE KERNEL (no host synchronisation; a replayed graph sees the values of the moment)
 *   seqLenDraft  1 <= seqLenDraft <= FA_TREE_MAX_Q, and at most the capacity
 * Per sequence b: L = min(kvLens[b], capacity) (NULL kvLens: the capacity) still counts the draft; L <= 0: nothing happens.
 * base = L - seqLenDraft, n = clamp(acceptLens[b], 0, seqLenDraft), j_t = clamp(acceptIdx[b, t], 0, seqLenDraft - 1).  For
 * t = 0 .. n - 1, IN ASCENDING ORDER OF t for every byte column, K and V of every K/V head at position base + j_t are copied to
 * position base + t: a copy of bits, 2 dHead or dHead bytes per row by kv_dtype -- nothing is rotated or quantised again.  A move whose
 * source or destination position is negative is skipped; a move whose source or destination page entry is outside [0, numPages) is
 * skipped, never clamped; the move j_t == t writes nothing.  No other byte of the caches or pools is written, and kvLens is not
 * written: the caller follows with kv_lens -= seqLenDraft - accept_lens, after which the positions from base + n on are garbage beyond
 * the length, which every read call tolerates.  For a path of a topologically ordered tree (j_t strictly increasing, hence j_t >= t)
 * the result is exactly "row t := the draft's row j_t": no source is overwritten before it is read.  For any other index list the
 * result is the sequential rule above: well defined, memory safe and of no use.  (Paged: two positions of one sequence that the table
 * maps to the same page are one row of memory; the result there is unspecified, and memory safe.)
 * With flash_attention_rope_append_pos (posOffsets = the depths) the path's t-th node was rotated at base + t, so after the call the
 * cache holds below base + n what flash_attention_rope_append of the accepted tokens, appended linearly, writes: byte for byte, bf16 and
 * e4m3fn.  The whole step is one graph: kv_lens += Sq; rope_append_pos; tree; (sampling -> acceptIdx, acceptLens); kv_accept;
 * kv_lens -= Sq - n.
 * Conventions: the append's -- validated before the launch; no allocation, no synchronisation, nothing printed; one launch moves K and
 * V, with 16-byte vector stores only.  Rejected before any launch, in the append's order: NULL caches, table, acceptIdx or acceptLens
 * FA_ERR_NULL_POINTER; a cache base not aligned to 16 bytes, or kvLens, the table, acceptIdx or acceptLens not aligned to 4,
 * FA_ERR_MISALIGNED; the append's paging and shape checks, with seqLenDraft outside [1, FA_TREE_MAX_Q] or above the capacity,
 * FA_ERR_BAD_SHAPE; then kv_dtype FA_ERR_UNSUPPORTED_DTYPE, dHead FA_ERR_UNSUPPORTED_DHEAD, the cache strides FA_ERR_BAD_STRIDE, the
 * extent and the grid FA_ERR_BAD_SHAPE.  A cache the append accepts, accept accepts.
 * Not done here: a ragged form (a draft size per sequence), writing kvLens, drafts above FA_TREE_MAX_Q, freeing the pages the rewind
 * leaves empty (the engine's).
 */
int flash_attention_kv_accept(void* K, void* V, const int32_t* kvLens, const int32_t* acceptIdx, const int32_t* acceptLens,
                              int batchSize, int numHeadsKV, int seqLenDraft, int seqLenK, int dHead,
                              int kv_dtype /* FA_DTYPE_BF16 | FA_DTYPE_FP8_E4M3 */,
                              const fa_strides* sK, const fa_strides* sV, void* stream);

int flash_attention_kv_accept_paged(void* Kpool, void* Vpool, const int32_t* kvLens, const int32_t* blockTable,
                                    const int32_t* acceptIdx, const int32_t* acceptLens,
                                    int batchSize, int numHeadsKV, int seqLenDraft,
                                    int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead, int kv_dtype,
                                    const fa_strides* sK, const fa_strides* sV, void* stream);

/*
 * flash_attention_mla_decode -- decode for multi-head latent attention (MLA: DeepSeek-V2 / V3 / R1, Kimi-K2) in its ABSORBED form: every
 * query head attends ONE shared cache row per token, dLatent = 512 latent columns followed by dRope = 64 rotary columns.  The score
 * uses all 576 columns, the value is the first 512 columns of the same row:
 *     O = softmax(scale * Q KV^T) * KV[:, :512]
 * The cache is fetched once per 64 packed (head, query row) rows and serves both products.
 *   Q        [batchSize, numHeads, seqLenQ, 576] bf16: the absorbed q_nope * W_UK in columns [0, 512), the rotated q_rope in [512, 576)
 *   KV       [batchSize, seqLenK, 576] bf16, seqLenK the CAPACITY.  sKV: strideB the batch stride, strideS the row stride; strideH is
 *            not read.  NULL = dense
 *   O        [batchSize, numHeads, seqLenQ, 512] in o_dtype;  LSE optional fp32 [batchSize, numHeads, seqLenQ], natural log
 *   scale    the caller's: a model passes mscale^2 / sqrt(192), its softmax scale before the absorption.  Finite and positive
 *   dLatent, dRope  only (512, 64); anything else FA_ERR_UNSUPPORTED_DHEAD
 * Everything else is flash_attention_decode's contract, word for word: 1 <= seqLenQ <= FA_DECODE_MAX_Q; kvLens (DEVICE int32, 4-byte
 * aligned, optional) is read by the kernel and clamped into [1, capacity], NULL = the capacity; is_causal is bottom-right aligned (row i
 * sees k <= len - seqLenQ + i, and at least key 0); rows at and beyond the length may hold NaN or inf; numSplits 0 = chosen on the host
 * from shapes only, 1 .. FA_DECODE_MAX_SPLITS forced; the workspace (flash_attention_mla_decode_workspace_size bytes, 16-byte aligned,
 * contents undefined before and after) may be NULL only under one split; slabs are combined in a fixed order, so results are the same
 * bits run to run; BF16 and F16 outputs are the F32 result rounded once; scores and softmax are fp32 and the weights enter the P.V
 * product as a bf16 hi + lo pair, so 1e-3 + 1e-3 |ref| holds for caches of a handful of keys.  Arguments are validated before any
 * launch, in flash_attention_decode's order and with its codes; the call allocates nothing, never synchronises the host, prints
 * nothing and can be captured into a graph.
 *
 * flash_attention_mla_decode_paged -- the same against a pool of pages: KVpool [numPages, pageSize, 576] bf16 (sKV: strideB the PAGE
 * stride, strideS the row stride), blockTable / tableStride / numPages / pageSize / maxPagesPerSeq as in flash_attention_decode_paged:
 * pages are a power of two >= 16, the pool may exceed 2^32 bytes, table entries are read and clamped by the kernel, pages no visible
 * key lies in are not read and their entries may hold anything.  Equal, bit for bit, to the contiguous call on a gathered copy with
 * the same split count.
 *
 * flash_attention_mla_decode_plan -- fa_decode_plan of such a call: rows_per_block = 64, row_blocks = ceil(numHeads * seqLenQ / 64),
 * grid = batchSize * row_blocks * num_splits, kv_block_rows / lds_bytes / threads of the MLA kernel.  The split rule (enough units for
 * one workgroup per CU, no split shorter than two key tiles of the capacity) is NOT measured.  The grid and row limits of
 * FA_DECODE_MAX_WORKGROUPS apply.  flash_attention_mla_decode_workspace_size = flash_attention_decode_workspace_size at dHead = 512.
 *
 * Not done: fp8 latent caches, a latent-cache append, windows, sinks, tree masks, ragged calls and chunked prefill, cascade, other
 * latent widths, a 128-row block that reads the cache once at numHeads = 128, a single-weights flag.
 */
int    flash_attention_mla_decode_plan(int batchSize, int numHeads, int seqLenQ, int seqLenK, int dLatent, int dRope,
                                       int o_dtype, int numSplits /* 0 = the library chooses */, fa_decode_plan* plan);
size_t flash_attention_mla_decode_workspace_size(int batchSize, int numHeads, int seqLenQ, int dLatent, int numSplits /* as planned */);

int flash_attention_mla_decode(const void* Q, const void* KV, void* O, float* LSE, const int32_t* kvLens, void* workspace,
                               int batchSize, int numHeads, int seqLenQ, int seqLenK, int dLatent, int dRope,
                               float scale, bool is_causal, int dtype, int o_dtype, int numSplits,
                               const fa_strides* sQ, const fa_strides* sKV, const fa_strides* sO, void* stream);

int flash_attention_mla_decode_paged(const void* Q, const void* KVpool, void* O, float* LSE, const int32_t* kvLens,
                                     const int32_t* blockTable, void* workspace,
                                     int batchSize, int numHeads, int seqLenQ,
                                     int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride,
                                     int dLatent, int dRope, float scale, bool is_causal, int dtype, int o_dtype, int numSplits,
                                     const fa_strides* sQ, const fa_strides* sKV, const fa_strides* sO, void* stream);

/* Human-readable text for a return code of the functions above (static storage). */
const char* flash_attention_error_string(int code);

/* Library version, e.g. "fa-mi355x 0.1 (gfx950)". */
const char* flash_attention_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTENTION_H */
