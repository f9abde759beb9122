// FlashAttention.hip -- kernel entries and the C-ABI launcher (include/flash_attention.h).
//
// Counterpart of the reference's kernels/FlashAttention.cuh:59-84 (kernel entry: role split into
// compute warps + two loader warps around four cuda::pipeline objects) and of the launch code in
// tests/main.cu:51-64.  Written for gfx950 only: hipcc --offload-arch=gfx950.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>

#include "../../include/flash_attention.h"
#include "../helpers.hpp"
#include "launchers.hip.h"
#include "generic.hip.h"
#include "weights.hip.h"
#include "bwd_bf16.hip.h"
#include "decode_bf16.hip.h"
#include "split_forms.hip.h"
#include "kv_accept.hip.h"
#include "kv_append.hip.h"
#include "rope_append.hip.h"
#include "mla_decode.hip.h"

namespace fa {

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The element strides of a [*, heads, rows, d] tensor into (strideB, strideH, strideS): the caller's, or (s = NULL) the dense ones
static void resolve_strides(const fa_strides* s, int64_t heads, int64_t rows, int64_t d, int64_t& sB, int64_t& sH, int64_t& sS) {
    sB = s ? s->strideB : heads * rows * d;
    sH = s ? s->strideH : rows * d;
    sS = s ? s->strideS : d;
}

// K / V are fetched through buffer descriptors with 32-bit byte offsets: the `rows` rows of one head, strideS elements of esz bytes
// apart, must end below 2^31 bytes.  The prefill-style paths pass seqLenK + KV_EXTENT_SLACK: two prefetch tiles of slack
constexpr int KV_EXTENT_SLACK = 192;
static bool kv_extent_ok(int64_t rows, int64_t strideS, int esz) { return rows * strideS * esz < (1ll << 31); }

static bool is_input_dtype(int t) { return t == FA_DTYPE_F32 || t == FA_DTYPE_BF16 || t == FA_DTYPE_FP8_E4M3; }
static bool is_output_dtype(int t) { return t == FA_DTYPE_F32 || t == FA_DTYPE_BF16 || t == FA_DTYPE_F16; }
static bool is_f32_or_bf16(int t) { return t == FA_DTYPE_F32 || t == FA_DTYPE_BF16; }   // the backward's O / dO and gradients

static int fill_params(Params& p, const void* Q, const void* K, const void* V, void* O, float* lse, int B, int H, int Hkv,
                       int S, int Sk, int d, float scale, const fa_strides* sQ, const fa_strides* sK,
                       const fa_strides* sV, const fa_strides* sO) {
    p.Q = Q; p.K = K; p.V = V; p.O = O; p.lse = lse;
    resolve_strides(sQ, H, S, d, p.qB, p.qH, p.qS);
    resolve_strides(sK, Hkv, Sk, d, p.kB, p.kH, p.kS);
    resolve_strides(sV, Hkv, Sk, d, p.vB, p.vH, p.vS);
    resolve_strides(sO, H, S, d, p.oB, p.oH, p.oS);
    p.B = B; p.H = H; p.S = S; p.Sk = Sk; p.d = d;
    p.scale = scale;
    p.scale_log2 = scale * 1.4426950408889634f;
    const int64_t G = H / Hkv;
    p.kv_mul = (unsigned)(((1ll << 31) + G - 1) / G);   // loaders.hip.h: kv_head
    return FA_OK;
}

static int elem_size(int dtype) {
    switch (dtype) {
        case FA_DTYPE_F32: return 4;
        case FA_DTYPE_BF16: case FA_DTYPE_F16: return 2;
        case FA_DTYPE_FP8_E4M3: return 1;
        default: return 0;
    }
}

// Grouped-query attention: Hkv K/V heads, each shared by the G = H / Hkv consecutive query heads h with h / G equal (Hkv = H: one
// each).  (H * G < 2^31: what the kernels' multiply-and-shift form of h / G is exact for -- loaders.hip.h: kv_head.)
static bool kv_heads_ok(int H, int Hkv) {
    return H > 0 && Hkv > 0 && H % Hkv == 0 && (int64_t)H * (H / Hkv) < (1ll << 31);
}

static bool strides_ok(const fa_strides* s, int esz, int d) {
    if (!s) return true;
    if (s->strideS < d || s->strideB < 0 || s->strideH < 0) return false;
    return (s->strideS * esz) % 16 == 0 && (s->strideH * esz) % 16 == 0 && (s->strideB * esz) % 16 == 0;
}

static int validate(const void* Q, const void* K, const void* V, void* O, int B, int H, int S, int d,
                    float scale, int dtype, int o_dtype) {
    if (!Q || !K || !V || !O) return FA_ERR_NULL_POINTER;
    if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(O)) return FA_ERR_MISALIGNED;
    if (B <= 0 || H <= 0 || S <= 0 || d <= 0) return FA_ERR_BAD_SHAPE;
    if ((int64_t)B * H > INT32_MAX / 2 || S > (1 << 24)) return FA_ERR_BAD_SHAPE;
    if (!std::isfinite(scale)) return FA_ERR_BAD_SCALE;
    if (!is_input_dtype(dtype) || !is_output_dtype(o_dtype)) return FA_ERR_UNSUPPORTED_DTYPE;
    if (d > 256) return FA_ERR_UNSUPPORTED_DHEAD;
    if (dtype == FA_DTYPE_FP8_E4M3 && d > 128) return FA_ERR_UNSUPPORTED_DHEAD;   // fp8: MFMA path only ...
    if (dtype == FA_DTYPE_FP8_E4M3 && !(scale > 0.f)) return FA_ERR_BAD_SCALE;    // ... which folds a positive scale into exp2
    if ((d * elem_size(dtype)) % 16 != 0 || (d * elem_size(o_dtype)) % 16 != 0) return FA_ERR_UNSUPPORTED_DHEAD;
    return FA_OK;
}

// Compute units of the current device (persistent grid = one workgroup per CU).  256 on MI355X, which is
// also the answer when no device is visible (flash_attention_plan is callable on a build machine).
static int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = cache[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
        cache[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// bf16 inputs: how many leading query blocks of every head run the fp16-weights kernel (the rest: the bf16-weights kernel).
// bf16 weights carry 2^-9 of relative rounding error each; summed over a row's keys it averages out, but a row that sees few
// keys keeps most of it: at FA_EARLY_KEYS = 1024 visible keys the worst element error measured over 40 random heads is 0.74 of
// the stated tolerance 1e-3 + 1e-3|ref| (0.90 at 256, 1.33 at 64: those rows miss it).  Default: a row that can see fewer than
// FA_EARLY_KEYS keys -- under the causal mask the rows q < FA_EARLY_KEYS, and every row when seqLenK < FA_EARLY_KEYS -- gets
// fp16 weights (11 significant bits; 8 x smaller errors), whole query blocks at a time.
static int early_q_blocks(int S, int Sk, int d, bool causal, unsigned flags, int q_block_rows) {
    const int nQ = getNumCta(S, q_block_rows);
    if (!(d == 64 || d == 128) || (flags & FA_FLAG_BF16_WEIGHTS)) return 0;   // (padded head dimensions have no fp16-weights kernel)
    if (flags & FA_FLAG_F16_WEIGHTS) return nQ;
    if (Sk < FA_EARLY_KEYS) return nQ;
    return causal ? std::min(nQ, FA_EARLY_KEYS / q_block_rows) : 0;
}

// Small problems take the pair kernel (kernel_bf16.hip.h: fwd_mfma_pair_kernel): 128-row units, one per workgroup of four waves.
// Causal, D = 64: two workgroups fit a CU -- at most one 256-row unit per CU (where the launch would last as long as its heaviest
// unit), and every XCD group's 128-row units within its two dispatch rounds.  Causal D = 128, and any D without the mask (equal units:
// nothing to pair): one workgroup per CU -- at most one 256-row unit per TWO CUs (half of the chip would idle), every group's 128-row
// units within one round.
static bool pair_kernel_applies(int B, int H, int S, int d, bool causal, int dtype, float scale) {
    if (!(dtype == FA_DTYPE_BF16 && (d == 64 || d == 128) && scale > 0.f)) return false;
    const int64_t heads = (int64_t)B * H;
    const int cus = device_cus(), jpx = cus / 8, rounds = (causal && d == 64) ? 2 : 1;
    if (heads * getNumCta(S, 256) * 2 > (int64_t)cus * rounds) return false;
    return ((heads + 7) / 8) * getNumCta(S, 128) <= rounds * jpx;
}

// Option flags: known, not contradictory, and applicable (the fp16-weights kernels exist for bf16 inputs at the natively
// instantiated head dimensions; run() also wants a positive scale for them)
static int check_flags(unsigned flags, int dtype, int d) {
    if (flags & ~(unsigned)(FA_FLAG_F16_WEIGHTS | FA_FLAG_BF16_WEIGHTS)) return FA_ERR_BAD_FLAGS;
    if ((flags & FA_FLAG_F16_WEIGHTS) && ((flags & FA_FLAG_BF16_WEIGHTS) || !(dtype == FA_DTYPE_BF16 && (d == 64 || d == 128))))
        return FA_ERR_BAD_FLAGS;
    if ((flags & FA_FLAG_BF16_WEIGHTS) && dtype != FA_DTYPE_BF16) return FA_ERR_BAD_FLAGS;
    return FA_OK;
}

// The generic VALU kernel (fp32 or bf16 inputs); its LDS limit is raised to what the largest head dimension takes (100 KiB at d = 256)
static Kernel generic_kernel(int dtype, bool causal, int o_dtype) {
    return by_out(o_dtype, [&]<class OutT>() {
        return by_bool(causal, [&]<bool CAUSAL>() {
            return dtype == FA_DTYPE_F32 ? kernel_of<fwd_generic_kernel<float, OutT, CAUSAL>>(generic_lds_bytes(256))
                                         : kernel_of<fwd_generic_kernel<__bf16, OutT, CAUSAL>>(generic_lds_bytes(256));
        });
    });
}

enum class Family { generic, f32, bf16, fp8, causal_mix, p16, pair };

// What a call launches: ONE kernel over all query blocks [0, nQ) of every head.  run() launches it, flash_attention_plan and
// flash_attention_plan_ex report it.
struct Route {
    Family family;
    int kernel_id;                 // fa_launch_plan::kernel_id
    int D;                         // the instantiated head dimension (generic: the call's)
    bool pad;                      // the call's rows are zero-padded to D
    int q_block_rows, kv_block_rows, threads;
    int nQ;                        // query blocks per head
    int hp;                        // how many leading query blocks of every head take fp16 weights (Params::hp)
    int64_t units, cpx;            // (head, query block) units; per XCD group
    int jpx;                       // Params::jpx: workgroups per XCD group (pair kernel: of one dispatch round)
    int grid;
    int lds_bytes;                 // the launch's dynamic LDS: kernel.lds_bytes but for the generic kernel
    int unit_lists;                // fa_launch_plan_ex::unit_lists: both precisions in one launch of the mixed-precision kernel
    Kernel kernel;

    fa_launch_plan plan() const { return {q_block_rows, kv_block_rows, threads, grid, lds_bytes, kernel_id}; }
};

// The one launch decision.  Arguments validated by the caller; lse: the call wants the LSE.
static Route route(int B, int H, int S, int Sk, int d, bool causal, int dtype, int o_dtype, float scale, unsigned flags, bool lse) {
    // bf16: d in {64,128} natively; any other multiple of 8 up to 128 runs the next larger instantiation with its rows zero-padded on
    // the fly (d/64 or d/128 of the MFMA work is useful -- still ~1000x the VALU kernel).  fp8: the D = 128 instantiation, d < 128
    // zero-padded.  fp32: the exact-fp32 MFMA kernel, d in {64,128} natively, other multiples of 4 up to 128 zero-padded.
    const bool mfma_bf16 = dtype == FA_DTYPE_BF16 && d % 8 == 0 && d <= 128 && scale > 0.f;
    const bool mfma_fp8 = dtype == FA_DTYPE_FP8_E4M3 && d % 16 == 0 && d <= 128 && scale > 0.f;
    const bool mfma_f32 = dtype == FA_DTYPE_F32 && d % 4 == 0 && d <= 128 && scale > 0.f;
    Route r{};
    if (mfma_bf16 || mfma_fp8 || mfma_f32) {
        r.family = mfma_f32 ? Family::f32 : mfma_fp8 ? Family::fp8 : Family::bf16;
        r.kernel_id = mfma_f32 ? 3 : mfma_fp8 ? 2 : 1;
        r.D = mfma_fp8 ? 128 : paddedDHead(d);
        r.q_block_rows = calculateSizeBlockQ(d, dtype);
        r.kv_block_rows = calculateSizeBlockKV(d, dtype);
        r.threads = mfma_f32 ? 256 : 512;
    } else {
        r.family = Family::generic;
        r.D = d;
        r.q_block_rows = GenericCfg::BQ;
        r.kv_block_rows = GenericCfg::BK;
        r.threads = GenericCfg::THREADS;
    }
    r.pad = d != r.D;
    if (r.family == Family::bf16) {
        if (pair_kernel_applies(B, H, S, d, causal, dtype, scale)) {
            r.family = Family::pair;
            r.q_block_rows = 128;
            r.threads = 256;
        }
        // Which query blocks take fp16 softmax weights (early_q_blocks): all with FA_FLAG_F16_WEIGHTS, none with
        // FA_FLAG_BF16_WEIGHTS, by default the rows that see few keys.  Both kinds present (a causal problem longer than
        // FA_EARLY_KEYS): ONE launch of ONE kernel over the list of all query blocks, in the single kernel's head-aligned order (all of
        // a head's blocks start in one round of one XCD group, so its K/V is streamed from that XCD's L2); every unit runs in the
        // precision of its block (kernel_bf16.hip.h: KernelCfg::MIX).  The pair kernel does the same in its own form.
        r.hp = early_q_blocks(S, Sk, d, causal, flags, r.q_block_rows);
        // hp = nQ (FA_FLAG_F16_WEIGHTS, or every row sees fewer than FA_EARLY_KEYS keys) makes the mixed-precision kernel the
        // fp16-weights kernel of the 32x32x16 engine, K by LDS-DMA: faster under the mask than the 16x16x32 one with both tiles through
        // registers (+2.4 % at S = 4096 d = 128, +8 % at S = 2048 d = 64: profiles/r04_tune_f_fp16_everywhere_*.log).  Without the mask
        // early_q_blocks is all or nothing: hp = nQ, every unit runs with fp16 weights.
        if (r.family == Family::bf16 && r.hp > 0) r.family = causal ? Family::causal_mix : Family::p16;
    }
    r.nQ = getNumCta(S, r.q_block_rows);
    r.units = (int64_t)B * H * r.nQ;
    r.cpx = (r.units + 7) / 8;
    const int cus_per_xcd = device_cus() / 8;
    switch (r.family) {
        case Family::generic:
        case Family::f32:   // one workgroup per unit
            r.grid = (int)(8 * r.cpx);
            r.jpx = r.grid / 8;
            break;
        case Family::pair: {
            // 128-row units, one per workgroup of four waves; grid: 8 XCD groups x (the largest group's units, or -- more units than
            // CUs in a group -- two workgroups per CU: d = 64 only, at d = 128 per_group <= cus_per_xcd always)
            const int64_t per_group = (((int64_t)B * H + 7) / 8) * r.nQ;
            r.grid = 8 * (int)(per_group <= cus_per_xcd ? per_group : 2 * cus_per_xcd);
            r.jpx = cus_per_xcd;   // (workgroups of one dispatch round per XCD group: what the pairing counts in)
            break;
        }
        default:   // persistent grid: one workgroup per CU (8 XCD groups x CUs/8), or per unit when there are fewer units
            r.grid = (int)(8 * std::min<int64_t>(r.cpx, cus_per_xcd));
            r.jpx = r.grid / 8;
    }
    switch (r.family) {
        case Family::generic: r.kernel = generic_kernel(dtype, causal, o_dtype); break;
        case Family::f32: r.kernel = (r.D == 128 ? f32_d128_kernel : f32_d64_kernel)(causal, r.pad, o_dtype); break;
        case Family::bf16: r.kernel = (r.D == 128 ? bf16_d128_kernel : bf16_d64_kernel)(causal, r.pad, lse, o_dtype); break;
        case Family::fp8: r.kernel = fp8_d128_kernel(causal, r.pad, o_dtype); break;
        case Family::causal_mix: r.kernel = bf16_causal_mix_kernel(d, o_dtype); break;
        case Family::p16: r.kernel = bf16_p16_kernel(d, o_dtype); break;
        case Family::pair: r.kernel = (d == 64 ? bf16_pair_d64_kernel : bf16_pair_d128_kernel)(causal, o_dtype); break;
    }
    r.lds_bytes = r.family == Family::generic ? generic_lds_bytes(d) : r.kernel.lds_bytes;
    r.unit_lists = r.family == Family::causal_mix && r.hp < r.nQ;
    return r;
}

// Every forward entry point ends here.  Hkv: K/V heads (flash_attention_gqa; every other entry point: Hkv = H).  The route -- the
// kernel, its units (query head, query block) and grid -- does not depend on Hkv: only the K/V head a unit reads does.
static int run(const void* Q, const void* K, const void* V, void* O, float* lse, int B, int H, int Hkv, int S, int Sk, int d,
               float scale, bool causal, int dtype, int o_dtype, const fa_strides* sQ,
               const fa_strides* sK, const fa_strides* sV, const fa_strides* sO, void* stream, unsigned flags = 0) {
    int rc = validate(Q, K, V, O, B, H, S, d, scale, dtype, o_dtype);
    if (rc != FA_OK) return rc;
    if (!kv_heads_ok(H, Hkv)) return FA_ERR_BAD_SHAPE;
    if ((rc = check_flags(flags, dtype, d)) != FA_OK) return rc;
    if ((flags & FA_FLAG_F16_WEIGHTS) && !(scale > 0.f)) return FA_ERR_BAD_FLAGS;
    if (Sk <= 0 || Sk > (1 << 24)) return FA_ERR_BAD_SHAPE;
    if (lse && !aligned16(lse)) return FA_ERR_MISALIGNED;
    const int esz = elem_size(dtype), osz = elem_size(o_dtype);
    if (!strides_ok(sQ, esz, d) || !strides_ok(sK, esz, d) || !strides_ok(sV, esz, d) || !strides_ok(sO, osz, d))
        return FA_ERR_BAD_STRIDE;
    const Route r = route(B, H, S, Sk, d, causal, dtype, o_dtype, scale, flags, lse != nullptr);
    if (r.kernel_id != 0) {
        // the MFMA paths' limit on one head's K / V extent (the generic kernel has none)
        const int64_t rows = (int64_t)Sk + KV_EXTENT_SLACK;
        if (!kv_extent_ok(rows, sK ? sK->strideS : d, esz) || !kv_extent_ok(rows, sV ? sV->strideS : d, esz)) return FA_ERR_BAD_SHAPE;
    }
    if (r.units > INT32_MAX / 2) return FA_ERR_BAD_SHAPE;   // unit indices are 32-bit
    Params p;
    fill_params(p, Q, K, V, O, lse, B, H, Hkv, S, Sk, d, scale, sQ, sK, sV, sO);
    p.dbg = nullptr;
    p.qb0 = 0;
    p.nQ = r.nQ;
    p.units = (int)r.units;
    p.cpx = (int)r.cpx;
    p.jpx = r.jpx;
    p.hp = r.hp;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (r.family == Family::pair) return (int)launch(r.kernel, r.grid, r.threads, r.lds_bytes, st, p, r.hp, r.jpx);
    if (r.family == Family::generic) return (int)launch(r.kernel, r.grid, r.threads, r.lds_bytes, st, p, d);
    return (int)launch(r.kernel, r.grid, r.threads, r.lds_bytes, st, p);
}

// ---- split-KV decode and chunked prefill against the decode caches (decode_bf16.hip.h: one kernel, split_kv_kernel) ----
// The launch decision of flash_attention_decode, from shapes only (seqLenK is the cache CAPACITY; the lengths live in device memory).
// Work units are (batch, K/V head, row block, split).  Library's choice of the split count: enough units for DECODE_WGS_PER_CU
// workgroups on every CU, no split shorter than DECODE_MIN_TILES key tiles of the capacity, at most FA_DECODE_MAX_SPLITS.
// With a window W > 0 a sequence spans at most W + Sq - 1 keys, wherever they start: at most ceil((W + Sq - 1) / TILE) + 1 tiles;
// `tiles` is the smaller of that and the capacity's, and the split count follows from it with the same constants.
// Measured (profiles/decode_split_sweep.log): the time is flat within 5 % from one to two workgroups per CU
// on uniform batches -- two or three are resident per CU, so either is one resident round -- and a batch of unequal lengths, which
// the host cannot see, balances 11 % better at two; a split of a single tile has nothing to prefetch behind and gains nothing.
constexpr int DECODE_WGS_PER_CU = 2, DECODE_MIN_TILES = 2;
// flash_attention_extend (the same kernel with ExtendCfg::RT 16-row tiles per wave): the same rule with
// units = B * Hkv * row blocks of ExtendCfg::ROWS packed rows.  Workgroups per CU: as many as are resident (ExtendCfg::WGS_PER_CU) -- in the forced
// sweep (profiles/extend_rt_sweep.log) a split beyond one resident round only costs: at 512 rows on an 8 k
// prefix, d = 128, two splits of 256 units are 14 % slower than one, and with units short of a round the time is flat within 5 %
// from half a round to one.  EXTEND_MIN_TILES is decode's value, not re-measured: no benchmark shape has a cache short enough for
// it to bind.  A long chunk's units fill the chip by themselves and ns = 1.
constexpr int EXTEND_MIN_TILES = 2;
// flash_attention_extend_varlen (the same kernel, the row count a per-sequence device value): extend's rule and constants with
// units = Hkv * NB, NB the host's BOUND on the batch's row blocks (decode_route) -- the host cannot see the real count, nor how unequal
// the units are (a decode row's unit walks a whole cache, a chunk's lower blocks a part of it).  NOT measured for mixed batches: the
// forced sweep of tools/bench_decode.py --varlen (profiles/extend_varlen_bench.log) shows what the rule costs.
// The _window calls of both extend families (WINDOW = true units, a per-row-block tile range: decode_bf16.hip.h):
// `tiles` is decode's windowed bound with Sq = seqLenQ or totalQ, and the split count follows by extend's unchanged rule and
// constants.  NOT measured for windowed chunks: tools/bench_decode.py --extend --window with --splits shows what the rule costs.

// What a call family is to the launch decision: built once per entry point (decode_form, extend_form, extend_varlen_form), read by
// decode_check_shape, decode_route and decode_run
struct SplitForm {
    int rows_per_block;    // packed rows of a row block: 16 per 16-row tile of a wave
    int wgs_per_cu;        // resident workgroups per CU the split rule fills
    int min_tiles;         // no split shorter than this many key tiles of the capacity
    bool extend;           // chunked prefill: the RT > 1 units, and seqLenQ is capped at the capacity, not at FA_DECODE_MAX_Q
    bool varlen;           // ragged: "Sq" is totalQ, the bound on the token-packed rows of the whole batch (not capped at the capacity),
                           // row_blocks the bound NB over the batch, batchSize <= FA_VARLEN_MAX_BATCH and cuSeqlensQ is required
};
static SplitForm decode_form() { return {DecodeCfg<128>::ROWS, DECODE_WGS_PER_CU, DECODE_MIN_TILES, false, false}; }
static SplitForm extend_form(int d) {   // (any d but 128 takes the d = 64 values: decode_check_shape refuses it before they matter)
    return d == 128 ? SplitForm{ExtendCfg<128>::ROWS, ExtendCfg<128>::WGS_PER_CU, EXTEND_MIN_TILES, true, false}
                    : SplitForm{ExtendCfg<64>::ROWS, ExtendCfg<64>::WGS_PER_CU, EXTEND_MIN_TILES, true, false};
}
static SplitForm extend_varlen_form(int d) {
    SplitForm f = extend_form(d);
    f.varlen = true;
    return f;
}

// The K/V cache of a call, read (flash_attention_decode*, flash_attention_extend*) or written (flash_attention_kv_append*).  Contiguous:
// K / V are [B, Hkv, capacity, d] and paging is NULL.  Paged: K / V are [numPages, Hkv, pageSize, d] pools (strideB = the page stride) and
// the capacity is maxPagesPerSeq * pageSize (cache_capacity).  kv_dtype is the element type of K / V: FA_DTYPE_BF16, or FA_DTYPE_FP8_E4M3
// with the two optional per-head descale arrays.
struct DecodePaging {
    const int32_t* table;
    int64_t table_stride;
    int num_pages, page_size, max_pages;
};
struct KvCache {
    const void *K, *V;
    const int32_t* kv_lens;
    const float *k_descale, *v_descale;
    int kv_dtype;
    int capacity;                  // seqLenK; paged: cache_capacity derives it
    const fa_strides *sK, *sV;
    const DecodePaging* paging;
};

// A call of the split-KV kernel: every flash_attention_decode* / flash_attention_extend* entry point fills one (a member it has no
// argument for stays 0 / NULL) and the three plan functions fill its shape.  window: 0, or the sliding window W of the _window entry
// points.  Ragged (form.varlen; flash_attention_extend*_varlen): Sq is totalQ, Q / O are packed by token (strideB is not read; NULL
// strides: [totalQ, H, d]), the LSE and the slabs are [H, totalQ], and cu_seqlens_q -- NULL in every other call -- is required.
// sinks: NULL, or the [H] attention-sink logits of the flash_attention_sink_* entry points (the last member: every other entry point's
// initialiser leaves it NULL).  tree_mask: NULL, or the [B, Sq] words of flash_attention_tree* (the last member, NULL in
// every other initialiser): the TREE split kernel under any split count, Sq capped at FA_TREE_MAX_Q, is_causal set by the entry point.
struct SplitCall {
    SplitForm form;
    const void* Q;
    void* O;
    float* LSE;
    const int32_t* cu_seqlens_q;
    KvCache cache;
    void* workspace;
    int B, H, Hkv, Sq, d;
    float scale;
    bool is_causal;
    int dtype, o_dtype, num_splits, window;
    const fa_strides *sQ, *sO;
    void* stream;
    const float* sinks;
    const uint64_t* tree_mask;
};

// A call of the append kernels: Sq new rows per sequence (ragged: totalQ token-packed rows, cu_seqlens_q required) into the cache
struct AppendCall {
    bool varlen;
    const void *Knew, *Vnew;
    const int32_t* cu_seqlens_q;
    KvCache cache;
    int B, Hkv, Sq, d, dtype;
    const fa_strides *sKnew, *sVnew;
    void* stream;
};

// What flash_attention_rope_append* adds to the append call of the same form: the query rows in and out, the cos / sin table and the
// pair style.  pos_offsets: NULL, or the [B, Sq] row offsets of the _pos entry points (the last member: every other
// entry point's initialiser leaves it NULL); with_pos says which, so that a _pos call with a NULL array is refused
struct RopeCall {
    const void* Q;
    void* Qout;
    const float* cos_sin;
    int H, rot_dim, max_pos, interleaved;
    const fa_strides *sQ, *sQout;
    bool with_pos;
    const int32_t* pos_offsets;
};

// A call of the acceptance kernel (kv_accept.hip.h): the accepted path of a draft of Sq nodes moved to the front of the draft's slots
struct AcceptCall {
    KvCache cache;                 // k_descale / v_descale NULL: the move is a bit copy
    const int32_t *accept_idx, *accept_lens;
    int B, Hkv, Sq, d;
    void* stream;
};

struct DecodeRoute {
    int ns, row_blocks, tiles;
    int64_t grid;
};

static DecodeRoute decode_route(const SplitCall& c) {
    const SplitForm& f = c.form;
    DecodeRoute r{};
    const int64_t rows = (int64_t)(c.H / c.Hkv) * c.Sq;        // packed rows per K/V head (ragged: of the whole batch, at most)
    // ragged: NB = floor((G totalQ + B (rows_per_block - 1)) / rows_per_block) >= sum_b ceil(G sq_b / rows_per_block) for every
    // partition of at most totalQ rows over the B sequences (each term is at most (G sq_b + rows_per_block - 1) / rows_per_block,
    // and a sum of integers below a bound is below its floor)
    r.row_blocks = (int)std::min<int64_t>(f.varlen ? (rows + (int64_t)c.B * (f.rows_per_block - 1)) / f.rows_per_block
                                                   : (rows + f.rows_per_block - 1) / f.rows_per_block, INT32_MAX);
    constexpr int TILE = DecodeCfg<128>::TILE;
    r.tiles = (c.cache.capacity + TILE - 1) / TILE;
    if (c.window > 0) r.tiles = (int)std::min<int64_t>(r.tiles, ((int64_t)c.window + c.Sq - 1 + TILE - 1) / TILE + 1);
    const int64_t units = (int64_t)(f.varlen ? 1 : c.B) * c.Hkv * r.row_blocks;
    if (c.num_splits > 0) r.ns = c.num_splits;
    else {
        const int64_t want = ((int64_t)f.wgs_per_cu * device_cus() + units - 1) / units;
        r.ns = (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)r.tiles / f.min_tiles, (int64_t)FA_DECODE_MAX_SPLITS}));
    }
    r.grid = units * r.ns;
    return r;
}

// the shape of a call or a plan: B, H, Hkv, Sq, d, the capacity, the types, the forced split count and the window
static int decode_check_shape(const SplitCall& c) {
    const SplitForm& f = c.form;
    const int B = c.B, H = c.H, Sq = c.Sq, Sk = c.cache.capacity, d = c.d;
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0 || d <= 0) return FA_ERR_BAD_SHAPE;
    if ((!f.varlen && Sq > (f.extend ? Sk : FA_DECODE_MAX_Q)) || Sk > (1 << 24) || (int64_t)B * H > INT32_MAX / 2) return FA_ERR_BAD_SHAPE;
    if (c.tree_mask && Sq > FA_TREE_MAX_Q) return FA_ERR_BAD_SHAPE;   // (one 64-bit word per draft node)
    if (f.extend && (int64_t)(f.varlen ? 1 : B) * H * Sq > INT32_MAX) return FA_ERR_BAD_SHAPE;
    if (f.varlen && B > FA_VARLEN_MAX_BATCH) return FA_ERR_BAD_SHAPE;
    if (!kv_heads_ok(H, c.Hkv)) return FA_ERR_BAD_SHAPE;
    if (c.num_splits < 0 || c.num_splits > FA_DECODE_MAX_SPLITS || c.window < 0) return FA_ERR_BAD_SHAPE;
    if (c.dtype != FA_DTYPE_BF16) return FA_ERR_UNSUPPORTED_DTYPE;
    if (!is_output_dtype(c.o_dtype)) return FA_ERR_UNSUPPORTED_DTYPE;
    if (d != 64 && d != 128) return FA_ERR_UNSUPPORTED_DHEAD;
    const DecodeRoute r = decode_route(c);
    if (r.grid > INT32_MAX || r.row_blocks == INT32_MAX) return FA_ERR_BAD_SHAPE;
    // one launch holds fewer than 2^32 threads (the runtime refuses more with a launch error, after the split kernel has run): the
    // split kernel's grid of 256-thread workgroups and, under more than one split, the combine kernel's workgroup per row of O
    const int64_t rows = (int64_t)(f.varlen ? 1 : B) * H * Sq;
    if (r.grid >= FA_DECODE_MAX_WORKGROUPS || (r.ns > 1 && rows >= FA_DECODE_MAX_WORKGROUPS)) return FA_ERR_BAD_SHAPE;
    return FA_OK;
}

static size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

// the strides of a token-packed [totalQ, heads, d] tensor: the caller's with strideB out of the way, or (s = NULL) the dense ones
static fa_strides token_strides(const fa_strides* s, int64_t heads, int64_t d) {
    return s ? fa_strides{0, s->strideH, s->strideS} : fa_strides{0, d, heads * d};
}

// ---- what decode_run and kv_append_run ask of a cache, in the order both ask it: a cache the append accepts is one the decode call
// of the same kv_dtype accepts.  Each call makes checks of its own in between, so these stay separate steps ----
static bool misaligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) & 3u; }

// after the NULL and 16-byte checks of the tensors: the int32 and fp32 arrays the kernel reads
static int cache_check_arrays(const KvCache& c, const int32_t* cuSeqlensQ) {
    if (c.kv_lens && misaligned4(c.kv_lens)) return FA_ERR_MISALIGNED;
    if (misaligned4(cuSeqlensQ)) return FA_ERR_MISALIGNED;
    if (c.paging && misaligned4(c.paging->table)) return FA_ERR_MISALIGNED;
    if (misaligned4(c.k_descale) || misaligned4(c.v_descale)) return FA_ERR_MISALIGNED;
    return FA_OK;
}

// then the paging geometry, which makes the capacity
static int cache_capacity(KvCache& c) {
    if (const DecodePaging* pg = c.paging) {
        if (pg->num_pages <= 0 || pg->max_pages <= 0 || pg->page_size < 16 || (pg->page_size & (pg->page_size - 1))) return FA_ERR_BAD_SHAPE;
        if ((int64_t)pg->max_pages * pg->page_size > (1 << 24) || pg->table_stride < pg->max_pages) return FA_ERR_BAD_SHAPE;
        c.capacity = pg->max_pages * pg->page_size;
    }
    return FA_OK;
}

// K / V: 16-byte row starts = strides in multiples of 16 / the element size
static bool cache_strides_ok(const KvCache& c, int d) {
    const int esz = elem_size(c.kv_dtype);
    return strides_ok(c.sK, esz, d) && strides_ok(c.sV, esz, d);
}

// last, the prefill paths' limit on one head's K / V extent -- of the whole cache, or of one page (page bases are 64-bit: the pool as a
// whole may be larger)
static bool cache_extent_ok(const KvCache& c, int d) {
    const int esz = elem_size(c.kv_dtype);
    const int64_t extent = c.paging ? c.paging->page_size : (int64_t)c.capacity + KV_EXTENT_SLACK;
    return kv_extent_ok(extent, c.sK ? c.sK->strideS : d, esz) && kv_extent_ok(extent, c.sV ? c.sV->strideS : d, esz);
}

// rows of one head of one batch entry / page: what NULL K / V strides are dense over
static int cache_rows(const KvCache& c) { return c.paging ? c.paging->page_size : c.capacity; }

// The forty-four units' launchers by row of SPLIT_FORMS (split_forms.hip.h): a unit missing from the build does not link.  Here and not in
// the header, so that no unit sees -- and compiles -- another unit's kernels
template <size_t... U>
constexpr std::array<int (*)(int, unsigned, hipStream_t, const SplitArgs&), sizeof...(U)> split_launchers(std::index_sequence<U...>) {
    return {&split_unit_launch<(SplitUnit)U>...};
}
constexpr auto SPLIT_LAUNCH = split_launchers(std::make_index_sequence<SPLIT_UNITS>{});

// flash_attention_decode*, flash_attention_extend*: one validation and launch sequence
static int decode_run(SplitCall c) {
    const SplitForm& f = c.form;
    const DecodePaging* pg = c.cache.paging;
    const int H = c.H, Hkv = c.Hkv, Sq = c.Sq, d = c.d;
    if (!c.Q || !c.cache.K || !c.cache.V || !c.O || (pg && !pg->table) || (f.varlen && !c.cu_seqlens_q)) return FA_ERR_NULL_POINTER;
    if (!aligned16(c.Q) || !aligned16(c.cache.K) || !aligned16(c.cache.V) || !aligned16(c.O) || !aligned16(c.LSE) || !aligned16(c.workspace))
        return FA_ERR_MISALIGNED;
    int rc = cache_check_arrays(c.cache, c.cu_seqlens_q);
    if (rc != FA_OK) return rc;
    if (misaligned4(c.sinks)) return FA_ERR_MISALIGNED;
    if (reinterpret_cast<uintptr_t>(c.tree_mask) & 7u) return FA_ERR_MISALIGNED;
    if ((rc = cache_capacity(c.cache)) != FA_OK) return rc;
    fa_strides tQ{}, tO{};   // ragged: Q and O on their token strides
    if (f.varlen) {
        tQ = token_strides(c.sQ, H, d); c.sQ = &tQ;
        tO = token_strides(c.sO, H, d); c.sO = &tO;
    }
    if ((rc = decode_check_shape(c)) != FA_OK) return rc;
    if (c.cache.kv_dtype != FA_DTYPE_BF16 && c.cache.kv_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED_DTYPE;
    if (!std::isfinite(c.scale) || !(c.scale > 0.f)) return FA_ERR_BAD_SCALE;   // (exp2 with the positive scale folded in)
    if (!strides_ok(c.sQ, 2, d) || !cache_strides_ok(c.cache, d) || !strides_ok(c.sO, elem_size(c.o_dtype), d)) return FA_ERR_BAD_STRIDE;
    if (!cache_extent_ok(c.cache, d)) return FA_ERR_BAD_SHAPE;
    const DecodeRoute r = decode_route(c);
    if (r.ns > 1 && !c.workspace) return FA_ERR_NULL_POINTER;
    const int64_t rows = (int64_t)(f.varlen ? 1 : c.B) * H * Sq;
    if (rows > INT32_MAX) return FA_ERR_BAD_SHAPE;

    const int rowsK = cache_rows(c.cache);
    SplitArgs p;   // (every form's launcher takes the part of it that is its kernel's parameter type: split_forms.hip.h)
    p.Q = (const __bf16*)c.Q; p.K = (const __bf16*)c.cache.K; p.V = (const __bf16*)c.cache.V; p.O = c.O; p.lse = c.LSE;
    p.kv_lens = c.cache.kv_lens;
    p.part_o = (float*)c.workspace;
    p.part_lse = r.ns > 1 ? (float*)((char*)c.workspace + round16((size_t)rows * r.ns * d * sizeof(float))) : nullptr;
    resolve_strides(c.sQ, H, Sq, d, p.qB, p.qH, p.qS);
    resolve_strides(c.cache.sK, Hkv, rowsK, d, p.kB, p.kH, p.kS);
    resolve_strides(c.cache.sV, Hkv, rowsK, d, p.vB, p.vH, p.vS);
    resolve_strides(c.sO, H, Sq, d, p.oB, p.oH, p.oS);
    p.H = H; p.Hkv = Hkv; p.G = H / Hkv; p.Sq = Sq; p.Sk = c.cache.capacity;
    p.row_blocks = r.row_blocks; p.ns = r.ns;
    p.rows = (int)rows;
    p.o_dtype = c.o_dtype;
    p.causal = c.is_causal;
    p.scale_log2 = c.scale * 1.4426950408889634f;
    p.block_table = pg ? pg->table : nullptr;
    p.table_stride = pg ? pg->table_stride : 0;
    p.num_pages = pg ? pg->num_pages : 0;
    p.page_shift = pg ? __builtin_ctz((unsigned)pg->page_size) : 0;
    p.k_descale = c.cache.k_descale;
    p.v_descale = c.cache.v_descale;
    p.window = c.window;
    p.cu_q = c.cu_seqlens_q;
    p.B = c.B;
    p.sinks = c.sinks;
    p.tree_mask = c.tree_mask;
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    // Sinks (c.sinks): the kernel that writes O applies them -- under one split the SINK split kernel; under more
    // the split kernel is the call's own without sinks (the slabs hold the keys alone) and the SINK combine adds the sink, once per row
    // Tree masks (c.tree_mask): the split kernel is the TREE form under any split count -- it takes the sinks
    // pointer, NULL or not, and reads it under one split only -- and the combine is the one the call would launch without the mask
    const bool sink = c.sinks != nullptr;
    const SplitKind form = split_form_of(f.extend, f.varlen, c.window > 0, pg != nullptr, c.cache.kv_dtype == FA_DTYPE_FP8_E4M3,
                                         sink && r.ns == 1, c.tree_mask != nullptr);
    const int unit = split_unit_of(form);
    if (unit < 0) return FA_ERR_BAD_FLAGS;   // (no entry point builds such a call: split_forms.hip.h asserts it for varlen <= extend, no ragged tree)
    rc = SPLIT_LAUNCH[unit](d, (unsigned)r.grid, st, p);
    if (rc != FA_OK || r.ns == 1) return rc;
    return combine_launch(f.varlen, sink, d, (unsigned)rows, st, p);
}

// ---- shared-prefix (cascade) decode: flash_attention_cascade_decode*  ----
// A decode call (`u`: the sequences' own suffixes, its cache, lengths, mask and forced split count) and the ONE cache every sequence
// sees in full before its own.  shared.kv_lens is sharedLen (one entry), shared.paging the one-row table; the descales are u.cache's.
struct CascadeCall {
    SplitCall u;
    KvCache shared;
    int num_splits_shared;
};

// The split counts, from shapes only.  Shared part: extend's rule and constants with units = Hkv * ceil(B G Sq / rows per block) and
// the tiles of the shared capacity; unique part: decode's rule, clamped into [2, 32] (decode's kernel writes slabs under more than
// one split only); the shared count is then capped at what is left of FA_DECODE_MAX_SPLITS.  A forced count is taken as given, and a
// chosen one makes room for it.  NOT measured: tools/bench_decode.py --cascade --splits shows what the rule costs
struct CascadeRoute {
    int ns_s, ns_u, row_blocks_s;
    int64_t grid_s;
    DecodeRoute unique;
};
constexpr int CASCADE_MAX_UNIQUE_SPLITS = 32;

static CascadeRoute cascade_route(const CascadeCall& c) {
    const SplitForm f = extend_form(c.u.d);
    CascadeRoute r{};
    const int64_t rows = (int64_t)c.u.B * (c.u.H / c.u.Hkv) * c.u.Sq;   // packed rows per K/V head, across the batch
    r.row_blocks_s = (int)std::min<int64_t>((rows + f.rows_per_block - 1) / f.rows_per_block, INT32_MAX);
    const int64_t units = (int64_t)c.u.Hkv * r.row_blocks_s;
    SplitCall u = c.u;
    if (u.num_splits == 0) {
        u.num_splits = std::clamp(decode_route(u).ns, 2, std::min(CASCADE_MAX_UNIQUE_SPLITS, FA_DECODE_MAX_SPLITS - c.num_splits_shared));
    }
    r.unique = decode_route(u);
    r.ns_u = r.unique.ns;
    if (c.num_splits_shared > 0) r.ns_s = c.num_splits_shared;
    else {
        constexpr int TILE = DecodeCfg<128>::TILE;
        const int tiles = (c.shared.capacity + TILE - 1) / TILE;
        const int64_t want = ((int64_t)f.wgs_per_cu * device_cus() + units - 1) / units;
        r.ns_s = (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)tiles / f.min_tiles, (int64_t)FA_DECODE_MAX_SPLITS - r.ns_u}));
    }
    r.grid_s = units * r.ns_s;
    return r;
}

// the shape of a cascade call or plan: decode's refusals at decode's places, the shared part's among the shape's
static int cascade_check_shape(const CascadeCall& c) {
    const int Ls = c.shared.capacity, ns_s = c.num_splits_shared, ns_u = c.u.num_splits;
    if (Ls <= 0 || Ls > (1 << 24)) return FA_ERR_BAD_SHAPE;
    // (a count left to the library is at least 1 for the shared part and 2 for the unique one: a forced one must leave that room)
    if (ns_s < 0 || ns_u < 0 || ns_u == 1 || (int64_t)std::max(ns_s, 1) + std::max(ns_u, 2) > FA_DECODE_MAX_SPLITS) return FA_ERR_BAD_SHAPE;
    const int rc = decode_check_shape(c.u);
    if (rc != FA_OK) return rc;
    const CascadeRoute r = cascade_route(c);
    const int64_t rows = (int64_t)c.u.B * c.u.H * c.u.Sq;
    if (r.row_blocks_s == INT32_MAX || r.grid_s >= FA_DECODE_MAX_WORKGROUPS || r.unique.grid >= FA_DECODE_MAX_WORKGROUPS
        || rows >= FA_DECODE_MAX_WORKGROUPS)
        return FA_ERR_BAD_SHAPE;
    return FA_OK;
}

// flash_attention_cascade_decode*: one validation, in decode_run's order with the shared cache beside the sequences' own, and three
// launches on the stream -- the SHARED unit into slabs [0, ns_s), decode's own unit on the suffixes into slabs [ns_s, ns_s + ns_u), the
// combine over all of them.  No host synchronisation: graph-capturable
static int cascade_run(CascadeCall c) {
    SplitCall& u = c.u;
    const DecodePaging *pg = u.cache.paging, *spg = c.shared.paging;
    const int B = u.B, H = u.H, Hkv = u.Hkv, Sq = u.Sq, d = u.d;
    if (!u.Q || !c.shared.K || !c.shared.V || !u.cache.K || !u.cache.V || !u.O || (spg && !spg->table) || (pg && !pg->table))
        return FA_ERR_NULL_POINTER;
    if (!aligned16(u.Q) || !aligned16(c.shared.K) || !aligned16(c.shared.V) || !aligned16(u.cache.K) || !aligned16(u.cache.V) || !aligned16(u.O)
        || !aligned16(u.LSE) || !aligned16(u.workspace))
        return FA_ERR_MISALIGNED;
    int rc = cache_check_arrays(c.shared, nullptr);
    if (rc != FA_OK || (rc = cache_check_arrays(u.cache, nullptr)) != FA_OK) return rc;
    if (misaligned4(u.sinks)) return FA_ERR_MISALIGNED;
    if ((rc = cache_capacity(c.shared)) != FA_OK || (rc = cache_capacity(u.cache)) != FA_OK) return rc;
    if ((rc = cascade_check_shape(c)) != FA_OK) return rc;
    if (u.cache.kv_dtype != FA_DTYPE_BF16 && u.cache.kv_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED_DTYPE;
    if (!std::isfinite(u.scale) || !(u.scale > 0.f)) return FA_ERR_BAD_SCALE;
    if (!strides_ok(u.sQ, 2, d) || !cache_strides_ok(c.shared, d) || !cache_strides_ok(u.cache, d) || !strides_ok(u.sO, elem_size(u.o_dtype), d))
        return FA_ERR_BAD_STRIDE;
    if (!cache_extent_ok(c.shared, d) || !cache_extent_ok(u.cache, d)) return FA_ERR_BAD_SHAPE;
    if (!u.workspace) return FA_ERR_NULL_POINTER;   // (both kernels write slabs, whatever the counts)
    const CascadeRoute r = cascade_route(c);
    const int ns = r.ns_s + r.ns_u;
    const int64_t rows = (int64_t)B * H * Sq;

    const bool kv8 = u.cache.kv_dtype == FA_DTYPE_FP8_E4M3;
    SplitArgs p{};
    p.Q = (const __bf16*)u.Q; p.O = u.O; p.lse = u.LSE;
    float* const part_o = (float*)u.workspace;
    float* const part_lse = (float*)((char*)u.workspace + round16((size_t)rows * ns * d * sizeof(float)));
    resolve_strides(u.sQ, H, Sq, d, p.qB, p.qH, p.qS);
    resolve_strides(u.sO, H, Sq, d, p.oB, p.oH, p.oS);
    p.H = H; p.Hkv = Hkv; p.G = H / Hkv; p.Sq = Sq; p.B = B;
    p.rows = (int)rows;
    p.o_dtype = u.o_dtype;
    p.scale_log2 = u.scale * 1.4426950408889634f;
    p.k_descale = u.cache.k_descale;
    p.v_descale = u.cache.v_descale;
    p.sinks = u.sinks;
    // the cache a launch reads: its tensors and strides, its lengths, its capacity and its table
    auto of_cache = [&](const KvCache& kc, const DecodePaging* g) {
        const int rowsK = cache_rows(kc);
        p.K = (const __bf16*)kc.K; p.V = (const __bf16*)kc.V;
        p.kv_lens = kc.kv_lens;
        p.Sk = kc.capacity;
        resolve_strides(kc.sK, Hkv, rowsK, d, p.kB, p.kH, p.kS);
        resolve_strides(kc.sV, Hkv, rowsK, d, p.vB, p.vH, p.vS);
        p.block_table = g ? g->table : nullptr;
        p.table_stride = g ? g->table_stride : 0;
        p.num_pages = g ? g->num_pages : 0;
        p.page_shift = g ? __builtin_ctz((unsigned)g->page_size) : 0;
    };
    hipStream_t st = reinterpret_cast<hipStream_t>(u.stream);
    // 1. the prefix, once per row block of the whole batch
    of_cache(c.shared, spg);
    p.part_o = part_o; p.part_lse = part_lse;
    p.row_blocks = r.row_blocks_s; p.ns = r.ns_s;
    p.causal = 0; p.window = 0;
    int unit = split_unit_of(split_form_of(false, false, false, spg != nullptr, kv8, false, false, true));
    if (unit < 0) return FA_ERR_BAD_FLAGS;
    if ((rc = SPLIT_LAUNCH[unit](d, (unsigned)r.grid_s, st, p)) != FA_OK) return rc;
    // 2. the suffixes: decode's own unit under ns_u >= 2 splits, its slabs behind the prefix's
    of_cache(u.cache, pg);
    p.part_o = part_o + (int64_t)r.ns_s * rows * d; p.part_lse = part_lse + (int64_t)r.ns_s * rows;
    p.row_blocks = r.unique.row_blocks; p.ns = r.ns_u;
    p.causal = u.is_causal;
    unit = split_unit_of(split_form_of(false, false, false, pg != nullptr, kv8, false, false));
    if (unit < 0) return FA_ERR_BAD_FLAGS;
    if ((rc = SPLIT_LAUNCH[unit](d, (unsigned)r.unique.grid, st, p)) != FA_OK) return rc;
    // 3. the one combine over both parts' slabs; the sinks join here, once per row
    p.part_o = part_o; p.part_lse = part_lse;
    p.ns = ns;
    return combine_launch(false, u.sinks != nullptr, d, (unsigned)rows, st, p);
}

// ---- K/V cache append (kv_append.hip.h) ----
// flash_attention_kv_append*: one validation and launch.  The caches are decode_run's and so are their checks (cache_*, above).  Sq is
// not capped at FA_DECODE_MAX_Q (the call also fills a cache after a prefill), only at the capacity.
// Ragged (varlen; flash_attention_kv_append*_varlen): Sq is totalQ, not capped at the capacity; Knew / Vnew are packed by token
// (strideB is not read; NULL strides: [totalQ, Hkv, d]); cu_seqlens_q -- NULL in the uniform calls -- is required; the token-major kernel.
// flash_attention_rope_append* (rope_append.hip.h): the same ladder with the steps of `rope` (NULL in the plain
// calls) beside the twin's of the same kind -- pointers, alignment, shape, then after the dHead check rotDim, maxPos and the pair
// style, strides -- and the fused kernels.  Heads: the grid is (units of the twin without its K/V heads and its K-or-V bit) x head
// slices; a slice is a run of consecutive K/V heads one workgroup loops over, reading each position's table row once.  As many slices
// as bring the grid to ROPE_WGS_PER_CU workgroups per CU, and no more: a decode step spreads its heads over the device, a long cache
// fill reads the table once per position.  (Eight: a workgroup's four waves each wait on one batch of loads at a time, so the bytes
// in flight come from the number of resident waves; the register count allows three workgroups per CU, and several rounds of them
// even out the tail.  The re-reads of a table row by the slices of one position are L2 hits.)
constexpr int ROPE_WGS_PER_CU = 8;
static int kv_append_run(AppendCall c, const RopeCall* rope = nullptr) {
    const DecodePaging* pg = c.cache.paging;
    const int B = c.B, Hkv = c.Hkv, Sq = c.Sq, d = c.d, kv_dtype = c.cache.kv_dtype;
    if (!c.Knew || !c.Vnew || !c.cache.K || !c.cache.V || (pg && !pg->table) || (c.varlen && !c.cu_seqlens_q)) return FA_ERR_NULL_POINTER;
    if (rope && (!rope->Q || !rope->Qout || !rope->cos_sin || (rope->with_pos && !rope->pos_offsets))) return FA_ERR_NULL_POINTER;
    if (!aligned16(c.Knew) || !aligned16(c.Vnew) || !aligned16(c.cache.K) || !aligned16(c.cache.V)) return FA_ERR_MISALIGNED;
    if (rope && (!aligned16(rope->Q) || !aligned16(rope->Qout) || !aligned16(rope->cos_sin))) return FA_ERR_MISALIGNED;
    int rc = cache_check_arrays(c.cache, c.cu_seqlens_q);
    if (rc != FA_OK) return rc;
    if (rope && misaligned4(rope->pos_offsets)) return FA_ERR_MISALIGNED;
    if ((rc = cache_capacity(c.cache)) != FA_OK) return rc;
    const int Sk = c.cache.capacity;
    if (B <= 0 || Hkv <= 0 || Sq <= 0 || Sk <= 0 || d <= 0) return FA_ERR_BAD_SHAPE;
    if (Sk > (1 << 24) || (!c.varlen && Sq > Sk) || (int64_t)B * Hkv > INT32_MAX / 2) return FA_ERR_BAD_SHAPE;
    if (c.varlen && B > FA_VARLEN_MAX_BATCH) return FA_ERR_BAD_SHAPE;
    const int H = rope ? rope->H : Hkv;
    if (rope && (!kv_heads_ok(H, Hkv) || (int64_t)B * H > INT32_MAX / 2)) return FA_ERR_BAD_SHAPE;
    if (c.dtype != FA_DTYPE_BF16) return FA_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype != FA_DTYPE_BF16 && kv_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype == FA_DTYPE_BF16 && (c.cache.k_descale || c.cache.v_descale)) return FA_ERR_UNSUPPORTED_DTYPE;   // a bf16 cache is a bit copy
    if (d != 64 && d != 128) return FA_ERR_UNSUPPORTED_DHEAD;
    if (rope) {
        if (rope->rot_dim < 16 || rope->rot_dim > d || rope->rot_dim % 16) return FA_ERR_BAD_SHAPE;
        if (rope->max_pos < Sk) return FA_ERR_BAD_SHAPE;   // every position the kernel can form lies in the table
        if (rope->interleaved != 0 && rope->interleaved != 1) return FA_ERR_BAD_FLAGS;
    }
    fa_strides tK{}, tV{}, tQ{}, tO{};   // ragged: the new rows on their token strides
    const fa_strides *sQ = rope ? rope->sQ : nullptr, *sQout = rope ? rope->sQout : nullptr;
    if (c.varlen) {
        tK = token_strides(c.sKnew, Hkv, d); c.sKnew = &tK;
        tV = token_strides(c.sVnew, Hkv, d); c.sVnew = &tV;
        tQ = token_strides(sQ, H, d); sQ = &tQ;
        tO = token_strides(sQout, H, d); sQout = &tO;
    }
    if (!strides_ok(c.sKnew, 2, d) || !strides_ok(c.sVnew, 2, d) || !cache_strides_ok(c.cache, d)) return FA_ERR_BAD_STRIDE;
    if (rope && (!strides_ok(sQ, 2, d) || !strides_ok(sQout, 2, d))) return FA_ERR_BAD_STRIDE;
    if (!cache_extent_ok(c.cache, d)) return FA_ERR_BAD_SHAPE;   // what is written can be read
    const int row_blocks = (Sq + KvAppendCfg::BLOCK - 1) / KvAppendCfg::BLOCK + 1;   // blocks are aligned in key positions
    const int tokens_per_block = KvAppendCfg::THREADS / (d / 8);                     // ragged: a row per d / 8 lanes
    const int token_blocks = (int)(((int64_t)Sq + tokens_per_block - 1) / tokens_per_block);
    const int64_t grid = c.varlen ? (int64_t)Hkv * token_blocks * 2 : (int64_t)B * Hkv * row_blocks * 2;
    if (grid > INT32_MAX) return FA_ERR_BAD_SHAPE;   // (the fused calls' limit too: their own grid is never larger)

    const int rowsK = cache_rows(c.cache);
    KvAppendParams p;
    p.Knew = (const __bf16*)c.Knew; p.Vnew = (const __bf16*)c.Vnew;
    p.K = const_cast<void*>(c.cache.K); p.V = const_cast<void*>(c.cache.V);   // (the entry points take them writable)
    p.kv_lens = c.cache.kv_lens;
    p.block_table = pg ? pg->table : nullptr;
    p.k_descale = c.cache.k_descale; p.v_descale = c.cache.v_descale;
    resolve_strides(c.sKnew, Hkv, Sq, d, p.knB, p.knH, p.knS);
    resolve_strides(c.sVnew, Hkv, Sq, d, p.vnB, p.vnH, p.vnS);
    resolve_strides(c.cache.sK, Hkv, rowsK, d, p.kB, p.kH, p.kS);
    resolve_strides(c.cache.sV, Hkv, rowsK, d, p.vB, p.vH, p.vS);
    p.table_stride = pg ? pg->table_stride : 0;
    p.Hkv = Hkv; p.Sq = Sq; p.cap = Sk; p.row_blocks = row_blocks;
    p.num_pages = pg ? pg->num_pages : 0;
    p.page_shift = pg ? __builtin_ctz((unsigned)pg->page_size) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    if (rope) {
        RopeAppendParams r;
        r.a = p;
        r.Q = (const __bf16*)rope->Q; r.Qout = (__bf16*)rope->Qout; r.cos_sin = rope->cos_sin;
        resolve_strides(sQ, H, Sq, d, r.qB, r.qH, r.qS);
        resolve_strides(sQout, H, Sq, d, r.oB, r.oH, r.oS);
        r.G = H / Hkv; r.rot = rope->rot_dim; r.interleaved = rope->interleaved;
        const int rope_token_blocks = (int)(((int64_t)Sq + 2 * tokens_per_block - 1) / (2 * tokens_per_block));   // a row per d / 16 lanes
        const int64_t base = c.varlen ? (int64_t)rope_token_blocks : (int64_t)B * row_blocks;                      // <= grid / (2 Hkv)
        const int64_t want = ((int64_t)ROPE_WGS_PER_CU * device_cus() + base - 1) / base;
        r.heads_per_slice = (int)((Hkv + std::min<int64_t>(want, Hkv) - 1) / std::min<int64_t>(want, Hkv));
        r.head_slices = (Hkv + r.heads_per_slice - 1) / r.heads_per_slice;
        const unsigned rope_grid = (unsigned)(base * r.head_slices);
        const bool kv8 = kv_dtype == FA_DTYPE_FP8_E4M3;
        if (c.varlen) {
            const RopeAppendVarlenParams rv{r, c.cu_seqlens_q, B, rope_token_blocks};
            return (int)launch(rope_append_varlen_kernel_of(d, kv8, pg != nullptr), rope_grid, KvAppendCfg::THREADS, 0, st, rv);
        }
        if (rope->with_pos) {   // (no ragged _pos entry point: c.varlen is false)
            RopePosParams rp;
            static_cast<RopeAppendParams&>(rp) = r;
            rp.pos_offsets = rope->pos_offsets;
            return (int)launch(rope_append_pos_kernel_of(d, kv8, pg != nullptr), rope_grid, KvAppendCfg::THREADS, 0, st, rp);
        }
        return (int)launch(rope_append_kernel_of(d, kv8, pg != nullptr), rope_grid, KvAppendCfg::THREADS, 0, st, r);
    }
    if (c.varlen) {
        const KvAppendVarlenParams pv{p, c.cu_seqlens_q, B, token_blocks};
        const Kernel kr = kv_append_varlen_kernel_of(d, kv_dtype == FA_DTYPE_FP8_E4M3, pg != nullptr);
        return (int)launch(kr, (unsigned)grid, KvAppendCfg::THREADS, 0, st, pv);
    }
    const Kernel k = kv_append_kernel_of(d, kv_dtype == FA_DTYPE_FP8_E4M3, pg != nullptr);
    return (int)launch(k, (unsigned)grid, KvAppendCfg::THREADS, 0, st, p);
}

// ---- in-cache acceptance (kv_accept.hip.h) ----
// flash_attention_kv_accept*: the append's ladder without the new rows -- pointers, alignment, cache_check_arrays with the two index
// arrays beside it, cache_capacity, shape (the draft capped at FA_TREE_MAX_Q and at the capacity), kv_dtype, dHead, cache strides,
// extent, grid: a cache the append accepts, accept accepts.  One wave per (sequence, K or V, 64 consecutive (K/V head, 16-byte chunk)
// pairs), four waves per workgroup.
static int kv_accept_run(AcceptCall c) {
    const DecodePaging* pg = c.cache.paging;
    const int B = c.B, Hkv = c.Hkv, Sq = c.Sq, d = c.d, kv_dtype = c.cache.kv_dtype;
    if (!c.cache.K || !c.cache.V || (pg && !pg->table) || !c.accept_idx || !c.accept_lens) return FA_ERR_NULL_POINTER;
    if (!aligned16(c.cache.K) || !aligned16(c.cache.V)) return FA_ERR_MISALIGNED;
    int rc = cache_check_arrays(c.cache, nullptr);
    if (rc != FA_OK) return rc;
    if (misaligned4(c.accept_idx) || misaligned4(c.accept_lens)) return FA_ERR_MISALIGNED;
    if ((rc = cache_capacity(c.cache)) != FA_OK) return rc;
    const int Sk = c.cache.capacity;
    if (B <= 0 || Hkv <= 0 || Sq <= 0 || Sk <= 0 || d <= 0) return FA_ERR_BAD_SHAPE;
    if (Sk > (1 << 24) || Sq > Sk || Sq > FA_TREE_MAX_Q || (int64_t)B * Hkv > INT32_MAX / 2) return FA_ERR_BAD_SHAPE;
    if (kv_dtype != FA_DTYPE_BF16 && kv_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED_DTYPE;
    if (d != 64 && d != 128) return FA_ERR_UNSUPPORTED_DHEAD;
    if (!cache_strides_ok(c.cache, d)) return FA_ERR_BAD_STRIDE;
    if (!cache_extent_ok(c.cache, d)) return FA_ERR_BAD_SHAPE;
    const int chunks = d * elem_size(kv_dtype) / 16;                       // 16-byte chunks per row
    const int head_groups = (int)(((int64_t)Hkv * chunks + 63) / 64);
    const int64_t grid = ((int64_t)B * head_groups * 2 + KvAcceptCfg::WAVES - 1) / KvAcceptCfg::WAVES;
    if (grid > INT32_MAX) return FA_ERR_BAD_SHAPE;

    const int rowsK = cache_rows(c.cache);
    KvAcceptParams p;
    p.K = const_cast<void*>(c.cache.K); p.V = const_cast<void*>(c.cache.V);   // (the entry points take them writable)
    p.kv_lens = c.cache.kv_lens;
    p.block_table = pg ? pg->table : nullptr;
    p.accept_idx = c.accept_idx; p.accept_lens = c.accept_lens;
    resolve_strides(c.cache.sK, Hkv, rowsK, d, p.kB, p.kH, p.kS);
    resolve_strides(c.cache.sV, Hkv, rowsK, d, p.vB, p.vH, p.vS);
    p.table_stride = pg ? pg->table_stride : 0;
    p.B = B; p.Hkv = Hkv; p.Sq = Sq; p.cap = Sk; p.head_groups = head_groups;
    p.num_pages = pg ? pg->num_pages : 0;
    p.page_shift = pg ? __builtin_ctz((unsigned)pg->page_size) : 0;
    const Kernel k = kv_accept_kernel_of(d, kv_dtype == FA_DTYPE_FP8_E4M3, pg != nullptr);
    return (int)launch(k, (unsigned)grid, KvAcceptCfg::THREADS, 0, reinterpret_cast<hipStream_t>(c.stream), p);
}

// ---- MLA decode: flash_attention_mla_decode* (mla_decode.hip.h) ----
// One latent cache [B, Sk, 576] (paged: [numPages, pageSize, 576]) read as K (all 576 columns) and as V (the first 512); one K/V "head"
// for all H query heads.  A kernel of its own around decode's pieces: DecodeParams, the slab workspace, the combine at D = 512, the
// cache checks.  The split rule is decode_route's formula with units = B * row blocks of 64 packed rows, one workgroup per CU and
// EXTEND_MIN_TILES, the tiles counted in the kernel's own key tile (MlaCfg::KT).  NOT measured: the constants are chunked prefill's (the
// other one-workgroup-per-CU form), and the forced sweep of tools/bench_decode.py --mla --splits (profiles/mla_decode_gpu.log,
// DESIGN.md section 35) shows what the rule costs.
struct MlaCall {
    const void* Q;
    const void* KV;
    void* O;
    float* LSE;
    const int32_t* kv_lens;
    void* workspace;
    int B, H, Sq, capacity, d_latent, d_rope;
    float scale;
    bool is_causal;
    int dtype, o_dtype, num_splits;
    const fa_strides *sQ, *sKV, *sO;
    const DecodePaging* paging;
    void* stream;
};

static DecodeRoute mla_route(const MlaCall& c) {
    DecodeRoute r{};
    const int64_t rows = (int64_t)c.H * c.Sq;
    r.row_blocks = (int)std::min<int64_t>((rows + MlaCfg::ROWS - 1) / MlaCfg::ROWS, INT32_MAX);
    r.tiles = (c.capacity + MlaCfg::KT - 1) / MlaCfg::KT;
    const int64_t units = (int64_t)c.B * r.row_blocks;
    if (c.num_splits > 0) r.ns = c.num_splits;
    else {
        const int64_t want = ((int64_t)device_cus() + units - 1) / units;   // (wgs_per_cu = 1)
        r.ns = (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)r.tiles / EXTEND_MIN_TILES, (int64_t)FA_DECODE_MAX_SPLITS}));
    }
    r.grid = units * r.ns;
    return r;
}

// the shape of a call or a plan, in decode_check_shape's order
static int mla_check_shape(const MlaCall& c) {
    const int B = c.B, H = c.H, Sq = c.Sq, Sk = c.capacity;
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0 || c.d_latent <= 0 || c.d_rope <= 0) return FA_ERR_BAD_SHAPE;
    if (Sq > FA_DECODE_MAX_Q || Sk > (1 << 24) || (int64_t)B * H > INT32_MAX / 2) return FA_ERR_BAD_SHAPE;
    if (c.num_splits < 0 || c.num_splits > FA_DECODE_MAX_SPLITS) return FA_ERR_BAD_SHAPE;
    if (c.dtype != FA_DTYPE_BF16) return FA_ERR_UNSUPPORTED_DTYPE;
    if (!is_output_dtype(c.o_dtype)) return FA_ERR_UNSUPPORTED_DTYPE;
    if (c.d_latent != MlaCfg::DL || c.d_rope != MlaCfg::DR) return FA_ERR_UNSUPPORTED_DHEAD;
    const DecodeRoute r = mla_route(c);
    if (r.grid > INT32_MAX || r.row_blocks == INT32_MAX) return FA_ERR_BAD_SHAPE;
    const int64_t rows = (int64_t)B * H * Sq;
    if (r.grid >= FA_DECODE_MAX_WORKGROUPS || (r.ns > 1 && rows >= FA_DECODE_MAX_WORKGROUPS)) return FA_ERR_BAD_SHAPE;
    return FA_OK;
}

// one validation, in decode_run's order, and the launches: the MLA kernel and, under more than one split, the combine at D = 512
static int mla_run(MlaCall c) {
    const DecodePaging* pg = c.paging;
    constexpr int D = MlaCfg::D, DL = MlaCfg::DL;
    if (!c.Q || !c.KV || !c.O || (pg && !pg->table)) return FA_ERR_NULL_POINTER;
    if (!aligned16(c.Q) || !aligned16(c.KV) || !aligned16(c.O) || !aligned16(c.LSE) || !aligned16(c.workspace)) return FA_ERR_MISALIGNED;
    fa_strides tKV{};   // the cache's strides without the head stride, which no MLA call reads
    if (c.sKV) tKV = fa_strides{c.sKV->strideB, 0, c.sKV->strideS};
    KvCache cache{.K = c.KV, .V = c.KV, .kv_lens = c.kv_lens, .kv_dtype = FA_DTYPE_BF16, .capacity = c.capacity,
                  .sK = c.sKV ? &tKV : nullptr, .sV = c.sKV ? &tKV : nullptr, .paging = pg};
    int rc = cache_check_arrays(cache, nullptr);
    if (rc != FA_OK) return rc;
    if ((rc = cache_capacity(cache)) != FA_OK) return rc;
    c.capacity = cache.capacity;
    if ((rc = mla_check_shape(c)) != FA_OK) return rc;
    if (!std::isfinite(c.scale) || !(c.scale > 0.f)) return FA_ERR_BAD_SCALE;   // (exp2 with the positive scale folded in)
    if (!strides_ok(c.sQ, 2, D) || !cache_strides_ok(cache, D) || !strides_ok(c.sO, elem_size(c.o_dtype), DL)) return FA_ERR_BAD_STRIDE;
    if (!cache_extent_ok(cache, D)) return FA_ERR_BAD_SHAPE;
    const DecodeRoute r = mla_route(c);
    if (r.ns > 1 && !c.workspace) return FA_ERR_NULL_POINTER;
    const int64_t rows = (int64_t)c.B * c.H * c.Sq;
    if (rows > INT32_MAX) return FA_ERR_BAD_SHAPE;

    DecodeParams p{};
    p.Q = (const __bf16*)c.Q; p.K = (const __bf16*)c.KV; p.V = (const __bf16*)c.KV; p.O = c.O; p.lse = c.LSE;
    p.kv_lens = c.kv_lens;
    p.part_o = (float*)c.workspace;
    p.part_lse = r.ns > 1 ? (float*)((char*)c.workspace + round16((size_t)rows * r.ns * DL * sizeof(float))) : nullptr;
    resolve_strides(c.sQ, c.H, c.Sq, D, p.qB, p.qH, p.qS);
    resolve_strides(cache.sK, 1, cache_rows(cache), D, p.kB, p.kH, p.kS);
    p.vB = p.kB; p.vH = p.kH; p.vS = p.kS;
    resolve_strides(c.sO, c.H, c.Sq, DL, p.oB, p.oH, p.oS);
    p.H = c.H; p.Hkv = 1; p.G = c.H; p.Sq = c.Sq; p.Sk = cache.capacity;
    p.row_blocks = r.row_blocks; p.ns = r.ns;
    p.rows = (int)rows;
    p.o_dtype = c.o_dtype;
    p.causal = c.is_causal;
    p.scale_log2 = c.scale * 1.4426950408889634f;
    p.block_table = pg ? pg->table : nullptr;
    p.table_stride = pg ? pg->table_stride : 0;
    p.num_pages = pg ? pg->num_pages : 0;
    p.page_shift = pg ? __builtin_ctz((unsigned)pg->page_size) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    rc = mla_decode_launch(pg != nullptr, (unsigned)r.grid, st, p);
    if (rc != FA_OK || r.ns == 1) return rc;
    return mla_combine_launch((unsigned)rows, st, p);
}
}  // namespace fa

extern "C" {

int flash_attention(const void* Q, const void* K, const void* V, void* O, int batchSize, int numHeads,
                    int seqLen, int dHead, float scale, bool is_causal, int dtype, int o_dtype,
                    void* stream) {
    return fa::run(Q, K, V, O, nullptr, batchSize, numHeads, numHeads, seqLen, seqLen, dHead, scale, is_causal, dtype, o_dtype,
                   nullptr, nullptr, nullptr, nullptr, stream);
}

int flash_attention_lse(const void* Q, const void* K, const void* V, void* O, float* LSE, int batchSize, int numHeads,
                        int seqLen, int dHead, float scale, bool is_causal, int dtype, int o_dtype, void* stream) {
    return fa::run(Q, K, V, O, LSE, batchSize, numHeads, numHeads, seqLen, seqLen, dHead, scale, is_causal, dtype, o_dtype,
                   nullptr, nullptr, nullptr, nullptr, stream);
}

int flash_attention_strided(const void* Q, const void* K, const void* V, void* O, int batchSize,
                            int numHeads, int seqLen, int dHead, float scale, bool is_causal, int dtype,
                            int o_dtype, const fa_strides* sQ, const fa_strides* sK,
                            const fa_strides* sV, const fa_strides* sO, void* stream) {
    return fa::run(Q, K, V, O, nullptr, batchSize, numHeads, numHeads, seqLen, seqLen, dHead, scale, is_causal, dtype, o_dtype, sQ,
                   sK, sV, sO, stream);
}

int flash_attention_cross(const void* Q, const void* K, const void* V, void* O, float* LSE, int batchSize, int numHeads,
                          int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype, int o_dtype,
                          const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                          void* stream) {
    return fa::run(Q, K, V, O, LSE, batchSize, numHeads, numHeads, seqLenQ, seqLenK, dHead, scale, is_causal, dtype, o_dtype, sQ,
                   sK, sV, sO, stream);
}

int flash_attention_ex(const void* Q, const void* K, const void* V, void* O, float* LSE, int batchSize, int numHeads,
                       int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype, int o_dtype,
                       const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                       unsigned flags, void* stream) {
    return flash_attention_gqa(Q, K, V, O, LSE, batchSize, numHeads, numHeads, seqLenQ, seqLenK, dHead, scale, is_causal, dtype,
                               o_dtype, sQ, sK, sV, sO, flags, stream);
}

int flash_attention_gqa(const void* Q, const void* K, const void* V, void* O, float* LSE, int batchSize, int numHeads,
                        int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype, int o_dtype,
                        const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                        unsigned flags, void* stream) {
    return fa::run(Q, K, V, O, LSE, batchSize, numHeads, numHeadsKV, seqLenQ, seqLenK, dHead, scale, is_causal, dtype, o_dtype,
                   sQ, sK, sV, sO, stream, flags);
}

int flash_attention_weights(const void* Q, const void* K, const float* LSE, float* P, int batchSize, int numHeads,
                            int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype,
                            const fa_strides* sQ, const fa_strides* sK, void* stream) {
    using namespace fa;
    if (!Q || !K || !LSE || !P) return FA_ERR_NULL_POINTER;
    if (!aligned16(Q) || !aligned16(K) || !aligned16(LSE) || !aligned16(P)) return FA_ERR_MISALIGNED;
    if (batchSize <= 0 || numHeads <= 0 || seqLenQ <= 0 || seqLenK <= 0 || dHead <= 0) return FA_ERR_BAD_SHAPE;
    if (!std::isfinite(scale)) return FA_ERR_BAD_SCALE;
    if (!is_input_dtype(dtype)) return FA_ERR_UNSUPPORTED_DTYPE;
    const int esz = elem_size(dtype);
    if (dHead > 256 || (dHead * esz) % 16 != 0) return FA_ERR_UNSUPPORTED_DHEAD;
    if (!strides_ok(sQ, esz, dHead) || !strides_ok(sK, esz, dHead)) return FA_ERR_BAD_STRIDE;
    WeightsParams p;
    p.Q = Q; p.K = K; p.lse = LSE; p.P = P;
    resolve_strides(sQ, numHeads, seqLenQ, dHead, p.qB, p.qH, p.qS);
    resolve_strides(sK, numHeads, seqLenK, dHead, p.kB, p.kH, p.kS);
    p.H = numHeads; p.Sq = seqLenQ; p.Sk = seqLenK; p.d = dHead;
    p.nQ = (seqLenQ + 15) / 16; p.nK = (seqLenK + 63) / 64;
    p.scale = scale; p.causal = is_causal;
    const int64_t blocks = (int64_t)batchSize * numHeads * p.nQ * p.nK;
    if (blocks > INT32_MAX) return FA_ERR_BAD_SHAPE;
    // (the LDS limit is raised to what dHead = 256 takes: 80 KiB)
    const Kernel k = dtype == FA_DTYPE_F32    ? kernel_of<attn_weights_kernel<float>>(weights_lds_bytes(256))
                     : dtype == FA_DTYPE_BF16 ? kernel_of<attn_weights_kernel<__bf16>>(weights_lds_bytes(256))
                                              : kernel_of<attn_weights_kernel<fp8_t>>(weights_lds_bytes(256));
    return (int)launch(k, (unsigned)blocks, 256, weights_lds_bytes(dHead), reinterpret_cast<hipStream_t>(stream), p);
}

int flash_attention_shard_range(int totalHeads, int rank, int nRanks, int* lo, int* hi) {
    if (!lo || !hi) return FA_ERR_NULL_POINTER;
    if (totalHeads < 0 || nRanks <= 0 || rank < 0 || rank >= nRanks) return FA_ERR_BAD_SHAPE;
    *lo = (int)(((int64_t)totalHeads * rank) / nRanks);
    *hi = (int)(((int64_t)totalHeads * (rank + 1)) / nRanks);
    return FA_OK;
}

int flash_attention_sharded(int nDevices, const int* deviceIds, const void* const* Q, const void* const* K,
                            const void* const* V, void* const* O, int batchSize, int numHeads, int seqLen, int dHead,
                            float scale, bool is_causal, int dtype, int o_dtype, void* const* streams) {
    if (!deviceIds || !Q || !K || !V || !O) return FA_ERR_NULL_POINTER;
    if (nDevices <= 0 || batchSize <= 0 || numHeads <= 0 || (int64_t)batchSize * numHeads > INT32_MAX / 2) return FA_ERR_BAD_SHAPE;
    int home = 0;
    hipError_t e = hipGetDevice(&home);
    if (e != hipSuccess) return (int)e;
    int rc = FA_OK;
    for (int r = 0; r < nDevices && rc == FA_OK; ++r) {
        int lo = 0, hi = 0;
        flash_attention_shard_range(batchSize * numHeads, r, nDevices, &lo, &hi);
        if (hi == lo) continue;                       // more devices than heads: nothing for this one
        if ((e = hipSetDevice(deviceIds[r])) != hipSuccess) { rc = (int)e; break; }
        // the slab is a [hi-lo, 1, seqLen, dHead] problem of its own
        rc = fa::run(Q[r], K[r], V[r], O[r], nullptr, hi - lo, 1, 1, seqLen, seqLen, dHead, scale, is_causal, dtype, o_dtype,
                     nullptr, nullptr, nullptr, nullptr, streams ? streams[r] : nullptr);
    }
    (void)hipSetDevice(home);
    return rc;
}

int flash_attention_plan(int batchSize, int numHeads, int seqLen, int dHead, bool is_causal, int dtype,
                         int o_dtype, fa_launch_plan* plan) {
    if (!plan) return FA_ERR_NULL_POINTER;
    if (batchSize <= 0 || numHeads <= 0 || seqLen <= 0 || dHead <= 0) return FA_ERR_BAD_SHAPE;
    if (!fa::is_input_dtype(dtype)) return FA_ERR_UNSUPPORTED_DTYPE;
    if (dtype == FA_DTYPE_FP8_E4M3 && dHead > 128) return FA_ERR_UNSUPPORTED_DHEAD;
    if (dHead > 256 || (dHead * fa::elem_size(dtype)) % 16 != 0) return FA_ERR_UNSUPPORTED_DHEAD;
    // (flash_attention_plan_ex with seqLenK = seqLen and bf16 weights: one range)
    *plan = fa::route(batchSize, numHeads, seqLen, seqLen, dHead, is_causal, dtype, o_dtype, 1.0f, FA_FLAG_BF16_WEIGHTS, false).plan();
    return FA_OK;
}

int flash_attention_plan_ex(int batchSize, int numHeads, int seqLenQ, int seqLenK, int dHead, bool is_causal, int dtype,
                            int o_dtype, unsigned flags, fa_launch_plan_ex* early, fa_launch_plan_ex* main_) {
    fa_launch_plan base;
    int rc = flash_attention_plan(batchSize, numHeads, seqLenQ, dHead, is_causal, dtype, o_dtype, &base);
    if (rc != FA_OK) return rc;
    if (seqLenK <= 0) return FA_ERR_BAD_SHAPE;
    if ((rc = fa::check_flags(flags, dtype, dHead)) != FA_OK) return rc;
    const fa::Route r = fa::route(batchSize, numHeads, seqLenQ, seqLenK, dHead, is_causal, dtype, o_dtype, 1.0f, flags, false);
    // early: query blocks [0, hp), main: [hp, nQ).  A range that exists describes the launch; one that does not has grid 0 and the
    // bf16-weights plan's other figures (the early one: the LDS size of the fp16-weights kernel at this d, mask and output type)
    auto fill = [&](fa_launch_plan_ex* out, int qb0, int nq, int empty_lds) {
        if (!out) return;
        out->launch = nq > 0 ? r.plan() : fa_launch_plan{base.q_block_rows, base.kv_block_rows, base.threads, 0, empty_lds, base.kernel_id};
        out->first_q_block = qb0;
        out->q_blocks = nq;
        out->unit_lists = r.unit_lists;
    };
    fill(early, 0, r.hp, (is_causal ? fa::bf16_causal_mix_kernel : fa::bf16_p16_kernel)(dHead, o_dtype).lds_bytes);
    fill(main_, r.hp, r.nQ - r.hp, base.lds_bytes);
    return FA_OK;
}

static size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

size_t flash_attention_backward_workspace_size(int batchSize, int numHeads, int seqLenQ, int dHead) {
    if (batchSize <= 0 || numHeads <= 0 || seqLenQ <= 0 || dHead <= 0) return 0;
    const size_t rows = (size_t)batchSize * numHeads * seqLenQ;
    return round256(rows * sizeof(float)) + round256(rows * dHead * sizeof(float));   // delta, then the fp32 dQ accumulator
}

int flash_attention_backward(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE,
                             void* dQ, void* dK, void* dV, void* workspace, int batchSize, int numHeads, int seqLenQ,
                             int seqLenK, int dHead, float scale, bool is_causal, int dtype, int o_dtype, int grad_dtype,
                             const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                             const fa_strides* sdO, const fa_strides* sdQ, const fa_strides* sdK, const fa_strides* sdV,
                             void* stream) {
    return flash_attention_backward_gqa(Q, K, V, O, dO, LSE, dQ, dK, dV, workspace, batchSize, numHeads, numHeads, seqLenQ, seqLenK,
                                        dHead, scale, is_causal, dtype, o_dtype, grad_dtype, sQ, sK, sV, sO, sdO, sdQ, sdK, sdV, stream);
}

int flash_attention_backward_gqa(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE,
                                 void* dQ, void* dK, void* dV, void* workspace, int batchSize, int numHeads, int numHeadsKV,
                                 int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype, int o_dtype,
                                 int grad_dtype, const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                                 const fa_strides* sO, const fa_strides* sdO, const fa_strides* sdQ, const fa_strides* sdK,
                                 const fa_strides* sdV, void* stream) {
    using namespace fa;
    const void* ptrs[] = {Q, K, V, O, dO, LSE, dQ, dK, dV, workspace};
    for (const void* q : ptrs)
        if (!q) return FA_ERR_NULL_POINTER;
    for (const void* q : ptrs)
        if (!aligned16(q)) return FA_ERR_MISALIGNED;
    const int B = batchSize, H = numHeads, Sq = seqLenQ, Sk = seqLenK, d = dHead;
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0 || d <= 0) return FA_ERR_BAD_SHAPE;
    if ((int64_t)B * H > INT32_MAX / 2 || Sq > (1 << 24) || Sk > (1 << 24)) return FA_ERR_BAD_SHAPE;
    if (!kv_heads_ok(H, numHeadsKV)) return FA_ERR_BAD_SHAPE;
    const int Hkv = numHeadsKV;
    if (!std::isfinite(scale) || !(scale > 0.f)) return FA_ERR_BAD_SCALE;   // (exp2 with the positive scale folded in)
    if (dtype != FA_DTYPE_BF16) return FA_ERR_UNSUPPORTED_DTYPE;
    if (!is_f32_or_bf16(o_dtype) || !is_f32_or_bf16(grad_dtype)) return FA_ERR_UNSUPPORTED_DTYPE;
    if (d != 64 && d != 128) return FA_ERR_UNSUPPORTED_DHEAD;
    const int esz = elem_size(dtype), osz = elem_size(o_dtype), gsz = elem_size(grad_dtype);
    if (!strides_ok(sQ, esz, d) || !strides_ok(sK, esz, d) || !strides_ok(sV, esz, d) || !strides_ok(sO, osz, d) ||
        !strides_ok(sdO, osz, d) || !strides_ok(sdQ, gsz, d) || !strides_ok(sdK, gsz, d) || !strides_ok(sdV, gsz, d))
        return FA_ERR_BAD_STRIDE;
    // the forward's MFMA-path limit on one head's K / V extent
    const int64_t extent = (int64_t)Sk + KV_EXTENT_SLACK;
    if (!kv_extent_ok(extent, sK ? sK->strideS : d, esz) || !kv_extent_ok(extent, sV ? sV->strideS : d, esz)) return FA_ERR_BAD_SHAPE;
    // the main kernel's grid: one workgroup per 256-key block of every (batch, K/V head)
    const int64_t heads = (int64_t)B * H, kv_heads = (int64_t)B * Hkv, nK = (Sk + 255) / 256, rows = heads * Sq;
    if (kv_heads * nK > INT32_MAX || rows * d / 4 / 256 + 1 > INT32_MAX) return FA_ERR_BAD_SHAPE;

    BwdParams p;
    p.Q = (const __bf16*)Q; p.K = (const __bf16*)K; p.V = (const __bf16*)V; p.O = O; p.dO = dO; p.lse = LSE;
    p.dQ = dQ; p.dK = dK; p.dV = dV;
    p.delta = (float*)workspace;
    p.dq_acc = (float*)((char*)workspace + round256((size_t)rows * sizeof(float)));
    resolve_strides(sQ, H, Sq, d, p.qB, p.qH, p.qS);       resolve_strides(sO, H, Sq, d, p.oB, p.oH, p.oS);
    resolve_strides(sdO, H, Sq, d, p.doB, p.doH, p.doS);   resolve_strides(sdQ, H, Sq, d, p.dqB, p.dqH, p.dqS);
    resolve_strides(sK, Hkv, Sk, d, p.kB, p.kH, p.kS);     resolve_strides(sV, Hkv, Sk, d, p.vB, p.vH, p.vS);
    resolve_strides(sdK, Hkv, Sk, d, p.dkB, p.dkH, p.dkS); resolve_strides(sdV, Hkv, Sk, d, p.dvB, p.dvH, p.dvS);
    p.H = H; p.Sq = Sq; p.Sk = Sk;
    p.heads = (int)heads;
    p.Hkv = Hkv; p.group = H / Hkv;
    p.kv_heads = (int)kv_heads;
    p.nK = (int)nK;
    p.scale = scale;
    p.inv_scale = 1.0f / scale;
    p.c = scale * 1.4426950408889634f;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int rpb = 256 / (d / 8);
    hipError_t e = launch(bwd_pre_kernel_of(d, o_dtype), (unsigned)((rows + rpb - 1) / rpb), 256, 0, st, p);
    if (e != hipSuccess) return (int)e;
    const Kernel mk = bwd_main_kernel_of(d, is_causal, o_dtype, grad_dtype, p.group > 1);
    if ((e = launch(mk, (unsigned)(kv_heads * nK), 256, mk.lds_bytes, st, p)) != hipSuccess) return (int)e;
    return (int)launch(bwd_post_kernel_of(d, grad_dtype), (unsigned)((rows * d / 4 + 255) / 256), 256, 0, st, p);
}

// The three plan functions: the shape's refusals, then what the route launches
static int split_plan(const fa::SplitCall& c, fa_decode_plan* plan) {
    using namespace fa;
    if (!plan) return FA_ERR_NULL_POINTER;
    const int rc = decode_check_shape(c);
    if (rc != FA_OK) return rc;
    const DecodeRoute r = decode_route(c);
    plan->num_splits = r.ns;
    plan->row_blocks = r.row_blocks;
    plan->rows_per_block = c.form.rows_per_block;
    plan->kv_block_rows = DecodeCfg<128>::TILE;
    plan->threads = DecodeCfg<128>::THREADS;
    plan->grid = (int)r.grid;
    plan->lds_bytes = c.d == 128 ? DecodeCfg<128>::LDS_BYTES : DecodeCfg<64>::LDS_BYTES;
    // one workgroup per (batch, head, query row); ragged: per (head, token)
    plan->combine_grid = r.ns > 1 ? (int)((int64_t)(c.form.varlen ? 1 : c.B) * c.H * c.Sq) : 0;
    plan->combine_threads = r.ns > 1 ? 256 : 0;
    return FA_OK;
}

int flash_attention_decode_plan_window(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, int o_dtype,
                                       int numSplits, int windowSize, fa_decode_plan* plan) {
    return split_plan({.form = fa::decode_form(), .cache = {.capacity = seqLenK}, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV,
                       .Sq = seqLenQ, .d = dHead, .dtype = FA_DTYPE_BF16, .o_dtype = o_dtype, .num_splits = numSplits, .window = windowSize},
                      plan);
}

int flash_attention_decode_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, int o_dtype,
                                int numSplits, fa_decode_plan* plan) {
    return flash_attention_decode_plan_window(batchSize, numHeads, numHeadsKV, seqLenQ, seqLenK, dHead, o_dtype, numSplits, 0, plan);
}

size_t flash_attention_decode_workspace_size(int batchSize, int numHeads, int seqLenQ, int dHead, int numSplits) {
    if (batchSize <= 0 || numHeads <= 0 || seqLenQ <= 0 || dHead <= 0 || numSplits <= 1) return 0;
    const size_t rows = (size_t)batchSize * numHeads * seqLenQ;
    return fa::round16(rows * numSplits * dHead * sizeof(float)) + fa::round16(rows * numSplits * sizeof(float));   // partial O, then partial LSE
}

int flash_attention_decode(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens, void* workspace,
                           int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale,
                           bool is_causal, int dtype, int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sK,
                           const fa_strides* sV, const fa_strides* sO, void* stream) {
    return fa::decode_run({.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = K, .V = V, .kv_lens = kvLens, .kv_dtype = FA_DTYPE_BF16, .capacity = seqLenK, .sK = sK, .sV = sV},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .sQ = sQ, .sO = sO, .stream = stream});
}

int flash_attention_decode_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                                 const int32_t* blockTable, void* workspace, int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                                 int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead, float scale,
                                 bool is_causal, int dtype, int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sK,
                                 const fa_strides* sV, const fa_strides* sO, void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::decode_run({.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .kv_dtype = FA_DTYPE_BF16, .sK = sK, .sV = sV, .paging = &pg},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .sQ = sQ, .sO = sO, .stream = stream});
}

int flash_attention_decode_fp8(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens,
                               const float* kDescale, const float* vDescale, void* workspace, int batchSize, int numHeads,
                               int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype, int kv_dtype,
                               int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                               const fa_strides* sO, void* stream) {
    if (kv_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED_DTYPE;
    return fa::decode_run({.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                                     .capacity = seqLenK, .sK = sK, .sV = sV},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .sQ = sQ, .sO = sO, .stream = stream});
}

int flash_attention_decode_paged_fp8(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                                     const int32_t* blockTable, const float* kDescale, const float* vDescale, void* workspace,
                                     int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int numPages, int pageSize,
                                     int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                     int kv_dtype, int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sK,
                                     const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (kv_dtype != FA_DTYPE_FP8_E4M3) return FA_ERR_UNSUPPORTED_DTYPE;
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::decode_run({.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                     .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .sQ = sQ, .sO = sO, .stream = stream});
}

// a bf16 cache has no descales: the logical cache is what lies in memory
static bool window_descales_ok(int kv_dtype, const float* kDescale, const float* vDescale) {
    return kv_dtype == FA_DTYPE_FP8_E4M3 || (!kDescale && !vDescale);
}

int flash_attention_sink_decode(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens,
                                const float* kDescale, const float* vDescale, const float* sinks, void* workspace, int batchSize,
                                int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype,
                                int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                                const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    return fa::decode_run({.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                                     .capacity = seqLenK, .sK = sK, .sV = sV},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks});
}

int flash_attention_decode_window(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens,
                                  const float* kDescale, const float* vDescale, void* workspace, int batchSize, int numHeads,
                                  int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype,
                                  int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                                  const fa_strides* sV, const fa_strides* sO, void* stream) {
    return flash_attention_sink_decode(Q, K, V, O, LSE, kvLens, kDescale, vDescale, nullptr, workspace, batchSize, numHeads, numHeadsKV,
                                       seqLenQ, seqLenK, dHead, scale, is_causal, dtype, kv_dtype, o_dtype, numSplits, windowSize, sQ, sK,
                                       sV, sO, stream);
}

int flash_attention_sink_decode_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                                      const int32_t* blockTable, const float* kDescale, const float* vDescale, const float* sinks,
                                      void* workspace, int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int numPages, int pageSize,
                                      int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                      int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                                      const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::decode_run({.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                     .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks});
}

int flash_attention_decode_paged_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                                        const int32_t* blockTable, const float* kDescale, const float* vDescale, void* workspace,
                                        int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int numPages, int pageSize,
                                        int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                        int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ,
                                        const fa_strides* sK, const fa_strides* sV, const fa_strides* sO, void* stream) {
    return flash_attention_sink_decode_paged(Q, Kpool, Vpool, O, LSE, kvLens, blockTable, kDescale, vDescale, nullptr, workspace, batchSize,
                                             numHeads, numHeadsKV, seqLenQ, numPages, pageSize, maxPagesPerSeq, tableStride, dHead, scale,
                                             is_causal, dtype, kv_dtype, o_dtype, numSplits, windowSize, sQ, sK, sV, sO, stream);
}

int flash_attention_extend_plan_window(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, int o_dtype,
                                       int numSplits, int windowSize, fa_decode_plan* plan) {
    return split_plan({.form = fa::extend_form(dHead), .cache = {.capacity = seqLenK}, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV,
                       .Sq = seqLenQ, .d = dHead, .dtype = FA_DTYPE_BF16, .o_dtype = o_dtype, .num_splits = numSplits, .window = windowSize},
                      plan);
}

int flash_attention_extend_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, int o_dtype,
                                int numSplits, fa_decode_plan* plan) {
    return flash_attention_extend_plan_window(batchSize, numHeads, numHeadsKV, seqLenQ, seqLenK, dHead, o_dtype, numSplits, 0, plan);
}

int flash_attention_sink_extend(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens,
                                const float* kDescale, const float* vDescale, const float* sinks, void* workspace, int batchSize,
                                int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype,
                                int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                                const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    return fa::decode_run({.form = fa::extend_form(dHead), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                                     .capacity = seqLenK, .sK = sK, .sV = sV},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks});
}

int flash_attention_extend_window(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens,
                           const float* kDescale, const float* vDescale, void* workspace, int batchSize, int numHeads,
                           int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype, int kv_dtype,
                           int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                           const fa_strides* sO, void* stream) {
    return flash_attention_sink_extend(Q, K, V, O, LSE, kvLens, kDescale, vDescale, nullptr, workspace, batchSize, numHeads, numHeadsKV,
                                       seqLenQ, seqLenK, dHead, scale, is_causal, dtype, kv_dtype, o_dtype, numSplits, windowSize, sQ, sK,
                                       sV, sO, stream);
}

int flash_attention_extend(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens,
                           const float* kDescale, const float* vDescale, void* workspace, int batchSize, int numHeads,
                           int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype, int kv_dtype,
                           int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                           const fa_strides* sO, void* stream) {
    return flash_attention_extend_window(Q, K, V, O, LSE, kvLens, kDescale, vDescale, workspace, batchSize, numHeads, numHeadsKV, seqLenQ,
                                         seqLenK, dHead, scale, is_causal, dtype, kv_dtype, o_dtype, numSplits, 0, sQ, sK, sV, sO, stream);
}

int flash_attention_sink_extend_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                                      const int32_t* blockTable, const float* kDescale, const float* vDescale, const float* sinks,
                                      void* workspace, int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int numPages, int pageSize,
                                      int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                      int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                                      const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::decode_run({.form = fa::extend_form(dHead), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                     .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks});
}

int flash_attention_extend_paged_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                                 const int32_t* blockTable, const float* kDescale, const float* vDescale, void* workspace,
                                 int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int numPages, int pageSize,
                                 int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                 int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                                 const fa_strides* sV, const fa_strides* sO, void* stream) {
    return flash_attention_sink_extend_paged(Q, Kpool, Vpool, O, LSE, kvLens, blockTable, kDescale, vDescale, nullptr, workspace, batchSize,
                                             numHeads, numHeadsKV, seqLenQ, numPages, pageSize, maxPagesPerSeq, tableStride, dHead, scale,
                                             is_causal, dtype, kv_dtype, o_dtype, numSplits, windowSize, sQ, sK, sV, sO, stream);
}

int flash_attention_extend_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                                 const int32_t* blockTable, const float* kDescale, const float* vDescale, void* workspace,
                                 int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int numPages, int pageSize,
                                 int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                 int kv_dtype, int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sK,
                                 const fa_strides* sV, const fa_strides* sO, void* stream) {
    return flash_attention_extend_paged_window(Q, Kpool, Vpool, O, LSE, kvLens, blockTable, kDescale, vDescale, workspace, batchSize,
                                               numHeads, numHeadsKV, seqLenQ, numPages, pageSize, maxPagesPerSeq, tableStride, dHead, scale,
                                               is_causal, dtype, kv_dtype, o_dtype, numSplits, 0, sQ, sK, sV, sO, stream);
}

int flash_attention_kv_append(const void* Knew, const void* Vnew, void* K, void* V, const int32_t* kvLens, const float* kDescale,
                              const float* vDescale, int batchSize, int numHeadsKV, int seqLenNew, int seqLenK, int dHead, int dtype,
                              int kv_dtype, const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sK, const fa_strides* sV,
                              void* stream) {
    return fa::kv_append_run({.varlen = false, .Knew = Knew, .Vnew = Vnew,
                              .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .capacity = seqLenK, .sK = sK, .sV = sV},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenNew, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream});
}

int flash_attention_kv_append_paged(const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int32_t* kvLens,
                                    const int32_t* blockTable, const float* kDescale, const float* vDescale, int batchSize,
                                    int numHeadsKV, int seqLenNew, int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride,
                                    int dHead, int dtype, int kv_dtype, const fa_strides* sKnew, const fa_strides* sVnew,
                                    const fa_strides* sK, const fa_strides* sV, void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::kv_append_run({.varlen = false, .Knew = Knew, .Vnew = Vnew,
                              .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenNew, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream});
}

int flash_attention_extend_varlen_plan_window(int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                              int o_dtype, int numSplits, int windowSize, fa_decode_plan* plan) {
    return split_plan({.form = fa::extend_varlen_form(dHead), .cache = {.capacity = seqLenK}, .B = batchSize, .H = numHeads,
                       .Hkv = numHeadsKV, .Sq = totalQ, .d = dHead, .dtype = FA_DTYPE_BF16, .o_dtype = o_dtype, .num_splits = numSplits,
                       .window = windowSize},
                      plan);
}

int flash_attention_extend_varlen_plan(int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead, int o_dtype,
                                       int numSplits, fa_decode_plan* plan) {
    return flash_attention_extend_varlen_plan_window(batchSize, numHeads, numHeadsKV, totalQ, seqLenK, dHead, o_dtype, numSplits, 0,
                                                     plan);
}

int flash_attention_sink_extend_varlen(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* cuSeqlensQ,
                                       const int32_t* kvLens, const float* kDescale, const float* vDescale, const float* sinks,
                                       void* workspace, int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead,
                                       float scale, bool is_causal, int dtype, int kv_dtype, int o_dtype, int numSplits, int windowSize,
                                       const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                       void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    return fa::decode_run({.form = fa::extend_varlen_form(dHead), .Q = Q, .O = O, .LSE = LSE, .cu_seqlens_q = cuSeqlensQ,
                           .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                                     .capacity = seqLenK, .sK = sK, .sV = sV},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = totalQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks});
}

int flash_attention_extend_varlen_window(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* cuSeqlensQ,
                                  const int32_t* kvLens, const float* kDescale, const float* vDescale, void* workspace, int batchSize,
                                  int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype,
                                  int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                                  const fa_strides* sV, const fa_strides* sO, void* stream) {
    return flash_attention_sink_extend_varlen(Q, K, V, O, LSE, cuSeqlensQ, kvLens, kDescale, vDescale, nullptr, workspace, batchSize,
                                              numHeads, numHeadsKV, totalQ, seqLenK, dHead, scale, is_causal, dtype, kv_dtype, o_dtype,
                                              numSplits, windowSize, sQ, sK, sV, sO, stream);
}

int flash_attention_extend_varlen(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* cuSeqlensQ,
                                  const int32_t* kvLens, const float* kDescale, const float* vDescale, void* workspace, int batchSize,
                                  int numHeads, int numHeadsKV, int totalQ, int seqLenK, int dHead, float scale, bool is_causal, int dtype,
                                  int kv_dtype, int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sK,
                                  const fa_strides* sV, const fa_strides* sO, void* stream) {
    return flash_attention_extend_varlen_window(Q, K, V, O, LSE, cuSeqlensQ, kvLens, kDescale, vDescale, workspace, batchSize, numHeads,
                                                numHeadsKV, totalQ, seqLenK, dHead, scale, is_causal, dtype, kv_dtype, o_dtype, numSplits,
                                                0, sQ, sK, sV, sO, stream);
}

int flash_attention_sink_extend_paged_varlen(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                             const int32_t* cuSeqlensQ, const int32_t* kvLens, const int32_t* blockTable,
                                             const float* kDescale, const float* vDescale, const float* sinks, void* workspace,
                                             int batchSize, int numHeads, int numHeadsKV, int totalQ, int numPages, int pageSize,
                                             int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                             int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ,
                                             const fa_strides* sK, const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::decode_run({.form = fa::extend_varlen_form(dHead), .Q = Q, .O = O, .LSE = LSE, .cu_seqlens_q = cuSeqlensQ,
                           .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                     .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = totalQ, .d = dHead,
                           .scale = scale, .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks});
}

int flash_attention_extend_paged_varlen_window(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                        const int32_t* cuSeqlensQ, const int32_t* kvLens, const int32_t* blockTable,
                                        const float* kDescale, const float* vDescale, void* workspace, int batchSize, int numHeads,
                                        int numHeadsKV, int totalQ, int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride,
                                        int dHead, float scale, bool is_causal, int dtype, int kv_dtype, int o_dtype, int numSplits, int windowSize,
                                        const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                        void* stream) {
    return flash_attention_sink_extend_paged_varlen(Q, Kpool, Vpool, O, LSE, cuSeqlensQ, kvLens, blockTable, kDescale, vDescale, nullptr,
                                                    workspace, batchSize, numHeads, numHeadsKV, totalQ, numPages, pageSize, maxPagesPerSeq,
                                                    tableStride, dHead, scale, is_causal, dtype, kv_dtype, o_dtype, numSplits, windowSize,
                                                    sQ, sK, sV, sO, stream);
}

int flash_attention_extend_paged_varlen(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE,
                                        const int32_t* cuSeqlensQ, const int32_t* kvLens, const int32_t* blockTable,
                                        const float* kDescale, const float* vDescale, void* workspace, int batchSize, int numHeads,
                                        int numHeadsKV, int totalQ, int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride,
                                        int dHead, float scale, bool is_causal, int dtype, int kv_dtype, int o_dtype, int numSplits,
                                        const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV, const fa_strides* sO,
                                        void* stream) {
    return flash_attention_extend_paged_varlen_window(Q, Kpool, Vpool, O, LSE, cuSeqlensQ, kvLens, blockTable, kDescale, vDescale,
                                                      workspace, batchSize, numHeads, numHeadsKV, totalQ, numPages, pageSize,
                                                      maxPagesPerSeq, tableStride, dHead, scale, is_causal, dtype, kv_dtype, o_dtype,
                                                      numSplits, 0, sQ, sK, sV, sO, stream);
}

int flash_attention_kv_append_varlen(const void* Knew, const void* Vnew, void* K, void* V, const int32_t* cuSeqlensQ,
                                     const int32_t* kvLens, const float* kDescale, const float* vDescale, int batchSize, int numHeadsKV,
                                     int totalQ, int seqLenK, int dHead, int dtype, int kv_dtype, const fa_strides* sKnew,
                                     const fa_strides* sVnew, const fa_strides* sK, const fa_strides* sV, void* stream) {
    return fa::kv_append_run({.varlen = true, .Knew = Knew, .Vnew = Vnew, .cu_seqlens_q = cuSeqlensQ,
                              .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .capacity = seqLenK, .sK = sK, .sV = sV},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = totalQ, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream});
}

int flash_attention_kv_append_paged_varlen(const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int32_t* cuSeqlensQ,
                                           const int32_t* kvLens, const int32_t* blockTable, const float* kDescale,
                                           const float* vDescale, int batchSize, int numHeadsKV, int totalQ, int numPages, int pageSize,
                                           int maxPagesPerSeq, int64_t tableStride, int dHead, int dtype, int kv_dtype,
                                           const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sK, const fa_strides* sV,
                                           void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::kv_append_run({.varlen = true, .Knew = Knew, .Vnew = Vnew, .cu_seqlens_q = cuSeqlensQ,
                              .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = totalQ, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream});
}

int flash_attention_rope_append(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* K, void* V, const float* cosSin,
                                const int32_t* kvLens, const float* kDescale, const float* vDescale, int batchSize, int numHeads,
                                int numHeadsKV, int seqLenNew, int seqLenK, int dHead, int rotDim, int maxPos, int interleaved, int dtype,
                                int kv_dtype, const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew,
                                const fa_strides* sQout, const fa_strides* sK, const fa_strides* sV, void* stream) {
    const fa::RopeCall rope{Q, Qout, cosSin, numHeads, rotDim, maxPos, interleaved, sQ, sQout};
    return fa::kv_append_run({.varlen = false, .Knew = Knew, .Vnew = Vnew,
                              .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .capacity = seqLenK, .sK = sK, .sV = sV},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenNew, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream},
                             &rope);
}

int flash_attention_rope_append_paged(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                      const float* cosSin, const int32_t* kvLens, const int32_t* blockTable, const float* kDescale,
                                      const float* vDescale, int batchSize, int numHeads, int numHeadsKV, int seqLenNew, int numPages,
                                      int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead, int rotDim, int maxPos,
                                      int interleaved, int dtype, int kv_dtype, const fa_strides* sQ, const fa_strides* sKnew,
                                      const fa_strides* sVnew, const fa_strides* sQout, const fa_strides* sK, const fa_strides* sV,
                                      void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    const fa::RopeCall rope{Q, Qout, cosSin, numHeads, rotDim, maxPos, interleaved, sQ, sQout};
    return fa::kv_append_run({.varlen = false, .Knew = Knew, .Vnew = Vnew,
                              .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenNew, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream},
                             &rope);
}

int flash_attention_rope_append_varlen(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* K, void* V,
                                       const float* cosSin, const int32_t* cuSeqlensQ, const int32_t* kvLens, const float* kDescale,
                                       const float* vDescale, int batchSize, int numHeads, int numHeadsKV, int totalQ, int seqLenK,
                                       int dHead, int rotDim, int maxPos, int interleaved, int dtype, int kv_dtype, const fa_strides* sQ,
                                       const fa_strides* sKnew, const fa_strides* sVnew, const fa_strides* sQout, const fa_strides* sK,
                                       const fa_strides* sV, void* stream) {
    const fa::RopeCall rope{Q, Qout, cosSin, numHeads, rotDim, maxPos, interleaved, sQ, sQout};
    return fa::kv_append_run({.varlen = true, .Knew = Knew, .Vnew = Vnew, .cu_seqlens_q = cuSeqlensQ,
                              .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .capacity = seqLenK, .sK = sK, .sV = sV},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = totalQ, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream},
                             &rope);
}

int flash_attention_rope_append_paged_varlen(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                             const float* cosSin, const int32_t* cuSeqlensQ, const int32_t* kvLens,
                                             const int32_t* blockTable, const float* kDescale, const float* vDescale, int batchSize,
                                             int numHeads, int numHeadsKV, int totalQ, int numPages, int pageSize, int maxPagesPerSeq,
                                             int64_t tableStride, int dHead, int rotDim, int maxPos, int interleaved, int dtype,
                                             int kv_dtype, const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew,
                                             const fa_strides* sQout, const fa_strides* sK, const fa_strides* sV, void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    const fa::RopeCall rope{Q, Qout, cosSin, numHeads, rotDim, maxPos, interleaved, sQ, sQout};
    return fa::kv_append_run({.varlen = true, .Knew = Knew, .Vnew = Vnew, .cu_seqlens_q = cuSeqlensQ,
                              .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = totalQ, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream},
                             &rope);
}

// ---- the speculative step's write side: the rope twins with posOffsets after cosSin; in-cache acceptance ----
int flash_attention_rope_append_pos(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* K, void* V, const float* cosSin,
                                    const int32_t* posOffsets, const int32_t* kvLens, const float* kDescale, const float* vDescale,
                                    int batchSize, int numHeads, int numHeadsKV, int seqLenNew, int seqLenK, int dHead, int rotDim,
                                    int maxPos, int interleaved, int dtype, int kv_dtype, const fa_strides* sQ, const fa_strides* sKnew,
                                    const fa_strides* sVnew, const fa_strides* sQout, const fa_strides* sK, const fa_strides* sV,
                                    void* stream) {
    const fa::RopeCall rope{Q, Qout, cosSin, numHeads, rotDim, maxPos, interleaved, sQ, sQout, true, posOffsets};
    return fa::kv_append_run({.varlen = false, .Knew = Knew, .Vnew = Vnew,
                              .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .capacity = seqLenK, .sK = sK, .sV = sV},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenNew, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream},
                             &rope);
}

int flash_attention_rope_append_paged_pos(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                          const float* cosSin, const int32_t* posOffsets, const int32_t* kvLens,
                                          const int32_t* blockTable, const float* kDescale, const float* vDescale, int batchSize,
                                          int numHeads, int numHeadsKV, int seqLenNew, int numPages, int pageSize, int maxPagesPerSeq,
                                          int64_t tableStride, int dHead, int rotDim, int maxPos, int interleaved, int dtype,
                                          int kv_dtype, const fa_strides* sQ, const fa_strides* sKnew, const fa_strides* sVnew,
                                          const fa_strides* sQout, const fa_strides* sK, const fa_strides* sV, void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    const fa::RopeCall rope{Q, Qout, cosSin, numHeads, rotDim, maxPos, interleaved, sQ, sQout, true, posOffsets};
    return fa::kv_append_run({.varlen = false, .Knew = Knew, .Vnew = Vnew,
                              .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                        .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                              .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenNew, .d = dHead, .dtype = dtype, .sKnew = sKnew,
                              .sVnew = sVnew, .stream = stream},
                             &rope);
}

int flash_attention_kv_accept(void* K, void* V, const int32_t* kvLens, const int32_t* acceptIdx, const int32_t* acceptLens,
                              int batchSize, int numHeadsKV, int seqLenDraft, int seqLenK, int dHead, int kv_dtype, const fa_strides* sK,
                              const fa_strides* sV, void* stream) {
    return fa::kv_accept_run({.cache = {.K = K, .V = V, .kv_lens = kvLens, .kv_dtype = kv_dtype, .capacity = seqLenK, .sK = sK, .sV = sV},
                              .accept_idx = acceptIdx, .accept_lens = acceptLens, .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenDraft,
                              .d = dHead, .stream = stream});
}

int flash_attention_kv_accept_paged(void* Kpool, void* Vpool, const int32_t* kvLens, const int32_t* blockTable, const int32_t* acceptIdx,
                                    const int32_t* acceptLens, int batchSize, int numHeadsKV, int seqLenDraft, int numPages,
                                    int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead, int kv_dtype, const fa_strides* sK,
                                    const fa_strides* sV, void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::kv_accept_run({.cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                              .accept_idx = acceptIdx, .accept_lens = acceptLens, .B = batchSize, .Hkv = numHeadsKV, .Sq = seqLenDraft,
                              .d = dHead, .stream = stream});
}

// ---- tree-masked verification: the sinks entry points of decode with the mask words, is_causal set ----
// the call family of a draft of seqLenQ nodes: decode's up to FA_DECODE_MAX_Q, chunked prefill's above (any d but 64 / 128 is refused later)
static fa::SplitForm tree_form(int seqLenQ, int dHead) { return seqLenQ <= FA_DECODE_MAX_Q ? fa::decode_form() : fa::extend_form(dHead); }

int flash_attention_tree_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenK, int dHead, int o_dtype, int numSplits,
                              int windowSize, fa_decode_plan* plan) {
    if (!plan) return FA_ERR_NULL_POINTER;
    if (seqLenQ > FA_TREE_MAX_Q) return FA_ERR_BAD_SHAPE;
    return seqLenQ <= FA_DECODE_MAX_Q
               ? flash_attention_decode_plan_window(batchSize, numHeads, numHeadsKV, seqLenQ, seqLenK, dHead, o_dtype, numSplits, windowSize, plan)
               : flash_attention_extend_plan_window(batchSize, numHeads, numHeadsKV, seqLenQ, seqLenK, dHead, o_dtype, numSplits, windowSize, plan);
}

int flash_attention_tree(const void* Q, const void* K, const void* V, void* O, float* LSE, const int32_t* kvLens, const float* kDescale,
                         const float* vDescale, const float* sinks, const uint64_t* treeMask, void* workspace, int batchSize, int numHeads,
                         int numHeadsKV, int seqLenQ, int seqLenK, int dHead, float scale, int dtype, int kv_dtype, int o_dtype,
                         int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK, const fa_strides* sV,
                         const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    if (!treeMask) return FA_ERR_NULL_POINTER;   // (with the other pointers: decode_run's first step returns the same code)
    return fa::decode_run({.form = tree_form(seqLenQ, dHead), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                                     .capacity = seqLenK, .sK = sK, .sV = sV},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = true, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks, .tree_mask = treeMask});
}

int flash_attention_tree_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* kvLens,
                               const int32_t* blockTable, const float* kDescale, const float* vDescale, const float* sinks,
                               const uint64_t* treeMask, void* workspace, int batchSize, int numHeads, int numHeadsKV, int seqLenQ,
                               int numPages, int pageSize, int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, int dtype,
                               int kv_dtype, int o_dtype, int numSplits, int windowSize, const fa_strides* sQ, const fa_strides* sK,
                               const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    if (!treeMask) return FA_ERR_NULL_POINTER;
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::decode_run({.form = tree_form(seqLenQ, dHead), .Q = Q, .O = O, .LSE = LSE,
                           .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale,
                                     .kv_dtype = kv_dtype, .sK = sK, .sV = sV, .paging = &pg},
                           .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead,
                           .scale = scale, .is_causal = true, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits,
                           .window = windowSize, .sQ = sQ, .sO = sO, .stream = stream, .sinks = sinks, .tree_mask = treeMask});
}

// ---- shared-prefix (cascade) decode ----
int flash_attention_cascade_plan(int batchSize, int numHeads, int numHeadsKV, int seqLenQ, int seqLenShared, int seqLenK, int dHead,
                                 int o_dtype, int numSplitsShared, int numSplitsUnique, fa_cascade_plan* plan) {
    using namespace fa;
    if (!plan) return FA_ERR_NULL_POINTER;
    const CascadeCall c{.u = {.form = decode_form(), .cache = {.capacity = seqLenK}, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV,
                              .Sq = seqLenQ, .d = dHead, .dtype = FA_DTYPE_BF16, .o_dtype = o_dtype, .num_splits = numSplitsUnique},
                        .shared = {.capacity = seqLenShared}, .num_splits_shared = numSplitsShared};
    int rc = cascade_check_shape(c);
    if (rc != FA_OK) return rc;
    const CascadeRoute r = cascade_route(c);
    if ((rc = flash_attention_decode_plan(batchSize, numHeads, numHeadsKV, seqLenQ, seqLenK, dHead, o_dtype, r.ns_u, &plan->unique)) != FA_OK)
        return rc;
    const SplitForm f = extend_form(dHead);
    plan->shared = plan->unique;   // (the tile, the threads, the LDS and the combine are the same)
    plan->shared.num_splits = r.ns_s;
    plan->shared.row_blocks = r.row_blocks_s;
    plan->shared.rows_per_block = f.rows_per_block;
    plan->shared.grid = (int)r.grid_s;
    plan->num_splits = r.ns_s + r.ns_u;
    return FA_OK;
}

int flash_attention_cascade_decode(const void* Q, const void* Kshared, const void* Vshared, const void* K, const void* V, void* O,
                                   float* LSE, const int32_t* sharedLen, const int32_t* kvLens, const float* kDescale,
                                   const float* vDescale, const float* sinks, void* workspace, int batchSize, int numHeads,
                                   int numHeadsKV, int seqLenQ, int seqLenShared, int seqLenK, int dHead, float scale, bool is_causal,
                                   int dtype, int kv_dtype, int o_dtype, int numSplitsShared, int numSplitsUnique, const fa_strides* sQ,
                                   const fa_strides* sKshared, const fa_strides* sVshared, const fa_strides* sK, const fa_strides* sV,
                                   const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    return fa::cascade_run(
        {.u = {.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
               .cache = {.K = K, .V = V, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                         .capacity = seqLenK, .sK = sK, .sV = sV},
               .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead, .scale = scale,
               .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplitsUnique, .sQ = sQ, .sO = sO,
               .stream = stream, .sinks = sinks},
         .shared = {.K = Kshared, .V = Vshared, .kv_lens = sharedLen, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                    .capacity = seqLenShared, .sK = sKshared, .sV = sVshared},
         .num_splits_shared = numSplitsShared});
}

int flash_attention_cascade_decode_paged(const void* Q, const void* Kpool, const void* Vpool, void* O, float* LSE, const int32_t* sharedLen,
                                         const int32_t* kvLens, const int32_t* sharedTable, const int32_t* blockTable,
                                         const float* kDescale, const float* vDescale, const float* sinks, void* workspace, int batchSize,
                                         int numHeads, int numHeadsKV, int seqLenQ, int numPages, int pageSize, int maxSharedPages,
                                         int maxPagesPerSeq, int64_t tableStride, int dHead, float scale, bool is_causal, int dtype,
                                         int kv_dtype, int o_dtype, int numSplitsShared, int numSplitsUnique, const fa_strides* sQ,
                                         const fa_strides* sK, const fa_strides* sV, const fa_strides* sO, void* stream) {
    if (!window_descales_ok(kv_dtype, kDescale, vDescale)) return FA_ERR_UNSUPPORTED_DTYPE;
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    const fa::DecodePaging spg{sharedTable, maxSharedPages, numPages, pageSize, maxSharedPages};   // one row
    return fa::cascade_run(
        {.u = {.form = fa::decode_form(), .Q = Q, .O = O, .LSE = LSE,
               .cache = {.K = Kpool, .V = Vpool, .kv_lens = kvLens, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                         .sK = sK, .sV = sV, .paging = &pg},
               .workspace = workspace, .B = batchSize, .H = numHeads, .Hkv = numHeadsKV, .Sq = seqLenQ, .d = dHead, .scale = scale,
               .is_causal = is_causal, .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplitsUnique, .sQ = sQ, .sO = sO,
               .stream = stream, .sinks = sinks},
         .shared = {.K = Kpool, .V = Vpool, .kv_lens = sharedLen, .k_descale = kDescale, .v_descale = vDescale, .kv_dtype = kv_dtype,
                    .sK = sK, .sV = sV, .paging = &spg},
         .num_splits_shared = numSplitsShared});
}

// ---- MLA decode ----
int flash_attention_mla_decode_plan(int batchSize, int numHeads, int seqLenQ, int seqLenK, int dLatent, int dRope, int o_dtype,
                                    int numSplits, fa_decode_plan* plan) {
    using namespace fa;
    if (!plan) return FA_ERR_NULL_POINTER;
    const MlaCall c{.B = batchSize, .H = numHeads, .Sq = seqLenQ, .capacity = seqLenK, .d_latent = dLatent, .d_rope = dRope,
                    .dtype = FA_DTYPE_BF16, .o_dtype = o_dtype, .num_splits = numSplits};
    const int rc = mla_check_shape(c);
    if (rc != FA_OK) return rc;
    const DecodeRoute r = mla_route(c);
    plan->num_splits = r.ns;
    plan->row_blocks = r.row_blocks;
    plan->rows_per_block = MlaCfg::ROWS;
    plan->kv_block_rows = MlaCfg::KT;
    plan->threads = MlaCfg::THREADS;
    plan->grid = (int)r.grid;
    plan->lds_bytes = MlaCfg::LDS_BYTES;
    plan->combine_grid = r.ns > 1 ? (int)((int64_t)batchSize * numHeads * seqLenQ) : 0;   // one workgroup per (batch, head, query row)
    plan->combine_threads = r.ns > 1 ? 256 : 0;
    return FA_OK;
}

size_t flash_attention_mla_decode_workspace_size(int batchSize, int numHeads, int seqLenQ, int dLatent, int numSplits) {
    return flash_attention_decode_workspace_size(batchSize, numHeads, seqLenQ, dLatent, numSplits);
}

int flash_attention_mla_decode(const void* Q, const void* KV, void* O, float* LSE, const int32_t* kvLens, void* workspace, int batchSize,
                               int numHeads, int seqLenQ, int seqLenK, int dLatent, int dRope, float scale, bool is_causal, int dtype,
                               int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sKV, const fa_strides* sO, void* stream) {
    return fa::mla_run({.Q = Q, .KV = KV, .O = O, .LSE = LSE, .kv_lens = kvLens, .workspace = workspace, .B = batchSize, .H = numHeads,
                        .Sq = seqLenQ, .capacity = seqLenK, .d_latent = dLatent, .d_rope = dRope, .scale = scale, .is_causal = is_causal,
                        .dtype = dtype, .o_dtype = o_dtype, .num_splits = numSplits, .sQ = sQ, .sKV = sKV, .sO = sO, .stream = stream});
}

int flash_attention_mla_decode_paged(const void* Q, const void* KVpool, void* O, float* LSE, const int32_t* kvLens,
                                     const int32_t* blockTable, void* workspace, int batchSize, int numHeads, int seqLenQ, int numPages,
                                     int pageSize, int maxPagesPerSeq, int64_t tableStride, int dLatent, int dRope, float scale,
                                     bool is_causal, int dtype, int o_dtype, int numSplits, const fa_strides* sQ, const fa_strides* sKV,
                                     const fa_strides* sO, void* stream) {
    const fa::DecodePaging pg{blockTable, tableStride, numPages, pageSize, maxPagesPerSeq};
    return fa::mla_run({.Q = Q, .KV = KVpool, .O = O, .LSE = LSE, .kv_lens = kvLens, .workspace = workspace, .B = batchSize, .H = numHeads,
                        .Sq = seqLenQ, .d_latent = dLatent, .d_rope = dRope, .scale = scale, .is_causal = is_causal, .dtype = dtype,
                        .o_dtype = o_dtype, .num_splits = numSplits, .sQ = sQ, .sKV = sKV, .sO = sO, .paging = &pg, .stream = stream});
}

const char* flash_attention_error_string(int code) {
    switch (code) {
        case FA_OK: return "success";
        case FA_ERR_NULL_POINTER: return "null pointer argument";
        case FA_ERR_MISALIGNED: return "base pointer not 16-byte aligned";
        case FA_ERR_BAD_SHAPE: return "batchSize/numHeads/seqLen/dHead out of range";
        case FA_ERR_UNSUPPORTED_DHEAD: return "unsupported dHead for this dtype";
        case FA_ERR_UNSUPPORTED_DTYPE: return "unsupported dtype / o_dtype";
        case FA_ERR_BAD_SCALE: return "scale is not finite (fp8 inputs: not positive)";
        case FA_ERR_BAD_FLAGS: return "unknown or contradictory flags, or a flag that does not apply to this dtype / dHead";
        case FA_ERR_BAD_STRIDE: return "bad or misaligned stride";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown flash_attention error";
    }
}

const char* flash_attention_version(void) { return "fa-mi355x 0.1 (gfx950)"; }

}  // extern "C"
