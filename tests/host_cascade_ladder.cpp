// tests/host_cascade_ladder.cpp -- the HOST code of the shared-prefix decode entry points (flash_attention_cascade_decode,
// flash_attention_cascade_decode_paged, flash_attention_cascade_plan) walked by a stand-alone program: every rung of the validation
// ladder of the _window twin of each, once through the twin and once through the cascade call -- the two must return the same code, the
// one written here -- then the rungs the cascade calls add, at their places, and the plan.  Aligned HOST pointers and no call that is
// valid as a whole (the workspace is NULL), so nothing is launched and no GPU is needed.  `make asan-host` builds it with
// -fsanitize=address,undefined against the library whose host code is built the same way, and runs it next to host_ladder.
// usage: host_cascade_ladder          exit status 0 = every call returned what is written here
#include "host_ladder.h"

struct Call {   // valid but for the workspace: stops at FA_ERR_NULL_POINTER, the last rung
    const void *Q = buffer, *Ks = buffer, *Vs = buffer, *K = buffer, *V = buffer;
    void* O = buffer;
    float* LSE = nullptr;
    const int32_t *sl = nullptr, *lens = nullptr, *stable = (const int32_t*)buffer, *table = (const int32_t*)buffer;
    const float *kd = nullptr, *vd = nullptr, *sinks = nullptr;
    void* ws = nullptr;
    int B = 2, H = 8, Hkv = 2, Sq = 4, Ls = 2048, Sk = 1024, P = 64, page = 64, maxsp = 32, maxp = 16, d = 64;
    int64_t ts = 16;
    float scale = 0.125f;
    int dtype = FA_DTYPE_BF16, kv = FA_DTYPE_BF16, o = FA_DTYPE_F32, nss = 0, ns = 2;
    const fa_strides *sQ = nullptr, *sKs = nullptr, *sVs = nullptr, *sK = nullptr, *sV = nullptr, *sO = nullptr;

    // form 0, 1: contiguous, paged
    int twin(int form) const {
        return form == 0 ? flash_attention_decode_window(Q, K, V, O, LSE, lens, kd, vd, ws, B, H, Hkv, Sq, Sk, d, scale, true, dtype, kv, o, ns, 0,
                                                         sQ, sK, sV, sO, nullptr)
                         : flash_attention_decode_paged_window(Q, K, V, O, LSE, lens, table, kd, vd, ws, B, H, Hkv, Sq, P, page, maxp, ts, d, scale,
                                                               true, dtype, kv, o, ns, 0, sQ, sK, sV, sO, nullptr);
    }
    int cascade(int form) const {
        return form == 0 ? flash_attention_cascade_decode(Q, Ks, Vs, K, V, O, LSE, sl, lens, kd, vd, sinks, ws, B, H, Hkv, Sq, Ls, Sk, d, scale, true,
                                                          dtype, kv, o, nss, ns, sQ, sKs, sVs, sK, sV, sO, nullptr)
                         : flash_attention_cascade_decode_paged(Q, K, V, O, LSE, sl, lens, stable, table, kd, vd, sinks, ws, B, H, Hkv, Sq, P, page,
                                                                maxsp, maxp, ts, d, scale, true, dtype, kv, o, nss, ns, sQ, sK, sV, sO, nullptr);
    }
};

static const char* const FORM[2] = {"cascade_decode", "cascade_decode_paged"};
enum { ALL = 3, CONTIGUOUS = 1, PAGED = 2 };

static std::array<Got, 2> both(const Call& c, int form) { return {{{"twin", c.twin(form)}, {"cascade", c.cascade(form)}}}; }
static std::array<Got, 1> mine(const Call& c, int form) { return {{{"cascade", c.cascade(form)}}}; }
#define RUNG(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, both, want, mask, __LINE__)
#define MINE(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, mine, want, mask, __LINE__)

int main() {
    static const fa_strides low{64, 16, 8}, odd_batch{-7, 64, 512};
    // ---- the twins' ladder, in the order of the checks ----
    RUNG((void)c, FA_ERR_NULL_POINTER, ALL);                                        // the workspace: the last rung
    RUNG(c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);               // a descale with a bf16 cache: the entry point's own check
    RUNG(c.kd = (const float*)buffer; c.Q = nullptr, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.V = nullptr; c.O = buffer + 8, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    RUNG(c.O = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.LSE = (float*)(buffer + 4), FA_ERR_MISALIGNED, ALL);
    RUNG(c.ws = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.lens = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    RUNG(c.lens = (const int32_t*)(buffer + 2); c.Sq = 0, FA_ERR_MISALIGNED, ALL);  // the arrays before the shape
    RUNG(c.table = (const int32_t*)(buffer + 1), FA_ERR_MISALIGNED, PAGED);
    RUNG(c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    RUNG(c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 4), FA_ERR_NULL_POINTER, ALL);
    RUNG(c.page = 24; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.ts = 15; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.Sq = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sq = FA_DECODE_MAX_Q + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sq = FA_DECODE_MAX_Q, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.Sk = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, CONTIGUOUS);
    RUNG(c.Hkv = 3; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.ns = FA_DECODE_MAX_SPLITS + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.ns = -1; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                 // the shape before the types
    RUNG(c.dtype = FA_DTYPE_F32, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.o = FA_DTYPE_FP8_E4M3, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);
    RUNG(c.kv = FA_DTYPE_F16; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);             // d before the cache's type
    RUNG(c.kv = FA_DTYPE_F16, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.scale = 0.f, FA_ERR_BAD_SCALE, ALL);
    RUNG(c.scale = -1.f; c.sQ = &low, FA_ERR_BAD_SCALE, ALL);                       // the scale before the strides
    RUNG(c.sQ = &low, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sK = &odd_batch, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sO = &low, FA_ERR_BAD_STRIDE, ALL);

    // ---- the rungs the cascade calls add, at their kind's place ----
    MINE(c.Ks = nullptr, FA_ERR_NULL_POINTER, CONTIGUOUS);                          // with the other pointers
    MINE(c.Vs = nullptr; c.O = buffer + 8; c.Sq = 0, FA_ERR_NULL_POINTER, CONTIGUOUS);
    MINE(c.stable = nullptr; c.ws = buffer; c.page = 24, FA_ERR_NULL_POINTER, PAGED);
    MINE(c.Ks = nullptr; c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, CONTIGUOUS);
    MINE(c.Ks = buffer + 8, FA_ERR_MISALIGNED, CONTIGUOUS);                         // with the other tensors
    MINE(c.sl = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);              // with the int32 / fp32 arrays
    MINE(c.sl = (const int32_t*)(buffer + 2); c.ws = buffer; c.Sq = 0, FA_ERR_MISALIGNED, ALL);
    MINE(c.sl = (const int32_t*)(buffer + 4), FA_ERR_NULL_POINTER, ALL);
    MINE(c.stable = (const int32_t*)(buffer + 3); c.ws = buffer; c.maxsp = 0, FA_ERR_MISALIGNED, PAGED);
    MINE(c.sinks = (const float*)(buffer + 34); c.ws = buffer; c.d = 96, FA_ERR_MISALIGNED, ALL);
    MINE(c.sinks = (const float*)(buffer + 32), FA_ERR_NULL_POINTER, ALL);
    MINE(c.sinks = (const float*)(buffer + 34); c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
    MINE(c.Ls = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, CONTIGUOUS);                    // the shape step
    MINE(c.Ls = (1 << 24) + 1; c.ws = buffer; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, CONTIGUOUS);
    MINE(c.maxsp = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    MINE(c.maxsp = (1 << 18) + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    MINE(c.ns = 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    MINE(c.ns = 1; c.ws = buffer; c.d = 96, FA_ERR_BAD_SHAPE, ALL);
    MINE(c.nss = -1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    MINE(c.nss = 33; c.ns = 32; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    MINE(c.nss = 63; c.ns = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    MINE(c.nss = 0; c.ns = 64; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    MINE(c.nss = 32; c.ns = 32, FA_ERR_NULL_POINTER, ALL);
    MINE(c.nss = 62; c.ns = 0, FA_ERR_NULL_POINTER, ALL);
    MINE(c.B = 20480; c.H = c.Hkv = 256; c.Sq = 2; c.nss = 62; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);   // the shared grid alone
    MINE(c.B = 20480; c.H = c.Hkv = 256; c.Sq = 2; c.nss = 32, FA_ERR_NULL_POINTER, ALL);
    MINE(c.sKs = &low, FA_ERR_BAD_STRIDE, CONTIGUOUS);                              // the shared tensors' strides are checked as K / V's
    MINE(c.sVs = &odd_batch; c.scale = 0.f, FA_ERR_BAD_SCALE, CONTIGUOUS);
    MINE(c.nss = 1; c.ns = 2, FA_ERR_NULL_POINTER, ALL);                            // a workspace whatever the counts

    // ---- the plan ----
    fa_cascade_plan p;
    for (int d : {64, 128})
        for (int B : {1, 3, 32, 300})
            for (int Sq : {1, 5, 16})
                for (int Ls : {1, 384, 8192, 1 << 24})
                    for (int nss : {0, 1, 7})
                        for (int ns : {0, 2, 9}) {
                            EXPECT(flash_attention_cascade_plan(B, 8, 2, Sq, Ls, 256, d, FA_DTYPE_BF16, nss, ns, &p), FA_OK);
                            const int rpb = d == 128 ? 64 : 32;
                            EXPECT(p.num_splits, p.shared.num_splits + p.unique.num_splits);
                            EXPECT(p.unique.num_splits >= 2 && p.shared.num_splits >= 1 && p.num_splits <= FA_DECODE_MAX_SPLITS, 1);
                            if (nss) EXPECT(p.shared.num_splits, nss);
                            if (ns) EXPECT(p.unique.num_splits, ns);
                            EXPECT(p.shared.rows_per_block, rpb);
                            EXPECT(p.shared.row_blocks, (B * 4 * Sq + rpb - 1) / rpb);
                            EXPECT(p.shared.grid, 2 * p.shared.row_blocks * p.shared.num_splits);
                            EXPECT(p.unique.grid, B * 2 * p.unique.row_blocks * p.unique.num_splits);
                            EXPECT(flash_attention_decode_workspace_size(B, 8, Sq, d, p.num_splits) > 0, 1);
                        }
    EXPECT(flash_attention_cascade_plan(2, 8, 2, 4, 384, 256, 128, FA_DTYPE_F32, 0, 0, nullptr), FA_ERR_NULL_POINTER);
    EXPECT(flash_attention_cascade_plan(2, 8, 2, 4, 0, 256, 128, FA_DTYPE_F32, 0, 0, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_cascade_plan(2, 8, 2, 4, 384, 256, 128, FA_DTYPE_F32, 0, 1, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_cascade_plan(2, 8, 2, 4, 384, 256, 128, FA_DTYPE_F32, 40, 30, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_cascade_plan(2, 8, 2, 17, 384, 256, 128, FA_DTYPE_F32, 0, 0, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_cascade_plan(2, 8, 2, 4, 384, 256, 96, FA_DTYPE_F32, 0, 0, &p), FA_ERR_UNSUPPORTED_DHEAD);
    return report("host_cascade_ladder", "all refusals and plans as declared");
}
