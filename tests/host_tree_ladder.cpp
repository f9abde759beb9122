// tests/host_tree_ladder.cpp -- the HOST code of the tree-masked verification entry points (flash_attention_tree, flash_attention_tree_paged,
// flash_attention_tree_plan) walked by a stand-alone program: every rung of the validation ladder of the sink twin -- flash_attention_sink_decode*
// up to FA_DECODE_MAX_Q rows, flash_attention_sink_extend* from 17 to FA_TREE_MAX_Q -- once through the twin and once through the tree entry
// point, which must return the same code, the one written here; then the three rungs the tree entry points add, each at its place: a NULL
// treeMask with the other pointers, a treeMask that is not 8-byte aligned directly after the sinks check, seqLenQ > FA_TREE_MAX_Q in the shape
// step; then the plan beside the plan it forwards to.  Aligned HOST pointers and no call that is valid as a whole (the workspace of its two
// splits is NULL), so nothing is launched and no GPU is needed.  `make asan-host` builds it with -fsanitize=address,undefined against the
// library whose host code is built the same way, and runs it next to the other ladders.
// usage: host_tree_ladder          exit status 0 = every call returned what is written here
#include <cstring>

#include "host_ladder.h"

struct Call {   // valid but for the workspace of its two splits: stops at FA_ERR_NULL_POINTER, the last rung
    const void *Q = buffer, *K = buffer, *V = buffer;
    void* O = buffer;
    float* LSE = nullptr;
    const int32_t *lens = nullptr, *table = (const int32_t*)buffer;
    const float *kd = nullptr, *vd = nullptr, *sinks = nullptr;
    const uint64_t* tree = (const uint64_t*)(buffer + 128);
    void* ws = nullptr;
    int B = 2, H = 8, Hkv = 2, Sq = 4, Sk = 1024, P = 64, page = 64, maxp = 16, d = 64;
    int64_t ts = 16;
    float scale = 0.125f;
    int dtype = FA_DTYPE_BF16, kv = FA_DTYPE_BF16, o = FA_DTYPE_F32, ns = 2, W = 128;
    const fa_strides *sQ = nullptr, *sK = nullptr, *sV = nullptr, *sO = nullptr;

    // form 0, 1: contiguous, paged.  The twin of the call's row count, with is_causal = true
    int twin(int form) const {
        const bool decode = Sq <= FA_DECODE_MAX_Q;
        if (form == 0)
            return (decode ? flash_attention_sink_decode : flash_attention_sink_extend)(Q, K, V, O, LSE, lens, kd, vd, sinks, ws, B, H, Hkv, Sq, Sk, d, scale,
                                                                                      true, dtype, kv, o, ns, W, sQ, sK, sV, sO, nullptr);
        return (decode ? flash_attention_sink_decode_paged : flash_attention_sink_extend_paged)(Q, K, V, O, LSE, lens, table, kd, vd, sinks, ws, B, H, Hkv, Sq, P,
                                                                                                page, maxp, ts, d, scale, true, dtype, kv, o, ns, W, sQ, sK,
                                                                                                sV, sO, nullptr);
    }
    int call(int form) const {
        if (form == 0)
            return flash_attention_tree(Q, K, V, O, LSE, lens, kd, vd, sinks, tree, ws, B, H, Hkv, Sq, Sk, d, scale, dtype, kv, o, ns, W, sQ, sK, sV, sO,
                                        nullptr);
        return flash_attention_tree_paged(Q, K, V, O, LSE, lens, table, kd, vd, sinks, tree, ws, B, H, Hkv, Sq, P, page, maxp, ts, d, scale, dtype, kv, o, ns,
                                          W, sQ, sK, sV, sO, nullptr);
    }
};

static const char* const FORM[2] = {"tree", "tree_paged"};
enum { ALL = 0x3, PAGED = 0x2, CONTIGUOUS = 0x1 };

// one rung: the twin and the tree entry point both return `want`
static std::array<Got, 2> both(const Call& c, int form) { return {{{"twin", c.twin(form)}, {"tree", c.call(form)}}}; }
#define RUNG(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, both, want, mask, __LINE__)

// a rung of the tree entry points alone
static std::array<Got, 1> tree_only(const Call& c, int form) { return {{{"tree", c.call(form)}}}; }
#define TREE(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, tree_only, want, mask, __LINE__)

static int plans_equal(int Sq, int ns, int W) {
    fa_decode_plan a, b;
    std::memset(&a, 0xAB, sizeof a);
    std::memset(&b, 0xAB, sizeof b);
    const int ra = flash_attention_tree_plan(2, 8, 2, Sq, 32768, 128, FA_DTYPE_BF16, ns, W, &a);
    const int rb = Sq <= FA_DECODE_MAX_Q ? flash_attention_decode_plan_window(2, 8, 2, Sq, 32768, 128, FA_DTYPE_BF16, ns, W, &b)
                                         : flash_attention_extend_plan_window(2, 8, 2, Sq, 32768, 128, FA_DTYPE_BF16, ns, W, &b);
    return ra == rb && ra == FA_OK && !std::memcmp(&a, &b, sizeof a);
}

int main() {
    static const fa_strides low{64, 16, 8}, odd_batch{-7, 64, 512};
    static const float* const some_sinks = (const float*)(buffer + 64);
    // ---- the sink twins' ladder, in the order of the checks; every rung at a decode row count and at a chunked-prefill one ----
    for (const int rows : {4, 40}) {
        static int Sq;
        Sq = rows;
        RUNG(c.Sq = Sq, FA_ERR_NULL_POINTER, ALL);                                                   // the workspace of two splits: the last rung
        RUNG(c.Sq = Sq; c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);                 // a descale with a bf16 cache: the entry point's own
        RUNG(c.Sq = Sq; c.kd = (const float*)buffer; c.Q = nullptr, FA_ERR_UNSUPPORTED_DTYPE, ALL);
        RUNG(c.Sq = Sq; c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
        RUNG(c.Sq = Sq; c.V = nullptr; c.O = buffer + 8, FA_ERR_NULL_POINTER, ALL);
        RUNG(c.Sq = Sq; c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
        RUNG(c.Sq = Sq; c.O = buffer + 8, FA_ERR_MISALIGNED, ALL);
        RUNG(c.Sq = Sq; c.LSE = (float*)(buffer + 4), FA_ERR_MISALIGNED, ALL);
        RUNG(c.Sq = Sq; c.ws = buffer + 8, FA_ERR_MISALIGNED, ALL);
        RUNG(c.Sq = Sq; c.lens = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
        RUNG(c.lens = (const int32_t*)(buffer + 2); c.Sq = 0, FA_ERR_MISALIGNED, ALL);               // the arrays before the shape
        RUNG(c.Sq = Sq; c.table = (const int32_t*)(buffer + 1), FA_ERR_MISALIGNED, PAGED);
        RUNG(c.Sq = Sq; c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
        RUNG(c.Sq = Sq; c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 4), FA_ERR_NULL_POINTER, ALL);
        RUNG(c.Sq = Sq; c.sinks = (const float*)(buffer + 66), FA_ERR_MISALIGNED, ALL);
        RUNG(c.Sq = Sq; c.sinks = (const float*)(buffer + 64), FA_ERR_NULL_POINTER, ALL);
        RUNG(c.Sq = Sq; c.page = 24; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
        RUNG(c.Sq = Sq; c.ts = 15; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
        RUNG(c.Sq = Sq; c.Hkv = 3; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
        RUNG(c.Sq = Sq; c.ns = FA_DECODE_MAX_SPLITS + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
        RUNG(c.Sq = Sq; c.W = -1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
        RUNG(c.Sq = Sq; c.W = 0, FA_ERR_NULL_POINTER, ALL);                                          // no window: accepted
        RUNG(c.Sq = Sq; c.W = -1; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                    // the shape before the types
        RUNG(c.Sq = Sq; c.dtype = FA_DTYPE_F32, FA_ERR_UNSUPPORTED_DTYPE, ALL);
        RUNG(c.Sq = Sq; c.o = FA_DTYPE_FP8_E4M3, FA_ERR_UNSUPPORTED_DTYPE, ALL);
        RUNG(c.Sq = Sq; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);
        RUNG(c.Sq = Sq; c.kv = FA_DTYPE_F16; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);               // d before the cache's type
        RUNG(c.Sq = Sq; c.kv = FA_DTYPE_F16, FA_ERR_UNSUPPORTED_DTYPE, ALL);
        RUNG(c.Sq = Sq; c.scale = 0.f, FA_ERR_BAD_SCALE, ALL);
        RUNG(c.Sq = Sq; c.scale = -1.f; c.sQ = &low, FA_ERR_BAD_SCALE, ALL);                         // the scale before the strides
        RUNG(c.Sq = Sq; c.sQ = &low, FA_ERR_BAD_STRIDE, ALL);
        RUNG(c.Sq = Sq; c.sK = &odd_batch, FA_ERR_BAD_STRIDE, ALL);
        RUNG(c.Sq = Sq; c.sO = &low, FA_ERR_BAD_STRIDE, ALL);
        RUNG(c.Sq = Sq; c.ns = 1; c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
        RUNG(c.Sq = Sq; c.ns = 0; c.W = 0; c.Sk = 32768; c.maxp = 512; c.ts = 512, FA_ERR_NULL_POINTER, ALL);   // the library's own split count
    }
    RUNG(c.Sq = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sq = FA_DECODE_MAX_Q, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.Sq = FA_DECODE_MAX_Q + 1, FA_ERR_NULL_POINTER, ALL);                                      // the chunked-prefill form takes over
    RUNG(c.Sq = FA_TREE_MAX_Q, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.Sq = 33; c.Sk = 32; c.ws = buffer, FA_ERR_BAD_SHAPE, CONTIGUOUS);                         // above the capacity

    // ---- a NULL treeMask: with the other pointers ----
    TREE(c.tree = nullptr, FA_ERR_NULL_POINTER, ALL);
    TREE(c.tree = nullptr; c.ws = buffer, FA_ERR_NULL_POINTER, ALL);                                 // (otherwise valid as a whole: still refused)
    TREE(c.tree = nullptr; c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);              // after the entry point's own check,
    TREE(c.tree = nullptr; c.O = buffer + 8, FA_ERR_NULL_POINTER, ALL);                              // before the alignment,
    TREE(c.tree = nullptr; c.lens = (const int32_t*)(buffer + 2), FA_ERR_NULL_POINTER, ALL);
    TREE(c.tree = nullptr; c.Sq = 0; c.ws = buffer, FA_ERR_NULL_POINTER, ALL);                       // ... the shape and the rest
    TREE(c.tree = nullptr; c.d = 96; c.ws = buffer, FA_ERR_NULL_POINTER, ALL);
    // ---- a treeMask that is not 8-byte aligned: directly after the sinks check ----
    TREE(c.tree = (const uint64_t*)(buffer + 132), FA_ERR_MISALIGNED, ALL);
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.ws = buffer, FA_ERR_MISALIGNED, ALL);
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);         // after the NULL checks,
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.page = 24; c.ws = buffer, FA_ERR_MISALIGNED, PAGED);   // before the paging geometry,
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.Sq = 0; c.ws = buffer, FA_ERR_MISALIGNED, ALL);        // ... the shape,
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.Sq = FA_TREE_MAX_Q + 1; c.ws = buffer, FA_ERR_MISALIGNED, ALL);
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.dtype = FA_DTYPE_F32, FA_ERR_MISALIGNED, ALL);         // ... the types,
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.d = 96, FA_ERR_MISALIGNED, ALL);
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.scale = 0.f, FA_ERR_MISALIGNED, ALL);                  // ... the scale
    TREE(c.tree = (const uint64_t*)(buffer + 132); c.sQ = &low, FA_ERR_MISALIGNED, ALL);                    // ... and the strides
    {   // every residue but 0 is refused
        Call c;
        for (int form = 0; form < 2; ++form)
            for (int r = 0; r < 16; ++r) {
                c.tree = (const uint64_t*)(buffer + 128 + r);
                const int got = c.call(form), want = r % 8 ? FA_ERR_MISALIGNED : FA_ERR_NULL_POINTER;
                if (got != want) {
                    std::printf("%s, treeMask at %d mod 16: %d, expected %d\n", FORM[form], r, got, want);
                    ++failures;
                }
            }
    }
    // ---- seqLenQ > FA_TREE_MAX_Q: the shape step (the twin of such a row count, chunked prefill, goes on to its workspace) ----
    for (const int rows : {FA_TREE_MAX_Q + 1, 300, 1024}) {
        static int Sq;
        Sq = rows;
        TREE(c.Sq = Sq, FA_ERR_BAD_SHAPE, ALL);
        TREE(c.Sq = Sq; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
        TREE(c.Sq = Sq; c.sinks = some_sinks, FA_ERR_BAD_SHAPE, ALL);
        TREE(c.Sq = Sq; c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);                                    // after the pointers
        TREE(c.Sq = Sq; c.lens = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);              // ... and the arrays,
        TREE(c.Sq = Sq; c.sinks = (const float*)(buffer + 66), FA_ERR_MISALIGNED, ALL);
        TREE(c.Sq = Sq; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                              // before the types,
        TREE(c.Sq = Sq; c.d = 96, FA_ERR_BAD_SHAPE, ALL);
        TREE(c.Sq = Sq; c.scale = 0.f, FA_ERR_BAD_SHAPE, ALL);                                       // ... the scale
        TREE(c.Sq = Sq; c.sQ = &low, FA_ERR_BAD_SHAPE, ALL);                                         // ... and the strides
        Call c;
        c.Sq = Sq;
        EXPECT(c.twin(0), FA_ERR_NULL_POINTER);
        EXPECT(c.twin(1), FA_ERR_NULL_POINTER);
    }

    // ---- the plan: the plan it forwards to on both sides of 16 / 17, its refusals ----
    for (const int Sq : {1, 5, FA_DECODE_MAX_Q, FA_DECODE_MAX_Q + 1, 33, FA_TREE_MAX_Q})
        for (const int ns : {0, 1, 3})
            for (const int W : {0, 130}) EXPECT(plans_equal(Sq, ns, W), 1);
    fa_decode_plan plan;
    EXPECT(flash_attention_tree_plan(2, 8, 2, 4, 384, 128, FA_DTYPE_BF16, 0, 0, nullptr), FA_ERR_NULL_POINTER);
    EXPECT(flash_attention_tree_plan(2, 8, 2, FA_TREE_MAX_Q + 1, 384, 128, FA_DTYPE_BF16, 0, 0, &plan), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_extend_plan_window(2, 8, 2, FA_TREE_MAX_Q + 1, 384, 128, FA_DTYPE_BF16, 0, 0, &plan), FA_OK);
    EXPECT(flash_attention_tree_plan(2, 8, 2, 0, 384, 128, FA_DTYPE_BF16, 0, 0, &plan), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_tree_plan(2, 8, 3, 4, 384, 128, FA_DTYPE_BF16, 0, 0, &plan), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_tree_plan(2, 8, 2, 4, 384, 96, FA_DTYPE_BF16, 0, 0, &plan), FA_ERR_UNSUPPORTED_DHEAD);
    EXPECT(flash_attention_tree_plan(2, 8, 2, 4, 384, 128, FA_DTYPE_BF16, 0, -1, &plan), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_tree_plan(2, 8, 2, 33, 32, 128, FA_DTYPE_BF16, 0, 0, &plan), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_decode_workspace_size(2, 8, 33, 128, 3), (size_t)(2 * 8 * 33 * 3 * 128 * 4 + 2 * 8 * 33 * 3 * 4));
    return report("host_tree_ladder", "all refusals as declared");
}
