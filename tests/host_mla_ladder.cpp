// tests/host_mla_ladder.cpp -- the HOST code of the MLA decode entry points (flash_attention_mla_decode, flash_attention_mla_decode_paged,
// flash_attention_mla_decode_plan, flash_attention_mla_decode_workspace_size) walked by a stand-alone program: every rung of the
// validation ladder of flash_attention_decode / _paged, once through the twin (K = V = the cache, one K/V head, d = 128) and once through
// the MLA call -- the two must return the same code, the one written here -- then the rungs the MLA calls add, at their places, and the
// plan.  Aligned HOST pointers and no call that is valid as a whole (the workspace is NULL under two forced splits), so nothing is
// launched and no GPU is needed.  `make asan-host` builds it with -fsanitize=address,undefined against the library whose host code is
// built the same way, and runs it next to host_ladder.
// usage: host_mla_ladder          exit status 0 = every call returned what is written here
#include "host_ladder.h"

struct Call {   // valid but for the workspace: stops at FA_ERR_NULL_POINTER, the last rung
    const void *Q = buffer, *KV = buffer;
    void* O = buffer;
    float* LSE = nullptr;
    const int32_t *lens = nullptr, *table = (const int32_t*)buffer;
    void* ws = nullptr;
    int B = 2, H = 8, Sq = 4, Sk = 1024, P = 64, page = 64, maxp = 16, d = 128, dl = 512, dr = 64;
    int64_t ts = 16;
    float scale = 0.125f;
    int dtype = FA_DTYPE_BF16, o = FA_DTYPE_F32, ns = 2;
    const fa_strides *sQ = nullptr, *sKV = nullptr, *sO = nullptr;

    // form 0, 1: contiguous, paged
    int twin(int form) const {
        return form == 0 ? flash_attention_decode(Q, KV, KV, O, LSE, lens, ws, B, H, 1, Sq, Sk, d, scale, true, dtype, o, ns, sQ, sKV, sKV, sO, nullptr)
                         : flash_attention_decode_paged(Q, KV, KV, O, LSE, lens, table, ws, B, H, 1, Sq, P, page, maxp, ts, d, scale, true, dtype, o,
                                                        ns, sQ, sKV, sKV, sO, nullptr);
    }
    int mla(int form) const {
        return form == 0 ? flash_attention_mla_decode(Q, KV, O, LSE, lens, ws, B, H, Sq, Sk, dl, dr, scale, true, dtype, o, ns, sQ, sKV, sO, nullptr)
                         : flash_attention_mla_decode_paged(Q, KV, O, LSE, lens, table, ws, B, H, Sq, P, page, maxp, ts, dl, dr, scale, true, dtype,
                                                            o, ns, sQ, sKV, sO, nullptr);
    }
};

static const char* const FORM[2] = {"mla_decode", "mla_decode_paged"};
enum { ALL = 3, CONTIGUOUS = 1, PAGED = 2 };

static std::array<Got, 2> both(const Call& c, int form) { return {{{"twin", c.twin(form)}, {"mla", c.mla(form)}}}; }
static std::array<Got, 1> mine(const Call& c, int form) { return {{{"mla", c.mla(form)}}}; }
#define RUNG(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, both, want, mask, __LINE__)
#define MINE(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, mine, want, mask, __LINE__)

int main() {
    static const fa_strides low{64, 16, 8}, odd_batch{-7, 0, 1024}, odd_head{1 << 20, 7, 576}, wide{0, 0, 1 << 25}, o512{1 << 20, 1 << 12, 512};
    // ---- the twins' ladder, in the order of the checks ----
    RUNG((void)c, FA_ERR_NULL_POINTER, ALL);                                        // the workspace: the last rung
    RUNG(c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.KV = nullptr; c.O = buffer + 8, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    RUNG(c.O = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.KV = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.LSE = (float*)(buffer + 4), FA_ERR_MISALIGNED, ALL);
    RUNG(c.ws = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.lens = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    RUNG(c.lens = (const int32_t*)(buffer + 2); c.Sq = 0, FA_ERR_MISALIGNED, ALL);  // the arrays before the shape
    RUNG(c.lens = (const int32_t*)(buffer + 4), FA_ERR_NULL_POINTER, ALL);
    RUNG(c.table = (const int32_t*)(buffer + 1), FA_ERR_MISALIGNED, PAGED);
    RUNG(c.page = 24; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.page = 8; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.ts = 15; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.P = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.Sq = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sq = FA_DECODE_MAX_Q + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sq = FA_DECODE_MAX_Q, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.Sk = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, CONTIGUOUS);
    RUNG(c.Sk = (1 << 24) + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, CONTIGUOUS);
    RUNG(c.B = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.H = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.ns = FA_DECODE_MAX_SPLITS + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.ns = -1; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                 // the shape before the types
    RUNG(c.dtype = FA_DTYPE_F32, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.o = FA_DTYPE_FP8_E4M3, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.d = 96; c.dl = 256, FA_ERR_UNSUPPORTED_DHEAD, ALL);                      // the widths where dHead stands
    RUNG(c.d = 96; c.dr = 32; c.scale = 0.f, FA_ERR_UNSUPPORTED_DHEAD, ALL);
    RUNG(c.d = 96; c.dl = 128; c.dtype = FA_DTYPE_F32, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.d = 0; c.dl = 0, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.d = -1; c.dr = 0; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.scale = 0.f, FA_ERR_BAD_SCALE, ALL);
    RUNG(c.scale = -1.f; c.sQ = &low, FA_ERR_BAD_SCALE, ALL);                       // the scale before the strides
    RUNG(c.sQ = &low, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sKV = &low, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sKV = &odd_batch, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sO = &low, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sKV = &wide; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);                      // the extent, after the strides
    RUNG(c.ns = 1; c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);

    // ---- the rungs the MLA calls add or move ----
    MINE(c.dl = 576; c.dr = 64, FA_ERR_UNSUPPORTED_DHEAD, ALL);                     // only (512, 64)
    MINE(c.dl = 64; c.dr = 512, FA_ERR_UNSUPPORTED_DHEAD, ALL);
    MINE(c.dl = 512; c.dr = 128; c.ws = buffer, FA_ERR_UNSUPPORTED_DHEAD, ALL);
    MINE(c.dl = 256; c.ns = FA_DECODE_MAX_SPLITS + 1, FA_ERR_BAD_SHAPE, ALL);
    MINE(c.sKV = &odd_head, FA_ERR_NULL_POINTER, ALL);                              // sKV->strideH is not read
    MINE(c.sO = &o512, FA_ERR_NULL_POINTER, ALL);                                   // O's rows are 512 wide ...
    MINE(c.sQ = &o512, FA_ERR_BAD_STRIDE, ALL);                                     // ... Q's 576
    MINE(c.B = 1 << 18; c.H = 1; c.Sq = 1; c.ns = 64; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);   // 2^24 workgroups
    MINE(c.B = 1 << 18; c.H = 1; c.Sq = 1; c.ns = 32, FA_ERR_NULL_POINTER, ALL);
    MINE(c.B = 1 << 20; c.H = 16; c.Sq = 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);             // 2^24 rows of O under two splits

    // ---- the plan and the workspace ----
    fa_decode_plan p;
    for (int B : {1, 3, 32, 300})
        for (int H : {1, 13, 16, 128})
            for (int Sq : {1, 5, 16})
                for (int Sk : {1, 384, 8192, 1 << 24})
                    for (int ns : {0, 1, 7, FA_DECODE_MAX_SPLITS}) {
                        EXPECT(flash_attention_mla_decode_plan(B, H, Sq, Sk, 512, 64, FA_DTYPE_BF16, ns, &p), FA_OK);
                        if (ns) EXPECT(p.num_splits, ns);
                        EXPECT(p.num_splits >= 1 && p.num_splits <= FA_DECODE_MAX_SPLITS, 1);
                        EXPECT(p.rows_per_block, 64);
                        EXPECT(p.row_blocks, (H * Sq + 63) / 64);
                        EXPECT(p.grid, B * p.row_blocks * p.num_splits);
                        EXPECT(p.threads, 256);
                        EXPECT(p.kv_block_rows > 0 && p.kv_block_rows % 16 == 0 && p.lds_bytes > 0 && p.lds_bytes <= 160 * 1024, 1);
                        if (!ns) EXPECT(p.num_splits <= (Sk + p.kv_block_rows - 1) / p.kv_block_rows / 2 || p.num_splits == 1, 1);
                        EXPECT(p.combine_grid, p.num_splits > 1 ? B * H * Sq : 0);
                        EXPECT(flash_attention_mla_decode_workspace_size(B, H, Sq, 512, p.num_splits),
                               flash_attention_decode_workspace_size(B, H, Sq, 512, p.num_splits));
                        EXPECT(flash_attention_mla_decode_workspace_size(B, H, Sq, 512, p.num_splits) > 0, p.num_splits > 1);
                    }
    EXPECT(flash_attention_mla_decode_plan(2, 8, 4, 384, 512, 64, FA_DTYPE_F32, 0, nullptr), FA_ERR_NULL_POINTER);
    EXPECT(flash_attention_mla_decode_plan(2, 8, 4, 0, 512, 64, FA_DTYPE_F32, 0, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_mla_decode_plan(2, 8, 17, 384, 512, 64, FA_DTYPE_F32, 0, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_mla_decode_plan(2, 8, 4, 384, 512, 64, FA_DTYPE_F32, 65, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_mla_decode_plan(2, 8, 4, 384, 512, 64, FA_DTYPE_FP8_E4M3, 0, &p), FA_ERR_UNSUPPORTED_DTYPE);
    EXPECT(flash_attention_mla_decode_plan(2, 8, 4, 384, 256, 64, FA_DTYPE_F32, 0, &p), FA_ERR_UNSUPPORTED_DHEAD);
    EXPECT(flash_attention_mla_decode_plan(2, 8, 4, 384, 512, 32, FA_DTYPE_F32, 0, &p), FA_ERR_UNSUPPORTED_DHEAD);
    return report("host_mla_ladder", "all refusals and plans as declared");
}
