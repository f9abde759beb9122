// tests/host_mla_prefill_ladder.cpp -- the HOST code of flash_attention_mla_prefill and its plan under `make asan-host`: the rungs shared
// with flash_attention_ex (the twin, at dHead = 128: both must return the code written here), its own rungs, the plan.  Aligned HOST
// pointers and no call that is valid as a whole: nothing is launched.  Exit status 0 = every call returned what is written here
#include "host_ladder.h"

struct Call {   // valid but for Q: every rung below adds its fault IN FRONT of that last one, or removes it
    const void *Q = nullptr, *K = buffer, *V = buffer;
    void* O = buffer;
    float* LSE = nullptr;
    int B = 2, H = 8, Sq = 300, Sk = 300, dqk = 192, dv = 128;
    float scale = 0.07f;
    int o = FA_DTYPE_F32;
    const fa_strides *sQ = nullptr, *sK = nullptr, *sV = nullptr, *sO = nullptr;
    unsigned flags = 0;

    int twin() const { return flash_attention_ex(Q, K, V, O, LSE, B, H, Sq, Sk, dv, scale, true, FA_DTYPE_BF16, o, sQ, sK, sV, sO, flags, nullptr); }
    int mla() const { return flash_attention_mla_prefill(Q, K, V, O, LSE, B, H, Sq, Sk, dqk, dv, scale, true, o, sQ, sK, sV, sO, flags, nullptr); }
};

static const char* const FORM[1] = {"mla_prefill"};
static std::array<Got, 2> both(const Call& c, int) { return {{{"twin", c.twin()}, {"mla", c.mla()}}}; }
static std::array<Got, 1> mine(const Call& c, int) { return {{{"mla", c.mla()}}}; }
#define RUNG(change, want) rung<Call>(FORM, [](Call& c) { change; }, both, want, 1, __LINE__)
#define MINE(change, want) rung<Call>(FORM, [](Call& c) { change; }, mine, want, 1, __LINE__)

int main() {
    static const fa_strides low{0, 0, 64}, wide{0, 0, 1 << 22}, v128{1 << 20, 1 << 12, 128};
    // ---- flash_attention_cross's ladder, in the order of the checks ----
    RUNG((void)c, FA_ERR_NULL_POINTER);
    RUNG(c.Q = buffer + 8, FA_ERR_MISALIGNED);
    RUNG(c.Q = buffer + 8; c.B = 0, FA_ERR_MISALIGNED);                      // alignment before the shape
    RUNG(c.Q = buffer; c.B = 0; c.scale = 1.f / 0.f, FA_ERR_BAD_SHAPE);      // the shape before the scale
    RUNG(c.Q = buffer; c.scale = 1.f / 0.f; c.o = FA_DTYPE_FP8_E4M3, FA_ERR_BAD_SCALE);
    RUNG(c.Q = buffer; c.o = FA_DTYPE_FP8_E4M3; c.flags = 4, FA_ERR_UNSUPPORTED_DTYPE);
    RUNG(c.Q = buffer; c.flags = 4; c.Sk = 0, FA_ERR_BAD_FLAGS);             // the flags before seqLenK
    RUNG(c.Q = buffer; c.Sk = 0; c.LSE = (float*)(buffer + 4), FA_ERR_BAD_SHAPE);
    RUNG(c.Q = buffer; c.LSE = (float*)(buffer + 4); c.sO = &low, FA_ERR_MISALIGNED);
    RUNG(c.Q = buffer; c.sO = &low, FA_ERR_BAD_STRIDE);
    RUNG(c.Q = buffer; c.sV = &wide, FA_ERR_BAD_SHAPE);                      // the extent, after the strides
    // ---- the rungs of its own ----
    MINE(c.Q = buffer; c.dqk = 0; c.o = 9, FA_ERR_BAD_SHAPE);
    MINE(c.Q = buffer; c.dqk = 128, FA_ERR_UNSUPPORTED_DHEAD);               // only (192, 128)
    MINE(c.Q = buffer; c.dv = 192, FA_ERR_UNSUPPORTED_DHEAD);
    MINE(c.Q = buffer; c.flags = FA_FLAG_F16_WEIGHTS, FA_ERR_BAD_FLAGS);     // there is no fp16 form
    MINE(c.Q = buffer; c.sQ = &v128, FA_ERR_BAD_STRIDE);                     // Q's and K's rows are 192 wide ...
    MINE(c.sV = &v128; c.sO = &v128, FA_ERR_NULL_POINTER);                   // ... V's and O's 128
    MINE(c.Q = buffer; c.Sk = 1 << 24, FA_ERR_BAD_SHAPE);                    // one head's K extent
    // ---- the plan ----
    fa_launch_plan p;
    for (int B : {1, 3, 300})
        for (int H : {1, 13, 128})
            for (int Sq : {1, 256, 257, 8192})
                for (int causal : {0, 1})
                    for (unsigned flags : {0u, (unsigned)FA_FLAG_BF16_WEIGHTS}) {
                        EXPECT(flash_attention_mla_prefill_plan(B, H, Sq, 4096, 192, 128, causal, FA_DTYPE_BF16, flags, &p), FA_OK);
                        EXPECT(p.q_block_rows == 256 && p.kernel_id == 4 && p.threads == 256, 1);
                        EXPECT(p.kv_block_rows > 0 && p.lds_bytes > 0 && p.lds_bytes <= 160 * 1024, 1);
                        EXPECT(p.grid, (B * H * ((Sq + 255) / 256) + 7) / 8 * 8);
                    }
    EXPECT(flash_attention_mla_prefill_plan(2, 8, 300, 300, 192, 128, true, FA_DTYPE_F32, 0, nullptr), FA_ERR_NULL_POINTER);
    EXPECT(flash_attention_mla_prefill_plan(2, 8, 300, 300, 128, 128, true, FA_DTYPE_F32, 0, &p), FA_ERR_UNSUPPORTED_DHEAD);
    EXPECT(flash_attention_mla_prefill_plan(2, 8, 300, 300, 192, 128, true, FA_DTYPE_F32, FA_FLAG_F16_WEIGHTS, &p), FA_ERR_BAD_FLAGS);
    return report("host_mla_prefill_ladder", "all refusals and plans as declared");
}
