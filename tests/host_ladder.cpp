// tests/host_ladder.cpp -- the HOST code of the ragged entry points (flash_attention_extend_varlen, _paged_varlen, _varlen_plan,
// flash_attention_kv_append_varlen, _paged_varlen) walked by a stand-alone program: every rung of the validation ladder with its code,
// the plan at ordinary and at extreme shapes (the 64-bit arithmetic of the row-block bound, the grid and the workspace), with aligned
// HOST pointers and no call that is valid as a whole, so nothing is launched and no GPU is needed.  `make asan` builds it with
// -fsanitize=address,undefined against the library whose host code is built the same way, and runs it.
// usage: host_ladder          exit status 0 = every call returned what is written here
#include <climits>
#include <initializer_list>

#include "host_ladder.h"

struct Extend {   // valid but for the workspace of its two splits: stops at FA_ERR_NULL_POINTER
    const void *Q = buffer, *K = buffer, *V = buffer;
    void* O = buffer;
    float* LSE = nullptr;
    const int32_t *cu = (const int32_t*)buffer, *lens = nullptr, *table = (const int32_t*)buffer;
    const float *kd = nullptr, *vd = nullptr;
    void* ws = nullptr;
    int B = 2, H = 8, Hkv = 2, T = 300, Sk = 1024, P = 64, page = 64, maxp = 16, d = 128;
    int64_t ts = 16;
    float scale = 0.125f;
    int dtype = FA_DTYPE_BF16, kv = FA_DTYPE_BF16, o = FA_DTYPE_F32, ns = 2;
    const fa_strides *sQ = nullptr, *sK = nullptr, *sV = nullptr, *sO = nullptr;
    int contiguous() const {
        return flash_attention_extend_varlen(Q, K, V, O, LSE, cu, lens, kd, vd, ws, B, H, Hkv, T, Sk, d, scale, true, dtype, kv, o, ns, sQ, sK,
                                             sV, sO, nullptr);
    }
    int paged() const {
        return flash_attention_extend_paged_varlen(Q, K, V, O, LSE, cu, lens, table, kd, vd, ws, B, H, Hkv, T, P, page, maxp, ts, d, scale,
                                                   true, dtype, kv, o, ns, sQ, sK, sV, sO, nullptr);
    }
};

struct Append {   // every call made with it is stopped by the argument under test
    const void *Kn = buffer, *Vn = buffer;
    void *K = buffer, *V = buffer;
    const int32_t *cu = (const int32_t*)buffer, *lens = nullptr, *table = (const int32_t*)buffer;
    const float *kd = nullptr, *vd = nullptr;
    int B = 2, Hkv = 2, T = 300, Sk = 1024, P = 64, page = 64, maxp = 16, d = 128;
    int64_t ts = 16;
    int dtype = FA_DTYPE_BF16, kv = FA_DTYPE_BF16;
    const fa_strides *sKn = nullptr, *sVn = nullptr, *sK = nullptr, *sV = nullptr;
    int contiguous() const {
        return flash_attention_kv_append_varlen(Kn, Vn, K, V, cu, lens, kd, vd, B, Hkv, T, Sk, d, dtype, kv, sKn, sVn, sK, sV, nullptr);
    }
    int paged() const {
        return flash_attention_kv_append_paged_varlen(Kn, Vn, K, V, cu, lens, table, kd, vd, B, Hkv, T, P, page, maxp, ts, d, dtype, kv, sKn,
                                                      sVn, sK, sV, nullptr);
    }
};

static const char* const FORM[2] = {"contiguous", "paged"};

template <class C>
static std::array<Got, 1> one(const C& c, int form) {
    return {{{"returned", form ? c.paged() : c.contiguous()}}};
}
#define BOTH(C, change, want) rung<C>(FORM, [](C& c) { change; }, one<C>, want, 3, __LINE__)

int main() {
    // ---- the attention ladder, in the order of the checks ----
    BOTH(Extend, (void)c, FA_ERR_NULL_POINTER);                       // the workspace of two splits
    BOTH(Extend, c.Q = nullptr, FA_ERR_NULL_POINTER);
    BOTH(Extend, c.cu = nullptr, FA_ERR_NULL_POINTER);
    BOTH(Extend, c.O = buffer + 8, FA_ERR_MISALIGNED);
    BOTH(Extend, c.cu = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED);
    BOTH(Extend, c.cu = (const int32_t*)(buffer + 4), FA_ERR_NULL_POINTER);
    BOTH(Extend, c.lens = (const int32_t*)(buffer + 1), FA_ERR_MISALIGNED);
    BOTH(Extend, c.T = 0; c.ws = buffer, FA_ERR_BAD_SHAPE);
    BOTH(Extend, c.B = FA_VARLEN_MAX_BATCH + 1; c.ws = buffer, FA_ERR_BAD_SHAPE);
    BOTH(Extend, c.B = FA_VARLEN_MAX_BATCH, FA_ERR_NULL_POINTER);
    BOTH(Extend, c.T = 100000, FA_ERR_NULL_POINTER);                  // above the capacity: accepted
    BOTH(Extend, c.H = 16; c.Hkv = 16; c.T = 1 << 27; c.ws = buffer, FA_ERR_BAD_SHAPE);            // numHeads * totalQ = 2^31
    BOTH(Extend, c.H = 16; c.Hkv = 16; c.T = (1 << 27) - 1; c.ws = buffer, FA_ERR_BAD_SHAPE);      // ... 2^31 - 16: FA_DECODE_MAX_WORKGROUPS
    BOTH(Extend, c.H = 16; c.Hkv = 16; c.T = 1 << 20; c.ws = buffer, FA_ERR_BAD_SHAPE);            // 2^24 rows of O under two splits
    BOTH(Extend, c.H = 16; c.Hkv = 16; c.T = (1 << 20) - 1, FA_ERR_NULL_POINTER);                  // ... 2^24 - 16
    BOTH(Extend, c.H = 16; c.Hkv = 16; c.T = 1 << 26; c.d = 64; c.ns = 64; c.ws = buffer, FA_ERR_BAD_SHAPE);   // the grid
    BOTH(Extend, c.T = INT_MAX; c.H = 1; c.Hkv = 1; c.B = FA_VARLEN_MAX_BATCH; c.ws = buffer, FA_ERR_BAD_SHAPE);
    BOTH(Extend, c.T = (1 << 24) - 1; c.H = 1; c.Hkv = 1; c.B = FA_VARLEN_MAX_BATCH, FA_ERR_NULL_POINTER);
    BOTH(Extend, c.Hkv = 3; c.ws = buffer, FA_ERR_BAD_SHAPE);
    BOTH(Extend, c.ns = FA_DECODE_MAX_SPLITS + 1; c.ws = buffer, FA_ERR_BAD_SHAPE);
    BOTH(Extend, c.dtype = FA_DTYPE_F32, FA_ERR_UNSUPPORTED_DTYPE);
    BOTH(Extend, c.kv = FA_DTYPE_F16, FA_ERR_UNSUPPORTED_DTYPE);
    BOTH(Extend, c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE);                           // a descale with a bf16 cache
    BOTH(Extend, c.kv = FA_DTYPE_FP8_E4M3; c.kd = (const float*)(buffer + 2), FA_ERR_MISALIGNED);
    BOTH(Extend, c.kv = FA_DTYPE_FP8_E4M3; c.kd = (const float*)(buffer + 4), FA_ERR_NULL_POINTER);
    BOTH(Extend, c.d = 96, FA_ERR_UNSUPPORTED_DHEAD);
    BOTH(Extend, c.scale = 0.f, FA_ERR_BAD_SCALE);
    static const fa_strides low{64, 16, 8}, odd_batch{-7, 64, 512};
    BOTH(Extend, c.d = 64; c.sQ = &low, FA_ERR_BAD_STRIDE);
    BOTH(Extend, c.d = 64; c.sK = &odd_batch, FA_ERR_BAD_STRIDE);
    BOTH(Extend, c.d = 64; c.sQ = &odd_batch; c.sO = &odd_batch, FA_ERR_NULL_POINTER);             // strideB of Q / O is not read
    BOTH(Extend, c.ns = 0; c.T = 17; c.Sk = 32768; c.maxp = 512; c.ts = 512, FA_ERR_NULL_POINTER);  // the library's own split count
    {
        Extend c;
        c.Sk = (1 << 24) + 1; c.ws = buffer;
        EXPECT(c.contiguous(), FA_ERR_BAD_SHAPE);
        c = Extend(); c.table = nullptr;
        EXPECT(c.paged(), FA_ERR_NULL_POINTER);
        c = Extend(); c.page = 24; c.ws = buffer;
        EXPECT(c.paged(), FA_ERR_BAD_SHAPE);
        c = Extend(); c.page = 1 << 16; c.maxp = 1 << 16; c.ts = 1 << 16; c.ws = buffer;           // capacity 2^32: no 32-bit wrap-around
        EXPECT(c.paged(), FA_ERR_BAD_SHAPE);
        c = Extend(); c.ts = 15; c.ws = buffer;
        EXPECT(c.paged(), FA_ERR_BAD_SHAPE);
    }

    // ---- the plan ----
    fa_decode_plan p{}, e{};
    EXPECT(flash_attention_extend_varlen_plan(2, 8, 2, 300, 1024, 128, FA_DTYPE_F32, 0, nullptr), FA_ERR_NULL_POINTER);
    EXPECT(flash_attention_extend_varlen_plan(2, 8, 2, 0, 1024, 128, FA_DTYPE_F32, 0, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_extend_varlen_plan(FA_VARLEN_MAX_BATCH + 1, 8, 2, 300, 1024, 128, FA_DTYPE_F32, 0, &p), FA_ERR_BAD_SHAPE);
    for (int d : {64, 128})
        for (int B : {1, 3, 64, 130, FA_VARLEN_MAX_BATCH})
            for (int T : {1, 17, 575, 4096, 1 << 17})   // (2^20 tokens of 32 heads are 2^25 rows of O: one split only, below)
                for (int ns : {0, 1, 3, FA_DECODE_MAX_SPLITS}) {
                    const int H = 32, Hkv = 8, G = H / Hkv;
                    EXPECT(flash_attention_extend_varlen_plan(B, H, Hkv, T, 32768, d, FA_DTYPE_BF16, ns, &p), FA_OK);
                    EXPECT(flash_attention_extend_plan(1, H, Hkv, 1, 32768, d, FA_DTYPE_BF16, 1, &e), FA_OK);
                    EXPECT(p.rows_per_block, e.rows_per_block);
                    const long long NB = ((long long)G * T + (long long)B * (p.rows_per_block - 1)) / p.rows_per_block;
                    EXPECT(p.row_blocks, NB);
                    EXPECT(p.grid, (long long)Hkv * NB * p.num_splits);
                    EXPECT(p.combine_grid, p.num_splits > 1 ? (long long)H * T : 0);
                    if (ns) EXPECT(p.num_splits, ns);
                    const size_t rows = (size_t)H * T, ns_ = (size_t)p.num_splits;
                    const size_t want = p.num_splits > 1 ? ((rows * ns_ * d * 4 + 15) & ~(size_t)15) + ((rows * ns_ * 4 + 15) & ~(size_t)15) : 0;
                    EXPECT(flash_attention_decode_workspace_size(1, H, T, d, p.num_splits), want);
                }
    EXPECT(flash_attention_extend_varlen_plan(3, 32, 8, 1 << 20, 32768, 128, FA_DTYPE_BF16, 0, &p), FA_OK);
    EXPECT(p.num_splits, 1);
    EXPECT(flash_attention_extend_varlen_plan(3, 32, 8, 1 << 20, 32768, 128, FA_DTYPE_BF16, 3, &p), FA_ERR_BAD_SHAPE);
    // a launch holds fewer than 2^32 threads: the grid under any split count, the rows of O under more than one
    EXPECT(flash_attention_extend_varlen_plan(FA_VARLEN_MAX_BATCH, 1, 1, INT_MAX, 1 << 24, 64, FA_DTYPE_F32, 1, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_extend_varlen_plan(FA_VARLEN_MAX_BATCH, 1, 1, 1 << 28, 1 << 24, 64, FA_DTYPE_F32, 1, &p), FA_OK);
    EXPECT(p.grid < FA_DECODE_MAX_WORKGROUPS, true);
    EXPECT(flash_attention_extend_varlen_plan(FA_VARLEN_MAX_BATCH, 1, 1, 1 << 28, 1 << 24, 64, FA_DTYPE_F32, 2, &p), FA_ERR_BAD_SHAPE);
    EXPECT(flash_attention_extend_varlen_plan(FA_VARLEN_MAX_BATCH, 1, 1, (1 << 24) - 1, 1 << 24, 64, FA_DTYPE_F32, 2, &p), FA_OK);
    EXPECT(flash_attention_extend_varlen_plan(FA_VARLEN_MAX_BATCH, 1, 1, 1 << 24, 1 << 24, 64, FA_DTYPE_F32, 2, &p), FA_ERR_BAD_SHAPE);

    // ---- the append ladder ----
    BOTH(Append, c.Kn = nullptr, FA_ERR_NULL_POINTER);
    BOTH(Append, c.cu = nullptr, FA_ERR_NULL_POINTER);
    BOTH(Append, c.V = buffer + 8, FA_ERR_MISALIGNED);
    BOTH(Append, c.cu = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED);
    BOTH(Append, c.T = 0, FA_ERR_BAD_SHAPE);
    BOTH(Append, c.B = FA_VARLEN_MAX_BATCH + 1, FA_ERR_BAD_SHAPE);
    BOTH(Append, c.dtype = FA_DTYPE_F32, FA_ERR_UNSUPPORTED_DTYPE);
    BOTH(Append, c.kv = FA_DTYPE_F32, FA_ERR_UNSUPPORTED_DTYPE);
    BOTH(Append, c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE);
    BOTH(Append, c.T = 100000; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD);   // above the capacity: past the shape checks
    BOTH(Append, c.T = INT_MAX; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD);
    BOTH(Append, c.d = 64; c.sKn = &low, FA_ERR_BAD_STRIDE);
    BOTH(Append, c.d = 64; c.sV = &odd_batch, FA_ERR_BAD_STRIDE);
    {
        Append c;
        c.table = nullptr;
        EXPECT(c.paged(), FA_ERR_NULL_POINTER);
        c = Append(); c.page = 8;
        EXPECT(c.paged(), FA_ERR_BAD_SHAPE);
        c = Append(); c.Sk = 0;
        EXPECT(c.contiguous(), FA_ERR_BAD_SHAPE);
    }
    return report("host_ladder", "all refusals and plans as declared");
}
