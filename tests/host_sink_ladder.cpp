// tests/host_sink_ladder.cpp -- the HOST code of the six attention-sink entry points (flash_attention_sink_decode, _decode_paged, _extend,
// _extend_paged, _extend_varlen, _extend_paged_varlen) walked by a stand-alone program: every rung of the validation ladder of the _window
// twin of each, once through the twin, once through the sink entry point with sinks = NULL and once with a valid sinks pointer -- the
// three must return the same code, the one written here -- and the place of the one rung the sink entry points add, a sinks pointer
// that is not 4-byte aligned.  Aligned HOST pointers and no call that is valid as a whole (the workspace of its two splits is NULL), so
// nothing is launched and no GPU is needed.  `make asan-host` builds it with -fsanitize=address,undefined against the library whose
// host code is built the same way, and runs it next to host_ladder.
// usage: host_sink_ladder          exit status 0 = every call returned what is written here
#include "host_ladder.h"

struct Call {   // valid but for the workspace of its two splits: stops at FA_ERR_NULL_POINTER, the last rung
    const void *Q = buffer, *K = buffer, *V = buffer;
    void* O = buffer;
    float* LSE = nullptr;
    const int32_t *cu = (const int32_t*)buffer, *lens = nullptr, *table = (const int32_t*)buffer;
    const float *kd = nullptr, *vd = nullptr, *sinks = nullptr;
    void* ws = nullptr;
    int B = 2, H = 8, Hkv = 2, Sq = 4, Sk = 1024, P = 64, page = 64, maxp = 16, d = 64;
    int64_t ts = 16;
    float scale = 0.125f;
    int dtype = FA_DTYPE_BF16, kv = FA_DTYPE_BF16, o = FA_DTYPE_F32, ns = 2, W = 128;
    const fa_strides *sQ = nullptr, *sK = nullptr, *sV = nullptr, *sO = nullptr;

    // form 0 .. 5: decode, decode_paged, extend, extend_paged, extend_varlen, extend_paged_varlen
    int twin(int form) const {
        switch (form) {
            case 0: return flash_attention_decode_window(Q, K, V, O, LSE, lens, kd, vd, ws, B, H, Hkv, Sq, Sk, d, scale, true, dtype, kv, o, ns, W,
                                                         sQ, sK, sV, sO, nullptr);
            case 1: return flash_attention_decode_paged_window(Q, K, V, O, LSE, lens, table, kd, vd, ws, B, H, Hkv, Sq, P, page, maxp, ts, d, scale,
                                                               true, dtype, kv, o, ns, W, sQ, sK, sV, sO, nullptr);
            case 2: return flash_attention_extend_window(Q, K, V, O, LSE, lens, kd, vd, ws, B, H, Hkv, Sq, Sk, d, scale, true, dtype, kv, o, ns, W,
                                                         sQ, sK, sV, sO, nullptr);
            case 3: return flash_attention_extend_paged_window(Q, K, V, O, LSE, lens, table, kd, vd, ws, B, H, Hkv, Sq, P, page, maxp, ts, d, scale,
                                                               true, dtype, kv, o, ns, W, sQ, sK, sV, sO, nullptr);
            case 4: return flash_attention_extend_varlen_window(Q, K, V, O, LSE, cu, lens, kd, vd, ws, B, H, Hkv, Sq, Sk, d, scale, true, dtype, kv,
                                                                o, ns, W, sQ, sK, sV, sO, nullptr);
            default: return flash_attention_extend_paged_varlen_window(Q, K, V, O, LSE, cu, lens, table, kd, vd, ws, B, H, Hkv, Sq, P, page, maxp,
                                                                       ts, d, scale, true, dtype, kv, o, ns, W, sQ, sK, sV, sO, nullptr);
        }
    }
    int sink(int form, const float* s) const {
        switch (form) {
            case 0: return flash_attention_sink_decode(Q, K, V, O, LSE, lens, kd, vd, s, ws, B, H, Hkv, Sq, Sk, d, scale, true, dtype, kv, o, ns, W,
                                                       sQ, sK, sV, sO, nullptr);
            case 1: return flash_attention_sink_decode_paged(Q, K, V, O, LSE, lens, table, kd, vd, s, ws, B, H, Hkv, Sq, P, page, maxp, ts, d, scale,
                                                             true, dtype, kv, o, ns, W, sQ, sK, sV, sO, nullptr);
            case 2: return flash_attention_sink_extend(Q, K, V, O, LSE, lens, kd, vd, s, ws, B, H, Hkv, Sq, Sk, d, scale, true, dtype, kv, o, ns, W,
                                                       sQ, sK, sV, sO, nullptr);
            case 3: return flash_attention_sink_extend_paged(Q, K, V, O, LSE, lens, table, kd, vd, s, ws, B, H, Hkv, Sq, P, page, maxp, ts, d, scale,
                                                             true, dtype, kv, o, ns, W, sQ, sK, sV, sO, nullptr);
            case 4: return flash_attention_sink_extend_varlen(Q, K, V, O, LSE, cu, lens, kd, vd, s, ws, B, H, Hkv, Sq, Sk, d, scale, true, dtype, kv,
                                                              o, ns, W, sQ, sK, sV, sO, nullptr);
            default: return flash_attention_sink_extend_paged_varlen(Q, K, V, O, LSE, cu, lens, table, kd, vd, s, ws, B, H, Hkv, Sq, P, page, maxp,
                                                                     ts, d, scale, true, dtype, kv, o, ns, W, sQ, sK, sV, sO, nullptr);
        }
    }
};

static const char* const FORM[6] = {"decode", "decode_paged", "extend", "extend_paged", "extend_varlen", "extend_paged_varlen"};
enum { ALL = 0x3F, PAGED = 0x2A, CONTIGUOUS = 0x15, RAGGED = 0x30, DECODE = 0x03 };

// one rung on the forms of `mask`: the twin, the sink call without sinks and the sink call with sinks all return `want`
static std::array<Got, 3> three(const Call& c, int form) {
    return {{{"twin", c.twin(form)}, {"sinks = NULL", c.sink(form, nullptr)}, {"with sinks", c.sink(form, (const float*)(buffer + 32))}}};
}
#define RUNG(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, three, want, mask, __LINE__)

// a sinks pointer at 2 mod 4 beside another fault: the code of whichever is checked first
static std::array<Got, 1> misaligned_sinks(const Call& c, int form) {
    return {{{"misaligned sinks", c.sink(form, (const float*)(buffer + 34))}}};
}
#define MISALIGNED(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, misaligned_sinks, want, mask, __LINE__)

int main() {
    static const fa_strides low{64, 16, 8}, odd_batch{-7, 64, 512};
    // ---- the twins' ladder, in the order of the checks ----
    RUNG((void)c, FA_ERR_NULL_POINTER, ALL);                                        // the workspace of two splits: the last rung
    RUNG(c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);               // a descale with a bf16 cache: the entry point's own check
    RUNG(c.kd = (const float*)buffer; c.Q = nullptr, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.V = nullptr; c.O = buffer + 8, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    RUNG(c.cu = nullptr, FA_ERR_NULL_POINTER, RAGGED);
    RUNG(c.O = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.LSE = (float*)(buffer + 4), FA_ERR_MISALIGNED, ALL);
    RUNG(c.ws = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.lens = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    RUNG(c.lens = (const int32_t*)(buffer + 2); c.Sq = 0, FA_ERR_MISALIGNED, ALL);  // the arrays before the shape
    RUNG(c.cu = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, RAGGED);
    RUNG(c.table = (const int32_t*)(buffer + 1), FA_ERR_MISALIGNED, PAGED);
    RUNG(c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    RUNG(c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 4), FA_ERR_NULL_POINTER, ALL);
    RUNG(c.page = 24; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.ts = 15; c.ws = buffer, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.Sq = 0; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sq = FA_DECODE_MAX_Q + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, DECODE);
    RUNG(c.Sq = FA_DECODE_MAX_Q + 1, FA_ERR_NULL_POINTER, ALL & ~DECODE);
    RUNG(c.Sq = 1025; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL & ~RAGGED);               // above the capacity
    RUNG(c.Sq = 1025, FA_ERR_NULL_POINTER, RAGGED);                                 // ... totalQ is not capped at it
    RUNG(c.B = FA_VARLEN_MAX_BATCH + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, RAGGED);
    RUNG(c.Hkv = 3; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.ns = FA_DECODE_MAX_SPLITS + 1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.W = -1; c.ws = buffer, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.W = 0, FA_ERR_NULL_POINTER, ALL);                                        // no window: accepted
    RUNG(c.W = -1; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                  // the shape before the types
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
    RUNG(c.ns = 1; c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.ns = 0; c.W = 0; c.Sk = 32768; c.maxp = 512; c.ts = 512, FA_ERR_NULL_POINTER, ALL);   // the library's own split count: a workspace

    // ---- the one rung more: sinks not aligned to 4 bytes, directly after the int32 / fp32 arrays of the cache ----
    MISALIGNED((void)c, FA_ERR_MISALIGNED, ALL);
    MISALIGNED(c.ws = buffer, FA_ERR_MISALIGNED, ALL);                               // (otherwise valid as a whole: still refused)
    MISALIGNED(c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);          // after the entry point's own check,
    MISALIGNED(c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);                             // ... the NULL checks
    MISALIGNED(c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    MISALIGNED(c.cu = nullptr, FA_ERR_NULL_POINTER, RAGGED);
    MISALIGNED(c.page = 24; c.ws = buffer, FA_ERR_MISALIGNED, PAGED);                // before the paging geometry,
    MISALIGNED(c.Sq = 0; c.ws = buffer, FA_ERR_MISALIGNED, ALL);                     // ... the shape,
    MISALIGNED(c.dtype = FA_DTYPE_F32, FA_ERR_MISALIGNED, ALL);                      // ... the types,
    MISALIGNED(c.d = 96, FA_ERR_MISALIGNED, ALL);
    MISALIGNED(c.scale = 0.f, FA_ERR_MISALIGNED, ALL);                               // ... the scale
    MISALIGNED(c.sQ = &low, FA_ERR_MISALIGNED, ALL);                                 // ... and the strides
    {   // every residue but 0 is refused
        Call c;
        for (int form = 0; form < 6; ++form)
            for (int r = 0; r < 8; ++r) {
                const int got = c.sink(form, (const float*)(buffer + 32 + r)), want = r % 4 ? FA_ERR_MISALIGNED : FA_ERR_NULL_POINTER;
                if (got != want) {
                    std::printf("%s, sinks at %d mod 8: %d, expected %d\n", FORM[form], r, got, want);
                    ++failures;
                }
            }
    }
    return report("host_sink_ladder", "all refusals as declared");
}
