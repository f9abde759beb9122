// tests/host_rope_ladder.cpp -- the HOST code of the four fused rotary-embedding + append entry points (flash_attention_rope_append,
// _paged, _varlen, _paged_varlen) walked by a stand-alone program: every rung of the validation ladder of the flash_attention_kv_append*
// twin of each, once through the twin and once through the rope entry point -- the two must return the same code, the one written
// here -- and the rungs the rope entry points add, each at its place among the twin's.  Aligned HOST pointers, and every call wrong in
// at least one way (a call that is valid as a whole would launch), so nothing is launched and no GPU is needed.  `make asan-host` builds
// it with -fsanitize=address,undefined against the library whose host code is built the same way, and runs it next to host_ladder.
// usage: host_rope_ladder          exit status 0 = every call returned what is written here
#include "host_ladder.h"

struct Call {   // valid as a whole: every use below breaks it
    const void *Q = buffer, *Kn = buffer, *Vn = buffer;
    void *Qo = buffer, *K = buffer, *V = buffer;
    const float* cs = (const float*)buffer;
    const int32_t *cu = (const int32_t*)buffer, *lens = nullptr, *table = (const int32_t*)buffer;
    const float *kd = nullptr, *vd = nullptr;
    int B = 2, H = 8, Hkv = 2, Sq = 4, Sk = 1024, P = 64, page = 64, maxp = 16, d = 64, rot = 32, maxpos = 1024, il = 0;
    int64_t ts = 16;
    int dtype = FA_DTYPE_BF16, kv = FA_DTYPE_BF16;
    const fa_strides *sQ = nullptr, *sKn = nullptr, *sVn = nullptr, *sQo = nullptr, *sK = nullptr, *sV = nullptr;

    // form 0 .. 3: contiguous, paged, ragged, ragged paged
    int twin(int form) const {
        switch (form) {
            case 0: return flash_attention_kv_append(Kn, Vn, K, V, lens, kd, vd, B, Hkv, Sq, Sk, d, dtype, kv, sKn, sVn, sK, sV, nullptr);
            case 1: return flash_attention_kv_append_paged(Kn, Vn, K, V, lens, table, kd, vd, B, Hkv, Sq, P, page, maxp, ts, d, dtype, kv, sKn, sVn,
                                                           sK, sV, nullptr);
            case 2: return flash_attention_kv_append_varlen(Kn, Vn, K, V, cu, lens, kd, vd, B, Hkv, Sq, Sk, d, dtype, kv, sKn, sVn, sK, sV, nullptr);
            default: return flash_attention_kv_append_paged_varlen(Kn, Vn, K, V, cu, lens, table, kd, vd, B, Hkv, Sq, P, page, maxp, ts, d, dtype,
                                                                   kv, sKn, sVn, sK, sV, nullptr);
        }
    }
    int rope(int form) const {
        switch (form) {
            case 0: return flash_attention_rope_append(Q, Kn, Vn, Qo, K, V, cs, lens, kd, vd, B, H, Hkv, Sq, Sk, d, rot, maxpos, il, dtype, kv, sQ,
                                                       sKn, sVn, sQo, sK, sV, nullptr);
            case 1: return flash_attention_rope_append_paged(Q, Kn, Vn, Qo, K, V, cs, lens, table, kd, vd, B, H, Hkv, Sq, P, page, maxp, ts, d, rot,
                                                             maxpos, il, dtype, kv, sQ, sKn, sVn, sQo, sK, sV, nullptr);
            case 2: return flash_attention_rope_append_varlen(Q, Kn, Vn, Qo, K, V, cs, cu, lens, kd, vd, B, H, Hkv, Sq, Sk, d, rot, maxpos, il,
                                                              dtype, kv, sQ, sKn, sVn, sQo, sK, sV, nullptr);
            default: return flash_attention_rope_append_paged_varlen(Q, Kn, Vn, Qo, K, V, cs, cu, lens, table, kd, vd, B, H, Hkv, Sq, P, page, maxp,
                                                                     ts, d, rot, maxpos, il, dtype, kv, sQ, sKn, sVn, sQo, sK, sV, nullptr);
        }
    }
};

static const char* const FORM[4] = {"rope_append", "rope_append_paged", "rope_append_varlen", "rope_append_paged_varlen"};
enum { ALL = 0xF, PAGED = 0xA, CONTIGUOUS = 0x5, RAGGED = 0xC, UNIFORM = 0x3 };

// one rung of the twin's ladder on the forms of `mask`: the twin and the rope call both return `want`
static std::array<Got, 2> twin_and_rope(const Call& c, int form) {
    return {{{"twin", c.twin(form)}, {"rope", c.rope(form)}}};
}
#define RUNG(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, twin_and_rope, want, mask, __LINE__)

// a rung of the rope calls alone
static std::array<Got, 1> rope_alone(const Call& c, int form) {
    return {{{"rope", c.rope(form)}}};
}
#define OWN(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, rope_alone, want, mask, __LINE__)

int main() {
    static const fa_strides low{64, 16, 8}, odd_batch{-7, 64, 512}, odd_row{1 << 20, 1 << 16, 68}, fine{1 << 20, 1 << 12, 80};
    // ---- the twins' ladder, in the order of the checks: both calls, the same code ----
    RUNG(c.Kn = nullptr, FA_ERR_NULL_POINTER, ALL);
    RUNG(c.V = nullptr; c.K = buffer + 8, FA_ERR_NULL_POINTER, ALL);                // NULL before alignment
    RUNG(c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    RUNG(c.cu = nullptr, FA_ERR_NULL_POINTER, RAGGED);
    RUNG(c.Vn = buffer + 8, FA_ERR_MISALIGNED, ALL);
    RUNG(c.K = buffer + 8; c.Sq = 0, FA_ERR_MISALIGNED, ALL);                       // alignment before the shape
    RUNG(c.lens = (const int32_t*)(buffer + 2); c.Sq = 0, FA_ERR_MISALIGNED, ALL);
    RUNG(c.cu = (const int32_t*)(buffer + 2); c.d = 96, FA_ERR_MISALIGNED, RAGGED);
    RUNG(c.table = (const int32_t*)(buffer + 1); c.d = 96, FA_ERR_MISALIGNED, PAGED);
    RUNG(c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    RUNG(c.page = 24, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.ts = 15, FA_ERR_BAD_SHAPE, PAGED);
    RUNG(c.Sq = 0, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sq = 1025; c.maxpos = 2048, FA_ERR_BAD_SHAPE, UNIFORM);                  // above the capacity
    RUNG(c.Sq = 1025; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, RAGGED);                  // ... totalQ is not capped at it
    RUNG(c.B = FA_VARLEN_MAX_BATCH + 1, FA_ERR_BAD_SHAPE, RAGGED);
    RUNG(c.Hkv = 0, FA_ERR_BAD_SHAPE, ALL);
    RUNG(c.Sk = (1 << 24) + 1; c.maxpos = 1 << 25, FA_ERR_BAD_SHAPE, CONTIGUOUS);
    RUNG(c.Sq = 0; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                  // the shape before the types
    RUNG(c.dtype = FA_DTYPE_F32; c.d = 96, FA_ERR_UNSUPPORTED_DTYPE, ALL);          // the types before dHead
    RUNG(c.kv = FA_DTYPE_F16, FA_ERR_UNSUPPORTED_DTYPE, ALL);
    RUNG(c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);               // a descale with a bf16 cache
    RUNG(c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);
    RUNG(c.d = 96; c.sKn = &low, FA_ERR_UNSUPPORTED_DHEAD, ALL);                    // dHead before the strides
    RUNG(c.sKn = &low, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sVn = &odd_row, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sK = &odd_batch, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.sV = &low, FA_ERR_BAD_STRIDE, ALL);
    RUNG(c.Sk = (1 << 24) - 192; c.maxpos = 1 << 24, FA_ERR_BAD_SHAPE, CONTIGUOUS); // one head's extent: 2^31 bytes
    RUNG(c.page = 1 << 24; c.maxp = 1; c.ts = 1; c.maxpos = 1 << 24, FA_ERR_BAD_SHAPE, PAGED);

    // ---- the rungs the rope calls add, each among the twin's of its kind ----
    OWN(c.Q = nullptr, FA_ERR_NULL_POINTER, ALL);
    OWN(c.Qo = nullptr, FA_ERR_NULL_POINTER, ALL);
    OWN(c.cs = nullptr, FA_ERR_NULL_POINTER, ALL);
    OWN(c.cs = nullptr; c.Kn = buffer + 8, FA_ERR_NULL_POINTER, ALL);               // every NULL before any alignment
    OWN(c.Q = buffer + 8, FA_ERR_MISALIGNED, ALL);
    OWN(c.Qo = buffer + 8, FA_ERR_MISALIGNED, ALL);
    OWN(c.cs = (const float*)(buffer + 4), FA_ERR_MISALIGNED, ALL);
    OWN(c.cs = (const float*)(buffer + 8); c.Sq = 0, FA_ERR_MISALIGNED, ALL);       // alignment before the shape
    OWN(c.Q = buffer + 8; c.page = 24, FA_ERR_MISALIGNED, PAGED);                   // ... and the paging geometry
    OWN(c.H = 0, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.H = -2, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.H = 7, FA_ERR_BAD_SHAPE, ALL);                                            // no multiple of numHeadsKV
    OWN(c.H = 3; c.Hkv = 6, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.H = 7; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                    // the heads with the shape, before the types
    OWN(c.H = 7; c.d = 96, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.rot = 0, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.rot = 8, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.rot = 24, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.rot = 80, FA_ERR_BAD_SHAPE, ALL);                                         // above dHead
    OWN(c.rot = -16, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.d = 128; c.rot = 144, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.rot = 24; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);                       // rotDim after dHead
    OWN(c.rot = 24; c.kv = FA_DTYPE_F16, FA_ERR_UNSUPPORTED_DTYPE, ALL);            // ... and the types
    OWN(c.maxpos = 1023, FA_ERR_BAD_SHAPE, ALL);                                    // below the capacity (1024 both ways)
    OWN(c.maxpos = 0, FA_ERR_BAD_SHAPE, ALL);
    OWN(c.maxpos = 1023; c.il = 2, FA_ERR_BAD_SHAPE, ALL);                          // maxPos before the pair style
    OWN(c.il = 2, FA_ERR_BAD_FLAGS, ALL);
    OWN(c.il = -1, FA_ERR_BAD_FLAGS, ALL);
    OWN(c.il = 2; c.sQ = &low, FA_ERR_BAD_FLAGS, ALL);                              // the pair style before the strides
    OWN(c.sQ = &low, FA_ERR_BAD_STRIDE, ALL);
    OWN(c.sQo = &low, FA_ERR_BAD_STRIDE, ALL);
    OWN(c.sQ = &odd_row, FA_ERR_BAD_STRIDE, ALL);
    OWN(c.sQo = &odd_batch, FA_ERR_BAD_STRIDE, UNIFORM);
    OWN(c.sQo = &odd_batch; c.il = 3, FA_ERR_BAD_FLAGS, RAGGED);                    // ragged: strideB is not read
    OWN(c.sQ = &fine; c.sQo = &fine; c.il = 3, FA_ERR_BAD_FLAGS, ALL);              // good strides pass on
    OWN(c.sQ = &low; c.Sk = (1 << 24) - 192; c.maxpos = 1 << 24, FA_ERR_BAD_STRIDE, CONTIGUOUS);   // the strides before the extent
    return report("host_rope_ladder", "all refusals as declared");
}
