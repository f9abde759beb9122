// tests/host_spec_ladder.cpp -- the HOST code of the speculative step's four write-side entry points (flash_attention_rope_append_pos,
// _paged_pos, flash_attention_kv_accept, _paged) walked by a stand-alone program.  The _pos calls: every rung of the rope_append twin's
// ladder once through the twin and once through the _pos call -- the same code, the one written here -- and the two rungs posOffsets
// adds, each at its place.  The accept calls: the rungs they share with flash_attention_kv_append* through both, and their own.  Aligned
// HOST pointers, and every call wrong in at least one way (a call that is valid as a whole would launch), so nothing is launched and
// no GPU is needed.  `make asan-host` builds it with -fsanitize=address,undefined against the library whose host code is built the
// same way, and runs it next to host_rope_ladder.
// usage: host_spec_ladder          exit status 0 = every call returned what is written here
#include "host_ladder.h"

struct Call {   // valid as a whole: every use below breaks it
    const void *Q = buffer, *Kn = buffer, *Vn = buffer;
    void *Qo = buffer, *K = buffer, *V = buffer;
    const float* cs = (const float*)buffer;
    const int32_t *pos = (const int32_t*)buffer, *idx = (const int32_t*)buffer, *nacc = (const int32_t*)buffer;
    const int32_t *lens = nullptr, *table = (const int32_t*)buffer;
    const float *kd = nullptr, *vd = nullptr;
    int B = 2, H = 8, Hkv = 2, Sq = 4, Sk = 1024, P = 64, page = 64, maxp = 16, d = 64, rot = 32, maxpos = 1024, il = 0;
    int64_t ts = 16;
    int dtype = FA_DTYPE_BF16, kv = FA_DTYPE_BF16;
    const fa_strides *sQ = nullptr, *sKn = nullptr, *sVn = nullptr, *sQo = nullptr, *sK = nullptr, *sV = nullptr;

    // form 0, 1: contiguous, paged
    int rope(int form) const {
        return form == 0 ? flash_attention_rope_append(Q, Kn, Vn, Qo, K, V, cs, lens, kd, vd, B, H, Hkv, Sq, Sk, d, rot, maxpos, il, dtype, kv, sQ, sKn,
                                                       sVn, sQo, sK, sV, nullptr)
                         : flash_attention_rope_append_paged(Q, Kn, Vn, Qo, K, V, cs, lens, table, kd, vd, B, H, Hkv, Sq, P, page, maxp, ts, d, rot,
                                                             maxpos, il, dtype, kv, sQ, sKn, sVn, sQo, sK, sV, nullptr);
    }
    int rope_pos(int form) const {
        return form == 0 ? flash_attention_rope_append_pos(Q, Kn, Vn, Qo, K, V, cs, pos, lens, kd, vd, B, H, Hkv, Sq, Sk, d, rot, maxpos, il, dtype, kv,
                                                           sQ, sKn, sVn, sQo, sK, sV, nullptr)
                         : flash_attention_rope_append_paged_pos(Q, Kn, Vn, Qo, K, V, cs, pos, lens, table, kd, vd, B, H, Hkv, Sq, P, page, maxp, ts, d,
                                                                 rot, maxpos, il, dtype, kv, sQ, sKn, sVn, sQo, sK, sV, nullptr);
    }
    int append(int form) const {
        return form == 0 ? flash_attention_kv_append(Kn, Vn, K, V, lens, kd, vd, B, Hkv, Sq, Sk, d, dtype, kv, sKn, sVn, sK, sV, nullptr)
                         : flash_attention_kv_append_paged(Kn, Vn, K, V, lens, table, kd, vd, B, Hkv, Sq, P, page, maxp, ts, d, dtype, kv, sKn, sVn,
                                                           sK, sV, nullptr);
    }
    int accept(int form) const {   // Sq: the draft's nodes
        return form == 0 ? flash_attention_kv_accept(K, V, lens, idx, nacc, B, Hkv, Sq, Sk, d, kv, sK, sV, nullptr)
                         : flash_attention_kv_accept_paged(K, V, lens, table, idx, nacc, B, Hkv, Sq, P, page, maxp, ts, d, kv, sK, sV, nullptr);
    }
};

static const char* const FORM[2] = {"contiguous", "paged"};
enum { ALL = 0x3, PAGED = 0x2, CONTIGUOUS = 0x1 };

static std::array<Got, 2> twin_and_pos(const Call& c, int form) {
    return {{{"rope_append", c.rope(form)}, {"rope_append_pos", c.rope_pos(form)}}};
}
static std::array<Got, 1> pos_alone(const Call& c, int form) {
    return {{{"rope_append_pos", c.rope_pos(form)}}};
}
static std::array<Got, 2> append_and_accept(const Call& c, int form) {
    return {{{"kv_append", c.append(form)}, {"kv_accept", c.accept(form)}}};
}
static std::array<Got, 1> accept_alone(const Call& c, int form) {
    return {{{"kv_accept", c.accept(form)}}};
}
#define ROPE(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, twin_and_pos, want, mask, __LINE__)
#define POS(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, pos_alone, want, mask, __LINE__)
#define BOTH(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, append_and_accept, want, mask, __LINE__)
#define ACCEPT(change, want, mask) rung<Call>(FORM, [](Call& c) { change; }, accept_alone, want, mask, __LINE__)

int main() {
    static const fa_strides low{64, 16, 8}, odd_batch{-7, 64, 512}, odd_row{1 << 20, 1 << 16, 68};
    // ---- the rope twin's ladder, in the order of the checks: the twin and the _pos call, the same code ----
    ROPE(c.Kn = nullptr, FA_ERR_NULL_POINTER, ALL);
    ROPE(c.Q = nullptr; c.K = buffer + 8, FA_ERR_NULL_POINTER, ALL);                // NULL before alignment
    ROPE(c.cs = nullptr, FA_ERR_NULL_POINTER, ALL);
    ROPE(c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    ROPE(c.Vn = buffer + 8, FA_ERR_MISALIGNED, ALL);
    ROPE(c.Qo = buffer + 8; c.Sq = 0, FA_ERR_MISALIGNED, ALL);                      // alignment before the shape
    ROPE(c.lens = (const int32_t*)(buffer + 2); c.Sq = 0, FA_ERR_MISALIGNED, ALL);
    ROPE(c.table = (const int32_t*)(buffer + 1); c.d = 96, FA_ERR_MISALIGNED, PAGED);
    ROPE(c.kv = FA_DTYPE_FP8_E4M3; c.vd = (const float*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    ROPE(c.page = 24, FA_ERR_BAD_SHAPE, PAGED);
    ROPE(c.ts = 15, FA_ERR_BAD_SHAPE, PAGED);
    ROPE(c.Sq = 0, FA_ERR_BAD_SHAPE, ALL);
    ROPE(c.Sq = 1025; c.maxpos = 2048, FA_ERR_BAD_SHAPE, ALL);                      // above the capacity
    ROPE(c.H = 7, FA_ERR_BAD_SHAPE, ALL);
    ROPE(c.H = 7; c.dtype = FA_DTYPE_F32, FA_ERR_BAD_SHAPE, ALL);                   // the shape before the types
    ROPE(c.dtype = FA_DTYPE_F32; c.d = 96, FA_ERR_UNSUPPORTED_DTYPE, ALL);          // the types before dHead
    ROPE(c.kd = (const float*)buffer, FA_ERR_UNSUPPORTED_DTYPE, ALL);               // a descale with a bf16 cache
    ROPE(c.d = 96; c.rot = 24, FA_ERR_UNSUPPORTED_DHEAD, ALL);
    ROPE(c.rot = 24, FA_ERR_BAD_SHAPE, ALL);
    ROPE(c.maxpos = 1023; c.il = 2, FA_ERR_BAD_SHAPE, ALL);
    ROPE(c.il = 2; c.sQ = &low, FA_ERR_BAD_FLAGS, ALL);                             // the pair style before the strides
    ROPE(c.sQ = &low, FA_ERR_BAD_STRIDE, ALL);
    ROPE(c.sVn = &odd_row, FA_ERR_BAD_STRIDE, ALL);
    ROPE(c.sQo = &odd_batch, FA_ERR_BAD_STRIDE, ALL);
    ROPE(c.sK = &odd_batch, FA_ERR_BAD_STRIDE, ALL);
    ROPE(c.Sk = (1 << 24) - 192; c.maxpos = 1 << 24, FA_ERR_BAD_SHAPE, CONTIGUOUS); // one head's extent: 2^31 bytes
    ROPE(c.page = 1 << 24; c.maxp = 1; c.ts = 1; c.maxpos = 1 << 24, FA_ERR_BAD_SHAPE, PAGED);
    // ---- posOffsets: NULL with the other pointers, 4 bytes with the other 4-byte arrays ----
    POS(c.pos = nullptr, FA_ERR_NULL_POINTER, ALL);
    POS(c.pos = nullptr; c.Kn = buffer + 8, FA_ERR_NULL_POINTER, ALL);              // every NULL before any alignment
    POS(c.pos = nullptr; c.lens = (const int32_t*)(buffer + 2), FA_ERR_NULL_POINTER, ALL);
    POS(c.pos = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    POS(c.pos = (const int32_t*)(buffer + 1); c.Sq = 0, FA_ERR_MISALIGNED, ALL);    // before the shape
    POS(c.pos = (const int32_t*)(buffer + 3); c.page = 24, FA_ERR_MISALIGNED, PAGED);   // ... and the paging geometry
    POS(c.pos = (const int32_t*)(buffer + 4); c.Sq = 0, FA_ERR_BAD_SHAPE, ALL);     // 4 bytes are enough
    POS(c.pos = (const int32_t*)(buffer + 12); c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);

    // ---- what the append and accept share, in the append's order: both calls, the same code ----
    BOTH(c.K = nullptr, FA_ERR_NULL_POINTER, ALL);
    BOTH(c.V = nullptr; c.K = buffer + 8, FA_ERR_NULL_POINTER, ALL);
    BOTH(c.table = nullptr, FA_ERR_NULL_POINTER, PAGED);
    BOTH(c.V = buffer + 8; c.Sq = 0, FA_ERR_MISALIGNED, ALL);
    BOTH(c.lens = (const int32_t*)(buffer + 2); c.Sq = 0, FA_ERR_MISALIGNED, ALL);
    BOTH(c.table = (const int32_t*)(buffer + 1); c.d = 96, FA_ERR_MISALIGNED, PAGED);
    BOTH(c.page = 24, FA_ERR_BAD_SHAPE, PAGED);
    BOTH(c.ts = 15, FA_ERR_BAD_SHAPE, PAGED);
    BOTH(c.Sq = 0, FA_ERR_BAD_SHAPE, ALL);
    BOTH(c.Sq = 40; c.Sk = 32; c.page = 16; c.maxp = 2; c.ts = 2, FA_ERR_BAD_SHAPE, ALL);   // above the capacity
    BOTH(c.Hkv = 0, FA_ERR_BAD_SHAPE, ALL);
    BOTH(c.Sk = (1 << 24) + 1, FA_ERR_BAD_SHAPE, CONTIGUOUS);
    BOTH(c.Sq = 0; c.kv = FA_DTYPE_F16, FA_ERR_BAD_SHAPE, ALL);                     // the shape before the types
    BOTH(c.kv = FA_DTYPE_F16; c.d = 96, FA_ERR_UNSUPPORTED_DTYPE, ALL);             // the types before dHead
    BOTH(c.d = 96; c.sK = &low, FA_ERR_UNSUPPORTED_DHEAD, ALL);                     // dHead before the strides
    BOTH(c.sK = &odd_batch, FA_ERR_BAD_STRIDE, ALL);
    BOTH(c.sV = &low, FA_ERR_BAD_STRIDE, ALL);
    BOTH(c.sV = &low; c.Sk = (1 << 24) - 192, FA_ERR_BAD_STRIDE, CONTIGUOUS);       // the strides before the extent
    BOTH(c.Sk = (1 << 24) - 192, FA_ERR_BAD_SHAPE, CONTIGUOUS);
    BOTH(c.page = 1 << 24; c.maxp = 1; c.ts = 1, FA_ERR_BAD_SHAPE, PAGED);
    // ---- accept's own: the two arrays, the draft's cap ----
    ACCEPT(c.idx = nullptr, FA_ERR_NULL_POINTER, ALL);
    ACCEPT(c.nacc = nullptr; c.K = buffer + 8, FA_ERR_NULL_POINTER, ALL);
    ACCEPT(c.idx = (const int32_t*)(buffer + 2), FA_ERR_MISALIGNED, ALL);
    ACCEPT(c.nacc = (const int32_t*)(buffer + 1); c.Sq = 0, FA_ERR_MISALIGNED, ALL);
    ACCEPT(c.idx = (const int32_t*)(buffer + 3); c.page = 24, FA_ERR_MISALIGNED, PAGED);
    ACCEPT(c.nacc = (const int32_t*)(buffer + 8); c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);
    ACCEPT(c.Sq = FA_TREE_MAX_Q + 1, FA_ERR_BAD_SHAPE, ALL);
    ACCEPT(c.Sq = FA_TREE_MAX_Q + 1; c.kv = FA_DTYPE_F16, FA_ERR_BAD_SHAPE, ALL);   // with the shape, before the types
    ACCEPT(c.Sq = FA_TREE_MAX_Q; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);          // the cap itself passes on
    ACCEPT(c.kv = FA_DTYPE_FP8_E4M3; c.d = 96, FA_ERR_UNSUPPORTED_DHEAD, ALL);      // both cache types pass on
    return report("host_spec_ladder", "all refusals as declared");
}
