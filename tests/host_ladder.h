// tests/host_ladder.h -- what the stand-alone ladder programs (host_ladder.cpp, host_sink_ladder.cpp, host_rope_ladder.cpp) share: the
// aligned HOST memory every pointer of a call points into, the failure counter, one rung -- a change applied to a fresh call on every
// form of a mask, each return code compared with the one written in the program, a miss reported with its line -- and the closing
// report.  A program keeps its own call struct (default-constructed = the call its rungs start from), its forms and its main().
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>

#include "../include/flash_attention.h"

static int failures = 0;
alignas(16) static char buffer[256];

#define EXPECT(call, want)                                                                   \
    do {                                                                                     \
        const long long got_ = (long long)(call), want_ = (long long)(want);                 \
        if (got_ != want_) {                                                                 \
            std::printf("line %d: %s = %lld, expected %lld\n", __LINE__, #call, got_, want_); \
            ++failures;                                                                      \
        }                                                                                    \
    } while (0)

struct Got {   // one call of a rung: what it was and what it returned
    const char* what;
    int code;
};

// One rung on the forms of `mask` (bit f = form[f]): `change` is applied to a fresh C, and every call `calls(c, f)` then makes -- a
// std::array of Got -- must return `want`
template <class C, int FORMS, class Change, class Calls>
static void rung(const char* const (&form)[FORMS], Change change, Calls calls, int want, int mask, int line) {
    for (int f = 0; f < FORMS; ++f) {
        if (!(mask >> f & 1)) continue;
        C c;
        change(c);
        for (const Got& g : calls(c, f))
            if (g.code != want) {
                std::printf("line %d, %s: %s %d, expected %d\n", line, form[f], g.what, g.code, want);
                ++failures;
            }
    }
}

// the last line of a program and its exit status
static int report(const char* program, const char* all_well) {
    if (failures) std::printf("%s: %d FAILED\n", program, failures);
    else std::printf("%s: %s\n", program, all_well);
    return failures ? 1 : 0;
}
