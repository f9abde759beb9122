// split_forms.hip.h -- THE list of the split-KV kernel's instantiations (decode_bf16.hip.h: split_kv_kernel): which combinations of its
// template flags exist, which of them a call launches, and how the host reaches each.  One row of SPLIT_FORMS is one translation unit of
// libflash_attention.so: split_unit.hip compiled with -DFA_SPLIT_UNIT=<the row's name> (the Makefile's SPLIT_UNITS names the same forty-four;
// a name missing there is a link error, one missing here a compile error), holding that form's kernels at D = 64 / 128 and their
// launcher.  FlashAttention.hip (decode_run) fills a SplitArgs, asks split_form_of for the form and calls its SPLIT_LAUNCH[split_unit_of(form)];
// under more than one split, combine_launch (inst_split_combine.hip) after it; cascade_run there launches a shared_* unit, a decode_* unit
// and the combine.  DESIGN.md sections 32 and 34.
#pragma once

#include "decode_bf16.hip.h"
#include "launchers.hip.h"

namespace fa {

// The template flags of one form; RT follows from extend (ExtendCfg<D>::RT, else 1), the parameter type from
// SplitParamsOf<varlen, sink, tree, shared>
struct SplitKind {
    bool extend, varlen, window, paged, kv8, sink, tree, shared;
    constexpr bool operator==(const SplitKind&) const = default;
};

// clang-format off
enum class SplitUnit : int {
    decode_bf16, decode_fp8, decode_paged_bf16, decode_paged_fp8,
    extend_bf16, extend_fp8, extend_paged_bf16, extend_paged_fp8,
    extend_window_bf16, extend_window_fp8, extend_window_paged_bf16, extend_window_paged_fp8,
    extend_varlen_bf16, extend_varlen_fp8, extend_varlen_paged_bf16, extend_varlen_paged_fp8,
    extend_window_varlen_bf16, extend_window_varlen_fp8, extend_window_varlen_paged_bf16, extend_window_varlen_paged_fp8,
    decode_sink_bf16, decode_sink_fp8, decode_sink_paged_bf16, decode_sink_paged_fp8,
    extend_sink_bf16, extend_sink_fp8, extend_sink_paged_bf16, extend_sink_paged_fp8,
    extend_sink_varlen_bf16, extend_sink_varlen_fp8, extend_sink_varlen_paged_bf16, extend_sink_varlen_paged_fp8,
    decode_tree_bf16, decode_tree_fp8, decode_tree_paged_bf16, decode_tree_paged_fp8,
    extend_tree_bf16, extend_tree_fp8, extend_tree_paged_bf16, extend_tree_paged_fp8,
    shared_bf16, shared_fp8, shared_paged_bf16, shared_paged_fp8,
};

// One row per enumerator, in the enumeration's order: {bf16, fp8} x {contiguous, paged} of each family.  No other combination exists.
inline constexpr SplitKind SPLIT_FORMS[] = {
    // decode_*: flash_attention_decode[_paged][_fp8] and decode[_paged]_window; flash_attention_sink_decode* under more than one split.
    // WINDOW = true serves window = 0 too
    {.window = true}, {.window = true, .kv8 = true}, {.window = true, .paged = true}, {.window = true, .paged = true, .kv8 = true},
    // extend_*: flash_attention_extend[_paged], and extend[_paged]_window with windowSize = 0
    {.extend = true}, {.extend = true, .kv8 = true}, {.extend = true, .paged = true}, {.extend = true, .paged = true, .kv8 = true},
    // extend_window_*: flash_attention_extend[_paged]_window with windowSize > 0
    {.extend = true, .window = true}, {.extend = true, .window = true, .kv8 = true},
    {.extend = true, .window = true, .paged = true}, {.extend = true, .window = true, .paged = true, .kv8 = true},
    // extend_varlen_*: flash_attention_extend[_paged]_varlen, and their _window twins with windowSize = 0
    {.extend = true, .varlen = true}, {.extend = true, .varlen = true, .kv8 = true},
    {.extend = true, .varlen = true, .paged = true}, {.extend = true, .varlen = true, .paged = true, .kv8 = true},
    // extend_window_varlen_*: flash_attention_extend[_paged]_varlen_window with windowSize > 0
    {.extend = true, .varlen = true, .window = true}, {.extend = true, .varlen = true, .window = true, .kv8 = true},
    {.extend = true, .varlen = true, .window = true, .paged = true}, {.extend = true, .varlen = true, .window = true, .paged = true, .kv8 = true},
    // (every extend_* row without SINK also serves the flash_attention_sink_extend* call of its shape under more than one split)
    // decode_sink_*: flash_attention_sink_decode[_paged] under ONE split (the kernel that writes O applies the sink); all SINK forms are WINDOW = true
    {.window = true, .sink = true}, {.window = true, .kv8 = true, .sink = true},
    {.window = true, .paged = true, .sink = true}, {.window = true, .paged = true, .kv8 = true, .sink = true},
    // extend_sink_*: flash_attention_sink_extend[_paged] under one split; windowSize = 0 runs at window = 0, as decode does
    {.extend = true, .window = true, .sink = true}, {.extend = true, .window = true, .kv8 = true, .sink = true},
    {.extend = true, .window = true, .paged = true, .sink = true}, {.extend = true, .window = true, .paged = true, .kv8 = true, .sink = true},
    // extend_sink_varlen_*: flash_attention_sink_extend[_paged]_varlen under one split
    {.extend = true, .varlen = true, .window = true, .sink = true}, {.extend = true, .varlen = true, .window = true, .kv8 = true, .sink = true},
    {.extend = true, .varlen = true, .window = true, .paged = true, .sink = true},
    {.extend = true, .varlen = true, .window = true, .paged = true, .kv8 = true, .sink = true},
    // decode_tree_*: flash_attention_tree[_paged] with seqLenQ <= FA_DECODE_MAX_Q, under any split count, sinks or not
    {.window = true, .sink = true, .tree = true}, {.window = true, .kv8 = true, .sink = true, .tree = true},
    {.window = true, .paged = true, .sink = true, .tree = true}, {.window = true, .paged = true, .kv8 = true, .sink = true, .tree = true},
    // extend_tree_*: flash_attention_tree[_paged] with more draft nodes than that
    {.extend = true, .window = true, .sink = true, .tree = true}, {.extend = true, .window = true, .kv8 = true, .sink = true, .tree = true},
    {.extend = true, .window = true, .paged = true, .sink = true, .tree = true},
    {.extend = true, .window = true, .paged = true, .kv8 = true, .sink = true, .tree = true},
    // shared_*: the shared-prefix launch of flash_attention_cascade_decode[_paged]: the chunked-prefill row block (extend = true: RT > 1 and
    // the VGPR-form flag) with the packed rows across the batch and every other flag false
    {.extend = true, .shared = true}, {.extend = true, .kv8 = true, .shared = true},
    {.extend = true, .paged = true, .shared = true}, {.extend = true, .paged = true, .kv8 = true, .shared = true},
};
// clang-format on
constexpr int SPLIT_UNITS = sizeof(SPLIT_FORMS) / sizeof(SPLIT_FORMS[0]);
static_assert(SPLIT_UNITS == (int)SplitUnit::shared_paged_fp8 + 1, "one row per enumerator");

// The form a call launches.  windowed: windowSize > 0; sink_in_split: the call has sinks and runs under ONE split (under more the split
// kernel is the call's own without sinks -- the slabs hold the keys alone -- and the SINK combine adds the sink); tree: the call has a
// tree mask, and launches a TREE form (which takes the sinks pointer, NULL or not) whatever the split count; shared: the shared-prefix
// launch of a cascade call, which is none of the others (its sinks are the combine's, under any split count)
constexpr SplitKind split_form_of(bool extend, bool varlen, bool windowed, bool paged, bool kv8, bool sink_in_split, bool tree,
                                  bool shared = false) {
    if (shared) return {.extend = true, .paged = paged, .kv8 = kv8, .shared = true};
    const bool sink = sink_in_split || tree;
    return {extend, varlen, !extend || windowed || sink, paged, kv8, sink, tree};
}

// the row of a form, or -1
constexpr int split_unit_of(const SplitKind& k) {
    for (int u = 0; u < SPLIT_UNITS; ++u)
        if (SPLIT_FORMS[u] == k) return u;
    return -1;
}

// Checked at every build, over everything a call can ask for (varlen only with extend; a tree call is never ragged; a shared launch is
// only ever contiguous or paged, bf16 or fp8): the number of calls whose form has no row or is not what the call asked for, and the
// number of rows no call selects
constexpr int split_calls_without_row() {
    int bad = 0;
    for (int i = 0; i < 256; ++i) {
        const bool extend = i & 1, varlen = i & 2, windowed = i & 4, paged = i & 8, kv8 = i & 16, sink_in_split = i & 32, tree = i & 64;
        const bool shared = i & 128;
        if ((varlen && !extend) || (tree && varlen) || (shared && (extend || varlen || windowed || sink_in_split || tree))) continue;
        const SplitKind k = split_form_of(extend, varlen, windowed, paged, kv8, sink_in_split, tree, shared);
        const bool passed = k.extend == (extend || shared) && k.varlen == varlen && k.paged == paged && k.kv8 == kv8 && k.tree == tree
                            && k.shared == shared;
        bad += !(split_unit_of(k) >= 0 && passed && k.sink == (sink_in_split || tree)
                 && k.window == (!shared && (!extend || windowed || k.sink)));
    }
    return bad;
}
constexpr int split_rows_without_call() {
    int dead = 0;
    for (int u = 0; u < SPLIT_UNITS; ++u) {   // (a row is selected by the call that asks for exactly it, or by none; a second copy of a row never is)
        const SplitKind& k = SPLIT_FORMS[u];
        dead += !(k.varlen <= k.extend && !(k.tree && k.varlen) && !(k.shared && (k.varlen || k.window || k.sink || k.tree))
                  && split_unit_of(split_form_of(k.extend && !k.shared, k.varlen, k.window, k.paged, k.kv8, k.sink && !k.tree, k.tree,
                                                 k.shared)) == u);
    }
    return dead;
}
static_assert(split_calls_without_row() == 0, "split_form_of selects a form that SPLIT_FORMS lacks, or not the form of the call");
static_assert(split_rows_without_call() == 0, "SPLIT_FORMS has a row that no call selects: a unit built for nothing");

// Everything any form's kernel takes; each launcher copies out the members its own parameter type has
struct SplitArgs : SinkVarlenDecodeParams {
    const uint64_t* tree_mask;
};

// Unit U's launcher: SPLIT_FORMS[U]'s kernel at D = d (128, else 64) with that form's exact parameter type.  Declared only: each unit
// (split_unit.hip) defines the one specialisation that is its own, so no translation unit can instantiate another unit's kernels, and
// FlashAttention.hip alone takes the forty-four addresses (SPLIT_LAUNCH there)
template <SplitUnit U>
int split_unit_launch(int d, unsigned grid, hipStream_t st, const SplitArgs& a);

// A form's parameter type from the arguments: the DecodeParams base, then only the members the type has
template <class P>
P split_params(const SplitArgs& a) {
    P p;
    static_cast<DecodeParams&>(p) = a;
    if constexpr (requires { p.cu_q; }) { p.cu_q = a.cu_q; p.B = a.B; }
    else if constexpr (requires { p.B; }) p.B = a.B;
    if constexpr (requires { p.sinks; }) p.sinks = a.sinks;
    if constexpr (requires { p.tree_mask; }) p.tree_mask = a.tree_mask;
    return p;
}

// The combine kernel of a call under more than one split (inst_split_combine.hip): one workgroup per row of O
int combine_launch(bool varlen, bool sink, int d, unsigned rows, hipStream_t st, const SplitArgs& a);

}  // namespace fa
