"""CPU tests of tree-masked verification (flash_attention_tree, flash_attention_tree_paged, flash_attention_tree_plan) at the C ABI, in
the binding and in the tests' own reference (tree_check.py):

* the symbols are exported and declared: the parameter list of flash_attention_sink_decode / _sink_decode_paged without is_causal and
  with ``treeMask`` directly after ``sinks``; the plan's list is flash_attention_decode_plan_window's;
* every refusal of the sink twin -- flash_attention_sink_decode* up to FA_DECODE_MAX_Q rows, flash_attention_sink_extend* from 17 to
  FA_TREE_MAX_Q -- comes back with the twin's code (fake aligned host pointers: no GPU is touched; no call here is valid as a whole), and
  the three refusals the calls add stand at their stated places: a NULL treeMask with the other pointers, a treeMask that is not 8-byte
  aligned directly after the sinks check, seqLenQ > FA_TREE_MAX_Q in the shape step;
* flash_attention_tree_plan equals the plan function it forwards to on both sides of seqLenQ = 16 / 17;
* the Python fronts raise on a tree_mask that is on the CPU, not int64, of the wrong shape, strided or on another device;
* tree_mask_from_parents and tree_depths equal a brute-force ancestor walk;
* tree_check's reference equals the causal reference for chain and all-ones words, and it REFUSES five wrong kernels emulated in
  float64, each on a named row.
"""
import ctypes
import itertools

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

import kv_cache_check as kv  # noqa: E402
import tree_check as tc  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, aligned_host_pointer, declared_parameters, host_call, plan_call)

TWINS = {"flash_attention_tree": ("flash_attention_sink_decode", "flash_attention_sink_extend"),
         "flash_attention_tree_paged": ("flash_attention_sink_decode_paged", "flash_attention_sink_extend_paged")}


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    assert sorted(fa._TREE_SYMBOLS.values()) == sorted(TWINS) and fa.FA_TREE_MAX_Q == 64
    for name, (twin, twin_extend) in TWINS.items():
        assert name in fa.EXPORTS and getattr(L, name) is not None
        want = declared_parameters(twin)
        assert declared_parameters(twin_extend) == want
        types = list(getattr(L, twin).argtypes)
        at = want.index("is_causal")
        del want[at], types[at]
        at = want.index("sinks") + 1
        want.insert(at, "treeMask")
        types.insert(at, ctypes.c_void_p)
        assert declared_parameters(name) == want, name
        assert list(getattr(L, name).argtypes) == types, name
        assert getattr(L, name).restype is ctypes.c_int
    assert "flash_attention_tree_plan" in fa.EXPORTS
    assert declared_parameters("flash_attention_tree_plan") == declared_parameters("flash_attention_decode_plan_window")
    assert list(L.flash_attention_tree_plan.argtypes) == list(L.flash_attention_decode_plan_window.argtypes)
    # the count that tests/test_split_fronts.py pins is untouched
    split = [s for s in fa.EXPORTS if s.startswith(("flash_attention_decode", "flash_attention_extend")) and "plan" not in s
             and "workspace" not in s]
    assert len(split) == 14


def calls(kv):
    """{tree entry point: call(**overrides)} on an aligned host pointer p, and p.  ``twin=True`` calls the sink twin of the call's row
    count on the same arguments.  Every call is valid but for its workspace: two splits and none given, so that passing every other
    check ends at NULL_POINTER.  treeMask sits at p + 128, sinks is NULL unless overridden"""
    host = aligned_host_pointer()
    p = host[1]
    ok = dict(B=2, H=8, Hkv=2, Sq=4, Sk=1024, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=True, dtype=BF16, kv=kv, o=F32, ns=2,
              W=128, sinks=None, tree=p + 128)

    def make(name):
        tree = host_call(name, ok, host)[0]

        def call(twin=False, **kw):
            if not twin:
                return tree(**kw)
            return tree(symbol=TWINS[name][kw.get("Sq", ok["Sq"]) > fa.FA_DECODE_MAX_Q], **kw)

        return call

    return {name: make(name) for name in TWINS}, p


def ladder(p, paged):
    """the arguments the sink twins refuse (and a few they accept up to the workspace check), as keyword overrides; row counts up to
    FA_TREE_MAX_Q only (above: test_the_three_new_refusals)"""
    out = [dict()]
    for name in ("Q", "K", "V", "O"):
        out += [{name: None}, {name: p + 8}]
    out += [dict(LSE=p + 4), dict(ws=p + 8), dict(lens=p + 2), dict(lens=p + 2, Sq=0), dict(Q=None, O=p + 8)]
    out += [dict(ws=p, **kw) for kw in (dict(Sq=0), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0),
                                        dict(Hkv=16), dict(ns=-1), dict(ns=CAP + 1), dict(W=-1))]
    # (a workspace is only ever passed with an argument that is invalid in that form: nothing here may reach a launch)
    out += [dict(Sq=s) for s in (1, 16, 17, 33, 64)]
    out += [dict(Sq=s, ws=p, ns=-1) for s in (16, 17, 64)]
    out += [dict(o=FP8), dict(o=7), dict(dtype=F32), dict(dtype=FP8), dict(dtype=9), dict(kv=F32), dict(kv=F16), dict(kv=-1),
            dict(kv=F16, d=96), dict(dtype=F32, ns=-1), dict(W=0), dict(W=-1, dtype=F32)]
    out += [dict(d=d) for d in (96, 32, 256)]
    out += [dict(scale=s) for s in (0.0, -0.5, float("nan"), float("inf"))]
    out += [dict(kd=p), dict(vd=p + 8), dict(kd=p + 4, vd=p + 12), dict(kd=p + 1), dict(vd=p + 2), dict(kd=p, Q=None)]
    out += [dict(sinks=p + 64), dict(sinks=p + 66), dict(sinks=p + 66, Q=None), dict(sinks=p + 66, ws=p, Sq=0), dict(sinks=p + 64, Sq=40)]
    if paged:
        out += [dict(table=None), dict(table=p + 2)]
        out += [dict(ws=p, **kw) for kw in (dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),
                                            dict(ts=15), dict(ts=-16))]
    else:
        out += [dict(ws=p, **kw) for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1), dict(Sk=32, Sq=33))]
        out += [dict(Sk=1 << 24)]
    return out


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_sink_twins_ladder_with_the_twins_codes(kv):
    """every rung through the twin of the rung's row count and through the tree entry point: one code"""
    fns, p = calls(kv)
    bad = fa.FaStrides(64, 16, 8)            # strideS < d
    mis = fa.FaStrides(1024, 66, 66)         # d = 64: rows that are no multiples of 16 bytes
    for name, call in fns.items():
        assert call() == call(twin=True) == NULL_POINTER, name                         # valid but for the workspace of its two splits
        for kw in ladder(p, "paged" in name):
            want = call(twin=True, **kw)
            assert NULL_POINTER >= want >= BAD_STRIDE, (name, kw, want)
            assert call(**kw) == want, (name, kw, want)
        for i, s, rows in itertools.product(range(4), (bad, mis), (4, 40)):
            st = [None] * 4
            st[i] = ctypes.byref(s)
            assert call(strides=st, d=64, Sq=rows) == call(twin=True, strides=st, d=64, Sq=rows) == BAD_STRIDE, (name, i)
        # a few of the ladder's codes spelled out
        assert call(Q=None) == NULL_POINTER and call(K=p + 8) == MISALIGNED and call(ws=p, ns=CAP + 1) == BAD_SHAPE
        assert call(d=96) == BAD_DHEAD and call(dtype=F32) == BAD_DTYPE and call(scale=0.0) == BAD_SCALE
        assert call(kd=p) == (NULL_POINTER if kv == FP8 else BAD_DTYPE)


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_three_new_refusals_at_their_places(kv):
    fns, p = calls(kv)
    bad = fa.FaStrides(64, 16, 8)
    for name, call in fns.items():
        paged = "paged" in name
        # a NULL treeMask: FA_ERR_NULL_POINTER, with the other pointers -- behind the entry point's own descale check, ahead of the alignment
        assert call(tree=None) == NULL_POINTER and call(tree=None, ws=p) == NULL_POINTER, name
        assert call(tree=None, K=p + 8) == NULL_POINTER and call(tree=None, lens=p + 2) == NULL_POINTER, name
        assert call(tree=None, ws=p, Sq=0) == NULL_POINTER and call(tree=None, ws=p, d=96) == NULL_POINTER, name
        if kv == BF16:
            assert call(tree=None, kd=p) == BAD_DTYPE, name
        # not 8-byte aligned: FA_ERR_MISALIGNED, directly after the sinks check
        for r in range(1, 16):
            assert call(tree=p + 128 + r) == (MISALIGNED if r % 8 else NULL_POINTER), (name, r)
        t = p + 132
        assert call(tree=t, ws=p) == MISALIGNED, name                                   # (otherwise valid as a whole: still refused)
        assert call(tree=t, Q=None) == NULL_POINTER and call(tree=t, V=None) == NULL_POINTER, name           # behind the NULL checks ...
        if paged:
            assert call(tree=t, table=None) == NULL_POINTER, name
        if kv == BF16:
            assert call(tree=t, kd=p) == BAD_DTYPE, name
        for kw in (dict(Sq=0), dict(Sq=65), dict(B=0), dict(Hkv=3), dict(ns=-1), dict(W=-1), dict(dtype=F32), dict(o=7), dict(d=96),
                   dict(scale=0.0), dict(strides=[ctypes.byref(bad), None, None, None], d=64)):                # ... ahead of the rest
            assert call(tree=t, ws=p, **kw) == MISALIGNED, (name, kw)
        assert call(tree=t, ws=p, **(dict(page=24) if paged else dict(Sk=0))) == MISALIGNED, name
        # seqLenQ > FA_TREE_MAX_Q: FA_ERR_BAD_SHAPE, in the shape step -- behind the pointers and the arrays, ahead of the types, the scale
        # and the strides; the twin of such a row count, chunked prefill, goes on to its workspace
        for rows in (65, 300, 1024):
            assert call(Sq=rows) == call(Sq=rows, ws=p) == BAD_SHAPE and call(twin=True, Sq=rows) == NULL_POINTER, (name, rows)
            assert call(Sq=rows, Q=None) == NULL_POINTER and call(Sq=rows, lens=p + 2) == MISALIGNED, (name, rows)
            assert call(Sq=rows, sinks=p + 66) == MISALIGNED, (name, rows)
            for kw in (dict(dtype=F32), dict(o=7), dict(d=96), dict(kv=F16), dict(scale=0.0),
                       dict(strides=[ctypes.byref(bad), None, None, None], d=64)):
                assert call(Sq=rows, ws=p, **kw) == BAD_SHAPE, (name, rows, kw)
        assert call(Sq=64) == NULL_POINTER and call(Sq=1025, ws=p) == BAD_SHAPE, name


def test_the_plan_is_the_plan_it_forwards_to():
    for (B, H, Hkv), d, Sk, ns, W in itertools.product(((2, 8, 2), (1, 32, 8), (7, 4, 4)), (64, 128), (384, 32768), (0, 1, 3), (0, 130)):
        for Sq in (1, 5, 16, 17, 33, 64):
            twin = "flash_attention_decode_plan_window" if Sq <= 16 else "flash_attention_extend_plan_window"
            got, want = (plan_call(s, B, H, Hkv, Sq, Sk, d, ns=ns, W=W) for s in ("flash_attention_tree_plan", twin))
            assert got == want and got[0] == 0, (B, H, Hkv, d, Sk, ns, W, Sq)
            assert fa.tree_plan(B, H, Hkv, Sq, Sk, d, F32, ns, W) == got[1]
    # the two sides of 16 / 17 are different plans
    a, b = (plan_call("flash_attention_tree_plan", 2, 8, 2, Sq, 384, 128, W=0)[1] for Sq in (16, 17))
    assert a["rows_per_block"] == 16 and b["rows_per_block"] == 64
    # refusals: the forwarded function's, a NULL plan, and the tree's own cap
    for kw in (dict(Sq=0), dict(Hkv=3), dict(d=96), dict(ns=CAP + 1), dict(W=-1), dict(Sk=0), dict(o=FP8)):
        v = dict(dict(B=2, H=8, Hkv=2, Sq=4, Sk=384, d=128, o=F32, ns=0, W=0), **kw)
        assert plan_call("flash_attention_tree_plan", **v)[0] == plan_call("flash_attention_decode_plan_window", **v)[0] < 0, kw
    assert plan_call("flash_attention_tree_plan", 2, 8, 2, 4, 384, 128, W=0, null_plan=True)[0] == NULL_POINTER
    assert plan_call("flash_attention_tree_plan", 2, 8, 2, 65, 384, 128, W=0)[0] == BAD_SHAPE
    assert plan_call("flash_attention_extend_plan_window", 2, 8, 2, 65, 384, 128, W=0)[0] == 0
    assert plan_call("flash_attention_tree_plan", 2, 8, 2, 33, 32, 128, W=0)[0] == BAD_SHAPE                 # above the capacity


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    H, Sq = 8, 5
    q = torch.zeros(2, H, Sq, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 64, 64, dtype=torch.bfloat16)
    pool = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    good = torch.zeros(2, Sq, dtype=torch.int64)
    fronts = {"flash_attention_tree": (T(q), T(k), T(k)), "flash_attention_tree_paged": (T(q), T(pool), T(pool), T(table))}
    wrong = {
        "on the CPU": good,
        "int32": T(good.int()),
        "float64": T(good.double()),
        "[B, Sq + 1]": T(torch.zeros(2, Sq + 1, dtype=torch.int64)),
        "[Sq]": T(good[0]),
        "[B, H, Sq]": T(torch.zeros(2, H, Sq, dtype=torch.int64)),
        "strided": T(torch.zeros(2, 2 * Sq, dtype=torch.int64)[:, ::2]),
        "on another device": T(good, device="cuda:1"),
        "a list": [[0] * Sq] * 2,
        "None": None,
    }
    for front, args in fronts.items():
        for what, mask in wrong.items():
            with pytest.raises(ValueError, match="tree_mask must be a dense int64 tensor"):
                getattr(fa, front)(*args, mask)
            with pytest.raises(ValueError, match="tree_mask"):
                getattr(fa, front)(*args, mask, window=16, sinks=T(torch.zeros(H)))
        # the tensors' own checks, the window's and the sinks' come first, with their usual messages
        with pytest.raises(ValueError, match="window"):
            getattr(fa, front)(*args, T(good), window=-1)
        with pytest.raises(ValueError, match="sinks"):
            getattr(fa, front)(*args, T(good), sinks=T(torch.zeros(H + 1)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_tree(q, k, k, T(good))
    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_tree(T(q), T(k[:, :, :, :32]), T(k[:, :, :, :32]), T(good))


def test_tree_mask_from_parents_is_the_ancestor_walk():
    torch = pytest.importorskip("torch")
    for Sq in (1, 2, 5, 16, 17, 33, 64):
        parents = [tc.parents_of(f, Sq, seed) for f, seed in (("chain", 0), ("star", 0), ("binary", 0), ("random", 1), ("random", 2))]
        want = [tc.words_of_parents(p) for p in parents]
        for p, w in zip(parents, want):                     # ancestor-closed, the self bit set, nothing above it
            assert all(w[i] >> i == 1 and all(w[i] | w[j] == w[i] for j in range(i) if w[i] >> j & 1) for i in range(Sq))
        got = fa.tree_mask_from_parents(torch.tensor(parents))
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(parents), Sq)
        assert torch.equal(got, tc.words_tensor(want)), Sq
        assert torch.equal(fa.tree_mask_from_parents(parents), got)                       # nested lists
        assert torch.equal(fa.tree_mask_from_parents(torch.tensor(parents, dtype=torch.int32)), got)
        depth = [[bin(w).count("1") - 1 for w in row] for row in want]                   # ancestors = depth
        d = fa.tree_depths(parents)
        assert d.dtype == torch.int32 and d.tolist() == depth
    assert tc.words_of("chain", 64)[63] == tc.FULL and int(tc.words_tensor([[tc.FULL]])[0, 0]) == -1
    for bad in ([[0]], [[-1, 1]], [[-1, 2, 0]], [[-2]], [[-1, -3]], [-1, 0], [[-1.0, 0.0]], [[-1] * 65], [[]]):
        with pytest.raises(ValueError, match="parents"):
            fa.tree_mask_from_parents(bad)
        with pytest.raises(ValueError, match="parents"):
            fa.tree_depths(bad)


# ---- the reference ----
LENGTHS = ((19, 136), (1, 300), (129, 300), (16, 9))


def test_chain_and_all_ones_words_are_the_causal_reference():
    torch = pytest.importorskip("torch")
    import sink_check as sc
    worst = 0.0
    for (d, G), Sq in itertools.product(((64, 4), (128, 1)), (1, 5, 16, 17, 64)):
        Q, K, V = sc.data(d, G, Sq, 300 + d + Sq)
        sinks = sc.sinks_for(sc.HKV * G)
        for lens, W in itertools.product(LENGTHS, sc.WINDOWS):
            want = sc.reference_sinks(Q, K, V, lens, True, W, sinks)[:2]
            plain = sc.reference_sinks(Q, K, V, lens, True, W, sinks)[2:]
            for family in tc.TWINS:
                words = [tc.words_of(family, Sq)] * tc.B
                O, lse = kv.reference(Q, K, V, lens, True, W, words=words, sinks=sinks)
                worst = max(worst, (O - want[0]).abs().max().item(), (lse - want[1]).abs().max().item())
                O, lse = kv.reference(Q, K, V, lens, True, W, words=words)
                worst = max(worst, (O - plain[0]).abs().max().item(), (lse - plain[1]).abs().max().item())
            # garbage in the ignored bits -- above i, at and beyond Sq -- and a missing self bit are not read by the rule
            words, _ = tc.case_words(Sq, Sq)
            dirty = [[(w & ~(1 << i)) | (tc.FULL << (i + 1) & tc.FULL) for i, w in enumerate(row)] for row in words]
            for b in range(tc.B):
                assert tc.effective(dirty[b], Sq) == tc.effective(words[b], Sq)
                assert torch.equal(kv.visible(lens[b], Sq, True, W, dirty[b]), kv.visible(lens[b], Sq, True, W, words[b]))
                assert bool(kv.visible(lens[b], Sq, True, W, words[b]).any(-1).all())       # no row is empty
    print(f"chain / all-ones against the causal reference: worst difference {worst:.2e}")
    assert worst < 1e-12


def test_the_condition_on_the_parity_cases_holds():
    """tree_check.run_parity without the GPU: the references of every case test_tree.py runs, and assert_masks_matter on them"""
    pytest.importorskip("torch")
    import sink_check as sc
    n = tc.run_parity(64, 4, sc.FORMS[0], (1, 5, 16, 17, 33, 64), run=False)
    assert n >= 30, n


def wrong_kernels(torch, Sq, G, W, words, lens):
    """{name: vis(b, h, L)} of five wrong ways to read the mask, each as a visibility in place of the rule's"""
    flat = [w for row in words for w in row]

    def parts(L, row_words):
        base = L - Sq
        k = torch.arange(L)[None, :]
        own = (base + torch.arange(Sq)).clamp(min=0)[:, None]
        w = tc.words_tensor([row_words])[0][:, None]
        return base, k, own, w, kv.visible(L, Sq, True, W)

    def key_index(b, h, L):                       # the bit index taken from the key, not from key - base
        base, k, own, w, causal = parts(L, words[b])
        return causal & ((k < base) | ((w >> (k & 63)) & 1).bool() | (k == own))

    def batch_zero(b, h, L):                      # the words of sequence 0 for every sequence
        return kv.visible(L, Sq, True, W, words[0])

    def no_self(b, h, L):                         # the self bit not forced
        base, k, own, w, causal = parts(L, words[b])
        return causal & ((k < base) | ((w >> (k - base).clamp(0, 63)) & 1).bool())

    def above(b, h, L):                           # bits above i honoured: the draft's keys cut by the word alone, not by the causal limit
        base, k, own, w, _ = parts(L, words[b])
        reach = kv.visible(L, Sq, False, W)   # (the window's left edge, no upper limit)
        return reach & ((k < base) | ((w >> (k - base).clamp(0, 63)) & 1).bool() | (k == own))

    def packed_row(b, h, L):                      # the word indexed by the packed row g * Sq + i instead of the query row
        g = h % G
        return kv.visible(L, Sq, True, W, [flat[(g * Sq + i) % len(flat)] for i in range(Sq)])

    return {"the bit index taken from the key": key_index, "the words of batch 0 for every sequence": batch_zero,
            "the self bit not forced": no_self, "bits above i honoured": above, "the word indexed by the packed row": packed_row}


def test_the_reference_refuses_five_wrong_kernels_each_on_a_named_row():
    """d = 64, G = 4, Sq = 16, lengths (19, 136): prefixes of 3 and 120 keys; N(0, 1) bf16 data, scale 1/8, sinks of sink_check.  The
    words: sequence 0 a binary tree, sequence 1 a star, both WITHOUT their self bits and with every bit above i set -- the rule
    ignores both, a wrong kernel need not.  Each emulation must miss kv_cache_check.assert_close's bounds by more than 10 x on the row
    named here (sequence, head, row), and the reference itself on the clean words must be the reference on the dirty ones."""
    torch = pytest.importorskip("torch")
    import sink_check as sc
    d, G, Sq, W, lens = 64, 4, 16, 0, (19, 136)
    Q, K, V = sc.data(d, G, Sq, 777)
    sinks = sc.sinks_for(sc.HKV * G)
    clean = [tc.words_of("binary", Sq), tc.words_of("star", Sq)]
    words = [[(w & ~(1 << i)) | (tc.FULL << (i + 1) & tc.FULL) for i, w in enumerate(row)] for row in clean]
    refO, refL = kv.reference(Q, K, V, lens, True, W, words=words, sinks=sinks)
    cleanO, cleanL = kv.reference(Q, K, V, lens, True, W, words=clean, sinks=sinks)
    assert torch.equal(refO, cleanO) and torch.equal(refL, cleanL)
    named = {"the bit index taken from the key": (0, 0, 9), "the words of batch 0 for every sequence": (1, 3, 7),
             "the self bit not forced": (1, 5, 4), "bits above i honoured": (0, 2, 0), "the word indexed by the packed row": (0, 1, 6)}
    kernels = wrong_kernels(torch, Sq, G, W, words, lens)
    assert sorted(kernels) == sorted(named) and len(kernels) == 5
    for name, vis in kernels.items():
        O, lse = kv.reference(Q, K, V, lens, True, W, words=words, sinks=sinks, vis=vis)
        off = tc.differing_rows(O, lse, refO, refL, factor=10.0)
        eo, el = sc.excess(O[off], lse[off], refO[off], refL[off])
        print(f"{name}: {int(off.sum())} of {off.numel()} rows beyond 10 x the tolerance; worst O {eo:.0f} x, LSE {el:.0f} x")
        assert bool(off[named[name]]), f"{name}: row {named[name]} passes"
