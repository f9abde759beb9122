"""CPU tests of the sliding-window decode entry points (flash_attention_decode_window, flash_attention_decode_paged_window,
flash_attention_decode_plan_window) at the C ABI and in the binding: the symbols exist with the declared parameter lists and argtypes,
every invalid argument is refused with its code before anything is launched (fake aligned host pointers: no GPU is touched; no call
here is valid as a whole), the plan follows the window's tiles, and the tests' own reference mask equals a brute-force double loop."""
import ctypes
import functools

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, declared_parameters, host_calls, plan_call, tiles)


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    i = ctypes.c_int
    # the _fp8 siblings' lists with windowSize after numSplits
    for name, sibling in (("flash_attention_decode_window", "flash_attention_decode_fp8"),
                          ("flash_attention_decode_paged_window", "flash_attention_decode_paged_fp8")):
        assert name in fa.EXPORTS and getattr(L, name) is not None
        want = declared_parameters(sibling)
        at = want.index("numSplits") + 1
        want.insert(at, "windowSize")
        assert declared_parameters(name) == want, name
        sib = list(getattr(L, sibling).argtypes)
        sib.insert(at, i)
        assert list(getattr(L, name).argtypes) == sib, name
        assert getattr(L, name).restype is i
    assert declared_parameters("flash_attention_decode_window") == [
        "Q", "K", "V", "O", "LSE", "kvLens", "kDescale", "vDescale", "workspace", "batchSize", "numHeads", "numHeadsKV", "seqLenQ",
        "seqLenK", "dHead", "scale", "is_causal", "dtype", "kv_dtype", "o_dtype", "numSplits", "windowSize", "sQ", "sK", "sV", "sO",
        "stream"]
    assert declared_parameters("flash_attention_decode_paged_window") == [
        "Q", "Kpool", "Vpool", "O", "LSE", "kvLens", "blockTable", "kDescale", "vDescale", "workspace", "batchSize", "numHeads",
        "numHeadsKV", "seqLenQ", "numPages", "pageSize", "maxPagesPerSeq", "tableStride", "dHead", "scale", "is_causal", "dtype",
        "kv_dtype", "o_dtype", "numSplits", "windowSize", "sQ", "sK", "sV", "sO", "stream"]
    name = "flash_attention_decode_plan_window"
    assert name in fa.EXPORTS
    want = declared_parameters("flash_attention_decode_plan")
    want.insert(want.index("numSplits") + 1, "windowSize")
    assert declared_parameters(name) == want == ["batchSize", "numHeads", "numHeadsKV", "seqLenQ", "seqLenK", "dHead", "o_dtype",
                                                 "numSplits", "windowSize", "plan"]
    sib = list(L.flash_attention_decode_plan.argtypes)
    sib.insert(8, i)
    assert list(getattr(L, name).argtypes) == sib and getattr(L, name).restype is i


def calls(kv):
    """(contiguous call, paged call, an aligned host pointer) for a cache of type `kv`; keyword arguments override a call that is
    valid but for its workspace: two splits and none given, so that a call that passes every other check stops at NULL_POINTER"""
    okc = dict(B=2, H=8, Hkv=2, Sq=1, Sk=1024, d=128, scale=0.125, causal=False, dtype=BF16, kv=kv, o=F32, ns=2, W=128)
    okp = dict(B=2, H=8, Hkv=2, Sq=1, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=False, dtype=BF16, kv=kv, o=F32, ns=2,
               W=128)
    return host_calls(("flash_attention_decode_window", okc), ("flash_attention_decode_paged_window", okp))


@pytest.mark.parametrize("W", [128, 0, 5000])
@pytest.mark.parametrize("kv", [BF16, FP8])
def test_what_the_siblings_refuse_is_refused_with_the_same_codes(kv, W):
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    contiguous, paged, p = calls(kv)
    for fn in (contiguous, paged):
        call = lambda fn=fn, **kw: fn(**dict(dict(W=W), **kw))
        assert call() == NULL_POINTER        # valid but for the workspace of its two splits
        for name in ("Q", "K", "V", "O"):
            assert call(**{name: None}) == NULL_POINTER, name
            assert call(**{name: p + 8}) == MISALIGNED, name
        assert call(LSE=p + 4) == MISALIGNED and call(ws=p + 8) == MISALIGNED and call(lens=p + 2) == MISALIGNED
        for kw in (dict(Sq=0), dict(Sq=17), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0), dict(Hkv=16),
                   dict(Hkv=-2), dict(ns=-1), dict(ns=CAP + 1)):
            assert call(ws=p, **kw) == BAD_SHAPE, kw
        for kw in (dict(o=FP8), dict(o=7), dict(dtype=F32), dict(dtype=FP8), dict(dtype=F16), dict(dtype=9), dict(kv=F32), dict(kv=F16),
                   dict(kv=9), dict(kv=-1)):
            assert call(**kw) == BAD_DTYPE, kw
        for d in (96, 32, 256, 120):
            assert call(d=d) == BAD_DHEAD, d
        for s in (0.0, -0.5, float("nan"), float("inf")):
            assert call(scale=s) == BAD_SCALE, s
        bad = fa.FaStrides(64, 16, 8)            # strideS < d
        mis = fa.FaStrides(1024, 66, 66)         # d = 64: 132-byte bf16 rows, 264-byte fp32 rows, 66-byte fp8 rows: no multiples of 16
        for i in range(4):
            for s in (bad, mis):
                st = [None] * 4
                st[i] = ctypes.byref(s)
                assert call(strides=st, d=64) == BAD_STRIDE, i
    for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1)):
        assert contiguous(ws=p, W=W, **kw) == BAD_SHAPE, kw
    assert paged(table=None, W=W) == NULL_POINTER
    assert paged(table=p + 2, W=W) == MISALIGNED and paged(table=p + 1, W=W) == MISALIGNED
    for kw in (dict(P=0), dict(P=-1), dict(maxp=0, ts=16), dict(maxp=-3), dict(page=8), dict(page=0), dict(page=-16), dict(page=1),
               dict(page=24), dict(page=48), dict(page=100), dict(page=(1 << 20) + 16),
               dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21),        # capacity 2^24 + 16: the cap stays
               dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),         # capacity 2^32: no 32-bit wrap-around
               dict(page=1 << 30, maxp=4, ts=4),
               dict(ts=15), dict(ts=0), dict(ts=-16)):
        assert paged(ws=p, W=W, **kw) == BAD_SHAPE, kw
    # the extent limit of the cache's type: (seqLenK + 192) x row stride in BYTES below 2^31
    big = (1 << 24) - 193
    assert contiguous(Sk=big, W=W) == (NULL_POINTER if kv == FP8 else BAD_SHAPE)
    assert contiguous(Sk=1 << 24, W=W) == BAD_SHAPE


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_new_refusals(kv):
    contiguous, paged, p = calls(kv)
    for call in (contiguous, paged):
        for W in (-1, -128, -(1 << 31)):
            assert call(W=W, ws=p) == BAD_SHAPE, W
        for W in (0, 1, 128, 1 << 24, (1 << 31) - 1):       # any window >= 0 passes on to the workspace check
            assert call(W=W) == NULL_POINTER, W
        # descales: those of an fp8 cache, 4-byte aligned; a bf16 cache has none
        for kw in (dict(kd=p), dict(vd=p + 8), dict(kd=p + 4, vd=p + 12)):
            assert call(**kw) == (NULL_POINTER if kv == FP8 else BAD_DTYPE), kw
            assert call(W=0, **kw) == (NULL_POINTER if kv == FP8 else BAD_DTYPE), kw
        if kv == FP8:
            for name in ("kd", "vd"):
                for off in (1, 2, 3, 6):
                    assert call(**{name: p + off}) == MISALIGNED, (name, off)
    # the library's own split count: without a window a capacity of 32 768 plans more than one split and the workspace is missing;
    # so it is under a window wide enough for two (a window of one tile plans one split, needs none, and would launch: not called)
    assert contiguous(ns=0, W=0, Sk=32768) == NULL_POINTER and paged(ns=0, W=0, maxp=512, ts=512) == NULL_POINTER
    assert fa.decode_plan(2, 8, 2, 1, 32768, 128, F32, 0, window=4096)["num_splits"] > 1
    assert contiguous(ns=0, W=4096, Sk=32768) == NULL_POINTER and paged(ns=0, W=4096, maxp=512, ts=512) == NULL_POINTER
    assert fa.decode_plan(2, 8, 2, 1, 32768, 128, F32, 0, window=128)["num_splits"] == 1


plan_window = functools.partial(plan_call, "flash_attention_decode_plan_window")


def test_the_plan_follows_the_window():
    shapes = [(1, 32, 8, 1, 131072, 128), (1, 32, 8, 1, 131072, 64), (4, 8, 2, 3, 32768, 128), (2, 8, 8, 16, 640, 64), (64, 32, 8, 1, 8192, 128),
              (1, 8, 2, 1, 100, 64), (3, 16, 1, 5, 4096, 128)]
    for B, H, Hkv, Sq, Sk, d in shapes:
        plain = fa.decode_plan(B, H, Hkv, Sq, Sk, d, F32)
        # window 0 and any window >= seqLenK: the un-windowed plan, field for field; C function and binding
        for W in (0, Sk, Sk + 1, 2 * Sk, (1 << 31) - 1):
            assert plan_window(B, H, Hkv, Sq, Sk, d, F32, 0, W) == (0, plain), W
            assert fa.decode_plan(B, H, Hkv, Sq, Sk, d, F32, 0, window=W) == plain, W
        assert fa.decode_plan(B, H, Hkv, Sq, Sk, d, F32, 0, window=None) == plain
        for W in (1, 2, 16, 127, 128, 129, 255, 256, 300, 1024, 4096, 4097, 20000, Sk - 1):
            if W < 1:
                continue
            rc, plan = plan_window(B, H, Hkv, Sq, Sk, d, F32, 0, W)
            assert rc == 0 and plan == fa.decode_plan(B, H, Hkv, Sq, Sk, d, F32, 0, window=W)
            ns = plan["num_splits"]
            assert 1 <= ns <= min(tiles(W + Sq - 1) + 1, CAP) and ns <= plain["num_splits"], (W, plan)
            # everything but the split count and what follows from it is the un-windowed plan's
            assert plan["grid"] == plain["grid"] // plain["num_splits"] * ns
            assert (plan["combine_grid"], plan["combine_threads"]) == ((B * H * Sq, 256) if ns > 1 else (0, 0))
            for k in ("row_blocks", "rows_per_block", "kv_block_rows", "threads", "lds_bytes"):
                assert plan[k] == plain[k], k
            # forced split counts are returned as given
            for forced in (1, 2, 3, 5, 8, CAP):
                rc, f = plan_window(B, H, Hkv, Sq, Sk, d, F32, forced, W)
                assert rc == 0 and f["num_splits"] == forced and f == fa.decode_plan(B, H, Hkv, Sq, Sk, d, F32, forced), (W, forced)
    rc, plan = plan_window(1, 32, 8, 1, 131072, 128, F32, 0, 128)
    assert rc == 0 and plan["num_splits"] == 1 and plan["combine_grid"] == 0 and plan["combine_threads"] == 0
    # a long cache that one sequence must be split over: the window decides, not the capacity
    assert fa.decode_plan(1, 32, 8, 1, 131072, 128, F32)["num_splits"] > 8
    assert 1 < fa.decode_plan(1, 32, 8, 1, 131072, 128, F32, 0, window=4096)["num_splits"] <= tiles(4096) + 1
    # refusals: the plan function's own, and a negative window; the binding raises before it calls
    assert plan_window(1, 32, 8, 1, 1024, 128, F32, 0, -1)[0] == BAD_SHAPE
    assert plan_window(1, 32, 8, 17, 1024, 128, F32, 0, 128)[0] == BAD_SHAPE
    assert plan_window(1, 32, 8, 1, 1024, 96, F32, 0, 128)[0] == BAD_DHEAD
    assert plan_window(1, 32, 8, 1, 1024, 128, FP8, 0, 128)[0] == BAD_DTYPE
    assert plan_window(1, 32, 8, 1, 1024, 128, F32, 0, 128, null_plan=True)[0] == NULL_POINTER
    with pytest.raises(ValueError, match="window"):
        fa.decode_plan(1, 32, 8, 1, 1024, 128, F32, 0, window=-1)


def test_the_reference_mask_equals_a_brute_force_double_loop():
    torch = pytest.importorskip("torch")
    from kv_cache_check import first_visible, visible
    for L in range(1, 41):
        for Sq in range(1, 6):
            for causal in (False, True):
                for W in range(1, 46):
                    want = torch.zeros(Sq, L, dtype=torch.bool)
                    for i in range(Sq):
                        limc = max(L - Sq + i + 1, 1)
                        lo = max(limc - W, 0)
                        for k in range(L):
                            want[i, k] = lo <= k < (limc if causal else L)
                    got = visible(L, Sq, causal, W)
                    assert got.dtype == torch.bool and torch.equal(got, want), (L, Sq, causal, W)
                    assert got.any(dim=1).all(), (L, Sq, causal, W)                     # every row sees at least one key
                    assert int(got.any(dim=0).nonzero()[0]) == first_visible(L, Sq, W)  # ... and row 0's left edge is the lowest
                    if causal:
                        assert (got.sum(dim=1) <= W).all()                             # at most the last W keys
                    if W >= L:
                        assert torch.equal(got, visible(L, Sq, causal)), (L, Sq, causal, W)
                assert torch.equal(visible(L, Sq, causal, 0), visible(L, Sq, causal))
                assert first_visible(L, Sq, 0) == 0


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    q = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 32, 64, dtype=torch.bfloat16)
    pool = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_decode(q, k, k, window=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_decode_paged(q, pool, pool, table, window=16)
    for W in (-1, -128):
        with pytest.raises(ValueError, match="window"):
            fa.flash_attention_decode(T(q), T(k), T(k), window=W)
        with pytest.raises(ValueError, match="window"):
            fa.flash_attention_decode_paged(T(q), T(pool), T(pool), T(table), window=W)
    # a bf16 cache takes no descales, window or not
    ones = torch.ones(2)
    with pytest.raises(ValueError, match="descale"):
        fa.flash_attention_decode(T(q), T(k), T(k), k_descale=T(ones), window=16)
