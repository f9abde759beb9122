"""CPU tests of windowed chunked prefill (flash_attention_extend_window, _extend_paged_window, _extend_varlen_window,
_extend_paged_varlen_window, flash_attention_extend_plan_window, flash_attention_extend_varlen_plan_window) at the C ABI and in the
binding: the six symbols with their declared parameter lists, every refusal of the un-windowed sibling returned with the same code at
windows 0 / 128 / 5000 (fake aligned host pointers: no GPU is touched; no call here is valid as a whole), the plan, and the Python
model of the per-row-block tile range (extend_window_check.block_range) against a brute-force hull over kv_cache_check.visible."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, aligned_host_pointer, declared_parameters, host_call, tiles)
from abi_decl import plan_call as plan_window  # noqa: E402

CALLS = ("flash_attention_extend", "flash_attention_extend_paged", "flash_attention_extend_varlen", "flash_attention_extend_paged_varlen")
PLANS = ("flash_attention_extend_plan", "flash_attention_extend_varlen_plan")


def test_the_six_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    i = ctypes.c_int
    for sibling in CALLS + PLANS:
        name = sibling + "_window"
        assert name in fa.EXPORTS and getattr(L, name) is not None
        want = declared_parameters(sibling)
        at = want.index("numSplits") + 1
        want.insert(at, "windowSize")              # directly after numSplits, as in the decode _window calls
        assert declared_parameters(name) == want, name
        sib = list(getattr(L, sibling).argtypes)
        sib.insert(at, i)
        assert list(getattr(L, name).argtypes) == sib, name
        assert getattr(L, name).restype is i
    assert declared_parameters("flash_attention_extend_window") == declared_parameters("flash_attention_decode_window")
    assert declared_parameters("flash_attention_extend_paged_window") == declared_parameters("flash_attention_decode_paged_window")
    assert declared_parameters("flash_attention_extend_plan_window") == declared_parameters("flash_attention_decode_plan_window")
    assert declared_parameters("flash_attention_extend_varlen_plan_window") == [
        "batchSize", "numHeads", "numHeadsKV", "totalQ", "seqLenK", "dHead", "o_dtype", "numSplits", "windowSize", "plan"]


def calls(kv):
    """{name: call(W, **overrides)} for the four forms and an aligned host pointer.  W = None calls the un-windowed sibling.  Every
    call is valid but for its workspace: two splits and none given, so that passing every other check ends at NULL_POINTER"""
    host = aligned_host_pointer()
    ok = dict(B=2, H=8, Hkv=2, Sq=300, Sk=1024, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=True, dtype=BF16, kv=kv, o=F32,
              ns=2)

    def make(name):
        sibling = host_call(name, ok, host)[0]
        return lambda W, **kw: sibling(**kw) if W is None else sibling(symbol=name + "_window", W=W, **kw)

    return {name: make(name) for name in CALLS}, host[1]


def ladder(p, kv, paged, ragged):
    """the arguments the siblings refuse (and a few they accept up to the workspace check), as keyword overrides"""
    out = [dict()]
    for name in ("Q", "K", "V", "O"):
        out += [{name: None}, {name: p + 8}]
    out += [dict(LSE=p + 4), dict(ws=p + 8), dict(lens=p + 2)]
    out += [dict(ws=p, **kw) for kw in (dict(Sq=0), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0),
                                        dict(Hkv=16), dict(Hkv=-2), dict(ns=-1), dict(ns=CAP + 1), dict(Sq=(1 << 31) - 1))]
    # (a workspace is only ever passed with an argument that is invalid in that form: nothing here may reach a launch)
    if ragged:      # totalQ is not capped by the capacity; the batch is
        out += [dict(Sq=1025), dict(Sq=5000), dict(ws=p, B=fa.FA_VARLEN_MAX_BATCH + 1)]
    else:
        out += [dict(ws=p, Sq=1025), dict(ws=p, Sq=5000)]
    out += [dict(Sq=s) for s in (1, 16, 17, 1023, 1024)]
    out += [dict(o=FP8), dict(o=7), dict(dtype=F32), dict(dtype=FP8), dict(dtype=F16), dict(dtype=9), dict(kv=F32), dict(kv=F16), dict(kv=9),
            dict(kv=-1)]
    out += [dict(d=d) for d in (96, 32, 256, 120)]
    out += [dict(scale=s) for s in (0.0, -0.5, float("nan"), float("inf"))]
    out += [dict(kd=p), dict(vd=p + 8), dict(kd=p + 4, vd=p + 12), dict(kd=p + 1), dict(vd=p + 2), dict(kd=p + 6)]
    if ragged:
        out += [dict(cu=None), dict(cu=p + 2), dict(cu=p + 1)]
    if paged:
        out += [dict(table=None), dict(table=p + 2), dict(table=p + 1)]
        out += [dict(ws=p, **kw) for kw in (dict(P=0), dict(P=-1), dict(maxp=0, ts=16), dict(maxp=-3), dict(page=8), dict(page=0),
                                            dict(page=-16), dict(page=24), dict(page=100), dict(page=(1 << 20) + 16),
                                            dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21), dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),
                                            dict(page=1 << 30, maxp=4, ts=4), dict(ts=15), dict(ts=0), dict(ts=-16))]
    else:
        out += [dict(ws=p, **kw) for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1))]
        out += [dict(Sk=(1 << 24) - 193), dict(Sk=1 << 24)]
    return out


@pytest.mark.parametrize("W", [0, 128, 5000])
@pytest.mark.parametrize("kv", [BF16, FP8])
def test_what_the_siblings_refuse_is_refused_with_the_same_codes(kv, W):
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    fns, p = calls(kv)
    bad = fa.FaStrides(64, 16, 8)            # strideS < d
    mis = fa.FaStrides(1024, 66, 66)         # d = 64: rows that are no multiples of 16 bytes
    for name, call in fns.items():
        assert call(W) == call(None) == NULL_POINTER, name          # valid but for the workspace of its two splits
        for kw in ladder(p, kv, "paged" in name, "varlen" in name):
            want = call(None, **kw)
            assert NULL_POINTER >= want >= BAD_STRIDE, (name, kw, want)
            assert call(W, **kw) == want, (name, kw)
        for i in range(4):
            for s in (bad, mis):
                st = [None] * 4
                st[i] = ctypes.byref(s)
                assert call(W, strides=st, d=64) == call(None, strides=st, d=64) == BAD_STRIDE, (name, i)
        # a few of the ladder's codes spelled out
        assert call(W, Q=None) == NULL_POINTER and call(W, K=p + 8) == MISALIGNED and call(W, ws=p, ns=CAP + 1) == BAD_SHAPE
        assert call(W, d=96) == BAD_DHEAD and call(W, dtype=F32) == BAD_DTYPE and call(W, scale=0.0) == BAD_SCALE
        assert call(W, kd=p) == (NULL_POINTER if kv == FP8 else BAD_DTYPE)
        if "varlen" not in name:
            assert call(W, ws=p, Sq=1025) == BAD_SHAPE                # the chunk is capped by the capacity


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_a_negative_window_is_refused_and_any_other_passes_on(kv):
    fns, p = calls(kv)
    for name, call in fns.items():
        for W in (-1, -128, -(1 << 31)):
            assert call(W, ws=p) == BAD_SHAPE, (name, W)
        for W in (0, 1, 128, 1 << 24, (1 << 31) - 1):       # any window >= 0 passes on to the workspace check
            assert call(W) == NULL_POINTER, (name, W)
    # the library's own split count under a window wide enough for two splits: the workspace is missing
    assert fa.extend_plan(2, 8, 2, 17, 32768, 128, F32, 0, window=4096)["num_splits"] > 1
    assert fns["flash_attention_extend"](4096, ns=0, Sq=17, Sk=32768) == NULL_POINTER
    assert fns["flash_attention_extend_paged"](4096, ns=0, Sq=17, maxp=512, ts=512) == NULL_POINTER


@pytest.mark.parametrize("ragged", [False, True])
def test_the_plan_follows_the_window(ragged):
    fn = "flash_attention_extend_varlen_plan_window" if ragged else "flash_attention_extend_plan_window"
    front = fa.extend_varlen_plan if ragged else fa.extend_plan
    shapes = [(1, 32, 8, 512, 8192 + 512, 128), (1, 32, 8, 512, 32768 + 512, 64), (1, 32, 8, 2048, 2048, 128), (1, 32, 8, 64, 32768, 128),
              (8, 32, 8, 300, 4096, 128), (2, 8, 8, 17, 640, 64), (3, 16, 1, 5, 4096, 128), (2, 8, 2, 200, 640, 64), (1, 8, 8, 17, 131072, 128)]
    for B, H, Hkv, Sq, Sk, d in shapes:
        plain = front(B, H, Hkv, Sq, Sk, d, F32)
        # window 0 and any window >= the capacity: the un-windowed plan, field for field; C function and binding
        for W in (0, Sk, Sk + 1, 2 * Sk, (1 << 31) - 1):
            assert plan_window(fn, B, H, Hkv, Sq, Sk, d, F32, 0, W) == (0, plain), W
            assert front(B, H, Hkv, Sq, Sk, d, F32, 0, window=W) == plain, W
        assert front(B, H, Hkv, Sq, Sk, d, F32, 0, window=None) == plain
        for W in (1, 16, 127, 128, 129, 300, 1024, 4096, 4097, 20000, Sk - 1):
            rc, plan = plan_window(fn, B, H, Hkv, Sq, Sk, d, F32, 0, W)
            assert rc == 0 and plan == front(B, H, Hkv, Sq, Sk, d, F32, 0, window=W)
            ns = plan["num_splits"]
            bound = min(tiles(Sk), tiles(W + Sq - 1) + 1)
            assert 1 <= ns <= min(bound, CAP) and ns <= plain["num_splits"], (W, plan)
            # everything but the split count and what follows from it is the un-windowed plan's
            assert plan["grid"] == plain["grid"] // plain["num_splits"] * ns
            rows = H * Sq if ragged else B * H * Sq
            assert (plan["combine_grid"], plan["combine_threads"]) == ((rows, 256) if ns > 1 else (0, 0))
            for k in ("row_blocks", "rows_per_block", "kv_block_rows", "threads", "lds_bytes"):
                assert plan[k] == plain[k], k
            for forced in (1, 2, 3, 5, 8, CAP):                   # forced split counts are returned as given
                rc, f = plan_window(fn, B, H, Hkv, Sq, Sk, d, F32, forced, W)
                assert rc == 0 and f["num_splits"] == forced and f == front(B, H, Hkv, Sq, Sk, d, F32, forced), (W, forced)
    # a short chunk on a long cache: the window decides, not the capacity
    assert front(1, 8, 8, 17, 131072, 128, F32)["num_splits"] > 8
    assert 1 < front(1, 8, 8, 17, 131072, 128, F32, 0, window=512)["num_splits"] <= tiles(512 + 16) + 1
    # refusals: the plan function's own, and a negative window; the binding raises before it calls
    assert plan_window(fn, 1, 32, 8, 20, 1024, 128, F32, 0, -1)[0] == BAD_SHAPE
    assert plan_window(fn, 1, 32, 8, 0, 1024, 128, F32, 0, 128)[0] == BAD_SHAPE
    assert plan_window(fn, 1, 32, 8, 20, 1024, 96, F32, 0, 128)[0] == BAD_DHEAD
    assert plan_window(fn, 1, 32, 8, 20, 1024, 128, FP8, 0, 128)[0] == BAD_DTYPE
    assert plan_window(fn, 1, 32, 8, 20, 1024, 128, F32, 0, 128, null_plan=True)[0] == NULL_POINTER
    if not ragged:
        assert plan_window(fn, 1, 32, 8, 1025, 1024, 128, F32, 0, 128)[0] == BAD_SHAPE
    with pytest.raises(ValueError, match="window"):
        front(1, 32, 8, 20, 1024, 128, F32, 0, window=-1)


def test_the_block_range_model_is_the_hull_of_the_tiles_a_block_sees():
    """extend_window_check.block_range against the brute-force hull over kv_cache_check.visible: equality for Sq > 16, decode's range for
    Sq <= 16 (which holds the hull).  Includes the issue's example"""
    pytest.importorskip("torch")
    from extend_window_check import block_hull, block_range, decode_range, row_edges
    assert [block_range(64, 1, 200, 640, 100, True, rb) for rb in range(4)] == [(2, 4), (3, 5), (3, 5), (4, 5)]
    checked = 0
    for Sq in (1, 5, 16, 17, 31, 32, 33, 40, 64, 65, 100, 130, 200):
        for L in (1, 15, 37, 128, 129, 200, 257, 400, 511, 640):
            for W in (1, 16, 17, 100, 127, 128, 129, 300, 640):
                for causal in (False, True):
                    edges = row_edges(L, Sq, causal, W)
                    for RPB in (32, 64):
                        for G in (1, 2, 4):
                            for rb in range(-(-G * Sq // RPB)):
                                got, hull = block_range(RPB, G, Sq, L, W, causal, rb), block_hull(edges, RPB, G, Sq, rb)
                                if Sq > 16:
                                    assert got == hull, (RPB, G, Sq, L, W, causal, rb)
                                else:
                                    assert got == decode_range(Sq, L, W), (RPB, G, Sq, L, W, causal, rb)
                                    assert got[0] <= hull[0] and hull[1] <= got[1]
                                checked += 1
    assert checked > 30000


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    q = torch.zeros(2, 8, 40, 64, dtype=torch.bfloat16)
    qt = torch.zeros(40, 8, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 64, 64, dtype=torch.bfloat16)
    pool = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    cu = torch.tensor([0, 30, 40], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_extend_window(q, k, k, window=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_extend_paged_window(q, pool, pool, table, window=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_extend_varlen_window(qt, k, k, cu, window=16)
    for W in (-1, -128):
        with pytest.raises(ValueError, match="window"):
            fa.flash_attention_extend_window(T(q), T(k), T(k), window=W)
        with pytest.raises(ValueError, match="window"):
            fa.flash_attention_extend_paged_window(T(q), T(pool), T(pool), T(table), window=W)
        with pytest.raises(ValueError, match="window"):
            fa.flash_attention_extend_varlen_window(T(qt), T(k), T(k), T(cu), window=W)
        with pytest.raises(ValueError, match="window"):
            fa.flash_attention_extend_paged_varlen_window(T(qt), T(pool), T(pool), T(table), T(cu), window=W)
        with pytest.raises(ValueError, match="window"):
            fa.extend_plan(2, 8, 2, 40, 64, 64, window=W)
        with pytest.raises(ValueError, match="window"):
            fa.extend_varlen_plan(2, 8, 2, 40, 64, 64, window=W)
    # a bf16 cache takes no descales, window or not
    with pytest.raises(ValueError, match="descale"):
        fa.flash_attention_extend_window(T(q), T(k), T(k), k_descale=T(torch.ones(2)), window=16)
