"""CPU tests of flash_attention_decode_fp8 and flash_attention_decode_paged_fp8 (split-KV decode against e4m3fn K/V caches) at the
C ABI and in the binding: the symbols exist with the declared parameter lists and argtypes, every invalid argument is refused with
its code before anything is launched (fake aligned host pointers: no GPU is touched), the plan does not depend on the cache type,
and the binding refuses host tensors, fp8 Q, mismatched dtypes and bad descales."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, declared_parameters, host_calls)


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    sp, vp, i = ctypes.POINTER(fa.FaStrides), ctypes.c_void_p, ctypes.c_int
    # the siblings' lists with kDescale, vDescale after kvLens (paged: after blockTable) and kv_dtype after dtype
    for name, sibling, after in (("flash_attention_decode_fp8", "flash_attention_decode", "kvLens"),
                                 ("flash_attention_decode_paged_fp8", "flash_attention_decode_paged", "blockTable")):
        assert name in fa.EXPORTS and getattr(L, name) is not None
        want = declared_parameters(sibling)
        want[want.index(after) + 1:want.index(after) + 1] = ["kDescale", "vDescale"]
        want.insert(want.index("dtype") + 1, "kv_dtype")
        assert declared_parameters(name) == want, name
        sib = list(getattr(L, sibling).argtypes)
        at = declared_parameters(sibling)
        sib[at.index(after) + 1:at.index(after) + 1] = [vp, vp]
        sib.insert(want.index("kv_dtype"), i)
        assert list(getattr(L, name).argtypes) == sib, name
        assert getattr(L, name).restype is i
    assert declared_parameters("flash_attention_decode_fp8") == [
        "Q", "K", "V", "O", "LSE", "kvLens", "kDescale", "vDescale", "workspace", "batchSize", "numHeads", "numHeadsKV", "seqLenQ",
        "seqLenK", "dHead", "scale", "is_causal", "dtype", "kv_dtype", "o_dtype", "numSplits", "sQ", "sK", "sV", "sO", "stream"]


def calls():
    """(contiguous call, paged call, an aligned host pointer); keyword arguments override a valid call"""
    okc = dict(B=2, H=8, Hkv=2, Sq=1, Sk=1024, d=128, scale=0.125, causal=False, dtype=BF16, kv=FP8, o=F32, ns=1)
    okp = dict(B=2, H=8, Hkv=2, Sq=1, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=False, dtype=BF16, kv=FP8, o=F32, ns=1)
    return host_calls(("flash_attention_decode_fp8", okc), ("flash_attention_decode_paged_fp8", okp))


def test_what_the_siblings_refuse_is_refused_with_the_same_codes():
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    contiguous, paged, p = calls()
    for call in (contiguous, paged):
        for name in ("Q", "K", "V", "O"):
            assert call(**{name: None}) == NULL_POINTER, name
            assert call(**{name: p + 8}) == MISALIGNED, name
        assert call(LSE=p + 4) == MISALIGNED and call(ws=p + 8, ns=2) == MISALIGNED and call(lens=p + 2) == MISALIGNED
        assert call(ns=2, ws=None) == NULL_POINTER
        for kw in (dict(Sq=0), dict(Sq=17), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0), dict(Hkv=16),
                   dict(Hkv=-2), dict(ns=-1), dict(ns=CAP + 1)):
            assert call(ws=p, **kw) == BAD_SHAPE, kw
        for kw in (dict(o=FP8), dict(o=7)):
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
    assert contiguous(ns=0, ws=None, Sk=32768) == NULL_POINTER           # (0: the library plans > 1 split for a capacity of 32 768)
    assert paged(ns=0, ws=None, maxp=512, ts=512) == NULL_POINTER
    for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1)):
        assert contiguous(ws=p, **kw) == BAD_SHAPE, kw
    assert paged(table=None) == NULL_POINTER
    assert paged(table=p + 2) == MISALIGNED and paged(table=p + 1) == MISALIGNED
    for kw in (dict(P=0), dict(P=-1), dict(maxp=0, ts=16), dict(maxp=-3), dict(page=8), dict(page=0), dict(page=-16), dict(page=1),
               dict(page=24), dict(page=48), dict(page=100), dict(page=(1 << 20) + 16),
               dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21),        # capacity 2^24 + 16: the cap stays
               dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),         # capacity 2^32: no 32-bit wrap-around
               dict(page=1 << 30, maxp=4, ts=4),
               dict(ts=15), dict(ts=0), dict(ts=-16)):
        assert paged(ws=p, **kw) == BAD_SHAPE, kw


def test_the_new_refusals():
    contiguous, paged, p = calls()
    for call in (contiguous, paged):
        # the cache type and the type of Q
        for kv in (BF16, F32, F16, 9, -1):
            assert call(kv=kv) == BAD_DTYPE, kv
        for dt in (F32, FP8, F16, 9):
            assert call(dtype=dt) == BAD_DTYPE, dt
        # descales: 4-byte aligned, each on its own; aligned ones pass on to the workspace two splits need
        for name in ("kd", "vd"):
            for off in (1, 2, 3, 6):
                assert call(**{name: p + off}) == MISALIGNED, (name, off)
        assert call(kd=p + 4, vd=p + 12, ns=2, ws=None) == NULL_POINTER
        assert call(kd=p, ns=2, ws=None) == NULL_POINTER and call(vd=p + 8, ns=2, ws=None) == NULL_POINTER
        # K / V strides are in one-byte elements: every one a multiple of 16.  8 elements were 16 bytes of bf16: not enough here
        for bad in (fa.FaStrides(1 << 20, 1 << 16, 136), fa.FaStrides(1 << 20, (1 << 16) + 8, 128), fa.FaStrides((1 << 20) + 8, 1 << 16, 128)):
            for i in (1, 2):
                st = [None] * 4
                st[i] = ctypes.byref(bad)
                assert call(strides=st) == BAD_STRIDE, i
            st = [ctypes.byref(bad), None, None, None]      # ... and Q is still bf16: 8 elements are 16 bytes
            assert call(strides=st, ns=2, ws=None) == NULL_POINTER
        good = fa.FaStrides(1 << 20, 1 << 16, 144)          # a row stride larger than d, multiple of 16
        assert call(strides=[None, ctypes.byref(good), ctypes.byref(good), None], ns=2, ws=None) == NULL_POINTER


def test_the_extent_limits_are_counted_in_bytes():
    contiguous, paged, p = calls()
    # contiguous: (seqLenK + 192) x row stride x 1 byte < 2^31.  Dense d = 128 rows: every capacity up to the cap of 2^24 keys has
    # (2^24 + 192) * 128 = 2^31 + 24576 bytes, so 2^24 itself is refused and 2^24 - 192 - 1 is accepted; the bf16 call refuses both
    assert contiguous(Sk=1 << 24, ns=2, ws=None) == BAD_SHAPE
    assert contiguous(Sk=(1 << 24) - 193, ns=2, ws=None) == NULL_POINTER
    assert contiguous(Sk=(1 << 24) - 192, ns=2, ws=None) == BAD_SHAPE
    assert contiguous(symbol="flash_attention_decode", Sk=(1 << 24) - 193, ns=2, ws=None) == BAD_SHAPE
    # a wide row stride, for K and for V: 1024 rows + 192 at 2^21 bytes is 2^31 + ...; at 2^20 bytes it fits (bf16: it would not)
    for stride, want in ((1 << 21, BAD_SHAPE), (1 << 20, NULL_POINTER)):
        s = fa.FaStrides(1 << 40, 1 << 36, stride)
        for i in (1, 2):
            st = [None] * 4
            st[i] = ctypes.byref(s)
            assert contiguous(Sk=1024, strides=st, ns=2, ws=None) == want, (stride, i)
    # paged: pageSize x row stride x 1 byte < 2^31
    assert paged(page=1 << 24, maxp=1, ts=1, ns=2, ws=None) == BAD_SHAPE      # 2^24 rows of 128 bytes: 2^31
    assert paged(page=1 << 23, maxp=2, ts=2, ns=2, ws=None) == NULL_POINTER   # 2^30 bytes a page (bf16: 2^31, refused)
    wide = fa.FaStrides(1 << 40, 128, 1 << 25)     # 64 rows x 2^25 bytes = 2^31
    fits = fa.FaStrides(1 << 40, 128, 1 << 24)     # 64 rows x 2^24 bytes = 2^30 (bf16: 2^31, refused)
    for i in (1, 2):
        st = [None] * 4
        st[i] = ctypes.byref(wide)
        assert paged(strides=st, ns=2, ws=None) == BAD_SHAPE, i
        st[i] = ctypes.byref(fits)
        assert paged(strides=st, ns=2, ws=None) == NULL_POINTER, i
    far = fa.FaStrides(1 << 40, 1 << 30, 128)      # page and head strides far beyond 2^32 bytes: page bases are 64-bit
    assert paged(strides=[None, ctypes.byref(far), ctypes.byref(far), None], ns=2, ws=None) == NULL_POINTER


def test_the_plan_does_not_depend_on_the_cache_type():
    # there is one plan function and it takes no cache type: where it says more than one split, the fp8 calls ask for the workspace,
    # and the workspace size is the bf16 call's
    contiguous, paged, p = calls()
    for page, maxp in ((16, 2048), (128, 256), (256, 16), (1024, 64)):
        plan = fa.decode_plan(2, 8, 2, 1, page * maxp, 128, F32)
        assert plan["num_splits"] > 1 and plan == fa.decode_plan(2, 8, 2, 1, page * maxp, 128, F32, 0)
        assert paged(page=page, maxp=maxp, ts=maxp, ns=0, ws=None) == NULL_POINTER, (page, maxp)
        assert contiguous(Sk=page * maxp, ns=0, ws=None) == NULL_POINTER, (page, maxp)
    assert fa.decode_plan(2, 8, 2, 1, 1024, 128, F32, 1)["lds_bytes"] == 37376      # the bf16 V image, whatever the cache holds
    assert "kv_dtype" not in declared_parameters("flash_attention_decode_plan")


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    f8 = torch.float8_e4m3fn
    q = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16)
    k, k8 = torch.zeros(2, 2, 32, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 32, 64, dtype=f8)
    pool, pool8 = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16), torch.zeros(6, 2, 16, 64, dtype=f8)
    table = torch.zeros(2, 3, dtype=torch.int32)
    ones = torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_decode(q, k8, k8, k_descale=ones, v_descale=ones)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_decode_paged(q, pool8, pool8, table, k_descale=ones, v_descale=ones)

    def both(Q, K, V, Kp, Vp, **kw):
        yield lambda: fa.flash_attention_decode(T(Q), T(K), T(V), **kw)
        yield lambda: fa.flash_attention_decode_paged(T(Q), T(Kp), T(Vp), T(table), **kw)

    # every dtype mismatch but (bf16 Q, fp8 K, fp8 V) is still "share a dtype": fp8 Q, float K under a bf16 Q, one fp8 tensor of two
    # (an fp8 Q with fp8 K/V shares a dtype: that call reaches the library, which refuses dtype != BF16 -- test_the_new_refusals)
    for Q, K, V, Kp, Vp in ((q.to(f8), k, k, pool, pool), (q, k.float(), k.float(), pool.float(), pool.float()),
                            (q, k8, k, pool8, pool), (q, k, k8, pool, pool8), (q.half(), k8, k8, pool8, pool8), (q.float(), k8, k8, pool8, pool8)):
        for call in both(Q, K, V, Kp, Vp):
            with pytest.raises(TypeError, match="share a dtype"):
                call()
    # descales belong to an fp8 cache
    for kw in (dict(k_descale=T(ones)), dict(v_descale=T(ones)), dict(k_descale=T(ones), v_descale=T(ones))):
        for call in both(q, k, k, pool, pool, **kw):
            with pytest.raises(ValueError, match="descale"):
                call()
    # ... and are dense fp32 [Hkv] on the device of Q (good ones pass: the next check speaks)
    for call in both(q, k8, k8, pool8, pool8, k_descale=T(ones), v_descale=T(ones), kv_lens=T(torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError, match="kv_lens"):
            call()
    for bad in (T(ones.double()), T(ones.half()), T(torch.ones(3)), T(torch.ones(2, 1)), T(torch.ones(4)[::2]), T(torch.ones(())),
                T(ones, device="cpu"), ones, [1.0, 1.0], 1.0):
        for name in ("k_descale", "v_descale"):
            for call in both(q, k8, k8, pool8, pool8, **{name: bad}):
                with pytest.raises(ValueError, match=name):
                    call()
