"""CPU tests of flash_attention_decode_paged (split-KV decode against paged K/V caches) at the C ABI and in the binding: the symbol
exists with the declared parameter list and argtypes, every invalid argument is refused with its code before anything is launched
(fake aligned host pointers: no GPU is touched), and the binding refuses host tensors and mismatched shapes."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, declared_parameters, host_call)


def test_the_symbol_is_exported_with_the_declared_signature():
    L = fa.lib()
    assert "flash_attention_decode_paged" in fa.EXPORTS and L.flash_attention_decode_paged is not None
    assert declared_parameters("flash_attention_decode_paged") == [
        "Q", "Kpool", "Vpool", "O", "LSE", "kvLens", "blockTable", "workspace", "batchSize", "numHeads", "numHeadsKV", "seqLenQ",
        "numPages", "pageSize", "maxPagesPerSeq", "tableStride", "dHead", "scale", "is_causal", "dtype", "o_dtype", "numSplits",
        "sQ", "sK", "sV", "sO", "stream"]
    sp, vp, i = ctypes.POINTER(fa.FaStrides), ctypes.c_void_p, ctypes.c_int
    assert list(L.flash_attention_decode_paged.argtypes) == \
        [vp] * 8 + [i] * 7 + [ctypes.c_int64, i, ctypes.c_float, ctypes.c_bool, i, i, i] + [sp] * 4 + [vp]
    assert len(L.flash_attention_decode_paged.argtypes) == len(declared_parameters("flash_attention_decode_paged"))
    assert L.flash_attention_decode_paged.restype is i
    assert callable(fa.flash_attention_decode_paged)


def paged_call():
    ok = dict(B=2, H=8, Hkv=2, Sq=1, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=False, dtype=BF16, o=F32, ns=1)
    return host_call("flash_attention_decode_paged", ok)


def test_what_flash_attention_decode_refuses_is_refused_with_the_same_codes():
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    call, p = paged_call()
    for name in ("Q", "K", "V", "O"):
        assert call(**{name: None}) == NULL_POINTER, name
        assert call(**{name: p + 8}) == MISALIGNED, name
    assert call(LSE=p + 4) == MISALIGNED and call(ws=p + 8, ns=2) == MISALIGNED and call(lens=p + 2) == MISALIGNED
    assert call(ns=2, ws=None) == NULL_POINTER
    assert call(ns=0, ws=None, maxp=512, ts=512) == NULL_POINTER     # (0: the library plans > 1 split for a capacity of 32 768)
    for kw in (dict(Sq=0), dict(Sq=17), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0), dict(Hkv=16),
               dict(Hkv=-2), dict(ns=-1), dict(ns=CAP + 1)):
        assert call(ws=p, **kw) == BAD_SHAPE, kw
    for kw in (dict(dtype=F32), dict(dtype=FP8), dict(dtype=F16), dict(dtype=9), dict(o=FP8), dict(o=7)):
        assert call(**kw) == BAD_DTYPE, kw
    for d in (96, 32, 256, 120):
        assert call(d=d) == BAD_DHEAD, d
    for s in (0.0, -0.5, float("nan"), float("inf")):
        assert call(scale=s) == BAD_SCALE, s
    bad = fa.FaStrides(64, 16, 8)            # strideS < d
    mis = fa.FaStrides(1024, 66, 66)         # d = 64: 132-byte bf16 rows, 264-byte fp32 rows: not multiples of 16 bytes
    for i in range(4):
        for s in (bad, mis):
            st = [None] * 4
            st[i] = ctypes.byref(s)
            assert call(strides=st, d=64) == BAD_STRIDE, i


def test_the_paged_refusals():
    call, p = paged_call()
    assert call(table=None) == NULL_POINTER
    assert call(table=p + 2) == MISALIGNED and call(table=p + 1) == MISALIGNED
    assert call(table=p + 4, ns=2, ws=None) == NULL_POINTER   # 4-byte alignment is enough: on to the workspace two splits need
    for kw in (dict(P=0), dict(P=-1), dict(maxp=0, ts=16), dict(maxp=-3), dict(page=8), dict(page=0), dict(page=-16), dict(page=1),
               dict(page=24), dict(page=48), dict(page=100), dict(page=(1 << 20) + 16),
               dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21),        # capacity 2^24 + 16
               dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),         # capacity 2^32: no 32-bit wrap-around
               dict(page=1 << 30, maxp=4, ts=4),
               dict(ts=15), dict(ts=0), dict(ts=-16)):
        assert call(ws=p, **kw) == BAD_SHAPE, kw
    # one page's head extent (pageSize x row stride): 2^31 bytes and more is refused, for K and for V; the page stride is free
    wide = fa.FaStrides(1 << 40, 128, 1 << 24)     # 64 rows x 2^25 bytes
    for i in (1, 2):
        st = [None] * 4
        st[i] = ctypes.byref(wide)
        assert call(strides=st) == BAD_SHAPE, i
    # the capacity itself may reach 2^24; a capacity whose contiguous extent would be refused is fine in pages
    # (nothing to launch on: these stop at the NULL workspace that two splits need, after every shape check has passed)
    assert call(page=16, maxp=1 << 20, ts=1 << 20, ns=2, ws=None) == NULL_POINTER
    assert call(page=1 << 23, maxp=2, ts=2, ns=2, ws=None) == BAD_SHAPE     # one 2^23-row page of 256-byte rows is 2^31 bytes
    assert call(page=1 << 22, maxp=4, ts=4, ns=2, ws=None) == NULL_POINTER  # ... 2^30 bytes a page; the capacity is 2^24 keys
    far = fa.FaStrides(1 << 40, 1 << 30, 128)      # page and head strides far beyond 2^32 bytes: page bases are 64-bit
    assert call(strides=[None, ctypes.byref(far), ctypes.byref(far), None], ns=2, ws=None) == NULL_POINTER


def test_the_plan_of_a_paged_call_is_the_plan_of_its_capacity():
    # flash_attention_decode_plan(seqLenK = maxPagesPerSeq * pageSize) describes a paged call: where that plan has more than one
    # split, the call asks for the workspace (a call the plan gives one split would be launched: not made here)
    call, p = paged_call()
    for page, maxp in ((16, 2048), (128, 256), (256, 16), (1024, 64)):
        assert fa.decode_plan(2, 8, 2, 1, page * maxp, 128, F32)["num_splits"] > 1
        assert call(page=page, maxp=maxp, ts=maxp, ns=0, ws=None) == NULL_POINTER, (page, maxp)


def test_binding_refuses_host_tensors_and_bad_shapes():
    torch = pytest.importorskip("torch")
    q, k = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16), torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_decode_paged(q, k, k, table)

    class T:
        is_cuda = True

        def __init__(self, t):
            self.shape, self.dtype, self.dim, self.stride = t.shape, t.dtype, t.dim, t.stride

    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_decode_paged(T(q), T(torch.zeros(6, 3, 16, 64)), T(torch.zeros(6, 3, 16, 64)), T(table))
    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_decode_paged(T(q), T(k), T(torch.zeros(6, 2, 32, 64)), T(table))           # K and V pools differ
    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_decode_paged(T(q), T(torch.zeros(6, 2, 16, 128)), T(torch.zeros(6, 2, 16, 128)), T(table))   # d differs
    with pytest.raises(TypeError, match="share a dtype"):
        fa.flash_attention_decode_paged(T(q), T(k.float()), T(k.float()), T(table))
    for bad in (table.long(), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                torch.zeros(3, 2, dtype=torch.int32).t(), torch.zeros(2, 0, dtype=torch.int32)):
        with pytest.raises(ValueError, match="block_table"):
            fa.flash_attention_decode_paged(T(q), T(k), T(k), T(bad))
