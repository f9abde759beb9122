"""CPU tests of the split-KV decode entry points of the C ABI (flash_attention_decode, _decode_plan, _decode_workspace_size): the
symbols exist with the declared signatures, every invalid argument is refused with its code before anything is launched (fake
aligned host pointers: no GPU is touched), and the plan and the workspace size are what the header says (host logic only)."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, declared_parameters, host_call)

CUS_WITHOUT_A_DEVICE = 256


def test_decode_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    names = ("flash_attention_decode", "flash_attention_decode_plan", "flash_attention_decode_workspace_size")
    for n in names:
        assert n in fa.EXPORTS and getattr(L, n) is not None
    assert declared_parameters("flash_attention_decode") == [
        "Q", "K", "V", "O", "LSE", "kvLens", "workspace", "batchSize", "numHeads", "numHeadsKV", "seqLenQ", "seqLenK", "dHead", "scale",
        "is_causal", "dtype", "o_dtype", "numSplits", "sQ", "sK", "sV", "sO", "stream"]
    assert declared_parameters("flash_attention_decode_plan") == [
        "batchSize", "numHeads", "numHeadsKV", "seqLenQ", "seqLenK", "dHead", "o_dtype", "numSplits", "plan"]
    assert declared_parameters("flash_attention_decode_workspace_size") == ["batchSize", "numHeads", "seqLenQ", "dHead", "numSplits"]
    for n in names:
        assert len(getattr(L, n).argtypes) == len(declared_parameters(n))
    sp, vp, i = ctypes.POINTER(fa.FaStrides), ctypes.c_void_p, ctypes.c_int
    assert list(L.flash_attention_decode.argtypes) == [vp] * 7 + [i] * 6 + [ctypes.c_float, ctypes.c_bool, i, i, i] + [sp] * 4 + [vp]
    assert L.flash_attention_decode.restype is i and L.flash_attention_decode_plan.restype is i
    assert L.flash_attention_decode_workspace_size.restype is ctypes.c_size_t
    assert [k for k, _ in fa.FaDecodePlan._fields_] == ["num_splits", "row_blocks", "rows_per_block", "kv_block_rows", "threads", "grid",
                                                        "lds_bytes", "combine_grid", "combine_threads"]
    assert fa.FA_DECODE_MAX_Q == 16


def decode_call():
    return host_call("flash_attention_decode", dict(B=2, H=8, Hkv=2, Sq=1, Sk=4096, d=128, scale=0.125, causal=False, dtype=BF16, o=F32, ns=1))


def test_every_invalid_argument_is_refused_before_any_launch():
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    call, p = decode_call()
    for name in ("Q", "K", "V", "O"):
        assert call(**{name: None}) == NULL_POINTER, name
        assert call(**{name: p + 8}) == MISALIGNED, name
    assert call(LSE=p + 4) == MISALIGNED and call(ws=p + 8, ns=2) == MISALIGNED and call(lens=p + 2) == MISALIGNED
    assert call(ns=2, ws=None) == NULL_POINTER and call(ns=0, ws=None) == NULL_POINTER     # (0: the library plans > 1 split here)
    for kw in (dict(Sq=0), dict(Sq=17), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(Sk=0), dict(Sk=(1 << 24) + 1), dict(d=0),
               dict(Hkv=3), dict(Hkv=0), dict(Hkv=16), dict(Hkv=-2), dict(ns=-1), dict(ns=CAP + 1), dict(Sk=1 << 23)):
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
    # one K/V head's extent through a strided view: 2^31 bytes and more is refused
    wide = fa.FaStrides(1 << 40, 128, 1 << 20)
    st = [None, ctypes.byref(wide), None, None]
    assert call(strides=st) == BAD_SHAPE


def test_the_plan():
    # forced split counts are returned as given
    for ns in (1, 2, 3, 16, CAP):
        pl = fa.decode_plan(1, 32, 8, 1, 32768, 128, BF16, ns)
        assert pl["num_splits"] == ns and pl["grid"] == 8 * ns
        assert (pl["combine_grid"] == 0 and pl["combine_threads"] == 0) if ns == 1 else (pl["combine_grid"] > 0 and pl["combine_threads"] > 0)
    with pytest.raises(fa.FlashAttentionError):
        fa.decode_plan(1, 32, 8, 1, 32768, 128, BF16, CAP + 1)
    with pytest.raises(fa.FlashAttentionError):
        fa.decode_plan(1, 32, 8, 1, 32768, 128, BF16, -1)
    with pytest.raises(fa.FlashAttentionError):
        fa.decode_plan(1, 32, 8, 17, 32768, 128)
    with pytest.raises(fa.FlashAttentionError):
        fa.decode_plan(1, 32, 8, 1, 32768, 96)
    # the library's choice: at least one split, never more than the capacity has key tiles, one split = one launch
    for (B, H, Hkv, Sq, Sk, d) in [(1, 32, 8, 1, 32768, 128), (1, 32, 8, 1, 131072, 128), (8, 32, 8, 1, 8192, 128), (64, 64, 8, 1, 4096, 128),
                                   (4, 32, 32, 1, 16384, 128), (8, 32, 8, 4, 32768, 128), (8, 32, 8, 1, 16384, 64), (1, 8, 8, 1, 1, 64),
                                   (1, 8, 1, 16, 64, 64), (2, 16, 2, 5, 129, 128), (1, 1, 1, 1, 300, 128), (512, 64, 8, 1, 2048, 128)]:
        pl = fa.decode_plan(B, H, Hkv, Sq, Sk, d)
        tiles = -(-Sk // pl["kv_block_rows"])
        assert 1 <= pl["num_splits"] <= min(tiles, CAP), (B, H, Hkv, Sq, Sk, d, pl)
        assert (pl["combine_grid"] == 0) == (pl["num_splits"] == 1)
        rows = (H // Hkv) * Sq
        assert pl["row_blocks"] == -(-rows // pl["rows_per_block"])
        if rows <= pl["rows_per_block"]:
            assert pl["row_blocks"] == 1                      # the K/V head is read once for the whole group
        assert pl["grid"] == B * Hkv * pl["row_blocks"] * pl["num_splits"] and pl["threads"] == 256 and 0 < pl["lds_bytes"] <= 160 * 1024
    # a single sequence puts the chip to work: at least half the compute units (the prefill route launches 32 workgroups here)
    pl = fa.decode_plan(1, 32, 8, 1, 32768, 128)
    assert pl["grid"] >= CUS_WITHOUT_A_DEVICE // 2


def test_the_workspace_size():
    sizes = [fa.decode_workspace_size(4, 32, 2, 128, ns) for ns in range(0, CAP + 1)]
    assert sizes[0] == 0 and sizes[1] == 0
    assert all(s % 16 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[2] > 0
    rows = 4 * 32 * 2
    assert sizes[8] >= 8 * rows * (128 + 1) * 4               # fp32 partial outputs and log-sum-exps, one slab per split


def test_binding_refuses_host_tensors_and_bad_shapes():
    torch = pytest.importorskip("torch")
    q, k = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 128, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_decode(q, k, k)

    class T:
        is_cuda = True

        def __init__(self, t):
            self.shape, self.dtype, self.dim = t.shape, t.dtype, t.dim

    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_decode(T(q), T(torch.zeros(2, 3, 128, 64)), T(torch.zeros(2, 3, 128, 64)))
