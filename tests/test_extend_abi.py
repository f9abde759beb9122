"""CPU tests of the chunked-prefill entry points (flash_attention_extend, flash_attention_extend_paged, flash_attention_extend_plan) at
the C ABI and in the binding: the symbols exist with the declared parameter lists and argtypes, every invalid argument is refused with
its code before anything is launched (fake aligned host pointers: no GPU is touched; no call here is valid as a whole), and the plan
is the documented one."""
import ctypes
import functools

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, TILE, MetaTensor as T, declared_parameters, host_calls, plan_call)


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    # the _fp8 decode siblings' lists, word for word
    for name, sibling in (("flash_attention_extend", "flash_attention_decode_fp8"),
                          ("flash_attention_extend_paged", "flash_attention_decode_paged_fp8"),
                          ("flash_attention_extend_plan", "flash_attention_decode_plan")):
        assert name in fa.EXPORTS and getattr(L, name) is not None
        assert declared_parameters(name) == declared_parameters(sibling), name
        assert list(getattr(L, name).argtypes) == list(getattr(L, sibling).argtypes), name
        assert getattr(L, name).restype is ctypes.c_int
    assert declared_parameters("flash_attention_extend_plan") == ["batchSize", "numHeads", "numHeadsKV", "seqLenQ", "seqLenK", "dHead",
                                                                  "o_dtype", "numSplits", "plan"]


def calls(kv):
    """(contiguous call, paged call, an aligned host pointer) for a cache of type `kv`; keyword arguments override a call that is
    valid but for its workspace: two splits and none given, so that a call that passes every other check stops at NULL_POINTER"""
    okc = dict(B=2, H=8, Hkv=2, Sq=300, Sk=1024, d=128, scale=0.125, causal=True, dtype=BF16, kv=kv, o=F32, ns=2)
    okp = dict(B=2, H=8, Hkv=2, Sq=300, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=True, dtype=BF16, kv=kv, o=F32, ns=2)
    return host_calls(("flash_attention_extend", okc), ("flash_attention_extend_paged", okp))


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_what_the_decode_siblings_refuse_is_refused_with_the_same_codes(kv):
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    contiguous, paged, p = calls(kv)
    for call in (contiguous, paged):
        assert call() == NULL_POINTER        # valid but for the workspace of its two splits
        for name in ("Q", "K", "V", "O"):
            assert call(**{name: None}) == NULL_POINTER, name
            assert call(**{name: p + 8}) == MISALIGNED, name
        assert call(LSE=p + 4) == MISALIGNED and call(ws=p + 8) == MISALIGNED and call(lens=p + 2) == MISALIGNED
        for kw in (dict(Sq=0), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0), dict(Hkv=16),
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
        # descales: those of an fp8 cache, 4-byte aligned; a bf16 cache has none
        for kw in (dict(kd=p), dict(vd=p + 8), dict(kd=p + 4, vd=p + 12)):
            assert call(**kw) == (NULL_POINTER if kv == FP8 else BAD_DTYPE), kw
        if kv == FP8:
            for name in ("kd", "vd"):
                for off in (1, 2, 3, 6):
                    assert call(**{name: p + off}) == MISALIGNED, (name, off)
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
    # the extent limit of the cache's type: (seqLenK + 192) x row stride in BYTES below 2^31
    big = (1 << 24) - 193
    assert contiguous(Sk=big) == (NULL_POINTER if kv == FP8 else BAD_SHAPE)
    assert contiguous(Sk=1 << 24) == BAD_SHAPE


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_chunk_is_capped_by_the_capacity_not_by_decodes_sixteen(kv):
    contiguous, paged, p = calls(kv)
    for Sq in (1, 16, 17, 300, 1023, 1024):      # up to the capacity: on to the workspace check
        assert contiguous(Sq=Sq) == NULL_POINTER and paged(Sq=Sq) == NULL_POINTER, Sq
    for Sq in (1025, 5000, (1 << 31) - 1):
        assert contiguous(Sq=Sq, ws=p) == BAD_SHAPE and paged(Sq=Sq, ws=p) == BAD_SHAPE, Sq
    assert paged(Sq=32, page=16, maxp=2, ts=2) == NULL_POINTER and paged(Sq=33, page=16, maxp=2, ts=2, ws=p) == BAD_SHAPE
    # batchSize * numHeads * seqLenQ must fit in an int32
    assert contiguous(B=1 << 12, H=1 << 4, Hkv=1 << 4, Sq=1 << 15, Sk=1 << 15, ws=p) == BAD_SHAPE
    # the library's own split count: a short chunk on a long cache plans more than one split and the workspace is missing
    assert fa.extend_plan(2, 8, 2, 17, 32768, 128, F32)["num_splits"] > 1
    assert contiguous(ns=0, Sq=17, Sk=32768) == NULL_POINTER and paged(ns=0, Sq=17, maxp=512, ts=512) == NULL_POINTER


plan = functools.partial(plan_call, "flash_attention_extend_plan")


def test_the_plan():
    shapes = [(1, 32, 8, 512, 8192 + 512, 128), (1, 32, 8, 512, 32768 + 512, 64), (1, 32, 8, 2048, 2048, 128), (1, 32, 8, 64, 32768, 128),
              (8, 32, 8, 300, 4096, 128), (2, 8, 8, 17, 17, 64), (3, 16, 1, 5, 4096, 128), (2, 8, 2, 16, 640, 64), (1, 4, 2, 33, 100, 128),
              (64, 32, 8, 1, 8192, 128)]
    for B, H, Hkv, Sq, Sk, d in shapes:
        rc, p = plan(B, H, Hkv, Sq, Sk, d)
        assert rc == 0 and p == fa.extend_plan(B, H, Hkv, Sq, Sk, d, F32)
        rpb, ns, G = p["rows_per_block"], p["num_splits"], H // Hkv
        assert rpb % 16 == 0 and rpb >= 16
        assert p["row_blocks"] == -(-G * Sq // rpb)               # row blocks are not head-aligned
        assert 1 <= ns <= min(CAP, max(1, -(-Sk // TILE)))
        assert p["grid"] == B * Hkv * p["row_blocks"] * ns
        assert (p["combine_grid"], p["combine_threads"]) == ((B * H * Sq, 256) if ns > 1 else (0, 0))
        dec = fa.decode_plan(B, H, Hkv, 1, Sk, d, F32)
        for k in ("kv_block_rows", "threads", "lds_bytes"):
            assert p[k] == dec[k], k
        assert p["kv_block_rows"] == TILE
        for forced in (1, 2, 3, 5, 8, CAP):                       # forced split counts are honoured
            rc, f = plan(B, H, Hkv, Sq, Sk, d, F32, forced)
            assert rc == 0 and f["num_splits"] == forced and f["grid"] == B * Hkv * p["row_blocks"] * forced
            assert f["combine_grid"] == (B * H * Sq if forced > 1 else 0)
    # a long chunk fills the chip with its units alone; a short one on a long cache is split
    assert fa.extend_plan(1, 32, 8, 2048, 2048, 128, F32)["num_splits"] == 1
    assert fa.extend_plan(8, 32, 8, 512, 8704, 128, F32)["num_splits"] == 1
    assert fa.extend_plan(1, 8, 8, 17, 32768, 128, F32)["num_splits"] > 1
    # seqLenQ = 17 and seqLenQ = capacity are accepted, capacity + 1 is not; the decode plan still stops at 16
    assert plan(1, 32, 8, 17, 1024, 128)[0] == 0 and plan(1, 32, 8, 1024, 1024, 128)[0] == 0
    assert plan(1, 32, 8, 1025, 1024, 128)[0] == BAD_SHAPE
    assert plan_call("flash_attention_decode_plan", 1, 32, 8, 17, 1024, 128, F32, 0)[0] == BAD_SHAPE
    assert plan(1, 32, 8, 0, 1024, 128)[0] == BAD_SHAPE and plan(1, 32, 3, 20, 1024, 128)[0] == BAD_SHAPE
    assert plan(1, 32, 8, 20, 1024, 128, ns=-1)[0] == BAD_SHAPE and plan(1, 32, 8, 20, 1024, 128, ns=CAP + 1)[0] == BAD_SHAPE
    assert plan(1, 32, 8, 20, 1024, 96)[0] == BAD_DHEAD
    assert plan(1, 32, 8, 20, 1024, 128, FP8)[0] == BAD_DTYPE
    assert plan(1, 32, 8, 20, 1024, 128, F32, 0, null_plan=True)[0] == NULL_POINTER


def test_a_launch_stays_below_2_pow_32_threads():
    """FA_DECODE_MAX_WORKGROUPS: the combine kernel runs one 256-thread workgroup per row of O, and the runtime refuses a launch of 2^32
    threads after the split kernel has run (tests/test_long_cache.py met that at B H Sq = 2^24).  The plan and the call refuse it first"""
    M = fa.FA_DECODE_MAX_WORKGROUPS
    assert M == 1 << 24
    B, H, Hkv, Sq, Sk, d = 2048, 8, 2, 1024, 1024, 64
    assert B * H * Sq == M
    for ns in (2, 3, CAP):
        assert plan(B, H, Hkv, Sq, Sk, d, BF16, ns)[0] == BAD_SHAPE
    for ns in (0, 1):                                             # one split has no combine launch; the library's choice at this size is one
        rc, p = plan(B, H, Hkv, Sq, Sk, d, BF16, ns)
        assert rc == 0 and p["num_splits"] == 1 and p["combine_grid"] == 0 and p["grid"] < M
    rc, p = plan(B - 1, H, Hkv, Sq, Sk, d, BF16, 2)
    assert rc == 0 and p["combine_grid"] == (B - 1) * H * Sq == M - H * Sq
    # the split kernel's own grid: units * splits
    units = (B - 1) * Hkv * p["row_blocks"]
    ok, over = (M - 1) // units, -(-M // units)
    assert 1 < ok < over <= CAP
    rc, p = plan(B - 1, H, Hkv, Sq, Sk, d, BF16, ok)
    assert rc == 0 and p["grid"] == units * ok < M
    assert plan(B - 1, H, Hkv, Sq, Sk, d, BF16, over)[0] == BAD_SHAPE
    # the same from the calls (fake pointers: a call that passes every check stops at its missing workspace), and from the ragged plan
    contiguous, paged, _ = calls(BF16)
    big = dict(B=B, H=H, Hkv=Hkv, Sq=Sq, d=d)
    assert contiguous(Sk=Sk, **big) == BAD_SHAPE and paged(P=64, page=64, maxp=16, ts=16, **big) == BAD_SHAPE
    assert contiguous(Sk=Sk, **dict(big, B=B - 1)) == NULL_POINTER and paged(P=64, page=64, maxp=16, ts=16, **dict(big, B=B - 1)) == NULL_POINTER
    with pytest.raises(fa.FlashAttentionError) as e:
        fa.extend_varlen_plan(4, H, Hkv, M // H, Sk, d, BF16, 2)
    assert e.value.code == BAD_SHAPE
    assert fa.extend_varlen_plan(4, H, Hkv, M // H - 1, Sk, d, BF16, 2)["combine_grid"] == M - H
    assert fa.extend_varlen_plan(4, H, Hkv, M // H, Sk, d, BF16, 0)["num_splits"] == 1


def test_the_workspace_formula_has_no_cap_on_the_chunk():
    """partial O [ns][rows][d] fp32, then partial LSE [ns][rows] fp32, each rounded up to 16 bytes; nothing for one split"""
    r16 = lambda n: (n + 15) & ~15
    for B, H, Sq, d, ns in ((1, 32, 300, 128, 2), (3, 5, 300, 64, 7), (2, 8, 300, 128, CAP), (1, 1, 300, 64, 3)):
        rows = B * H * Sq
        assert fa.decode_workspace_size(B, H, Sq, d, ns) == r16(rows * ns * d * 4) + r16(rows * ns * 4)
    assert fa.decode_workspace_size(1, 32, 300, 128, 1) == 0 and fa.decode_workspace_size(1, 32, 300, 128, 0) == 0


def test_binding_refusals():
    """the decode fronts' errors, under the extend fronts' names"""
    torch = pytest.importorskip("torch")
    q = torch.zeros(2, 8, 40, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 64, 64, dtype=torch.bfloat16)
    pool = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="flash_attention_extend needs device tensors \\(no CPU fallback\\)"):
        fa.flash_attention_extend(q, k, k)
    with pytest.raises(RuntimeError, match="flash_attention_extend_paged needs device tensors \\(no CPU fallback\\)"):
        fa.flash_attention_extend_paged(q, pool, pool, table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_extend_paged(T(q), T(pool), T(pool), table)      # a host table under device tensors
    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_extend(T(q), T(torch.zeros(2, 3, 64, 64, dtype=torch.bfloat16)), T(torch.zeros(2, 3, 64, 64, dtype=torch.bfloat16)))
    with pytest.raises(TypeError, match="share a dtype"):
        fa.flash_attention_extend(T(q), T(k.float()), T(k.float()))
    ones = torch.ones(2)
    with pytest.raises(ValueError, match="descale"):
        fa.flash_attention_extend(T(q), T(k), T(k), k_descale=T(ones))
    with pytest.raises(ValueError, match="descale"):
        fa.flash_attention_extend_paged(T(q), T(pool), T(pool), T(table), v_descale=T(ones))
    for bad in (table.long(), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, 6, dtype=torch.int32)[:, ::2], torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="block_table must be an int32 device tensor"):
            fa.flash_attention_extend_paged(T(q), T(pool), T(pool), T(bad))
    with pytest.raises(ValueError, match="kv_lens must be a dense int32 device tensor"):
        fa.flash_attention_extend(T(q), T(k), T(k), kv_lens=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="window"):
        fa.flash_attention_extend(T(q), T(k), T(k), window=16)              # not in this call
    # the decode front still stops at 16 rows, with its own code
    assert fa.FA_DECODE_MAX_Q == 16
