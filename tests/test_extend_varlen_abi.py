"""CPU tests of the ragged entry points (flash_attention_extend_varlen, flash_attention_extend_paged_varlen,
flash_attention_extend_varlen_plan, flash_attention_kv_append_varlen, flash_attention_kv_append_paged_varlen) at the C ABI and in the
binding: the symbols exist with parameter lists that differ from their uniform siblings exactly as declared (seqLenQ / seqLenNew ->
totalQ, cuSeqlensQ before kvLens), every invalid argument is refused with its code before anything is launched (fake aligned host
pointers: no GPU is touched; no call here is valid as a whole), and the plan is the documented one."""
import ctypes
import functools
import random

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, TILE, MetaTensor, declared_parameters, host_calls, plan_call)

MAXB = fa.FA_VARLEN_MAX_BATCH

SIBLINGS = (("flash_attention_extend_varlen", "flash_attention_extend", "seqLenQ"),
            ("flash_attention_extend_paged_varlen", "flash_attention_extend_paged", "seqLenQ"),
            ("flash_attention_kv_append_varlen", "flash_attention_kv_append", "seqLenNew"),
            ("flash_attention_kv_append_paged_varlen", "flash_attention_kv_append_paged", "seqLenNew"))


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    for name, sibling, rows in SIBLINGS:
        assert name in fa.EXPORTS and getattr(L, name) is not None
        want = declared_parameters(sibling)
        want[want.index(rows)] = "totalQ"
        want.insert(want.index("kvLens"), "cuSeqlensQ")
        assert declared_parameters(name) == want, name
        types = list(getattr(L, sibling).argtypes)
        types.insert(declared_parameters(sibling).index("kvLens"), ctypes.c_void_p)
        assert list(getattr(L, name).argtypes) == types, name
        assert getattr(L, name).restype is ctypes.c_int
    assert "flash_attention_extend_varlen_plan" in fa.EXPORTS
    assert declared_parameters("flash_attention_extend_varlen_plan") == ["batchSize", "numHeads", "numHeadsKV", "totalQ", "seqLenK", "dHead",
                                                                         "o_dtype", "numSplits", "plan"]
    assert list(L.flash_attention_extend_varlen_plan.argtypes) == list(L.flash_attention_extend_plan.argtypes)
    text = open(entry.ROOT + "/include/flash_attention.h").read()
    assert "#define FA_VARLEN_MAX_BATCH %d" % MAXB in text and MAXB >= 1024


def calls(kv):
    """(contiguous call, paged call, an aligned host pointer) for a cache of type `kv`; keyword arguments override a call that is
    valid but for its workspace: two splits and none given, so that a call that passes every other check stops at NULL_POINTER"""
    okc = dict(B=2, H=8, Hkv=2, T=300, Sk=1024, d=128, scale=0.125, causal=True, dtype=BF16, kv=kv, o=F32, ns=2)
    okp = dict(B=2, H=8, Hkv=2, T=300, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=True, dtype=BF16, kv=kv, o=F32, ns=2)
    return host_calls(("flash_attention_extend_varlen", okc), ("flash_attention_extend_paged_varlen", okp))


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_what_extend_refuses_is_refused_with_the_same_codes(kv):
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    contiguous, paged, p = calls(kv)
    for call in (contiguous, paged):
        assert call() == NULL_POINTER        # valid but for the workspace of its two splits
        for name in ("Q", "K", "V", "O", "cu"):
            assert call(**{name: None}) == NULL_POINTER, name
        for name in ("Q", "K", "V", "O"):
            assert call(**{name: p + 8}) == MISALIGNED, name
        for off in (1, 2, 3, 6):
            assert call(cu=p + off) == MISALIGNED, off
        assert call(cu=p + 4) == NULL_POINTER                 # 4-byte alignment is enough: on to the workspace check
        assert call(LSE=p + 4) == MISALIGNED and call(ws=p + 8) == MISALIGNED and call(lens=p + 2) == MISALIGNED
        for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0), dict(Hkv=16),
                   dict(Hkv=-2), dict(ns=-1), dict(ns=CAP + 1), dict(B=MAXB + 1), dict(B=1 << 20)):
            assert call(ws=p, **kw) == BAD_SHAPE, kw
        assert call(B=MAXB) == NULL_POINTER
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
        # strideB of Q and O is ignored, whatever it holds; of K and V it is the batch / page stride and is checked
        odd = fa.FaStrides(-7, 64, 512)
        for i, want in ((0, NULL_POINTER), (3, NULL_POINTER), (1, BAD_STRIDE), (2, BAD_STRIDE)):
            st = [None] * 4
            st[i] = ctypes.byref(odd)
            assert call(strides=st, d=64) == want, i
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
               dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21), dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),
               dict(page=1 << 30, maxp=4, ts=4), dict(ts=15), dict(ts=0), dict(ts=-16)):
        assert paged(ws=p, **kw) == BAD_SHAPE, kw
    big = (1 << 24) - 193
    assert contiguous(Sk=big) == (NULL_POINTER if kv == FP8 else BAD_SHAPE)
    assert contiguous(Sk=1 << 24) == BAD_SHAPE


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_total_q_is_a_bound_of_its_own_not_capped_by_the_capacity(kv):
    contiguous, paged, p = calls(kv)
    for T in (1, 16, 17, 300, 1024, 1025, 5000, 100000):      # above the capacity too: on to the workspace check
        assert contiguous(T=T) == NULL_POINTER and paged(T=T) == NULL_POINTER, T
    assert paged(T=33, page=16, maxp=2, ts=2) == NULL_POINTER
    # numHeads * totalQ must fit in an int32 (whatever the batch), and so must the grid
    assert contiguous(H=16, Hkv=16, T=1 << 27, ws=p) == BAD_SHAPE
    assert contiguous(H=16, Hkv=16, T=1 << 26, d=64, ns=CAP, ws=p) == BAD_SHAPE       # (the grid: 16 * (2^21 + 1) * 64 > 2^31 - 1)
    # ... and a launch holds fewer than 2^32 threads, FA_DECODE_MAX_WORKGROUPS = 2^24 workgroups of 256 (a launch of more is refused by
    # the runtime, after the split kernel has run: tests/test_long_cache.py): the rows of O under more than one split -- the combine
    # kernel's workgroups -- and the split kernel's grid under any.  (2^31 - 16 rows, which this test took for accepted, never ran)
    M = fa.FA_DECODE_MAX_WORKGROUPS
    assert contiguous(H=16, Hkv=16, T=(1 << 27) - 1, ws=p) == BAD_SHAPE
    assert contiguous(H=16, Hkv=16, T=M // 16, ws=p) == BAD_SHAPE                      # 2^24 rows under two splits
    assert contiguous(H=16, Hkv=16, T=M // 16 - 1) == NULL_POINTER                     # 2^24 - 16 rows: on to the workspace check
    assert plan(2, 16, 16, M // 16, 1024, 128, ns=1)[0] == 0                           # one split has no combine launch
    # the grid: d = 64 has 32-row blocks, NB = 2^14 + 1, 16 * NB * 64 >= 2^24; with 32 splits it fits
    assert contiguous(H=16, Hkv=16, T=1 << 19, d=64, ns=CAP, ws=p) == BAD_SHAPE
    assert contiguous(H=16, Hkv=16, T=1 << 19, d=64, ns=32) == NULL_POINTER
    # the library's own split count: a few rows on a long cache plan more than one split and the workspace is missing
    assert fa.extend_varlen_plan(2, 8, 2, 17, 32768, 128, F32)["num_splits"] > 1
    assert contiguous(ns=0, T=17, Sk=32768) == NULL_POINTER and paged(ns=0, T=17, maxp=512, ts=512) == NULL_POINTER


plan = functools.partial(plan_call, "flash_attention_extend_varlen_plan")


def test_the_plan():
    shapes = [(64, 32, 8, 575, 32768, 128), (64, 32, 8, 575, 32768, 64), (8, 32, 8, 4000, 32768, 128), (8, 32, 8, 4096, 8704, 64),
              (64, 32, 8, 64, 16384, 128), (1, 8, 8, 17, 17, 64), (3, 16, 1, 5, 4096, 128), (130, 8, 2, 400, 640, 64), (1, 4, 2, 33, 100, 128),
              (MAXB, 32, 8, MAXB, 8192, 128), (10, 8, 2, 5000, 1024, 128)]
    for B, H, Hkv, T, Sk, d in shapes:
        rc, p = plan(B, H, Hkv, T, Sk, d)
        assert rc == 0 and p == fa.extend_varlen_plan(B, H, Hkv, T, Sk, d, F32)
        rpb, ns, G = p["rows_per_block"], p["num_splits"], H // Hkv
        assert rpb == fa.extend_plan(1, H, Hkv, 1, Sk, d, F32)["rows_per_block"]      # extend's
        NB = (G * T + B * (rpb - 1)) // rpb                                            # the bound over the whole batch
        assert p["row_blocks"] == NB
        assert 1 <= ns <= min(CAP, max(1, -(-Sk // TILE)))
        assert p["grid"] == Hkv * NB * ns
        assert (p["combine_grid"], p["combine_threads"]) == ((H * T, 256) if ns > 1 else (0, 0))
        dec = fa.decode_plan(1, H, Hkv, 1, Sk, d, F32)
        for k in ("kv_block_rows", "threads", "lds_bytes"):
            assert p[k] == dec[k], k
        for forced in (1, 2, 3, 5, 8, CAP):                       # forced split counts are honoured
            rc, f = plan(B, H, Hkv, T, Sk, d, F32, forced)
            assert rc == 0 and f["num_splits"] == forced and f["grid"] == Hkv * NB * forced
            assert f["combine_grid"] == (H * T if forced > 1 else 0)
    # numSplits = 0 is extend's rule with units = Hkv * NB: one ragged sequence of B * Sq rows has the units of a uniform batch of
    # B chunks of Sq rows (G * Sq a multiple of the row block: NB = B * row_blocks), and gets the split count extend gives that batch
    for B, Sq, Sk, d in ((8, 512, 8704, 128), (1, 64, 32768, 128), (1, 64, 32768, 64), (4, 128, 16384, 64)):
        u = fa.extend_plan(B, 32, 8, Sq, Sk, d, F32)
        assert (4 * Sq) % u["rows_per_block"] == 0
        v = fa.extend_varlen_plan(1, 32, 8, B * Sq, Sk, d, F32)
        assert v["row_blocks"] == B * u["row_blocks"] and v["num_splits"] == u["num_splits"], (B, Sq, Sk, d)
    assert plan(1, 32, 8, 0, 1024, 128)[0] == BAD_SHAPE and plan(1, 32, 3, 20, 1024, 128)[0] == BAD_SHAPE
    assert plan(MAXB + 1, 32, 8, 20, 1024, 128)[0] == BAD_SHAPE and plan(MAXB, 32, 8, 20, 1024, 128)[0] == 0
    assert plan(1, 32, 8, 5000, 1024, 128)[0] == 0                # above the capacity
    assert plan(1, 32, 8, 20, 1024, 128, ns=-1)[0] == BAD_SHAPE and plan(1, 32, 8, 20, 1024, 128, ns=CAP + 1)[0] == BAD_SHAPE
    assert plan(1, 32, 8, 20, 1024, 96)[0] == BAD_DHEAD
    assert plan(1, 32, 8, 20, 1024, 128, FP8)[0] == BAD_DTYPE
    assert plan(1, 32, 8, 20, 1024, 128, F32, 0, null_plan=True)[0] == NULL_POINTER


def test_the_bound_covers_every_partition():
    """NB >= sum_b ceil(G * sq_b / rows_per_block) by brute force: seeded random partitions of at most totalQ rows over B sequences,
    many of them with most sequences empty"""
    rng = random.Random(2024)
    n = 0
    for rpb in (32, 64):
        for _ in range(2500):
            B = rng.choice((1, 2, 3, 7, 64, 65, 130, 500))
            G = rng.choice((1, 2, 4, 8, 16))
            T = rng.randint(1, 3000)
            used = rng.choice((T, T, rng.randint(0, T)))                       # cu[-1] <= totalQ
            live = B if rng.random() < 0.5 else rng.randint(1, max(1, B // 8))  # ... the others are idle slots
            cuts = sorted(rng.randint(0, used) for _ in range(live - 1))
            sq = [b - a for a, b in zip([0] + cuts, cuts + [used])] + [0] * (B - live)
            rng.shuffle(sq)
            assert sum(sq) == used and len(sq) == B
            NB = (G * T + B * (rpb - 1)) // rpb
            assert NB >= sum(-(-G * s // rpb) for s in sq), (B, G, T, rpb, sq)
            n += 1
    assert n == 5000
    # ... and the library reports exactly that NB
    for B, G, T in ((130, 4, 271), (7, 8, 1), (500, 1, 499)):
        for d, rpb in ((64, fa.extend_plan(1, 8, 8, 1, 128, 64, F32)["rows_per_block"]), (128, fa.extend_plan(1, 8, 8, 1, 128, 128, F32)["rows_per_block"])):
            assert fa.extend_varlen_plan(B, 2 * G, 2, T, 1024, d, F32)["row_blocks"] == (G * T + B * (rpb - 1)) // rpb


def test_the_workspace_formula():
    """flash_attention_decode_workspace_size(1, numHeads, totalQ, dHead, ns), unchanged: partial O [ns][H * T][d] fp32, then partial LSE"""
    r16 = lambda n: (n + 15) & ~15
    for H, T, d, ns in ((32, 575, 128, 2), (5, 300, 64, 7), (8, 4096, 128, CAP), (1, 1, 64, 3)):
        rows = H * T
        assert fa.decode_workspace_size(1, H, T, d, ns) == r16(rows * ns * d * 4) + r16(rows * ns * 4)
    assert fa.decode_workspace_size(1, 32, 575, 128, 1) == 0


def append_calls(kv):
    okc = dict(B=2, Hkv=2, T=300, Sk=1024, d=128, dtype=BF16, kv=kv)
    okp = dict(B=2, Hkv=2, T=300, P=64, page=64, maxp=16, ts=16, d=128, dtype=BF16, kv=kv)
    return host_calls(("flash_attention_kv_append_varlen", okc), ("flash_attention_kv_append_paged_varlen", okp))


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_append_refuses_what_the_uniform_append_refuses(kv):
    """(no call here passes validation: each is stopped by the argument under test; one that passed would try to launch)"""
    contiguous, paged, p = append_calls(kv)
    for call in (contiguous, paged):
        for name in ("Kn", "Vn", "K", "V", "cu"):
            assert call(**{name: None}) == NULL_POINTER, name
        for name in ("Kn", "Vn", "K", "V"):
            assert call(**{name: p + 8}) == MISALIGNED, name
        for off in (1, 2, 3, 6):
            assert call(cu=p + off) == MISALIGNED and call(lens=p + off) == MISALIGNED, off
        for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(Hkv=0), dict(d=0), dict(B=MAXB + 1)):
            assert call(**kw) == BAD_SHAPE, kw
        for kw in (dict(dtype=F32), dict(dtype=FP8), dict(kv=F32), dict(kv=F16), dict(kv=9)):
            assert call(**kw) == BAD_DTYPE, kw
        if kv == BF16:
            assert call(kd=p) == BAD_DTYPE and call(vd=p) == BAD_DTYPE
        else:
            assert call(kd=p + 2) == MISALIGNED and call(vd=p + 1) == MISALIGNED
        for d in (96, 32, 256):
            assert call(d=d) == BAD_DHEAD, d
        bad = fa.FaStrides(64, 16, 8)
        for i in range(4):
            st = [None] * 4
            st[i] = ctypes.byref(bad)
            assert call(strides=st, d=64) == BAD_STRIDE, i
    for kw in (dict(Sk=0), dict(Sk=(1 << 24) + 1)):
        assert contiguous(**kw) == BAD_SHAPE, kw
    assert paged(table=None) == NULL_POINTER and paged(table=p + 2) == MISALIGNED
    for kw in (dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(ts=15), dict(page=1 << 30, maxp=4, ts=4)):
        assert paged(**kw) == BAD_SHAPE, kw
    # totalQ above the capacity passes the shape checks: the next refusal in line is reached (an unsupported dHead)
    assert contiguous(T=5000, d=96) == BAD_DHEAD and paged(T=5000, d=96) == BAD_DHEAD
    assert contiguous(symbol="flash_attention_kv_append", Sq=5000, d=96) == BAD_SHAPE


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    T = MetaTensor
    q = torch.zeros(40, 8, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 64, 64, dtype=torch.bfloat16)
    kn = torch.zeros(40, 2, 64, dtype=torch.bfloat16)
    pool = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    cu = torch.tensor([0, 30, 40], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="flash_attention_extend_varlen needs device tensors \\(no CPU fallback\\)"):
        fa.flash_attention_extend_varlen(q, k, k, cu)
    with pytest.raises(RuntimeError, match="flash_attention_extend_paged_varlen needs device tensors \\(no CPU fallback\\)"):
        fa.flash_attention_extend_paged_varlen(q, pool, pool, table, cu)
    with pytest.raises(RuntimeError, match="kv_cache_append_varlen needs device tensors \\(no CPU fallback\\)"):
        fa.kv_cache_append_varlen(kn, kn, k, k, cu)
    with pytest.raises(RuntimeError, match="kv_cache_append_paged_varlen needs device tensors \\(no CPU fallback\\)"):
        fa.kv_cache_append_paged_varlen(kn, kn, pool, pool, table, cu)
    with pytest.raises(ValueError, match="packed by token"):
        fa.flash_attention_extend_varlen(T(torch.zeros(2, 8, 20, 64, dtype=torch.bfloat16)), T(k), T(k), T(cu))
    with pytest.raises(ValueError, match="packed by token"):
        fa.kv_cache_append_varlen(T(torch.zeros(2, 2, 20, 64, dtype=torch.bfloat16)), T(kn), T(k), T(k), T(cu))
    for bad in (cu, T(cu.long()), T(cu[:1]), T(torch.zeros(2, 3, dtype=torch.int32)), T(torch.zeros(6, dtype=torch.int32)[::2]), T(cu, "cuda:1")):
        with pytest.raises(ValueError, match="cu_seqlens_q must be a dense int32 device tensor"):
            fa.flash_attention_extend_varlen(T(q), T(k), T(k), bad)
        with pytest.raises(ValueError, match="cu_seqlens_q must be a dense int32 device tensor"):
            fa.kv_cache_append_paged_varlen(T(kn), T(kn), T(pool), T(pool), T(table), bad)
    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_extend_varlen(T(q), T(k), T(k), T(torch.zeros(4, dtype=torch.int32)))     # a batch of 3 against a cache of 2
    with pytest.raises(ValueError, match="Hkv dividing H"):
        fa.flash_attention_extend_varlen(T(q), T(torch.zeros(2, 3, 64, 64, dtype=torch.bfloat16)), T(torch.zeros(2, 3, 64, 64, dtype=torch.bfloat16)), T(cu))
    with pytest.raises(TypeError, match="share a dtype"):
        fa.flash_attention_extend_varlen(T(q), T(k.float()), T(k.float()), T(cu))
    with pytest.raises(ValueError, match="descale"):
        fa.flash_attention_extend_paged_varlen(T(q), T(pool), T(pool), T(table), T(cu), v_descale=T(torch.ones(2)))
    for bad in (table.long(), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, 6, dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="block_table must be an int32 device tensor"):
            fa.flash_attention_extend_paged_varlen(T(q), T(pool), T(pool), T(bad), T(cu))
        with pytest.raises(ValueError, match="block_table must be an int32 device tensor"):
            fa.kv_cache_append_paged_varlen(T(kn), T(kn), T(pool), T(pool), T(bad), T(cu))
    with pytest.raises(ValueError, match="kv_lens must be a dense int32 device tensor"):
        fa.flash_attention_extend_varlen(T(q), T(k), T(k), T(cu), kv_lens=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="kv_lens must be a dense int32 device tensor"):
        fa.kv_cache_append_varlen(T(kn), T(kn), T(k), T(k), T(cu), kv_lens=T(torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(TypeError, match="window"):
        fa.flash_attention_extend_varlen(T(q), T(k), T(k), T(cu), window=16)              # not in this call
    assert fa.FA_VARLEN_MAX_BATCH == MAXB
