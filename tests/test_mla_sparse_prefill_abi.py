"""CPU tests of sparse MLA prefill at the C ABI and in the binding (flash_attention_mla_sparse_prefill, _paged, _plan; DESIGN.md
section 42): the three signatures; the refusal ladder beside flash_attention_mla_sparse_decode's, code for code (fake aligned host
pointers; every call is refused before a launch), with the new refusals at their places; the plan; the fronts."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

import mla_check as mc  # noqa: E402
import mla_sparse_check as sc  # noqa: E402
from abi_decl import (BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, F32, FP8, MISALIGNED, NULL_POINTER,  # noqa: E402
                      MetaTensor as T, aligned_host_pointer, declared_parameters)
from test_mla_abi import ladder  # noqa: E402

NAMES = [fa._MLA_SPARSE_PREFILL_SYMBOLS[paged] for paged in (False, True)]
TWIN = {NAMES[0]: sc.symbol(True, False), NAMES[1]: sc.symbol(True, True)}       # the _fp8 decode calls: they take kv_dtype and kvDescale


def test_the_three_signatures():
    L = fa.lib()
    for name in NAMES:
        mine, theirs = declared_parameters(name), declared_parameters(TWIN[name])
        # the decode signature with cuSeqlensQ before kvLens, totalQ for seqLenQ, and no indexStrideB, workspace or numSplits
        want = [{"seqLenQ": "totalQ"}.get(n, n) for n in theirs if n not in ("indexStrideB", "workspace", "numSplits")]
        want.insert(want.index("kvLens"), "cuSeqlensQ")
        assert mine == want, name
        assert name in fa.EXPORTS and getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) == len(mine)
    assert declared_parameters("flash_attention_mla_sparse_prefill_plan") == "batchSize numHeads totalQ topk dLatent dRope o_dtype plan".split()


def calls(name):
    """call(twin=False, **overrides): `name` -- or its decode twin -- on an aligned host pointer.  Valid but for the cache's extent, the
    last rung of both ladders (a row stride of 2^25 elements), so nothing is ever launched"""
    host = aligned_host_pointer()
    p = host[1]
    wide = fa.FaStrides(0, 0, 1 << 25)
    ok = dict(Q=p, KV=p, KVpool=p, O=p, LSE=None, cuSeqlensQ=p, kvLens=None, indices=p, topk=64, indexStrideB=256, indexStrideQ=64,
              blockTable=p, kvDescale=None, workspace=p, batchSize=2, numHeads=8, seqLenQ=4, totalQ=4, seqLenK=1024, numPages=64,
              pageSize=64, maxPagesPerSeq=16, tableStride=16, dLatent=512, dRope=64, scale=0.125, is_causal=True, dtype=BF16, kv_dtype=FP8,
              o_dtype=F32, numSplits=1, sQ=None, sKV=ctypes.byref(wide), sO=None, stream=None)

    def call(twin=False, _keep=(host, wide), **kw):
        named = dict(ok)
        for key, value in kw.items():
            for n in mc.KEYS.get(key, (key,)) + (("totalQ",) if key == "Sq" else ()):
                named[n] = value
        return sc.c_call(TWIN[name] if twin else name, **named)

    return call, p


@pytest.mark.parametrize("name", NAMES)
def test_the_decode_ladder_code_for_code_and_the_new_refusals_at_their_places(name):
    call, p = calls(name)
    assert call() == call(twin=True) == BAD_SHAPE                                        # valid but for the extent
    for kw in ladder(p, "paged" in name):
        if "ns" in kw or kw.get("Sq") == 17 or kw.get("ws") == p + 8:                    # (no split count or workspace; totalQ is not capped)
            continue
        assert call(**kw) == call(twin=True, **kw), kw
    for s, key in ((s, key) for s in (fa.FaStrides(64, 16, 8), fa.FaStrides(1 << 20, 1 << 20, 1030)) for key in ("sQ", "sKV", "sO")):
        assert call(**{key: ctypes.byref(s)}) == call(twin=True, **{key: ctypes.byref(s)}) == BAD_STRIDE
    for kw in (dict(indices=None), dict(indices=p + 2), dict(topk=0), dict(topk=(1 << 20) + 1), dict(indexStrideQ=63), dict(kv_dtype=F32)):
        assert call(**kw) == call(twin=True, **kw), kw
    assert call(kv_dtype=BF16) == BAD_SHAPE and call(kv_dtype=BF16, kvDescale=p) == BAD_DTYPE and call(kvDescale=p + 2) == MISALIGNED
    # a NULL cuSeqlensQ: with the pointers, ahead of every alignment
    assert call(cuSeqlensQ=None) == call(cuSeqlensQ=None, Q=p + 8) == call(cuSeqlensQ=None, Sq=0) == NULL_POINTER
    # its alignment: with the arrays', after the tensors', ahead of the index list's, the geometry and the shape
    assert call(cuSeqlensQ=p + 2) == call(cuSeqlensQ=p + 2, Sq=0) == call(cuSeqlensQ=p + 2, topk=0) == MISALIGNED
    assert call(cuSeqlensQ=p + 2, Q=None) == NULL_POINTER and call(cuSeqlensQ=p + 4) == BAD_SHAPE
    # totalQ, the batch and the grid: with the shapes -- behind the alignments, ahead of the types, the scale and the strides
    for kw in (dict(Sq=0), dict(Sq=-1), dict(B=fa.FA_VARLEN_MAX_BATCH + 1), dict(H=1 << 16, Sq=1 << 15)):
        assert call(**kw) == call(dtype=F32, **kw) == call(scale=0.0, **kw) == call(indexStrideQ=1, **kw) == BAD_SHAPE, kw
        assert call(lens=p + 2, **kw) == MISALIGNED and call(Q=None, **kw) == NULL_POINTER
    for kw in (dict(Sq=1 << 24), dict(H=129, Sq=1 << 23)):                               # (the grid: after the types, as in the twin)
        assert call(**kw) == call(scale=0.0, **kw) == call(indexStrideQ=1, **kw) == BAD_SHAPE and call(dtype=F32, **kw) == BAD_DTYPE, kw
    assert call(Sq=17, dtype=F32) == BAD_DTYPE and call(Sq=(1 << 24) - 1, scale=0.0) == BAD_SCALE
    # the index row stride: with the strides -- behind the scale, ahead of the extent
    for kw in (dict(indexStrideQ=63), dict(indexStrideQ=0)):
        assert call(**kw) == BAD_STRIDE and call(scale=0.0, **kw) == BAD_SCALE and call(dtype=F32, **kw) == BAD_DTYPE
    assert call(indexStrideQ=1 << 40) == BAD_SHAPE


def test_plan_fields():
    L = fa.lib()
    for B, H, T, topk in ((1, 1, 1, 1), (4, 16, 26, 33), (8, 128, 4096, 2048), (65, 129, 1088, 2048), (1024, 257, 7, 1 << 20)):
        got = fa.mla_sparse_prefill_plan(B, H, T, topk)
        blocks = -(-H // 128)
        assert got["rows_per_block"] == 128 and got["row_blocks"] == blocks and got["num_splits"] == 1 and got["grid"] == T * blocks
        assert got["kv_block_rows"] == 32 and got["threads"] == 512 and got["lds_bytes"] <= 160 * 1024
        assert (got["combine_grid"], got["combine_threads"]) == (0, 0)
    p = fa.FaDecodePlan()
    rc = lambda *a, plan=p: L.flash_attention_mla_sparse_prefill_plan(*a, ctypes.byref(plan) if plan is not None else None)
    assert rc(2, 8, 4, 64, 512, 64, F32) == 0 and rc(2, 8, 4, 64, 512, 64, F32, plan=None) == NULL_POINTER
    for a in ((2, 8, 0, 64, 512, 64, F32), (2, 8, 4, 0, 512, 64, F32), (1025, 8, 4, 64, 512, 64, F32), (2, 8, 1 << 24, 64, 512, 64, F32),
              (2, 129, 1 << 23, 64, 512, 64, F32), (0, 8, 4, 64, 512, 64, F32)):
        assert rc(*a) == BAD_SHAPE, a
    assert rc(2, 8, 4, 64, 512, 64, FP8) == BAD_DTYPE and rc(2, 8, (1 << 24) - 1, 64, 512, 64, F32) == 0


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    bf = torch.bfloat16
    q, kv = torch.zeros(7, 8, 576, dtype=bf), torch.zeros(2, 64, 576, dtype=bf)
    pool, table = torch.zeros(9, 16, 576, dtype=bf), torch.zeros(2, 3, dtype=torch.int32)
    idx, cu = torch.zeros(7, 40, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    contig = lambda i, c, **kw: fa.flash_attention_mla_sparse_prefill(T(q), T(kv), i, c, **kw)
    paged = lambda i, c, **kw: fa.flash_attention_mla_sparse_prefill_paged(T(q), T(pool), T(table), i, c, **kw)
    for front in (contig, paged):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            front(idx, T(cu))
        with pytest.raises(ValueError, match="are required"):
            front(None, T(cu))
        for wrong in (T(idx.long()), T(idx[:6]), T(idx[0]), T(idx[:, :0]), T(idx[:, ::2]), T(idx, device="cuda:1")):
            with pytest.raises(ValueError, match=r"indices must be an int32 tensor \[T, topk >= 1\]"):
                front(wrong, T(cu))
        for wrong in (T(cu.long()), T(cu[:1]), T(cu.reshape(1, 3)), cu):
            with pytest.raises(ValueError, match="cu_seqlens_q must be a dense int32 device tensor"):
                front(T(idx), wrong)
        with pytest.raises(ValueError, match="kv_descale belongs to an fp8"):
            front(T(idx), T(cu), kv_descale=T(torch.ones(1)))
        with pytest.raises(TypeError, match="num_splits"):
            front(T(idx), T(cu), num_splits=2)
    with pytest.raises(ValueError, match="one cache per sequence"):
        contig(T(idx), T(torch.zeros(4, dtype=torch.int32)))
    assert "576 ** -0.5" in fa.flash_attention_mla_sparse_prefill.__doc__
