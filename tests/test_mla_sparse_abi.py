"""CPU tests of sparse MLA decode at the C ABI and in the binding (flash_attention_mla_sparse_decode, _paged, _fp8, _paged_fp8,
flash_attention_mla_sparse_plan): the five signatures; the refusal ladder of every call beside its dense twin's,
code for code (fake aligned host pointers: no GPU is touched), with the four new refusals at their places; the plan; the fronts."""
import ctypes
import itertools

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

import mla_check as mc  # noqa: E402
import mla_sparse_check as sc  # noqa: E402
from abi_decl import (BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F32, FP8, MISALIGNED, NULL_POINTER,  # noqa: E402
                      MetaTensor as T, aligned_host_pointer, declared_parameters)
from test_mla_abi import ladder  # noqa: E402

NAMES = [sc.symbol(fp8, paged) for fp8 in (False, True) for paged in (False, True)]
INDEX_ARGS = ["indices", "topk", "indexStrideB", "indexStrideQ"]


def test_the_five_signatures():
    L = fa.lib()
    kinds = {"topk": ctypes.c_int, "indexStrideB": ctypes.c_int64, "indexStrideQ": ctypes.c_int64, "indices": ctypes.c_void_p}
    for name in NAMES:
        dense = name.replace("_sparse", "")
        mine, theirs = declared_parameters(name), declared_parameters(dense)
        at = theirs.index("kvLens") + 1
        assert mine == theirs[:at] + INDEX_ARGS + theirs[at:], name          # the dense signature, the index list after kvLens
        want = list(getattr(L, dense).argtypes)
        assert list(getattr(L, name).argtypes) == want[:at] + [kinds[n] for n in INDEX_ARGS] + want[at:], name
        assert name in fa.EXPORTS and getattr(L, name).restype is ctypes.c_int
    assert declared_parameters("flash_attention_mla_sparse_plan") == ["batchSize", "numHeads", "seqLenQ", "topk", "dLatent", "dRope", "o_dtype",
                                                                      "numSplits", "plan"]
    assert list(L.flash_attention_mla_sparse_plan.argtypes) == [ctypes.c_int] * 8 + [ctypes.POINTER(fa.FaDecodePlan)]
    assert "flash_attention_mla_sparse_plan" in fa.EXPORTS


def calls(name):
    """(call(twin=False, **overrides), p): `name` -- or with twin=True its dense twin -- on an aligned host pointer p; overrides under
    mla_check's short keys or the header's own names.  Valid but for the workspace (two forced splits)"""
    host = aligned_host_pointer()
    p = host[1]
    ok = dict(Q=p, KV=p, KVpool=p, O=p, LSE=None, kvLens=None, indices=p, topk=64, indexStrideB=256, indexStrideQ=64, blockTable=p,
              kvDescale=None, workspace=None, batchSize=2, numHeads=8, seqLenQ=4, seqLenK=1024, numPages=64, pageSize=64, maxPagesPerSeq=16,
              tableStride=16, dLatent=512, dRope=64, scale=0.125, is_causal=True, dtype=BF16, kv_dtype=FP8, o_dtype=F32, numSplits=2,
              sQ=None, sKV=None, sO=None, stream=None)

    def call(twin=False, _keep=host, **kw):
        named = dict(ok)
        for key, value in kw.items():
            for n in mc.KEYS.get(key, (key,)):
                named[n] = value
        return sc.c_call(name.replace("_sparse", "") if twin else name, **named)

    return call, p


@pytest.mark.parametrize("name", NAMES)
def test_the_dense_ladder_code_for_code_and_the_new_refusals_at_their_places(name):
    call, p = calls(name)
    assert call() == call(twin=True) == NULL_POINTER                                    # valid but for the workspace
    for kw in ladder(p, "paged" in name):
        assert call(**kw) == call(twin=True, **kw), kw
    for s in (fa.FaStrides(64, 16, 8), fa.FaStrides(1 << 20, 1 << 20, 1030)):
        for key in ("sQ", "sKV", "sO"):
            assert call(**{key: ctypes.byref(s)}) == call(twin=True, **{key: ctypes.byref(s)}) == BAD_STRIDE
    if "fp8" in name:
        assert call(kv_dtype=BF16) == call(twin=True, kv_dtype=BF16) == BAD_DTYPE
    # a NULL index list: with the pointers, ahead of every alignment
    assert call(indices=None) == NULL_POINTER and call(indices=None, Q=p + 8) == NULL_POINTER and call(indices=None, ws=p) == NULL_POINTER
    # its alignment: after the tensors' and the other arrays', ahead of the geometry and the shape
    assert call(indices=p + 2, ws=p) == MISALIGNED and call(indices=p + 2, Sq=0) == MISALIGNED and call(indices=p + 4) == NULL_POINTER
    assert call(indices=p + 2, Q=None) == NULL_POINTER and call(indices=p + 2, **(dict(page=24) if "paged" in name else dict(Sk=0))) == MISALIGNED
    # topk: with the shapes -- behind the alignments, ahead of the types, the scale and the strides
    for topk in (0, -1, (1 << 20) + 1):
        assert call(topk=topk, ws=p) == BAD_SHAPE and call(topk=topk, dtype=F32) == BAD_SHAPE and call(topk=topk, scale=0.0) == BAD_SHAPE
        assert call(topk=topk, lens=p + 2) == MISALIGNED and call(topk=topk, Q=None) == NULL_POINTER
    assert call(topk=1) == NULL_POINTER and call(topk=1 << 20, indexStrideQ=1 << 20) == NULL_POINTER
    # the index row stride: with the strides -- behind the scale, ahead of the extent and the workspace
    for kw in (dict(indexStrideQ=63), dict(indexStrideQ=0), dict(indexStrideB=-1)):
        assert call(**kw) == call(ws=p, **kw) == BAD_STRIDE and call(scale=0.0, **kw) == BAD_SCALE and call(dtype=F32, **kw) == BAD_DTYPE
    assert call(indexStrideB=0) == NULL_POINTER and call(indexStrideQ=1 << 40) == NULL_POINTER


def test_plan_properties_and_the_workspace_size():
    L = fa.lib()
    for B, H, Sq, topk in itertools.product((1, 3, 32, 128), (1, 16, 64, 65, 128), (1, 2, 16), (1, 31, 32, 33, 200, 2048, 1 << 20)):
        auto = fa.mla_sparse_plan(B, H, Sq, topk)
        blocks, tiles = -(-H // 64), -(-topk // 32)
        units = B * Sq * blocks
        assert auto["rows_per_block"] == 64 and auto["kv_block_rows"] == 32 and auto["threads"] == 256 and auto["row_blocks"] == blocks
        assert auto["grid"] == units * auto["num_splits"] and auto["lds_bytes"] == fa.mla_decode_plan(B, H, Sq, 384)["lds_bytes"]
        # mla_route's formula on these units and tiles
        assert 1 <= auto["num_splits"] <= max(1, min(CAP, tiles // 2)) and (auto["num_splits"] == 1 or units < 256)
        assert (auto["combine_grid"], auto["combine_threads"]) == ((B * H * Sq, 256) if auto["num_splits"] > 1 else (0, 0))
        for ns in (1, 3, CAP):
            got = fa.mla_sparse_plan(B, H, Sq, topk, num_splits=ns)
            assert got["num_splits"] == ns and got["grid"] == units * ns
            assert int(L.flash_attention_mla_decode_workspace_size(B, H, Sq, 512, ns)) == fa.decode_workspace_size(B, H, Sq, 512, ns)
    assert fa.mla_sparse_plan(1, 16, 1, 2048)["num_splits"] == 32 and fa.mla_sparse_plan(128, 128, 1, 2048)["num_splits"] == 1
    p = fa.FaDecodePlan()
    rc = lambda *a, plan=p: L.flash_attention_mla_sparse_plan(*a, ctypes.byref(plan) if plan is not None else None)
    assert rc(2, 8, 4, 64, 512, 64, F32, 0) == 0 and rc(2, 8, 4, 64, 512, 64, F32, 0, plan=None) == NULL_POINTER
    for a in ((2, 8, 4, 0, 512, 64, F32, 0), (2, 8, 4, (1 << 20) + 1, 512, 64, F32, 0), (2, 8, 17, 64, 512, 64, F32, 0),
              (2, 8, 4, 64, 512, 64, F32, CAP + 1), (1 << 18, 1, 1, 2048, 512, 64, F32, 64)):
        assert rc(*a) == BAD_SHAPE, a
    assert rc(2, 8, 4, 64, 512, 64, FP8, 0) == BAD_DTYPE


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    bf = torch.bfloat16
    q, kv = torch.zeros(2, 8, 3, 576, dtype=bf), torch.zeros(2, 64, 576, dtype=bf)
    pool, table = torch.zeros(9, 16, 576, dtype=bf), torch.zeros(2, 3, dtype=torch.int32)
    idx = torch.zeros(2, 3, 40, dtype=torch.int32)
    contig = lambda i, **kw: fa.flash_attention_mla_sparse_decode(T(q), T(kv), i, **kw)
    paged = lambda i, **kw: fa.flash_attention_mla_sparse_decode_paged(T(q), T(pool), T(table), i, **kw)
    for front in (contig, paged):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            front(idx)
        for wrong in (None, T(idx.long()), T(idx[:1]), T(idx[:, :2]), T(idx[0]), T(idx, device="cuda:1")):
            with pytest.raises(ValueError, match=r"indices must be an int32 tensor \[B, Sq, topk\]"):
                front(wrong)
        for wrong in (T(idx[:, :, :0]), T(idx[:, :, ::2])):
            with pytest.raises(ValueError, match="contiguous last dimension"):
                front(wrong)
        for ns in (-1, CAP + 1):
            with pytest.raises(fa.FlashAttentionError) as e:
                front(T(idx), num_splits=ns)
            assert e.value.code == BAD_SHAPE
        with pytest.raises(TypeError, match="window"):
            front(T(idx), window=16)
    assert "576 ** -0.5" in fa.flash_attention_mla_sparse_decode.__doc__
