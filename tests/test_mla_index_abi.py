"""CPU tests of the MLA indexer at the C ABI and in the binding (flash_attention_mla_index_topk, _paged): the two
signatures, the refusal ladder beside flash_attention_mla_decode's (fake aligned host pointers; no call here is valid as a whole, so no
GPU is touched), the fronts' refusals, and the float64 reference's tie and padding rule on a hand-written row."""
import ctypes

import pytest
import torch

import __graft_entry__ as entry

fa = entry.load_package()

import mla_sparse_check as sc  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_SHAPE, BAD_STRIDE, MISALIGNED, NULL_POINTER, MetaTensor as T, aligned_host_pointer,  # noqa: E402
                      declared_parameters)
from test_mla_abi import calls as mla_calls  # noqa: E402
from test_mla_index import select  # noqa: E402

NAMES = {False: "flash_attention_mla_index_topk", True: "flash_attention_mla_index_topk_paged"}
# the header's name -> mla_check's short key of the argument flash_attention_mla_decode* shares
SHARED = dict(kvLens="lens", blockTable="table", batchSize="B", seqLenQ="Sq", seqLenK="Sk", numPages="P", pageSize="page",
              maxPagesPerSeq="maxp", tableStride="ts")


def test_the_two_signatures():
    L = fa.lib()
    vp, i, i64, b = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_bool
    head = [("Qidx", vp), ("W", vp), ("Kidx", vp), ("kScale", vp), ("kvLens", vp)]
    mid = [("logits", vp), ("indices", vp), ("topk", i), ("logitStride", i64), ("indexStrideB", i64), ("indexStrideQ", i64),
           ("batchSize", i), ("seqLenQ", i)]
    tail = [("numIndexHeads", i), ("dIndex", i), ("is_causal", b), ("stream", vp)]
    paging = [("numPages", i), ("pageSize", i), ("maxPagesPerSeq", i), ("tableStride", i64)]
    want = {False: head + mid + [("seqLenK", i)] + tail,
            True: head[:2] + [("Kpool", vp), ("kScalePool", vp), ("kvLens", vp), ("blockTable", vp)] + mid + paging + tail}
    for paged, name in NAMES.items():
        assert name in fa.EXPORTS and fa._MLA_INDEX_SYMBOLS[paged] == name and getattr(L, name).restype is i
        assert declared_parameters(name) == [n for n, _ in want[paged]]
        assert list(getattr(L, name).argtypes) == [t for _, t in want[paged]]


@pytest.mark.parametrize("paged", [False, True])
def test_the_ladder_beside_mla_decodes_with_the_new_refusals_at_their_places(paged):
    host = aligned_host_pointer()
    p = host[1]
    # valid but for the grid (2^20 sequences x 16 blocks of 256 keys): passing every other check ends at BAD_SHAPE, behind the strides
    ok = dict(Qidx=p, W=p, Kidx=p, Kpool=p, kScale=p, kScalePool=p, kvLens=None, blockTable=p, logits=p, indices=p, topk=64, logitStride=4096,
              indexStrideB=64, indexStrideQ=64, batchSize=1 << 20, seqLenQ=1, seqLenK=4096, numPages=64, pageSize=64, maxPagesPerSeq=64,
              tableStride=64, numIndexHeads=64, dIndex=128, is_causal=True, stream=None)
    call = lambda _keep=host, **kw: sc.c_call(NAMES[paged], **dict(ok, **kw))
    twin = mla_calls()[0]["flash_attention_mla_decode" + ("_paged" if paged else "")]
    assert call() == BAD_SHAPE and call(seqLenQ=4) == call(seqLenQ=4, dIndex=64) == BAD_SHAPE     # the grid; 2^22 rows of the selection
    # what both calls take, code for code: the lengths' and the table's pointers, the paging geometry, the shape
    shared = [dict(kvLens=p + 2), dict(kvLens=p + 2, seqLenQ=0)] + [dict(seqLenQ=s) for s in (0, -1, 17)] + [dict(batchSize=0)]
    shared += [dict(blockTable=None), dict(blockTable=p + 2), dict(blockTable=p + 2, seqLenQ=0), dict(numPages=0), dict(maxPagesPerSeq=0),
               dict(pageSize=8), dict(pageSize=24), dict(tableStride=63), dict(pageSize=1 << 16, maxPagesPerSeq=1 << 16, tableStride=1 << 16)] \
        if paged else [dict(seqLenK=0), dict(seqLenK=-128), dict(seqLenK=(1 << 24) + 1)]
    for kw in shared:
        want = twin(**dict(dict(maxp=64, ts=64), **{SHARED[k]: v for k, v in kw.items()}))     # (no workspace: the twin never launches)
        assert call(**kw) == want and call(numIndexHeads=32, indexStrideQ=1, **kw) == want and want in (NULL_POINTER, MISALIGNED, BAD_SHAPE), kw
    # the pointers first, ahead of every alignment
    for name in ("Qidx", "W", "Kpool" if paged else "Kidx", "kScalePool" if paged else "kScale", "logits", "indices"):
        assert call(**{name: None}) == call(**{name: None, "kvLens": p + 2, "logits" if name != "logits" else "Qidx": p + 8}) == NULL_POINTER
    # 16 bytes for the tensors, then 4 for the arrays, ahead of the geometry and the shape
    for name in ("Qidx", "Kpool" if paged else "Kidx", "logits"):
        assert call(**{name: p + 8}) == call(**{name: p + 8, "seqLenQ": 0, "pageSize": 24, "W": p + 2}) == MISALIGNED
    for name in ("W", "kScalePool" if paged else "kScale", "indices"):
        assert call(**{name: p + 2}) == call(**{name: p + 2, "seqLenQ": 0, "pageSize": 24, "seqLenK": 0}) == MISALIGNED
        assert call(**{name: p + 4}) == BAD_SHAPE
    # topk with the shapes: behind the alignments, ahead of the widths and the strides
    for topk in (0, -1, (1 << 20) + 1):
        assert call(topk=topk, numIndexHeads=32, logitStride=1) == BAD_SHAPE and call(topk=topk, W=p + 2) == MISALIGNED
    # the widths where the MLA calls refuse theirs: behind the shape, ahead of the strides
    for kw in (dict(numIndexHeads=32), dict(numIndexHeads=128), dict(dIndex=64), dict(dIndex=576), dict(numIndexHeads=128, dIndex=64)):
        assert call(**kw) == call(logitStride=1, **kw) == BAD_DHEAD and call(seqLenQ=17, **kw) == BAD_SHAPE
    # the strides last before the grid
    for kw in (dict(logitStride=4095), dict(logitStride=0), dict(indexStrideQ=63), dict(indexStrideB=-1), dict(topk=1 << 20)):
        assert call(**kw) == BAD_STRIDE, kw
    assert call(logitStride=1 << 40, indexStrideB=0, indexStrideQ=1 << 40) == BAD_SHAPE


def test_binding_refusals():
    f8 = torch.float8_e4m3fn
    q, w = torch.zeros(2, 3, 64, 128).to(f8), torch.zeros(2, 3, 64)
    k, ks = torch.zeros(2, 48, 128).to(f8), torch.zeros(2, 48)
    table = torch.zeros(2, 3, dtype=torch.int32)
    contig = lambda q=q, w=w, k=k, ks=ks, topk=8, **kw: fa.mla_index_topk(T(q), T(w), T(k), T(ks), topk, **kw)
    paged = lambda q=q, w=w, k=k[:, :16].contiguous(), ks=ks[:, :16].contiguous(), topk=8, **kw: \
        fa.mla_index_topk_paged(T(q), T(w), T(k), T(ks), T(table), topk, **kw)
    for front in (fa.mla_index_topk, lambda *a: fa.mla_index_topk_paged(*a[:4], table, a[4])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            front(q, w, k, ks, 8)
    for front in (contig, paged):
        for kw in (dict(q=q.float()), dict(k=k.to(torch.bfloat16))):
            with pytest.raises(TypeError, match="float8_e4m3fn"):
                front(**kw)
        for kw in (dict(q=q[:, :, :32]), dict(q=q[..., :64]), dict(q=q[0]), dict(k=k[..., :64])):
            with pytest.raises(ValueError, match=r"Qidx must be \[B, Sq, 64, 128\]"):
                front(**kw)
        for kw in (dict(w=w.double()), dict(w=w[:, :2]), dict(w=w[..., :32])):
            with pytest.raises(ValueError, match=r"W must be an fp32 tensor \[B, Sq, 64\]"):
                front(**kw)
        for kw in (dict(ks=ks.double()), dict(ks=ks[:, :8])):
            with pytest.raises(ValueError, match="k_scale must be an fp32 tensor"):
                front(**kw)
        with pytest.raises(ValueError, match="must be dense"):
            front(w=torch.zeros(2, 3, 128)[..., ::2])
        for topk in (0, -3, 2.0, True):
            with pytest.raises(ValueError, match="topk must be an int >= 1"):
                front(topk=topk)
        with pytest.raises(ValueError, match="kv_lens must be a dense int32 device tensor"):
            front(kv_lens=T(torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"Qidx must be \[B, Sq, 64, 128\]"):
        contig(k=k[:1])
    with pytest.raises(ValueError, match="block_table must be an int32"):
        fa.mla_index_topk_paged(T(q), T(w), T(k), T(ks), None, 8)


def test_the_references_tie_and_padding_rule_on_a_hand_written_row():
    logits = torch.tensor([[[1.0, 3.0, 3.0, 0.0, 2.0, 3.0, 0.0, 2.0]]])
    vis = torch.arange(8)[None, None] < 7                         # position 7 is beyond the limit
    want = {1: [1], 2: [1, 2], 4: [1, 2, 4, 5], 6: [0, 1, 2, 3, 4, 5], 9: [0, 1, 2, 3, 4, 5, 6, -1, -1]}
    for topk, row in want.items():
        assert select(logits, vis, topk).tolist() == [[row]], topk
