"""CPU tests of the MLA index-cache append at the C ABI and in the binding: the signatures, the refusal ladder
beside flash_attention_mla_append's with the new refusals at their places (fake host pointers: no call is valid as a whole, no GPU is
touched), the fronts' refusals, the reference's transform against float64, and a hand-written row under each scale format."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as entry

fa = entry.load_package()

import mla_index_append_check as ic  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, FA_ERR, MISALIGNED, NULL_POINTER, MetaTensor as T,  # noqa: E402
                      aligned_host_pointer, declared_parameters)

BAD_FLAGS = FA_ERR["BAD_FLAGS"]
NAMES = {False: "flash_attention_mla_index_append", True: "flash_attention_mla_index_append_paged"}
TWINS = {False: "flash_attention_mla_append", True: "flash_attention_mla_append_paged"}
HOST = aligned_host_pointer()
P = HOST[1]
by_name = lambda symbol, v: getattr(fa.lib(), symbol)(*[v[n] for n in declared_parameters(symbol)])   # (other keys are the siblings')
S = lambda b, s, h=0: ctypes.byref(fa.FaStrides(b, h, s))
# valid but for the grid (2^28 sequences x 17 position blocks): a call that passes every other check ends at BAD_SHAPE
GEOMETRY = dict(kvLens=None, blockTable=P, batchSize=1 << 28, seqLenNew=1024, seqLenK=1024, numPages=64, pageSize=64, maxPagesPerSeq=16,
                tableStride=16, stream=None)
OK = dict(GEOMETRY, Knew=P, Kidx=P, Kpool=P, kScale=P, kScalePool=P, Qraw=None, Wraw=None, Qidx=None, W=None, cosSin=None, numIndexHeads=64,
          dIndex=128, rotDim=64, maxPos=1024, interleaved=0, scaleFmt=1, wScale=1.0, sKnew=None, sQraw=None)
TWIN_OK = dict(GEOMETRY, Cnew=P, Rnew=P, KV=P, KVpool=P, kvDescale=None, dLatent=512, dRope=64, dtype=fa.FA_DTYPE_BF16,
               kv_dtype=fa.FA_DTYPE_FP8_E4M3, sC=None, sR=None, sKV=None)
Q_SIDE = dict(Qraw=P, Wraw=P, Qidx=P, W=P)
# (what refuses the new call, what refuses flash_attention_mla_append the same way)
LADDER = [(dict(), dict()), (dict(Knew=None), dict(Cnew=None)), (dict(Kidx=None, Kpool=None), dict(KV=None, KVpool=None)),
          (dict(blockTable=None, Kidx=None), dict(blockTable=None, KV=None)), (dict(Knew=P + 8), dict(Cnew=P + 8)),
          (dict(Kidx=P + 4, Kpool=P + 4), dict(KV=P + 4, KVpool=P + 4)), (dict(kvLens=P + 2, seqLenNew=0),) * 2,
          (dict(blockTable=P + 2, seqLenK=0),) * 2, (dict(seqLenNew=0),) * 2, (dict(seqLenNew=1025),) * 2, (dict(batchSize=0),) * 2,
          (dict(seqLenK=0, pageSize=8),) * 2, (dict(seqLenK=(1 << 24) + 1, maxPagesPerSeq=17),) * 2, (dict(numIndexHeads=0), dict(dLatent=0)),
          (dict(numIndexHeads=32), dict(dLatent=256)), (dict(dIndex=64), dict(dRope=32)),
          (dict(numIndexHeads=32, sKnew=S(64, 8)), dict(dLatent=256, sC=S(64, 8))), (dict(sKnew=S(1 << 20, 120)), dict(sC=S(1 << 20, 504))),
          (dict(sKnew=S(1001, 128)), dict(sC=S(1001, 512)))]


def test_the_two_signatures():
    vp, i, f, sp = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(fa.FaStrides)
    tensors = ["Qraw", "Wraw", "Qidx", "W", "cosSin", "kvLens"]
    tail = ["numIndexHeads", "dIndex", "rotDim", "maxPos", "interleaved", "scaleFmt", "wScale", "sKnew", "sQraw", "stream"]
    want = {False: ["Knew", "Kidx", "kScale"] + tensors + ["batchSize", "seqLenNew", "seqLenK"] + tail,
            True: ["Knew", "Kpool", "kScalePool"] + tensors + ["blockTable", "batchSize", "seqLenNew", "numPages", "pageSize", "maxPagesPerSeq",
                                                               "tableStride"] + tail}
    for paged, name in NAMES.items():
        fn = getattr(fa.lib(), name)
        assert name in fa.EXPORTS and fa._MLA_INDEX_APPEND_SYMBOLS[paged] == name and fn.restype is i
        assert declared_parameters(name) == want[paged] and len(fn.argtypes) == len(want[paged])
        assert list(fn.argtypes[:9 + paged]) == [vp] * (9 + paged) and list(fn.argtypes[-4:]) == [f, sp, sp, vp]
    assert (fa.FA_INDEX_SCALE_F32, fa.FA_INDEX_SCALE_POW2) == (0, 1)


@pytest.mark.parametrize("paged", [False, True])
def test_the_ladder_beside_mla_appends_with_the_new_refusals_at_their_places(paged):
    call = lambda **kw: by_name(NAMES[paged], dict(OK, **kw))
    seen = set()
    for mine, twins in LADDER:
        want = by_name(TWINS[paged], dict(TWIN_OK, **twins))
        assert call(**mine) == want, (mine, want)
        seen.add(want)
    assert seen == {NULL_POINTER, MISALIGNED, BAD_SHAPE, BAD_DHEAD, BAD_STRIDE}
    scale = "kScalePool" if paged else "kScale"
    # the pointers first: the scales, and the Q side all or nothing -- ahead of every alignment
    assert call(**{scale: None}) == call(**{scale: None, "Knew": P + 8}) == NULL_POINTER
    for n in range(1, 15):
        some = {k: v for bit, (k, v) in enumerate(Q_SIDE.items()) if n >> bit & 1}
        assert call(**some) == call(Knew=P + 8, kvLens=P + 2, **some) == NULL_POINTER, some
    q = lambda **kw: call(**dict(Q_SIDE, **kw))
    assert q() == BAD_SHAPE
    # 16 bytes for the tensors and the table, then 4 for the arrays, ahead of the geometry and the shape
    for name in ("Qraw", "Qidx", "cosSin"):
        assert q(**{name: P + 8}) == q(**{name: P + 8, "seqLenNew": 0, "pageSize": 24, scale: P + 2}) == MISALIGNED
    for name in (scale, "Wraw", "W"):
        assert q(**{name: P + 2}) == q(**{name: P + 2, "seqLenNew": 0, "pageSize": 24, "seqLenK": 0}) == MISALIGNED and q(**{name: P + 4}) == BAD_SHAPE
    # the table's rules behind the widths, ahead of the flags and the strides; without a table rotDim and maxPos are not read
    for kw in (dict(rotDim=0), dict(rotDim=8), dict(rotDim=24), dict(rotDim=144), dict(maxPos=1023)):
        assert call(cosSin=P, interleaved=2, sKnew=S(64, 8), **kw) == BAD_SHAPE and call(cosSin=P, numIndexHeads=32, **kw) == BAD_DHEAD
        assert call(interleaved=2, **kw) == BAD_FLAGS
    assert call(cosSin=P, rotDim=128, maxPos=1 << 20, interleaved=2) == call(cosSin=P, rotDim=16, interleaved=2) == BAD_FLAGS
    for kw in (dict(interleaved=2), dict(interleaved=-1), dict(scaleFmt=2), dict(scaleFmt=-1)):
        assert call(**kw) == call(wScale=float("nan"), sKnew=S(64, 8), **kw) == BAD_FLAGS and call(dIndex=64, **kw) == BAD_DHEAD
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(wScale=bad) == call(wScale=bad, sKnew=S(64, 8)) == BAD_SCALE and call(wScale=bad, scaleFmt=3) == BAD_FLAGS
    assert call(wScale=-0.5) == call(wScale=0.0) == BAD_SHAPE
    # the strides of Qraw with Knew's, read only with the Q side
    for s in (S(1 << 24, 120, 1 << 13), S(1 << 24, 1 << 13, 100), S(1001, 1 << 13, 128), S(-8, 1 << 13, 128)):
        assert q(sQraw=s) == BAD_STRIDE and call(sQraw=s) == BAD_SHAPE
    assert q(sQraw=S(1 << 24, 128, 1 << 13)) == BAD_SHAPE


def test_binding_refusals():
    bf, f8 = torch.bfloat16, torch.float8_e4m3fn
    k, q, w = torch.zeros(2, 3, 128, dtype=bf), torch.zeros(2, 3, 64, 128, dtype=bf), torch.zeros(2, 3, 64)
    cache, sc, table, cs = torch.zeros(2, 48, 128).to(f8), torch.zeros(2, 48), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(48, 64)
    meta = lambda kw: {n: T(v) if torch.is_tensor(v) else v for n, v in kw.items()}
    contig = lambda k=k, cache=cache, sc=sc, **kw: fa.mla_index_append(T(k), T(cache), T(sc), **meta(kw))
    paged = lambda k=k, cache=cache[:, :16].contiguous(), sc=sc[:, :16].contiguous(), **kw: \
        fa.mla_index_append_paged(T(k), T(cache), T(sc), T(table), **meta(kw))
    refusals = [(ValueError, r"k_new must be \[B, Sq, 128\]", [dict(k=k[..., :64]), dict(k=k[0]), dict(cache=torch.zeros(2, 48, 64).to(f8))]),
                (TypeError, "k_new must be bfloat16", [dict(k=k.float()), dict(cache=torch.zeros(2, 48, 128, dtype=bf))]),
                (ValueError, "k_scale must be an fp32 tensor", [dict(sc=sc.double()), dict(sc=sc[:, :8])]),
                (ValueError, "new rows: must be 1 .. the capacity", [dict(k=torch.zeros(2, 49, 128, dtype=bf))]),
                (ValueError, "kv_lens must be a dense int32 device tensor", [dict(kv_lens=torch.zeros(3, dtype=torch.int32))]),
                (ValueError, "q and w go together", [dict(q=q), dict(w=w), dict(Qidx=q.to(f8)), dict(W=w)]),
                (ValueError, r"q must be a bfloat16 tensor \[B, Sq, 64, 128\]", [dict(w=w, q=q[:, :, :32]), dict(w=w, q=q.float()), dict(w=w, q=q[:, :2])]),
                (ValueError, r"w must be a dense fp32 tensor \[B, Sq, 64\]", [dict(q=q, w=w.double()), dict(q=q, w=torch.zeros(2, 3, 128)[..., ::2])]),
                (ValueError, "scale_fmt must be", [dict(scale_fmt="ue8m0"), dict(scale_fmt=1)]),
                (ValueError, "w_scale must be finite", [dict(w_scale=float("inf"))]),
                (ValueError, "cos_sin", [dict(cos_sin=c) for c in (cs.double(), cs[:, :24], torch.zeros(48, 144), cs[:47])])]
    for front in (contig, paged):
        for error, match, cases in refusals:
            for kw in cases:
                with pytest.raises(error, match=match):
                    front(**kw)
    for front in (lambda: fa.mla_index_append(k, cache, sc), lambda: fa.mla_index_append_paged(k, cache, sc, table)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            front()
    with pytest.raises(ValueError, match="block_table must be an int32"):
        fa.mla_index_append_paged(T(k), T(cache), T(sc), None)


def test_the_references_transform_against_the_sylvester_matrix_in_float64():
    """|hadamard(x) c0 - 2^-3.5 x H| <= 2^-20 128^-0.5 sum |x_j|: twice gamma_8 = 8 * 2^-24 -- seven add stages and one multiply"""
    j = np.arange(128)
    Hm = np.where(np.array([[bin(a & b).count("1") & 1 for b in j] for a in j]) == 1, -1.0, 1.0)
    assert (Hm[:2, :4] == [[1, 1, 1, 1], [1, -1, 1, -1]]).all() and (Hm @ Hm == 128 * np.eye(128)).all()
    x = (torch.randn(64, 128, generator=torch.Generator().manual_seed(9000)) * 3).to(torch.bfloat16).float().numpy()
    err = np.abs((ic.hadamard(x) * ic.C0).astype(np.float64) - x.astype(np.float64) @ Hm * 2.0 ** -3.5).max(-1)
    bound = 2.0 ** -20 * 128 ** -0.5 * np.abs(x).sum(-1)
    print(f"worst error / bound {(err / bound).max():.4f}")
    assert (err <= bound).all() and ic.hadamard(x).dtype == np.float32


def test_a_hand_written_row_under_each_scale_format():
    """8 e_0 and 8 e_1: every |t| is 8, r = bf16(8 * 2^-3.5) = 0.70703125 (0x3F35); s0 = 0.70703125 / 448 = 0.0015782...; f32: the
    quotient rounds to 448 (0x7E); pow2: s = 2^-9, the quotient is 362, which e4m3fn rounds to 352 (0x7B).  e_1 alternates the sign"""
    x = torch.zeros(1, 1, 2, 128, dtype=torch.bfloat16)
    x[0, 0, 0, 0] = x[0, 0, 1, 1] = 8.0
    for pow2, code, scale in ((False, 0x7E, np.float32(0.70703125) * np.float32(1.0 / 448.0)), (True, 0x7B, np.float32(2.0 ** -9))):
        codes, s = ic.transform(x, pow2)
        assert s.numpy().tobytes() == np.array([scale, scale], dtype=np.float32).tobytes() and 0.70703125 / 448 - 2e-10 < scale < 2 * 0.70703125 / 448
        assert codes[0, 0, 0].tolist() == [code] * 128 and codes[0, 0, 1].tolist() == [code, code | 0x80] * 64
    assert ic.scale_of(np.float32([0.0, 2.0 ** -9 * 448, 448.0]), True).tolist() == [2.0 ** -22, 2.0 ** -9, 1.0]
