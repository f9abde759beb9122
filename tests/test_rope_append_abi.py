"""CPU tests of flash_attention_rope_append, _paged, _varlen and _paged_varlen at the C ABI and in the binding: the symbols exist with the
declared parameter lists and argtypes, each list its kv_append twin's plus the arguments the header names; every invalid argument is
refused before anything is launched, the twin's mistakes with the twin's codes and the new ones at their place in the ladder, for both
cache types (aligned host pointers: no GPU is touched, and no case is valid as a whole); the binding's own refusals; rope_table."""
import ctypes

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import rope_call as call  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BF16, F16, F32, FA_ERR, FP8, MISALIGNED, NULL_POINTER,  # noqa: E402
                      MetaTensor as T, declared_parameters, host_calls)

BAD_FLAGS = FA_ERR["BAD_FLAGS"]
FORMS = [(False, False), (True, False), (False, True), (True, True)]


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    sp, vp, i = ctypes.POINTER(fa.FaStrides), ctypes.c_void_p, ctypes.c_int
    kinds = {"batchSize": i, "numHeads": i, "numHeadsKV": i, "seqLenNew": i, "totalQ": i, "seqLenK": i, "numPages": i, "pageSize": i,
             "maxPagesPerSeq": i, "tableStride": ctypes.c_int64, "dHead": i, "rotDim": i, "maxPos": i, "interleaved": i, "dtype": i,
             "kv_dtype": i, "sQ": sp, "sKnew": sp, "sVnew": sp, "sQout": sp, "sK": sp, "sV": sp}
    for form in FORMS:
        name, twin = call.ROPE[form], call.TWIN[form]
        assert name in fa.EXPORTS and getattr(L, name) is not None
        params = declared_parameters(name)
        assert list(getattr(L, name).argtypes) == [kinds.get(p, vp) for p in params], name
        assert getattr(L, name).restype is i
        # the twin's list with Q in front, Qout behind the new rows, cosSin behind the caches, numHeads behind batchSize, rotDim, maxPos
        # and interleaved behind dHead, sQ in front of the strides and sQout behind the new rows'
        want = declared_parameters(twin)
        for new, after in (("Q", None), ("Qout", "Vnew"), ("cosSin", "V"), ("numHeads", "batchSize"), ("rotDim", "dHead"), ("maxPos", "rotDim"),
                           ("interleaved", "maxPos"), ("sQ", "kv_dtype"), ("sQout", "sVnew")):
            want.insert(0 if after is None else [x.replace("pool", "") for x in want].index(after) + 1, new)
        assert params == want, name


def calls(kv):
    """the four calls on one aligned host pointer: keyword arguments override a call that is valid as a whole -- so every use below
    overrides something"""
    okc = dict(B=2, H=8, Hkv=2, Sq=3, Sk=1024, d=128, rot=64, maxpos=1024, il=0, dtype=BF16, kv=kv)
    okp = dict(B=2, H=8, Hkv=2, Sq=3, P=64, page=64, maxp=16, ts=16, d=128, rot=64, maxpos=1024, il=0, dtype=BF16, kv=kv)
    return host_calls(*((call.ROPE[paged, ragged], okp if paged else okc) for paged, ragged in FORMS))


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_what_the_twins_refuse_is_refused_with_the_same_codes(kv):
    *four, p = calls(kv)
    esz = 2 if kv == BF16 else 1
    for (paged, ragged), c in zip(FORMS, four):
        for name in ("Kn", "Vn", "K", "V"):
            assert c(**{name: None}) == NULL_POINTER, name
            assert c(**{name: p + 8}, d=96) == MISALIGNED, name
        assert c(lens=p + 2, d=96) == MISALIGNED and c(lens=p + 4, d=96) == BAD_DHEAD
        for name in ("kd", "vd"):
            assert c(**{name: p + 2}, d=96) == MISALIGNED, name
        for kw in (dict(Sq=0), dict(Sq=-1), dict(B=0), dict(Hkv=0), dict(d=0), dict(B=1 << 16, Hkv=1 << 15, H=1 << 15)):
            assert c(**kw) == BAD_SHAPE, kw
        assert c(Sq=1025, d=96) == (BAD_DHEAD if ragged else BAD_SHAPE)       # totalQ is not capped at the capacity
        for dt in (F32, FP8, F16, 9, -1):
            assert c(dtype=dt, d=96) == BAD_DTYPE, dt
        for other in (F32, F16, 9, -1):
            assert c(kv=other, d=96) == BAD_DTYPE, other
        if kv == BF16:
            assert c(kd=p, d=96) == BAD_DTYPE and c(vd=p + 4, d=96) == BAD_DTYPE
        else:
            assert c(kd=p, vd=p + 4, d=96) == BAD_DHEAD
        for d in (96, 32, 256, 120, 8):
            assert c(d=d) == BAD_DHEAD, d
        bad, mis = fa.FaStrides(1 << 20, 1 << 16, 56), fa.FaStrides(1 << 20, 1 << 16, 66)
        misH, neg = fa.FaStrides(1 << 20, (1 << 16) + 4, 64), fa.FaStrides(-(1 << 20), 1 << 16, 64)
        for at in range(6):                                   # sQ, sKnew, sVnew, sQout, sK, sV
            for s in (bad, mis, misH, neg):
                if s is neg and ragged and at < 4:
                    continue                                  # (strideB of the packed rows is not read)
                st = [None] * 6
                st[at] = ctypes.byref(s)
                assert c(strides=st, d=64, rot=64) == BAD_STRIDE, (at, s.strideS)
        if ragged:
            assert c(cu=None) == NULL_POINTER and c(cu=p + 2, d=96) == MISALIGNED and c(B=fa.FA_VARLEN_MAX_BATCH + 1) == BAD_SHAPE
        if paged:
            assert c(table=None) == NULL_POINTER and c(table=p + 2, d=96) == MISALIGNED
            for kw in (dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(ts=15), dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21, maxpos=1 << 25)):
                assert c(**kw) == BAD_SHAPE, kw
            assert c(page=(1 << 31) // (128 * esz), maxp=1, ts=1, maxpos=1 << 25) == BAD_SHAPE        # one page's extent
        else:
            for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1, maxpos=1 << 25)):
                assert c(**kw) == BAD_SHAPE, kw
            assert c(Sk=(1 << 31) // (128 * esz) - 192, maxpos=1 << 25) == BAD_SHAPE                   # one head's extent


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_new_refusals_in_ladder_order(kv):
    *four, p = calls(kv)
    low = fa.FaStrides(1 << 20, 1 << 16, 56)
    for (paged, ragged), c in zip(FORMS, four):
        # pointers: with the twin's NULL checks, before any alignment check; then 16 bytes, before the int32 / fp32 arrays and the shape
        for name in ("Q", "Qo", "cs"):
            assert c(**{name: None}) == NULL_POINTER, name
            assert c(**{name: None}, Kn=p + 8) == NULL_POINTER, name
            for off in (4, 8):
                assert c(**{name: p + off}) == MISALIGNED, (name, off)
            assert c(**{name: p + 8}, Sq=0) == MISALIGNED and c(**{name: p + 8}, lens=p + 2) == MISALIGNED
            if paged:
                assert c(**{name: p + 8}, page=24) == MISALIGNED
        # numHeads: with the shape, before the types and dHead
        for H in (0, -2, 7, 1, 9):
            assert c(H=H) == BAD_SHAPE and c(H=H, dtype=F32) == BAD_SHAPE and c(H=H, d=96) == BAD_SHAPE, H
        assert c(H=2, d=96) == BAD_DHEAD and c(H=64, d=96) == BAD_DHEAD          # one or many query heads per K/V head pass on
        # rotDim, maxPos, interleaved: after dHead and the types, before the strides and the extent
        for rot in (0, 8, 24, 72, 144, 256, -16):
            assert c(rot=rot) == BAD_SHAPE, rot
            assert c(rot=rot, d=96) == BAD_DHEAD and c(rot=rot, kv=F16) == BAD_DTYPE, rot
        assert c(d=64, rot=128) == BAD_SHAPE and c(d=64, rot=80) == BAD_SHAPE
        for rot in (16, 32, 128):
            assert c(rot=rot, il=2) == BAD_FLAGS, rot                            # every multiple of 16 up to dHead passes on
        for mp in (1023, 0, -1):
            assert c(maxpos=mp) == BAD_SHAPE and c(maxpos=mp, il=2) == BAD_SHAPE, mp
        assert c(maxpos=1 << 30, il=2) == BAD_FLAGS
        for il in (2, -1, 255):
            assert c(il=il) == BAD_FLAGS, il
            st = [ctypes.byref(low)] + [None] * 5
            assert c(il=il, strides=st) == BAD_FLAGS, il
        assert c(il=1, d=96) == BAD_DHEAD
        st = [ctypes.byref(low)] + [None] * 5
        big = dict(page=(1 << 31) // 128, maxp=1, ts=1, maxpos=1 << 25) if paged else dict(Sk=(1 << 31) // 128 - 192, maxpos=1 << 25)
        assert c(strides=st, **big) == BAD_STRIDE                               # Q's strides before the extent


def test_rope_table_is_the_float64_one_rounded_once():
    import math
    for max_pos, rot, base in ((7, 16, 10000.0), (130, 64, 500000.0), (33, 128, 10000.0)):
        t = fa.rope_table(max_pos, rot, base)
        assert t.shape == (max_pos, rot) and t.dtype == torch.float32 and t.is_contiguous()
        for p in (0, 1, max_pos // 2, max_pos - 1):
            for j in (0, 1, rot // 4, rot // 2 - 1):
                a = p * base ** (-2.0 * j / rot)
                # (math.cos of the float64 angle, rounded once: one fp32 ulp of slack for the last bit of the library functions)
                assert abs(float(t[p, j]) - math.cos(a)) <= 2.0 ** -23 and abs(float(t[p, rot // 2 + j]) - math.sin(a)) <= 2.0 ** -23, (p, j)
        assert torch.equal(t[0, :rot // 2], torch.ones(rot // 2)) and torch.equal(t[0, rot // 2:], torch.zeros(rot // 2))
    for bad in ((0, 16), (8, 15), (8, 0)):
        with pytest.raises(ValueError):
            fa.rope_table(*bad)


def test_binding_refusals():
    f8, bf = torch.float8_e4m3fn, torch.bfloat16
    q, new = torch.zeros(2, 4, 3, 64, dtype=bf), torch.zeros(2, 2, 3, 64, dtype=bf)
    k, k8 = torch.zeros(2, 2, 32, 64, dtype=bf), torch.zeros(2, 2, 32, 64, dtype=f8)
    pool = torch.zeros(6, 2, 16, 64, dtype=bf)
    table = torch.zeros(2, 2, dtype=torch.int32)
    cs = torch.zeros(32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.rope_cache_append(q, new, new, k, k, cs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.rope_cache_append_paged(q, new, new, pool, pool, table, cs)

    def both(Q, Kn, Vn, table_=table, cos_sin=cs, K=k, Kp=pool, **kw):
        yield lambda: fa.rope_cache_append(T(Q), T(Kn), T(Vn), T(K), T(K), T(cos_sin), **kw)
        yield lambda: fa.rope_cache_append_paged(T(Q), T(Kn), T(Vn), T(Kp), T(Kp), T(table_), T(cos_sin), **kw)

    # Q: [B, H, Sq, d] of the new rows' dtype, Hkv dividing H
    for Q in (q[:1], q[:, :3], q[:, :, :2], q[..., :32], q[0], q.half()):
        for c in both(Q, new, new):
            with pytest.raises(ValueError, match="Q must be"):
                c()
    # the new rows and the caches: the append fronts' checks
    for c in both(q, new, new[:, :, :2]):
        with pytest.raises(ValueError):
            c()
    for Sq in (0, 33):
        n, qq = torch.zeros(2, 2, Sq, 64, dtype=bf), torch.zeros(2, 4, Sq, 64, dtype=bf)
        for c in both(qq, n, n):
            with pytest.raises(ValueError, match="new rows"):
                c()
    for c in both(q, new, new, K=k.float(), Kp=pool.float()):
        with pytest.raises(TypeError, match="share a dtype"):
            c()
    # the table: dense fp32 [max_pos, rot_dim] on Q's device, rot_dim a multiple of 16 up to d, max_pos at least the capacity
    for bad in (cs.double(), torch.zeros(32, 64)[:, ::2], torch.zeros(32), torch.zeros(32, 24), torch.zeros(32, 80), torch.zeros(31, 32), T(cs, device="cpu")):
        for call_ in (lambda: fa.rope_cache_append(T(q), T(new), T(new), T(k), T(k), bad if isinstance(bad, T) else T(bad)),
                      lambda: fa.rope_cache_append_paged(T(q), T(new), T(new), T(pool), T(pool), T(table), bad if isinstance(bad, T) else T(bad))):
            with pytest.raises(ValueError, match="cos_sin"):
                call_()
    with pytest.raises(ValueError, match="cos_sin"):
        fa.rope_cache_append(T(q), T(new), T(new), T(k), T(k), cs)              # not on a device
    # Q_out: shaped like Q, its dtype
    for out in (T(q[:, :2]), T(q.half()), q):
        with pytest.raises(ValueError, match="Q_out"):
            fa.rope_cache_append(T(q), T(new), T(new), T(k8), T(k8), T(cs), Q_out=out)
    # lengths and descales: the append fronts' texts
    with pytest.raises(ValueError, match="kv_lens"):
        fa.rope_cache_append(T(q), T(new), T(new), T(k), T(k), T(cs), kv_lens=T(torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="descale"):
        fa.rope_cache_append(T(q), T(new), T(new), T(k), T(k), T(cs), k_descale=T(torch.ones(2)))
    # the ragged fronts: packed by token, cu_seqlens_q
    qt, nt = torch.zeros(5, 4, 64, dtype=bf), torch.zeros(5, 2, 64, dtype=bf)
    cu = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="packed by token"):
        fa.rope_cache_append_varlen(T(qt), T(new), T(new), T(k), T(k), T(cu), T(cs))
    with pytest.raises(ValueError, match="packed by token"):
        fa.rope_cache_append_varlen(T(q), T(nt), T(nt), T(k), T(k), T(cu), T(cs))
    with pytest.raises(ValueError, match="cu_seqlens_q"):
        fa.rope_cache_append_varlen(T(qt), T(nt), T(nt), T(k), T(k), T(cu.long()), T(cs))
    with pytest.raises(ValueError, match="Q must be"):
        fa.rope_cache_append_paged_varlen(T(qt[:4]), T(nt), T(nt), T(pool), T(pool), T(table), T(cu), T(cs))
