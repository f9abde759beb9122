"""CPU tests of the fp8 latent cache at the C ABI: the four signatures by name, the fp8 decode ladder beside the bf16
call's and the append ladder beside flash_attention_kv_append's with the new refusals at their places, the fronts' refusals.  Fake
aligned host pointers: no call here is valid as a whole (a valid append would launch on host memory), no GPU is touched."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, aligned_host_pointer, declared_parameters)

DECODE = {"flash_attention_mla_decode_fp8": "flash_attention_mla_decode", "flash_attention_mla_decode_paged_fp8": "flash_attention_mla_decode_paged"}
APPEND = {"flash_attention_mla_append": "flash_attention_kv_append", "flash_attention_mla_append_paged": "flash_attention_kv_append_paged"}
HOST = aligned_host_pointer()
P = HOST[1]
by_name = lambda symbol, v: getattr(fa.lib(), symbol)(*[v[n] for n in declared_parameters(symbol)])   # (other keys are the siblings')
S = lambda b, s: ctypes.byref(fa.FaStrides(b, 0, s))


def test_the_four_symbols_are_exported_with_the_declared_signatures():
    for paged in (False, True):
        mine, twin = declared_parameters(fa._MLA_FP8_SYMBOLS[paged]), declared_parameters(fa._MLA_SYMBOLS[paged])
        assert [n for n in mine if n not in ("kvDescale", "kv_dtype")] == twin      # the twin's list with the two additions ...
        assert mine[mine.index("kvDescale") - 1] == ("blockTable" if paged else "kvLens") and mine[mine.index("kv_dtype") - 1] == "dtype"
        geometry = ["numPages", "pageSize", "maxPagesPerSeq", "tableStride"] if paged else ["seqLenK"]
        assert declared_parameters(fa._MLA_APPEND_SYMBOLS[paged]) == ["Cnew", "Rnew", "KVpool" if paged else "KV", "kvLens"] + ["blockTable"] * paged \
            + ["kvDescale", "batchSize", "seqLenNew"] + geometry + ["dLatent", "dRope", "dtype", "kv_dtype", "sC", "sR", "sKV", "stream"]
        for name in (fa._MLA_FP8_SYMBOLS[paged], fa._MLA_APPEND_SYMBOLS[paged]):
            fn = getattr(fa.lib(), name)
            assert name in fa.EXPORTS and name in {**DECODE, **APPEND} and fn.restype is ctypes.c_int
            assert len(fn.argtypes) == len(declared_parameters(name)) and fn.argtypes[-1] is ctypes.c_void_p
    # the plan does not know the cache's type: one plan, one workspace size for both
    assert not {"kv_dtype", "kvDescale"} & set(declared_parameters("flash_attention_mla_decode_plan")
                                              + declared_parameters("flash_attention_mla_decode_workspace_size"))


# valid but for the workspace (two forced splits): a call that passes every other check ends at NULL_POINTER
OK = dict(Q=P, KV=P, KVpool=P, O=P, LSE=None, kvLens=None, blockTable=P, kvDescale=None, workspace=None, batchSize=2, numHeads=8, seqLenQ=4,
          seqLenK=1024, numPages=64, pageSize=64, maxPagesPerSeq=16, tableStride=16, dLatent=512, dRope=64, scale=0.125, is_causal=True,
          dtype=BF16, kv_dtype=FP8, o_dtype=F32, numSplits=2, sQ=None, sKV=None, sO=None, stream=None)
LADDER = [dict(), dict(Q=None), dict(KV=None, KVpool=None), dict(Q=P + 8), dict(LSE=P + 4), dict(workspace=P + 8), dict(kvLens=P + 2, seqLenQ=0),
          dict(blockTable=P + 2, seqLenK=0), dict(seqLenQ=17), dict(batchSize=0), dict(numSplits=CAP + 1), dict(seqLenK=0, pageSize=24),
          dict(seqLenK=(1 << 24) + 1, tableStride=15), dict(o_dtype=FP8), dict(dtype=F32), dict(dtype=FP8), dict(dtype=F32, numSplits=-1),
          dict(o_dtype=7, scale=0.0), dict(dLatent=256), dict(dLatent=0), dict(dLatent=256, dtype=F32), dict(dRope=32, scale=0.0), dict(scale=0.0),
          dict(scale=float("nan")), dict(sQ=S(64, 8)), dict(sQ=S(64, 8), scale=0.0), dict(sO=S(1 << 20, 504)), dict(sKV=S(1 << 20, 575)),
          dict(sKV=S(1 << 20, 1 << 25), workspace=P), dict(numSplits=1, Q=None), dict(batchSize=1 << 18, numHeads=1, seqLenQ=1, numSplits=64, workspace=P)]


@pytest.mark.parametrize("name", DECODE)
def test_decode_refuses_what_its_bf16_twin_refuses_and_its_own_at_their_places(name):
    call, twin = (lambda **kw: by_name(name, dict(OK, **kw))), (lambda **kw: by_name(DECODE[name], dict(OK, **kw)))
    for kw in LADDER:
        assert NULL_POINTER >= twin(**kw) >= BAD_STRIDE and call(**kw) == twin(**kw), kw
    # the cache's type: fp8 only, asked first (as flash_attention_decode_fp8 asks it); Q stays bf16
    assert all(call(kv_dtype=t) == call(kv_dtype=t, Q=None) == BAD_DTYPE for t in (BF16, F32, F16, 7))
    # kvDescale: 4-byte aligned, beside kvLens -- behind the pointers, ahead of the shape
    assert call(kvDescale=P + 4) == NULL_POINTER and call(kvDescale=P + 2) == call(kvDescale=P + 2, seqLenQ=0) == MISALIGNED
    assert call(kvDescale=P + 2, Q=None) == NULL_POINTER
    # sKV counts bytes: multiples of 16 (584 elements are 16-byte rows in bf16 only), behind the scale
    assert call(sKV=S(1 << 20, 584)) == call(sKV=S(1000, 576)) == BAD_STRIDE and twin(sKV=S(1 << 20, 584)) == NULL_POINTER
    assert call(sKV=S(1 << 20, 584), scale=0.0) == BAD_SCALE and call(sKV=S(1 << 20, 592)) == NULL_POINTER
    # the extent (contiguous: capacity + 192 rows; paged: one page) at one byte per element: twice the bf16 call's row stride
    s = 1 << (24 if "paged" in name else 20)
    assert call(sKV=S(0, s)) == NULL_POINTER and twin(sKV=S(0, s)) == BAD_SHAPE and call(sKV=S(0, 2 * s)) == BAD_SHAPE


AOK = dict(Cnew=P, Rnew=P, KV=P, KVpool=P, Knew=P, Vnew=P, K=P, V=P, Kpool=P, Vpool=P, kvLens=None, blockTable=P, kvDescale=None, kDescale=None,
           vDescale=None, batchSize=2, numHeadsKV=1, seqLenNew=4, seqLenK=1024, numPages=64, pageSize=64, maxPagesPerSeq=16, tableStride=16,
           dLatent=512, dRope=64, dHead=128, dtype=BF16, kv_dtype=FP8, sC=None, sR=None, sKV=None, sKnew=None, sVnew=None, sK=None, sV=None,
           stream=None)
# (what refuses the MLA call, what refuses the twin the same way)
APPEND_LADDER = [(dict(Cnew=None), dict(Knew=None)), (dict(Rnew=None), dict(Vnew=None)), (dict(KV=None, KVpool=None), dict(K=None, Kpool=None)),
                 (dict(blockTable=None, KV=None), dict(blockTable=None, K=None)), (dict(Rnew=P + 8), dict(Vnew=P + 8)),
                 (dict(KV=P + 4, KVpool=P + 4), dict(V=P + 4, Vpool=P + 4)), (dict(kvLens=P + 2, seqLenNew=0),) * 2,
                 (dict(kvDescale=P + 2), dict(kDescale=P + 2)), (dict(kvDescale=P + 2, Cnew=None), dict(vDescale=P + 2, Knew=None)),
                 (dict(seqLenNew=0),) * 2, (dict(seqLenNew=1025),) * 2, (dict(batchSize=0),) * 2, (dict(seqLenK=0, pageSize=8),) * 2,
                 (dict(seqLenK=(1 << 24) + 1, maxPagesPerSeq=17),) * 2, (dict(seqLenNew=0, dtype=F32),) * 2, (dict(dtype=F32),) * 2,
                 (dict(kv_dtype=F16),) * 2, (dict(kv_dtype=BF16, kvDescale=P), dict(kv_dtype=BF16, kDescale=P)), (dict(dLatent=0), dict(dHead=0)),
                 (dict(dLatent=256), dict(dHead=96)), (dict(dRope=32), dict(dHead=96)), (dict(dLatent=64, dRope=512), dict(dHead=96)),
                 (dict(dLatent=256, dtype=F32), dict(dHead=96, dtype=F32)), (dict(dLatent=256, sC=S(64, 8)), dict(dHead=96, sKnew=S(64, 8))),
                 (dict(sC=S(1 << 20, 504)), dict(sKnew=S(1 << 20, 120))), (dict(sC=S(1 << 20, 516)), dict(sKnew=S(1 << 20, 132))),
                 (dict(sR=S(1 << 20, 56)), dict(sVnew=S(1 << 20, 120))), (dict(sR=S(1001, 64)), dict(sVnew=S(1001, 128))),
                 (dict(sKV=S(1 << 20, 584)), dict(sK=S(1 << 20, 136))), (dict(sKV=S(0, 1 << 26)), dict(sK=S(0, 1 << 26)))]


@pytest.mark.parametrize("name", APPEND)
def test_the_append_ladder_is_kv_appends_with_the_widths_at_the_place_of_dhead(name):
    seen = set()
    for mine, twins in APPEND_LADDER:
        want = by_name(APPEND[name], dict(AOK, **twins))
        assert NULL_POINTER >= want >= BAD_STRIDE and by_name(name, dict(AOK, **mine)) == want, (mine, want)
        seen.add(want)
    assert seen == {NULL_POINTER, MISALIGNED, BAD_SHAPE, BAD_DTYPE, BAD_DHEAD, BAD_STRIDE}


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    bf, f8 = torch.bfloat16, torch.float8_e4m3fn
    q, kv, one = torch.zeros(2, 8, 3, 576, dtype=bf), torch.zeros(2, 64, 576, dtype=bf), torch.ones(1)
    pool, table = torch.zeros(9, 16, 576, dtype=bf), T(torch.zeros(2, 3, dtype=torch.int32))
    c, r = torch.zeros(2, 3, 512, dtype=bf), torch.zeros(2, 3, 64, dtype=bf)
    fronts = {(False, kv): lambda **kw: fa.flash_attention_mla_decode(kw.pop("Q", T(q)), kw.pop("KV", T(kv.to(f8))), **kw),
              (False, pool): lambda **kw: fa.flash_attention_mla_decode_paged(kw.pop("Q", T(q)), kw.pop("KV", T(pool.to(f8))), table, **kw),
              (True, kv): lambda **kw: fa.mla_cache_append(kw.pop("c", T(c)), kw.pop("r", T(r)), kw.pop("KV", T(kv.to(f8))), **kw),
              (True, pool): lambda **kw: fa.mla_cache_append_paged(kw.pop("c", T(c)), kw.pop("r", T(r)), kw.pop("KV", T(pool.to(f8))), table, **kw)}
    for (write, cache), front in fronts.items():
        with pytest.raises(ValueError, match="kv_descale belongs to an fp8"):          # a bf16 cache has no descale
            front(KV=T(cache), kv_descale=T(one))
        for bad in (one, T(one.double()), T(torch.ones(2)), T(one, device="cuda:1")):
            with pytest.raises(ValueError, match="kv_descale must be an fp32 tensor of one element"):
                front(kv_descale=bad)
        if not write:                                                                  # an fp8 cache under a Q that is not bf16
            with pytest.raises(TypeError, match="Q, KV must share a dtype"):
                front(Q=T(q.float()))
            continue
        for kw in (dict(c=T(torch.zeros(2, 3, 576, dtype=bf))), dict(r=T(torch.zeros(2, 4, 64, dtype=bf))), dict(KV=T(torch.zeros(2, 64, 512, dtype=bf)))):
            with pytest.raises(ValueError, match=r"c_kv must be \[B, Sq, 512\], k_pe \[B, Sq, 64\]"):
                front(**kw)
        for kw in (dict(c=T(c.float())), dict(r=T(r.half())), dict(KV=T(cache.half()))):
            with pytest.raises(TypeError, match="c_kv, k_pe must be bfloat16"):
                front(**kw)
        with pytest.raises(ValueError, match="Sq = 65 new rows: must be 1 .. the capacity"):
            front(c=T(torch.zeros(2, 65, 512, dtype=bf)), r=T(torch.zeros(2, 65, 64, dtype=bf)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.mla_cache_append(c, r, kv)
