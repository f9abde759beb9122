"""CPU tests of the packed latent row at the C ABI and in the binding: the signatures, the read and write ladders
code for code beside their twins', the new refusals at their places, the fronts' refusals.  Fake host pointers: no GPU is touched."""
import ctypes

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, F32, FA_ERR, NULL_POINTER, MetaTensor as T,  # noqa: E402
                      declared_parameters)
from mla_sparse_check import c_call  # noqa: E402
from test_mla_abi import ladder  # noqa: E402
from test_mla_fp8_abi import AOK, APPEND_LADDER  # noqa: E402
from test_mla_sparse_abi import calls  # noqa: E402

READ = {fa._MLA_PACKED_SYMBOLS[paged]: fa._MLA_SPARSE_SYMBOLS[True][paged] for paged in (False, True)}
WRITE = {fa._MLA_APPEND_PACKED_SYMBOLS[paged]: fa._MLA_APPEND_SYMBOLS[paged] for paged in (False, True)}
S = lambda b, s: ctypes.byref(fa.FaStrides(b, 0, s))
BAD_ROWS = (S(1 << 20, 655), S(1 << 20, 640), S(1 << 20, 664), S(1000, 656))      # sKV in bytes: a row >= 656 and a multiple of 16


@pytest.mark.parametrize("name", READ)
def test_the_read_ladder_is_the_fp8_sparse_calls_and_the_row_stride_is_656_bytes(name):
    (call, p), (twin, _) = calls(name), calls(READ[name])
    assert name in fa.EXPORTS and declared_parameters(name) == [n for n in declared_parameters(READ[name]) if n not in ("kvDescale", "kv_dtype")]
    assert call() == twin() == NULL_POINTER                                              # valid but for the workspace
    for kw in ladder(p, "paged" in name) + [dict(indices=None), dict(indices=p + 2), dict(topk=0, ws=p), dict(indexStrideQ=63, scale=0.0)]:
        assert call(**kw) == twin(**kw), kw
    for bad in BAD_ROWS:                 # with the strides: behind the dtype and the scale, ahead of the extent and the workspace
        assert call(sKV=bad) == call(sKV=bad, ws=p) == BAD_STRIDE and call(sKV=bad, scale=0.0) == BAD_SCALE and call(sKV=bad, dtype=F32) == BAD_DTYPE
    assert call(sKV=S(1 << 20, 656)) == call(sKV=S(1 << 20, 672)) == twin(sKV=S(1 << 20, 640)) == NULL_POINTER


@pytest.mark.parametrize("name", WRITE)
def test_the_write_ladder_is_mla_appends_with_scalefmt_where_the_cache_type_stands(name):
    theirs = [("scaleFmt" if n == "kvDescale" else n) for n in declared_parameters(WRITE[name]) if n != "kv_dtype"]
    assert name in fa.EXPORTS and declared_parameters(name) == theirs
    call, twin = (lambda **kw: c_call(name, **{**AOK, "scaleFmt": 1, **kw})), (lambda **kw: c_call(WRITE[name], **{**AOK, **kw}))
    for mine, _ in APPEND_LADDER:
        if not {"kvDescale", "kv_dtype", "sKV"} & set(mine):
            assert call(**mine) == twin(**mine), mine
    for fmt in (-1, 2):                  # outside the enum, where kv_dtype is asked: behind the shapes and dtype, ahead of widths and strides
        assert call(scaleFmt=fmt) == call(scaleFmt=fmt, dLatent=256) == call(scaleFmt=fmt, sC=S(64, 8)) == FA_ERR["BAD_FLAGS"]
        assert call(scaleFmt=fmt, dtype=F32) == BAD_DTYPE and call(scaleFmt=fmt, seqLenNew=0) == BAD_SHAPE
    assert all(call(sKV=bad) == BAD_STRIDE for bad in BAD_ROWS) and call(sKV=S(0, 1 << 26)) == BAD_SHAPE


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    bf, u8 = torch.bfloat16, torch.uint8
    q, kv, pool = T(torch.zeros(2, 8, 3, 576, dtype=bf)), torch.zeros(2, 64, 656, dtype=u8), torch.zeros(9, 16, 656, dtype=u8)
    table, idx = T(torch.zeros(2, 3, dtype=torch.int32)), T(torch.zeros(2, 3, 40, dtype=torch.int32))
    c, r = T(torch.zeros(2, 3, 512, dtype=bf)), T(torch.zeros(2, 3, 64, dtype=bf))
    fronts = [(kv, lambda KV, **kw: fa.flash_attention_mla_sparse_decode_packed(q, KV, idx, **kw)),
              (pool, lambda KV, **kw: fa.flash_attention_mla_sparse_decode_paged_packed(q, KV, table, idx, **kw)),
              (kv, lambda KV, **kw: fa.mla_cache_append_packed(c, r, KV, **kw)),
              (pool, lambda KV, **kw: fa.mla_cache_append_paged_packed(c, r, KV, table, **kw))]
    for n, (cache, front) in enumerate(fronts):
        for error, match, KV in [(RuntimeError, "no CPU fallback", cache), (ValueError, "656", T(cache[..., :640])),
                                 (TypeError, "uint8", T(cache.view(torch.float8_e4m3fn))), (TypeError, "uint8", T(cache.to(bf))),
                                 (ValueError, "last dimension must be contiguous", T(torch.zeros(*cache.shape[:2], 1312, dtype=u8)[..., ::2]))]:
            with pytest.raises(error, match=match):
                front(KV)
        if n >= 2:
            with pytest.raises(ValueError, match="scale_fmt must be 'f32' or 'pow2'"):
                front(T(cache), scale_fmt="e8m0")
