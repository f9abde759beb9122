"""GPU: the memory rules of tests/test_mla_memory_contract.py on the four sparse MLA entry points (flash_attention_mla_sparse_decode,
_paged, _fp8, _paged_fp8), one case per cache form: every tensor of the call carved out of one guarded arena of 0xFF bytes
(tests/arena.py) at the `offset` placement -- tensors at 16 mod 256, the side inputs (``indices`` among them, with ``kvLens``, the table
and the descale) at 4 mod 16 -- with the workspace entering as NaNs at exactly the stated size.  The result must be the run on plain
allocations bit for bit and the arena untouched outside O, the LSE and the workspace.  Through the C ABI by name."""
import ctypes

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import memory_contract as mem  # noqa: E402
import mla_check as mc  # noqa: E402
import mla_sparse_check as sc  # noqa: E402
from memory_contract import CODE, f32, i32, spec  # noqa: E402

pytestmark = pytest.mark.gpu
B, H, SQ, TOPK, NS = 3, 65, 2, 96, 3
LENS = [129, 384, 40]


@pytest.mark.parametrize("fp8,page", [(False, 0), (False, 16), (True, 0), (True, 128)])
def test_sparse_mla_calls(fp8, page):
    Q, KV = mc.data(H, SQ, 6700 + page)
    c = sc.Cache(KV, fp8, page, seed=6701)
    idx = sc.index_lists(SQ, TOPK, LENS, 6702)
    assert fa.mla_sparse_plan(B, H, SQ, TOPK, CODE[f32], NS)["num_splits"] == NS
    cache = c.pool if page else c.stored
    data = dict(Q=Q, KV=cache.view(mem.F8) if fp8 else cache, lens=torch.tensor(LENS, dtype=i32), idx=idx)
    if page:
        data["table"] = c.table
    if fp8:
        data["ds"] = c.ds.reshape(1)
    specs = {n: spec(t.shape, t.dtype, side=n in ("lens", "idx", "table", "ds")) for n, t in data.items()}
    specs.update(O=spec((B, H, SQ, mc.DL), f32, True), lse=spec((B, H, SQ), f32, True))
    name = sc.symbol(fp8, page)

    def go(v):
        keep = [fa.FaStrides(*v["Q"].stride()[:3]), fa.FaStrides(v["KV"].stride(0), 0, v["KV"].stride(1)), fa.FaStrides(*v["O"].stride()[:3])]
        rc = sc.c_call(name, Q=v["Q"].data_ptr(), KV=v["KV"].data_ptr(), KVpool=v["KV"].data_ptr(), O=v["O"].data_ptr(), LSE=v["lse"].data_ptr(),
                       kvLens=v["lens"].data_ptr(), indices=v["idx"].data_ptr(), topk=TOPK, indexStrideB=SQ * TOPK, indexStrideQ=TOPK,
                       blockTable=mem.ptr(v, "table"), kvDescale=mem.ptr(v, "ds"), workspace=mem.ptr(v, "ws"), batchSize=B, numHeads=H,
                       seqLenQ=SQ, seqLenK=mc.CAPACITY, numPages=v["KV"].shape[0], pageSize=page, maxPagesPerSeq=mc.CAPACITY // (page or 1),
                       tableStride=mc.CAPACITY // (page or 1), dLatent=mc.DL, dRope=mc.DR, scale=mc.DEFAULT_SCALE, is_causal=True,
                       dtype=fa.FA_DTYPE_BF16, kv_dtype=fa.FA_DTYPE_FP8_E4M3, o_dtype=CODE[f32], numSplits=NS, sQ=ctypes.byref(keep[0]),
                       sKV=ctypes.byref(keep[1]), sO=ctypes.byref(keep[2]), stream=mem.stream())
        assert rc == 0, (name, fa.error_string(rc))

    need = int(fa.lib().flash_attention_mla_decode_workspace_size(B, H, SQ, mc.DL, NS))
    call = mem.Call(specs, data, go, ["O", "lse"], need, f"{name} page {page}")
    _, plain = mem.run(call, None)
    arena, got = mem.run(call, "offset")
    assert got["idx"].data_ptr() % 16 == 4 and got["ws"].numel() == need > 0
    for n in call.outs:
        assert mem.same(got[n], plain[n]), f"{call.note}: {n} differs from the run on plain allocations"
    arena.check()
    sc.assert_close(got["O"], got["lse"], *sc.reference(Q, c.logical, idx, LENS, True), call.note)
