"""GPU: the memory rules of tests/test_memory_contract.py on the two MLA decode entry points (flash_attention_mla_decode,
flash_attention_mla_decode_paged): every tensor of the call carved out of one guarded arena of 0xFF bytes (tests/arena.py), at both
placements -- `aligned`, everything at 0 mod 512, and `offset`, tensors at 16 mod 256 and the side inputs, ``kvLens`` and the block
table, at 4 mod 16 -- with the workspace entering as NaNs at exactly the stated size, flash_attention_mla_decode_workspace_size at the
plan's num_splits.  The result must be the run on plain allocations bit for bit, the arena untouched outside O, the LSE and the
workspace, and the result is also held to the float64 reference (mla_check.py; kv_cache_check.assert_close, unchanged).  The calls go
through the C ABI by name (mla_check.c_call); the placements and the arena are memory_contract.py's."""
import ctypes

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import kv_cache_check as kv  # noqa: E402
import memory_contract as mem  # noqa: E402
import mla_check as mc  # noqa: E402
from memory_contract import CODE, bf, f32, i32, spec  # noqa: E402

pytestmark = pytest.mark.gpu
B, H, SQ = 3, 13, 5                 # 65 packed rows: two row blocks, head 12 across the seam
LENS = [129, 384, 3]
WIDE = 3                            # the page-16 table is a row slice of one this much wider


def mla_call(Q, KV, page, lens, causal, ns, odt):
    """the tensors of one MLA call and the C entry point on them; kvLens and the table are side inputs.  The plan is asserted: a forced
    count is taken, and the workspace is the stated size at the plan's count"""
    plan = fa.mla_decode_plan(B, H, SQ, mc.CAPACITY, CODE[odt], ns)
    assert ns == 0 or plan["num_splits"] == ns
    data = dict(Q=Q, lens=torch.tensor(lens, dtype=i32))
    if page:
        table = mc.table_for(B, page, 1800 + page)
        data["KV"] = mc.pool_of(KV, table, page)
        data["table"] = torch.cat([table, torch.full((B, WIDE), 2 ** 31 - 1, dtype=i32)], 1) if page == 16 else table
    else:
        data["KV"] = KV
    specs = {n: spec(t.shape, t.dtype, side=n in ("lens", "table")) for n, t in data.items()}
    specs.update(O=spec((B, H, SQ, mc.DL), odt, True), lse=spec((B, H, SQ), f32, True))
    name = mc.SYMBOLS[bool(page)]

    def go(v):
        keep = [fa.FaStrides(*v["Q"].stride()[:3]), fa.FaStrides(v["KV"].stride(0), 0, v["KV"].stride(1)), fa.FaStrides(*v["O"].stride()[:3])]
        values = dict(Q=v["Q"].data_ptr(), KV=v["KV"].data_ptr(), O=v["O"].data_ptr(), LSE=v["lse"].data_ptr(), lens=v["lens"].data_ptr(),
                      ws=mem.ptr(v, "ws"), B=B, H=H, Sq=SQ, dl=mc.DL, dr=mc.DR, scale=mc.DEFAULT_SCALE, causal=causal, dtype=fa.FA_DTYPE_BF16,
                      o=CODE[odt], ns=plan["num_splits"], sQ=ctypes.byref(keep[0]), sKV=ctypes.byref(keep[1]), sO=ctypes.byref(keep[2]),
                      stream=mem.stream())
        if page:
            values.update(table=v["table"].data_ptr(), P=v["KV"].shape[0], page=page, maxp=mc.CAPACITY // page, ts=v["table"].shape[1])
        else:
            values.update(Sk=mc.CAPACITY)
        rc = mc.c_call(name, values)
        assert rc == 0, (name, fa.error_string(rc))

    need = int(fa.lib().flash_attention_mla_decode_workspace_size(B, H, SQ, mc.DL, plan["num_splits"]))
    assert need == fa.decode_workspace_size(B, H, SQ, mc.DL, plan["num_splits"])
    return mem.Call(specs, data, go, ["O", "lse"], need, f"{name} page {page} causal {causal} splits {ns} O {odt}")


@pytest.mark.parametrize("page", [0, 16, 128])
def test_mla_calls(page):
    Q, KV = mc.data(H, SQ, 1810 + page)
    for causal, ns, odt in ((True, 1, f32), (False, 3, bf), (True, 0, f32)):
        refO, refL = mc.reference(Q, KV, LENS, causal)
        call = mla_call(Q, KV, page, LENS, causal, ns, odt)
        assert (call.ws_bytes > 0) == (ns != 1)
        _, plain = mem.run(call, None)
        for placement in mem.PLACEMENTS:
            arena, got = mem.run(call, placement)
            if placement == "offset":
                for n in ("lens",) + (("table",) if page else ()):
                    assert got[n].data_ptr() % 16 == 4, n
            if call.ws_bytes:
                assert got["ws"].numel() == call.ws_bytes
            for n in call.outs:
                assert mem.same(got[n], plain[n]), f"{call.note} [{placement}]: {n} differs from the run on plain allocations"
            arena.check()
            if odt == f32:      # (a BF16 O is the F32 one rounded once: tests/test_mla_decode.py; here it is held to the plain run's bits)
                kv.assert_close(got["O"], got["lse"], refO, refL, f"{call.note} [{placement}]")
            else:
                assert (kv.lse_ratio(got["lse"].cpu(), refL) <= 1).all(), f"{call.note} [{placement}]"
