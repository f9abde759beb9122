"""GPU: the memory rules of tests/test_memory_contract.py on the six attention-sink entry points (flash_attention_sink_decode,
_decode_paged, _extend, _extend_paged, _extend_varlen, _extend_paged_varlen): every tensor of the call carved out of one guarded arena of
0xFF bytes (tests/arena.py), at both placements -- `aligned`, everything at 0 mod 512, and `offset`, tensors at 16 mod 256 and the side
inputs at 4 mod 16, the ``sinks`` array among them -- with the workspace entering as NaNs at exactly its stated size.  The result must be
the run on plain allocations bit for bit, the arena untouched outside O, the LSE and the workspace, and the result is also held to the
float64 reference with sinks (sink_check.py; kv_cache_check.assert_close, unchanged).  One split (the split kernel's SINK form reads the
array) and three (the combine's does).  The calls, the placements and the arena are memory_contract.py's, imported."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import kv_cache_check as kv  # noqa: E402
import memory_contract as mc  # noqa: E402
import sink_check as sc  # noqa: E402
from memory_contract import f32  # noqa: E402

pytestmark = pytest.mark.gpu
LENS = [129, 300]
H = mc.HKV * mc.G
assert (mc.HKV, mc.CAPACITY, len(LENS)) == (sc.HKV, sc.CAP, sc.B)


def sink_call(family, cache, Q, lens, causal, ns, W, sinks, cu=None):
    """memory_contract.split_kv_call's tensors plus ``sinks`` as a side input, through the family's flash_attention_sink_* entry point"""
    call = mc.split_kv_call(family, cache, Q, lens, causal, ns, W, cu=cu, sink=True)
    call.specs["sinks"], call.data["sinks"] = mc.spec((H,), f32, side=True), sinks
    return call


@pytest.mark.parametrize("page,fp8", [(None, False), (16, False), (None, True), (128, True)])
@pytest.mark.parametrize("family,d,rows", [("decode", 64, 5), ("decode", 128, 16), ("extend", 64, 40), ("extend", 128, 17)])
def test_sink_calls_uniform(family, d, rows, page, fp8):
    cache = mc.Cache(len(LENS), d, page, fp8, seed=1200 + d + (page or 0) + 7 * fp8)
    Q = mc.randn((len(LENS), H, rows, d), 1201 + rows)
    sinks = sc.sinks_for(H)
    for (causal, W), ns in ((c, n) for c in ((True, 0), (False, 130)) for n in (1, 3)):
        refO, refL, _, _ = sc.reference_sinks(Q, cache.refK, cache.refV, LENS, causal, W, sinks)
        call = sink_call(family, cache, Q, LENS, causal, ns, W, sinks)
        assert call.ws_bytes == fa.decode_workspace_size(len(LENS), H, rows, d, ns) and (call.ws_bytes > 0) == (ns > 1)
        _, plain = mc.run(call, None)
        for placement in mc.PLACEMENTS:
            arena, got = mc.run(call, placement)
            if placement == "offset":
                assert got["sinks"].data_ptr() % 16 == 4
            for n in call.outs:
                assert mc.same(got[n], plain[n]), f"{call.note} [{placement}]: {n} differs from the run on plain allocations"
            arena.check()
            kv.assert_close(got["O"], got["lse"], refO, refL, f"{call.note} [{placement}]")


@pytest.mark.parametrize("page,fp8", [(None, False), (16, False), (None, True), (128, True)])
@pytest.mark.parametrize("d", [64, 128])
def test_sink_calls_ragged(d, page, fp8):
    """rows (5, 130) and 23 rows behind them that no sequence owns: those must come back as the 0xFF they went in as"""
    rows, unowned = (5, 130), 23
    cache = mc.Cache(len(LENS), d, page, fp8, seed=1250 + d + (page or 0) + 7 * fp8)
    cu = kv.cu_of(rows)
    T = cu[-1] + unowned
    Q = mc.randn((T, H, d), 1251 + d)
    sinks = sc.sinks_for(H)
    for (causal, W), ns in ((c, n) for c in ((True, 0), (False, 130)) for n in (1, 3)):
        refO, refL, owned = kv.reference_ragged(Q, cache.refK, cache.refV, rows, LENS, causal, W, sinks)
        assert int(owned.sum()) == cu[-1] and not bool(owned[cu[-1]:].any())
        call = sink_call("varlen", cache, Q, LENS, causal, ns, W, sinks, cu=cu)
        assert call.ws_bytes == fa.decode_workspace_size(1, H, T, d, ns)
        _, plain = mc.run(call, None)
        assert not plain["O"][cu[-1]:].any() and not plain["lse"][:, cu[-1]:].any()
        for placement in mc.PLACEMENTS:
            arena, got = mc.run(call, placement)
            assert mc.same(got["O"][:cu[-1]], plain["O"][:cu[-1]]) and mc.same(got["lse"][:, :cu[-1]], plain["lse"][:, :cu[-1]]), \
                f"{call.note} [{placement}]: differs from the run on plain allocations"
            arena.check()
            O, lse = got["O"].cpu(), got["lse"].cpu()
            kv.assert_close(O[owned], lse[:, owned], refO[owned], refL[:, owned], f"{call.note} [{placement}]")
            assert bool((O[~owned].view(torch.int32) == -1).all()) and bool((lse[:, ~owned].view(torch.int32) == -1).all()), \
                f"{call.note} [{placement}]: a row that no sequence owns was written"
