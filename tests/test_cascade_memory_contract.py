"""GPU: the memory rules of tests/test_memory_contract.py on the two shared-prefix decode entry points (flash_attention_cascade_decode,
flash_attention_cascade_decode_paged): every tensor of the call carved out of one guarded arena of 0xFF bytes (tests/arena.py), at both
placements -- `aligned`, everything at 0 mod 512, and `offset`, tensors at 16 mod 256 and the side inputs at 4 mod 16, ``sharedLen``,
``sinks`` and ``sharedTable`` among them -- with the workspace entering as NaNs at exactly the stated size,
flash_attention_decode_workspace_size at the plan's num_splits.  The result must be the run on plain allocations bit for bit, the arena
untouched outside O, the LSE and the workspace, and the result is also held to the float64 reference (cascade_check.py;
kv_cache_check.assert_close, unchanged).  The calls go through the C ABI; the placements and the arena are memory_contract.py's."""
import ctypes
import math

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import cascade_check as cc  # noqa: E402
import kv_cache_check as kv  # noqa: E402
import memory_contract as mc  # noqa: E402
import sink_check as sc  # noqa: E402
from memory_contract import CODE, bf, f32, i32, spec  # noqa: E402

pytestmark = pytest.mark.gpu
B, H, HKV, SQ = 5, 8, 2, 3
LENS = [129, 256, 3, 4, 1]


def cascade_call(caches, Q, ls, lens, causal, ns, odt, sinks):
    """the tensors of one cascade call and the C entry point on them; sharedLen, kvLens, the tables, the descales and sinks are side
    inputs.  The plan is asserted: forced counts are taken, and the workspace is the decode function's at their sum"""
    d, page = caches.d, caches.page
    plan = fa.cascade_plan(B, H, HKV, SQ, cc.LS_CAP, cc.LU_CAP, d, CODE[odt], ns)
    assert ns == (0, 0) or (plan["shared"]["num_splits"], plan["unique"]["num_splits"]) == ns
    view = (lambda t: t.view(kv.F8)) if caches.fp8 else (lambda t: t)
    if page:
        data = dict(K=view(caches.pool(caches.sK, caches.uK)), V=view(caches.pool(caches.sV, caches.uV)), st=caches.shared_table,
                    table=caches.block_table)
    else:
        data = dict(Ks=view(caches.sK), Vs=view(caches.sV), K=view(caches.uK), V=view(caches.uV))
    data.update(Q=Q, sl=torch.tensor([ls], dtype=i32), lens=torch.tensor(lens, dtype=i32), sinks=sinks)
    if caches.fp8:
        data.update(kd=caches.kd, vd=caches.vd)
    side = ("sl", "lens", "sinks", "st", "table", "kd", "vd")
    specs = {n: spec(t.shape, t.dtype, side=n in side) for n, t in data.items()}
    specs.update(O=spec(Q.shape, odt, True), lse=spec((B, H, SQ), f32, True))
    name = fa._CASCADE_SYMBOLS[bool(page)]

    def go(v):
        p = lambda n: v[n].data_ptr() if n in v else None
        caches_ = ("K", "V") if page else ("Ks", "Vs", "K", "V")
        keep = [fa.FaStrides(*(v[n].stride()[:3] if v[n].dim() == 4 else (0,) + tuple(v[n].stride()[:2]))) for n in ("Q", *caches_, "O")]
        geometry = (v["K"].shape[0], page, caches.shared_table.numel(), caches.block_table.shape[1], caches.block_table.shape[1]) if page \
            else (cc.LS_CAP, cc.LU_CAP)
        rc = getattr(fa.lib(), name)(p("Q"), *(p(n) for n in caches_), p("O"), p("lse"), p("sl"), p("lens"),
                                     *((p("st"), p("table")) if page else ()), p("kd"), p("vd"), p("sinks"), p("ws"), B, H, HKV, SQ, *geometry,
                                     d, 1.0 / math.sqrt(d), causal, fa.FA_DTYPE_BF16, CODE[data["K"].dtype], CODE[odt],
                                     plan["shared"]["num_splits"], plan["unique"]["num_splits"], *[ctypes.byref(s) for s in keep], mc.stream())
        assert rc == 0, (name, fa.error_string(rc))

    return mc.Call(specs, data, go, ["O", "lse"], fa.decode_workspace_size(B, H, SQ, d, plan["num_splits"]),
                   f"{name} d {d} ls {ls} causal {causal} splits {ns} O {odt}")


@pytest.mark.parametrize("page,fp8", [(0, False), (16, False), (128, False), (0, True), (16, True), (128, True)])
@pytest.mark.parametrize("d", [64, 128])
def test_cascade_calls(d, page, fp8):
    if fp8 and kv.F8 is None:
        pytest.skip("this torch has no float8_e4m3fn")
    caches = cc.Caches(B, HKV, d, page, fp8, seed=1700 + d + page + 7 * fp8)
    Q = mc.randn((B, H, SQ, d), 1701 + d)
    sinks = sc.sinks_for(H)
    for ls, causal, ns, odt in ((129, True, (1, 2), f32), (384, False, (3, 5), bf), (1, True, (0, 0), f32)):
        refO, refL = caches.reference(Q, ls, LENS, causal, sinks=sinks)
        call = cascade_call(caches, Q, ls, LENS, causal, ns, odt, sinks)
        assert call.ws_bytes > 0
        _, plain = mc.run(call, None)
        for placement in mc.PLACEMENTS:
            arena, got = mc.run(call, placement)
            if placement == "offset":
                for n in ("sl", "sinks") + (("st",) if page else ()):
                    assert got[n].data_ptr() % 16 == 4, n
            assert got["ws"].numel() == call.ws_bytes
            for n in call.outs:
                assert mc.same(got[n], plain[n]), f"{call.note} [{placement}]: {n} differs from the run on plain allocations"
            arena.check()
            if odt == f32:      # (a BF16 O is the F32 one rounded once: tests/test_cascade.py; here it is held to the plain run's bits)
                kv.assert_close(got["O"], got["lse"], refO, refL, f"{call.note} [{placement}]")
            else:
                assert (kv.lse_ratio(got["lse"].cpu(), refL) <= 1).all(), f"{call.note} [{placement}]"
