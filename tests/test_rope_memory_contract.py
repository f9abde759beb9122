"""GPU tests of what the four flash_attention_rope_append* calls read and write, in the guarded arena of tests/test_memory_contract.py
(tests/arena.py, tests/memory_contract.py): every call once on plain torch allocations and then with all its tensors carved out of one
arena of 0xFF bytes -- everything at 0 mod 512, then the tensors (the cos / sin table among them: the kernel loads it 16 bytes at a
time) at 16 mod 256 and kv_lens, cu_seqlens_q, the block table and the descales at 4 mod 16.  Qout enters as NaNs, the caches as the
cache's own bytes.  The results must equal the plain run's bit for bit and tests/rope_check.py's, the arena must be untouched outside
Qout and the caches, and the inputs unchanged."""
import ctypes

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import arena as ar  # noqa: E402
import memory_contract as mc  # noqa: E402
import rope_call  # noqa: E402
import rope_check as rc  # noqa: E402
from kv_cache_check import cu_of  # noqa: E402

pytestmark = pytest.mark.gpu
bf, f32, i32, i16, u8 = torch.bfloat16, torch.float32, torch.int32, torch.int16, torch.uint8
ROWS, LENS = 5, [5, 129, 300, 3]                 # the first rows of a cache, rows across a tile and page seam, more rows than keys
RAGGED_ROWS, RAGGED_LENS, UNOWNED = [5, 0, 130, 17], [129, -5, 300, 1], 23      # an idle slot; 17 rows on 1 key; tokens nobody owns


def rope_call_of(cache, Q, Knew, Vnew, table, lens, il, cu=None):
    """the call as a memory_contract.Call: the cache's K and V writable, Qout an output of its own"""
    ragged = cu is not None
    rows = Q.shape[0] if ragged else Q.shape[2]
    specs = dict(cache.specs(writable=True), Q=mc.spec(Q.shape, bf), Knew=mc.spec(Knew.shape, bf), Vnew=mc.spec(Vnew.shape, bf),
                 Qout=mc.spec(Q.shape, bf, writable=True), cs=mc.spec(table.shape, f32), lens=mc.spec((cache.B,), i32, side=True))
    data = dict(cache.data(), Q=Q, Knew=Knew, Vnew=Vnew, cs=table, lens=torch.tensor(lens, dtype=i32))
    if ragged:
        specs["cu"], data["cu"] = mc.spec((cache.B + 1,), i32, side=True), torch.tensor(cu, dtype=i32)
    name = rope_call.ROPE[bool(cache.page), ragged]

    def go(v):
        keep = [rope_call.strides3(v[n], ragged) for n in ("Q", "Knew", "Vnew", "Qout")]
        sQ, sKn, sVn, sQo = (ctypes.byref(s) for s in keep)
        values = dict(cache.values(v), Q=v["Q"].data_ptr(), Kn=v["Knew"].data_ptr(), Vn=v["Vnew"].data_ptr(), Qo=v["Qout"].data_ptr(),
                      cs=v["cs"].data_ptr(), H=Q.shape[1], Sq=rows, rot=table.shape[1], maxpos=table.shape[0], il=int(il),
                      dtype=fa.FA_DTYPE_BF16, sQ=sQ, sKn=sKn, sVn=sVn, sQo=sQo, stream=mc.stream())
        rc_ = mc.c_call(name, values)
        assert rc_ == 0, (name, fa.error_string(rc_))

    return mc.Call(specs, data, go, ["Qout", "K", "V"], 0, f"{name} d {cache.d} rows {rows} interleaved {il}")


def ints(t):
    return t.view(u8) if t.dtype == mc.F8 else t.view(i16)


@pytest.mark.parametrize("page,fp8", [(None, False), (None, True), (16, False), (128, True)])
@pytest.mark.parametrize("ragged", [False, True])
def test_rope_append(ragged, page, fp8):
    d, B, il = (128 if fp8 else 64), 4, bool(page)
    H = mc.HKV * mc.G
    cache = mc.Cache(B, d, page, fp8, seed=900 + d + (page or 0))
    table = fa.rope_table(mc.CAPACITY, d // 2)
    bt = cache.table[:, :mc.CAPACITY // page] if page else None
    if ragged:
        cu, lens = cu_of(RAGGED_ROWS), RAGGED_LENS
        T = cu[-1] + UNOWNED
        Q, Knew, Vnew = mc.randn((T, H, d), 901), mc.randn((T, mc.HKV, d), 902), mc.randn((T, mc.HKV, d), 903)
        nan = torch.full((T, H, d), -1, dtype=i16).view(bf)                 # what the arena's Qout holds before: 0xFF bytes
        want = rc.rope_append_varlen(Q, Knew, Vnew, nan, ints(cache.K), ints(cache.V), table, cu, lens, il, cache.kd, cache.vd, bt)
    else:
        cu, lens = None, LENS
        Q, Knew, Vnew = mc.randn((B, H, ROWS, d), 904), mc.randn((B, mc.HKV, ROWS, d), 905), mc.randn((B, mc.HKV, ROWS, d), 906)
        want = rc.rope_append(Q, Knew, Vnew, ints(cache.K), ints(cache.V), table, lens, il, cache.kd, cache.vd, bt)[:3]
    assert not torch.equal(want[1], ints(cache.K)), "the append changes the cache"
    call = rope_call_of(cache, Q, Knew, Vnew, table, lens, il, cu)
    owned = slice(0, cu[-1]) if ragged else slice(None)
    _, plain = mc.run(call, None)
    for placement in mc.PLACEMENTS:
        arena, got = mc.run(call, placement)
        what = f"{call.note} [{placement}]"
        assert mc.same(got["Qout"][owned], plain["Qout"][owned]) and mc.same(got["K"], plain["K"]) and mc.same(got["V"], plain["V"]), \
            f"{what}: differs from the run on plain allocations"
        arena.check()                                                       # nothing outside Qout and the caches; the inputs as loaded
        for n, w in zip(("Qout", "K", "V"), want):
            rc.assert_same(f"{what}: {n}", ints(got[n]), w)                 # (ragged: the tokens nobody owns still hold 0xFF bytes)
    if ragged:
        assert not ar.bits(plain["Qout"][cu[-1]:]).any()                    # ... and zeros on the plain allocations
