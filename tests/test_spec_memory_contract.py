"""GPU: the memory rules of tests/test_memory_contract.py on the four entry points of the speculative step's write side
(flash_attention_rope_append_pos, _paged_pos, flash_attention_kv_accept, _paged): every tensor of the call carved out of one guarded
arena of 0xFF bytes (tests/arena.py, tests/memory_contract.py), at both placements -- `aligned`, everything at 0 mod 512, and `offset`,
the tensors at 16 mod 256 and kv_lens, the block table, the descales, posOffsets, acceptIdx and acceptLens at 4 mod 16, the least the
library accepts for them.  The results must equal the run on plain allocations bit for bit and tests/spec_step_check.py's, and the
arena must be untouched outside Qout and the caches, the inputs unchanged."""
import ctypes

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import memory_contract as mc  # noqa: E402
import rope_call  # noqa: E402
import rope_check as rc  # noqa: E402
import spec_step_call as call_  # noqa: E402
import spec_step_check as sp  # noqa: E402

pytestmark = pytest.mark.gpu
bf, f32, i32, i16, u8 = torch.bfloat16, torch.float32, torch.int32, torch.int16, torch.uint8
B, ROWS, LENS = 4, 21, [21, 140, 300, 3]         # no prefix; across a tile and page seam; deep in the cache; more nodes than keys
FORMS = [(None, False), (None, True), (16, False), (128, True)]


def ints(t):
    return t.view(u8) if t.dtype == mc.F8 else t.view(i16)


def trees():
    return [sp.binary(ROWS), sp.star(ROWS), sp.random_tree(ROWS, 3000), sp.chain(ROWS)]


def rope_pos_call(cache, Q, Knew, Vnew, table, lens, offs, il):
    specs = dict(cache.specs(writable=True), Q=mc.spec(Q.shape, bf), Knew=mc.spec(Knew.shape, bf), Vnew=mc.spec(Vnew.shape, bf),
                 Qout=mc.spec(Q.shape, bf, writable=True), cs=mc.spec(table.shape, f32), lens=mc.spec((cache.B,), i32, side=True),
                 pos=mc.spec((cache.B, ROWS), i32, side=True))
    data = dict(cache.data(), Q=Q, Knew=Knew, Vnew=Vnew, cs=table, lens=torch.tensor(lens, dtype=i32), pos=torch.tensor(offs, dtype=i32))
    name = call_.ROPE_POS[bool(cache.page)]

    def go(v):
        keep = [rope_call.strides3(v[n]) for n in ("Q", "Knew", "Vnew", "Qout")]
        sQ, sKn, sVn, sQo = (ctypes.byref(s) for s in keep)
        values = dict(cache.values(v), Q=v["Q"].data_ptr(), Kn=v["Knew"].data_ptr(), Vn=v["Vnew"].data_ptr(), Qo=v["Qout"].data_ptr(),
                      cs=v["cs"].data_ptr(), pos=v["pos"].data_ptr(), H=Q.shape[1], Sq=ROWS, rot=table.shape[1], maxpos=table.shape[0],
                      il=int(il), dtype=fa.FA_DTYPE_BF16, sQ=sQ, sKn=sKn, sVn=sVn, sQo=sQo, stream=mc.stream())
        code = mc.c_call(name, values)
        assert code == 0, (name, fa.error_string(code))

    return mc.Call(specs, data, go, ["Qout", "K", "V"], 0, f"{name} d {cache.d} interleaved {il}")


def accept_call(cache, lens, idx, nacc):
    specs = dict(cache.specs(writable=True), lens=mc.spec((cache.B,), i32, side=True), idx=mc.spec((cache.B, ROWS), i32, side=True),
                 nacc=mc.spec((cache.B,), i32, side=True))
    data = dict(cache.data(), lens=torch.tensor(lens, dtype=i32), idx=torch.tensor(idx, dtype=i32), nacc=torch.tensor(nacc, dtype=i32))
    name = call_.ACCEPT[bool(cache.page)]

    def go(v):
        values = {k: x for k, x in cache.values(v).items() if k not in ("kd", "vd", "cu")}
        code = mc.c_call(name, dict(values, idx=v["idx"].data_ptr(), nacc=v["nacc"].data_ptr(), draft=ROWS, stream=mc.stream()))
        assert code == 0, (name, fa.error_string(code))

    return mc.Call(specs, data, go, ["K", "V"], 0, f"{name} d {cache.d}")


def in_the_arena(call, want, side):
    _, plain = mc.run(call, None)
    for placement in mc.PLACEMENTS:
        arena, got = mc.run(call, placement)
        what = f"{call.note} [{placement}]"
        if placement == "offset":
            assert all(got[n].data_ptr() % 16 == 4 for n in side), what
        assert all(mc.same(got[n], plain[n]) for n in call.outs), f"{what}: differs from the run on plain allocations"
        arena.check()                                           # nothing outside Qout and the caches; the inputs as loaded
        for n, w in zip(call.outs, want):
            rc.assert_same(f"{what}: {n}", got[n], w)


@pytest.mark.parametrize("page,fp8", FORMS)
def test_rope_append_pos(page, fp8):
    d, il = (128 if fp8 else 64), bool(page)
    H = mc.HKV * mc.G
    cache = mc.Cache(B, d, page, fp8, seed=3100 + d + (page or 0))
    table = fa.rope_table(mc.CAPACITY, d // 2)
    bt = cache.table[:, :mc.CAPACITY // page] if page else None
    Q, Knew, Vnew = mc.randn((B, H, ROWS, d), 3101), mc.randn((B, mc.HKV, ROWS, d), 3102), mc.randn((B, mc.HKV, ROWS, d), 3103)
    offs = [sp.depths(t) for t in trees()]
    want = sp.rope_append_pos(Q, Knew, Vnew, ints(cache.K), ints(cache.V), table, LENS, offs, il, cache.kd, cache.vd, bt)
    assert not torch.equal(want[1], ints(cache.K)), "the append changes the cache"
    in_the_arena(rope_pos_call(cache, Q, Knew, Vnew, table, LENS, offs, il), want, ("lens", "pos"))


@pytest.mark.parametrize("page,fp8", FORMS)
def test_kv_accept(page, fp8):
    d = 128 if fp8 else 64
    cache = mc.Cache(B, d, page, fp8, seed=3200 + d + (page or 0))
    bt = cache.table[:, :mc.CAPACITY // page] if page else None
    paths = [sp.tree_path(t, leaf) for t, leaf in zip(trees(), (ROWS - 1, 7, ROWS // 2, ROWS - 1))]
    paths[3] = (list(range(1, ROWS)) + [ROWS - 1], ROWS - 1)                   # the chain 1, 2, 3, ...
    idx, nacc = [p[0] for p in paths], [p[1] for p in paths]
    want = sp.accept(ints(cache.K), ints(cache.V), LENS, idx, nacc, ROWS, bt)
    assert not torch.equal(want[0], ints(cache.K)), "the acceptance changes the cache"
    in_the_arena(accept_call(cache, LENS, idx, nacc), want, ("lens", "idx", "nacc"))
