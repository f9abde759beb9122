"""GPU: the memory rules of tests/test_memory_contract.py on the two tree-masked verification entry points (flash_attention_tree,
flash_attention_tree_paged): every tensor of the call carved out of one guarded arena of 0xFF bytes (tests/arena.py), at both
placements -- `aligned`, everything at 0 mod 512, and `offset`, tensors at 16 mod 256, the side inputs at 4 mod 16 and the mask words at
8 mod 16, the least the library accepts for them -- with the workspace entering as NaNs at exactly its stated size.  The result must be
the run on plain allocations bit for bit, the arena untouched outside O, the LSE and the workspace, and the result is also held to the
float64 reference of tree_check.py (kv_cache_check.assert_close, unchanged).  One split and three; a decode row count and a
chunked-prefill one.  The cache, the specs and the arena are memory_contract.py's, imported."""
import math

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import arena as ar  # noqa: E402
import kv_cache_check as kv  # noqa: E402
import memory_contract as mc  # noqa: E402
import sink_check as sc  # noqa: E402
import tree_check as tc  # noqa: E402
from abi_decl import c_call  # noqa: E402
from memory_contract import CODE, DEV, bf, f32, i32  # noqa: E402

pytestmark = pytest.mark.gpu
LENS = [129, 300]
H = mc.HKV * mc.G
MASK = (8, 16)                              # the residue of the mask words under the `offset` placement
assert (mc.HKV, mc.CAPACITY, len(LENS)) == (tc.HKV, tc.CAP, tc.B)


def tree_call(cache, Q, lens, ns, W, sinks, words):
    """memory_contract.split_kv_call's tensors plus ``sinks`` and the mask words as side inputs, through flash_attention_tree*"""
    d, B, rows = cache.d, cache.B, Q.shape[2]
    plan = fa.tree_plan(B, H, mc.HKV, rows, mc.CAPACITY, d, CODE[f32], ns, window=W)
    assert plan["num_splits"] == ns and (plan["combine_grid"] > 0) == (ns > 1), plan
    specs = dict(cache.specs(), Q=mc.spec(Q.shape, bf), O=mc.spec(Q.shape, f32, True), lse=mc.spec((B, H, rows), f32, True),
                 lens=mc.spec((B,), i32, side=True), sinks=mc.spec((H,), f32, side=True), tree=mc.spec((B, rows), torch.int64, side=True))
    data = dict(cache.data(), Q=Q, lens=torch.tensor(lens, dtype=i32), sinks=sinks, tree=tc.words_tensor(words))
    name = "flash_attention_tree" + ("_paged" if cache.page else "")

    def go(v):
        _, (sQ, sO) = mc.strides(v["Q"], v["O"])
        rc = c_call(name, dict(cache.values(v), Q=v["Q"].data_ptr(), O=v["O"].data_ptr(), LSE=v["lse"].data_ptr(), ws=mc.ptr(v, "ws"), H=H,
                               Sq=rows, scale=1.0 / math.sqrt(d), dtype=fa.FA_DTYPE_BF16, o=CODE[f32], ns=ns, W=W, sQ=sQ, sO=sO,
                               stream=mc.stream(), sinks=v["sinks"].data_ptr(), tree=v["tree"].data_ptr()))
        assert rc == 0, (name, fa.error_string(rc))

    return mc.Call(specs, data, go, ["O", "lse"], fa.decode_workspace_size(B, H, rows, d, ns), f"{name} d {d} rows {rows} splits {ns} window {W}")


def run(call, placement):
    """memory_contract.run with the mask words at MASK under `offset` (memory_contract.place knows two residues, 16 mod 256 and 4 mod 16)"""
    if placement != "offset":
        return mc.run(call, placement)
    specs = dict(call.specs, ws=mc.spec((call.ws_bytes,), torch.uint8, writable=True)) if call.ws_bytes else dict(call.specs)
    residue = lambda n, s: MASK if n == "tree" else ar.SIDE if s["side"] else ar.OFFSET
    arena, v = ar.Arena.of(DEV, {n: dict(shape=s["shape"], dtype=s["dtype"], strides=s["strides"], writable=s["writable"],
                                         residue=residue(n, s)) for n, s in specs.items()})
    for n, t in call.data.items():
        arena.load(v[n], t)
    call.run(v)
    torch.cuda.synchronize()
    return arena, v


@pytest.mark.parametrize("page,fp8", [(None, False), (16, False), (None, True), (128, True)])
@pytest.mark.parametrize("d,rows", [(64, 5), (128, 16), (64, 40), (128, 17), (128, 64)])
def test_tree_calls(d, rows, page, fp8):
    cache = mc.Cache(len(LENS), d, page, fp8, seed=2100 + d + (page or 0) + 7 * fp8)
    Q = mc.randn((len(LENS), H, rows, d), 2101 + rows)
    sinks = sc.sinks_for(H)
    words = [tc.words_of("binary", rows), tc.words_of("random", rows, 3)]
    for W, ns in ((w, n) for w in (0, 130) for n in (1, 3)):
        refO, refL = kv.reference(Q, cache.refK, cache.refV, LENS, True, W, words=words, sinks=sinks)
        call = tree_call(cache, Q, LENS, ns, W, sinks, words)
        assert call.ws_bytes == fa.decode_workspace_size(len(LENS), H, rows, d, ns) and (call.ws_bytes > 0) == (ns > 1)
        _, plain = run(call, None)
        for placement in mc.PLACEMENTS:
            arena, got = run(call, placement)
            if placement == "offset":
                assert got["tree"].data_ptr() % 16 == 8 and got["sinks"].data_ptr() % 16 == 4
            for n in call.outs:
                assert mc.same(got[n], plain[n]), f"{call.note} [{placement}]: {n} differs from the run on plain allocations"
            arena.check()
            kv.assert_close(got["O"], got["lse"], refO, refL, f"{call.note} [{placement}]")
