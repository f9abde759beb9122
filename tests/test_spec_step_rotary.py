"""GPU test of ONE SPECULATIVE STEP of a rotary model, end to end and without a host synchronisation inside it:

    lens += Sq;  Qr = rope_cache_append(..., pos_offsets=tree_depths(parents));  O = flash_attention_tree(Qr, ...);
    leaf chosen on the device;  accept_idx, accept_lens = tree_path(parents, leaf);  kv_cache_accept(...);  lens -= Sq - accept_lens

for d = 64 / 128, a bf16 contiguous cache and an fp8 paged one.  Afterwards the caches below the new length equal, byte for byte, a
cache filled by the fused rotary append of the accepted tokens one linear step at a time (tests/rope_check.py); every accepted node's
row of the tree call, and a further token through rope_cache_append + flash_attention_decode, meet kv_cache_check.assert_close
(unchanged: 1e-3 + 1e-3 |ref| on O, 2e-4 + 2e-6 |ref| on the LSE) against float64 attention on that linear rotated sequence; and the
same step captured once as a graph and replayed with other leaves and lengths gives the bits of the eager run."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_cache_check as kv  # noqa: E402
import rope_check as rc  # noqa: E402
import spec_step_check as sp  # noqa: E402
from kv_append_check import as_cache, sentinel  # noqa: E402
from kv_cache_check import DEV, assert_close, dequantise, gather, reference  # noqa: E402
from rope_check import table_of  # noqa: E402

pytestmark = pytest.mark.gpu
bf, f32, i16, i32 = torch.bfloat16, torch.float32, torch.int16, torch.int32
B, HKV, G, CAP, PAGE = 2, 2, 2, 384, 16
H = HKV * G


def dev(t):
    return None if t is None else t.to(DEV)


def mk(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(bf)


class Scene:
    """the caches with a rotated history up to `start`, on the CPU (the reference's integers) and on the device"""

    def __init__(self, d, paged, fp8, il, start):
        self.d, self.fp8, self.il, self.start = d, fp8, il, list(start)
        self.table = fa.rope_table(CAP, d // 2)
        self.kd, self.vd = (torch.tensor([0.02, 0.031]), torch.tensor([0.017, 0.025])) if fp8 else (None, None)
        if paged:
            P, self.bt = table_of(B, CAP // PAGE, 3, 1100 + d)
            K, V = sentinel((P, HKV, PAGE, d), fp8), sentinel((P, HKV, PAGE, d), fp8)
        else:
            self.bt, K, V = None, sentinel((B, HKV, CAP, d), fp8), sentinel((B, HKV, CAP, d), fp8)
        for b, L in enumerate(start):
            one = [L if x == b else 0 for x in range(B)]
            _, K, V, _ = rc.rope_append(mk((B, H, L, d), 1101), mk((B, HKV, L, d), 1102 + b), mk((B, HKV, L, d), 1104 + b), K, V, self.table, one, il,
                                        self.kd, self.vd, self.bt)
        self.K0, self.V0 = K, V
        self.ds = dict(k_descale=dev(self.kd), v_descale=dev(self.vd)) if fp8 else {}

    def linear(self, K, V, b, L, q, k, v):
        """one linear step of sequence b on the reference's caches: its row q / k / v ([1, heads, 1, d] of sequence b) appended as
        the L-th token -> (the rotated q, K, V)"""
        one = [L if x == b else 0 for x in range(B)]
        wide = lambda x: torch.cat([x if y == b else torch.zeros_like(x) for y in range(B)])
        qo, K, V, _ = rc.rope_append(wide(q), wide(k), wide(v), K, V, self.table, one, self.il, self.kd, self.vd, self.bt)
        return qo[b:b + 1], K, V

    def floats(self, K, V):
        """the reference's caches as the values attention reads: [B, Hkv, CAP, d]"""
        K, V = (K, V) if self.bt is None else (gather(K, self.bt), gather(V, self.bt))
        return (dequantise(K, self.kd), dequantise(V, self.vd)) if self.fp8 else (K.view(bf), V.view(bf))


@pytest.mark.parametrize("paged,fp8", [(False, False), (True, True)])
@pytest.mark.parametrize("d,Sq", [(64, 15), (128, 31)])
def test_one_rotary_speculative_step_end_to_end(d, Sq, paged, fp8):
    il = d == 128
    s = Scene(d, paged, fp8, il, (100, 250))
    parents = [sp.binary(Sq), sp.random_tree(Sq, 1110 + d)]
    pd = torch.tensor(parents, device=DEV)
    mask, depths = fa.tree_mask_from_parents(pd), fa.tree_depths(pd)            # (checked on the host: outside the step)
    Kd, Vd, btd, csd = dev(s.K0), dev(s.V0), dev(s.bt), dev(s.table)
    Kc, Vc = as_cache(Kd), as_cache(Vd)
    lens = torch.zeros(B, dtype=i32, device=DEV)
    Q_s, Kn_s, Vn_s = (torch.zeros(shape, dtype=bf, device=DEV) for shape in ((B, H, Sq, d), (B, HKV, Sq, d), (B, HKV, Sq, d)))
    shift = torch.zeros(B, dtype=torch.int64, device=DEV)
    tables = (btd,) if paged else ()
    append, tree, accept = ((fa.rope_cache_append_paged, fa.flash_attention_tree_paged, fa.kv_cache_accept_paged) if paged else
                            (fa.rope_cache_append, fa.flash_attention_tree, fa.kv_cache_accept))

    def step():
        lens.add_(Sq)
        Qr = append(Q_s, Kn_s, Vn_s, Kc, Vc, *tables, csd, lens, interleaved=il, pos_offsets=depths, **s.ds)
        O, lse = tree(Qr, Kc, Vc, *tables, mask, lens, return_lse=True, out_dtype=f32, num_splits=2, **s.ds)
        leaf = (lse[:, 0, :].argmax(dim=-1) + shift) % Sq                       # the "sampling": a node chosen on the device
        idx, n = fa.tree_path(pd, leaf)
        accept(Kc, Vc, *tables, idx, n, lens)
        lens.sub_(Sq - n)
        return Qr, O, lse, leaf, idx, n

    def load(state):
        start, sh, seed = state
        Q, Kn, Vn = mk(Q_s.shape, seed), mk(Kn_s.shape, seed + 1), mk(Vn_s.shape, seed + 2)
        for t, x in ((Q_s, Q), (Kn_s, Kn), (Vn_s, Vn), (Kd, s.K0), (Vd, s.V0)):
            t.copy_(x)
        lens.copy_(torch.tensor(start, dtype=i32))
        shift.copy_(torch.tensor(sh))
        return Q, Kn, Vn

    snap = lambda out: [x.clone() for x in out] + [Kd.clone(), Vd.clone(), lens.clone()]
    states = [((100, 250), (0, 0), 1120), ((97, 250), (3, Sq - 1), 1130), ((100, 200), (Sq // 2, 1), 1140)]
    load(states[0])
    step()                                                                      # every kernel of the step has run once before the capture
    torch.cuda.synchronize()
    load(states[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # ONE stream, no host read-back inside
        held = step()
    leaves = []
    for state in states:
        Q, Kn, Vn = load(state)
        eager = snap(step())
        load(state)
        graph.replay()
        torch.cuda.synchronize()
        replay = snap(held)
        assert all(kv.same_bits(a, b) for a, b in zip(eager, replay)), state      # Qr, O, LSE, the leaf, the path, the caches, the lengths
        Qr, O, lse, leaf, idx, n, K1, V1, L1 = (x.cpu() for x in replay)
        start = state[0]
        leaves.append(leaf.tolist())
        refK, refV = s.K0, s.V0
        for b in range(B):
            path, count = sp.tree_path(parents[b], int(leaf[b]))
            assert idx[b].tolist() == path and int(n[b]) == count and int(L1[b]) == start[b] + count
            for t, node in enumerate(path[:count]):
                one = lambda x: x[b:b + 1, :, node:node + 1]
                # the linear sequence: the accepted tokens one step at a time through the reference of the fused append
                qo, refK, refV = s.linear(refK, refV, b, start[b] + t + 1, one(Q), one(Kn), one(Vn))
                rc.assert_same(f"sequence {b} node {node}: the rotated query", one(Qr), qo)
                Kf, Vf = s.floats(refK, refV)
                wantO, wantL = reference(qo, Kf[b:b + 1], Vf[b:b + 1], [start[b] + t + 1], True)
                assert_close(one(O), lse[b:b + 1, :, node:node + 1], wantO, wantL, f"d {d} fp8 {fp8} sequence {b}: accepted node {node} (depth {t})")
        # the caches below the new lengths: byte for byte the linear sequence's
        got = (K1, V1) if s.bt is None else (gather(K1, s.bt), gather(V1, s.bt))
        want = (refK, refV) if s.bt is None else (gather(refK, s.bt), gather(refV, s.bt))
        for b in range(B):
            for name, g, w in zip("KV", got, want):
                assert torch.equal(g[b, :, :int(L1[b])], w[b, :, :int(L1[b])]), (name, b, state)
        # a further token: the plain fused append and decode on the accepted sequence
        q1, k1, v1 = mk((B, H, 1, d), state[2] + 5), mk((B, HKV, 1, d), state[2] + 6), mk((B, HKV, 1, d), state[2] + 7)
        lens.add_(1)
        Qn = append(dev(q1), dev(k1), dev(v1), Kc, Vc, *tables, csd, lens, interleaved=il, **s.ds)
        decode = fa.flash_attention_decode_paged if paged else fa.flash_attention_decode
        O1, lse1 = decode(Qn, Kc, Vc, *tables, lens, is_causal=True, return_lse=True, out_dtype=f32, **s.ds)
        torch.cuda.synchronize()
        now = [int(L) + 1 for L in L1]
        assert lens.tolist() == now
        qn = []
        for b in range(B):
            qo, refK, refV = s.linear(refK, refV, b, now[b], q1[b:b + 1], k1[b:b + 1], v1[b:b + 1])
            qn.append(qo)
        rc.assert_same("the next token's query", Qn, torch.cat(qn))
        assert_close(O1, lse1, *reference(torch.cat(qn), *s.floats(refK, refV), now, True), f"d {d} fp8 {fp8}: the next token")
    assert len({tuple(x) for x in leaves}) == len(states)                       # the replays took other leaves
