"""GPU tests of flash_attention_rope_append_pos and flash_attention_rope_append_paged_pos (rope_cache_append*(..., pos_offsets=)): the
fused rotary append with the table row of every new row taken from a per-row offset -- a draft tree's node rotated at base + its depth
while it is stored at slot base + its index.

Everything is a comparison of BITS with tests/spec_step_check.py (rope_check.rotate at the rule's positions, kv_append_check.append for
the slots; held against its twin and against four wrong kernels in tests/test_spec_step_abi.py): Qout, the K cache and the V cache as
integers, NaN codes by class, no tolerance.  Caches and Qout are pre-filled with a sentinel and compared WHOLE, so what must not be
written is checked with what must.  The calls go through the C ABI by name (tests/spec_step_call.py)."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_append_check as kc  # noqa: E402
import rope_check as rc  # noqa: E402
import spec_step_call as call  # noqa: E402
import spec_step_check as sp  # noqa: E402
from kv_append_check import SENT, descales, sentinel  # noqa: E402
from kv_cache_check import DEV, i32 as lens_tensor  # noqa: E402
from rope_check import check, qsent, rows, table_of  # noqa: E402

pytestmark = pytest.mark.gpu
bf, i16, u8, i32 = torch.bfloat16, torch.int16, torch.uint8, torch.int32
B, HKV, CAP = 2, 2, 384
SQS = (1, 7, 31, 64, 100)                         # across the 16-row wave and the 64-row block of the kernel


def dev(t):
    return None if t is None else t.to(DEV)


def offsets(family, Sq, seed=0):
    """the offsets of one sequence: the depths of a tree of Sq nodes, or a family of plain values"""
    if family == "binary":
        return sp.depths(sp.binary(Sq))
    if family == "star":
        return sp.depths(sp.star(Sq))
    if family == "random":
        return sp.depths(sp.random_tree(Sq, seed))
    if family == "identity":
        return list(range(Sq))
    if family == "zero":
        return [0] * Sq
    raise KeyError(family)


def run(Q, Kn, Vn, Kc, Vc, cs, offs, lens, il, kd, vd, table=None, Qo=None):
    """the call on copies of the CPU tensors -> (Qout, K cache, V cache) on the device; offs None: the twin without offsets"""
    Qo = dev(qsent(Q.shape) if Qo is None else Qo)
    Kd, Vd = dev(Kc), dev(Vc)
    pos = None if offs is None else torch.tensor(offs, dtype=i32).to(DEV)
    call.rope_pos(dev(Q), dev(Kn), dev(Vn), Qo, Kd, Vd, dev(cs), pos, lens_tensor(lens), il, dev(kd), dev(vd), dev(table))
    torch.cuda.synchronize()
    return Qo, Kd, Vd


def caches(page, d, fp8, seed):
    if page:
        P, bt = table_of(B, CAP // page, 3, seed)
        return bt, sentinel((P, HKV, page, d), fp8), sentinel((P, HKV, page, d), fp8)
    return None, sentinel((B, HKV, CAP, d), fp8), sentinel((B, HKV, CAP, d), fp8)


def lengths(Sq, page):
    """lengths that put first = L - Sq just below, on and above a page start and a 64-position block start; fewer keys than rows; an
    inactive slot; the capacity and beyond"""
    out = {-3, 0, Sq - 1, Sq, CAP, CAP + 7}
    for edge in {page, 64, 128}:
        out |= {Sq + edge - 1, Sq + edge, Sq + edge + 1}
    out = sorted(L for L in out if L <= CAP + 7)
    return out + out[:len(out) % 2]               # (pairs: B = 2)


# ---- 1. bit for bit against the reference ----
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [None, 16, 128])
def test_bit_for_bit(page, d, fp8):
    families = ("binary", "star", "random", "zero", "identity")
    salt = (0 if page is None else page // 16) + d // 64 + int(fp8)
    for si, Sq in enumerate(SQS):
        il, rot = bool((si + salt) % 2), (16, 32, d)[(si + salt) % 3]     # over the twelve cases: both pair styles with every rotDim
        G = (1, 4, 2)[si % 3]
        table = fa.rope_table(CAP, rot)
        bt, Kc, Vc = caches(page, d, fp8, 5 + Sq)
        Q, Kn, Vn = rows((B, HKV * G, Sq, d), 1 + Sq), rows((B, HKV, Sq, d), 2 + Sq, special=True), rows((B, HKV, Sq, d), 3 + Sq, special=True)
        kd, vd = descales(4 + Sq, fp8, HKV)
        every = lengths(Sq, page or 32)
        for at in range(0, len(every), 2):
            lens = every[at:at + 2]
            offs = [offsets(families[(at // 2 + b) % 5], Sq, 11 * at + b) for b in range(B)]
            for L in ((lens, None) if at == 0 else (lens,)):
                got = run(Q, Kn, Vn, Kc, Vc, table, offs, L, il, kd, vd, bt)
                want = sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, L, offs, il, kd, vd, bt)
                check(got, want, f"page {page} d {d} fp8 {fp8} il {il} rot {rot} Sq {Sq} lens {L}")


# ---- 2. the twin, the clamp ----
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16])
def test_identity_offsets_are_the_twin_and_offsets_are_clamped(page, fp8):
    d, rot, G = 128, 64, 2
    table = fa.rope_table(CAP, rot)
    for Sq, lens in ((1, [200, 0]), (31, [77, 20]), (100, [384, 165])):
        bt, Kc, Vc = caches(page, d, fp8, 20 + Sq)
        Q, Kn, Vn = rows((B, HKV * G, Sq, d), 21 + Sq), rows((B, HKV, Sq, d), 22 + Sq, special=True), rows((B, HKV, Sq, d), 23 + Sq, special=True)
        kd, vd = descales(24 + Sq, fp8, HKV)
        twin = run(Q, Kn, Vn, Kc, Vc, table, None, lens, True, kd, vd, bt)
        same = run(Q, Kn, Vn, Kc, Vc, table, [list(range(Sq))] * B, lens, True, kd, vd, bt)
        assert all(torch.equal(bits(g), bits(w)) for g, w in zip(same, twin)), Sq             # all three outputs, byte for byte
        assert not bool((twin[1].cpu() == SENT[Kc.dtype]).all())
        # offsets out of range equal the call on the clamped values
        wild = [[(-5, Sq + 9, 2 ** 31 - 1, -2 ** 31, i)[(i + b) % 5] for i in range(Sq)] for b in range(B)]
        tame = [[sp.clamp(o, 0, Sq - 1) for o in row] for row in wild]
        a, b_ = run(Q, Kn, Vn, Kc, Vc, table, wild, lens, True, kd, vd, bt), run(Q, Kn, Vn, Kc, Vc, table, tame, lens, True, kd, vd, bt)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b_)), Sq
        check(a, sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, wild, True, kd, vd, bt), f"wild offsets Sq {Sq}")


def bits(t):
    return t.view(i16) if t.dtype == bf else t


# ---- 3. exact probes: every output element is +- one named input element, by the row's position mod 4 ----
@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("d,rot", [(64, 64), (64, 16), (128, 32), (128, 128)])
@pytest.mark.parametrize("page", [None, 16])
def test_probes_read_back_every_rows_position(page, d, rot, il):
    Sq, G = 21, 2
    lens = [77, 12]
    table = rc.probe_table(CAP, rot)

    def coded(shape, base):      # index-coded: |value| = 1 .. 251 by the flat index, exact in bf16, never zero
        n = torch.arange(shape[0] * shape[1] * shape[2] * shape[3]).reshape(shape)
        return (((n * 7 + base) % 251 + 1) * torch.where(n % 3 == 0, -1, 1)).to(bf)

    Q, Kn, Vn = coded((B, HKV * G, Sq, d), 0), coded((B, HKV, Sq, d), 5), coded((B, HKV, Sq, d), 9)
    bt, Kc, Vc = caches(page, d, False, 31)
    offs = [offsets("random", Sq, 32), offsets("binary", Sq)]
    Qo, K, V = run(Q, Kn, Vn, Kc, Vc, table, offs, lens, il, None, None, bt)
    pos = torch.tensor([sp.pos_positions(L, Sq, CAP, o) for L, o in zip(lens, offs)])
    assert len({int(p) % 4 for p in pos.flatten()}) == 4 and pos.tolist() != [rc.q_positions(L, Sq, CAP) for L in lens]
    rc.assert_same("probe Qout", Qo, rc.probe_expect(Q, pos, rot, il))
    rc.assert_same("probe Kcache", K, kc.append(rc.probe_expect(Kn, pos, rot, il), Kc, lens, None, bt))
    rc.assert_same("probe Vcache", V, kc.append(Vn, Vc, lens, None, bt))


# ---- 4. in place, strided rows ----
@pytest.mark.parametrize("fp8", [False, True])
def test_in_place_and_a_fused_projection(fp8):
    d, Sq, G, rot = 64, 19, 2, 32
    H = HKV * G
    lens = [50, 96]
    kd, vd = descales(41, fp8, HKV)
    table = fa.rope_table(CAP, rot)
    offs = [offsets("binary", Sq), offsets("star", Sq)]
    pos = torch.tensor(offs, dtype=i32).to(DEV)
    # Q, K and V are slices of one fused [B, Sq, (H + 2 Hkv) d] projection; Qout goes IN PLACE into the projection
    fused = rows((B, Sq, (H + 2 * HKV) * d), 42)
    fd = dev(fused)
    heads = lambda t: t.view(B, Sq, H + 2 * HKV, d)
    part = lambda t: (heads(t)[:, :, :H].transpose(1, 2), heads(t)[:, :, H:H + HKV].transpose(1, 2), heads(t)[:, :, H + HKV:].transpose(1, 2))
    Q, Kn, Vn = part(fused)
    Qd, Knd, Vnd = part(fd)
    rawK, rawV = sentinel((B, HKV, CAP, d + 16), fp8), sentinel((B, HKV, CAP, d + 32), fp8)      # caches with row strides d + 16, d + 32
    Kd, Vd = dev(rawK), dev(rawV)
    call.rope_pos(Qd, Knd, Vnd, Qd, Kd[..., :d], Vd[..., :d], dev(table), pos, lens_tensor(lens), True, dev(kd), dev(vd))
    torch.cuda.synchronize()
    qo, k, v = sp.rope_append_pos(Q, Kn, Vn, rawK[..., :d].contiguous(), rawV[..., :d].contiguous(), table, lens, offs, True, kd, vd)
    want = fused.clone()
    heads(want)[:, :, :H] = qo.transpose(1, 2)
    rc.assert_same("the projection", fd, want)                   # the K and V slices as they were, Q rotated in place
    wantK, wantV = rawK.clone(), rawV.clone()
    wantK[..., :d], wantV[..., :d] = k, v
    rc.assert_same("K rows of d + 16", Kd, wantK)
    rc.assert_same("V rows of d + 32", Vd, wantV)


# ---- 5. a bad table entry: K / V skipped, Q written ----
@pytest.mark.parametrize("fp8", [False, True])
def test_bad_table_entries_skip_k_and_v_not_q(fp8):
    d, Sq, G, page, rot = 64, 40, 2, 16, 32
    n = CAP // page
    lens = [100, CAP]
    Q, Kn, Vn = rows((B, HKV * G, Sq, d), 51), rows((B, HKV, Sq, d), 52), rows((B, HKV, Sq, d), 53)
    kd, vd = descales(54, fp8, HKV)
    table = fa.rope_table(CAP, rot)
    P, bt = table_of(B, n, 3, 55)
    Kc, Vc = sentinel((P, HKV, page, d), fp8), sentinel((P, HKV, page, d), fp8)
    offs = [offsets("random", Sq, 56), offsets("binary", Sq)]
    base = run(Q, Kn, Vn, Kc, Vc, table, offs, lens, False, kd, vd, bt)
    receives = torch.zeros(B, n, dtype=torch.bool)
    for b, L in enumerate(lens):
        for _, p in kc.positions(L, Sq, CAP):
            receives[b, p // page] = True
    t3 = bt.clone()
    for k, (b, j) in enumerate(receives.nonzero()[::2].tolist()):
        t3[b, j] = (-1, P, 2 ** 31 - 1, -2 ** 31, P + 5)[k % 5]
    # ... and the entries of pages that receive no row are not read: any int32 there
    t3 = torch.where(receives, t3, torch.full_like(t3, 2 ** 31 - 1))
    got = run(Q, Kn, Vn, Kc, Vc, table, offs, lens, False, kd, vd, t3)
    check(got, sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, offs, False, kd, vd, t3), "entries out of range")
    assert torch.equal(got[0].view(i16), base[0].view(i16))      # every Q row as with the good table
    skipped = torch.zeros(P, dtype=torch.bool)
    skipped[bt[receives & (t3 != bt)].long()] = True
    assert int(skipped.sum()) > 2
    assert bool((got[1].cpu()[skipped] == SENT[Kc.dtype]).all()) and bool((got[2].cpu()[skipped] == SENT[Kc.dtype]).all())


# ---- 6. a captured graph sees the offsets and the lengths of the moment ----
@pytest.mark.parametrize("page,fp8", [(None, True), (128, False)])
def test_a_graph_replays_on_rewritten_offsets_and_lengths(page, fp8):
    d, Sq, G, rot = 128, 33, 2, 64
    table = fa.rope_table(CAP, rot)
    bt, Kc, Vc = caches(page, d, fp8, 61)
    kd, vd = descales(62, fp8, HKV)
    Q_s, Kn_s, Vn_s = (torch.zeros(s, dtype=bf, device=DEV) for s in ((B, HKV * G, Sq, d), (B, HKV, Sq, d), (B, HKV, Sq, d)))
    Qo_s, Kd, Vd = qsent(Q_s.shape, DEV), dev(Kc), dev(Vc)
    pos_s, lens_s = torch.zeros((B, Sq), dtype=i32, device=DEV), lens_tensor([Sq, Sq])
    csd, kdd, vdd, btd = dev(table), dev(kd), dev(vd), dev(bt)
    step = lambda: call.rope_pos(Q_s, Kn_s, Vn_s, Qo_s, Kd, Vd, csd, pos_s, lens_s, False, kdd, vdd, btd)
    step()                                                       # the kernel has run once before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for r, (fams, lens) in enumerate(((("binary", "star"), [100, 300]), (("random", "identity"), [Sq + 127, 40]), (("zero", "random"), [CAP, 20]))):
        Q, Kn, Vn = rows(Q_s.shape, 63 + r), rows(Kn_s.shape, 66 + r), rows(Vn_s.shape, 69 + r)
        offs = [offsets(f, Sq, 70 + r) for f in fams]
        for t, x in ((Q_s, Q), (Kn_s, Kn), (Vn_s, Vn), (Kd, Kc), (Vd, Vc), (Qo_s, qsent(Q.shape))):
            t.copy_(x)
        pos_s.copy_(torch.tensor(offs, dtype=i32))
        lens_s.copy_(torch.tensor(lens, dtype=i32))
        graph.replay()
        torch.cuda.synchronize()
        check((Qo_s, Kd, Vd), sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, offs, False, kd, vd, bt), f"replay {r}")


# ---- 7. the binding ----
def test_the_fronts_take_pos_offsets():
    d, Sq, G, rot, page = 64, 7, 2, 32, 16
    lens = [40, 64]
    parents = [sp.binary(Sq), sp.random_tree(Sq, 81)]
    depths = fa.tree_depths(torch.tensor(parents, device=DEV))
    assert depths.dtype == i32 and depths.is_cuda and depths.tolist() == [sp.depths(p) for p in parents]
    Q, Kn, Vn = rows((B, HKV * G, Sq, d), 82), rows((B, HKV, Sq, d), 83), rows((B, HKV, Sq, d), 84)
    table = fa.rope_table(CAP, rot)
    kd, vd = descales(85, True, HKV)
    bt, Kc, Vc = caches(None, d, True, 86)
    Kd, Vd = dev(Kc), dev(Vc)
    Qo = fa.rope_cache_append(dev(Q), dev(Kn), dev(Vn), kc.as_cache(Kd), kc.as_cache(Vd), dev(table), lens_tensor(lens), interleaved=True,
                              k_descale=dev(kd), v_descale=dev(vd), pos_offsets=depths)
    torch.cuda.synchronize()
    check((Qo, Kd, Vd), sp.rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, depths.tolist(), True, kd, vd), "rope_cache_append(pos_offsets=)")
    bt, Kp, Vp = caches(page, d, False, 87)
    Kd, Vd, Qd = dev(Kp), dev(Vp), dev(Q)
    out = fa.rope_cache_append_paged(Qd, dev(Kn), dev(Vn), kc.as_cache(Kd), kc.as_cache(Vd), dev(bt), dev(table), lens_tensor(lens), Q_out=Qd,
                                     pos_offsets=depths)
    torch.cuda.synchronize()
    assert out is Qd
    check((Qd, Kd, Vd), sp.rope_append_pos(Q, Kn, Vn, Kp, Vp, table, lens, depths.tolist(), False, None, None, bt), "rope_cache_append_paged(pos_offsets=)")
