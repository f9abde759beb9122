"""GPU tests of flash_attention_rope_append and flash_attention_rope_append_paged (rope_cache_append, rope_cache_append_paged): the K/V
cache append with the rotary embedding of K and of the step's Q fused in.

Everything is a comparison of BITS with tests/rope_check.py, the header's contract in torch on the CPU (held against exact rational
arithmetic and against nine wrong implementations in tests/test_rope_check.py): Qout, the K cache and the V cache as integers, NaN
codes by class, no tolerance -- but in the end-to-end steps, whose O and LSE are held bit for bit against the same attention call on
the reference's tensors and, by kv_cache_check.assert_close, against float64 attention on them.  Caches and Qout are pre-filled with a
sentinel and compared WHOLE, padding and spare pages included, so what must not be written is checked with what must.  The calls go
through the C ABI by name (tests/rope_call.py); the attention calls of the end-to-end steps through the binding."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_append_check as kc  # noqa: E402
from kv_append_check import SENT, as_cache, descales, sentinel  # noqa: E402
import rope_call as call  # noqa: E402
import rope_check as rc  # noqa: E402
from kv_cache_check import DEV, assert_close, dequantise, gather, i32 as lens_tensor, reference  # noqa: E402
from rope_check import check, qsent, rows, table_of  # noqa: E402

pytestmark = pytest.mark.gpu
bf, i16, u8, i32 = torch.bfloat16, torch.int16, torch.uint8, torch.int32
def dev(t):
    return None if t is None else t.to(DEV)


def run(Q, Kn, Vn, Kc, Vc, cs, lens, il, kd, vd, table=None, Qo=None):
    """the call on copies of the CPU tensors -> (Qout, K cache, V cache) on the device; Qo: what Qout holds before (default: the
    sentinel)"""
    Qo = dev(qsent(Q.shape) if Qo is None else Qo)
    Kd, Vd = dev(Kc), dev(Vc)
    call.launch(dev(Q), dev(Kn), dev(Vn), Qo, Kd, Vd, dev(cs), lens_tensor(lens), il, dev(kd), dev(vd), dev(table))
    torch.cuda.synchronize()
    return Qo, Kd, Vd


def lengths(Sq, cap, page):
    """lengths that put `first` = L - Sq and L on either side of a 16-position wave, a 64-position block and a page boundary; fewer
    keys than rows; inactive slots; lengths above the capacity"""
    out = {-3, 0, 1, Sq - 1, Sq, Sq + 1, cap - 1, cap, cap + 7}
    for edge in {16, 64, page, 128, 2 * page}:
        for x in (edge - 1, edge, edge + 1):
            out |= {x, x + Sq}
    return sorted(L for L in out if L <= cap + 7)


HEADS = {0: (1, 1), 1: (2, 4), 2: (2, 1)}       # by the index of rotDim: (Hkv, G)


# ---- 1. bit for bit against the reference ----
@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [None, 16, 64])
def test_bit_for_bit(page, d, fp8, il):
    cap = 192
    for ri, rot in enumerate((16, d // 2, d)):
        Hkv, G = HEADS[ri] if not il else HEADS[(ri + 1) % 3]
        table = fa.rope_table(cap, rot)
        for Sq in (1, 3, 16, 40, 70):
            every = lengths(Sq, cap, page or 32)
            for at in range(0, len(every), 3):
                lens = every[at:at + 3]
                B = len(lens)
                Q, Kn, Vn = rows((B, Hkv * G, Sq, d), 1 + Sq), rows((B, Hkv, Sq, d), 2 + Sq, special=True), rows((B, Hkv, Sq, d), 3 + Sq, special=True)
                kd, vd = descales(4 + Sq, fp8, Hkv)
                if page:
                    n = cap // page
                    P, bt = table_of(B, n, 3, 5 + Sq + at)
                    Kc, Vc = sentinel((P, Hkv, page, d), fp8), sentinel((P, Hkv, page, d), fp8)
                else:
                    bt, Kc, Vc = None, sentinel((B, Hkv, cap, d), fp8), sentinel((B, Hkv, cap, d), fp8)
                for L in ((lens, None) if at == 0 else (lens,)):
                    got = run(Q, Kn, Vn, Kc, Vc, table, L, il, kd, vd, bt)
                    want = rc.rope_append(Q, Kn, Vn, Kc, Vc, table, L, il, kd, vd, bt)[:3]
                    check(got, want, f"page {page} d {d} fp8 {fp8} il {il} rot {rot} Sq {Sq} lens {L}")


def test_a_slice_of_several_heads():
    """enough (sequence, position block) pairs -- 1040, against the eight workgroups per CU the host aims at -- that one workgroup takes
    two or all four of the K/V heads: the loop over a slice's heads, and over several batches of its units"""
    B, Hkv, G, Sq, d, cap = 520, 4, 4, 3, 64, 64
    table = fa.rope_table(cap, 32)
    lens = [(37 * b) % (cap + 20) - 5 for b in range(B)]
    Q, Kn, Vn = rows((B, Hkv * G, Sq, d), 11), rows((B, Hkv, Sq, d), 12), rows((B, Hkv, Sq, d), 13)
    kd, vd = descales(14, True, Hkv)
    Kc, Vc = sentinel((B, Hkv, cap, d), True), sentinel((B, Hkv, cap, d), True)
    check(run(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd), rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd)[:3], "slices")


# ---- 2. exact probes: every output element is +- one named input element ----
@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("d,rot", [(64, 64), (64, 16), (128, 64), (128, 128)])
@pytest.mark.parametrize("page", [None, 16])
def test_probes_name_position_and_partner(page, d, rot, il):
    B, Hkv, G, Sq, cap = 3, 2, 2, 21, 128
    lens = [77, 12, 128]
    table = rc.probe_table(cap, rot)

    def coded(shape, base):      # index-coded: |value| = 1 .. 251 by the flat index, exact in bf16, never zero
        n = torch.arange(shape[0] * shape[1] * shape[2] * shape[3]).reshape(shape)
        return (((n * 7 + base) % 251 + 1) * torch.where(n % 3 == 0, -1, 1)).to(bf)

    Q, Kn, Vn = coded((B, Hkv * G, Sq, d), 0), coded((B, Hkv, Sq, d), 5), coded((B, Hkv, Sq, d), 9)
    if page:
        P, bt = table_of(B, cap // page, 2, 21)
        Kc, Vc = sentinel((P, Hkv, page, d), False), sentinel((P, Hkv, page, d), False)
    else:
        bt, Kc, Vc = None, sentinel((B, Hkv, cap, d), False), sentinel((B, Hkv, cap, d), False)
    Qo, K, V = run(Q, Kn, Vn, Kc, Vc, table, lens, il, None, None, bt)
    pos = torch.tensor([rc.q_positions(L, Sq, cap) for L in lens])
    rc.assert_same("probe Qout", Qo, rc.probe_expect(Q, pos, rot, il))
    rc.assert_same("probe Kcache", K, kc.append(rc.probe_expect(Kn, pos, rot, il), Kc, lens, None, bt))
    rc.assert_same("probe Vcache", V, kc.append(Vn, Vc, lens, None, bt))


# ---- 3. seams ----
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 64])
def test_seams_with_the_plain_append(page, fp8):
    B, Hkv, G, Sq, d, cap, rot = 3, 2, 4, 40, 128, 256, 64
    lens = [200, 33, 256]
    Q, Kn, Vn = rows((B, Hkv * G, Sq, d), 31), rows((B, Hkv, Sq, d), 32), rows((B, Hkv, Sq, d), 33, special=True)
    kd, vd = descales(34, fp8, Hkv)
    table = fa.rope_table(cap, rot)
    if page:
        P, bt = table_of(B, cap // page, 3, 35)
        Kc, Vc = sentinel((P, Hkv, page, d), fp8), sentinel((P, Hkv, page, d), fp8)
    else:
        bt, Kc, Vc = None, sentinel((B, Hkv, cap, d), fp8), sentinel((B, Hkv, cap, d), fp8)
    ld, btd, kdd, vdd = lens_tensor(lens), dev(bt), dev(kd), dev(vd)

    def plain(K_rows, V_rows):
        Kd, Vd = dev(Kc), dev(Vc)
        call.twin(dev(K_rows), dev(V_rows), Kd, Vd, ld, kdd, vdd, btd)
        torch.cuda.synchronize()
        return Kd, Vd

    # the fused caches are the plain append's of the reference's bf16 rotation of K, and of V itself (NaN payloads and -0 in it):
    # byte for byte, NaN codes included -- the same instructions made them
    Qo, K, V = run(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd, bt)
    Krot = rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd, bt)[3]
    K2, V2 = plain(Krot, Vn)
    assert torch.equal(K, K2) and torch.equal(V, V2)
    # the identity table: the plain append of K itself (finite, no -0), and Qout == Q
    ident = torch.cat([torch.ones(cap, rot // 2), torch.zeros(cap, rot // 2)], 1)
    Qf, Kf = rows((B, Hkv * G, Sq, d), 36), rows((B, Hkv, Sq, d), 37)
    assert bool(torch.isfinite(Kf.float()).all()) and not bool((Kf.view(i16) == -0x8000).any()) and not bool((Qf.view(i16) == -0x8000).any())
    Qo, K, V = run(Qf, Kf, Vn, Kc, Vc, ident, lens, False, kd, vd, bt)
    K2, V2 = plain(Kf, Vn)
    assert torch.equal(K, K2) and torch.equal(V, V2) and torch.equal(Qo.view(i16), dev(Qf).view(i16))
    # in place equals out of place
    Qo, K, V = run(Q, Kn, Vn, Kc, Vc, table, lens, True, kd, vd, bt)
    Qd, Kd, Vd = dev(Q), dev(Kc), dev(Vc)
    call.launch(Qd, dev(Kn), dev(Vn), Qd, Kd, Vd, dev(table), ld, True, kdd, vdd, btd)
    torch.cuda.synchronize()
    assert torch.equal(Qd.view(i16), Qo.view(i16)) and torch.equal(Kd, K) and torch.equal(Vd, V)
    # paged equals contiguous on a gathered copy
    if page:
        Qc, K3, V3 = run(Q, Kn, Vn, sentinel((B, Hkv, cap, d), fp8), sentinel((B, Hkv, cap, d), fp8), table, lens, True, kd, vd)
        assert torch.equal(gather(K, btd), K3) and torch.equal(gather(V, btd), V3) and torch.equal(Qc.view(i16), Qo.view(i16))


# ---- 4. nothing else is written ----
@pytest.mark.parametrize("fp8", [False, True])
def test_bad_table_entries_skip_k_and_v_not_q(fp8):
    B, Hkv, G, Sq, d, page, n, rot = 3, 2, 2, 40, 64, 16, 12, 32
    cap = n * page
    lens = [100, 7, cap]
    Q, Kn, Vn = rows((B, Hkv * G, Sq, d), 41), rows((B, Hkv, Sq, d), 42), rows((B, Hkv, Sq, d), 43)
    kd, vd = descales(44, fp8, Hkv)
    table = fa.rope_table(cap, rot)
    P, bt = table_of(B, n, 3, 45)
    Kc, Vc = sentinel((P, Hkv, page, d), fp8), sentinel((P, Hkv, page, d), fp8)
    base = run(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd, bt)
    check(base, rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd, bt)[:3], "the table as it is")
    receives = torch.zeros(B, n, dtype=torch.bool)
    for b, L in enumerate(lens):
        for _, p in kc.positions(L, Sq, cap):
            receives[b, p // page] = True
    assert int((~receives).sum()) > 0 and int(receives.sum()) > 3
    # entries of pages that receive no row are not read: any int32 there, the same bytes everywhere
    for junk in (-1, 2 ** 31 - 1, P + 5):
        got = run(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd, torch.where(receives, bt, torch.full_like(bt, junk)))
        assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, base)), junk
    # entries outside [0, P) at pages that receive rows: those K / V rows are skipped, never clamped; every Q row is still written
    t3 = bt.clone()
    for k, (b, j) in enumerate(receives.nonzero()[::2].tolist()):
        t3[b, j] = (-1, P, 2 ** 31 - 1, -2 ** 31, P + 5)[k % 5]
    got = run(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd, t3)
    check(got, rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd, t3)[:3], "entries out of range")
    assert torch.equal(got[0].view(i16), base[0].view(i16))
    skipped = torch.zeros(P, dtype=torch.bool)
    skipped[bt[t3 != bt].long()] = True
    assert bool((got[1].cpu()[skipped] == SENT[Kc.dtype]).all()) and bool((got[2].cpu()[skipped] == SENT[Kc.dtype]).all())


def bits(t):
    return t.view(i16) if t.dtype == bf else t


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_strided_rows_and_a_fused_projection_keep_their_padding(d, fp8):
    B, Hkv, G, Sq, cap, rot = 2, 2, 2, 19, 96, d // 2
    H = Hkv * G
    lens = [50, 96]
    kd, vd = descales(51 + d, fp8, Hkv)
    table = fa.rope_table(cap, rot)
    # Q, K and V are slices of one fused [B, Sq, (H + 2 Hkv) d] projection; Qout goes IN PLACE into the projection
    fused = rows((B, Sq, (H + 2 * Hkv) * d), 52 + d)
    fd = dev(fused)
    heads = lambda t: t.view(B, Sq, H + 2 * Hkv, d)
    part = lambda t: (heads(t)[:, :, :H].transpose(1, 2), heads(t)[:, :, H:H + Hkv].transpose(1, 2), heads(t)[:, :, H + Hkv:].transpose(1, 2))
    Q, Kn, Vn = part(fused)
    Qd, Knd, Vnd = part(fd)
    # caches with row strides d + 16 (K) and d + 32 (V)
    rawK, rawV = sentinel((B, Hkv, cap, d + 16), fp8), sentinel((B, Hkv, cap, d + 32), fp8)
    Kd, Vd = dev(rawK), dev(rawV)
    call.launch(Qd, Knd, Vnd, Qd, Kd[..., :d], Vd[..., :d], dev(table), lens_tensor(lens), True, dev(kd), dev(vd))
    torch.cuda.synchronize()
    qo, k, v, _ = rc.rope_append(Q, Kn, Vn, rawK[..., :d].contiguous(), rawV[..., :d].contiguous(), table, lens, True, kd, vd)
    want = fused.clone()
    heads(want)[:, :, :H] = qo.transpose(1, 2)
    rc.assert_same("the projection", fd, want)                   # the K and V slices as they were, Q rotated
    wantK, wantV = rawK.clone(), rawV.clone()
    wantK[..., :d], wantV[..., :d] = k, v
    rc.assert_same("K rows of d + 16", Kd, wantK)
    rc.assert_same("V rows of d + 32", Vd, wantV)
    # Qout with rows of d + 16 of its own
    rawQo = qsent((B, H, Sq, d + 16), DEV)
    Kd, Vd = dev(rawK), dev(rawV)
    call.launch(dev(Q), dev(Kn), dev(Vn), rawQo[..., :d], Kd[..., :d], Vd[..., :d], dev(table), lens_tensor(lens), True, dev(kd), dev(vd))
    torch.cuda.synchronize()
    wantQ = qsent((B, H, Sq, d + 16))
    wantQ[..., :d] = qo
    rc.assert_same("Qout rows of d + 16", rawQo, wantQ)
    rc.assert_same("K rows of d + 16", Kd, wantK)


# ---- 5. a pool just above 2^32 bytes ----
def test_page_bases_are_64_bit():
    Hkv, G, page, d, Sq, rot = 2, 1, 128, 128, 3, 128
    per_page = Hkv * page * d                       # bytes of one fp8 page
    P = (1 << 32) // per_page + 8
    Kp, Vp = torch.empty((P, Hkv, page, d), dtype=u8, device=DEV), torch.empty((P, Hkv, page, d), dtype=u8, device=DEV)
    assert Kp.numel() > 1 << 32
    hi = P - 1                                      # rows land in the LAST page
    alias = hi - (1 << 32) // per_page              # where a 32-bit byte offset of page `hi` would land
    assert 0 <= alias < P and hi * per_page >= 1 << 32
    for pool in (Kp, Vp):
        pool[hi] = SENT[u8]
        pool[alias] = SENT[u8]
    bt = torch.tensor([[alias + 1, hi, alias + 2]], dtype=i32)     # positions 128 .. 255 live in page `hi`
    lens = [page + 70]
    Q, Kn, Vn = rows((1, Hkv * G, Sq, d), 60), rows((1, Hkv, Sq, d), 61), rows((1, Hkv, Sq, d), 62)
    kd, vd = descales(63, True, Hkv)
    table = fa.rope_table(3 * page, rot)
    Qo = qsent(Q.shape, DEV)
    call.launch(dev(Q), dev(Kn), dev(Vn), Qo, Kp, Vp, dev(table), lens_tensor(lens), False, dev(kd), dev(vd), dev(bt))
    torch.cuda.synchronize()
    pos = torch.tensor([rc.q_positions(lens[0], Sq, 3 * page)])
    assert pos.tolist() == [[195, 196, 197]]
    rc.assert_same("Qout", Qo, rc.rotate(Q, table, pos, False))
    for pool, new, ds in ((Kp, rc.rotate(Kn, table, pos, False), kd), (Vp, Vn, vd)):
        want = sentinel((1, Hkv, page, d), True)
        want[0, :, 70 - Sq:70] = kc.encode(new, ds, True)[0]
        rc.assert_same("the last page", pool[hi][None], want)
        assert bool((pool[alias] == SENT[u8]).all())


# ---- 6. a decode step end to end, one graph ----
@pytest.mark.parametrize("fp8,Sq,d,il", [(True, 1, 128, False), (True, 4, 64, True), (False, 1, 64, True), (False, 4, 128, False)])
def test_decode_step_in_one_graph(fp8, Sq, d, il):
    B, Hkv, G, page, n, steps, rot = 2, 2, 2, 16, 20, 6, d // 2
    H, cap = G * Hkv, n * page
    start = [125, 13]
    P, bt = table_of(B, n, 5, 90 + Sq)
    kd, vd = (torch.tensor([0.02, 0.031]), torch.tensor([0.017, 0.025])) if fp8 else (None, None)
    table = fa.rope_table(cap, rot)
    mk = lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(bf)
    # the history: the CPU writer fills the pools up to the starting lengths (rotated like everything that follows)
    refK, refV = sentinel((P, Hkv, page, d), fp8), sentinel((P, Hkv, page, d), fp8)
    for b, L in enumerate(start):
        one = [L if x == b else 0 for x in range(B)]
        _, refK, refV, _ = rc.rope_append(mk((B, H, L, d), 95), mk((B, Hkv, L, d), 91 + b), mk((B, Hkv, L, d), 93 + b), refK, refV, table, one,
                                          il, kd, vd, bt)
    Kp, Vp, td, csd = dev(refK), dev(refV), dev(bt), dev(table)
    lens = torch.tensor(start, dtype=i32, device=DEV)
    Kn_s, Vn_s = torch.zeros((B, Hkv, Sq, d), dtype=bf, device=DEV), torch.zeros((B, Hkv, Sq, d), dtype=bf, device=DEV)
    Q_s, Qr_s = torch.zeros((B, H, Sq, d), dtype=bf, device=DEV), torch.zeros((B, H, Sq, d), dtype=bf, device=DEV)
    O_s = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
    ns = 2
    ws = torch.empty(fa.decode_workspace_size(B, H, Sq, d, ns), dtype=u8, device=DEV)
    ds = dict(k_descale=dev(kd), v_descale=dev(vd)) if fp8 else {}
    dkw = dict(is_causal=True, num_splits=ns, return_lse=True, **ds)

    def step():
        lens.add_(Sq)
        call.launch(Q_s, Kn_s, Vn_s, Qr_s, Kp, Vp, csd, lens, il, ds.get("k_descale"), ds.get("v_descale"), td)
        return fa.flash_attention_decode_paged(Qr_s, as_cache(Kp), as_cache(Vp), td, lens, O=O_s, workspace=ws, **dkw)

    step()                                    # (first calls outside the capture; then the state as it was)
    torch.cuda.synchronize()
    lens.copy_(torch.tensor(start, dtype=i32))
    Kp.copy_(refK)
    Vp.copy_(refV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse_s = step()
    lens.copy_(torch.tensor(start, dtype=i32))
    now = list(start)
    for t in range(steps):
        Kn, Vn, Q = mk((B, Hkv, Sq, d), 100 + t), mk((B, Hkv, Sq, d), 200 + t), mk((B, H, Sq, d), 300 + t)
        Kn_s.copy_(Kn)
        Vn_s.copy_(Vn)
        Q_s.copy_(Q)
        graph.replay()
        torch.cuda.synchronize()
        now = [L + Sq for L in now]
        assert lens.tolist() == now
        Qr, refK, refV, _ = rc.rope_append(Q, Kn, Vn, refK, refV, table, now, il, kd, vd, bt)
        check((Qr_s, Kp, Vp), (Qr, refK, refV), f"step {t}")
        O, lse = O_s.clone(), lse_s.clone()
        # the same decode call on the reference's tensors: the same bits
        O2, lse2 = fa.flash_attention_decode_paged(dev(Qr), as_cache(dev(refK)), as_cache(dev(refV)), td, lens, out_dtype=torch.float32, **dkw)
        torch.cuda.synchronize()
        assert torch.equal(O, O2) and torch.equal(lse, lse2), t
        # ... and float64 attention on the values they hold
        Kg, Vg = gather(refK, bt), gather(refV, bt)
        Kf, Vf = (dequantise(Kg, kd), dequantise(Vg, vd)) if fp8 else (Kg.view(bf), Vg.view(bf))
        refO, refL = reference(Qr, Kf, Vf, now, True, 0)
        assert_close(O, lse, refO, refL, f"rope decode step {t} fp8 {fp8} Sq {Sq} d {d} lengths {now}")
    assert now[0] > 128 >= start[0] and now[1] > 16 >= start[1]          # the steps crossed the tile and a page boundary


# ---- 7. determinism and streams ----
@pytest.mark.parametrize("fp8", [True, False])
def test_the_same_call_gives_the_same_bytes_and_a_side_stream_orders_it(fp8):
    B, Hkv, G, Sq, d, cap, rot = 3, 2, 4, 40, 128, 320, 128
    lens = [cap, 200, 7]
    Q, Kn, Vn = rows((B, Hkv * G, Sq, d), 110), rows((B, Hkv, Sq, d), 111), rows((B, Hkv, Sq, d), 112)
    kd, vd = descales(113, fp8, Hkv)
    table = fa.rope_table(cap, rot)
    Kc, Vc = sentinel((B, Hkv, cap, d), fp8), sentinel((B, Hkv, cap, d), fp8)
    want = rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd)[:3]
    a, b = run(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd), run(Q, Kn, Vn, Kc, Vc, table, lens, False, kd, vd)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    check(a, want, "twice")
    # a side stream: the rows are produced on it just before the call, and the result is read after it alone is waited for
    side = torch.cuda.Stream()
    Qd, Knd, Vnd, ld, csd, kdd, vdd = dev(Q), dev(Kn), dev(Vn), lens_tensor(lens), dev(table), dev(kd), dev(vd)
    sq, sk, sv = torch.zeros_like(Qd), torch.zeros_like(Knd), torch.zeros_like(Vnd)
    Qo, Kd, Vd = qsent(Q.shape, DEV), dev(Kc), dev(Vc)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sq.copy_(Qd)
        sk.copy_(Knd)
        sv.copy_(Vnd)
    call.launch(sq, sk, sv, Qo, Kd, Vd, csd, ld, False, kdd, vdd, stream=side)
    side.synchronize()
    check((Qo, Kd, Vd), want, "side stream")


# ---- 8. the binding ----
def test_the_fronts_make_the_same_calls():
    B, Hkv, G, Sq, d, cap, page, rot = 2, 2, 2, 5, 64, 64, 16, 32
    lens = [40, 64]
    Q, Kn, Vn = rows((B, Hkv * G, Sq, d), 120), rows((B, Hkv, Sq, d), 121), rows((B, Hkv, Sq, d), 122)
    table = fa.rope_table(cap, rot)
    Kc, Vc = sentinel((B, Hkv, cap, d), True), sentinel((B, Hkv, cap, d), True)
    kd, vd = descales(123, True, Hkv)
    Kd, Vd = dev(Kc), dev(Vc)
    Qo = fa.rope_cache_append(dev(Q), dev(Kn), dev(Vn), as_cache(Kd), as_cache(Vd), dev(table), lens_tensor(lens), interleaved=True,
                              k_descale=dev(kd), v_descale=dev(vd))
    torch.cuda.synchronize()
    check((Qo, Kd, Vd), rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, True, kd, vd)[:3], "rope_cache_append")
    P, bt = table_of(B, cap // page, 2, 124)
    Kp, Vp = sentinel((P, Hkv, page, d), False), sentinel((P, Hkv, page, d), False)
    Kd, Vd, Qd = dev(Kp), dev(Vp), dev(Q)
    out = fa.rope_cache_append_paged(Qd, dev(Kn), dev(Vn), as_cache(Kd), as_cache(Vd), dev(bt), dev(table), lens_tensor(lens), Q_out=Qd)
    torch.cuda.synchronize()
    assert out is Qd
    check((Qd, Kd, Vd), rc.rope_append(Q, Kn, Vn, Kp, Vp, table, lens, False, None, None, bt)[:3], "rope_cache_append_paged")
