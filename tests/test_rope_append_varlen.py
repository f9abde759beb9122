"""GPU tests of flash_attention_rope_append_varlen and flash_attention_rope_append_paged_varlen (rope_cache_append_varlen,
rope_cache_append_paged_varlen): the RAGGED cache append with the rotary embedding of K and of the step's Q fused in -- rows packed by
token, a per-sequence row count.  As in tests/test_rope_append.py everything is a comparison of bits with tests/rope_check.py, Qout and
the caches pre-filled and compared whole; the seam the header states -- a sequence's bytes are the uniform call's on that sequence
alone -- is held GPU against GPU; the end-to-end step runs with flash_attention_extend_paged_varlen in one graph."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_append_check as kc  # noqa: E402
import rope_call as call  # noqa: E402
import rope_check as rc  # noqa: E402
from kv_append_check import as_cache, descales, sentinel  # noqa: E402
from kv_cache_check import DEV, assert_close, cu_of, dequantise, gather, i32 as t32, reference_ragged  # noqa: E402
from rope_check import check, qsent, rows, table_of  # noqa: E402

pytestmark = pytest.mark.gpu
bf, i16, u8, i32 = torch.bfloat16, torch.int16, torch.uint8, torch.int32
# the mixed batch: decode rows, idle slots, rows across 16, across a 64-token workgroup, more rows than keys, more than the capacity
SQ = [1, 0, 5, 16, 17, 70, 3, 0, 40, 200]
LENS = [129, -77, 128, 16, 65, 192, 2, 50, 0, 300]
CAP, PAD = 192, 9
SQ_ALL = SQ


def dev(t):
    return None if t is None else t.to(DEV)


def caches(B, Hkv, d, fp8, page, seed):
    if page:
        P, bt = table_of(B, CAP // page, 3, seed)
        return bt, sentinel((P, Hkv, page, d), fp8), sentinel((P, Hkv, page, d), fp8)
    return None, sentinel((B, Hkv, CAP, d), fp8), sentinel((B, Hkv, CAP, d), fp8)


def run(Q, Kn, Vn, Kc, Vc, cs, cu, lens, il, kd, vd, bt=None, Qo=None):
    Qo = dev(qsent(Q.shape) if Qo is None else Qo)
    Kd, Vd = dev(Kc), dev(Vc)
    call.launch(dev(Q), dev(Kn), dev(Vn), Qo, Kd, Vd, dev(cs), t32(lens), il, dev(kd), dev(vd), dev(bt), cu=t32(cu))
    torch.cuda.synchronize()
    return Qo, Kd, Vd


@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [None, 16, 64])
def test_bit_for_bit(page, d, fp8, il):
    B, T = len(SQ), sum(SQ) + PAD
    cu = cu_of(SQ)
    for ri, rot in enumerate((16, d // 2, d)):
        Hkv, G = ((1, 1), (2, 4), (2, 1))[(ri + il) % 3]
        table = fa.rope_table(CAP, rot)
        Q, Kn, Vn = rows((T, Hkv * G, d), 1 + ri), rows((T, Hkv, d), 2 + ri, special=True), rows((T, Hkv, d), 3 + ri, special=True)
        kd, vd = descales(4 + ri, fp8, Hkv)
        bt, Kc, Vc = caches(B, Hkv, d, fp8, page, 5 + ri)
        for L in (LENS, None):
            got = run(Q, Kn, Vn, Kc, Vc, table, cu, L, il, kd, vd, bt)
            want = rc.rope_append_varlen(Q, Kn, Vn, qsent(Q.shape), Kc, Vc, table, cu, L, il, kd, vd, bt)
            check(got, want, f"page {page} d {d} fp8 {fp8} il {il} rot {rot} lens {L}")
            assert bool((got[0].view(i16)[cu[-1]:] == 0x4B4B).all())          # tokens nobody owns (the reference says so too)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d,page", [(64, None), (128, 16)])
def test_seam_every_sequence_is_the_uniform_call_on_that_sequence_alone(d, page, fp8):
    SQ = SQ_ALL[:-1] + [150]                         # (the uniform call takes at most the capacity)
    B, T, Hkv, G, rot = len(SQ), sum(SQ) + PAD, 2, 2, 32
    cu = cu_of(SQ)
    table = fa.rope_table(CAP, rot)
    Q, Kn, Vn = rows((T, Hkv * G, d), 11), rows((T, Hkv, d), 12), rows((T, Hkv, d), 13)
    kd, vd = descales(14, fp8, Hkv)
    bt, Kc, Vc = caches(B, Hkv, d, fp8, page, 15)
    Qo, K, V = run(Q, Kn, Vn, Kc, Vc, table, cu, LENS, True, kd, vd, bt)
    Qd, Knd, Vnd, csd, kdd, vdd = dev(Q), dev(Kn), dev(Vn), dev(table), dev(kd), dev(vd)
    Qo2, K2, V2 = dev(qsent(Q.shape)), dev(Kc), dev(Vc)
    for b, s in enumerate(SQ):
        if s == 0:
            continue
        view = lambda x: x[cu[b]:cu[b + 1]].transpose(0, 1).unsqueeze(0)       # [1, heads, s, d] of the packed rows, no copy
        if page:
            call.launch(view(Qd), view(Knd), view(Vnd), view(Qo2), K2, V2, csd, t32([LENS[b]]), True, kdd, vdd, dev(bt[b:b + 1]))
        else:
            call.launch(view(Qd), view(Knd), view(Vnd), view(Qo2), K2[b:b + 1], V2[b:b + 1], csd, t32([LENS[b]]), True, kdd, vdd)
    torch.cuda.synchronize()
    assert torch.equal(Qo.view(i16), Qo2.view(i16)) and torch.equal(K, K2) and torch.equal(V, V2)


def test_offsets_beyond_total_q_are_clamped():
    Hkv, G, d, rot = 2, 2, 64, 64
    sq = [10, 30, 20]
    cu = cu_of(sq)
    T = 25                                           # sequence 1 keeps 15 of its rows, sequence 2 none
    table = fa.rope_table(CAP, rot)
    Q, Kn, Vn = rows((T, Hkv * G, d), 21), rows((T, Hkv, d), 22), rows((T, Hkv, d), 23)
    bt, Kc, Vc = caches(3, Hkv, d, False, None, 24)
    lens = [50, 60, 70]
    got = run(Q, Kn, Vn, Kc, Vc, table, cu, lens, False, None, None)
    check(got, rc.rope_append_varlen(Q, Kn, Vn, qsent(Q.shape), Kc, Vc, table, cu, lens, False), "clamped offsets")
    assert torch.equal(got[1][2].cpu(), Kc[2])


@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("page", [None, 16])
def test_probes_name_position_and_partner(page, il):
    B, T, Hkv, G, d, rot = len(SQ), sum(SQ) + PAD, 2, 2, 128, 64
    cu = cu_of(SQ)
    table = rc.probe_table(CAP, rot)
    coded = lambda shape, base: (((torch.arange(shape[0] * shape[1] * shape[2]).reshape(shape) * 7 + base) % 251 + 1)
                                 * torch.where(torch.arange(shape[0] * shape[1] * shape[2]).reshape(shape) % 3 == 0, -1, 1)).to(bf)
    Q, Kn, Vn = coded((T, Hkv * G, d), 0), coded((T, Hkv, d), 5), coded((T, Hkv, d), 9)
    bt, Kc, Vc = caches(B, Hkv, d, False, page, 31)
    Qo, K, V = run(Q, Kn, Vn, Kc, Vc, table, cu, LENS, il, None, None, bt)
    wantQ, wantK = qsent(Q.shape), Kc.clone()
    for b, s in enumerate(SQ):
        if s == 0:
            continue
        pos = torch.tensor([rc.q_positions(LENS[b], s, CAP)])
        view = lambda x: x[cu[b]:cu[b + 1]].transpose(0, 1).unsqueeze(0)
        wantQ[cu[b]:cu[b + 1]] = rc.probe_expect(view(Q), pos, rot, il)[0].transpose(0, 1)
        kr = rc.probe_expect(view(Kn), pos, rot, il)
        if page:
            wantK = kc.append(kr, wantK, [LENS[b]], None, bt[b:b + 1])
        else:
            wantK[b:b + 1] = kc.append(kr, wantK[b:b + 1], [LENS[b]])
    rc.assert_same("probe Qout", Qo, wantQ)
    rc.assert_same("probe Kcache", K, wantK)


@pytest.mark.parametrize("fp8", [False, True])
def test_strided_tokens_in_place_and_bad_table_entries(fp8):
    B, T, Hkv, G, d, page, rot = len(SQ), sum(SQ) + PAD, 2, 2, 64, 16, 32
    H = Hkv * G
    cu = cu_of(SQ)
    table = fa.rope_table(CAP, rot)
    kd, vd = descales(41, fp8, Hkv)
    # Q, K and V are slices of one fused [T, (H + 2 Hkv) d] projection; Qout goes in place
    fused = rows((T, (H + 2 * Hkv) * d), 42)
    heads = lambda t: t.view(T, H + 2 * Hkv, d)
    part = lambda t: (heads(t)[:, :H], heads(t)[:, H:H + Hkv], heads(t)[:, H + Hkv:])
    Q, Kn, Vn = part(fused)
    bt, Kc, Vc = caches(B, Hkv, d, fp8, page, 43)
    # a third of the entries that receive rows are out of range
    receives = torch.zeros(B, CAP // page, dtype=torch.bool)
    for b, s in enumerate(SQ):
        for _, p in kc.positions(LENS[b], s, CAP):
            receives[b, p // page] = True
    bad = bt.clone()
    P = Kc.shape[0]
    for k, (b, j) in enumerate(receives.nonzero()[::3].tolist()):
        bad[b, j] = (-1, P, 2 ** 31 - 1, -2 ** 31, P + 5)[k % 5]
    bad = torch.where(receives, bad, torch.full_like(bad, 2 ** 31 - 1))        # ... and the entries that receive none are not read
    fd = dev(fused)
    Qd, Knd, Vnd = part(fd)
    Kd, Vd = dev(Kc), dev(Vc)
    call.launch(Qd, Knd, Vnd, Qd, Kd, Vd, dev(table), t32(LENS), False, dev(kd), dev(vd), dev(bad), cu=t32(cu))
    torch.cuda.synchronize()
    qo, k, v = rc.rope_append_varlen(Q, Kn, Vn, Q.clone(), Kc, Vc, table, cu, LENS, False, kd, vd, bad)
    want = fused.clone()
    heads(want)[:, :H] = qo
    rc.assert_same("the projection", fd, want)
    rc.assert_same("Kcache", Kd, k)
    rc.assert_same("Vcache", Vd, v)


def test_the_fronts_make_the_same_calls():
    B, T, Hkv, G, d, page, rot = len(SQ), sum(SQ) + PAD, 2, 2, 64, 16, 32
    cu = cu_of(SQ)
    table = fa.rope_table(CAP, rot)
    Q, Kn, Vn = rows((T, Hkv * G, d), 51), rows((T, Hkv, d), 52), rows((T, Hkv, d), 53)
    kd, vd = descales(54, True, Hkv)
    for pg in (None, page):
        bt, Kc, Vc = caches(B, Hkv, d, True, pg, 55)
        Kd, Vd, Qo = dev(Kc), dev(Vc), dev(qsent(Q.shape))
        kw = dict(kv_lens=t32(LENS), interleaved=True, k_descale=dev(kd), v_descale=dev(vd), Q_out=Qo)
        if pg:
            out = fa.rope_cache_append_paged_varlen(dev(Q), dev(Kn), dev(Vn), as_cache(Kd), as_cache(Vd), dev(bt), t32(cu), dev(table), **kw)
        else:
            out = fa.rope_cache_append_varlen(dev(Q), dev(Kn), dev(Vn), as_cache(Kd), as_cache(Vd), t32(cu), dev(table), **kw)
        torch.cuda.synchronize()
        assert out.data_ptr() == Qo.data_ptr() and out.shape == Qo.shape
        check((Qo, Kd, Vd), rc.rope_append_varlen(Q, Kn, Vn, qsent(Q.shape), Kc, Vc, table, cu, LENS, True, kd, vd, bt), f"front, page {pg}")


def test_mixed_batch_steps_as_one_graph():
    """`kv_lens += q_lens; rope_append_paged_varlen; flash_attention_extend_paged_varlen` into a page-16 fp8 pool: one graph, captured
    once at a fixed totalQ and replayed for three steps with cu_seqlens_q and the lengths changed in place.  Sequence 0 goes from a
    96-row chunk to a 40-row chunk to 1-row decode; sequence 1 decodes behind 57 cached keys and then goes idle; sequence 2 joins at
    step 1; slot 3 stays idle.  Caches and Qout against the reference; O / LSE bit for bit against the same attention call on the
    reference's tensors, and by kv_cache_check.assert_close against float64 attention on them"""
    B, Hkv, G, d, page, n, T, rot = 4, 2, 4, 128, 16, 16, 128, 64
    H, cap = Hkv * G, n * page
    steps = [[96, 1, 0, 0], [40, 1, 30, 0], [1, 0, 2, 0]]
    start = [0, 57, 0, 0]
    mk = lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(bf)
    kd, vd = torch.tensor([0.02, 0.031]), torch.tensor([0.017, 0.025])
    table = fa.rope_table(cap, rot)
    P, bt = table_of(B, n, 3, 153)
    refK, refV = sentinel((P, Hkv, page, d), True), sentinel((P, Hkv, page, d), True)
    _, refK, refV, _ = rc.rope_append(mk((B, H, 57, d), 150), mk((B, Hkv, 57, d), 151), mk((B, Hkv, 57, d), 152), refK, refV, table, start, False,
                                      kd, vd, bt)
    Kp, Vp, td, csd, kdd, vdd = dev(refK), dev(refV), dev(bt), dev(table), dev(kd), dev(vd)
    lens, cu, q_lens = t32(start), t32([0] * (B + 1)), t32([0] * B)
    Qs, Qr = torch.zeros((T, H, d), dtype=bf, device=DEV), torch.zeros((T, H, d), dtype=bf, device=DEV)
    Kn, Vn = (torch.zeros((T, Hkv, d), dtype=bf, device=DEV) for _ in range(2))
    Os = torch.zeros((T, H, d), dtype=torch.float32, device=DEV)
    ws = torch.empty(fa.decode_workspace_size(1, H, T, d, 2), dtype=u8, device=DEV)
    akw = dict(is_causal=True, num_splits=2, return_lse=True, k_descale=kdd, v_descale=vdd)

    def step():
        lens.add_(q_lens)
        call.launch(Qs, Kn, Vn, Qr, Kp, Vp, csd, lens, False, kdd, vdd, td, cu=cu)
        return fa.flash_attention_extend_paged_varlen(Qr, as_cache(Kp), as_cache(Vp), td, cu, lens, O=Os, workspace=ws, **akw)

    step()                                                       # every kernel has run once before the capture (all slots idle)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse_s = step()
    pos = list(start)
    for it, sq in enumerate(steps):
        c = cu_of(sq)
        q, kn, vn = mk((T, H, d), 160 + it), mk((T, Hkv, d), 170 + it), mk((T, Hkv, d), 180 + it)
        Qs.copy_(q); Kn.copy_(kn); Vn.copy_(vn); cu.copy_(t32(c)); q_lens.copy_(t32(sq))
        Qr.copy_(qsent(q.shape))
        Os.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        pos = [p + s for p, s in zip(pos, sq)]
        assert lens.tolist() == pos
        qr, refK, refV = rc.rope_append_varlen(q, kn, vn, qsent(q.shape), refK, refV, table, c, pos, False, kd, vd, bt)
        check((Qr, Kp, Vp), (qr, refK, refV), f"step {it}")
        O, lse = Os.clone(), lse_s.clone()
        O2 = torch.zeros_like(Os)
        _, lse2 = fa.flash_attention_extend_paged_varlen(dev(qr), as_cache(dev(refK)), as_cache(dev(refV)), td, cu, lens, O=O2, **akw)
        torch.cuda.synchronize()
        owned = torch.zeros(T, dtype=torch.bool)
        owned[:c[-1]] = True
        assert torch.equal(O[owned], O2[owned]) and torch.equal(lse[:, owned], lse2[:, owned]), it
        K64, V64 = gather(dequantise(refK, kd), bt), gather(dequantise(refV, vd), bt)
        refO, refL, own = reference_ragged(qr, K64, V64, sq, pos, True)
        assert torch.equal(own, owned)
        assert_close(O[owned], lse[:, owned], refO[owned], refL[:, owned], f"rope ragged step {it} rows {sq} lengths {pos}")
