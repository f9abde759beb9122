"""GPU tests of flash_attention_kv_accept and flash_attention_kv_accept_paged (kv_cache_accept, kv_cache_accept_paged): the accepted path
of a verified draft tree moved, inside the K/V caches, to the front of the draft's slots.

The WHOLE cache or pool is compared byte for byte with tests/spec_step_check.py's `accept()` -- the header's sequential rule on the CPU,
held against five wrong kernels in tests/test_spec_step_abi.py -- so "nothing else is written" is part of every case.  The caches hold
random BYTES, every NaN code of either format among them: the move is a copy of bits, and torch.equal on integers is the comparison.
The calls go through the C ABI by name (tests/spec_step_call.py)."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_append_check as kc  # noqa: E402
import spec_step_call as call  # noqa: E402
import spec_step_check as sp  # noqa: E402
from kv_cache_check import DEV, i32 as lens_tensor, random_table  # noqa: E402

pytestmark = pytest.mark.gpu
i16, u8, i32 = torch.int16, torch.uint8, torch.int32
B, HKV, CAP = 2, 2, 384
SQS = (1, 5, 16, 33, 64)


def dev(t):
    return None if t is None else t.to(DEV)


def random_cache(shape, fp8, seed):
    """random bytes: every bit pattern of the format, NaN codes among them, so that a row is told from every other"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, tuple(shape[:-1]) + (shape[-1] * (1 if fp8 else 2),), generator=g, dtype=torch.int32).to(u8)
    return raw if fp8 else raw.view(i16)


def caches(page, d, fp8, seed, spare=3):
    if page:
        n = CAP // page
        bt = random_table(B, n, seed, spare)
        P = B * n + spare
        return bt, random_cache((P, HKV, page, d), fp8, seed + 1), random_cache((P, HKV, page, d), fp8, seed + 2)
    return None, random_cache((B, HKV, CAP, d), fp8, seed + 1), random_cache((B, HKV, CAP, d), fp8, seed + 2)


def run(Kc, Vc, idx, nacc, lens, bt=None):
    Kd, Vd = dev(Kc), dev(Vc)
    call.accept(Kd, Vd, torch.tensor(idx, dtype=i32).to(DEV), torch.tensor(nacc, dtype=i32).to(DEV), lens_tensor(lens), dev(bt))
    torch.cuda.synchronize()
    return Kd.cpu(), Vd.cpu()


def check(Kc, Vc, idx, nacc, lens, bt, what):
    Sq = len(idx[0])
    got = run(Kc, Vc, idx, nacc, lens, bt)
    want = sp.accept(Kc, Vc, lens, idx, nacc, Sq, bt)
    for name, g, w in zip("KV", got, want):
        if not torch.equal(g, w):
            at = tuple(int(i) for i in (g != w).nonzero()[0])
            raise AssertionError(f"{what}: {name}cache{list(at)}: got {int(g[at]):#x}, want {int(w[at]):#x} ({int((g != w).sum())} elements differ)")
    return got, want


def pad(path, Sq):
    return list(path) + [Sq - 1] * (Sq - len(path))


def paths(Sq, seed):
    """[(accept_idx of one sequence, n)]: identity; the chain 1, 2, ...; the last leaf's path of a binary tree; random increasing
    subsets; n = 0, Sq, -3, Sq + 7"""
    g = torch.Generator().manual_seed(seed)
    subset = lambda k: sorted(torch.randperm(Sq, generator=g)[:k].tolist())
    out = [(list(range(Sq)), Sq), (pad(range(1, Sq), Sq), Sq - 1), sp.tree_path(sp.binary(Sq), Sq - 1),
           (pad(subset(max(Sq // 2, 1)), Sq), max(Sq // 2, 1)), (pad(subset(max(Sq - 1, 1)), Sq), max(Sq - 1, 1)),
           (pad(subset(1), Sq), 0), (pad(subset(max(Sq // 3, 1)), Sq), -3), (pad(range(1, Sq), Sq), Sq + 7),
           (sp.tree_path(sp.random_tree(Sq, seed), Sq // 2)[0], Sq)]
    return out


# ---- 1. the four cache forms, both head dimensions, every draft size ----
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [None, 16, 128])
def test_byte_for_byte(page, d, fp8):
    bt, Kc, Vc = caches(page, d, fp8, 100 + d)
    p = page or 64
    for Sq in SQS:
        every = paths(Sq, 7 * Sq)
        # lengths: the draft inside one page, across one page start and (page 16: Sq = 33, 64) across two and more; at the front of the
        # cache; up to the capacity and beyond it; fewer keys than draft nodes; an inactive slot
        lens = [Sq + p + 3, Sq + 2 * p - max(Sq // 2, 1), Sq, CAP, CAP + 9, Sq + 3 * p - 1, Sq - 1, 0, -4, Sq + 1]
        for k, (idx, n) in enumerate(every):
            other = every[(k + 3) % len(every)]
            L = [lens[k % len(lens)], lens[(k + 5) % len(lens)]]
            check(Kc, Vc, [idx, other[0]], [n, other[1]], L, bt, f"page {page} d {d} fp8 {fp8} Sq {Sq} path {k} lens {L}")
        check(Kc, Vc, [every[1][0], every[2][0]], [every[1][1], every[2][1]], None, bt, f"page {page} Sq {Sq} without lengths")
        (K, V), _ = check(Kc, Vc, [every[0][0]] * B, [Sq, Sq], [Sq + p + 3, CAP], bt, f"page {page} Sq {Sq} identity")
        assert torch.equal(K, Kc) and torch.equal(V, Vc)        # identity: no byte changes


def test_the_chain_moves_every_row_one_down():
    """accept_idx = 1, 2, 3, ...: every destination is the previous move's source -- the case a lane-per-move kernel gets wrong"""
    d, Sq = 128, 64
    _, Kc, Vc = caches(None, d, False, 200)
    lens = [300, Sq]
    (K, V), _ = check(Kc, Vc, [pad(range(1, Sq), Sq)] * B, [Sq - 1, Sq - 1], lens, None, "the chain")
    for b, L in enumerate(lens):
        base = L - Sq
        assert torch.equal(K[b, :, base:base + Sq - 1], Kc[b, :, base + 1:base + Sq]) and torch.equal(V[b, :, base:base + Sq - 1], Vc[b, :, base + 1:base + Sq])
        assert torch.equal(K[b, :, base + Sq - 1], Kc[b, :, base + Sq - 1])


# ---- 2. any index list gives the sequential rule ----
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16])
def test_indices_out_of_range_and_out_of_order_follow_the_sequential_rule(page, fp8):
    d = 64
    bt, Kc, Vc = caches(page, d, fp8, 300)
    g = torch.Generator().manual_seed(301)
    for Sq in (5, 16, 33, 64):
        wild = [(-5, Sq + 9, 2 ** 31 - 1, -2 ** 31, i)[i % 5] for i in range(Sq)]
        down = list(range(Sq - 1, -1, -1))                      # descending: sources that earlier moves have overwritten
        back = [max(t - 1, 0) for t in range(Sq)]               # each move reads the row the previous one wrote, inside a batch and across
        swap = [t ^ 1 if (t ^ 1) < Sq else t for t in range(Sq)]
        rand = [torch.randint(0, Sq, (Sq,), generator=g).tolist() for _ in range(4)]
        lists = [wild, down, back, swap] + rand
        for k in range(0, len(lists), 2):
            check(Kc, Vc, [lists[k], lists[k + 1]], [Sq, Sq - (k % 3)], [Sq + 50 + k, CAP - k], bt, f"page {page} fp8 {fp8} Sq {Sq} lists {k}")


# ---- 3. pages ----
@pytest.mark.parametrize("fp8", [False, True])
def test_two_sequences_in_reversed_pool_order_share_no_page(fp8):
    d, page, Sq = 64, 16, 33
    n = CAP // page
    P = B * n + 2
    bt = torch.stack([torch.arange(P - 1, P - 1 - n, -1), torch.arange(n - 1, -1, -1)]).to(i32)      # descending page numbers
    Kc, Vc = random_cache((P, HKV, page, d), fp8, 400), random_cache((P, HKV, page, d), fp8, 401)
    idx = [sp.tree_path(sp.binary(Sq), Sq - 1)[0], pad(range(1, Sq, 2), Sq)]
    lens = [16 * 5 + 3 + Sq, 16 * 9 - 1 + Sq]                  # base = 83, 143: the draft lies in three and four pages
    (K, V), _ = check(Kc, Vc, idx, [6, 16], lens, bt, "reversed tables")
    touched = torch.zeros(P, dtype=torch.bool)
    for b, L in enumerate(lens):
        for p in range(L - Sq, L):
            touched[bt[b, p // page]] = True
    assert torch.equal(K[~touched], Kc[~touched]) and torch.equal(V[~touched], Vc[~touched]) and not torch.equal(K, Kc)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("side", ["source", "destination"])
def test_bad_table_entries_skip_the_move(side, fp8):
    d, page, Sq = 128, 16, 33
    bt, Kc, Vc = caches(page, d, fp8, 500)
    P = Kc.shape[0]
    lens = [16 * 4 + 5 + Sq, 16 * 7 + Sq]                       # base = 69 (pages 4, 5, 6), 112 (pages 7, 8, 9)
    idx = [pad(range(1, Sq, 2), Sq), pad([0, 2, 20, 21, 30, 32], Sq)]
    nacc = [16, 6]
    # sequence 0: destinations base .. base + 15 lie in pages 4, 5; sources base + 1 .. base + 31 in pages 4, 5, 6
    for b, pg, bad in ((0, 6 if side == "source" else 4, -1), (1, 9 if side == "source" else 7, P), (0, 5, 2 ** 31 - 1), (1, 8, -2 ** 31)):
        t = bt.clone()
        t[b, pg] = bad
        (K, V), _ = check(Kc, Vc, idx, nacc, lens, t, f"{side} page {pg} of sequence {b} = {bad}")
        assert torch.equal(K[bt[b, pg]], Kc[bt[b, pg]]) and torch.equal(V[bt[b, pg]], Vc[bt[b, pg]])      # never clamped into another page
    # the entries of pages the draft does not touch are not read: any int32 there
    t = torch.full_like(bt, 2 ** 31 - 1)
    for b, pages in ((0, (4, 5, 6)), (1, (7, 8, 9))):
        for pg in pages:
            t[b, pg] = bt[b, pg]
    good = run(Kc, Vc, idx, nacc, lens, bt)
    junk = run(Kc, Vc, idx, nacc, lens, t)
    assert torch.equal(good[0], junk[0]) and torch.equal(good[1], junk[1])


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_strided_pools(d, fp8):
    """pools kept as [P, page, Hkv, d] with padded rows: the call takes the transposed view"""
    page, Sq = 16, 16
    n = CAP // page
    bt = random_table(B, n, 600, 2)
    P = B * n + 2
    rawK, rawV = random_cache((P, page, HKV, d + 16), fp8, 601), random_cache((P, page, HKV, d + 32), fp8, 602)
    Kd, Vd = dev(rawK), dev(rawV)
    idx, nacc, lens = [sp.tree_path(sp.binary(Sq), Sq - 1)[0], pad(range(1, Sq), Sq)], [5, Sq - 1], [Sq + 40, Sq + 200 - 7]
    call.accept(Kd[..., :d].transpose(1, 2), Vd[..., :d].transpose(1, 2), torch.tensor(idx, dtype=i32).to(DEV), torch.tensor(nacc, dtype=i32).to(DEV),
                lens_tensor(lens), dev(bt))
    torch.cuda.synchronize()
    view = lambda raw: raw[..., :d].transpose(1, 2).contiguous()
    K, V = sp.accept(view(rawK), view(rawV), lens, idx, nacc, Sq, bt)
    wantK, wantV = rawK.clone(), rawV.clone()
    wantK[..., :d], wantV[..., :d] = K.transpose(1, 2), V.transpose(1, 2)
    assert torch.equal(Kd.cpu(), wantK) and torch.equal(Vd.cpu(), wantV) and not torch.equal(wantK, rawK)      # the padding as it was


# ---- 4. a copy of bits ----
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 128])
def test_nan_codes_move_as_bytes_and_stay_as_bytes(page, fp8):
    d, Sq = 64, 5
    bt, Kc, Vc = caches(page, d, fp8, 700)
    lens = [100, 259]
    flat = lambda c, b, p: (c[b, :, p] if bt is None else c[int(bt[b, p // page]), :, p % page])
    for c in (Kc, Vc):
        for b, L in enumerate(lens):
            base = L - Sq
            for p, byte in ((base + 1, 0x7F), (base + 3, 0xFF), (base + 4, 0x7F), (base - 1, 0xFF), (base + Sq, 0x7F)):
                flat(c, b, p).view(u8)[...] = byte              # rows that move (1, 3), a row that does not (4), rows outside the draft
    (K, V), _ = check(Kc, Vc, [[1, 3, 4, 4, 4]] * B, [2, 2], lens, bt, "NaN rows")
    for got, was in ((K, Kc), (V, Vc)):
        for b, L in enumerate(lens):
            base = L - Sq
            assert bool((flat(got, b, base).view(u8) == 0x7F).all()) and bool((flat(got, b, base + 1).view(u8) == 0xFF).all())
            for p in (base + 3, base + 4, base - 1, base + Sq):
                assert torch.equal(flat(got, b, p), flat(was, b, p))


# ---- 5. the binding ----
def test_the_fronts_make_the_same_calls():
    d, Sq, page = 64, 7, 16
    parents = torch.tensor([sp.binary(Sq), sp.random_tree(Sq, 800)], device=DEV)
    idx, nacc = fa.tree_path(parents, torch.tensor([Sq - 1, 3], device=DEV))
    assert idx.is_cuda and idx.dtype == i32 and nacc.dtype == i32
    assert [idx[b].tolist() for b in range(B)] == [sp.tree_path(parents[b].tolist(), leaf)[0] for b, leaf in enumerate((Sq - 1, 3))]
    lens = [50, CAP]
    _, Kc, Vc = caches(None, d, True, 801)
    Kd, Vd = dev(Kc), dev(Vc)
    assert fa.kv_cache_accept(kc.as_cache(Kd), kc.as_cache(Vd), idx, nacc, lens_tensor(lens)) is None
    torch.cuda.synchronize()
    want = sp.accept(Kc, Vc, lens, idx.tolist(), nacc.tolist(), Sq)
    assert torch.equal(Kd.cpu(), want[0]) and torch.equal(Vd.cpu(), want[1]) and not torch.equal(want[0], Kc)
    bt, Kp, Vp = caches(page, d, False, 802)
    Kd, Vd = dev(Kp), dev(Vp)
    assert fa.kv_cache_accept_paged(kc.as_cache(Kd), kc.as_cache(Vd), dev(bt), idx, nacc, lens_tensor(lens)) is None
    torch.cuda.synchronize()
    want = sp.accept(Kp, Vp, lens, idx.tolist(), nacc.tolist(), Sq, bt)
    assert torch.equal(Kd.cpu(), want[0]) and torch.equal(Vd.cpu(), want[1]) and not torch.equal(want[0], Kp)
