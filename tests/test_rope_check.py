"""CPU tests of the reference of the fused rotary embedding + cache append (tests/rope_check.py): its fp32 fma against exact rational
arithmetic, the whole rotation against float64, its position rules, and -- the yardstick's own test -- nine wrong implementations,
each refused by the check the GPU tests use (rope_check.assert_same) on a named tensor."""
import math
import random
from fractions import Fraction

import pytest

torch = pytest.importorskip("torch")

import kv_append_check as kc  # noqa: E402
import rope_check as rc  # noqa: E402

bf16 = torch.bfloat16


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def round_f32(q):
    """a Fraction rounded to fp32, nearest even (normal range: the test keeps away from fp32's subnormals and overflow)"""
    if q == 0:
        return 0.0
    sign, a = (-1, -q) if q < 0 else (1, q)
    e = math.floor(math.log2(a)) if a.numerator.bit_length() < 900 else 0
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    m = a / Fraction(2) ** (e - 23)              # in [2^23, 2^24)
    n = m.numerator // m.denominator
    r = m - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return sign * float(Fraction(n) * Fraction(2) ** (e - 23))


def test_the_fma_is_the_exactly_rounded_one():
    rnd = random.Random(5)
    a, b, c = [], [], []
    for n in range(6000):
        x1, x2 = f32(rnd.gauss(0, 1)), f32(rnd.gauss(0, 1))
        co, si = f32(rnd.uniform(-1, 1)), f32(rnd.uniform(-1, 1))
        kind = n % 4
        if kind == 0:                            # built to cancel: x1 c ~ x2 s, the addend being the ROUNDED product x2 s
            si = f32(x1 * co / x2) if x2 else si
            a.append(x1), b.append(co), c.append(-f32(float(Fraction(x2) * Fraction(si))))
        elif kind == 1:                          # a tie-like sum: the addend far below the product's last bit
            a.append(x1), b.append(co), c.append(f32(x1 * co * 2.0 ** -30) or f32(2.0 ** -60))
        elif kind == 2:
            a.append(x1), b.append(co), c.append(f32(x2 * si))
        else:                                    # bf16 operands, as the kernel sees them
            xb = float(torch.tensor(x1).to(bf16).float())
            a.append(xb), b.append(co), c.append(-f32(float(torch.tensor(x2).to(bf16).float()) * si))
    # built to fool a float64 sum that is rounded twice: c = m 2^-23 with m odd, the product +-(2^-24 - 2^-70) -- a hair on the near
    # side of the tie between c and its neighbour; float64 rounds the sum ONTO the tie and the second rounding goes to the even side
    for n in range(200):
        m, sign, e1, e2 = rnd.randrange(1 << 23, 1 << 24) | 1, rnd.choice((-1.0, 1.0)), rnd.randrange(-20, 20), rnd.randrange(-20, 20)
        a.append(sign * 2.0 ** (-12 + e1) * (1 + 2.0 ** -23)), b.append(2.0 ** (-12 + e2) * (1 - 2.0 ** -23))
        c.append(rnd.choice((-1.0, 1.0)) * m * 2.0 ** (-23 + e1 + e2))
    A, B, C = (torch.tensor(v, dtype=torch.float32) for v in (a, b, c))
    assert A.double().tolist() == a and B.double().tolist() == b and C.double().tolist() == c     # all exact fp32
    got = rc.fmaf(A, B, C)
    worst = 0
    for n in range(len(a)):
        want = round_f32(Fraction(float(A[n])) * Fraction(float(B[n])) + Fraction(float(C[n])))
        assert float(got[n]) == want, (n, float(A[n]), float(B[n]), float(C[n]), float(got[n]), want)
        worst += float(got[n]) != f32(float(A[n]) * float(B[n]) + float(C[n]))
    assert worst >= 100       # the built cases are not idle: a float64 sum rounded twice is wrong on them (half of them, by the signs)
    # mul: the exact product rounded once
    M = rc.mul(A, B)
    for n in range(0, len(a), 7):
        assert float(M[n]) == round_f32(Fraction(float(A[n])) * Fraction(float(B[n]))), n


def case(B=2, H=4, Hkv=2, Sq=5, d=64, rot=32, cap=48, seed=0, fp8=False):
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(B, H, Sq, d, generator=g).to(bf16)
    Kn = torch.randn(B, Hkv, Sq, d, generator=g).to(bf16)
    Vn = torch.randn(B, Hkv, Sq, d, generator=g).to(bf16)
    cache = lambda: torch.full((B, Hkv, cap, d), 0x11 if fp8 else 0x1111, dtype=torch.uint8 if fp8 else torch.int16)
    import __graft_entry__ as entry
    table = entry.load_package().rope_table(cap, rot)
    return Q, Kn, Vn, cache(), cache(), table


@pytest.mark.parametrize("interleaved", [False, True])
def test_the_rotation_is_the_float64_one_to_half_a_bf16_ulp(interleaved):
    Q, Kn, Vn, Kc, Vc, table = case(rot=32)
    lens = [7, 48]
    Qo, K, V, Krot = rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, interleaved)
    pos = torch.tensor([rc.q_positions(L, 5, 48) for L in lens])
    cs = table.double()[pos]
    c, s = cs[:, None, :, :16], cs[:, None, :, 16:]
    for x, got in ((Q, Qo), (Kn, Krot)):
        xd = x.double()
        x1, x2 = (xd[..., 0:32:2], xd[..., 1:32:2]) if interleaved else (xd[..., :16], xd[..., 16:32])
        want = xd.clone()
        if interleaved:
            want[..., 0:32:2], want[..., 1:32:2] = x1 * c - x2 * s, x2 * c + x1 * s
        else:
            want[..., :16], want[..., 16:32] = x1 * c - x2 * s, x2 * c + x1 * s
        # one rounding to bf16 of a value that carries two fp32 roundings: half a bf16 ulp of the result (2^-9 relative, the ulp
        # of the binade above at a power of two) plus 2^-23 of the two products' magnitudes
        mag = x1.abs() * c.abs() + x2.abs() * s.abs()
        slack = torch.zeros_like(want)
        slack[..., :32] = (torch.cat([mag, mag], -1) if not interleaved else torch.stack([mag, mag], -1).flatten(-2)) * 2.0 ** -23
        ulp = 2.0 ** (torch.floor(torch.log2(want.abs().clamp(min=1e-30))) - 7)
        assert bool(((got.double() - want).abs() <= 0.5 * ulp * (1 + 2.0 ** -7) + slack).all())
        assert torch.equal(got[..., 32:].view(torch.int16), x[..., 32:].view(torch.int16))       # a bit copy
    # the caches are kv_append's of the rotated K and of V itself
    assert torch.equal(K, kc.append(Krot, Kc, lens)) and torch.equal(V, kc.append(Vn, Vc, lens))


def test_the_position_rules():
    cap = 32
    for L in range(-2, 41):
        for Sq in range(1, 7):
            pq = rc.q_positions(L, Sq, cap)
            lq = min(max(L, 1), cap)
            assert pq == [max(lq - Sq + i, 0) for i in range(Sq)] and len(pq) == Sq and all(0 <= p < cap for p in pq)
            for i, p in kc.positions(L, Sq, cap):
                assert pq[i] == p                # where K is written, Q is rotated
    assert rc.q_positions(0, 3, 8) == [0, 0, 0] and rc.q_positions(-5, 2, 8) == [0, 0] and rc.q_positions(2, 4, 8) == [0, 0, 0, 1]
    assert rc.q_positions(100, 3, 8) == [5, 6, 7]


def test_the_probe_table_names_position_and_partner():
    x = (torch.arange(1, 1 + 2 * 3 * 8 * 32).reshape(2, 3, 8, 32) % 251 + 1).to(bf16)
    pos = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7], [3, 3, 2, 2, 1, 1, 0, 0]])
    for rot in (16, 32):
        for il in (False, True):
            assert torch.equal(rc.rotate(x, rc.probe_table(8, rot), pos, il).view(torch.int16), rc.probe_expect(x, pos, rot, il).view(torch.int16))


def ragged_case(fp8):
    g = torch.Generator().manual_seed(3)
    cu, T, H, Hkv, d, cap = [0, 3, 3, 9], 11, 4, 2, 64, 32
    Q = torch.randn(T, H, d, generator=g).to(bf16)
    Kn, Vn = torch.randn(T, Hkv, d, generator=g).to(bf16), torch.randn(T, Hkv, d, generator=g).to(bf16)
    cache = lambda: torch.full((3, Hkv, cap, d), 0x11 if fp8 else 0x1111, dtype=torch.uint8 if fp8 else torch.int16)
    return Q, Kn, Vn, torch.full_like(Q, 7.0), cache(), cache(), cu


def test_the_ragged_writer_is_the_uniform_one_per_sequence():
    Q, Kn, Vn, Q0, Kc, Vc, cu = ragged_case(False)
    table = rc.probe_table(32, 32)
    lens = [10, 5, 4]
    Qo, K, V = rc.rope_append_varlen(Q, Kn, Vn, Q0, Kc, Vc, table, cu, lens, False)
    assert torch.equal(Qo[9:], Q0[9:])                                    # tokens nobody owns
    q, k, v, _ = rc.rope_append(Q[3:9].transpose(0, 1)[None], Kn[3:9].transpose(0, 1)[None], Vn[3:9].transpose(0, 1)[None], Kc[2:3], Vc[2:3],
                                table, [4], False)
    assert torch.equal(Qo[3:9], q[0].transpose(0, 1)) and torch.equal(K[2:3], k) and torch.equal(V[2:3], v)
    assert torch.equal(K[1], Kc[1]) and torch.equal(V[1], Vc[1])          # a sequence without rows
    assert not torch.equal(K[0], Kc[0])


# ---- mutants: what a wrong kernel would write, held against the reference by the GPU tests' own check ----
NAMES = ("Qout", "Kcache", "Vcache")


def mutants(fp8):
    """({what is wrong: (the tensor's name, what the wrong kernel leaves in it, what the reference does)}, the reference's three)"""
    Q, Kn, Vn, Kc, Vc, table = case(B=1, H=2, Hkv=1, Sq=5, d=64, rot=32, cap=48, fp8=fp8)
    lens = [3]                                    # fewer keys than rows: rows 0, 1 have no K; Q rows 0 .. 2 sit at position 0
    ds = torch.tensor([0.37]) if fp8 else None
    want = rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, False, ds, ds)[:3]
    pos = torch.tensor([rc.q_positions(3, 5, 48)])
    out = {}
    out["the other pair style"] = ("Qout", rc.rope_append(Q, Kn, Vn, Kc, Vc, table, lens, True, ds, ds)[:3])
    neg = table.clone()
    neg[:, 16:] *= -1
    out["sin negated"] = ("Kcache", rc.rope_append(Q, Kn, Vn, Kc, Vc, neg, lens, False, ds, ds)[:3])
    out["position p + 1"] = ("Kcache", rc.rope_append(Q, Kn, Vn, Kc, Vc, torch.roll(table, -1, 0), lens, False, ds, ds)[:3])
    out["position p - 1"] = ("Qout", rc.rope_append(Q, Kn, Vn, Kc, Vc, torch.roll(table, 1, 0), lens, False, ds, ds)[:3])
    # the row index i instead of the position p: with first = L - Sq = -2, p = i - 2
    out["row index for position"] = ("Kcache", (rc.rotate(Q, table, torch.arange(5)[None], False),
                                                kc.append(rc.rotate(Kn, table, torch.arange(5)[None], False), Kc, lens, ds), want[2]))
    out["V rotated"] = ("Vcache", (want[0], want[1], kc.append(rc.rotate(Vn, table, pos, False), Vc, lens, ds)))
    wide = torch.cat([table[:, :16], table[:, :16], table[:, 16:], table[:, 16:]], 1)      # rot = d: the tail columns turn too
    out["columns >= rotDim rotated"] = ("Qout", rc.rope_append(Q, Kn, Vn, Kc, Vc, wide, lens, False, ds, ds)[:3])
    # Q at K's unclamped position L - Sq + i for L < Sq (read as an index from the table's end)
    out["Q at the unclamped position"] = ("Qout", (rc.rotate(Q, table, torch.tensor([[46, 47, 0, 1, 2]]), False), want[1], want[2]))
    out = {what: (where, got[NAMES.index(where)], want[NAMES.index(where)]) for what, (where, got) in out.items()}
    if fp8:
        # two roundings differ from one only where the bf16 value lands on a tie of e4m3fn: a case with enough rows to meet some
        Q, Kn, Vn, Kc, Vc, table = case(B=1, H=2, Hkv=2, Sq=40, d=64, rot=64, cap=48, fp8=True)
        pos = torch.tensor([rc.q_positions(48, 40, 48)])
        y1, y2 = rc.rotate_f32(Kn, table, pos, False)
        k8 = Kc.clone()
        enc = (torch.cat([y1, y2], -1) / 0.37).clamp(-448, 448).to(kc.F8).view(torch.uint8)
        for i, p in kc.positions(48, 40, 48):
            k8[0, :, p] = enc[0, :, i]
        out["bf16 rounding skipped before fp8"] = ("Kcache", k8, rc.rope_append(Q, Kn, Vn, Kc, Vc, table, [48], False, ds, ds)[1])
    return out, want


@pytest.mark.parametrize("fp8", [False, True])
def test_every_mutant_is_refused_on_a_named_tensor(fp8):
    out, want = mutants(fp8)
    assert len(out) == 8 + fp8
    for name, w in zip(NAMES, want):              # the reference passes its own check
        rc.assert_same(name, w, w.clone())
    for what, (where, got, ref) in out.items():
        with pytest.raises(AssertionError, match=where + r"\[\d+, \d+, \d+, \d+\]"):
            rc.assert_same(where, got, ref)


def test_the_check_compares_nan_by_class_and_everything_else_by_bits():
    a = torch.tensor([0x7FC0, 0x0000, 0x3F80], dtype=torch.int16)
    rc.assert_same("x", a, torch.tensor([0x7FC1, 0x0000, 0x3F80], dtype=torch.int16))            # two NaN patterns
    with pytest.raises(AssertionError, match=r"x\[1\]"):
        rc.assert_same("x", a, torch.tensor([0x7FC0, -0x8000, 0x3F80], dtype=torch.int16))       # +0 against -0
    with pytest.raises(AssertionError, match=r"x\[0\]"):
        rc.assert_same("x", a, torch.tensor([0x7F80, 0x0000, 0x3F80], dtype=torch.int16))        # NaN against inf
    b = torch.tensor([0x7F, 0x80], dtype=torch.uint8)
    rc.assert_same("y", b, torch.tensor([0xFF, 0x80], dtype=torch.uint8))
    with pytest.raises(AssertionError, match=r"y\[1\]"):
        rc.assert_same("y", b, torch.tensor([0x7F, 0x00], dtype=torch.uint8))
