"""Reference shared by the tests of the fused rotary embedding + K/V cache append (flash_attention_rope_append*; tests/test_rope_check.py
and tests/test_rope_append_abi.py on the CPU, tests/test_rope_append*.py and tests/test_rope_memory_contract.py on the GPU; no tests in
here).  Plain torch on the CPU, BIT EXACT: the contract of include/flash_attention.h spelled out.

Values.  `fmaf()` is the fp32 fused multiply-add through float64: the product of two fp32 is exact in float64 (48 bits); the sum with
the addend is rounded to ODD in float64 (TwoSum gives the rounding error of the float64 sum; where it is not zero and the sum's last
bit is even, the sum moves one ulp towards the error), and a round-to-odd value of 53 >= 24 + 2 bits rounds to fp32 as the exact
value would.  tests/test_rope_check.py holds it against exact rational arithmetic.  `mul()` is the fp32 product (exact in float64,
rounded once).  `rotate()` is y1 = fmaf(x1, c, -(x2 s)), y2 = fmaf(x2, c, x1 s), rounded once to bf16 (nearest even); the columns
>= rotDim are a bit copy.  The cache bytes are then `kv_append_check.encode`'s.

Positions.  `q_positions()` is the header's rule for Q, `kv_append_check.positions()` the twin's for K and V; a K row is rotated at
the position it is written to.  Writers: `rope_append()` (contiguous or paged, on `kv_append_check.append`) and `rope_append_varlen()`
(every sequence through `rope_append` alone).  `assert_same()` is the check the GPU tests use: integers, NaN by class, the first
differing element named.
"""
import torch

import kv_append_check as kc
from kv_cache_check import random_table

i16, u8, bf16 = torch.int16, torch.uint8, torch.bfloat16


def mul(a, b):
    """fp32 a * b, rounded once (fp32 tensors)"""
    return (a.double() * b.double()).float()


def fmaf(a, b, c):
    """fp32 fma(a, b, c) with ONE rounding (fp32 tensors, broadcast)"""
    a, b, c = torch.broadcast_tensors(a.double(), b.double(), c.double())
    p = a * b                                   # exact
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)             # TwoSum: p + c = s + err exactly
    fix = torch.isfinite(s) & torch.isfinite(err) & (err != 0)
    bits = s.contiguous().view(torch.int64).clone()
    even = (bits & 1) == 0
    up = (err > 0) == (s > 0)                   # towards the error = away from zero
    bits = torch.where(fix & even, bits + torch.where(up, 1, -1), bits)
    return bits.view(torch.float64).float()


def rotate_f32(x, table, pos, interleaved):
    """the rotated columns before the rounding to bf16: x bf16 [B, heads, R, d], pos int64 [B, R], table fp32 [max_pos, rot] ->
    (y1, y2) fp32 [B, heads, R, rot / 2]: the first and second members of the pairs, pair j at index j"""
    rot = table.shape[1]
    half = rot // 2
    assert x.dtype == bf16 and table.dtype == torch.float32 and int(pos.min()) >= 0 and int(pos.max()) < table.shape[0]
    xf = x.float()
    cs = table[pos]                              # [B, R, rot]
    c, s = cs[:, None, :, :half], cs[:, None, :, half:]
    x1, x2 = (xf[..., 0:rot:2], xf[..., 1:rot:2]) if interleaved else (xf[..., :half], xf[..., half:rot])
    return fmaf(x1, c, -mul(x2, s)), fmaf(x2, c, mul(x1, s))


def rotate(x, table, pos, interleaved):
    """x rotated at `pos`, bf16: one rounding to nearest even; the columns >= rot are x's bits"""
    rot = table.shape[1]
    y1, y2 = rotate_f32(x, table, pos, interleaved)
    out = x.clone()
    if interleaved:
        out[..., 0:rot:2], out[..., 1:rot:2] = y1.to(bf16), y2.to(bf16)
    else:
        out[..., :rot // 2], out[..., rot // 2:rot] = y1.to(bf16), y2.to(bf16)
    return out


def q_positions(L, Sq, cap):
    """[pq]: Q row i of a sequence whose length (the new rows counted) is L is rotated at pq[i]; every row is written"""
    lq = min(max(int(L), 1), cap)
    return [max(lq - Sq + i, 0) for i in range(Sq)]


def rope_append(Q, Kn, Vn, Kc, Vc, table, lens, interleaved, kds=None, vds=None, block_table=None):
    """-> (Qout bf16, K cache, V cache, Krot bf16): Q bf16 [B, H, Sq, d], Kn / Vn bf16 [B, Hkv, Sq, d]; the caches as
    kv_append_check.append takes them (int16 / uint8; with block_table pools).  Krot: the bf16 rotation of Kn (rows that are not
    written rotated at their Q position)"""
    B, _, Sq, _ = Kn.shape
    cap = Kc.shape[2] * (block_table.shape[1] if block_table is not None else 1)
    assert table.shape[0] >= cap
    pos = torch.tensor([q_positions(cap if lens is None else lens[b], Sq, cap) for b in range(B)], dtype=torch.int64)
    for b in range(B):                               # a K row that is written is rotated where it is written
        for i, p in kc.positions(cap if lens is None else lens[b], Sq, cap):
            assert int(pos[b, i]) == p
    Krot = rotate(Kn, table, pos, interleaved)
    return (rotate(Q, table, pos, interleaved), kc.append(Krot, Kc, lens, kds, block_table), kc.append(Vn, Vc, lens, vds, block_table),
            Krot)


def rope_append_varlen(Q, Kn, Vn, Qout, Kc, Vc, table, cu, lens, interleaved, kds=None, vds=None, block_table=None):
    """the ragged call: Q [T, H, d], Kn / Vn [T, Hkv, d] packed by token, cu the B + 1 offsets (clamped as the kernel clamps them);
    Qout: what the output held before (tokens nobody owns keep it).  -> (Qout, K cache, V cache)"""
    T = Q.shape[0]
    Qout, Kc, Vc = Qout.clone(), Kc.clone(), Vc.clone()
    B = len(cu) - 1
    for b in range(B):                               # (cu ascending: the kernel's owner of a token is this loop's)
        q0 = min(max(int(cu[b]), 0), T)
        q1 = min(max(int(cu[b + 1]), q0), T)
        if q1 <= q0:
            continue
        view = lambda x: x[q0:q1].transpose(0, 1).unsqueeze(0)
        L = None if lens is None else [lens[b]]
        if block_table is None:
            qo, k, v, _ = rope_append(view(Q), view(Kn), view(Vn), Kc[b:b + 1], Vc[b:b + 1], table, L, interleaved, kds, vds)
            Kc[b:b + 1], Vc[b:b + 1] = k, v
        else:
            qo, Kc, Vc, _ = rope_append(view(Q), view(Kn), view(Vn), Kc, Vc, table, L, interleaved, kds, vds, block_table[b:b + 1])
        Qout[q0:q1] = qo[0].transpose(0, 1)
    return Qout, Kc, Vc


def bits(x):
    """a tensor as integers: bf16 -> int16, float8 -> uint8, integers as they are"""
    x = x.detach().cpu()
    if x.dtype == bf16:
        return x.contiguous().view(i16)
    if kc.F8 is not None and x.dtype == kc.F8:
        return x.contiguous().view(u8)
    assert x.dtype in (i16, u8), x.dtype
    return x


def assert_same(name, got, want):
    """`got` equals `want` bit for bit, NaN codes compared by class (bf16 patterns or e4m3fn bytes); names the first element that
    differs"""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype == u8:
        gn, wn = (g & 0x7F) == 0x7F, (w & 0x7F) == 0x7F
    else:
        gn, wn = (g & 0x7FFF) > 0x7F80, (w & 0x7FFF) > 0x7F80
    bad = (gn != wn) | (~wn & (g != w))
    if bool(bad.any()):
        at = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{name}{list(at)}: got {int(g[at]) & 0xFFFF:#06x}, want {int(w[at]) & 0xFFFF:#06x} "
                             f"({int(bad.sum())} of {bad.numel()} elements differ)")


def probe_table(max_pos, rot):
    """the exact probe table: row p is (c, s) = (1, 0), (0, 1), (-1, 0), (0, -1) by p mod 4, for every angle"""
    c = torch.tensor([1.0, 0.0, -1.0, 0.0])[torch.arange(max_pos) % 4]
    s = torch.tensor([0.0, 1.0, 0.0, -1.0])[torch.arange(max_pos) % 4]
    return torch.cat([c[:, None].expand(max_pos, rot // 2), s[:, None].expand(max_pos, rot // 2)], dim=1).contiguous()


def probe_expect(x, pos, rot, interleaved):
    """what the probe table makes of x (bf16 [B, heads, R, d], NO zeros, NaN or infinities in it): every output element is +- one
    named input element -- by p mod 4: (x1, x2), (-x2, x1), (-x1, -x2), (x2, -x1) -- written without any arithmetic but the sign"""
    out = x.clone()
    half = rot // 2
    a, b = (slice(0, rot, 2), slice(1, rot, 2)) if interleaved else (slice(0, half), slice(half, rot))
    x1, x2 = x[..., a], x[..., b]
    m = (pos % 4)[:, None, :, None]
    out[..., a] = torch.where(m == 0, x1, torch.where(m == 1, -x2, torch.where(m == 2, -x1, x2)))
    out[..., b] = torch.where(m == 0, x2, torch.where(m == 1, x1, torch.where(m == 2, -x2, -x1)))
    return out


# ---- what the GPU tests (test_rope_append.py, test_rope_append_varlen.py) build and check alike -------------------------------------------
QSENT = 0x4B4B                        # what Qout holds before a call: finite in bf16


def qsent(shape, device="cpu"):
    return torch.full(shape, QSENT, dtype=i16, device=device).view(bf16)


def rows(shape, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 3).to(bf16)
    if special:       # NaN payloads, infinities, -0, tiny and huge values among them
        flat = x.reshape(-1)
        s = torch.tensor([0x7FC1, -0x0040 + 0x0001, 0x7F80, -0x0080, -0x8000, 0x0000, 0x0001, -0x7FFF, 0x43E0, 0x7F7F],
                         dtype=torch.int32).to(i16).view(bf16)
        flat[:s.numel()] = s
        flat[-s.numel():] = s.flip(0)
    return x


def table_of(B, n, spare, seed):
    """(P, block table [B, n]): a seeded permutation of the P = B * n + spare pages"""
    return B * n + spare, random_table(B, n, seed, spare)


def check(got, want, what):
    for name, g, w in zip(("Qout", "Kcache", "Vcache"), got, want):
        assert_same(f"{what}: {name}", g, w)
