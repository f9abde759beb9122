"""A wave's last tile in the optimistic passes of the causal mixed-precision kernels (csrc/kernel_bf16.hip.h: KernelCfg::TAIL;
csrc/slot_engine.hip.h: SlotEngine::tail_step): a step of phase B alone -- no look-ahead QK^T -- which, for the wave whose 32 rows start
on a 64-row boundary, also skips the keys 32 .. 63 of its diagonal tile, masked in every row (TAIL_HALF).

Shapes: the smallest that take the route under test, asserted through plan_ex.  The persistent kernels get heads enough for three units
per workgroup (units >= 3 * grid), so every workgroup has unit seams; S = 1281 gives units with an odd and units with an even number of
tiles, so a wave's last tile falls on either score buffer.  Every shape is compared with the float64 reference
(tests/forward_routes.py: head_reference) on sampled heads, all rows, at the library's stated tolerance 1e-3 + 1e-3 |ref| (tests/parity.py;
fp32 O, default precision, N(0,1) inputs with a fixed seed).

What two runs of the library must agree on is compared bit for bit:

  * HALF: O and the LSE of every 32-row slab of the bf16-weights blocks (qb >= hp) against the same call with FA_FLAG_BF16_WEIGHTS, which
    runs the plain bf16 kernel -- the same arithmetic, every tile through tile_step, no tail step.  THAT is the comparison that pins the
    skipped half.  The slabs of the fp16-weights blocks (qb < hp) are compared with the FA_FLAG_F16_WEIGHTS call; that call runs the
    mixed-precision kernel with hp = all blocks, tail step included, so for them the comparison pins only that a block's result does not
    depend on hp.  Their tail steps are covered by the float64 comparison and by the next test.
  * nothing past the diagonal reaches O: finite garbage (+-1e4) in K and V on every key k > q leaves the rows <= q as the clean call
    gave them, for q the last row of an even and of an odd slab of the first, a middle and the last block.  The garbage call asks for
    the rows <= q only (seqLenQ = q + 1 against the full K and V), and q ends a slab so that q's wave has no row behind q: a row that
    sees a key of 1e4 overflows its optimistic pass, its whole unit is repeated by the tracked pass, and that pass moves the
    reference max of every row of a wave together -- other bits for row q in the parent commit's kernels as well, for a reason that
    has nothing to do with what lies past q's diagonal.  In the even slab the 32 keys behind q are the half the tail step skips.

Non-finite V on masked keys is out of scope: 0 * inf is NaN in tile_step and is never formed in the skipped half.
"""
from collections import namedtuple

import numpy as np
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import forward_routes as fr  # noqa: E402
from parity import STATED_ATOL, STATED_RTOL  # noqa: E402

DEV = "cuda:0"
bf, f32 = torch.bfloat16, torch.float32
TILE, SLAB = 64, 32

Shape = namedtuple("Shape", "name B H Hkv Sq Sk d family layout", defaults=("dense",))
C128 = Shape("mix_d128", 8, 16, 16, 1536, 1536, 128, "causal_mix")
SHAPES = [
    C128,
    Shape("mix_d128_ragged", 8, 16, 16, 1281, 1281, 128, "causal_mix"),
    Shape("mix_d64_gqa", 8, 16, 4, 1536, 1536, 64, "causal_mix"),
    Shape("mix_d64_strided", 8, 16, 16, 1281, 1281, 64, "causal_mix", "model"),
    Shape("pair_d128", 1, 4, 4, 600, 600, 128, "pair"),
    Shape("pair_d64", 1, 8, 8, 512, 512, 64, "pair"),
]
# seqLenK ends inside tile 16 (keys 1024 .. 1087), which is the last tile of the wave whose rows start at 1088 = 17 * 64
CROSS = Shape("mix_d128_cross", 8, 16, 16, 1536, 1084, 128, "causal_mix")


def assert_route(s, flags=0, family=None):
    """(rows of a query block, hp) of the call; persistent routes: at least three units per workgroup"""
    assert fr.family(s.B, s.H, s.Sq, s.Sk, s.d, True, fa.FA_DTYPE_BF16, fa.FA_DTYPE_F32, flags) == (family or s.family)
    rows, hp = fr.blocks(s.B, s.H, s.Sq, s.Sk, s.d, True, flags=flags)
    if (family or s.family) != "pair":
        units, grid = fr.walks(s.B, s.H, s.Sq, s.Sk, s.d, True, flags=flags)
        assert rows == 256 and units >= 3 * grid, f"{s.name}: {units} units on {grid} workgroups"
    else:
        assert rows == 128
    return rows, hp


_cache = {}


def inputs(s):
    """(Q, K, V) on the host and on the device, one shape at a time"""
    key = s.name
    if key not in _cache:
        _cache.clear()
        seed = 4700 + 5 * s.d + s.Sq + s.Sk + s.B
        host = (fr.randn((s.B, s.H, s.Sq, s.d), seed), fr.randn((s.B, s.Hkv, s.Sk, s.d), seed + 1), fr.randn((s.B, s.Hkv, s.Sk, s.d), seed + 2))
        _cache[key] = (host, tuple(to_device(s, t) for t in host))
    return _cache[key]


def to_device(s, t):
    if s.layout == "dense":
        return t.to(DEV)
    B, heads, S, d = t.shape
    v = torch.empty(B, S, heads * d, dtype=t.dtype, device=DEV).view(B, S, heads, d).transpose(1, 2)   # (B, S, H * d) storage
    v.copy_(t.to(DEV))
    return v


def run(s, Qd, Kd, Vd, **kw):
    O = None
    if s.layout == "model":
        O = torch.full((s.B, s.Sq, s.H * s.d), float("nan"), dtype=f32, device=DEV).view(s.B, s.Sq, s.H, s.d).transpose(1, 2)
    out = fa.flash_attention(Qd, Kd, Vd, O, is_causal=True, out_dtype=f32, **kw)
    torch.cuda.synchronize()
    return out


def ratio(got, ref, atol, rtol):
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def check_against_reference(s):
    (Q, K, V), dev = inputs(s)
    O = run(s, *dev)
    assert torch.isfinite(O).all()
    n, worst = s.B * s.H, 0.0
    for g in sorted({0, n // 3, (2 * n) // 3, n - 1}):
        b, h = divmod(g, s.H)
        hk = h // (s.H // s.Hkv)
        ref, _ = fr.head_reference(Q[b, h].float(), K[b, hk].float(), V[b, hk].float(), 1 / s.d ** 0.5, True)
        q = ratio(O[b, h].cpu().numpy(), ref, STATED_ATOL, STATED_RTOL)
        worst = max(worst, q)
        assert q <= 1.0, f"{s.name}, head {g}: worst error / tolerance {q:.3f} at {STATED_ATOL:g} + {STATED_RTOL:g}|ref|"
    print(f"TAIL {s.name}: worst error / tolerance {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("s", SHAPES, ids=lambda s: s.name)
def test_against_the_oracle(s):
    rows, hp = assert_route(s)
    nQ = -(-s.Sq // rows)
    if s.family == "causal_mix":
        assert 0 < hp < nQ, "blocks of both precisions in every head"
    if s.name.endswith("ragged") or s.name.endswith("strided"):
        tiles = {min(-(-s.Sk // TILE), -(-min(s.Sq, (qb + 1) * rows) // TILE)) for qb in range(nQ)}
        assert {t & 1 for t in tiles} == {0, 1}, "units with an odd and with an even number of tiles"
    check_against_reference(s)


@pytest.mark.gpu
def test_cross_lengths_tail_is_not_the_diagonal_tile():
    s = CROSS
    rows, hp = assert_route(s)
    k_tiles = -(-s.Sk // TILE)
    q_row0 = k_tiles * TILE                      # a wave whose slab starts on a 64-row boundary ...
    assert q_row0 % TILE == 0 and q_row0 % rows != 0 and q_row0 + SLAB <= s.Sq
    my_tiles = min(k_tiles, (q_row0 + SLAB - 1) // TILE + 1)
    last = my_tiles - 1
    assert my_tiles == k_tiles                   # ... whose last tile is the one seqLenK cuts,
    assert last * TILE + 32 < s.Sk < (last + 1) * TILE   # with visible keys in its second half,
    assert not last * TILE + 32 > q_row0 + SLAB - 1      # and which is not its diagonal tile: the half step must not fire
    assert 0 < hp < -(-s.Sq // rows)
    check_against_reference(s)


@pytest.mark.gpu
def test_half_step_bit_for_bit():
    s = C128
    rows, hp = assert_route(s)
    assert_route(s, fa.FA_FLAG_BF16_WEIGHTS, "bf16")
    _, dev = inputs(s)
    O, lse = run(s, *dev, return_lse=True)
    Ob, lseb = run(s, *dev, return_lse=True, weights_dtype=bf)
    Of, lsef = run(s, *dev, return_lse=True, weights_dtype=torch.float16)
    assert torch.isfinite(O).all() and torch.isfinite(lse).all()
    split = hp * rows
    assert not torch.equal(O[:, :, :split], Ob[:, :, :split]), "the two precisions must differ somewhere, or nothing was compared"
    for r0 in range(0, s.Sq, SLAB):
        sl = slice(r0, r0 + SLAB)
        other, other_lse, what = (Ob, lseb, "bf16-weights (plain kernel, no tail step)") if r0 >= split else (Of, lsef, "fp16-weights")
        assert torch.equal(O[:, :, sl], other[:, :, sl]), f"O, rows {r0} .. {r0 + SLAB - 1}, against the {what} call"
        assert torch.equal(lse[:, :, sl], other_lse[:, :, sl]), f"LSE, rows {r0} .. {r0 + SLAB - 1}, against the {what} call"
    print(f"TAIL half: {(s.Sq - split) // SLAB} slabs against the plain bf16-weights kernel, {split // SLAB} against the fp16-weights call")


@pytest.mark.gpu
def test_nothing_past_the_diagonal_reaches_o():
    s = C128
    rows, hp = assert_route(s)
    nQ = s.Sq // rows
    _, (Qd, Kd, Vd) = inputs(s)
    O0 = run(s, Qd, Kd, Vd)
    g = torch.Generator().manual_seed(31)
    sign = (torch.randint(0, 2, Kd.shape, generator=g).float() * 2 - 1).to(DEV)
    garbage = (1e4 * sign).to(bf)
    sampled = []
    for qb in (0, hp - 1, nQ - 1):                 # first block, a middle one (the last with fp16 weights), last block
        sampled += [qb * rows + 64 + 31, qb * rows + 128 + 63]   # the last row of an even slab, the last row of an odd slab
    for q in sampled:
        assert (q % TILE < SLAB) == (q // SLAB % 2 == 0)
        K2, V2 = Kd.clone(), Vd.clone()
        K2[:, :, q + 1:] = garbage[:, :, q + 1:]
        V2[:, :, q + 1:] = garbage[:, :, q + 1:]
        # ("f16_weights": every block of the shorter call is an fp16-weights block; under the mask that is the mixed kernel with hp = all)
        assert fr.family(s.B, s.H, q + 1, s.Sk, s.d, True, fa.FA_DTYPE_BF16, fa.FA_DTYPE_F32, 0) in ("causal_mix", "f16_weights", "pair")
        O = run(s, Qd[:, :, :q + 1].contiguous(), K2, V2)
        assert torch.isfinite(O).all()
        assert torch.equal(O, O0[:, :, :q + 1]), f"rows <= {q} changed with what lies past their diagonal"
