"""The unit seam of the persistent causal kernels (csrc/kernel_bf16.hip.h: run_units), which ends a unit's K/V buffer descriptors at its
diagonal (KernelCfg::KV_CLAMP) and fetches Q with non-temporal loads (Q_CACHE).

The shapes are the smallest that still take the persistent 512-thread route (heads * ceil(S / 256) * 2 > 256 on a 256-CU device),
asserted through the plan.  Every shape is compared with the float64 reference (tests/forward_routes.py: head_reference) on four
sampled heads, all rows, at the library's stated tolerance 1e-3 + 1e-3 |ref| (tests/parity.py; fp32 O, default precision); the LSE at
rtol 2e-5, atol 2e-3 (the bound of tests/test_forward_fallbacks.py).  These are what guards a descriptor that ends too EARLY (ragged
and cross above all): a needed tile would arrive as zeros.

What two runs of the library must agree on is compared bitwise:

  * rows of K and V at and past 256 (qb + 1), overwritten with large finite values in every head, change no bit of the query blocks
    <= qb, while the last block, which sees them, changes;
  * the same inside the fallback passes: a unit that is sent through the tracked pass (a score spike) or through the bf16-weights
    last resort (|V| > 65504 in an fp16-weights block) gives the same bits whatever lies past its diagonal.

The bitwise tests pin that NOTHING PAST THE DIAGONAL REACHES O -- the property the descriptors' end relies on.  They do not pin where
the descriptors end: a kernel that fetches those tiles and drops their look-ahead scores, as the one before KV_CLAMP did, passes too.
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
QB = 256                   # query rows of a unit on this route
BF16W = (4e-3, 4e-3)       # poisoned heads: the bound of tests/test_forward_fallbacks.py

Shape = namedtuple("Shape", "name B H Hkv Sq Sk d layout walks", defaults=("dense", 0))
C128 = Shape("c128", 1, 16, 16, 2304, 2304, 128)                      # four fp16-weights and five bf16-weights blocks per head
SHAPES = [
    C128,
    Shape("ragged", 3, 11, 11, 1100, 1100, 128),                      # ragged last block and ragged last tile
    Shape("d64", 8, 8, 8, 2048, 2048, 64),
    Shape("gqa", 1, 16, 4, 2304, 2304, 128),
    Shape("strided", 1, 16, 16, 2304, 2304, 128, "model"),           # (B, S, H * d) storage
    Shape("cross", 1, 16, 16, 2304, 2000, 128),                       # seqLenK != seqLenQ, ragged last key tile: flash_attention_cross
    # (the shapes above have about one unit per workgroup at d = 128.)  Two units and more per workgroup: the next unit's descriptors,
    # tile 0 and Q are set up at the seam, under the current unit's epilogue
    Shape("walk", 4, 16, 16, 2304, 2304, 128, walks=2),
]


def assert_route(s):
    if s.Sq == s.Sk:
        assert fa.plan(s.B, s.H, s.Sq, s.d, True)["threads"] == 512
    e, m = fa.plan_ex(s.B, s.H, s.Sq, s.Sk, s.d, True)
    live = m if m["q_blocks"] else e
    assert live["threads"] == 512 and live["q_block_rows"] == QB
    if s.walks:
        assert s.B * s.H * (e["q_blocks"] + m["q_blocks"]) >= s.walks * live["grid"], f"every workgroup must walk {s.walks} units"
    return e["q_blocks"]   # hp: the leading fp16-weights blocks


_inputs = {}


def inputs(s):
    key = (s.B, s.H, s.Hkv, s.Sq, s.Sk, s.d)
    if key not in _inputs:
        _inputs.clear()
        seed = 9100 + 3 * s.d + s.Sk + s.B
        _inputs[key] = (fr.randn((s.B, s.H, s.Sq, s.d), seed), fr.randn((s.B, s.Hkv, s.Sk, s.d), seed + 1), fr.randn((s.B, s.Hkv, s.Sk, s.d), seed + 2))
    return _inputs[key]


def to_device(s, t):
    if s.layout == "dense":
        return t.to(DEV)
    B, heads, S, d = t.shape
    buf = torch.empty(B, S, heads * d, dtype=t.dtype, device=DEV)
    v = buf.view(B, S, heads, d).transpose(1, 2)
    v.copy_(t.to(DEV))
    return v


def run(s, Q, K, V, want_lse=False):
    O = None
    if s.layout == "model":
        O = torch.full((s.B, s.Sq, s.H * s.d), float("nan"), dtype=f32, device=DEV).view(s.B, s.Sq, s.H, s.d).transpose(1, 2)
    out = fa.flash_attention(to_device(s, Q), to_device(s, K), to_device(s, V), O, is_causal=True, out_dtype=f32, return_lse=want_lse)
    torch.cuda.synchronize()
    return out


def ratio(got, ref, atol, rtol):
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def reference(s, Q, K, V, g):
    """(O, LSE) in float64 of flattened query head g"""
    b, h = divmod(g, s.H)
    hk = h // (s.H // s.Hkv)
    return fr.head_reference(Q[b, h].float(), K[b, hk].float(), V[b, hk].float(), 1 / s.d ** 0.5, True)


def sampled_heads(s):
    n = s.B * s.H
    return sorted({0, n // 3, (2 * n) // 3, n - 1})


@pytest.mark.gpu
@pytest.mark.parametrize("s", SHAPES, ids=lambda s: s.name)
def test_against_the_oracle(s):
    assert_route(s)
    Q, K, V = inputs(s)
    O = run(s, Q, K, V)
    assert torch.isfinite(O).all()
    worst = 0.0
    for g in sampled_heads(s):
        ref, _ = reference(s, Q, K, V, g)
        q = ratio(O[g // s.H, g % s.H].cpu().numpy(), ref, STATED_ATOL, STATED_RTOL)
        worst = max(worst, q)
        assert q <= 1.0, f"{s.name}, head {g}: worst error / tolerance {q:.3f} at {STATED_ATOL:g} + {STATED_RTOL:g}|ref|"
    print(f"SEAM {s.name}: worst error / tolerance {worst:.3f}")


@pytest.mark.gpu
def test_lse_against_the_oracle():
    s = C128
    assert_route(s)
    Q, K, V = inputs(s)
    O, lse = run(s, Q, K, V, want_lse=True)
    assert torch.isfinite(O).all() and torch.isfinite(lse).all()
    for g in sampled_heads(s):
        ref, ref_lse = reference(s, Q, K, V, g)
        q = ratio(O[0, g].cpu().numpy(), ref, STATED_ATOL, STATED_RTOL)
        ql = ratio(lse[0, g].cpu().numpy(), ref_lse, 2e-3, 2e-5)
        print(f"SEAM lse head {g}: worst error / tolerance O {q:.3f} LSE {ql:.3f}")
        assert q <= 1.0 and ql <= 1.0


def past_diagonal(K, V, qb, seed):
    """copies of K and V with the rows >= 256 (qb + 1) of every head overwritten: K +-2 (scores of a few sigma more than N(0,1)
    data gives: a unit that sees them stays in its optimistic pass with bf16 weights), V 1000"""
    r0 = QB * (qb + 1)
    K2, V2 = K.clone(), V.clone()
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, K2[:, :, r0:].shape, generator=g).float() * 2 - 1
    K2[:, :, r0:] = (2.0 * sign).to(K.dtype)
    V2[:, :, r0:] = 1000.0
    return K2, V2


@pytest.mark.gpu
@pytest.mark.parametrize("s", [C128, SHAPES[3], SHAPES[6]], ids=lambda s: s.name)
def test_nothing_past_the_diagonal_is_seen(s):
    hp = assert_route(s)
    nQ = -(-s.Sq // QB)
    assert 0 < hp < nQ - 1
    Q, K, V = inputs(s)
    O0 = run(s, Q, K, V)
    for qb in (0, hp - 1, nQ - 2):     # the first block, the last fp16-weights block, the last block but one
        K2, V2 = past_diagonal(K, V, qb, 77 + qb)
        O = run(s, Q, K2, V2)
        rows = QB * (qb + 1)
        assert torch.equal(O[:, :, :rows], O0[:, :, :rows]), f"qb = {qb}: rows < {rows} changed with what lies past their diagonal"
        last = slice(QB * (nQ - 1), s.Sq)
        assert torch.isfinite(O).all()
        assert not torch.equal(O[:, :, last], O0[:, :, last]), "the last block sees the overwritten rows and must change"
        assert (O[:, :, last] != O0[:, :, last]).any(dim=-1).all(), "every row of the last block sees them"


# (recipe of forward_routes.poison, its (row, key)): a spike that overflows the optimistic pass of a bf16-weights unit (block 4) and of an
# fp16-weights unit (block 2), and |V| = 1e5 at a key that the fp16-weights blocks 1 .. 3 load
FALLBACKS = [("spike_over", (1100, 1030)), ("spike_over", (700, 300)), ("v_big", (700, 300))]


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,place", FALLBACKS, ids=lambda x: x if isinstance(x, str) else f"{x[0]}_{x[1]}")
def test_fallback_passes_end_at_the_diagonal(recipe, place):
    s = C128
    hp = assert_route(s)
    Q, K, V = inputs(s)
    heads = fr.poisoned_heads(s.Hkv)
    p = fr.poison(Q, K, V, heads, recipe, [[place]], QB, hp, True)
    fr.check_intent(p, recipe, QB, hp, True)
    if recipe == "v_big":
        assert all(len(u) >= 1 for u in fr.v_big_units(p, QB, hp, -(-s.Sq // QB), True).values())
    O0 = run(s, Q, K, V)
    O1 = run(s, p.Q, p.K, p.V)
    clean = torch.tensor([h for h in range(s.H) if h not in p.touched], device=DEV)
    assert torch.equal(O1[0, clean], O0[0, clean]), "an untouched head changed"
    assert torch.isfinite(O1).all()
    for h in p.touched:   # the units that fell back, against float64
        ref, _ = fr.head_reference(p.Q[0, h].float(), p.K[0, h].float(), p.V[0, h].float(), 1 / s.d ** 0.5, True)
        q = ratio(O1[0, h].cpu().numpy(), ref, *BF16W)
        print(f"SEAM fallback {recipe} {place}, head {h}: worst error / tolerance {q:.3f}")
        assert q <= 1.0, f"head {h}: worst error / tolerance {q:.3f} at {BF16W[0]:g} + {BF16W[1]:g}|ref|"
    # the same call with other values past the diagonal of the unit that falls back (and of every unit in front of it)
    qb = place[0] // QB
    K2, V2 = past_diagonal(p.K, p.V, qb, 5)
    O2 = run(s, p.Q, K2, V2)
    rows = QB * (qb + 1)
    assert torch.equal(O2[:, :, :rows], O1[:, :, :rows]), f"{recipe}: rows < {rows} changed with what lies past their diagonal"
    assert not torch.equal(O2[:, :, QB * 8:], O1[:, :, QB * 8:])
