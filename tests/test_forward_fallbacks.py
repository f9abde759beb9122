"""The fallback passes of every forward kernel family, the family asserted through plan_ex.

Every bf16 / fp8 forward unit runs an optimistic pass first and is repeated by the tracked pass (fp16-weights units: then by the
bf16-weights tracked pass) when the result is not finite (csrc/kernel_bf16.hip.h: run_units).  The persistent kernels walk several
units per workgroup, request the next unit's Q and tile 0 under the current unit's epilogue and reuse the flag words in LDS from pass
to pass.  Here chosen units of roughly every fifth head are driven through those passes (tests/forward_routes.py: poison), on shapes
where every workgroup walks at least three units, and

  1. the heads the recipe did not touch are BIT-IDENTICAL to the run on the unpoisoned tensors (a unit reads only its own head:
     anything else is state leaking across a unit seam or between passes);
  2. so are, under the mask, the query blocks of the poisoned heads that end in front of the poisoned key's tile;
  3. the unpoisoned run meets the project's tolerance of its route (test_flash_attention.py: tol_for) against the float64 oracle on
     four sampled heads;
  4. the poisoned heads are finite everywhere and meet 4e-3 + 4e-3|ref| (BF16W, the bound of the existing spiked-data and |V| = 1e5
     tests; plus the output's rounding as in tol_for where O is bf16) against float64 on ALL rows, the LSE rtol 2e-5, atol 2e-3;
  5. spike_under (the optimistic pass gets through with weights up to 2^90, fp16 weights 2^10) differs bitwise from the same rows
     forced through the tracked pass.  Forcing is possible through the public API only under the mask: K[r2] = a Q[r2] on the LAST row
     r2 of the unit overflows that row and is visible to no other row of the unit.  Without the mask every row sees every key, so
     the non-causal families (bf16, f16_weights, bf16_padded d = 96, fp8) have no such comparison.

That a recipe makes a unit leave (or stay in) the optimistic pass is asserted on the CPU from the inputs alone
(test_recipes_mean_what_they_say, no GPU needed); fallback counts have not been measured on a device.
"""
from collections import namedtuple

import numpy as np
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import oracle  # noqa: E402  (checker only)
import forward_routes as fr  # noqa: E402

DEV = "cuda:0"
bf, f32, f16 = torch.bfloat16, torch.float32, torch.float16
FP8 = getattr(torch, "float8_e4m3fn", None)
BF16W = (4e-3, 4e-3)      # test_flash_attention.py: BF16W
STATED = (1e-3, 1e-3)     # test_flash_attention.py: STATED


def tol_for(in_dtype, out_dtype, weights=None, padded=False):
    """test_flash_attention.py: tol_for (bf16 / fp8 inputs, fp32 / bf16 outputs)"""
    atol, rtol = BF16W if (weights == bf or padded or in_dtype != bf) else STATED
    if out_dtype == bf:
        atol, rtol = atol + 4e-3, rtol + 4e-3
    return atol, rtol


# placements: lists of (row, key).  S = 1280 under the mask, 256-row blocks: blocks 0 .. 3 see fewer than FA_EARLY_KEYS keys
LATE, EARLY, SEAM = [(1100, 1030)], [(700, 300)], [(1000, 900), (1200, 1100)]   # late unit only / early units / blocks hp-1 and hp
C1280 = (LATE, EARLY, SEAM)
LAST = [(1280, 1270)]                                                            # S = 1281: the block with one live row
NC = ([(100, 700)], [(300, 200)], [(255, 500), (256, 600)])                     # no mask, Sq = 512: block 0, block 1, both
NC640 = ([(100, 500)], [(300, 200)], [(255, 400), (256, 600)])                  # ... against 640 keys
C512 = ([(300, 100)], [(500, 400)], [(200, 70), (400, 300)])                    # S = 512 under the mask
SPIKES, ALL = ("spike_over", "spike_under"), fr.RECIPES

Route = namedtuple("Route", "name fam idt odt H Hkv Sq Sk d causal wdt places recipes heads layout quiet", defaults=(None, "dense", ()))
ROUTES = [
    # the causal default above FA_EARLY_KEYS: fp16-weights and bf16-weights units in one walk.  LATE: the early blocks end in front
    # of key 1030 and never load it; quiet: (placement, block) that sees the key and stays in its optimistic pass all the same --
    # the late block when an early unit is poisoned
    Route("mix128", "causal_mix", bf, f32, 160, 160, 1280, 1280, 128, True, None, C1280, ALL, quiet=((1, 4),)),
    Route("mix64", "causal_mix", bf, bf, 256, 256, 1280, 1280, 64, True, None, C1280, ALL, quiet=((1, 4),)),
    Route("mix128_ragged", "causal_mix", bf, f32, 132, 132, 1281, 1281, 128, True, None, C1280 + (LAST,), ALL),
    Route("bf16w_causal128", "bf16", bf, f32, 160, 160, 1280, 1280, 128, True, bf, C1280, SPIKES),
    Route("bf16_nc128", "bf16", bf, f32, 400, 400, 512, 1024, 128, False, None, NC, SPIKES),
    Route("bf16_nc64", "bf16", bf, bf, 400, 400, 512, 1024, 64, False, None, NC, SPIKES),
    Route("f16w_nc128", "f16_weights", bf, f32, 400, 400, 512, 640, 128, False, None, NC640, ALL),
    Route("padded_nc96", "bf16_padded", bf, f32, 400, 400, 512, 1024, 96, False, None, NC, SPIKES),
    Route("padded_c40", "bf16_padded", bf, f32, 160, 160, 1280, 1280, 40, True, None, C1280, SPIKES),
    Route("fp8_c128", "fp8", "fp8", bf, 400, 400, 512, 512, 128, True, None, C512, SPIKES),
    Route("fp8_nc128", "fp8", "fp8", bf, 400, 400, 512, 512, 128, False, None, C512, SPIKES),
    # the pair kernel, d = 128: three passes in one kernel; |V| beyond fp16 at keys 300 / 100
    Route("pair128_c", "pair", bf, f32, 4, 4, 600, 600, 128, True, None, ([(400, 300)],), ALL, heads=(0, 2)),
    Route("pair128_nc", "pair", bf, f32, 8, 8, 512, 700, 128, False, None, ([(200, 100)],), ALL, heads=(0, 2, 7)),
    # ... d = 64: both configurations in one launch, one early and one late block poisoned
    Route("pair64_c", "pair", bf, f32, 2, 2, 1280, 1280, 64, True, None, ([(700, 300), (1200, 1100)],), ALL, heads=(1,)),
    # one more per persistent route: grouped queries (one K/V head poisons its whole group), Sq != Sk, model-layout strided views
    Route("mix128_gqa", "causal_mix", bf, bf, 160, 40, 1280, 1280, 128, True, None, C1280, ("spike_over", "v_big")),
    Route("mix64_strided", "causal_mix", bf, f32, 256, 256, 1280, 1280, 64, True, None, C1280, ("spike_over",), layout="model"),
    Route("bf16w_causal128_strided", "bf16", bf, bf, 160, 40, 1280, 1280, 128, True, bf, C1280, ("spike_over",), layout="model"),
    Route("bf16_nc128_gqa", "bf16", bf, bf, 400, 100, 512, 1024, 128, False, None, NC, ("spike_over",)),
    Route("bf16_nc64_strided", "bf16", bf, f32, 400, 400, 512, 1024, 64, False, None, NC, ("spike_over",), layout="model"),
    Route("f16w_nc128_gqa", "f16_weights", bf, f32, 400, 100, 512, 640, 128, False, None, NC640, ("spike_over+v_big",)),
    Route("padded_nc96_gqa", "bf16_padded", bf, f32, 400, 100, 512, 1024, 96, False, None, NC, ("spike_over",)),
    Route("padded_c40_strided", "bf16_padded", bf, f32, 160, 160, 1280, 1280, 40, True, None, C1280, ("spike_over",), layout="model"),
    Route("fp8_c128_gqa", "fp8", "fp8", bf, 400, 100, 512, 512, 128, True, None, C512, ("spike_over",)),
    Route("fp8_nc128_cross", "fp8", "fp8", bf, 400, 400, 512, 700, 128, False, None, C512, ("spike_over",)),
]
CASES = [(r, recipe) for r in ROUTES for recipe in r.recipes]
case_id = lambda c: f"{c[0].name}-{c[1]}"


def codes(r):
    flags = {None: 0, f16: fa.FA_FLAG_F16_WEIGHTS, bf: fa.FA_FLAG_BF16_WEIGHTS}[r.wdt]
    return (fa.FA_DTYPE_FP8_E4M3 if r.idt == "fp8" else fa.FA_DTYPE_BF16), {bf: fa.FA_DTYPE_BF16, f32: fa.FA_DTYPE_F32}[r.odt], flags


def geometry(r):
    """asserts the route, returns (rows of a query block, hp)"""
    args = (1, r.H, r.Sq, r.Sk, r.d, r.causal, *codes(r))
    assert fr.family(*args) == r.fam
    if r.fam == "pair":
        e, m = fa.plan_ex(*args)
        assert (m if m["q_blocks"] else e)["threads"] == 256
    else:
        units, grid = fr.walks(*args)
        assert units >= 3 * grid, f"{units} units on {grid} workgroups: every workgroup must walk at least three"
    return fr.blocks(*args)


_inputs = {}


def inputs(r):
    """the unpoisoned N(0,1) tensors of a route (fp8: already on the e4m3 grid, as float32), made once per route"""
    key = (r.idt, r.H, r.Hkv, r.Sq, r.Sk, r.d)
    if key not in _inputs:
        _inputs.clear()
        seed = 5000 + 7 * r.d + r.Sk
        t = [fr.randn((1, r.H, r.Sq, r.d), seed, f32), fr.randn((1, r.Hkv, r.Sk, r.d), seed + 1, f32), fr.randn((1, r.Hkv, r.Sk, r.d), seed + 2, f32)]
        _inputs[key] = tuple(x.to(FP8).float() if r.idt == "fp8" else x.to(bf) for x in t)
    return _inputs[key]


def poisoned(r, recipe, qbr, hp):
    Q, K, V = inputs(r)
    heads = list(r.heads) if r.heads else fr.poisoned_heads(r.Hkv)
    p = fr.poison(Q, K, V, heads, recipe, r.places, qbr, hp, r.causal, exact_pow2=r.idt == "fp8")
    if r.idt == "fp8":   # the spike survived the quantisation: it was built on the grid
        assert torch.equal(p.K.to(FP8).float(), p.K)
    return p


def forced(r, p, qbr, hp):
    """spike_under inputs with the unit of every head's first spike forced through the tracked pass: K[r2] = a Q[r2] on the unit's
    last row r2, which no other row of the unit sees.  Returns (Poison, {head: (first row of the unit, r2)})."""
    places, rows = [], []
    for place in r.places:
        row, key = place[0]
        r2 = min((row // qbr + 1) * qbr, r.Sq) - 1
        ok = r2 > row and r2 > key
        places.append([(r2, r2)] if ok else [])
        rows.append((row // qbr * qbr, r2) if ok else None)
    pf = fr.poison(p.Q, p.K, p.V, p.heads, "spike_over", places, qbr, hp, True, exact_pow2=r.idt == "fp8")
    return pf, {h: rows[i % len(rows)] for i, h in enumerate(p.heads) if rows[i % len(rows)]}


def has_forced(r, recipe):
    return recipe == "spike_under" and r.causal and r.Hkv == r.H


# ---- CPU: the recipes' preconditions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_recipes_mean_what_they_say(case):
    """No GPU: the route (plan_ex answers for a 256-CU device where none is visible), and in float64 from the inputs alone that
    spike_over rows overflow their unit's optimistic pass (e >= 140 with bf16 weights, >= 24 with fp16 weights), that spike_under
    rows sit in [8, 100] / [8, 12] with EVERY other row of the poisoned heads under the cap, that the units meant to stay quiet do,
    and that v_big is beyond fp16 in a unit that holds V as fp16 wherever the route has such units."""
    r, recipe = case
    qbr, hp = geometry(r)
    p = poisoned(r, recipe, qbr, hp)
    assert set(p.touched).isdisjoint(clean_heads(r, p)) and len(clean_heads(r, p)) >= 1
    fr.check_intent(p, recipe, qbr, hp, r.causal, expect_quiet=r.quiet if recipe.startswith("spike") else (), n_places=len(r.places))
    if "v_big" in recipe and hp > 0:
        nQ = -(-r.Sq // qbr)
        units = fr.v_big_units(p, qbr, hp, nQ, r.causal)
        assert sum(len(u) for u in units.values()) >= 1
    if has_forced(r, recipe):
        pf, rows = forced(r, p, qbr, hp)
        assert rows
        G = r.H // r.Hkv
        for h, (r0, r2) in rows.items():
            e = fr.row_excess(pf.Q[0, h * G].float(), pf.K[0, h].float(), 1 / r.d ** 0.5, True)
            assert e[r2] >= fr.OVER[fr.weights_of(r2, qbr, hp)]
            assert torch.equal(pf.K[0, h, :r2], p.K[0, h, :r2]) and torch.equal(pf.Q[0, h * G], p.Q[0, h * G])   # rows r0 .. r2-1 see the same inputs


def clean_heads(r, p):
    touched = set(p.touched)
    return [h for h in range(r.H) if h not in touched]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def to_device(r, t, heads):
    """a [1, heads, S, d] tensor on the device in the route's input type and layout"""
    t = t.to(FP8) if r.idt == "fp8" else t
    if r.layout == "dense":
        return t.to(DEV)
    S = t.shape[2]
    buf = torch.empty(1, S, heads * r.d, dtype=t.dtype, device=DEV)
    v = buf.view(1, S, heads, r.d).transpose(1, 2)
    if t.element_size() == 1:
        v.view(torch.uint8).copy_(t.view(torch.uint8).to(DEV))
    else:
        v.copy_(t.to(DEV))
    return v


def run(r, Q, K, V, want_lse):
    """the route's call: same shape, flags, layout and kind of output buffer whatever the data"""
    O = None
    if r.layout == "model":
        O = torch.full((1, r.Sq, r.H * r.d), float("nan"), dtype=r.odt, device=DEV).view(1, r.Sq, r.H, r.d).transpose(1, 2)
    out = fa.flash_attention(to_device(r, Q, r.H), to_device(r, K, r.Hkv), to_device(r, V, r.Hkv), O, is_causal=r.causal, out_dtype=r.odt,
                             weights_dtype=r.wdt, return_lse=want_lse)
    torch.cuda.synchronize()
    return out if want_lse else (out, None)


def lse_modes(r):
    # bf16 without the mask: the LSE request selects another instantiation (fp32 row sums) -- both
    return (True, False) if r.fam == "bf16" and not r.causal else (True,)


def ratio(got, ref, atol, rtol):
    """worst error / tolerance"""
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def one_head_oracle(r, Q, K, V, h):
    """float64 oracle of query head h: oracle.attention_rows (square problems), oracle.attention_numpy (Sq != Sk)"""
    hk = h // (r.H // r.Hkv)
    q, k, v = Q[:, h:h + 1].float().numpy(), K[:, hk:hk + 1].float().numpy(), V[:, hk:hk + 1].float().numpy()
    if r.Sq == r.Sk:
        return oracle.attention_rows(q, k, v, (0, 1), (0, r.Sq), causal=r.causal)[0]
    return oracle.attention_numpy(q, k, v, causal=r.causal)[0, 0]


_clean = {}


def clean_run(r):
    """the route's run on the unpoisoned tensors, once per route: outputs per LSE mode, checked against the oracle on four heads"""
    if r.name not in _clean:
        _clean.clear()
        Q, K, V = inputs(r)
        outs = {m: run(r, Q, K, V, m) for m in lse_modes(r)}
        atol, rtol = tol_for(bf if r.idt != "fp8" else FP8, r.odt, weights=r.wdt, padded=r.fam == "bf16_padded")
        worst = 0.0
        for h in sorted({0, r.H // 3, (2 * r.H) // 3, r.H - 1}):
            ref = one_head_oracle(r, Q, K, V, h)
            for m, (O, _) in outs.items():
                got = O[0, h].float().cpu().numpy()
                assert np.isfinite(got).all()
                q = ratio(got, ref, atol, rtol)
                worst = max(worst, q)
                assert q <= 1.0, f"clean run, head {h}, lse={m}: worst error / tolerance {q:.3f} at {atol:g} + {rtol:g}|ref|"
        _clean[r.name] = (outs, worst)
    return _clean[r.name]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fallback_passes(case):
    r, recipe = case
    if r.idt == "fp8" and FP8 is None:
        pytest.skip("torch build without float8_e4m3fn")
    qbr, hp = geometry(r)
    clean, clean_worst = clean_run(r)
    p = poisoned(r, recipe, qbr, hp)
    untouched = torch.tensor(clean_heads(r, p), device=DEV)
    G = r.H // r.Hkv
    atol, rtol = BF16W if r.odt == f32 else (BF16W[0] + 4e-3, BF16W[1] + 4e-3)      # (bf16 O: its rounding, as tol_for adds it)
    # the float64 reference of the touched heads, all rows (at most 24 of them: every placement is among the first)
    checked = p.touched if len(p.touched) <= 24 else [hq for h in p.heads[:24 // G] for hq in range(h * G, (h + 1) * G)]
    refs = {hq: fr.head_reference(p.Q[0, hq].float(), p.K[0, hq // G].float(), p.V[0, hq // G].float(), 1 / r.d ** 0.5, r.causal) for hq in checked}
    worst_o = worst_lse = 0.0
    last = None
    for m in lse_modes(r):
        O, lse = run(r, p.Q, p.K, p.V, m)
        O0, lse0 = clean[m]
        # 1. the heads the recipe did not touch: bit for bit the unpoisoned run
        assert torch.equal(O[0, untouched], O0[0, untouched]), "an untouched head changed"
        if m:
            assert torch.equal(lse[0, untouched], lse0[0, untouched]), "the LSE of an untouched head changed"
        # 2. under the mask: the query blocks of a poisoned head that end in front of the poisoned key's tile
        if r.causal:
            for h in p.heads:
                rows = (p.first_key[h] // fr.TILE * fr.TILE) // qbr * qbr
                if rows:
                    sl = slice(h * G, (h + 1) * G)
                    assert torch.equal(O[0, sl, :rows], O0[0, sl, :rows]), f"head(s) {sl}: rows < {rows} never load the poisoned key"
                    assert not m or torch.equal(lse[0, sl, :rows], lse0[0, sl, :rows])
        # 4. the poisoned heads: finite everywhere, all rows of the checked ones against float64
        idx = torch.tensor(p.touched, device=DEV)
        assert torch.isfinite(O[0, idx].float()).all(), "non-finite output in a poisoned head"
        assert not m or torch.isfinite(lse[0, idx]).all()
        for hq, (ref, ref_lse) in refs.items():
            got = O[0, hq].float().cpu().numpy()
            q = ratio(got, ref, atol, rtol)
            worst_o = max(worst_o, q)
            assert q <= 1.0, f"{recipe}, head {hq}, lse={m}: worst error / tolerance {q:.3f} at {atol:g} + {rtol:g}|ref|"
            if m:
                ql = ratio(lse[0, hq].cpu().numpy(), ref_lse, 2e-3, 2e-5)
                worst_lse = max(worst_lse, ql)
                assert ql <= 1.0, f"{recipe}, head {hq}: LSE worst error / tolerance {ql:.3f} at rtol 2e-5, atol 2e-3"
        last = O
    differ = ""
    if has_forced(r, recipe):
        # 5. the same rows through the tracked pass: inside the tolerance too, and other bits
        pf, rows = forced(r, p, qbr, hp)
        Of, _ = run(r, pf.Q, pf.K, pf.V, lse_modes(r)[-1])
        same = 0
        for h, (r0, r2) in rows.items():
            a, b = last[0, h, r0:r2], Of[0, h, r0:r2]
            same += int(torch.equal(a, b))
            if h in refs:
                q = ratio(b.float().cpu().numpy(), refs[h][0][r0:r2], atol, rtol)
                worst_o = max(worst_o, q)
                assert q <= 1.0, f"tracked pass forced, head {h}: worst error / tolerance {q:.3f}"
        assert same == 0, f"{same} of {len(rows)} units gave the same bits through the optimistic and the tracked pass"
        differ = f"  tracked pass forced on {len(rows)} units: other bits in all"
    print(f"FALLBACK {r.name} [{r.fam}] {recipe}: {len(p.touched)} poisoned heads of {r.H}, worst error / tolerance O {worst_o:.3f}  "
          f"LSE {worst_lse:.3f}  clean run {clean_worst:.3f}{differ}")
