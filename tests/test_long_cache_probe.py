"""CPU proof of the long-cache instrument (tests/long_cache_probe.py) on a few thousand keys whose codes, through `base`, are the 24-bit
ones of a long cache: (a) ranges() is kv_cache_check.visible, (b) the closed forms equal the suite's float64 references
(kv_cache_check.reference, reference_ragged) to 1e-12 -- decode, chunked prefill, ragged,
W = 0 / 100 / 4096, len < Sq, empty sequences, all four cache forms --, (c) the fp32 emulation of csrc/decode_bf16.hip.h returns the
expected bits under 1, 3 and 64 splits and stays within 0.7 of the LSE bound, (d) every wrong kernel of long_cache_probe.MUTANTS is refused
on a named row, (e) for every case tests/test_long_cache.py runs on the GPU both sides of every split boundary of every row block are
targeted, a head-straddling block exists where the case claims one, and every row has a closed form.  Conditions on the instrument,
not measurements."""
import dataclasses
import functools

import numpy as np
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import extend_window_check as ewc  # noqa: E402
import kv_cache_check as kv  # noqa: E402
import long_cache_probe as cp  # noqa: E402

BASE = 2 ** 24 - 8192
S = functools.partial(cp.Spec, H=4, Hkv=2)
# (spec, rows per block): decode 16; chunked prefill 64 at d = 128 and 32 at d = 64 (asserted against the library's plan below)
SPECS = {
    "decode_sq1": S("decode", ((1, 4019), (1, 3000), (1, 130)), 4096, 128, base=BASE, seed=1),
    "decode_sq16_full": S("decode", ((16, 4096), (16, 3967), (16, 7)), 4096, 64, causal=False, base=BASE, seed=2),
    "decode_paged_fp8_w100": S("decode", ((16, 4019), (16, 1000)), 4096, 128, W=100, fp8=True, page=32, base=BASE, seed=3),
    "decode_paged_shared": S("decode", ((16, 4019), (16, 1000)), 4096, 64, page=32, share=20, base=BASE, seed=13),
    "decode_fp8_w4096": cp.Spec("decode", ((5, 6000),), 6144, 64, 4, 1, W=4096, fp8=True, base=BASE, seed=4),
    "extend_short": S("extend", ((150, 4019), (150, 100)), 4096, 128, base=BASE, seed=5),
    "extend_straddle_d64_full": S("extend", ((250, 3000),), 4096, 64, causal=False, base=BASE, seed=6),
    "extend_paged_w4096": S("extend", ((200, 6000),), 6144, 128, W=4096, page=128, base=BASE, seed=7),
    "extend_fp8_w100": S("extend", ((250, 4019),), 4096, 64, W=100, fp8=True, base=BASE, seed=8),
    "extend_paged_fp8_w100_full": S("extend", ((250, 4019),), 4096, 128, causal=False, W=100, fp8=True, page=64, base=BASE, seed=9),
    "ragged": S("varlen", ((17, 4019), (0, 77), (250, 3000), (64, 30), (1, 1), (0, 4096), (3, 4096)), 4096, 128, pad=50, base=BASE, seed=10),
    "ragged_paged_w100": S("varlen", ((17, 4019), (0, 77), (250, 3000), (64, 30), (1, 1)), 4096, 64, W=100, page=16, pad=50, base=BASE, seed=11),
    "ragged_paged_fp8_w4096": S("varlen", ((250, 6000), (0, 5), (3, 5000)), 6144, 128, W=4096, fp8=True, page=128, pad=50, base=BASE, seed=12),
}


def rpb_of(spec):
    return 16 if spec.kind == "decode" else (64 if spec.d == 128 else 32)


@functools.lru_cache(maxsize=None)
def problem(name, ns=1):
    spec = SPECS[name]
    if spec.fp8 and cp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")
    cache = cp.build_cache(spec)
    rounds, missing = cp.plan_targets(spec, ns, rpb_of(spec), cache["phys"])
    return spec, cache, [cp.build_queries(spec, r) for r in rounds], missing


def dense_logical(spec, cache):
    """float64 [B, Hkv, cap, d] of the logical cache (paged: gathered, fp8: dequantised), 0 where the contract lets anything lie"""
    B = len(spec.seqs)
    K, V = torch.zeros((2, B, spec.Hkv, spec.cap, spec.d), dtype=torch.float64)
    for b in range(B):
        if spec.seqs[b][0] == 0 and spec.kind == "varlen":
            continue
        lo, L = spec.first(b), spec.length(b)
        j = torch.arange(lo, L)
        for kvh in range(spec.Hkv):
            if spec.page:
                page = torch.as_tensor(cache["phys"][b])[j // spec.page]
                assert int(page.min()) >= 0
                k, v = cache["K"][page, kvh, j % spec.page], cache["V"][page, kvh, j % spec.page]
            else:
                k, v = cache["K"][b, kvh, lo:L], cache["V"][b, kvh, lo:L]
            K[b, kvh, lo:L] = k.float().double() * (cp.KD[kvh % 4] if spec.fp8 else 1.0)
            V[b, kvh, lo:L] = v.float().double() * (cp.VD[kvh % 4] if spec.fp8 else 1.0)
    assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(V).all())
    return K, V


def test_the_plan_has_the_row_blocks_the_proof_uses():
    for name, spec in SPECS.items():
        assert cp.plan_of(spec, 1)["rows_per_block"] == rpb_of(spec), name


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("W", [0, 1, 16, 100, 4096])
def test_ranges_are_the_visible_windows(causal, W):
    for L, Sq in ((1, 1), (130, 1), (130, 16), (300, 300), (200, 300), (1, 40), (1000, 257)):
        lo, lim = cp.ranges(L, Sq, causal, W)
        elo, ehi = ewc.row_edges(L, Sq, causal, W)
        assert lo.tolist() == elo and (lim - 1).tolist() == ehi, (L, Sq)
        assert int(kv.visible(L, Sq, causal, W).sum()) == int((lim - lo).sum())
    x = np.arange(0, 700)
    for a in (64, 16):
        assert (cp.anchors_below(x, a) == np.cumsum(np.concatenate([[0], cp.is_anchor(x, a)[:-1]]))).all()


@pytest.mark.parametrize("name", list(SPECS))
def test_closed_forms_are_the_float64_truth(name):
    spec, cache, qs, _ = problem(name)
    K, V = dense_logical(spec, cache)
    scale = cp.fp.PREFILL_SCALE(0)
    for q in qs[:2]:
        exp = cp.expected(spec, q, torch.float32)
        if spec.kind == "varlen":
            sq = [s for s, _ in spec.seqs]
            O, L, owned = kv.reference_ragged(q["Q"].float(), K, V, sq, [L for _, L in spec.seqs], spec.causal, spec.W, scale=scale)
            refs = [(O[a:b].transpose(0, 1), L[:, a:b]) if owned[a:b].any() else None for a, b in zip(kv.cu_of(sq), kv.cu_of(sq)[1:])]
            assert [r is None for r in refs] == [e is None for e in exp]
        else:
            O, L = kv.reference(q["Q"].float(), K, V, [L for _, L in spec.seqs], spec.causal, spec.W, scale=scale)
            refs = list(zip(O, L))
        hidden = 0
        for e, r in zip(exp, refs):
            if e is None:
                continue
            assert float((e["O"].double() - r[0]).abs().max()) <= 1e-12
            assert bool(((e["lse"] - r[1]).abs() <= 1e-12 * r[1].abs()).all())
            assert bool((e["O"][torch.as_tensor(~e["vis"])] == 0).all())
            hidden += int((~e["vis"]).sum())
        assert hidden > 0, "no row with a hidden target"


def test_hidden_targets_come_in_all_three_kinds():
    spec, _, qs, _ = problem("extend_fp8_w100")
    t, (lo, lim) = qs[0]["target"][0], cp.ranges(4019, 250, True, 100)
    assert ((t >= lim[None]) & (t < 4019)).any() and (t < lo[None]).any() and (t >= 4019).any()
    vis = (t >= lo[None]) & (t < lim[None])
    assert 0.08 < 1 - vis.mean() < 0.25 and (vis & (lim[None] - t <= cp.NEAR)).mean() > 0.4


@functools.lru_cache(maxsize=None)
def emulated(name, ns, b):
    spec, cache, qs, _ = problem(name, ns)
    return cp.emulate(spec, cache, qs[0], b, ns, rpb_of(spec))


@pytest.mark.parametrize("ns", [1, 3, 64])
@pytest.mark.parametrize("name", list(SPECS))
def test_the_fp32_emulation_returns_the_expected_bits(name, ns):
    """every form is bit-exact in the emulation: none needed a bound of its own"""
    spec, cache, qs, _ = problem(name, ns)
    rpb = rpb_of(spec)
    q = qs[0]
    for o_dtype in (torch.bfloat16, torch.float32):
        exp = cp.expected(spec, q, o_dtype)
        for b, e in enumerate(exp):
            if e is None:
                continue
            O, lse = emulated(name, ns, b)
            assert torch.equal(cp.lp._bits_of(O.to(o_dtype)), cp.lp._bits_of(e["O"])), (name, b)
            ratio = (lse.double() - e["lse"]).abs() / cp.lse_bound(e["lse"], e["log2k"])
            assert float(ratio.max()) <= 0.7, (name, b, float(ratio.max()))


# mutant -> (problem, splits, sequence, a part of the named row's forced place; None: any row)
MUTANT_PLACES = {
    "split_one_tile_short": ("extend_short", 3, 0, "last key below split 1"),
    "split_one_tile_long": ("extend_short", 3, 0, "first key of split 1"),
    "limb_of_the_last_row": ("extend_short", 1, 0, "lim - 1 of the first row"),
    "firstb_one_tile_high": ("extend_paged_w4096", 3, 0, "lo of the first row"),
    "lo_plus_1": ("extend_fp8_w100", 1, 0, "lo of the"),
    "lo_minus_1": ("extend_fp8_w100", 1, 0, "lo - 1 of the"),
    "records_of_the_capacity": ("decode_sq1", 3, 0, "last key of the length"),
    "page_plus_1": ("decode_paged_fp8_w100", 1, 0, "first key past a page seam"),
    "table_row_0": ("ragged_paged_w100", 3, 2, None),
    "page_shift_minus_1": ("extend_paged_w4096", 1, 0, "a page seam"),
    "key_minus_2^16": ("extend_short", 1, 0, "last key of the length"),
    "key_minus_2^(31-log2 row bytes)": ("extend_short", 1, 0, "first key of the length"),
    "slab_row_of_the_next_token": ("ragged", 3, 2, None),
    "q0_of_the_next_sequence": ("ragged", 1, 0, None),
    "descale_of_the_next_head": ("decode_paged_fp8_w100", 3, 1, None),
}


def test_every_mutant_has_a_place():
    assert set(MUTANT_PLACES) == set(cp.MUTANTS)


@pytest.mark.parametrize("mutant", cp.MUTANTS)
def test_every_mutant_is_refused_on_a_named_row(mutant):
    name, ns, b, place = MUTANT_PLACES[mutant]
    spec, cache, qs, _ = problem(name, ns)
    rpb = rpb_of(spec)
    refused = []
    for q in qs:
        e = cp.expected(spec, q, torch.bfloat16)[b]
        O, lse = cp.emulate(spec, cache, q, b, ns, rpb, mutant)
        O = O.to(torch.bfloat16)
        bad = (cp.lp._bits_of(O) != cp.lp._bits_of(e["O"])).any(-1) | ~((lse.double() - e["lse"]).abs() <= cp.lse_bound(e["lse"], e["log2k"]))
        rows = [(h, i) for h, i in torch.nonzero(bad).tolist()]
        named = [(h, i) for h, i in rows if (b, h, i) in q["named"] and (place is None or place in q["named"][(b, h, i)])]
        if place is None:
            named = rows
        refused += named
        if mutant == "split_one_tile_long" and named:        # the doubled tile: O = (V + V) / 2 keeps its bits, the LSE gains ln 2
            h, i = named[0]
            assert torch.equal(cp.lp._bits_of(O[h, i]), cp.lp._bits_of(e["O"][h, i])) and abs(float(lse[h, i]) - float(e["lse"][h, i]) - np.log(2)) < 1e-3
        if named:
            with pytest.raises(AssertionError, match=f"head {named[0][0]} row {named[0][1]} \\(row block"):
                (h, i), Om, Lm = named[0], e["O"].clone(), e["lse"].float()       # the mutant's result on that row alone: the checker names it
                Om[h, i], Lm[h, i] = O[h, i], lse[h, i]
                Ob, Lb = Om[None] if spec.kind != "varlen" else Om.transpose(0, 1), Lm[None] if spec.kind != "varlen" else Lm
                one = dataclasses.replace(spec, seqs=(spec.seqs[b],), pad=0, share=0)
                q1 = dict(target=[q["target"][b]], named={(0, h, i): n for (bb, h, i), n in q["named"].items() if bb == b})
                cp.check(mutant, one, q1, [e], Ob, Lb, ns, rpb)
            break
    print(f"{mutant}: refused on {len(refused)} rows, first {refused[:3]}")
    assert refused, mutant


# ---- the GPU cases: coverage asserted, not assumed ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_cases():
    return cp.gpu_cases()


@pytest.mark.parametrize("case", list(cp.gpu_cases()))
def test_coverage_of_the_gpu_cases(case):
    spec, splits = gpu_cases()[case]
    if spec.fp8 and cp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")
    phys = cp.layout(spec)[1] if spec.page else None
    for ns_asked in splits:
        plan = cp.plan_of(spec, ns_asked)
        ns, rpb = plan["num_splits"], plan["rows_per_block"]
        assert ns == ns_asked or ns_asked == 0
        rounds, missing = cp.plan_targets(spec, ns, rpb, phys)      # (asserts that every row has a closed form)
        for b, (sq, _) in enumerate(spec.seqs):
            if sq == 0:
                continue
            L, first = spec.length(b), spec.first(b)
            lo, lim = cp.ranges(L, sq, spec.causal, spec.W)
            hit = {}
            for r in rounds:
                for (bb, h, i), n in r["named"].items():
                    if bb == b and "split" in n:
                        hit[(h // spec.G, ((h % spec.G) * sq + i) // rpb, int(r["target"][b][h, i]))] = lo[i] <= r["target"][b][h, i] < lim[i]
            nrows = spec.G * sq
            for rb in range(-(-nrows // rpb)):
                tlo, ntb = ewc.block_range(rpb, spec.G, sq, L, spec.W, spec.causal, rb)
                rows_i = np.array([pr % sq for pr in range(rb * rpb, min((rb + 1) * rpb, nrows))])
                for s in range(1, ns):
                    t0 = tlo + (ntb - tlo) * s // ns
                    for k in (t0 * cp.TILE - 1, t0 * cp.TILE):
                        if not (max(first, 1) <= k < L):
                            continue
                        seen = bool(((lo[rows_i] <= k) & (k < lim[rows_i])).any())
                        for kvh in range(spec.Hkv):
                            assert hit.get((kvh, rb, k), False) == seen, (case, ns, b, kvh, rb, s, k)
            if spec.kind != "decode" and sq % rpb and spec.G > 1:
                straddling = [rb for rb in range(-(-nrows // rpb)) if (rb * rpb) // sq != (min((rb + 1) * rpb, nrows) - 1) // sq]
                assert straddling, case
    if "sq1000" in case:
        assert 1000 % rpb != 0                                    # the blocks that straddle two heads
        if spec.d == 128:
            assert (spec.G * 1000) % rpb != 0
