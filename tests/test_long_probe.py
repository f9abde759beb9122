"""CPU proof of the long-sequence instrument (tests/long_probe.py) at Sk <= 4096 with `base` chosen so that the codes reach 2^24:
(a) its O(S d) closed forms are the truth (float64 oracle, float64 autograd; hidden targets, ragged Sq != Sk), (b) the fp32 emulation of
the kernels' arithmetic returns the expected O bit for bit, in the optimistic and in the tracked pass, (c) the rows that run with bf16
weights stay in the optimistic pass, (d) every wrong kernel of long_probe.MUTANTS is refused on a named row.  Conditions on the
instrument, not measurements."""
import functools
import math

import numpy as np
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import oracle  # noqa: E402  (checker only)
import forward_routes as fr  # noqa: E402
import grad_check as gc  # noqa: E402
import long_probe as lp  # noqa: E402

BASE = 2 ** 24 - 4096
# (Sq, Sk, d, causal, format): self-attention with a ragged last tile, rows past the last key, fewer rows than keys, no mask, fp8
SHAPES = [(4019, 4019, 64, True, "bf16"), (1000, 700, 64, True, "bf16"), (700, 1000, 128, True, "f32"), (300, 1000, 128, False, "bf16"),
          (900, 900, 128, True, "fp8")]


@functools.lru_cache(maxsize=None)
def problem(Sq, Sk, d, causal, fmt, H=1, Hkv=1):
    if fmt == "fp8" and lp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")
    p = lp.build(Sq, Sk, d, fmt, H, Hkv, causal, BASE, seed=3)
    assert p["nb"] == 24 and int(p["target"].max()) + BASE < 2 ** 24
    return p


def f64(t):
    return t.to(torch.float32).double().numpy()


def test_the_format_constants_are_exact():
    """the kernels' c = fp32(scale * fp32(log2 e)) is 2^k, a c is 128 in every format, the anchor's query value splits into exact parts"""
    for fmt, (dtype, a, k) in lp.FORMATS.items():
        if dtype is None:                                     # torch without float8_e4m3fn
            continue
        c = np.float32(np.float32(lp.fp.PREFILL_SCALE(k)) * np.float32(1.4426950408889634))
        assert float(c) == 2.0 ** k and a * 2 ** k == lp.UNIT, fmt
        for nb in range(2, 25):
            parts = lp.anchor_values(a * nb - lp.E // 2 ** k, dtype)
            assert len(parts) <= (2 if fmt == "fp8" else 1), (fmt, nb, parts)


@pytest.mark.parametrize("Sq,Sk,d,causal,fmt", SHAPES)
def test_targets_cover_what_the_docstring_says(Sq, Sk, d, causal, fmt):
    p = problem(Sq, Sk, d, causal, fmt)
    t, vis = p["target"][0], lp.seen(p)[0]
    i = torch.arange(Sq)
    assert int(t.min()) >= 1 and int(t.max()) <= Sk - 1
    assert p["named"]["last row"] == Sq - 1 and int(t[Sq - 1]) == min(Sq - 1, Sk - 1) if causal else Sk - 1
    for name, k in lp.forced_keys(Sk, p["stride_bytes"]).items():
        if name in p["named"]:
            assert int(t[p["named"][name]]) == k and bool(vis[p["named"][name]]), name
    if causal:
        hidden = ~vis & (i > 0)
        assert 0.10 < float(hidden[:Sk - 1].float().mean()) < 0.20 and int((t - i)[hidden].max()) <= lp.NEAR and int((t - i)[hidden].min()) >= 1
        near = vis & (i - t < lp.NEAR)
        assert float(near.float().mean()) > 0.35
        assert {"last key of a middle tile", "first key of a middle tile"} <= set(p["named"]) or Sq < Sk
    assert len(torch.unique(t // lp.TILE)) > 0.5 * (min(Sq, Sk) // lp.TILE)                   # the rest spread over the tiles


def test_byte_lines_are_forced_at_a_long_heads_stride():
    keys = lp.forced_keys(2 ** 18 - 256, 8192)
    assert keys["first key past byte 1073741824"] == 2 ** 17 and keys["last key below byte 1073741824"] == 2 ** 17 - 1
    t, named = lp.targets(512, 2 ** 23 - 193, False, 0, "cpu", 256)
    for line in lp.BYTE_LINES:
        assert int(t[named[f"first key past byte {line}"]]) * 256 == line and int(t[named[f"last key below byte {line}"]]) * 256 == line - 256
    assert int((t >= 2 ** 23 - 193 - 512 - lp.NEAR).sum()) > 200                             # cross-attention: half on the last keys


@pytest.mark.parametrize("Sq,Sk,d,causal,fmt", SHAPES)
def test_forward_closed_form_is_the_float64_truth(Sq, Sk, d, causal, fmt):
    p = problem(Sq, Sk, d, causal, fmt)
    expO, expL, _ = lp.expected_forward(p)
    q, k, v = f64(p["Q"]), f64(p["K"]), f64(p["V"])
    O = oracle.attention_numpy(q, k, v, scale=p["scale"], causal=causal)
    L = oracle.lse_numpy(q, k, scale=p["scale"], causal=causal)
    assert np.abs(O - expO.double().numpy()).max() <= 1e-12
    assert (np.abs(L - expL.numpy()) <= 1e-12 * np.abs(expL.numpy())).all()
    if causal:
        hidden = ~lp.seen(p)[0]
        assert bool(hidden[0]) and bool((expO[0, 0, hidden] == 0).all()) and float(expL[0, 0, hidden].max()) == lp.LN2 * (128 * 24 - 64) < float(expL.max())


@pytest.mark.parametrize("Sq,Sk,d,H,Hkv,causal", [(900, 900, 64, 1, 1, True), (700, 1000, 128, 1, 1, True), (1000, 700, 64, 1, 1, True),
                                                  (300, 1000, 128, 1, 1, False), (600, 600, 64, 4, 1, True)])
def test_backward_closed_form_is_the_float64_truth(Sq, Sk, d, H, Hkv, causal):
    p = lp.build_backward(Sq, Sk, d, H, Hkv, causal, BASE, seed=5)
    ref = lp.backward_closed_form(p)
    (dQ, dK, dV), _ = gc.reference_grads(p["Q"], p["K"], p["V"], p["scale"], causal, dO=p["dO"])
    mQ, mK, mV = gc.magnitudes(p["Q"], p["K"], p["V"], p["dO"], p["scale"], causal)
    for name, truth, mine in (("dQ", dQ, ref["dQ"]), ("dK", dK, lp.dense(p, ref, "dK")), ("dV", dV, lp.dense(p, ref, "dV")),
                              ("mag dQ", mQ, ref["mag_dQ"]), ("mag dK", mK, lp.dense(p, ref, "mag_dK")), ("mag dV", mV, lp.dense(p, ref, "mag_dV"))):
        assert float((truth - mine).abs().max()) <= 1e-12 * max(1.0, float(truth.abs().max())), name
    O = gc.explicit_attention(p["Q"].double(), p["K"].double(), p["V"].double(), p["scale"], causal)
    assert float((O - ref["O"]).abs().max()) <= 1e-12
    # what the construction promises: dQ lives at column 0, both halves of a pair carry weight, the signal is of the magnitude's size
    assert float(ref["dQ"][..., 1:].abs().max()) <= 1e-12 * float(ref["dQ"].abs().max())
    both = (p["target"] | 1) <= torch.arange(Sq)[None] if causal else torch.ones_like(p["target"], dtype=torch.bool)
    sig, mag = ref["dQ"][0, ..., 0].abs()[both], ref["mag_dQ"][0, ..., 0][both]
    assert float(both.float().mean()) > 0.7 and float((sig / mag).median()) > 0.05
    untouched = torch.ones(Sk, dtype=torch.bool)
    untouched[ref["heads"][0]["keys"]] = False
    assert int(untouched.sum()) > 0 and float(dK[0, 0, untouched].abs().max()) < 1e-45 and float(dV[0, 0, untouched].abs().max()) < 1e-50   # weights <= 2^-192: 0 in fp32


@pytest.mark.parametrize("tracked", [False, True], ids=["optimistic", "tracked"])
@pytest.mark.parametrize("Sq,Sk,d,causal,fmt", SHAPES)
def test_the_fp32_emulation_returns_the_expected_bits(Sq, Sk, d, causal, fmt, tracked):
    p = problem(Sq, Sk, d, causal, fmt)
    expO = lp.expected_forward(p)[0]
    O = lp.emulate(p, 0, torch.arange(Sq), tracked)
    assert torch.equal(lp._bits_of(O), lp._bits_of(expO[0, 0]))
    assert torch.equal(lp._bits_of(O.to(torch.bfloat16)), lp._bits_of(lp.expected_forward(p, torch.bfloat16)[0][0, 0]))


def test_rows_with_bf16_weights_stay_in_the_optimistic_pass():
    Sq, Sk, d = 4019, 4019, 64
    p = problem(Sq, Sk, d, True, "bf16")
    codes = (fa.FA_DTYPE_BF16, fa.FA_DTYPE_F32, 0)
    assert fr.family(1, 32, Sq, Sk, d, True, *codes) == "causal_mix"
    rows_per_block, hp = fr.blocks(1, 32, Sq, Sk, d, True, *codes)
    rows = np.arange(hp * rows_per_block, Sq)
    assert len(rows) > 2000
    e = fr.row_excess(p["Q"][0, 0].float(), p["K"][0, 0].float(), p["scale"], True, rows)
    beyond = (lp.seen(p)[0] & (p["target"][0] >= lp.TILE)).numpy()[rows]
    assert beyond.mean() > 0.7
    assert (np.abs(e[beyond] - lp.E) < 1e-3).all() and 30.0 <= e[beyond].min() and e.max() <= fr.UNDER["bf16"]
    assert (np.abs(e[~beyond]) < 1e-3).all()                 # target in tile 0 or hidden: tile 0 holds the row maximum
    assert lp.E >= fr.OVER["f16"]                            # an fp16-weights unit leaves its optimistic pass: exactness holds in the tracked one


MUTANT_SHAPE = (4019, 4019, 128, True, "bf16")               # 256-byte rows: byte 2^31 of a head is key 2^23


def mutant_places(p):
    """{mutant: (argument, named rows)}"""
    n, t = p["named"], p["target"][0]
    i = torch.arange(len(t))
    close = torch.nonzero((t > i) & (t - i <= lp.TILE) & (i >= lp.TILE))[:, 0]
    mid = int(t[n["first key of a middle tile"]]) // lp.TILE
    everywhere = [n["first key"], n["last key of a middle tile"], n["last row"]]
    return {"key_minus_2^16": (16, everywhere), "key_minus_2^21": (21, everywhere),
            "key_minus_2^(31-log2 row bytes)": (31 - int(math.log2(p["stride_bytes"])), everywhere),
            "tile_skipped": (mid, [n["first key of a middle tile"], n["last key of a middle tile"]]),
            "last_partial_tile_dropped": (None, [n["last row"]]), "mask_plus_64": (None, close[:4].tolist()),
            "mask_minus_64": (None, [n["last key of a middle tile"], n["last row"]]),
            "kv_rows_one_tile_short": (None, [n["last key of a middle tile"]]), "v_of_the_next_key": (None, everywhere)}


@pytest.mark.parametrize("tracked", [False, True], ids=["optimistic", "tracked"])
def test_every_mutant_is_refused_on_a_named_row(tracked):
    p = problem(*MUTANT_SHAPE)
    assert p["stride_bytes"] == 256 and 4019 % lp.TILE and (p["named"]["last key of a middle tile"] + 1) % lp.QBLOCK == 0
    expO = lp.expected_forward(p)[0][0, 0]
    places = mutant_places(p)
    assert set(places) | {"rows_alias_mod_2^16"} == set(lp.MUTANTS)
    for mutant, (arg, rows) in places.items():
        assert rows, mutant
        assert torch.equal(lp._bits_of(lp.emulate(p, 0, rows, tracked)), lp._bits_of(expO[rows])), mutant
        refused = (lp._bits_of(lp.emulate(p, 0, rows, tracked, mutant, arg)) != lp._bits_of(expO[rows])).any(-1)
        print(f"{mutant}: refused on rows {[r for r, bad in zip(rows, refused.tolist()) if bad]} of {rows}")
        assert bool(refused.all()), (mutant, rows, refused.tolist())


def test_aliased_rows_are_refused():
    """rows >= 2^16 computed from (or stored over) row mod 2^16: a 16-bit row index"""
    Sq, Sk, d = 2 ** 16 + 256, 1000, 64
    p = problem(Sq, Sk, d, False, "bf16")
    t = p["target"][0]
    rows = torch.arange(2 ** 16, Sq)
    rows = rows[t[rows] != t[rows - 2 ** 16]]
    assert len(rows) > 200
    expO = lp.expected_forward(p)[0][0, 0, rows]
    assert torch.equal(lp._bits_of(lp.emulate(p, 0, rows)), lp._bits_of(expO))
    refused = (lp._bits_of(lp.emulate(p, 0, rows, False, "rows_alias_mod_2^16")) != lp._bits_of(expO)).any(-1)
    assert bool(refused.all())


def test_the_checker_names_the_row_and_its_target():
    p = problem(*MUTANT_SHAPE)
    expO, expL, _ = lp.expected_forward(p)
    lp.check_forward("exact", p, expO.clone(), expL.float())
    row = p["named"]["last key of a middle tile"]
    O = expO.clone()
    O[0, 0, row, 5] = -0.0 if float(O[0, 0, row, 5]) == 0 else 0.0
    with pytest.raises(AssertionError, match=f"row {row} .*targets key {row} .tile {row // 64}, byte {row * 256} "):
        lp.check_forward("one element", p, O, expL.float())
    L = expL.float().clone()
    L[0, 0, row] *= 1.0 + 2.0 ** -19
    with pytest.raises(AssertionError, match="LSE entries outside the bound"):
        lp.check_forward("one LSE", p, expO, L)
