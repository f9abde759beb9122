"""CPU tests of the per-pair probes (tests/weight_probe.py), on every case the GPU tests run (test_probe_forward.py,
test_probe_decode.py, test_probe_backward.py): a float64 emulation of the documented arithmetic stays at or below 0.7 of the probe's
bound, and every float64 mutant -- one key dropped, one pair hidden, one hidden pair shown, one key counted twice, V of two
neighbouring keys exchanged, a length one too long or too short; for the backward the first four on P and on dS -- is at least 4 x the
bound at the element it touches, at the seam of every window.  Conditions, not measurements: a case that misses one gets other data,
not another bound.  No GPU and no kernel: the library is asked for its plans only (plan_ex, decode_plan), like
tests/test_forward_fallbacks.py does."""
import functools

import pytest

torch = pytest.importorskip("torch")

import weight_probe as wp  # noqa: E402


def assert_mutants(found, what, need):
    """found: (mutant, ..., error / bound at its element) tuples; need: the mutants that must have been tried"""
    found = list(found)
    least = {}
    for kind, *where, ratio in found:
        if kind not in least or not ratio >= least[kind][0]:
            least[kind] = (ratio, where)
    print(f"{what}: {len(found)} mutants; least error / bound " + ", ".join(f"{k} {v[0]:.3g}" for k, v in least.items()))
    assert set(need) <= set(least), (what, sorted(least))
    weak = [(k, v) for k, v in least.items() if not v[0] >= wp.MUTANT_AT_LEAST]
    assert not weak, f"{what}: mutants below {wp.MUTANT_AT_LEAST} x the bound: {weak}"


@pytest.mark.parametrize("name", [c.name for c in wp.FORWARD])
def test_forward_probe_admits_the_emulation_and_refuses_every_mutant(name):
    c = wp.FORWARD_BY_NAME[name]
    p = wp.build_forward(c)
    t = wp.forward_truth(c, p)
    assert len(set(p["seams"])) >= min(4, p["Hkv"]) and all(0 <= w <= c.Sk - c.d // 2 for w in p["w0"])
    worst, _ = wp.report(f"emulation of {name}", wp.ratios(wp.forward_emulation(c, p), t["O"], t["bound"]), [p["w0"]], c.H // c.Hkv)
    assert worst <= wp.EMULATION_AT_MOST
    need = set(wp.MUTANTS) - (set() if c.causal else {"pair_shown"})
    assert_mutants(wp.forward_mutants(c, p, t), name, need)


@functools.lru_cache(maxsize=None)
def decode_case(Sq, G, d, fp8):
    return wp.build_decode(Sq, G, d, fp8)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("Sq,G,causal", wp.DEC_SHAPES)
def test_decode_probe_admits_the_emulation_and_refuses_every_mutant(Sq, G, causal, d, fp8):
    p = decode_case(Sq, G, d, fp8)
    t = wp.decode_truth(p, causal)
    what = f"decode Sq {Sq} G {G} d {d} {'fp8' if fp8 else 'bf16'} mask {causal}"
    worst, _ = wp.report(f"emulation of {what}", wp.ratios(wp.decode_emulation(p, causal), t["O"], t["bound"]), p["w0"], G)
    assert worst <= wp.EMULATION_AT_MOST
    need = set(wp.MUTANTS) | {"length + 1", "length - 1"}
    if not causal or Sq == 1:
        need -= {"pair_shown"}
    assert_mutants(wp.decode_mutants(p, t, causal), what, need)


def test_decode_probe_of_the_long_case():
    p = wp.build_decode_long()
    t = wp.decode_truth(p, True)
    worst, _ = wp.report("emulation of the long decode case", wp.ratios(wp.decode_emulation(p, True), t["O"], t["bound"]), p["w0"], p["G"])
    assert worst <= wp.EMULATION_AT_MOST
    assert_mutants(wp.decode_mutants(p, t, True), "long decode case", set(wp.MUTANTS) | {"length + 1", "length - 1"})


def test_split_bounds_follow_the_documented_division():
    assert wp.split_bounds(1024, 3, 128) == [256, 640] and wp.split_bounds(640, 64, 128) == [128, 256, 384, 512]
    assert wp.split_bounds(129, 3, 128) == [128] and wp.split_bounds(128, 64, 128) == [] and wp.split_bounds(1, 3, 128) == []


BWD = [(d, causal, G, shape) for d in (64, 128) for causal in (False, True) for G in (1, 4) for shape in wp.BWD_SHAPES]


@pytest.mark.parametrize("d,causal,G,shape", BWD + [(128, True, 4, "bf16")], ids=lambda v: str(v).replace(" ", ""))
def test_backward_probes_admit_the_emulation_and_refuse_every_mutant(d, causal, G, shape):
    grad_dtype = wp.bf if shape == "bf16" else wp.f32
    Sq, Sk = wp.BWD_SHAPES[0] if shape == "bf16" else shape
    for probe in wp.BWD_PROBES:
        p = wp.build_backward(probe, Sq, Sk, d, G)
        t = wp.backward_truth(probe, p, causal, grad_dtype)
        what = f"{probe} probe d {d} mask {causal} G {G} {Sq} x {Sk} {grad_dtype}"
        worst, _ = wp.backward_report(probe, p, wp.backward_emulation(probe, p, causal, grad_dtype, grad_dtype), t, f"emulation of {what}")
        assert worst <= wp.EMULATION_AT_MOST
        need = {"key_dropped", "pair_hidden", "key_twice"} | ({"pair_shown"} if causal else set())
        assert_mutants(wp.backward_mutants(probe, p, t, causal), what, need)
