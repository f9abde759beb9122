"""CPU tests of the gradient checker (tests/grad_check.py) on the cases of tests/backward_edge_cases.py: a float64 emulation of the
documented backward arithmetic passes on every case, and each of five deliberately wrong gradients fails on at least one -- so the
bound admits the documented arithmetic and nothing grossly wrong.  No GPU, no library."""
import pytest

torch = pytest.importorskip("torch")

import backward_edge_cases as bec  # noqa: E402
import grad_check as gc  # noqa: E402


@pytest.mark.parametrize("name", [c.name for c in bec.CASES])
def test_the_documented_arithmetic_passes(name):
    c = bec.BY_NAME[name]
    Q, K, V, dO, scale = bec.build(c)
    ref, mag = bec.truth(c)
    got = gc.emulate(Q, K, V, dO, scale, c.causal, c.o_dtype, c.grad_dtype)
    gc.assert_grads(got, ref, mag, f"emulation of {name}")


def test_the_manual_formulas_equal_autograd():
    c = bec.BY_NAME["scalesmall-d128-128x700-H8kv2-full-bf16-bf16"]
    Q, K, V, dO, scale = bec.build(c)
    ref, _ = bec.truth(c)
    for g, r in zip(gc.exact(Q, K, V, dO, scale, c.causal), ref):
        assert (g - r).abs().max().item() <= 1e-12 * (1 + r.abs().max().item())


# one case per distinct data set, the 2048 x 2048 ones left out (the controls need no large case to be caught)
CONTROL_CASES = [c for c in {bec._data_key(c): c for c in reversed(bec.CASES)}.values() if c.Sq * c.Sk <= 10 ** 6][::-1]


def test_every_wrong_answer_is_caught_somewhere():
    caught = {name: [] for name in gc.CONTROLS}
    for c in CONTROL_CASES:
        Q, K, V, dO, scale = bec.build(c)
        ref, mag = bec.truth(c)
        for name, wrong in gc.CONTROLS.items():
            worst, failures = gc.check(wrong(Q, K, V, dO, scale, c.causal), ref, mag)
            if failures:
                caught[name].append(f"{c.name} ({max(worst.values()):.3g})")
    for name, cases in caught.items():
        print(f"control '{name}' is caught by {len(cases)} of {len(CONTROL_CASES)} cases (worst error / bound): {', '.join(cases) or 'none'}")
    assert all(caught.values()), {k: len(v) for k, v in caught.items()}


def test_the_checker_sees_one_wrong_block_and_non_finite_values():
    """one 16-row block of one head off by a quarter is caught and located; NaN is a failure"""
    c = bec.BY_NAME["scalesmall-d64-320x320-H2kv2-causal-f32-f32"]
    ref, mag = bec.truth(c)
    assert not gc.check(ref, ref, mag)[1]
    bad = [t.clone() for t in ref]
    bad[2][0, 1, 160:176] *= 1.25
    worst, failures = gc.check(bad, ref, mag)
    assert len(failures) == 1 and failures[0].startswith("dV: 1 of") and "head 1 rows [160, 176)" in failures[0]
    bad = [t.clone() for t in ref]
    bad[0][0, 0, 5, 7] = float("nan")
    assert gc.check(bad, ref, mag)[1]
