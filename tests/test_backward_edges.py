"""GPU tests of flash_attention_backward off the N(0,1) / scale = 1/sqrt(d) path: the fixed cases of tests/backward_edge_cases.py
(custom scales, a sharp softmax, a common score offset, large and small dO and V, a one-hot P) against float64 autograd with the
per-16-row-block criterion of tests/grad_check.py, the scale through attention(), linearity in dO, dO = 0.  The LSE comes from the
library's own forward with the same scale and mask.  Every case prints its worst error / bound."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import backward_edge_cases as bec  # noqa: E402
import grad_check as gc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(Q, K, V, dO, scale, causal, o_dtype, grad_dtype):
    """forward (O, LSE) and backward on the GPU with the scale passed to both; the gradients as float64 CPU tensors"""
    Qd, Kd, Vd = (t.to(DEV) for t in (Q, K, V))
    O, lse = fa.flash_attention(Qd, Kd, Vd, scale=scale, is_causal=causal, out_dtype=o_dtype, return_lse=True)
    g = fa.flash_attention_backward(Qd, Kd, Vd, O, dO.to(DEV, o_dtype), lse, scale=scale, is_causal=causal, grad_dtype=grad_dtype)
    torch.cuda.synchronize()
    assert all(t.dtype == grad_dtype for t in g)
    return g


@pytest.mark.parametrize("name", [c.name for c in bec.CASES])
def test_case_against_float64(name):
    c = bec.BY_NAME[name]
    Q, K, V, dO, scale = bec.build(c)
    ref, mag = bec.truth(c)
    got = [t.double().cpu() for t in run(Q, K, V, dO, scale, c.causal, c.o_dtype, c.grad_dtype)]
    gc.assert_grads(got, ref, mag, name)


@pytest.mark.parametrize("name", [c.name for c in bec.CASES if c.kind == "scale"])
def test_scale_through_attention(name):
    """attention(..., scale=): the forward and the backward both get it; gradients in the inputs' type"""
    c = bec.BY_NAME[name]
    Q, K, V, dO, scale = bec.build(c)
    ref, mag = bec.truth(c)
    q, k, v = (t.to(DEV).requires_grad_() for t in (Q, K, V))
    fa.attention(q, k, v, is_causal=c.causal, scale=scale, out_dtype=c.o_dtype).backward(dO.to(DEV, c.o_dtype))
    torch.cuda.synchronize()
    gc.assert_grads([t.grad.double().cpu() for t in (q, k, v)], ref, mag, f"attention() {name}")


@pytest.mark.parametrize("name", [c.name for c in bec.CASES if c.kind == "onehot"])
def test_one_hot_rows_leave_dq_and_dk_at_the_cancellation_term(name):
    """P is one-hot to fp32: dQ and dK are zero in exact arithmetic and are held to the `mag` term alone (no share of ||ref||);
    dV is the scatter of dO"""
    c = bec.BY_NAME[name]
    Q, K, V, dO, scale = bec.build(c)
    ref, mag = bec.truth(c)
    assert max(ref[0].abs().max().item(), ref[1].abs().max().item()) < 1e-12
    got = [t.double().cpu() for t in run(Q, K, V, dO, scale, c.causal, c.o_dtype, c.grad_dtype)]
    gc.assert_grads(got, ref, mag, f"{name}, dQ and dK against mag only", rel=(0.0, 0.0, gc.REL))
    keys = torch.tensor([bec.hot_key(q, c.Sk, c.causal) for q in range(c.Sq)])
    scatter = torch.zeros(1, c.H, c.Sk, c.d, dtype=torch.float64).index_add_(2, keys, dO.double())
    assert (gc.reduce_kv(scatter, c.Hkv) - ref[2]).abs().max().item() < 1e-9


@pytest.mark.parametrize("d,heads,causal", [(64, bec.G4, True), (128, bec.MHA, False), (128, bec.MQA, True)])
def test_gradients_are_linear_in_dO(d, heads, causal):
    """backward(a dO) = a backward(dO) for a power of two a (2^13 ~ 1e4, 2^-13 ~ 1e-4), fp32 dO and gradients: every rounding step
    commutes with the factor.  dK and dV are summed in a fixed order: bit equality.  dQ is summed with atomics: the run-to-run
    allowance of tests/test_backward.py.  dO = 0: all three exactly zero."""
    H, Hkv = heads
    g = torch.Generator().manual_seed(97 + d + H)
    Q, dO = (torch.randn((2, H, 700, d), generator=g).bfloat16() for _ in range(2))
    K, V = (torch.randn((2, Hkv, 555, d), generator=g).bfloat16() for _ in range(2))
    Qd, Kd, Vd, dOd = (t.to(DEV) for t in (Q, K, V, dO.float()))
    O, lse = fa.flash_attention(Qd, Kd, Vd, is_causal=causal, out_dtype=torch.float32, return_lse=True)
    base = fa.flash_attention_backward(Qd, Kd, Vd, O, dOd, lse, is_causal=causal)
    for e in (13, -13):
        a = 2.0 ** e
        got = fa.flash_attention_backward(Qd, Kd, Vd, O, dOd * a, lse, is_causal=causal)
        torch.cuda.synchronize()
        assert torch.equal(got[1], base[1] * a) and torch.equal(got[2], base[2] * a), e
        assert (got[0] - base[0] * a).abs().max().item() <= 1e-5 * a * (1 + base[0].abs().max().item()), e
    nan = lambda t: torch.full_like(t, float("nan"))
    zero = fa.flash_attention_backward(Qd, Kd, Vd, O, torch.zeros_like(dOd), lse, is_causal=causal, dQ=nan(base[0]), dK=nan(base[1]),
                                       dV=nan(base[2]))
    torch.cuda.synchronize()
    assert all(bool((t == 0).all()) for t in zero)


@pytest.mark.parametrize("o_dtype,grad_dtype", bec.DTYPES)
def test_zero_dO_gives_zero_gradients_on_sharp_data(o_dtype, grad_dtype):
    c = bec.BY_NAME["sharp12-d128-1000x1000-H8kv2-full-f32-f32"]
    Q, K, V, dO, scale = bec.build(c)
    got = run(Q, K, V, torch.zeros_like(dO), scale, c.causal, o_dtype, grad_dtype)
    assert all(bool((t == 0).all()) for t in got)
