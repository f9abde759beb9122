"""GPU: per-pair probes of the forward kernels' softmax weights (tests/weight_probe.py: P through V).  One call per case of
wp.FORWARD -- every kernel family, its route asserted through plan_ex, with and without the mask -- whose heads carry windows over the
case's seams; every element of O is one weight P[q, k] and is held to the fuzz sweep's bound against float64, a hidden pair to exactly
0.0, the LSE to the sweep's LSE bound.  tests/test_weight_probe.py shows on the CPU that the same check admits the documented arithmetic
at <= 0.7 of the bound and refuses one dropped, hidden, shown, doubled or exchanged pair at >= 4 x, for each of these cases."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import weight_probe as wp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def to_device(t, layout):
    """dense [1, H, S, d], or the [1, H, S, d] view of a (1, S, H * d) model-layout buffer"""
    bits = t.view(torch.uint8) if t.dtype == wp.FP8 else t
    if layout == "model":
        bits = bits.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
        assert not bits.is_contiguous()
    else:
        bits = bits.to(DEV)
    return bits.view(wp.FP8) if t.dtype == wp.FP8 else bits


@pytest.mark.parametrize("name", [c.name for c in wp.FORWARD])
def test_every_weight_of_the_windows(name):
    c = wp.FORWARD_BY_NAME[name]
    p = wp.build_forward(c)          # asserts the family
    t = wp.forward_truth(c, p)
    Q, K, V = (to_device(p[n], c.layout) for n in ("Q", "K", "V"))
    res = fa.flash_attention(Q, K, V, is_causal=c.causal, out_dtype=c.odt, return_lse=c.lse, weights_dtype=c.wdt)
    torch.cuda.synchronize()
    O, lse = res if c.lse else (res, None)
    worst, pair = wp.report(f"forward {name} ({c.fam})", wp.ratios(O.double().cpu(), t["O"], t["bound"]), [p["w0"]], c.H // c.Hkv)
    assert worst <= 1.0, f"{name}: pair (batch, head, q, k) = {pair} at {worst:.3g} x the bound"
    if c.lse:
        lr = (lse.double().cpu() - t["lse"]).abs() / t["lse_bound"]
        print(f"forward {name}: worst LSE error / bound {lr.max().item():.3f}")
        assert torch.isfinite(lse).all() and lr.max().item() <= 1.0
