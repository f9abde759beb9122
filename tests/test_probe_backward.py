"""GPU: per-pair probes of the backward kernels' P and dS (tests/weight_probe.py: P through dO into dV, dS through Q into dK, dS
through K into dQ), which the backward recomputes with code of its own.  d in {64, 128}, with and without the mask, MHA and G = 4,
(Sq, Sk) in {(320, 320), (300, 700), (700, 300)}, fp32 O and gradients, and one case in bf16.  Row windows lie over a 32-row slice
seam, the last rows and the rows whose diagonal crosses a wave's 64 keys or a 256-key block (dV and dK then cover EVERY key for those
rows); key windows over keys 64 and 256, the last key and further wave seams (dQ covers every row for those keys).  Every element of
the probed gradient is one pair, held to the element-wise form of grad_check's bound against float64 autograd; hidden pairs to exactly
0.0.  CPU proof of the instrument: tests/test_weight_probe.py."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import weight_probe as wp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(d, causal, G, shape) for d in (64, 128) for causal in (False, True) for G in (1, 4) for shape in wp.BWD_SHAPES]


@pytest.mark.parametrize("d,causal,G,shape", CASES + [(128, True, 4, "bf16")], ids=lambda v: str(v).replace(" ", ""))
def test_every_pair_of_the_windows(d, causal, G, shape):
    dt = wp.bf if shape == "bf16" else wp.f32
    Sq, Sk = wp.BWD_SHAPES[0] if shape == "bf16" else shape
    for probe in wp.BWD_PROBES:
        p = wp.build_backward(probe, Sq, Sk, d, G)
        t = wp.backward_truth(probe, p, causal, dt)
        Q, K, V, dO = p["Q"].to(DEV), p["K"].to(DEV), p["V"].to(DEV), p["dO"].to(dt).to(DEV)
        O, lse = fa.flash_attention(Q, K, V, scale=p["scale"], is_causal=causal, out_dtype=dt, return_lse=True)
        grads = fa.flash_attention_backward(Q, K, V, O, dO, lse, scale=p["scale"], is_causal=causal, grad_dtype=dt)
        torch.cuda.synchronize()
        what = f"backward {probe} probe d {d} mask {causal} G {G} {Sq} x {Sk} {str(dt).split('.')[-1]}"
        worst, pair = wp.backward_report(probe, p, grads[t["index"]].double().cpu(), t, what)
        assert worst <= 1.0, f"{what}: pair (batch, head, q, k) = {pair} at {worst:.3g} x the bound"
