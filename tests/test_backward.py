"""GPU tests of flash_attention_backward and the differentiable attention(): parity with float64 autograd on the CPU, the mask,
coverage of every output element, determinism of dK / dV, graph capture and the autograd path."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def randn(shape, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def explicit_attention(Q, K, V, scale, causal):
    S = (Q @ K.transpose(-1, -2)) * scale
    if causal:
        Sq, Sk = S.shape[-2:]
        hidden = torch.arange(Sk)[None, :] > torch.arange(Sq)[:, None]
        S = S.masked_fill(hidden, float("-inf"))
    return torch.softmax(S, dim=-1) @ V


def cpu_grads(Q, K, V, dO, scale, causal, dtype):
    """torch autograd on the CPU of the explicit softmax(QK^T scale)V in `dtype`, on the given (bf16-valued) tensors."""
    q, k, v = (t.to(dtype).requires_grad_() for t in (Q, K, V))
    explicit_attention(q, k, v, scale, causal).backward(dO.to(dtype))
    return [t.grad.double() for t in (q, k, v)]


def run(Q, K, V, dO, causal, o_dtype, grad_dtype, scale=None):
    """forward (LSE) + backward on the GPU; dO is bf16-valued, passed in o_dtype"""
    Qd, Kd, Vd = (t.to(DEV) for t in (Q, K, V))
    O, lse = fa.flash_attention(Qd, Kd, Vd, scale=scale, is_causal=causal, out_dtype=o_dtype, return_lse=True)
    g = fa.flash_attention_backward(Qd, Kd, Vd, O, dO.to(DEV, o_dtype), lse, scale=scale, is_causal=causal, grad_dtype=grad_dtype)
    torch.cuda.synchronize()
    return [x.double().cpu() for x in g]


def check_parity(Q, K, V, dO, causal, o_dtype, grad_dtype):
    d = Q.shape[-1]
    scale = 1.0 / d ** 0.5
    ours = run(Q, K, V, dO, causal, o_dtype, grad_dtype)
    ref = cpu_grads(Q, K, V, dO, scale, causal, torch.float64)
    bf = cpu_grads(Q, K, V, dO, scale, causal, torch.bfloat16)
    margins, rels = [], [0.0]
    for name, g, r, b in zip(("dQ", "dK", "dV"), ours, ref, bf):
        assert torch.isfinite(g).all(), name
        for bh in range(g.shape[0] * g.shape[1]):
            gi, ri, bi = (x.reshape(-1, *x.shape[2:])[bh] for x in (g, r, b))
            err = (gi - ri).abs().max().item()
            bound = 2 * (bi - ri).abs().max().item() + 1e-5
            assert err <= bound, f"{name} head {bh}: max err {err:.3e} > bound {bound:.3e}"
            rn = ri.norm().item()
            # a gradient that is zero in exact arithmetic (one visible key: the softmax is constant) has no relative error
            if rn > 1e-3 * ri.numel() ** 0.5:
                rel = (gi - ri).norm().item() / rn
                assert rel <= 1e-2, f"{name} head {bh}: relative Frobenius error {rel:.3e}"
                rels.append(rel)
            margins.append(err / bound)
    return max(margins), max(rels)     # the worst max|g - ref| / bound and relative Frobenius error over the three tensors


SHAPES = [(1, 1), (77, 77), (320, 320), (1000, 1000), (128, 700), (700, 128), (4096, 4096)]
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16),
          (torch.bfloat16, torch.float32)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_backward_parity_sweep(d, causal, si):
    Sq, Sk = SHAPES[si]
    o_dtype, grad_dtype = DTYPES[(si + 2 * causal + (d == 128)) % 4]     # every (O / dO, gradient) type pair on every d and mask
    H = 1 if Sq * Sk > 10 ** 6 else 2
    seed = 1000 * si + 10 * d + causal
    Q, K, V = randn((1, H, Sq, d), seed), randn((1, H, Sk, d), seed + 1), randn((1, H, Sk, d), seed + 2)
    dO = randn((1, H, Sq, d), seed + 3)
    check_parity(Q, K, V, dO, causal, o_dtype, grad_dtype)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("o_dtype,grad_dtype", DTYPES)
def test_backward_parity_all_dtype_pairs(d, causal, o_dtype, grad_dtype):
    Q, K, V, dO = (randn((2, 2, 320, d), 77 + i) for i in range(4))
    check_parity(Q, K, V, dO, causal, o_dtype, grad_dtype)


def test_backward_strided_views():
    """Q, K, V, O, dO and the gradients as views of (B, S, H*d) buffers (the model layout)"""
    B, S, H, d = 2, 300, 4, 64
    view = lambda t: t.view(B, S, H, d).transpose(1, 2)
    Qm, Km, Vm, dOm = (randn((B, S, H * d), 900 + i) for i in range(4))
    Q, K, V, dO = (view(t.to(DEV)) for t in (Qm, Km, Vm, dOm))
    O = view(torch.empty(B, S, H * d, device=DEV, dtype=torch.float32))
    _, lse = fa.flash_attention(Q, K, V, O, is_causal=True, return_lse=True)
    dQ, dK, dV = (view(torch.empty(B, S, H * d, device=DEV, dtype=torch.float32)) for _ in range(3))
    fa.flash_attention_backward(Q, K, V, O, dO.float(), lse, is_causal=True, dQ=dQ, dK=dK, dV=dV)
    torch.cuda.synchronize()
    dense = run(*(view(t).contiguous() for t in (Qm, Km, Vm)), view(dOm).contiguous(), True, torch.float32, torch.float32)
    for g, r in zip((dQ, dK, dV), dense):
        assert (g.double().cpu() - r).abs().max().item() <= 1e-5 * (1 + r.abs().max().item())
    ref = cpu_grads(*(view(t).contiguous() for t in (Qm, Km, Vm)), view(dOm).contiguous(), 1 / d ** 0.5, True, torch.float64)
    for g, r in zip((dQ, dK, dV), ref):
        assert (g.double().cpu() - r).norm().item() <= 1e-2 * r.norm().item()


def test_backward_large_causal_shape():
    """B 8, H 16, S 4096, d 128, causal: float64 on two sampled heads, and two identities on every head"""
    B, H, S, d = 8, 16, 4096, 128
    Q, K, V, dO = (randn((B, H, S, d), 4242 + i).to(DEV) for i in range(4))
    O, lse = fa.flash_attention(Q, K, V, is_causal=True, out_dtype=torch.float32, return_lse=True)
    dQ, dK, dV = fa.flash_attention_backward(Q, K, V, O, dO.float(), lse, is_causal=True, grad_dtype=torch.float32)
    torch.cuda.synchronize()
    for t in (dQ, dK, dV):
        assert torch.isfinite(t).all()
    # sum_k dV[k] = sum_q (sum_k P[q,k]) dO[q] = sum_q dO[q]: exact but for the bf16 rounding of P (relative 2^-9 per weight; a
    # row's weights sum to 1 within ~2^-9), so the bound is 2^-8 of sum_q |dO|
    lhs, rhs = dO.double().sum(2), dV.double().sum(2)
    assert ((lhs - rhs).abs() <= 2 ** -8 * dO.double().abs().sum(2) + 1e-4).all()
    # sum dQ * Q = scale sum_{q,k} dS[q,k] <Q[q], K[k]> = sum dK * K: both from the same bf16 dS, so fp32 accumulation only
    a = (dQ.double() * Q.double()).sum((2, 3))
    b = (dK.double() * K.double()).sum((2, 3))
    scale_ = (dQ.double().abs() * Q.double().abs()).sum((2, 3))
    assert ((a - b).abs() <= 1e-4 * scale_ + 1e-4).all()
    for bh in (5, 117):
        b_, h_ = divmod(bh, H)
        sl = lambda t: t[b_:b_ + 1, h_:h_ + 1].cpu()
        ref = cpu_grads(sl(Q), sl(K), sl(V), sl(dO), 1 / d ** 0.5, True, torch.float64)
        for g, r in zip((dQ, dK, dV), ref):
            assert (sl(g).double() - r).norm().item() <= 1e-2 * r.norm().item()


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(100, 700), (300, 1000), (1, 513)])
def test_backward_writes_every_element_and_zeroes_unseen_keys(d, Sq, Sk):
    Q, dO = randn((2, 3, Sq, d), 5), randn((2, 3, Sq, d), 6)
    K, V = randn((2, 3, Sk, d), 7), randn((2, 3, Sk, d), 8)
    Qd, Kd, Vd = (t.to(DEV) for t in (Q, K, V))
    for causal in (False, True):
        O, lse = fa.flash_attention(Qd, Kd, Vd, is_causal=causal, out_dtype=torch.float32, return_lse=True)
        dQ = torch.full((2, 3, Sq, d), float("nan"), device=DEV)
        dK = torch.full((2, 3, Sk, d), float("nan"), device=DEV)
        dV = torch.full((2, 3, Sk, d), float("nan"), device=DEV)
        fa.flash_attention_backward(Qd, Kd, Vd, O, dO.float().to(DEV), lse, is_causal=causal, dQ=dQ, dK=dK, dV=dV)
        torch.cuda.synchronize()
        for t in (dQ, dK, dV):
            assert torch.isfinite(t).all()
        if causal:   # keys k >= Sq are seen by no query: exactly zero
            assert (dK[:, :, Sq:] == 0).all() and (dV[:, :, Sq:] == 0).all()
            assert (dV[:, :, :Sq].abs().sum() > 0)


def test_backward_dk_dv_are_deterministic():
    Q, K, V, dO = (randn((2, 4, 1500, 128), 31 + i).to(DEV) for i in range(4))
    for causal in (False, True):
        O, lse = fa.flash_attention(Q, K, V, is_causal=causal, out_dtype=torch.float32, return_lse=True)
        a = fa.flash_attention_backward(Q, K, V, O, dO.float(), lse, is_causal=causal)
        b = fa.flash_attention_backward(Q, K, V, O, dO.float(), lse, is_causal=causal)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert (a[0] - b[0]).abs().max().item() <= 1e-5 * (1 + a[0].abs().max().item())


def test_backward_graph_capture_replays_equal_to_eager():
    Q, K, V, dO = (randn((2, 4, 700, 64), 51 + i).to(DEV) for i in range(4))
    dOf = dO.float()

    def step():
        O, lse = fa.flash_attention(Q, K, V, is_causal=True, out_dtype=torch.float32, return_lse=True)
        return fa.flash_attention_backward(Q, K, V, O, dOf, lse, is_causal=True)

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step()                                   # warm-up on the side stream (the LDS limits are raised outside the capture)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2])
    assert (out[0] - eager[0]).abs().max().item() <= 1e-5 * (1 + eager[0].abs().max().item())


def test_backward_on_a_side_stream_keeps_its_workspace():
    """stream=: the kernels run on a side stream while the current stream goes on allocating blocks of the workspace's size and
    overwriting them; the workspace released at return must not be one of them while the kernels still use it"""
    B, H, S, d = 4, 16, 2048, 128
    Q, K, V, dO = (randn((B, H, S, d), 71 + i).to(DEV) for i in range(4))
    O, lse = fa.flash_attention(Q, K, V, out_dtype=torch.float32, return_lse=True)
    dOf = dO.float()
    ref = fa.flash_attention_backward(Q, K, V, O, dOf, lse)
    torch.cuda.synchronize()
    n = fa.backward_workspace_size(B, H, S, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        got = fa.flash_attention_backward(Q, K, V, O, dOf, lse, stream=side)
        junk = [torch.full((n,), 255, dtype=torch.uint8, device=DEV) for _ in range(4)]   # NaN bytes, on the current stream
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
        assert torch.isfinite(got[0]).all()
        assert (got[0] - ref[0]).abs().max().item() <= 1e-5 * (1 + ref[0].abs().max().item())
        del junk, got


def test_attention_autograd_matches_the_direct_call():
    Q, K, V, dO = (randn((2, 2, 333, 128), 61 + i).to(DEV) for i in range(4))
    q, k, v = (t.clone().requires_grad_() for t in (Q, K, V))
    O = fa.attention(q, k, v, is_causal=True, out_dtype=torch.float32)
    O.backward(dO.float())
    O2, lse = fa.flash_attention(Q, K, V, is_causal=True, out_dtype=torch.float32, return_lse=True)
    dQ, dK, dV = fa.flash_attention_backward(Q, K, V, O2, dO.float(), lse, is_causal=True)
    torch.cuda.synchronize()
    assert torch.equal(O.detach(), O2)
    assert torch.equal(k.grad, dK.to(torch.bfloat16)) and torch.equal(v.grad, dV.to(torch.bfloat16))
    assert (q.grad.float() - dQ).abs().max().item() <= 1e-2 * (1 + dQ.abs().max().item())
