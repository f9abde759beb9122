"""GPU tests of grouped-query attention (K, V with fewer heads than Q; query head h attends K/V head h // G).

Forward: no tolerance.  The reference is this library's own one-K/V-head-per-query-head path on K, V expanded with
repeat_interleave(G, 1) -- the grouped call runs the same kernels on the same values in the same order, so O and the LSE are equal bit
for bit -- on one shape per kernel family the router can choose, the family asserted through plan_ex.

Backward: float64 torch autograd on the CPU of the explicit softmax with K, V expanded inside the graph (autograd sums each group's
gradients), under the acceptance rule of tests/test_backward.py::check_parity, per head and tensor:
    max|g - ref64| <= 2 max|ref_bf16 - ref64| + 1e-5,      relative Frobenius error <= 1e-2 (where the exact gradient is not zero)
"""
import ctypes

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32, FP8 = fa.FA_DTYPE_BF16, fa.FA_DTYPE_F32, fa.FA_DTYPE_FP8_E4M3


def randn(shape, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def expand(t, G):
    """every K/V head G times, consecutively"""
    if t.element_size() == 1:   # fp8: copied as bytes
        return t.view(torch.uint8).repeat_interleave(G, 1).contiguous().view(t.dtype)
    return t.repeat_interleave(G, 1).contiguous()


# ---- forward ---------------------------------------------------------------------------------------------------------------------
from forward_routes import family  # noqa: E402  (the kernel family a call takes, from what plan_ex reports)


# (family, in dtype, out dtype, B, Hq, Hkv, Sq, Sk, d, causal, weights_dtype)
bf, f32, f16 = torch.bfloat16, torch.float32, torch.float16
FORWARD_CASES = [
    ("bf16", bf, f32, 2, 16, 4, 1280, 2048, 128, False, None),             # persistent, no mask: G = 4, Sq != Sk
    ("bf16", bf, bf, 3, 8, 1, 2048, 2048, 64, False, None),                # ... d = 64, MQA (G = 8)
    ("causal_mix", bf, f32, 2, 16, 2, 2048, 2048, 128, True, None),        # S > 1024 under the mask: both precisions in one launch, G = 8
    ("causal_mix", bf, bf, 2, 16, 8, 2304, 2304, 64, True, None),          # ... d = 64, G = 2
    ("f16_weights", bf, f32, 2, 16, 4, 1280, 2048, 128, False, f16),       # FA_FLAG_F16_WEIGHTS
    ("bf16", bf, f32, 2, 16, 8, 2048, 2048, 128, True, bf),                # FA_FLAG_BF16_WEIGHTS under the mask: the bf16 persistent kernel
    ("pair", bf, f32, 1, 4, 2, 512, 512, 64, True, None),                  # pair kernel, d = 64, causal
    ("pair", bf, f32, 2, 4, 1, 300, 700, 128, False, None),                # pair kernel, d = 128, MQA, Sq != Sk
    ("pair", bf, bf, 2, 8, 2, 384, 384, 128, True, None),
    ("bf16_padded", bf, f32, 2, 8, 2, 600, 900, 96, False, None),          # d = 96 zero-padded to 128
    ("bf16_padded", bf, f32, 2, 4, 2, 700, 700, 40, True, None),           # d = 40 zero-padded to 64
    ("fp8", "fp8", bf, 2, 8, 2, 512, 768, 128, False, None),
    ("fp8", "fp8", bf, 1, 8, 4, 600, 600, 64, True, None),
    ("f32", f32, f32, 2, 8, 2, 300, 500, 64, False, None),
    ("f32", f32, f32, 2, 4, 1, 400, 400, 128, True, None),
    ("generic", f32, f32, 2, 4, 2, 100, 150, 256, True, None),
    ("generic", bf, f32, 2, 8, 2, 130, 90, 256, False, None),
]


@pytest.mark.parametrize("case", FORWARD_CASES, ids=lambda c: f"{c[0]}-B{c[3]}H{c[4]}kv{c[5]}S{c[6]}x{c[7]}d{c[8]}{'c' if c[9] else ''}")
def test_forward_is_bitwise_the_mha_call_on_expanded_kv(case):
    fam, idt, odt, B, H, Hkv, Sq, Sk, d, causal, wdt = case
    if idt == "fp8":
        idt = torch.float8_e4m3fn
    G = H // Hkv
    flags = {None: 0, f16: fa.FA_FLAG_F16_WEIGHTS, bf: fa.FA_FLAG_BF16_WEIGHTS}[wdt]
    code = {bf: BF16, f32: F32}.get(idt, FP8)
    assert family(B, H, Sq, Sk, d, causal, code, {bf: BF16, f32: F32}[odt], flags) == fam
    Q = randn((B, H, Sq, d), 1, torch.float32).to(idt).to(DEV)
    K = randn((B, Hkv, Sk, d), 2, torch.float32).to(idt).to(DEV)
    V = randn((B, Hkv, Sk, d), 3, torch.float32).to(idt).to(DEV)
    kw = dict(is_causal=causal, out_dtype=odt, weights_dtype=wdt)
    for want_lse in (True, False):   # (bf16 without the mask: the LSE request selects another normaliser -- both forms)
        got = fa.flash_attention(Q, K, V, return_lse=want_lse, **kw)
        ref = fa.flash_attention(Q, expand(K, G), expand(V, G), return_lse=want_lse, **kw)
        torch.cuda.synchronize()
        if want_lse:
            assert torch.isfinite(got[1]).all() and torch.equal(got[1], ref[1])
            got, ref = got[0], ref[0]
        assert torch.isfinite(got.float()).all() and torch.equal(got, ref)
    # the group's heads do differ (the test would pass on a kernel that ignored h otherwise only by luck of equal Q)
    assert not torch.equal(got[:, 0], got[:, 1])


def test_forward_strided_model_layout_views():
    """Q and O as views of (B, S, H*d) buffers, K and V of (B, Sk, Hkv*d) buffers"""
    B, Sq, Sk, H, Hkv, d = 2, 1280, 1500, 16, 4, 128
    G = H // Hkv
    view = lambda t, h: t.view(B, -1, h, d).transpose(1, 2)
    Qm, Km, Vm = randn((B, Sq, H * d), 11).to(DEV), randn((B, Sk, Hkv * d), 12).to(DEV), randn((B, Sk, Hkv * d), 13).to(DEV)
    Om = torch.empty(B, Sq, H * d, device=DEV, dtype=torch.float32)
    assert family(B, H, Sq, Sk, d, True, BF16, F32, 0) == "causal_mix"
    O, lse = fa.flash_attention(view(Qm, H), view(Km, Hkv), view(Vm, Hkv), view(Om, H), is_causal=True, return_lse=True)
    Or, lser = fa.flash_attention(view(Qm, H).contiguous(), expand(view(Km, Hkv), G), expand(view(Vm, Hkv), G), is_causal=True,
                                  out_dtype=torch.float32, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(O, Or) and torch.equal(lse, lser) and O.data_ptr() == Om.data_ptr()


@pytest.mark.parametrize("causal", [False, True])
def test_gqa_entry_point_with_equal_head_counts_is_flash_attention_ex(causal):
    B, H, Sq, Sk, d = 2, 8, 700, 900, 128
    Q, K, V = randn((B, H, Sq, d), 21).to(DEV), randn((B, H, Sk, d), 22).to(DEV), randn((B, H, Sk, d), 23).to(DEV)
    L = fa.lib()
    out = []
    for gqa in (False, True):
        O = torch.full((B, H, Sq, d), float("nan"), device=DEV)
        lse = torch.full((B, H, Sq), float("nan"), device=DEV)
        head = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), lse.data_ptr(), B, H)
        tail = (Sq, Sk, d, 1 / d ** 0.5, causal, BF16, F32, None, None, None, None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        rc = L.flash_attention_gqa(*head, H, *tail) if gqa else L.flash_attention_ex(*head, *tail)
        assert rc == 0
        torch.cuda.synchronize()
        out.append((O, lse))
    assert torch.isfinite(out[0][0]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- backward --------------------------------------------------------------------------------------------------------------------
def explicit_attention(Q, K, V, scale, causal):
    S = (Q @ K.transpose(-1, -2)) * scale
    if causal:
        Sq, Sk = S.shape[-2:]
        hidden = torch.arange(Sk)[None, :] > torch.arange(Sq)[:, None]
        S = S.masked_fill(hidden, float("-inf"))
    return torch.softmax(S, dim=-1) @ V


def cpu_grads(Q, K, V, dO, scale, causal, dtype):
    """torch autograd on the CPU of the explicit softmax(QK^T scale)V in `dtype` with K, V expanded inside the graph: dK, dV come
    back per K/V head, each group's sum taken by autograd"""
    G = Q.shape[1] // K.shape[1]
    q, k, v = (t.to(dtype).requires_grad_() for t in (Q, K, V))
    explicit_attention(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), scale, causal).backward(dO.to(dtype))
    return [t.grad.double() for t in (q, k, v)]


def run(Q, K, V, dO, causal, o_dtype, grad_dtype):
    Qd, Kd, Vd = (t.to(DEV) for t in (Q, K, V))
    O, lse = fa.flash_attention(Qd, Kd, Vd, is_causal=causal, out_dtype=o_dtype, return_lse=True)
    nan = lambda t: torch.full(t.shape, float("nan"), device=DEV, dtype=grad_dtype)
    g = fa.flash_attention_backward(Qd, Kd, Vd, O, dO.to(DEV, o_dtype), lse, is_causal=causal, dQ=nan(Q), dK=nan(K), dV=nan(V))
    torch.cuda.synchronize()
    return [x.double().cpu() for x in g]


def assert_within_rule(ours, ref, bfr):
    """the acceptance rule of tests/test_backward.py::check_parity, per head and tensor"""
    for name, g, r, b in zip(("dQ", "dK", "dV"), ours, ref, bfr):
        assert g.shape == r.shape, name
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


def check_parity(Q, K, V, dO, causal, o_dtype, grad_dtype):
    scale = 1.0 / Q.shape[-1] ** 0.5
    ours = run(Q, K, V, dO, causal, o_dtype, grad_dtype)
    assert_within_rule(ours, cpu_grads(Q, K, V, dO, scale, causal, torch.float64), cpu_grads(Q, K, V, dO, scale, causal, torch.bfloat16))
    if causal and K.shape[2] > Q.shape[2]:   # keys no query sees: exactly zero (and written: the outputs were NaN)
        Sq = Q.shape[2]
        assert (ours[1][:, :, Sq:] == 0).all() and (ours[2][:, :, Sq:] == 0).all()


SHAPES = [(1, 1), (77, 77), (320, 320), (1000, 1000), (128, 700), (700, 128), (4096, 4096)]
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16),
          (torch.bfloat16, torch.float32)]
GROUPS = [(8, 4), (8, 2), (8, 1)]    # (Hq, Hkv): G = 2, G = 4, MQA


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_backward_parity_sweep(d, causal, si):
    Sq, Sk = SHAPES[si]
    o_dtype, grad_dtype = DTYPES[(si + 2 * causal + (d == 128)) % 4]     # every (O / dO, gradient) type pair on every d and mask
    H, Hkv = GROUPS[(si + causal + 2 * (d == 128)) % 3]                  # ... and every group size
    if Sq * Sk > 10 ** 6:
        H, Hkv = 2, 1                                                    # (the CPU references take (Sq x Sk) float64 matrices per head)
    B = 2 if Sq * Sk < 10 ** 6 else 1
    seed = 1000 * si + 10 * d + causal
    Q, K, V = randn((B, H, Sq, d), seed), randn((B, Hkv, Sk, d), seed + 1), randn((B, Hkv, Sk, d), seed + 2)
    dO = randn((B, H, Sq, d), seed + 3)
    check_parity(Q, K, V, dO, causal, o_dtype, grad_dtype)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("o_dtype,grad_dtype", DTYPES)
@pytest.mark.parametrize("H,Hkv", [(4, 2), (4, 1)])
def test_backward_parity_all_dtype_pairs(d, causal, o_dtype, grad_dtype, H, Hkv):
    Q, dO = randn((2, H, 320, d), 77), randn((2, H, 320, d), 78)
    K, V = randn((2, Hkv, 320, d), 79), randn((2, Hkv, 320, d), 80)
    check_parity(Q, K, V, dO, causal, o_dtype, grad_dtype)


@pytest.mark.parametrize("B,H,Hkv,Sq,Sk,d,causal", [(1, 8, 2, 320, 320, 64, True), (2, 8, 1, 300, 700, 128, False),
                                                     (1, 6, 2, 1000, 1000, 128, True), (1, 4, 2, 77, 77, 64, False)])
def test_backward_parity_on_the_stated_shapes(B, H, Hkv, Sq, Sk, d, causal):
    Q, dO = randn((B, H, Sq, d), 301), randn((B, H, Sq, d), 302)
    K, V = randn((B, Hkv, Sk, d), 303), randn((B, Hkv, Sk, d), 304)
    check_parity(Q, K, V, dO, causal, torch.float32, torch.float32)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(100, 700), (300, 1000), (1, 513)])
def test_backward_writes_every_element_and_zeroes_unseen_keys(d, Sq, Sk):
    B, H, Hkv = 2, 6, 2
    Q, dO = randn((B, H, Sq, d), 5), randn((B, H, Sq, d), 6)
    K, V = randn((B, Hkv, Sk, d), 7), randn((B, Hkv, Sk, d), 8)
    Qd, Kd, Vd = (t.to(DEV) for t in (Q, K, V))
    for causal in (False, True):
        O, lse = fa.flash_attention(Qd, Kd, Vd, is_causal=causal, out_dtype=torch.float32, return_lse=True)
        dQ = torch.full((B, H, Sq, d), float("nan"), device=DEV)
        dK = torch.full((B, Hkv, Sk, d), float("nan"), device=DEV)
        dV = torch.full((B, Hkv, Sk, d), float("nan"), device=DEV)
        fa.flash_attention_backward(Qd, Kd, Vd, O, dO.float().to(DEV), lse, is_causal=causal, dQ=dQ, dK=dK, dV=dV)
        torch.cuda.synchronize()
        for t in (dQ, dK, dV):
            assert torch.isfinite(t).all()
        if causal:   # keys k >= Sq are seen by no query: exactly zero
            assert (dK[:, :, Sq:] == 0).all() and (dV[:, :, Sq:] == 0).all()
            assert (dV[:, :, :Sq].abs().sum() > 0)


@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_backward_dk_dv_are_deterministic(H, Hkv):
    Q, dO = randn((2, H, 1500, 128), 31).to(DEV), randn((2, H, 1500, 128), 32).to(DEV)
    K, V = randn((2, Hkv, 1500, 128), 33).to(DEV), randn((2, Hkv, 1500, 128), 34).to(DEV)
    for causal in (False, True):
        O, lse = fa.flash_attention(Q, K, V, is_causal=causal, out_dtype=torch.float32, return_lse=True)
        a = fa.flash_attention_backward(Q, K, V, O, dO.float(), lse, is_causal=causal)
        b = fa.flash_attention_backward(Q, K, V, O, dO.float(), lse, is_causal=causal)
        torch.cuda.synchronize()
        assert a[1].shape == K.shape and a[2].shape == V.shape
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert (a[0] - b[0]).abs().max().item() <= 1e-5 * (1 + a[0].abs().max().item())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_backward_is_the_group_sum_of_the_expanded_mha_backward(d, causal):
    """fp32 gradients: both are fp32 sums of the same bf16 products in a different association"""
    B, H, Hkv, Sq, Sk = 2, 8, 2, 600, 900
    G = H // Hkv
    Q, dO = randn((B, H, Sq, d), 41).to(DEV), randn((B, H, Sq, d), 42).to(DEV).float()
    K, V = randn((B, Hkv, Sk, d), 43).to(DEV), randn((B, Hkv, Sk, d), 44).to(DEV)
    O, lse = fa.flash_attention(Q, K, V, is_causal=causal, out_dtype=torch.float32, return_lse=True)
    dQ, dK, dV = fa.flash_attention_backward(Q, K, V, O, dO, lse, is_causal=causal)
    Ke, Ve = expand(K, G), expand(V, G)
    Oe, lsee = fa.flash_attention(Q, Ke, Ve, is_causal=causal, out_dtype=torch.float32, return_lse=True)
    dQe, dKe, dVe = fa.flash_attention_backward(Q, Ke, Ve, Oe, dO, lsee, is_causal=causal)
    torch.cuda.synchronize()
    assert torch.equal(O, Oe) and torch.equal(lse, lsee)
    group_sum = lambda t: t.view(B, Hkv, G, Sk, d).sum(2)
    for g, r in ((dK, group_sum(dKe)), (dV, group_sum(dVe)), (dQ, dQe)):
        assert (g - r).abs().max().item() <= 1e-5 * (1 + r.abs().max().item())


def test_backward_strided_views():
    """Q, O, dO, dQ as views of (B, S, H*d) buffers, K, V, dK, dV of (B, Sk, Hkv*d) buffers (the model layout)"""
    B, Sq, Sk, H, Hkv, d = 2, 300, 420, 8, 2, 64
    view = lambda t, h: t.view(B, -1, h, d).transpose(1, 2)
    Qm, dOm = randn((B, Sq, H * d), 900), randn((B, Sq, H * d), 901)
    Km, Vm = randn((B, Sk, Hkv * d), 902), randn((B, Sk, Hkv * d), 903)
    Q, dO, K, V = view(Qm.to(DEV), H), view(dOm.to(DEV), H), view(Km.to(DEV), Hkv), view(Vm.to(DEV), Hkv)
    O = view(torch.empty(B, Sq, H * d, device=DEV, dtype=torch.float32), H)
    _, lse = fa.flash_attention(Q, K, V, O, is_causal=True, return_lse=True)
    dQ = view(torch.full((B, Sq, H * d), float("nan"), device=DEV), H)
    dK, dV = (view(torch.full((B, Sk, Hkv * d), float("nan"), device=DEV), Hkv) for _ in range(2))
    fa.flash_attention_backward(Q, K, V, O, dO.float(), lse, is_causal=True, dQ=dQ, dK=dK, dV=dV)
    torch.cuda.synchronize()
    dense_in = [view(Qm, H).contiguous(), view(Km, Hkv).contiguous(), view(Vm, Hkv).contiguous(), view(dOm, H).contiguous()]
    dense = run(*dense_in, True, torch.float32, torch.float32)
    for g, r in zip((dQ, dK, dV), dense):
        assert (g.double().cpu() - r).abs().max().item() <= 1e-5 * (1 + r.abs().max().item())
    ours = [g.double().cpu() for g in (dQ, dK, dV)]
    assert_within_rule(ours, cpu_grads(*dense_in, 1 / d ** 0.5, True, torch.float64), cpu_grads(*dense_in, 1 / d ** 0.5, True, torch.bfloat16))


def test_graph_capture_of_forward_and_backward_replays_equal_to_eager():
    Q, dO = randn((2, 8, 700, 64), 51).to(DEV), randn((2, 8, 700, 64), 52).to(DEV).float()
    K, V = randn((2, 2, 700, 64), 53).to(DEV), randn((2, 2, 700, 64), 54).to(DEV)

    def step():
        O, lse = fa.flash_attention(Q, K, V, is_causal=True, out_dtype=torch.float32, return_lse=True)
        return fa.flash_attention_backward(Q, K, V, O, dO, lse, is_causal=True)

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
    assert out[1].shape == K.shape
    assert torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2])
    assert (out[0] - eager[0]).abs().max().item() <= 1e-5 * (1 + eager[0].abs().max().item())


@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_attention_autograd_through_a_grouped_call(H, Hkv):
    B, Sq, Sk, d = 2, 333, 400, 128
    Q, dO = randn((B, H, Sq, d), 61), randn((B, H, Sq, d), 62)
    K, V = randn((B, Hkv, Sk, d), 63), randn((B, Hkv, Sk, d), 64)
    q, k, v = (t.to(DEV).requires_grad_() for t in (Q, K, V))
    O = fa.attention(q, k, v, is_causal=True, out_dtype=torch.float32)
    O.backward(dO.to(DEV).float())
    torch.cuda.synchronize()
    assert q.grad.shape == Q.shape and k.grad.shape == K.shape and v.grad.shape == V.shape and k.grad.dtype == torch.bfloat16
    ours = [t.grad.double().cpu() for t in (q, k, v)]
    scale = 1 / d ** 0.5
    assert_within_rule(ours, cpu_grads(Q, K, V, dO, scale, True, torch.float64), cpu_grads(Q, K, V, dO, scale, True, torch.bfloat16))
    # ... and it is the direct call
    O2, lse = fa.flash_attention(q.detach(), k.detach(), v.detach(), is_causal=True, out_dtype=torch.float32, return_lse=True)
    _, dK, dV = fa.flash_attention_backward(q.detach(), k.detach(), v.detach(), O2, dO.to(DEV).float(), lse, is_causal=True)
    torch.cuda.synchronize()
    assert torch.equal(O.detach(), O2) and torch.equal(k.grad, dK.to(torch.bfloat16)) and torch.equal(v.grad, dV.to(torch.bfloat16))


def test_mismatched_head_counts_still_raise():
    q = torch.zeros(2, 8, 16, 64, dtype=torch.bfloat16, device=DEV)
    for shape in ((2, 3, 16, 64), (2, 16, 16, 64), (1, 2, 16, 64), (2, 2, 16, 128)):
        k = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError):
            fa.flash_attention(q, k, k)
        with pytest.raises(ValueError):
            fa.attention(q, k, k)
