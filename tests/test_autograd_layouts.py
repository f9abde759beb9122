"""GPU tests of attention() inside real losses: autograd hands _Attention.backward whatever view of dO the loss produced -- expanded
(strideS = 0, or every stride 0), narrowed out of a wider buffer (row stride d + k), transposed (the model layout) -- and q.grad,
k.grad, v.grad must equal float64 autograd of the same loss on the explicit formula (the criterion of tests/grad_check.py).
Each test also asserts the layout it is about really reached the wrapper, and which layouts go to the library uncopied."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import grad_check as gc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, SQ, SK = 2, 300, 500
# (H, Hkv, d, causal)
HEADS = {"mha": (4, 4, 64, False), "gqa": (8, 2, 128, True)}
KINDS = ["sum_over_seq", "sum", "cat_k8", "cat_k3", "model_layout", "other_dtype"]


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def extras(kind, H, d):
    """the loss's own constants (float32 CPU tensors)"""
    if kind.startswith("cat"):
        k = int(kind[5:])
        return {"x": randn((B, H, SQ, k), 11), "W": randn((d + k, 24), 12) / (d + k) ** 0.5}
    if kind == "model_layout":
        return {"W": randn((H * d, 40), 13) / (H * d) ** 0.5}
    if kind == "other_dtype":
        return {"W": randn((B, H, SQ, d), 14)}
    return {}


def loss_of(kind, O, ex, work):
    """the loss on O (the GPU's O in its own type, or the float64 reference); `work`: the type the loss itself is computed in"""
    if kind == "sum_over_seq":
        return O.sum(dim=2).to(work).square().sum()             # dO: expanded over the rows, strides (H d, d, 0, 1)
    if kind == "sum":
        return O.sum().to(work)                                 # dO: one value expanded, every stride 0
    if kind.startswith("cat"):
        return (torch.cat([O, ex["x"].to(O.dtype)], -1).to(work) @ ex["W"].to(work)).square().sum()   # dO: row stride d + k
    if kind == "model_layout":
        return (O.transpose(1, 2).reshape(B, SQ, -1).to(work) @ ex["W"].to(work)).square().sum()      # dO: a [B, S, H d] buffer
    if kind == "other_dtype":
        return (O.to(work) * ex["W"].to(work)).sum()            # an fp32 loss on a bf16 O (fp64 on an fp32 O)
    raise KeyError(kind)


def expected_layout(kind, dO, H, d):
    """(the view of dO the loss must have produced, whether the wrapper must copy it before the library sees it)"""
    esz, st = dO.element_size(), dO.stride()
    if kind == "sum_over_seq":
        return st == (H * d, d, 0, 1), True
    if kind == "sum":
        return st == (0, 0, 0, 0), True
    if kind.startswith("cat"):
        k = int(kind[5:])
        return st[2] == d + k and st[3] == 1, ((d + k) * esz) % 16 != 0
    if kind == "model_layout":
        return st == (SQ * H * d, d, H * d, 1), False
    return dO.is_contiguous(), False


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("heads", list(HEADS))
@pytest.mark.parametrize("kind", KINDS)
def test_loss_gradients_against_float64(kind, heads, out_dtype, monkeypatch):
    H, Hkv, d, causal = HEADS[heads]
    scale = 1.0 / d ** 0.5
    Q, K, V = randn((B, H, SQ, d), 1).bfloat16(), randn((B, Hkv, SK, d), 2).bfloat16(), randn((B, Hkv, SK, d), 3).bfloat16()
    ex = extras(kind, H, d)
    ref, dO64 = gc.reference_grads(Q, K, V, scale, causal, loss=lambda O: loss_of(kind, O, ex, torch.float64))
    mag = gc.magnitudes(Q, K, V, dO64, scale, causal)

    seen = {}
    inner = fa.flash_attention_backward

    def spy(Q_, K_, V_, O_, dO_, *a, **kw):
        seen["given"] = dO_
        return inner(Q_, K_, V_, O_, dO_, *a, **kw)

    real_accepts = fa._library_accepts

    def spy_accepts(t):
        seen["arrived"] = t
        return real_accepts(t)

    monkeypatch.setattr(fa, "flash_attention_backward", spy)
    monkeypatch.setattr(fa, "_library_accepts", spy_accepts)
    q, k, v = (t.to(DEV).requires_grad_() for t in (Q, K, V))
    exd = {n: t.to(DEV) for n, t in ex.items()}
    work = torch.float32 if kind != "other_dtype" or out_dtype == torch.bfloat16 else torch.float64
    O = fa.attention(q, k, v, is_causal=causal, out_dtype=out_dtype)
    loss_of(kind, O, exd, work).backward()
    torch.cuda.synchronize()
    arrived, given = seen["arrived"], seen["given"]
    is_the_layout, must_copy = expected_layout(kind, arrived, H, d)
    assert is_the_layout, f"{kind}: autograd handed over strides {arrived.stride()}"
    assert arrived.dtype == out_dtype and given.dtype == out_dtype
    if must_copy:
        assert given.is_contiguous() and given.data_ptr() != arrived.data_ptr()
    else:
        assert given.data_ptr() == arrived.data_ptr() and given.stride() == arrived.stride(), "a view the library accepts was copied"
    assert all(t.grad.dtype == torch.bfloat16 for t in (q, k, v))
    gc.assert_grads([t.grad.double().cpu() for t in (q, k, v)], ref, mag, f"{kind} {heads} O {out_dtype}")


def test_a_model_layout_dO_reaches_the_library_uncopied_with_the_result_unchanged():
    """O.backward(dO) with dO a transposed view of a [B, S, H d] buffer: the same bits (dK, dV: fixed summation order) as the
    dense copy of that dO (test_loss_gradients_against_float64[model_layout-*] checks the pointer the library got)"""
    H, Hkv, d = 8, 2, 128
    Q, K, V = (randn(s, 20 + i).bfloat16().to(DEV) for i, s in enumerate(((B, H, SQ, d), (B, Hkv, SK, d), (B, Hkv, SK, d))))
    buf = randn((B, SQ, H * d), 23).to(DEV)
    dO = buf.view(B, SQ, H, d).transpose(1, 2)
    assert not dO.is_contiguous() and fa._library_accepts(dO)
    grads = []
    for g in (dO, dO.contiguous()):
        q, k, v = (t.clone().requires_grad_() for t in (Q, K, V))
        fa.attention(q, k, v, is_causal=True, out_dtype=torch.float32).backward(g)
        torch.cuda.synchronize()
        grads.append((q.grad, k.grad, v.grad))
    assert torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][2], grads[1][2])
    assert (grads[0][0].float() - grads[1][0].float()).abs().max().item() <= 1e-2 * (1 + grads[1][0].float().abs().max().item())
    # what must be copied: rows that overlap, strides off the 16-byte grid, a base pointer off it
    assert not fa._library_accepts(dO[:, :, :1].expand(B, H, SQ, d))
    assert not fa._library_accepts(torch.zeros((B, H, SQ, d + 3), device=DEV)[..., :d])          # 524-byte rows
    assert not fa._library_accepts(torch.zeros((B, H, SQ, d + 4), device=DEV)[..., 2:d + 2])     # base 8 bytes off
    assert fa._library_accepts(torch.zeros((B, H, SQ, d + 4), device=DEV)[..., :d])
