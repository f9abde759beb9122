"""GPU test of the backward pass across the 2^31-byte and 2^32-byte lines: one causal problem, B H = 8704 heads of S = 2048, d = 128,
in which every bf16 tensor holds 2^32 + 2^28 bytes (more than 2^31 ELEMENTS) and the fp32 workspace more than 2^33 bytes.  Once with
one K/V head per query head, once grouped (G = 8).  Needs ~48 GiB of device memory (5 bf16 tensors of 4.25 GiB, three bf16 gradients,
8.6 GiB of workspace, and the temporaries of the checks); skipped below that, as tests/test_baseline_configs.py skips cfg4."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import grad_check as gc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BH, S, D = 8704, 2048, 128
HEAD_BF16 = S * D * 2                    # 2^19 bytes: head 4096 starts at byte 2^31, head 8192 at byte 2^32 (element 2^31)
HEAD_ACC = S * D * 4                     # 2^20 bytes of the fp32 dQ accumulator, which follows delta (BH S floats) in the workspace


def device_randn(heads, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.empty((heads, 1, S, D), dtype=torch.bfloat16, device=DEV)
    for h0 in range(0, heads, 512):
        out[h0:h0 + 512] = torch.randn((min(512, heads - h0), 1, S, D), generator=g, device=DEV).bfloat16()
    return out


def heads_to_check():
    """the heads on both sides of byte 2^31 and byte 2^32 of the bf16 tensors, of byte 2^32 and byte 2^33 of the dQ accumulator
    (counted from the accumulator's start, where they coincide with the former, and from the workspace's start), the first, the last"""
    delta_heads = -(-BH * S * 4 // HEAD_ACC)         # heads' worth of accumulator that delta pushes the lines down by
    lines = {2 ** 31 // HEAD_BF16, 2 ** 32 // HEAD_BF16, 2 ** 32 // HEAD_ACC - delta_heads, 2 ** 33 // HEAD_ACC - delta_heads}
    heads = {0, BH - 1}
    for h in lines:
        heads |= {h - 1, h}
    assert max(heads) == BH - 1 and 2 ** 32 // HEAD_BF16 in heads
    return sorted(heads)


@pytest.mark.parametrize("G", [1, 8])
def test_backward_beyond_2_pow_32_bytes(G):
    free, _ = torch.cuda.mem_get_info()
    if free < 56 * 2 ** 30:
        pytest.skip("needs ~48 GiB of device memory")
    Hq = 8                                            # [BH / 8, 8, S, D]: B = 1088 sequences of 8 query heads
    B, Hkv = BH // Hq, Hq // G
    grad_dtype = torch.bfloat16 if G == 1 else torch.float32
    shape = lambda t, h: t.view(B, h, S, D)
    Q, dO = (shape(device_randn(BH, 500 + i), Hq) for i in range(2))
    K, V = (shape(device_randn(B * Hkv, 502 + i), Hkv) for i in range(2))
    assert Q.numel() * 2 > 2 ** 32 and fa.backward_workspace_size(B, Hq, S, D) > 2 ** 33
    O, lse = fa.flash_attention(Q, K, V, is_causal=True, out_dtype=torch.bfloat16, return_lse=True)
    dQ = torch.full((B, Hq, S, D), float("nan"), dtype=grad_dtype, device=DEV)
    dK, dV = (torch.full((B, Hkv, S, D), float("nan"), dtype=grad_dtype, device=DEV) for _ in range(2))
    fa.flash_attention_backward(Q, K, V, O, dO, lse, is_causal=True, dQ=dQ, dK=dK, dV=dV)
    torch.cuda.synchronize()
    step = 32                                         # sequences per chunk: bounds the float64 temporaries
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        for name, t in (("dQ", dQ), ("dK", dK), ("dV", dV)):
            assert bool(torch.isfinite(t[sl]).all()), f"unwritten / non-finite {name} in sequences [{b0}, {b0 + step})"
        # the two whole-tensor identities of tests/test_backward.py::test_backward_large_causal_shape, with its bounds, here per K/V
        # head (the sums over a group's query heads).  sum_k dV = sum_q dO: exact but for the bf16 rounding of P
        g64 = dO[sl].double()
        lhs = g64.view(-1, Hkv, G, S, D).sum((2, 3))
        assert ((lhs - dV[sl].double().sum(2)).abs() <= 2 ** -8 * g64.abs().view(-1, Hkv, G, S, D).sum((2, 3)) + 1e-4).all(), b0
        # sum dQ Q = sum dK K: both from the same bf16 dS.  (bf16 gradients add independent roundings of 2^-9 relative per element:
        # over the 2^18 elements of a head, 2^-9 / 2^9 = 4e-6 of the sum of magnitudes -- inside the 1e-4)
        a = (dQ[sl].double() * Q[sl].double()).sum((2, 3)).view(-1, Hkv, G).sum(2)
        b = (dK[sl].double() * K[sl].double()).sum((2, 3))
        mags = (dQ[sl].double().abs() * Q[sl].double().abs()).sum((2, 3)).view(-1, Hkv, G).sum(2)
        assert ((a - b).abs() <= 1e-4 * mags + 1e-4).all(), b0
        del g64, lhs, a, b, mags
    # float64 on whole K/V heads (with all the query heads of their group): the per-block criterion of tests/grad_check.py
    scale = 1.0 / D ** 0.5
    for head in heads_to_check():
        b_, hq = divmod(head, Hq)
        kvh = hq // G
        hs = slice(kvh * G, kvh * G + G)
        q, g = Q[b_:b_ + 1, hs].cpu(), dO[b_:b_ + 1, hs].cpu()
        k, v = K[b_:b_ + 1, kvh:kvh + 1].cpu(), V[b_:b_ + 1, kvh:kvh + 1].cpu()
        ref, _ = gc.reference_grads(q, k, v, scale, True, dO=g)
        mag = gc.magnitudes(q, k, v, g, scale, True)
        got = [dQ[b_:b_ + 1, hs].double().cpu(), dK[b_:b_ + 1, kvh:kvh + 1].double().cpu(), dV[b_:b_ + 1, kvh:kvh + 1].double().cpu()]
        gc.assert_grads(got, ref, mag, f"G {G}, flattened query head {head}")
    # heads are distinct draws: a wrapped offset would make a head past the line alias one before it
    line = 2 ** 32 // HEAD_BF16
    flat = dQ.view(BH, S, D)
    assert not torch.equal(flat[line], flat[0]) and not torch.equal(flat[line + 1], flat[1])
