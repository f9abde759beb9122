"""flash_attention_mla_prefill / _plan without a GPU: signatures against the header, the refusal ladder in flash_attention_cross's order
on aligned host pointers (nothing is launched), the plan, the front's own refusals, the arithmetic of the bf16 hi + lo weight pair."""
import ctypes

import pytest
import torch

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, F32, FA_ERR, FP8, MISALIGNED, NULL_POINTER,
                      MetaTensor, aligned_host_pointer, declared_parameters, fa)

RUN, PLAN = "flash_attention_mla_prefill", "flash_attention_mla_prefill_plan"
BAD_FLAGS = FA_ERR["BAD_FLAGS"]
BUF, P = aligned_host_pointer()


def call(symbol=RUN, **over):
    """`symbol` by the header's parameter names: a valid call on the host pointer P but for `over`"""
    base = dict(Q=P, K=P, V=P, O=P, LSE=None, batchSize=2, numHeads=3, seqLenQ=300, seqLenK=300, dQK=192, dV=128, scale=0.07,
                is_causal=True, o_dtype=F32, sQ=None, sK=None, sV=None, sO=None, flags=0, stream=None, plan=None)
    return getattr(fa.lib(), symbol)(*[dict(base, **over)[n] for n in declared_parameters(symbol)])


def test_signatures():
    assert declared_parameters(RUN) == ["Q", "K", "V", "O", "LSE", "batchSize", "numHeads", "seqLenQ", "seqLenK", "dQK", "dV", "scale",
                                        "is_causal", "o_dtype", "sQ", "sK", "sV", "sO", "flags", "stream"]
    assert declared_parameters(PLAN) == ["batchSize", "numHeads", "seqLenQ", "seqLenK", "dQK", "dV", "is_causal", "o_dtype", "flags", "plan"]


S = fa.FaStrides
LADDER = [   # in the order of the checks: each rung with every later rung's fault present as well
    (dict(Q=None), NULL_POINTER), (dict(O=None, K=P + 8), NULL_POINTER),
    (dict(V=P + 8, seqLenQ=0), MISALIGNED), (dict(O=P + 4), MISALIGNED),
    (dict(batchSize=0, scale=float("inf")), BAD_SHAPE), (dict(seqLenQ=0), BAD_SHAPE), (dict(dQK=0, o_dtype=FP8), BAD_SHAPE),
    (dict(scale=float("nan"), o_dtype=FP8), BAD_SCALE),
    (dict(o_dtype=FP8, dV=192), BAD_DTYPE), (dict(o_dtype=7), BAD_DTYPE),
    (dict(dQK=128, flags=1), BAD_DHEAD), (dict(dV=192), BAD_DHEAD), (dict(dQK=576, dV=512), BAD_DHEAD), (dict(dQK=128, dV=192), BAD_DHEAD),
    (dict(flags=fa.FA_FLAG_F16_WEIGHTS, seqLenK=0), BAD_FLAGS), (dict(flags=3), BAD_FLAGS), (dict(flags=4), BAD_FLAGS),
    (dict(seqLenK=0, LSE=P + 4), BAD_SHAPE),
    (dict(LSE=P + 4, sQ=ctypes.byref(S(0, 0, 128))), MISALIGNED),
    (dict(sQ=ctypes.byref(S(0, 0, 128))), BAD_STRIDE), (dict(sK=ctypes.byref(S(8, 8, 196))), BAD_STRIDE),
    (dict(sV=ctypes.byref(S(0, 0, 120))), BAD_STRIDE), (dict(sO=ctypes.byref(S(-8, 0, 128))), BAD_STRIDE),
    (dict(sK=ctypes.byref(S(0, 0, 1 << 22))), BAD_SHAPE), (dict(seqLenK=1 << 24), BAD_SHAPE),   # one head's extent
]


@pytest.mark.parametrize("over,want", LADDER, ids=[f"{i}-{'-'.join(o)}" for i, (o, _) in enumerate(LADDER)])
def test_refusal_ladder(over, want):
    assert call(**over) == want


@pytest.mark.parametrize("B,H,Sq,Sk,causal", [(1, 1, 1, 1, False), (2, 3, 300, 40, True), (1, 128, 8192, 8192, True), (4, 16, 257, 9000, False)])
def test_plan(B, H, Sq, Sk, causal):
    p = fa.mla_prefill_plan(B, H, Sq, Sk, causal)
    assert p["kernel_id"] == 4 and 0 < p["lds_bytes"] <= 160 * 1024 and p["threads"] > 0 and p["kv_block_rows"] > 0
    units = B * H * -(-Sq // p["q_block_rows"])
    assert units <= p["grid"] < units + 8
    assert call(PLAN, plan=None) == NULL_POINTER and call(PLAN, dQK=128, plan=ctypes.byref(fa.FaLaunchPlan())) == BAD_DHEAD
    assert call(PLAN, flags=fa.FA_FLAG_F16_WEIGHTS, plan=ctypes.byref(fa.FaLaunchPlan())) == BAD_FLAGS


def test_front_refusals():
    q, k, v = torch.zeros(1, 2, 8, 192, dtype=torch.bfloat16), torch.zeros(1, 2, 9, 192, dtype=torch.bfloat16), torch.zeros(1, 2, 9, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        fa.flash_attention_mla_prefill(q, k, v)                                            # CPU tensors
    Q, K, V = MetaTensor(q), MetaTensor(k), MetaTensor(v)
    for bad in ((Q, K, MetaTensor(v[:, :, :8])), (Q, MetaTensor(k[:, :1]), V), (Q, MetaTensor(k[..., :128]), V), (MetaTensor(q[0]), K, V)):
        with pytest.raises(ValueError):
            fa.flash_attention_mla_prefill(*bad)
    for bad in ((MetaTensor(q.float()), K, V), (Q, K, MetaTensor(v.half()))):
        with pytest.raises(TypeError):
            fa.flash_attention_mla_prefill(*bad)


def test_pair_carries_sixteen_bits():
    """hi = bf16(p), lo = bf16(p - hi): |p - hi - lo| <= 2^-17 p, so the early rows need no fp32 emulation of the weights"""
    p = torch.rand(1 << 16, generator=torch.Generator().manual_seed(1)).double().clamp_min(2.0 ** -100)
    hi = p.float().to(torch.bfloat16)
    lo = (p.float() - hi.float()).to(torch.bfloat16)
    assert ((p.float().double() - hi.double() - lo.double()).abs() <= 2.0 ** -17 * p).all()
