"""What the tests of flash_attention_mla_prefill share: data, the float64 reference under the top-left mask, the model layout."""
import functools

import torch

from kv_cache_check import DEV, fa, randn

DQK, DV = 192, 128


def visible(Sq, Sk, causal):
    q, k = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    return (k <= q) if causal else torch.ones(Sq, Sk, dtype=torch.bool)


def reference(Q, K, V, causal, scale=DQK ** -0.5):
    """(O, LSE, sum_k p_k |v_k|) in float64 on the CPU: the explicit softmax over the keys each row sees"""
    s = torch.einsum("bhqd,bhkd->bhqk", Q.double(), K.double()) * scale
    s = s.masked_fill(~visible(Q.shape[2], K.shape[2], causal), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    return p @ V.double(), lse, p @ V.double().abs()


@functools.lru_cache(maxsize=None)
def case(B, H, Sq, Sk, causal):
    """bf16 N(0, 1) Q, K, V on the CPU and their reference; shared by the tests, never written to"""
    Q, K, V = (randn((B, H, S, d), 7 + i, torch.bfloat16) for i, (S, d) in enumerate(((Sq, DQK), (Sk, DQK), (Sk, DV))))
    return Q, K, V, reference(Q, K, V, causal)


def model_layout(t):
    """t [B, H, S, d] on the device as a view of a [B, S, H * d] tensor"""
    B, H, S, d = t.shape
    return t.to(DEV).transpose(1, 2).reshape(B, S, H * d).view(B, S, H, d).transpose(1, 2)


def run(Q, K, V, causal, strided=False, out_dtype=torch.float32, **kw):
    """the Python front on device copies (strided: every tensor, O included, in the model layout) -> (O, LSE)"""
    put = model_layout if strided else (lambda t: t.to(DEV))
    O = put(torch.empty(Q.shape[:3] + (DV,), dtype=out_dtype)) if strided else None
    return fa.flash_attention_mla_prefill(put(Q), put(K), put(V), O=O, is_causal=causal, out_dtype=out_dtype, return_lse=True, **kw)
