"""Checker shared by the sliding-window decode tests (tests/test_decode_window.py, test_decode_window_abi.py): the window's visibility
rule and the float64 ground truth under it.  Plain torch on the CPU; the criterion is decode_check.assert_close, unchanged.

`visible_window(L, Sq, causal, W)`: with limC_i = max(L - Sq + i + 1, 1) -- decode_check.visible's bottom-right causal limit -- and
lo_i = max(limC_i - W, 0), row i sees lo_i <= k < limC_i (causal) or lo_i <= k < L (not causal: the left edge still follows the
row's own position).  W = 0: no window.  `first_visible` is lo_0, the lowest key any row sees: keys below it are outside the
library's contract and the tests poison them.
"""
import torch

from decode_check import visible


def first_visible(L, Sq, W):
    """lo_0: the lowest key any of the Sq rows sees of a sequence of L keys under the window W (0: none)"""
    return max(max(L - Sq + 1, 1) - W, 0) if W > 0 else 0


def visible_window(L, Sq, causal, W):
    """bool [Sq, L]: row i sees key k under the window W"""
    if W <= 0:
        return visible(L, Sq, causal)
    k = torch.arange(L)[None, :]
    limc = (L - Sq + 1 + torch.arange(Sq)).clamp(min=1)[:, None]
    lo = (limc - W).clamp(min=0)
    return (k >= lo) & (k < (limc if causal else L))


def reference_window(Q, K, V, lens, causal, W, scale=None):
    """decode_check.reference under visible_window: float64 explicit softmax over the keys each row sees (CPU tensors; K, V
    [B, Hkv, capacity, d] in bf16, fp32 or float64): O [B, H, Sq, d], LSE [B, H, Sq]"""
    B, H, Sq, d = Q.shape
    G = H // K.shape[1]
    scale = scale or 1.0 / d ** 0.5
    O = torch.zeros(B, H, Sq, d, dtype=torch.float64)
    lse = torch.zeros(B, H, Sq, dtype=torch.float64)
    for b in range(B):
        L = K.shape[2] if lens is None else int(lens[b])
        k = K[b, :, :L].double().repeat_interleave(G, 0)
        v = V[b, :, :L].double().repeat_interleave(G, 0)
        S = (Q[b].double() @ k.transpose(-1, -2)) * scale
        S = S.masked_fill(~visible_window(L, Sq, causal, W)[None], float("-inf"))
        lse[b] = torch.logsumexp(S, -1)
        O[b] = torch.softmax(S, -1) @ v
    return O, lse
