"""Checker for the gradients of O = softmax(scale * Q K^T + mask) V (tests/test_backward_edges.py, test_autograd_layouts.py,
test_backward_offsets.py; its own CPU tests: tests/test_grad_check.py).  Plain torch on the CPU, no GPU, no library.

Reference.  float64 torch autograd of the explicit formula, top-left mask (key k hidden when k > q); grouped-query attention by
`repeat_interleave` of the K/V heads, so dK / dV come back summed over the group.

Criterion.  Per tensor and per block of BLOCK = 16 consecutive rows of one head (query rows for dQ, keys for dK and dV; every block,
no sampling):

    ||g - ref||_2  <=  1e-2 ||ref||_2  +  2^-7 ||mag||_2  +  1e-5 sqrt(n)

  1e-2   the relative Frobenius error the project already holds these gradients to (tests/test_backward.py)
  mag    the same block of the same formula in float64 with every product and sum taken in absolute value -- the magnitude that does
         not cancel:   dV: P^T |dO|      dK: scale (P (|dO| |V|^T + |delta|))^T |Q|      dQ: scale (P (|dO| |V|^T + |delta|)) |K|
         With a sharp softmax dP - delta cancels and ||ref|| can be tiny while the rounding errors stay at the size of `mag`.
  2^-7   four half-ulps of bf16 (2^-9 each), from the arithmetic include/flash_attention.h documents: P rounded to bf16 before dV;
         dS rounded to bf16 before dK and dQ; the forward's weight rounding, which enters delta through O; bf16 storage of O, dO or
         the gradients.  Derived, not measured; the fp32 terms are orders of magnitude below.
  n      elements in the block

`emulate()` is a float64 model of the documented arithmetic (it must pass), `wrong_*()` are deliberately wrong gradients (each must
fail somewhere): tests/test_grad_check.py runs both on every case of tests/backward_edge_cases.py.
"""
import torch

BLOCK = 16
REL, CANCEL, ABS = 1e-2, 2.0 ** -7, 1e-5
EARLY_KEYS = 1024   # include/flash_attention.h FA_EARLY_KEYS: rows that can see fewer keys run the forward with fp16 weights


def hidden(Sq, Sk, shift=0):
    """bool [Sq, Sk]: key k is hidden from row q.  shift 0 is the library's mask (k > q); -1 the off-by-one k >= q"""
    return torch.arange(Sk)[None, :] > torch.arange(Sq)[:, None] + shift


def expand_kv(T, H, index=None):
    """[B, Hkv, S, d] -> [B, H, S, d]: query head h reads K/V head h // G (or index[h])"""
    if index is not None:
        return T[:, index]
    return T.repeat_interleave(H // T.shape[1], dim=1) if T.shape[1] != H else T


def reduce_kv(T, Hkv, index=None):
    """[B, H, S, d] per-query-head sums -> [B, Hkv, S, d]"""
    B, H, S, d = T.shape
    if index is not None:
        return torch.zeros(B, Hkv, S, d, dtype=T.dtype).index_add_(1, index, T)
    return T.view(B, Hkv, H // Hkv, S, d).sum(2)


def explicit_attention(q, k, v, scale, causal, index=None):
    H = q.shape[1]
    S = (q @ expand_kv(k, H, index).transpose(-1, -2)) * scale
    if causal:
        S = S.masked_fill(hidden(*S.shape[-2:]), float("-inf"))
    return torch.softmax(S, dim=-1) @ expand_kv(v, H, index)


def reference_grads(Q, K, V, scale, causal, dO=None, loss=None, index=None):
    """float64 autograd.  Either dO (the gradient of O) or loss (a function of the float64 O returning a scalar) is given.
    Returns (dQ, dK, dV) and the float64 dO that reached O."""
    q, k, v = (t.double().detach().clone().requires_grad_() for t in (Q, K, V))
    O = explicit_attention(q, k, v, scale, causal, index)
    O.retain_grad()
    if loss is not None:
        loss(O).backward()
    else:
        O.backward(dO.double())
    return (q.grad, k.grad, v.grad), O.grad


def _parts(Q, K, V, scale, causal):
    """float64 q, k, v (K/V heads expanded), the scores, LSE and P"""
    H = Q.shape[1]
    q, k, v = Q.double(), expand_kv(K.double(), H), expand_kv(V.double(), H)
    S = (q @ k.transpose(-1, -2)) * scale
    if causal:
        S = S.masked_fill(hidden(*S.shape[-2:]), float("-inf"))
    lse = torch.logsumexp(S, -1, keepdim=True)
    return q, k, v, S, lse, torch.exp(S - lse)


def magnitudes(Q, K, V, dO, scale, causal):
    """(mag_dQ, mag_dK, mag_dV): the gradient formulas with every product and sum in absolute value (float64)"""
    q, k, v, _, _, P = _parts(Q, K, V, scale, causal)
    g = dO.double()
    delta = (g * (P @ v)).sum(-1, keepdim=True)
    A = P * (g.abs() @ v.abs().transpose(-1, -2) + delta.abs())
    Hkv = K.shape[1]
    return scale * (A @ k.abs()), reduce_kv(scale * (A.transpose(-1, -2) @ q.abs()), Hkv), reduce_kv(P.transpose(-1, -2) @ g.abs(), Hkv)


def block_norms(x):
    """[B, H, S, d] -> [B, H, ceil(S / BLOCK)]: the 2-norm of every block of BLOCK consecutive rows"""
    sq = (x.double() ** 2).sum(-1)
    pad = -sq.shape[-1] % BLOCK
    sq = torch.nn.functional.pad(sq, (0, pad))
    return sq.view(*sq.shape[:-1], -1, BLOCK).sum(-1).sqrt()


def block_ratios(g, ref, mag, rel=REL):
    """error / bound of every block: [B, H, ceil(S / BLOCK)]; a non-finite gradient gives inf"""
    S, d = ref.shape[-2:]
    rows = torch.full((-(-S // BLOCK),), float(BLOCK))
    if S % BLOCK:
        rows[-1] = S % BLOCK
    bound = rel * block_norms(ref) + CANCEL * block_norms(mag) + ABS * (rows * d).sqrt()
    err = block_norms(g.double() - ref)
    return torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))


def check(grads, refs, mags, rel=(REL, REL, REL)):
    """-> (worst error / bound per tensor as a dict, list of failure messages); nothing is sampled"""
    worst, failures = {}, []
    for name, g, r, m, rl in zip(("dQ", "dK", "dV"), grads, refs, mags, rel):
        assert g.shape == r.shape == m.shape, (name, g.shape, r.shape, m.shape)
        ratio = block_ratios(g, r, m, rl)
        worst[name] = ratio.max().item()
        bad = (ratio > 1).nonzero()
        if len(bad):
            b, h, blk = bad[ratio[tuple(bad.T)].argmax()].tolist()
            failures.append(f"{name}: {len(bad)} of {ratio.numel()} blocks over the bound, worst error / bound {worst[name]:.3g} "
                            f"at batch {b} head {h} rows [{blk * BLOCK}, {blk * BLOCK + BLOCK})")
    return worst, failures


def assert_grads(grads, refs, mags, what, rel=(REL, REL, REL)):
    worst, failures = check(grads, refs, mags, rel)
    print(f"{what}: worst error / bound dQ {worst['dQ']:.3f} dK {worst['dK']:.3f} dV {worst['dV']:.3f}")
    assert not failures, f"{what}: " + "; ".join(failures)
    return worst


# ---- the documented arithmetic, in float64 ---------------------------------------------------------------------------------

def _rb(x):
    return x.to(torch.bfloat16).double()


def emulate(Q, K, V, dO, scale, causal, o_dtype, grad_dtype):
    """include/flash_attention.h "Precision" in float64: the forward's O from weights rounded to its precision (fp16 on rows that can
    see fewer than FA_EARLY_KEYS keys, bf16 elsewhere) and stored in o_dtype; dO given in o_dtype and rounded to bf16 for the
    products; delta from that O and the given dO; the LSE stored in fp32; P rounded to bf16 before dV, dS before dK and dQ; the
    gradients rounded to grad_dtype."""
    q, k, v, S, lse, _ = _parts(Q, K, V, scale, causal)
    Sq, Sk = S.shape[-2:]
    W = torch.exp(S - S.max(-1, keepdim=True).values)
    seen = torch.arange(1, Sq + 1).clamp(max=Sk) if causal else torch.full((Sq,), Sk)
    Wr = torch.where((seen < EARLY_KEYS)[:, None], W.to(torch.float16).double(), _rb(W))
    O = ((Wr @ v) / W.sum(-1, keepdim=True)).to(o_dtype).double()
    g = dO.to(o_dtype).double()
    gb = _rb(g)
    delta = (g * O).sum(-1, keepdim=True).float().double()
    P = torch.exp(S - lse.float().double())
    dS = _rb(P * (gb @ v.transpose(-1, -2) - delta))
    Hkv = K.shape[1]
    out = (scale * (dS @ k), reduce_kv(scale * (dS.transpose(-1, -2) @ q), Hkv), reduce_kv(_rb(P).transpose(-1, -2) @ gb, Hkv))
    return tuple(t.to(grad_dtype).double() for t in out)


# ---- deliberately wrong gradients (float64, exact but for the one mistake) ------------------------------------------------

def _manual(Q, K, V, dO, scale, causal, drop=None, shift=0, zero_delta=False):
    q, k, v, _, _, P = _parts(Q, K, V, scale, causal)
    g = dO.double()
    delta = (g * (P @ v)).sum(-1, keepdim=True)
    if drop is not None:
        P = P.clone()
        P[:, drop[0], :, drop[1]:drop[1] + BLOCK] = 0
    if shift:
        P = P.masked_fill(hidden(*P.shape[-2:], shift), 0.0)
    if zero_delta:
        delta = torch.zeros_like(delta)
    dS = P * (g @ v.transpose(-1, -2) - delta)
    Hkv = K.shape[1]
    return scale * (dS @ k), reduce_kv(scale * (dS.transpose(-1, -2) @ q), Hkv), reduce_kv(P.transpose(-1, -2) @ g, Hkv)


def exact(Q, K, V, dO, scale, causal):
    """the manual formulas with no mistake: equals reference_grads to float64 rounding (tests/test_grad_check.py)"""
    return _manual(Q, K, V, dO, scale, causal)


def wrong_dropped_keys(Q, K, V, dO, scale, causal):
    """one 16-key slice of the last query head skipped by the backward (the second slice where there is one)"""
    return _manual(Q, K, V, dO, scale, causal, drop=(Q.shape[1] - 1, BLOCK if K.shape[2] >= 2 * BLOCK else 0))


def wrong_mask(Q, K, V, dO, scale, causal):
    """k >= q hidden instead of k > q (the forward, and so the LSE, are right)"""
    return _manual(Q, K, V, dO, scale, causal, shift=-1 if causal else 0)


def wrong_scale(Q, K, V, dO, scale, causal):
    """1 / sqrt(d) whatever the case's scale"""
    return reference_grads(Q, K, V, Q.shape[-1] ** -0.5, causal, dO=dO)[0]


def wrong_kv_head(Q, K, V, dO, scale, causal):
    """query head h reads K/V head h % Hkv instead of h // G"""
    return reference_grads(Q, K, V, scale, causal, dO=dO, index=torch.arange(Q.shape[1]) % K.shape[1])[0]


def wrong_zero_delta(Q, K, V, dO, scale, causal):
    """delta = 0: dS = P * dP"""
    return _manual(Q, K, V, dO, scale, causal, zero_delta=True)


CONTROLS = {"16 keys of a head left out": wrong_dropped_keys, "mask off by one": wrong_mask, "1/sqrt(d) for the scale": wrong_scale,
            "K/V head h % Hkv": wrong_kv_head, "delta = 0": wrong_zero_delta}
