"""Per-pair probes of the softmax weights the fused kernels compute (no tests in here; tests/test_weight_probe.py proves the
instrument on the CPU, tests/test_probe_forward.py, test_probe_decode.py and test_probe_backward.py use it on the GPU).

Every parity test compares sums over all keys, so one (query, key) pair handled wrongly disappears in the tolerance of the sum.  The
probes choose inputs so that every output element depends on exactly ONE pair; the ordinary element-wise comparison with the existing
float64 references (oracle.attention_numpy / lse_numpy, kv_cache_check.reference, grad_check.reference_grads) is then a per-pair one.
A window is d consecutive indices from w0 = seam - d/2 (it straddles its seam); every head of a call has its own window.

  P through V   (forward, decode)  V[w0+j, j] = 1, V = 0 elsewhere (exact in every type)       O[q, j]  = P[q, w0+j]
  P through dO  (backward, dV)     dO[w0+j, j] = 1, dO = 0 on every other row                  dV[k, j] = P[w0+j, k]
  dS through Q  (backward, dK)     the same dO, Q[w0+j] = c e_j on the window rows              dK[k, j] = scale c dS[w0+j, k]
  dS through K  (backward, dQ)     K[w0+j] = c e_j, K = 0 elsewhere (visible, score 0)           dQ[q, j] = scale c dS[q, w0+j]

(grouped queries: dK, dV are the sums over the group's query heads, each with its own window.)  A pair the mask hides must read
exactly 0.0.  Scores are quiet -- Q, K = 0.5 N(0,1) where random, scale c ~ 0.7 -- so that every weight stands well above the 1e-5
floor of the bounds.  Where a probe's signal is P (dP - delta), V (and dO) are drawn so that |dP - delta| is of the size of the
non-cancelling magnitude the bound is built from (build_backward).

Bounds.  Forward and decode: term by term the bound of tests/fuzz_gpu.py (its docstring derives every term):
    1e-5 + 2^-8 ref_abs + 8 max(smax, 4) 2^-23 ref_abs   [+ 2 EPS_FP8 Mmax ref_abs: fp8 inputs of the forward]
    [+ 2^-8 |ref|: bf16, no mask, no LSE request]  [+ 2^-8 |ref|: bf16 output];   fp32 inputs: 1e-5 + 8 max(smax, 4) 2^-23 ref_abs + 1e-5 |ref|
(ref_abs = ref here: V >= 0).  Decode enters P as a bf16 hi + lo pair and converts an fp8 cache exactly: it is held to the bf16 line, with
no fp8 term.  Backward: the element-wise form of grad_check's bound, 1e-2 |ref| + 2^-7 mag + 1e-5 with mag = gc.magnitudes (+ 2^-8 |ref|
for gradients stored in bf16).

Seams come from what plan_ex and decode_plan report (q_block_rows, kv_block_rows, the early / main split, num_splits); the backward's
256-key blocks, 64 keys per wave and 32-row slices are the figures of DESIGN.md section 12 (it has no plan call).
"""
import math
from collections import namedtuple

import numpy as np
import torch

import __graft_entry__ as entry

fa = entry.load_package()
import oracle  # noqa: E402  (checker only)
import forward_routes as fr  # noqa: E402
import grad_check as gc  # noqa: E402
import kv_cache_check as kv  # noqa: E402  (reference, visible)
from fuzz_gpu import EPS_FP8  # noqa: E402

bf, f32, f16 = torch.bfloat16, torch.float32, torch.float16
FP8 = getattr(torch, "float8_e4m3fn", None)
NEG = float("-inf")
EMULATION_AT_MOST, MUTANT_AT_LEAST = 0.7, 4.0        # tests/test_weight_probe.py: conditions on the instrument, not measurements
MUTANTS = ("key_dropped", "pair_hidden", "pair_shown", "key_twice", "v_swapped")


def quiet(shape, seed, dtype=bf):
    """0.5 N(0,1) in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(shape, generator=g)).to(dtype)


def window(seam, d, n):
    """w0 of the window that straddles `seam` among n indices (the columns j with w0 + j >= n stay empty)"""
    return max(0, min(seam, n) - d // 2)


def take(priority, n, limit):
    """windows for n heads: the seams of `priority` that lie in (0, limit], in that order, repeated round-robin"""
    seams = list(dict.fromkeys(s for s in priority if 0 < s <= limit))
    return [seams[i % len(seams)] for i in range(n)], seams


def one_hot_rows(n_heads, n, d, w0s, dtype):
    """[1, n_heads, n, d]: X[h, w0s[h] + j, j] = 1"""
    X = torch.zeros(1, n_heads, n, d, dtype=torch.float32)
    for h, w0 in enumerate(w0s):
        j = torch.arange(min(d, n - w0))
        X[0, h, w0 + j, j] = 1.0
    return X.to(dtype)


def ratios(got, ref, bound, zero=None):
    """error / bound of every element (float64 tensors); inf where `got` is not finite, or is not exactly 0 on the elements `zero`
    that stand for a hidden pair or for a column no window reaches (default: where the reference is exactly 0, which P through V
    gives there and nowhere else)"""
    r = (got - ref).abs() / bound
    zero = (ref == 0) if zero is None else zero
    return torch.where(torch.isfinite(got) & (~zero | (got == 0)), r, torch.full_like(r, float("inf")))


def worst_pair(ratio, w0s, G=1, rows_are="q"):
    """(worst ratio, (batch, head, q, k)) of a [B, H, S, d] ratio tensor whose column j of head h of batch b stands for index
    w0s[b][h // G] + j (rows_are "q": the rows are queries and the columns keys; "k": the other way round)"""
    flat = int(torch.argmax(ratio))
    b, h, s, j = (int(x) for x in np.unravel_index(flat, ratio.shape))
    other = w0s[b][h // G] + j
    return float(ratio.reshape(-1)[flat]), ((b, h, s, other) if rows_are == "q" else (b, h, other, s))


def report(what, ratio, w0s, G=1, rows_are="q"):
    """prints and returns (worst error / bound, its (batch, head, q, k))"""
    worst, pair = worst_pair(ratio, w0s, G, rows_are)
    print(f"{what}: worst error / bound {worst:.3f} at (batch, head, q, k) = {pair}, {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound")
    return worst, pair


# ---- float64 mutants of one head --------------------------------------------------------------------------------------------------
def mutant_scores(raw, vis, kind, q, k):
    """scores [rows, keys] (float64, -inf = hidden) of one head with one mistake at pair (q, k); raw: the unmasked scores"""
    S = raw.masked_fill(~vis, NEG)
    if kind == "key_dropped":
        S[:, k] = NEG
    elif kind == "pair_hidden":
        assert vis[q, k]
        S[q, k] = NEG
    elif kind == "pair_shown":
        assert not vis[q, k]
        S[q, k] = raw[q, k]
    elif kind == "key_twice":
        S[:, k] += math.log(2.0)
    return S


def mutant_output(raw, vis, V, kind, q, k, k2=None):
    """O [rows, d] of one head with one mistake: MUTANTS; v_swapped exchanges V[k] and V[k2]"""
    if kind == "v_swapped":
        V = V.clone()
        V[[k, k2]] = V[[k2, k]]
    return torch.softmax(mutant_scores(raw, vis, kind, q, k), -1) @ V


def mutant_elements(kind, vis, q, k, w0, d, k2=None):
    """(rows, column) of the elements of O = P-through-V the mutant at (q, k) touches, and how they are judged: "all" = every one of
    them must fail, "any" = the worst of them (two neighbouring weights may happen to be close on one row, not on all)"""
    j = k - w0
    assert 0 <= j < d
    if kind in ("pair_hidden", "pair_shown"):
        return [q], j, "all"
    if kind == "v_swapped":
        return torch.nonzero(vis[:, k] | vis[:, k2])[:, 0].tolist(), j, "any"
    if kind == "key_twice":                                    # (a softmax over one key cannot show it counted twice)
        return torch.nonzero(vis[:, k] & (vis.sum(-1) > 1))[:, 0].tolist(), j, "all"
    return torch.nonzero(vis[:, k])[:, 0].tolist(), j, "all"


def swap_partner(k, w0, d, n):
    return k + 1 if k + 1 < min(n, w0 + d) else k - 1


# ---- forward -----------------------------------------------------------------------------------------------------------------------
FwdCase = namedtuple("FwdCase", "name fam idt odt H Hkv Sq Sk d causal lse wdt layout", defaults=(True, None, "dense"))
# The persistent kernels are chosen when B * H * ceil(Sq / 256) exceeds half the device's compute units (below that the pair kernel
# takes every bf16 call at d = 64 / 128): H = 32 at Sq = 1280 is the smallest round head count on their routes.
FORWARD = [
    FwdCase("pair", "pair", bf, f32, 8, 8, 600, 600, 128, True),
    FwdCase("pair_nc", "pair", bf, f32, 8, 8, 512, 700, 128, False),
    FwdCase("bf16", "bf16", bf, f32, 32, 32, 1280, 1152, 128, False),
    FwdCase("bf16_causal", "bf16", bf, f32, 32, 32, 1280, 1280, 128, True, True, bf),
    FwdCase("bf16_no_lse", "bf16", bf, f32, 32, 32, 1280, 1152, 128, False, False),
    FwdCase("bf16_output", "bf16", bf, bf, 32, 32, 1280, 1152, 128, False),
    FwdCase("f16_weights", "f16_weights", bf, f32, 32, 32, 1280, 640, 128, False),
    FwdCase("f16_weights_causal", "f16_weights", bf, f32, 32, 32, 1280, 640, 128, True),
    FwdCase("causal_mix", "causal_mix", bf, f32, 32, 32, 1280, 1280, 128, True),
    FwdCase("causal_mix_strided", "causal_mix", bf, f32, 32, 32, 1280, 1280, 128, True, True, None, "model"),
    FwdCase("bf16_padded", "bf16_padded", bf, f32, 8, 8, 512, 1152, 80, False),
    FwdCase("bf16_padded_causal", "bf16_padded", bf, f32, 8, 8, 1280, 1280, 80, True),
    FwdCase("fp8", "fp8", "fp8", f32, 8, 8, 512, 512, 128, False),
    FwdCase("fp8_causal", "fp8", "fp8", f32, 8, 8, 512, 512, 128, True),
    FwdCase("f32", "f32", f32, f32, 8, 8, 300, 300, 128, False),
    FwdCase("f32_causal", "f32", f32, f32, 8, 8, 300, 300, 128, True),
    FwdCase("generic", "generic", bf, f32, 8, 8, 200, 200, 136, False),
    FwdCase("generic_causal", "generic", bf, f32, 8, 8, 200, 200, 136, True),
    FwdCase("gqa", "pair", bf, f32, 8, 2, 600, 600, 128, True),
    FwdCase("gqa_causal_mix", "causal_mix", bf, f32, 32, 8, 1280, 1280, 128, True),
    FwdCase("cross_ragged", "pair", bf, f32, 8, 8, 300, 700, 128, False),
    FwdCase("cross_rows_past_the_last_key", "pair", bf, f32, 8, 8, 700, 300, 128, True),
]
FORWARD_BY_NAME = {c.name: c for c in FORWARD}


def forward_codes(c):
    flags = {None: 0, f16: fa.FA_FLAG_F16_WEIGHTS, bf: fa.FA_FLAG_BF16_WEIGHTS}[c.wdt]
    idt = fa.FA_DTYPE_FP8_E4M3 if c.idt == "fp8" else {bf: fa.FA_DTYPE_BF16, f32: fa.FA_DTYPE_F32}[c.idt]
    return idt, {bf: fa.FA_DTYPE_BF16, f32: fa.FA_DTYPE_F32}[c.odt], flags


def forward_seams(c, H):
    """key seams of the case, most important first, from plan_ex: the K/V tile, the query block (under the mask its diagonal tile),
    the early / main split and FA_EARLY_KEYS, the middle of the first bf16-weights block, the ragged last tile, the last key"""
    e, m = fa.plan_ex(1, H, c.Sq, c.Sk, c.d, c.causal, *forward_codes(c))
    live = m if m["q_blocks"] else e
    kv, qb = live["kv_block_rows"], live["q_block_rows"]
    seams = [kv, c.Sk, qb, c.Sk // kv * kv]
    if e["q_blocks"] and m["q_blocks"]:
        split = m["first_q_block"] * qb if m["first_q_block"] else e["q_blocks"] * qb
        seams = [split, split + qb // 2] + seams
    seams += [fa.FA_EARLY_KEYS, 2 * qb, 2 * kv, 3 * qb, 5 * kv]
    return seams


SILENT_BELOW = 512


def fp16_rows(c):
    """bool [Sq]: the rows of the query blocks plan_ex runs with fp16 softmax weights"""
    rows, hp = fr.blocks(1, c.H, c.Sq, c.Sk, c.d, c.causal, *forward_codes(c)) if c.idt == bf and c.fam != "generic" else (1, 0)
    return torch.arange(c.Sq) // rows < hp


def silent_rows(c):
    """bool [Sq]: rows that get Q = 0.  One bf16-rounded weight is off by up to 2^-8 of itself -- the whole of the bound's 2^-8 ref_abs
    term, which is sized for a sum over keys.  The arithmetic fits into 0.7 of the bound where the 1e-5 floor carries the rest:
    2^-8 P <= 7/3 1e-5, i.e. P <= 6e-3, which quiet scores give on rows that see SILENT_BELOW keys (P <= 2.4 / keys).  Rows that see
    fewer AND run with bf16 weights (under the mask, in the families without fp16 weights) are silenced instead: all scores 0, every
    weight exactly 1 whatever maximum it is taken relative to, P = 1 / keys -- a missing or an extra pair still shows in full."""
    seen = torch.arange(1, c.Sq + 1).clamp(max=c.Sk) if c.causal else torch.full((c.Sq,), c.Sk)
    return (seen < SILENT_BELOW) & ~fp16_rows(c) & torch.tensor(c.fam not in ("f32", "generic"))


def build_forward(c, seed=0):
    """-> dict(Q, K, V: CPU tensors [1, H, S, d] in the input type, w0: one window start per K/V head, seams, H, Hkv)"""
    H, Hkv = c.H, c.Hkv
    assert fr.family(1, H, c.Sq, c.Sk, c.d, c.causal, *forward_codes(c)) == c.fam, c.name
    per_head, seams = take(forward_seams(c, H), Hkv, c.Sk)
    w0 = [window(s, c.d, c.Sk) for s in per_head]
    dt = FP8 if c.idt == "fp8" else c.idt
    Q, K = quiet((1, H, c.Sq, c.d), 10 + seed, dt), quiet((1, Hkv, c.Sk, c.d), 20 + seed, dt)
    Q = torch.where(silent_rows(c)[:, None], torch.zeros((), dtype=torch.float32).to(dt), Q)
    return dict(Q=Q, K=K, V=one_hot_rows(Hkv, c.Sk, c.d, w0, dt), w0=w0, seams=per_head, H=H, Hkv=Hkv)


def _np(t, H):
    t = t.float().double()
    return (t.repeat_interleave(H // t.shape[1], 1) if t.shape[1] != H else t).numpy()


def forward_truth(c, p):
    """float64 reference and bounds: dict(O, lse, bound, lse_bound) as float64 tensors"""
    q, k, v = _np(p["Q"], p["H"]), _np(p["K"], p["H"]), _np(p["V"], p["H"])
    ref = oracle.attention_numpy(q, k, v, causal=c.causal)
    lref = oracle.lse_numpy(q, k, causal=c.causal)
    scale = 1.0 / math.sqrt(c.d)
    smax = float(np.abs(q @ np.swapaxes(k, -1, -2)).max()) * scale
    ref_abs = np.abs(ref)                                     # V >= 0: the oracle on |V| is the oracle
    noise = 8.0 * max(smax, 4.0) * 2.0 ** -23
    if c.idt == f32:
        bound = 1e-5 + noise * ref_abs + 1e-5 * ref_abs
    else:
        bound = 1e-5 + 2.0 ** -8 * ref_abs + noise * ref_abs
    lbound = 1e-5 + 2.0 * noise + 2.0 ** -22 * np.abs(lref)
    if c.idt == "fp8":
        qmax, kmax = np.abs(q).max(-1), np.abs(k).max(-1)
        if c.causal:
            kvis = np.maximum.accumulate(kmax, axis=-1)[..., np.minimum(np.arange(c.Sq), c.Sk - 1)]
        else:
            kvis = np.broadcast_to(kmax.max(-1, keepdims=True), qmax.shape)
        m_rowmax = scale * qmax * kvis
        bound = bound + 2.0 * EPS_FP8 * float(m_rowmax.max()) * ref_abs
        lbound = lbound + EPS_FP8 * m_rowmax
    if c.idt == bf and not c.causal and not c.lse:
        bound = bound + 2.0 ** -8 * ref_abs
    if c.odt == bf:
        bound = bound + 2.0 ** -8 * ref_abs
    return dict(O=torch.from_numpy(ref), lse=torch.from_numpy(lref), bound=torch.from_numpy(bound), lse_bound=torch.from_numpy(np.broadcast_to(lbound, lref.shape).copy()))


def forward_visible(c):
    vis = torch.ones(c.Sq, c.Sk, dtype=torch.bool)
    return ~gc.hidden(c.Sq, c.Sk) if c.causal else vis


def forward_emulation(c, p):
    """the documented arithmetic in float64: weights relative to the row maximum rounded to bf16 -- to fp16 in the query blocks
    plan_ex runs with fp16 weights (the rows that see fewer than FA_EARLY_KEYS keys) --, the normaliser the fp32 sum of the unrounded
    weights (bf16 without the mask and without an LSE request: the sum of the rounded ones); fp32 inputs and the generic kernel keep
    fp32 weights.  O rounded to the output type."""
    H = p["H"]
    q, k, v = (torch.from_numpy(_np(p[n], H)) for n in ("Q", "K", "V"))
    S = (q @ k.transpose(-1, -2)) / math.sqrt(c.d)
    S = S.masked_fill(~forward_visible(c), NEG)
    W = torch.exp(S - S.max(-1, keepdim=True).values)
    Wr = W
    if c.fam not in ("f32", "generic"):
        Wr = torch.where(fp16_rows(c)[:, None], W.to(f16).double(), W.to(bf).double())
    den = Wr if (c.idt == bf and not c.causal and not c.lse) else W
    return ((Wr @ v) / den.sum(-1, keepdim=True)).to(c.odt).double()


def forward_mutant_places(c, p):
    """[(K/V head, query head, q, k)]: one pair at every head's seam -- the first key behind it; under the mask on the diagonal"""
    out = []
    G = p["H"] // p["Hkv"]
    for h, seam in enumerate(p["seams"]):
        k = min(seam, c.Sk - 1)
        q = min(k, c.Sq - 1)
        out.append((h, h * G + G - 1, q, k))
    return out


def forward_mutants(c, p, truth):
    """yields (mutant, K/V head, (q, k), worst-or-least error / bound at the elements it touches) for every mutant at every seam"""
    vis = forward_visible(c)
    for h, hq, q, k in forward_mutant_places(c, p):
        Qh, Kh, Vh = p["Q"][0, hq].float().double(), p["K"][0, h].float().double(), p["V"][0, h].float().double()
        raw = (Qh @ Kh.T) / math.sqrt(c.d)
        w0 = p["w0"][h]
        for kind in MUTANTS:
            qq, kk = q, k
            if kind == "pair_shown":
                if not c.causal or k + 1 >= min(c.Sk, w0 + c.d) or q != k:
                    continue
                kk = k + 1                                    # the mask off by one on row q
            k2 = swap_partner(kk, w0, c.d, c.Sk)
            O = mutant_output(raw, vis, Vh, kind, qq, kk, k2)
            r = ratios(O, truth["O"][0, hq], truth["bound"][0, hq])
            rows, j, mode = mutant_elements(kind, vis, qq, kk, w0, c.d, k2)
            cols = [j, k2 - w0] if kind == "v_swapped" else [j]
            hit = r[rows][:, cols]
            yield kind, h, (qq, kk), float(hit.max() if mode == "any" else hit.min())


# ---- decode ------------------------------------------------------------------------------------------------------------------------
DEC_CAP, DEC_HKV = 1024, 8
DEC_SHAPES = [(1, 4, True), (5, 8, True), (5, 8, False), (16, 16, True)]       # (Sq, G, mask)
DEC_SPLITS = (0, 1, 3, fa.FA_DECODE_MAX_SPLITS)


def split_bounds(L, ns, tile):
    """the key at which each split of a sequence of L keys starts (the ceil(L / tile) tiles are divided over the
    splits in whole tiles, split s taking tiles [nt s / ns, nt (s + 1) / ns)), empty splits left out"""
    nt = -(-L // tile)
    return sorted({nt * s // ns * tile for s in range(1, ns)} - {0, nt * tile} - set(range(L, nt * tile + 1)))


def decode_lengths(Sq, cap=DEC_CAP):
    return sorted({1, Sq, 127, 128, 129, 640, cap})


def decode_seams(L, Sq, G, d, cap=DEC_CAP, B=None, Hkv=DEC_HKV):
    """seams of a sequence of L keys: its end (under the mask the diagonals of all packed rows lie within Sq <= d / 2 keys of it) and
    every tile seam below it -- which contains every split boundary of every split count run, as asserted here from decode_plan"""
    B = B or len(decode_lengths(Sq, cap))
    tile = fa.decode_plan(B, G * Hkv, Hkv, Sq, cap, d, fa.FA_DTYPE_F32, 0)["kv_block_rows"]
    tiles = [t for t in range(tile, L, tile)]
    for ns in DEC_SPLITS:
        n = fa.decode_plan(B, G * Hkv, Hkv, Sq, cap, d, fa.FA_DTYPE_F32, ns)["num_splits"]
        assert set(split_bounds(L, n, tile)) <= set(tiles), (L, n)
    return [L] + tiles


def build_decode(Sq, G, d, fp8, seed=0, cap=DEC_CAP, lens=None, Hkv=DEC_HKV, seams=None, lift=0.0):
    """one sequence per length, DEC_HKV K/V heads, one window per (sequence, K/V head) over the sequence's seams in turn.
    lift (bf16 caches): added to every element of Q and of the windows' rows of K, which raises the windows' scores by about
    scale d lift^2 -- for a cache so long that a weight of 1 / keys would sit on the bound's 1e-5 floor.
    -> dict(Q bf16, K, V: the logical caches in float64, Kc, Vc: the caches as stored (bf16, or e4m3 with kd, vd), lens, w0 [B][Hkv])"""
    lens = lens or decode_lengths(Sq, cap)
    B, H = len(lens), G * Hkv
    Q = (quiet((B, H, Sq, d), 30 + seed, torch.float32) + lift).to(bf)
    if fp8:
        g = torch.Generator().manual_seed(40 + seed)
        Kc = torch.randn((B, Hkv, cap, d), generator=g).to(FP8)
        kd = (0.5 + torch.arange(Hkv) / 64.0).float()
        K = Kc.float().double() * kd.double()[None, :, None, None]
    else:
        Kc, kd = quiet((B, Hkv, cap, d), 40 + seed, torch.float32), None
    w0, V = [], torch.zeros(B, Hkv, cap, d)
    for b, L in enumerate(lens):
        mine = seams[b] if seams else decode_seams(L, Sq, G, d, cap, B, Hkv)
        assert len(mine) <= Hkv or seams
        w0.append([window(mine[h % len(mine)], d, cap) for h in range(Hkv)])
        V[b] = one_hot_rows(Hkv, cap, d, w0[b], torch.float32)[0]
        if not fp8:
            Kc[b] += lift * (V[b].sum(-1, keepdim=True) > 0)
    if not fp8:
        Kc = Kc.to(bf)
        K = Kc.double()
    Vc = V.to(FP8) if fp8 else V.to(bf)
    return dict(Q=Q, K=K, V=V.double(), Kc=Kc, Vc=Vc, kd=kd, vd=torch.ones(Hkv) if fp8 else None, lens=lens, w0=w0, G=G, Sq=Sq, d=d)


LONG_KEYS, LONG_LEN = 70000, 69999


def build_decode_long(d=128, seed=7):
    """70 000 keys x 2 rows, one K/V head with its window over the last split boundary of the planned split count, one over the end"""
    pl = fa.decode_plan(1, 2, 2, 2, LONG_KEYS, d, fa.FA_DTYPE_F32, 0)
    last = split_bounds(LONG_LEN, pl["num_splits"], pl["kv_block_rows"])[-1]
    return build_decode(2, 1, d, False, seed, LONG_KEYS, [LONG_LEN], 2, [[last, LONG_LEN]], lift=0.75)


def decode_truth(p, causal):
    refO, refL = kv.reference(p["Q"], p["K"], p["V"], p["lens"], causal)
    scale = 1.0 / math.sqrt(p["d"])
    smax = max(float((p["Q"][b].double() @ p["K"][b].repeat_interleave(p["G"], 0).transpose(-1, -2)).abs().max()) for b in range(len(p["lens"]))) * scale
    noise = 8.0 * max(smax, 4.0) * 2.0 ** -23
    return dict(O=refO, lse=refL, bound=1e-5 + 2.0 ** -8 * refO.abs() + noise * refO.abs(), lse_bound=1e-5 + 2.0 * noise + 2.0 ** -22 * refL.abs())


def decode_visible(L, Sq, cap, causal):
    vis = torch.zeros(Sq, cap, dtype=torch.bool)
    vis[:, :L] = kv.visible(L, Sq, causal)
    return vis


def decode_emulation(p, causal):
    """the documented arithmetic in float64: weights relative to the row maximum enter P V as a bf16 hi + lo pair, fp32 normaliser"""
    B, H, Sq, d = p["Q"].shape
    O = torch.zeros(B, H, Sq, d, dtype=torch.float64)
    for b, L in enumerate(p["lens"]):
        S = (p["Q"][b].double() @ p["K"][b].repeat_interleave(p["G"], 0).transpose(-1, -2)) / math.sqrt(d)
        S = S.masked_fill(~decode_visible(L, Sq, S.shape[-1], causal), NEG)
        W = torch.exp(S - S.max(-1, keepdim=True).values)
        hi = W.to(bf).double()
        O[b] = ((hi + (W - hi).to(bf).double()) @ p["V"][b].repeat_interleave(p["G"], 0)) / W.sum(-1, keepdim=True)
    return O


def decode_mutants(p, truth, causal):
    """yields (mutant, sequence, K/V head, (row, k), error / bound at the touched elements): MUTANTS at the seam of every window, and
    for the windows over the end of a length the lengths L + 1 and L - 1"""
    Sq, G, d = p["Sq"], p["G"], p["d"]
    cap = p["K"].shape[2]
    for b, L in enumerate(p["lens"]):
        vis = decode_visible(L, Sq, cap, causal)
        for h, w0 in enumerate(p["w0"][b]):
            hq = h * G + G - 1
            raw = (p["Q"][b, hq].double() @ p["K"][b, h].T) / math.sqrt(d)
            Vh = p["V"][b, h]
            seam = min(w0 + d // 2, L) if w0 else min(d // 2, L)
            at_end = seam == L
            k = L - 1 if at_end else seam                               # the last key / the first key behind the seam
            if not w0 <= k < w0 + d:
                k = w0
            q = Sq - 1                                                  # the row that sees every key of the length
            for kind in MUTANTS:
                qq, kk = q, k
                if kind == "pair_shown":
                    if not (causal and at_end and Sq > 1 and L >= Sq):
                        continue
                    qq, kk = 0, L - Sq + 1                              # row 0 sees k <= L - Sq: the mask off by one on it
                if kind == "v_swapped" and L < 2:
                    continue
                k2 = swap_partner(kk, w0, d, L)
                rows, j, mode = mutant_elements(kind, vis, qq, kk, w0, d, k2)
                if not rows:
                    continue
                cols = [j, k2 - w0] if kind == "v_swapped" else [j]
                hits = []
                for g in (range(h * G, h * G + G) if kind == "v_swapped" else [hq]):     # V is the group's: the exchange touches all its heads
                    raw_g = (p["Q"][b, g].double() @ p["K"][b, h].T) / math.sqrt(d)
                    r = ratios(mutant_output(raw_g, vis, Vh, kind, qq, kk, k2), truth["O"][b, g], truth["bound"][b, g])
                    hits.append(r[rows][:, cols])
                hit = torch.stack(hits)
                yield kind, b, h, (qq, kk), float(hit.max() if mode == "any" else hit.min())
            if at_end:
                for Lm in (L + 1, L - 1):
                    if not 1 <= Lm <= cap:
                        continue
                    O = torch.softmax(raw.masked_fill(~decode_visible(Lm, Sq, cap, causal), NEG), -1) @ Vh
                    r = ratios(O, truth["O"][b, hq], truth["bound"][b, hq])
                    kk = max(L, Lm) - 1                                 # the key that appears or goes
                    if w0 <= kk < w0 + d:
                        yield f"length {'+' if Lm > L else '-'} 1", b, h, (Sq - 1, kk), float(r[Sq - 1, kk - w0])


def paged(cache, page, seed=0, spare=5):
    """[B, Hkv, cap, d] -> (pool [P, Hkv, page, d], int32 table [B, cap / page]): the pages scattered by a seeded permutation, the
    pool's spare pages left as zeros"""
    B, Hkv, cap, d = cache.shape
    n = cap // page
    assert n * page == cap
    g = torch.Generator().manual_seed(50 + seed)
    table = torch.randperm(B * n + spare, generator=g)[:B * n].reshape(B, n)
    bits = cache.view(torch.uint8) if cache.dtype == FP8 else cache
    pool = torch.zeros((B * n + spare, Hkv, page, d), dtype=bits.dtype)
    pool[table] = bits.view(B, Hkv, n, page, d).permute(0, 2, 1, 3, 4)
    return (pool.view(FP8) if cache.dtype == FP8 else pool), table.to(torch.int32)


# ---- backward ----------------------------------------------------------------------------------------------------------------------
BWD_KEY_BLOCK, BWD_WAVE_KEYS, BWD_ROW_SLICE = 256, 64, 32        # keys per workgroup, per wave, rows per slice
BWD_SHAPES = [(320, 320), (300, 700), (700, 300)]
BWD_PROBES = ("dV", "dK", "dQ")
SCALE_C = 0.7                                                     # scale * c of the one-hot rows of Q / K


def backward_heads(G):
    """(H, Hkv): eight windows over the rows, four or eight over the keys"""
    return (8, 8) if G == 1 else (4 * G, 4)


def backward_seams(Sq, Sk, G):
    """(row seams per query head, key seams per K/V head): a slice seam, the last rows, the rows whose diagonal crosses a wave's 64 keys
    and a 256-key block; keys 64 and 256, the last key, further wave seams"""
    H, Hkv = backward_heads(G)
    rows, _ = take([BWD_ROW_SLICE, Sq, BWD_WAVE_KEYS, BWD_KEY_BLOCK, 5 * BWD_ROW_SLICE, 3 * BWD_WAVE_KEYS, 2 * BWD_KEY_BLOCK, 9 * BWD_ROW_SLICE], H, Sq)
    keys, _ = take([BWD_WAVE_KEYS, BWD_KEY_BLOCK, Sk, 2 * BWD_WAVE_KEYS, 2 * BWD_KEY_BLOCK, 3 * BWD_WAVE_KEYS, 5 * BWD_WAVE_KEYS, 7 * BWD_WAVE_KEYS], Hkv, Sk)
    return rows, keys


def _floored(shape, seed):
    """+-(0.5 + |N(0,1)|): random, and nowhere near 0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    return torch.sign(x) * (0.5 + x.abs())


def build_backward(probe, Sq, Sk, d, G, seed=0):
    """-> dict(Q, K, V bf16, dO fp32, scale, w0 (per query head for dV / dK, per K/V head for dQ), seams, G)

    dV, dK: V = +-(0.5 + |N|): dK's signal is P (V[k, j] - delta) against a magnitude P (|V[k, j]| + |delta|).
    dQ: dP = dO . V over all d; random dO and V would cancel to sqrt(d) of the d the magnitude sums, and 2^-7 mag would swallow a
    pair.  dO[q] = a_q r + n / 4 and V[k] = b_k r + n / 4 with |a|, |b| >= 0.5 share the direction r: dP ~ a_q b_k |r|^2 is of the
    size of its magnitude, and its sign still changes from pair to pair."""
    H, Hkv = backward_heads(G)
    scale = 1.0 / math.sqrt(d)
    c = float(torch.tensor(SCALE_C / scale).to(bf))
    Q, K = quiet((1, H, Sq, d), 60 + seed), quiet((1, Hkv, Sk, d), 70 + seed)
    rows, keys = backward_seams(Sq, Sk, G)
    if probe == "dQ":
        w0 = [window(s, d, Sk) for s in keys]
        K = (c * one_hot_rows(Hkv, Sk, d, w0, torch.float32)).to(bf)
        g = torch.Generator().manual_seed(80 + seed)
        r = torch.randn(d, generator=g)
        V = (_floored((1, Hkv, Sk, 1), 81 + seed) * r + 0.25 * torch.randn((1, Hkv, Sk, d), generator=g)).to(bf)
        dO = (_floored((1, H, Sq, 1), 82 + seed) * r + 0.25 * torch.randn((1, H, Sq, d), generator=g)).to(bf).float()
        return dict(Q=Q, K=K, V=V, dO=dO, scale=scale, w0=w0, seams=keys, G=G, c=c)
    w0 = [window(s, d, Sq) for s in rows]
    dO = one_hot_rows(H, Sq, d, w0, torch.float32)
    if probe == "dK":
        E = one_hot_rows(H, Sq, d, w0, torch.float32)
        on = E.sum(-1, keepdim=True) > 0
        Q = torch.where(on, (c * E).to(bf), Q)
    return dict(Q=Q, K=K, V=_floored((1, Hkv, Sk, d), 83 + seed).to(bf), dO=dO, scale=scale, w0=w0, seams=rows, G=G, c=c)


def backward_truth(probe, p, causal, grad_dtype=f32):
    """the float64 reference of the probed gradient and its element-wise bound"""
    i = {"dQ": 0, "dK": 1, "dV": 2}[probe]
    refs, _ = gc.reference_grads(p["Q"], p["K"], p["V"], p["scale"], causal, dO=p["dO"])
    mag = gc.magnitudes(p["Q"], p["K"], p["V"], p["dO"], p["scale"], causal)[i]
    ref = refs[i]
    bound = gc.REL * ref.abs() + gc.CANCEL * mag + gc.ABS
    if grad_dtype == bf:
        bound = bound + 2.0 ** -8 * ref.abs()
    zero = backward_zero(probe, p, causal)
    assert (ref[zero] == 0).all()
    return dict(ref=ref, bound=bound, index=i, zero=zero)


def backward_zero(probe, p, causal):
    """bool, shaped like the probed gradient: the elements that must be exactly 0 -- every pair they stand for is hidden, or their
    column lies beyond the window's last index (a visible pair may have an exact gradient of 0 too: that is not asked bit for bit)"""
    H, Sq, d = p["Q"].shape[1:]
    Hkv, Sk = p["K"].shape[1:3]
    G, j = p["G"], torch.arange(d)
    hid = gc.hidden(Sq, Sk) if causal else torch.zeros(Sq, Sk, dtype=torch.bool)
    if probe == "dQ":
        z = torch.ones(1, H, Sq, d, dtype=torch.bool)
        for h in range(H):
            k = p["w0"][h // G] + j
            z[0, h][:, k < Sk] = hid[:, k[k < Sk]]
        return z
    z = torch.ones(1, Hkv, Sk, d, dtype=torch.bool)
    for h in range(H):
        q = p["w0"][h] + j
        z[0, h // G][:, q < Sq] &= hid[q[q < Sq]].T
    return z


def backward_report(probe, p, got, truth, what):
    """the probed gradient (float64) against its reference -> (worst error / bound, (head, q, k)); for dK, dV the head is the K/V head
    and q the window row of its group's first query head"""
    r = ratios(got, truth["ref"], truth["bound"], truth["zero"])
    if probe == "dQ":
        return report(what, r, [p["w0"]], p["G"], "q")
    return report(what, r, [p["w0"][::p["G"]]], 1, "k")


def backward_emulation(probe, p, causal, o_dtype=f32, grad_dtype=f32):
    return gc.emulate(p["Q"], p["K"], p["V"], p["dO"], p["scale"], causal, o_dtype, grad_dtype)[{"dQ": 0, "dK": 1, "dV": 2}[probe]]


def backward_mutants(probe, p, truth, causal):
    """yields (mutant, query head, (q, k), error / bound at the element it touches): key_dropped, pair_hidden, pair_shown and key_twice
    applied to P (dV) or to dS (dK, dQ) of ONE query head, at the seam of that head's window.  A pair's dS is P (dP - delta), and on a
    row that sees few keys dP - delta cancels for some key: the mutants of dS are judged at the pair (q, k) itself, those of P that touch
    a whole key on every row of the window"""
    Q, K, V, dO, scale, G = p["Q"], p["K"], p["V"], p["dO"], p["scale"], p["G"]
    H, Sq, Sk, d = Q.shape[1], Q.shape[2], K.shape[2], Q.shape[3]
    q64, k64, v64, S, lse, P = gc._parts(Q, K, V, scale, causal)
    g = dO.double()
    delta = (g * (P @ v64)).sum(-1, keepdim=True)
    raw = (q64 @ k64.transpose(-1, -2)) * scale
    T = g @ v64.transpose(-1, -2) - delta                      # dP - delta
    ref, bound = truth["ref"], truth["bound"]
    for hq in range(H):
        h = hq // G
        w0 = p["w0"][h if probe == "dQ" else hq]
        seam = p["seams"][h if probe == "dQ" else hq]
        if probe == "dQ":
            k = min(seam, Sk - 1, Sq - 1 if causal else Sk)
            q = min(k, Sq - 1) if causal else min(BWD_ROW_SLICE * (1 + hq), Sq - 1)
            if not w0 <= k < w0 + d:
                continue
        else:
            q = min(seam, Sq - 1)
            k = min(q, Sk - 1) if causal else [BWD_WAVE_KEYS, BWD_KEY_BLOCK, Sk - 1][hq % 3]
        for kind in ("key_dropped", "pair_hidden", "pair_shown", "key_twice"):
            qq, kk = q, k
            if kind == "pair_shown":
                if not causal or q != k or k + 1 >= Sk or (probe == "dQ" and k + 1 >= w0 + d):
                    continue
                kk = k + 1
            Pm = P[0, hq].clone()
            if kind == "key_dropped":
                Pm[:, kk] = 0
            elif kind == "pair_hidden":
                Pm[qq, kk] = 0
            elif kind == "pair_shown":
                Pm[qq, kk] = torch.exp(raw[0, hq, qq, kk] - lse[0, hq, qq, 0])
            else:
                Pm[:, kk] *= 2
            dP_ = Pm - P[0, hq]                                 # the change of this head's P; dS changes by dP_ * T
            if probe == "dV":
                change = dP_.T @ g[0, hq]
            elif probe == "dK":
                change = scale * ((dP_ * T[0, hq]).T @ q64[0, hq])
            else:
                change = scale * ((dP_ * T[0, hq]) @ k64[0, hq])
            if probe == "dQ":
                r = change.abs() / bound[0, hq]
                hit = r[qq, kk - w0]
            else:
                r = change.abs() / bound[0, h]
                cols = torch.arange(min(d, Sq - w0))
                if kind.startswith("pair") or probe == "dK":
                    if not 0 <= qq - w0 < len(cols):
                        continue
                    hit = r[kk, qq - w0]
                else:
                    seen = P[0, hq][w0 + cols, kk] > 0
                    hit = r[kk, cols][seen].min()
            yield kind, hq, (qq, kk), float(hit)
