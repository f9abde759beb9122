"""Helpers of the forward tests (no tests in here): which kernel family a call takes and how many units its workgroups walk, both
read from plan_ex, and a builder of inputs that drive chosen units of chosen heads through the forward kernels' fallback passes.

The forward kernels (csrc/kernel_bf16.hip.h: run_units / attention_pass) first run an OPTIMISTIC pass per unit -- exponentials relative
to the row max of key tile 0 (the first 64 keys), no running max -- and repeat the unit with the TRACKED pass when the result is not
finite; units with fp16 softmax weights hold V as fp16 and have a third stage, the bf16-weights tracked pass.  Whether a unit must or
must not leave the optimistic pass is decided HERE from the inputs alone, in float64:

    e[row] = scale * log2(e) * (max_k s[row, k] - max_{k < 64, visible} s[row, k])

the excess of the row max over tile 0's row max in exp2 units: the largest weight of the optimistic pass is 2^e.
  bf16 weights: e >= 140 overflows for certain (fp32 ends at 2^128), e <= 100 stays finite (2^100 x |v| x keys is far below 2^128);
  fp16 weights: e >= 24 overflows for certain (fp16 ends at 65504 < 2^16), e <= 12 stays finite.
Nothing here looks at what a kernel returned.
"""
import math
from collections import namedtuple

import numpy as np
import torch

import __graft_entry__ as entry

fa = entry.load_package()

LOG2E = math.log2(math.e)
TILE = 64                                   # keys per K/V tile: tile 0 is the reference of the optimistic pass
OVER = {"bf16": 140.0, "f16": 24.0}         # e at and above which the optimistic pass of a unit overflows for certain
UNDER = {"bf16": 100.0, "f16": 12.0}        # e at and below which it stays finite
NONTRIVIAL = 8.0                            # spike_under: the least e that is worth a test
# what the builder aims at (the spike's own row); between the bounds above with room for the bf16 rounding of a * Q
AIM = {("spike_over", "bf16"): 200.0, ("spike_over", "f16"): 60.0, ("spike_under", "bf16"): 90.0, ("spike_under", "f16"): 10.0}
RECIPES = ("spike_over", "spike_under", "v_big", "spike_over+v_big")


def family(B, H, Sq, Sk, d, causal, dtype, o_dtype, flags):
    """the kernel family a call takes, from what plan_ex reports"""
    e, m = fa.plan_ex(B, H, Sq, Sk, d, causal, dtype, o_dtype, flags)
    live = m if m["q_blocks"] else e
    kid = live["kernel_id"]
    if kid != 1:
        return {0: "generic", 2: "fp8", 3: "f32"}[kid]
    if live["q_block_rows"] == 128:
        return "pair"
    if d not in (64, 128):
        return "bf16_padded"
    if e["q_blocks"] and m["q_blocks"]:
        assert e["unit_lists"] == 1
        return "causal_mix"
    if e["q_blocks"]:
        return "f16_weights"
    return "bf16"


def walks(B, H, Sq, Sk, d, causal, dtype=fa.FA_DTYPE_BF16, o_dtype=fa.FA_DTYPE_F32, flags=0):
    """(units, grid) of the call's launch: units = B * H * query blocks (early + main records), grid = its workgroups"""
    e, m = fa.plan_ex(B, H, Sq, Sk, d, causal, dtype, o_dtype, flags)
    live = m if m["q_blocks"] else e
    return B * H * (e["q_blocks"] + m["q_blocks"]), live["grid"]


def blocks(B, H, Sq, Sk, d, causal, dtype=fa.FA_DTYPE_BF16, o_dtype=fa.FA_DTYPE_F32, flags=0):
    """(rows of a query block, hp): the query blocks qb < hp of every head run with fp16 softmax weights, the others with bf16"""
    e, m = fa.plan_ex(B, H, Sq, Sk, d, causal, dtype, o_dtype, flags)
    live = m if m["q_blocks"] else e
    return live["q_block_rows"], e["q_blocks"]


def randn(shape, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def poisoned_heads(H):
    """roughly every fifth head at an irregular spacing: h % 5 == 2, plus the first and the last head"""
    return sorted({0, H - 1} | {h for h in range(H) if h % 5 == 2})


# ---- float64 reference of one head, and e ---------------------------------------------------------------------------------------
def _scores(Qh, Kh, scale, causal, rows=None):
    rows = np.arange(Qh.shape[0]) if rows is None else np.asarray(rows)
    q, k = Qh.double().numpy()[rows], Kh.double().numpy()
    s = (q @ k.T) * scale
    if causal:
        s = np.where(np.arange(k.shape[0])[None, :] > rows[:, None], -np.inf, s)
    return s


def row_excess(Qh, Kh, scale, causal, rows=None):
    """e per query row (all, or `rows`) of one head ([Sq, d], [Sk, d] tensors), float64 (s carries the scale; key 0 is visible to
    every row)"""
    s = _scores(Qh, Kh, scale, causal, rows)
    return LOG2E * (s.max(axis=1) - s[:, :TILE].max(axis=1))


def head_reference(Qh, Kh, Vh, scale, causal):
    """(O, LSE) of one head in float64: softmax(scale Q K^T [+ mask]) V and ln sum exp"""
    s = _scores(Qh, Kh, scale, causal)
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return (p @ Vh.double().numpy()) / l[:, None], mx + np.log(l)


# ---- the poison builder ---------------------------------------------------------------------------------------------------------
Spike = namedtuple("Spike", "row key kind")      # K[key] = a * Q[row]; kind: the weights of the row's unit ("bf16" / "f16")
Poison = namedtuple("Poison", "Q K V heads touched spikes v_keys first_key")


def weights_of(row, q_block_rows, hp):
    return "f16" if row // q_block_rows < hp else "bf16"


def _spike_factor(Qrow, K0, scale, causal, row, aim):
    """a with e[row] = aim for K[key] = a * Q[row]: scale * a * |q|^2 = aim / log2(e) + (tile 0's row max)"""
    q = Qrow.double()
    vis = min(TILE, row + 1) if causal else TILE
    m0 = float((K0[:vis].double() @ q).max()) * scale
    return (aim / LOG2E + m0) / (scale * float(q @ q))


def poison(Q, K, V, heads, recipe, places, q_block_rows, hp, causal, scale=None, exact_pow2=False):
    """Copies of Q, K, V ([1, H, Sq, d], [1, Hkv, Sk, d]) with `recipe` applied to the K/V heads `heads`, and what was done.

    places[i % len(places)] is the placement of heads[i]: a list of (row, key) with key >= 64 (and row >= key under the mask);
    an empty list leaves the head alone.
      spike_over / spike_under: K[h, key] = a * Q[hq, row], a aimed at AIM[recipe, weights of the row's unit]; hq is the first query
        head of the group, and with grouped queries that row of Q is copied to the group's other heads (every one of them meets
        the spike);
      v_big: V[h, key] = 1e5 (the first poisoned head: -1e28);
      spike_over+v_big: both.
    exact_pow2: a is rounded up (spike_over) or down (spike_under) to a power of two, so that a * Q stays on the grid of a narrow
    type (fp8 e4m3: the tensors are passed as the float values of already quantised data).
    Returns Poison(Q, K, V, heads, touched query heads, {K/V head: [Spike]}, {K/V head: [key]}, {K/V head: first poisoned key})."""
    assert recipe in RECIPES
    Q, K, V = Q.clone(), K.clone(), V.clone()
    H, Hkv, d = Q.shape[1], K.shape[1], Q.shape[3]
    G = H // Hkv
    scale = scale if scale is not None else 1.0 / d ** 0.5
    spikes, v_keys, first_key = {}, {}, {}
    base = "spike_over" if recipe.startswith("spike_over") else recipe
    for i, h in enumerate(heads):
        place = places[i % len(places)]
        spikes[h], v_keys[h] = [], []
        for row, key in place:
            assert key >= TILE and key < K.shape[2] and row < Q.shape[2] and (row >= key or not causal)
            if recipe != "v_big":
                kind = weights_of(row, q_block_rows, hp)
                a = _spike_factor(Q[0, h * G, row], K[0, h], scale, causal, row, AIM[base, kind])
                if exact_pow2:
                    a = 2.0 ** (math.ceil(math.log2(a)) if base == "spike_over" else math.floor(math.log2(a)))
                K[0, h, key] = (a * Q[0, h * G, row].float()).to(K.dtype)
                if G > 1:
                    Q[0, h * G:(h + 1) * G, row] = Q[0, h * G, row].clone()
                spikes[h].append(Spike(row, key, kind))
            if recipe in ("v_big", "spike_over+v_big"):
                V[0, h, key] = -1.0e28 if i == 0 else 1.0e5
                v_keys[h].append(key)
        first_key[h] = min((key for _, key in place), default=None)
    touched = sorted(hq for h in heads for hq in range(h * G, (h + 1) * G))
    return Poison(Q, K, V, list(heads), touched, spikes, v_keys, first_key)


def check_intent(p, recipe, q_block_rows, hp, causal, scale=None, expect_quiet=(), n_places=1):
    """The recipe's intent, asserted in float64 from the poisoned inputs alone (module docstring).  expect_quiet: (K/V head index in
    p.heads modulo the number of placements, query block) pairs that must NOT leave their optimistic pass although the head is
    poisoned.  Returns {query head: e per row} of the touched heads."""
    H, Hkv, d = p.Q.shape[1], p.K.shape[1], p.Q.shape[3]
    G = H // Hkv
    scale = scale if scale is not None else 1.0 / d ** 0.5
    refs = {}
    for i, h in enumerate(p.heads):
        for hq in range(h * G, (h + 1) * G):
            # every row where the recipe claims something about every row, else the spikes' rows and the quiet blocks
            Sq = p.Q.shape[2]
            quiet = [qb for (j, qb) in expect_quiet if j == i % n_places]
            need = np.zeros(Sq, dtype=bool)
            need[[s.row for s in p.spikes[h]]] = True
            for qb in quiet:
                need[qb * q_block_rows:(qb + 1) * q_block_rows] = True
            if recipe == "spike_under":
                need[:] = True
            e = np.full(Sq, np.nan)
            if need.any():
                e[need] = row_excess(p.Q[0, hq].float(), p.K[0, h].float(), scale, causal, np.nonzero(need)[0])
            refs[hq] = e
            kinds = np.arange(len(e)) // q_block_rows < hp
            if recipe.startswith("spike_over"):
                for s in p.spikes[h]:
                    assert e[s.row] >= OVER[s.kind], f"head {hq} row {s.row}: e = {e[s.row]:.1f} does not overflow {s.kind} weights"
            if recipe == "spike_under":
                for s in p.spikes[h]:
                    assert NONTRIVIAL <= e[s.row] <= UNDER[s.kind], f"head {hq} row {s.row}: e = {e[s.row]:.1f} ({s.kind} weights)"
                cap = np.where(kinds, UNDER["f16"], UNDER["bf16"])
                assert (e <= cap).all(), f"head {hq}: rows {np.nonzero(e > cap)[0][:8]} would fall back by accident"
            for qb in quiet:
                rows = slice(qb * q_block_rows, (qb + 1) * q_block_rows)
                cap = UNDER["f16" if qb < hp else "bf16"]
                assert (e[rows] <= cap).all(), f"head {hq} block {qb}: e up to {e[rows].max():.1f}, meant to stay in the optimistic pass"
        if recipe in ("v_big", "spike_over+v_big"):
            # both fp16 passes come out non-finite in every fp16-weights unit that loads the key's tile: |v| is beyond fp16
            for key in p.v_keys[h]:
                assert abs(float(p.V[0, h, key, 0])) > 65504.0
    return refs


def v_big_units(p, q_block_rows, hp, nQ, causal):
    """{K/V head: query blocks whose fp16 passes must come out non-finite}: the fp16-weights blocks that load a poisoned V row"""
    out = {}
    for h in p.heads:
        out[h] = sorted({qb for key in p.v_keys[h] for qb in range(min(hp, nQ))
                         if not causal or (qb + 1) * q_block_rows > key // TILE * TILE})
    return out
