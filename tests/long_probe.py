"""Index-coded long-sequence problems whose exact answer costs O(S d) (no tests in here; tests/test_long_probe.py proves the instrument
on the CPU, tests/test_long_context.py and tests/test_long_context_backward.py use it on the GPU).

A float64 reference costs O(S^2 d), and on N(0,1) data at S = 2^20 every softmax weight is about 1e-6 -- under the 1e-5 floor of
every bound, so a key read from a wrong address or a tile left out disappears in the sum.  The per-pair windows (tests/weight_probe.py)
share that floor and the one-hot probes (tests/format_probe.py) address at most d keys.  Here a key is addressed by its INDEX, written
in binary over the first nb columns, and a row names the one key it wants:

  keys     key j >= 1 holds +1 / -1 at column b < nb by bit b of code(j) = base + j, 0 elsewhere.  nb = bits of the largest code; `base`
           lets a problem of a few thousand keys carry the 24-bit codes of a long one.  Exact in bf16, fp8 and fp32.
  anchor   key 0 is 0 but for a 1 at column nb (fp8: at columns nb and nb + 1), V[0] = 0.
  queries  row i holds a * (+1 / -1 by the bits of code(target(i))) at the columns < nb and a nb - E / c at column nb.  The scale is
           format_probe.PREFILL_SCALE(k): the kernels' c = fp32(scale log2 e) is exactly 2^k and every score an exact integer.
           bf16 / fp32: a = 128, k = 0.  fp8 (448 caps a value): a = 16, k = 3, and the anchor column's 16 nb - 8 is split over two
           columns of e4m3fn-exact values.  In exp2 units (c times the score), with E = 64:
               the target  128 nb,     the anchor  128 nb - 64,     every other key  <= 128 nb - 256  (one differing bit costs 256).
  weights  relative to tile 0's row maximum (the optimistic pass's reference; the anchor is in tile 0) the target weighs 2^64 or 1 and
           the anchor 1 or 2^-64: the anchor vanishes from the fp32 row sum and carries V = 0; every other weight is
           exp2(<= -192) = 0 in fp32.  128 nb - 64 = 64 (2 nb - 1) is exact in bf16 for nb <= 24.
  V        V[j, c] = a hash of (code(j), c, head) in -8 .. 8 (v_rows): small integers, exact in every type (fp16 included: the units
           with fp16 weights hold V as fp16); the rows of two keys, or of one key in two heads, differ in about 16 columns of 17.

Closed forms (expected_forward):   O[i] = V[target(i)] BIT FOR BIT (a bf16 output: that value rounded once; a zero reads +0, as
format_probe.ZERO_OUT explains), LSE[i] = ln 2 * 128 nb.  A row whose target the mask hides (under the mask about every seventh row
targets a key 1 .. 300 above itself; row 0 sees the anchor alone) has the anchor for its best key: O = +0 exactly and
LSE = ln 2 * (128 nb - 64); a mask that lets the key in gives V[target] instead -- the long-S check of the mask, with no non-finite
value in it.

Targets (targets()): seeded; about half within 300 keys below the row's diagonal (cross-attention: the diagonal is aligned to the
last key), the rest uniform over the visible keys; forced onto the first and last key of the first, a middle and the last 64-key
tile (the middle tile is the last of a 256-row query block: the diagonal end of kv_rows()), the last row, and the keys on both sides
of byte 2^30 and byte 2^31 - 2^20 of the head.

Backward form (pairs=True).  The row's two targets are t & ~1 and t | 1, whose codes differ in bit 0 (base is even), and the query holds
0 at column 0: both score 128 (nb - 1), P = (1/2, 1/2) -- or (1, 0) where the diagonal runs between them.  backward_closed_form()
sums over the three keys a row can see with a weight above exp2(-192) -- the pair and the anchor, whose weight of 2^-65 it keeps --
in float64: O, LSE, dQ, dK, dV and the magnitudes of grad_check.magnitudes in O(S d).  dK and dV come as the rows of the keys some row
targets; every other key but the anchor gets EXACTLY 0 (exp2 of a score 256 below the LSE is 0 in fp32).  V and dO share a direction,
as in weight_probe.build_backward, so that dP[t] - dP[t ^ 1] is of the size of the magnitude.

LSE bound.  format_probe.LSE_REL |ref|, plus e 2^-23 ln 2 for the log2 of a row sum of 2^e rather than 1 (one ulp of the hardware log
at e; e = 64 on the rows whose visible target lies beyond tile 0, else 0).  Both terms are derived, not measured.
"""
import torch

import __graft_entry__ as entry

fa = entry.load_package()
import format_probe as fp  # noqa: E402

bf, f32, f64, i64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
FP8 = fp.FP8
TILE, QBLOCK, E, UNIT = 64, 256, 64, 128          # keys per tile, rows per query block, the anchor's deficit, a * c
NEAR, CHUNK = 300, 2 ** 18
LN2 = fp.LN2_F32                                  # the scale is fp32(ln 2) 2^k: scale * score = LN2 * (exp2 units), exactly
BYTE_LINES = (2 ** 30, 2 ** 31 - 2 ** 20)
FORMATS = {"bf16": (bf, 128, 0), "f32": (f32, 128, 0), "fp8": (FP8, 16, 3)}      # dtype, a, k of PREFILL_SCALE(k)


def bits(code, nb):
    """int64 [...] -> int64 [..., nb] of +1 / -1 by bit b of the code"""
    return ((code[..., None] >> torch.arange(nb, device=code.device)) & 1) * 2 - 1


def v_rows(code, head, d):
    """int64 [...] codes -> int64 [..., d] in -8 .. 8"""
    c = torch.arange(d, device=code.device)
    x = (code[..., None] + 1) * (2 * c + 3) * 40503 + 7919 * head
    return ((x >> 7) ^ (x >> 13)) % 17 - 8


def anchor_values(total, dtype):
    """the anchor column's query value, split so that every part is exact in `dtype`"""
    hi = float(torch.tensor(float(total)).to(dtype).float())
    if hi > total:                                         # rounded up: step down to the grid point below
        hi = float(torch.tensor(total - (hi - total)).to(dtype).float())
    parts = [hi] if hi == total else [hi, total - hi]
    assert sum(parts) == total and all(float(torch.tensor(x).to(dtype).float()) == x for x in parts), (total, parts)
    return parts


def forced_keys(Sk, stride_bytes):
    """{name: key} the targets are forced onto"""
    nt = -(-Sk // TILE)
    mt = min((nt // 2) | 3, nt - 1)
    out = {"first key": 1, "last key of tile 0": min(TILE - 1, Sk - 1), "first key of a middle tile": TILE * mt,
           "last key of a middle tile": min(TILE * mt + TILE - 1, Sk - 1), "first key of the last tile": TILE * (nt - 1), "last key": Sk - 1}
    for line in BYTE_LINES:
        k = line // stride_bytes
        if 2 <= k < Sk:
            out[f"last key below byte {line}"], out[f"first key past byte {line}"] = k - 1, k
    return {n: k for n, k in out.items() if 1 <= k < Sk}


def targets(Sq, Sk, causal, seed, device, stride_bytes, pairs=False):
    """-> (int64 [Sq] target of every row, {name: row} of the forced rows)"""
    g = torch.Generator(device=device).manual_seed(seed)
    i = torch.arange(Sq, device=device)
    lo = 2 if pairs else 1
    diag = (i if causal or Sq >= Sk else i + (Sk - Sq)).clamp(max=Sk - 1)
    top = diag if causal else torch.full_like(i, Sk - 1)
    r = torch.randint(0, 2 ** 31 - 1, (3, Sq), generator=g, device=device)
    t = torch.where(r[2] % 2 == 0, diag - r[0] % NEAR, lo + r[1] % (top - lo + 1).clamp(min=1))
    named = {}
    if causal:
        future = (i % 7 == 3) & (i < Sk - 1)
        t = torch.where(future, i + 1 + r[0] % NEAR, t)
    forced = forced_keys(Sk, stride_bytes)
    for n, (name, k) in enumerate(forced.items()):
        row = k if causal else 1 + n * ((Sq - 2) // len(forced))
        if row < Sq - 1:
            t[row], named[name] = k, row
    t[Sq - 1], named["last row"] = int(top[Sq - 1]), Sq - 1
    t = t.clamp(lo, Sk - 1)
    if pairs:
        t = torch.where((t | 1) > Sk - 1, t - 2, t)
    return t, named


def _alloc(H, S, d, dtype, device, layout):
    """zeros [1, H, S, d]: dense, or ("model") a view of a [1, S, H d] buffer"""
    if layout == "model":
        return torch.zeros((1, S, H, d), dtype=dtype, device=device).transpose(1, 2)
    return torch.zeros((1, H, S, d), dtype=dtype, device=device)


def _put(T, h, r0, rows):
    """T[0, h, r0 : r0 + len] = rows (fp8: through the bytes)"""
    rows = rows.to(f32).to(T.dtype)
    if T.dtype == FP8:
        T.view(torch.uint8)[0, h, r0:r0 + rows.shape[-2]] = rows.view(torch.uint8)
    else:
        T[0, h, r0:r0 + rows.shape[-2]] = rows
    return T


def build(Sq, Sk, d, fmt="bf16", H=1, Hkv=1, causal=True, base=0, seed=0, device="cpu", layout="dense", pairs=False):
    """-> dict(Q [1, H, Sq, d], K, V [1, Hkv, Sk, d] in the format's type, target int64 [H, Sq], named, nb, scale, ...).  pairs: the
    backward form (V is then drawn by build_backward)."""
    dtype, a, k = FORMATS[fmt]
    c = 2 ** k
    assert base % 2 == 0 and Sk >= 4 and Sq >= 2
    nb = max(2, (base + Sk - 1).bit_length())
    live = nb - 1 if pairs else nb                           # bit columns the query holds
    anchor = anchor_values(a * live - E // c, dtype)
    assert nb <= 24 and nb + len(anchor) <= d
    esz = torch.empty((), dtype=dtype).element_size()
    Q, K, V = _alloc(H, Sq, d, dtype, device, layout), _alloc(Hkv, Sk, d, dtype, device, layout), _alloc(Hkv, Sk, d, dtype, device, layout)
    stride_bytes = K.stride(2) * esz
    for r0 in range(0, Sk, CHUNK):
        code = base + torch.arange(r0, min(Sk, r0 + CHUNK), device=device)
        rows = torch.zeros((len(code), d), dtype=i64, device=device)
        rows[:, :nb] = bits(code, nb)
        if r0 == 0:
            rows[0] = 0
            rows[0, nb:nb + len(anchor)] = 1
        for h in range(Hkv):
            _put(K, h, r0, rows)
            if not pairs:
                v = v_rows(code, h, d)
                if r0 == 0:
                    v[0] = 0
                _put(V, h, r0, v)
    target = torch.empty((H, Sq), dtype=i64, device=device)
    for h in range(H):
        target[h], named = targets(Sq, Sk, causal, 1000 * seed + h, device, stride_bytes, pairs)
        for r0 in range(0, Sq, CHUNK):
            t = target[h, r0:r0 + CHUNK]
            rows = torch.zeros((len(t), d), dtype=f64, device=device)
            rows[:, :nb] = a * bits(base + t, nb)
            if pairs:
                rows[:, 0] = 0
            rows[:, nb:nb + len(anchor)] = torch.tensor(anchor, dtype=f64, device=device)
            _put(Q, h, r0, rows)
    return dict(Q=Q, K=K, V=V, target=target, named=named, nb=nb, live=live, scale=fp.PREFILL_SCALE(k), c=c, fmt=fmt, causal=causal,
                base=base, pairs=pairs, stride_bytes=stride_bytes, extent=(Sk - 1) * stride_bytes + d * esz)


def seen(p):
    """bool [H, Sq]: the row's target is visible to it"""
    t = p["target"]
    return (t <= torch.arange(t.shape[1], device=t.device)[None]) if p["causal"] else torch.ones_like(t, dtype=torch.bool)


def expected_forward(p, o_dtype=f32):
    """(O [1, H, Sq, d] in o_dtype, LSE float64 [1, H, Sq], e [1, H, Sq]: the exponent of the optimistic pass's row sum)"""
    t, vis = p["target"], seen(p)
    H, Sq = t.shape
    G = H // p["V"].shape[1]
    O = torch.empty((1, H, Sq, p["V"].shape[3]), dtype=o_dtype, device=t.device)
    for h in range(H):
        Vh = p["V"][0, h // G]
        rows = (Vh.view(torch.uint8)[t[h]].view(FP8) if Vh.dtype == FP8 else Vh[t[h]]).to(f32)
        O[0, h] = torch.where(vis[h][:, None], rows, torch.zeros((), device=t.device)).to(o_dtype)
    O = torch.where(O == 0, torch.full_like(O, fp.ZERO_OUT), O)
    lse = LN2 * (UNIT * p["live"] - E * (~vis).double())
    return O, lse[None], (E * (vis & (t >= TILE)))[None]


def lse_bound(ref, e):
    return fp.LSE_REL * ref.abs() + e * 2.0 ** -23 * LN2


def _bits_of(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def describe(p, h, row):
    """where a failing row's target lies: its tile, byte offset in the head and the query block (the unit) of the row"""
    t = int(p["target"][h, row])
    return (f"head {h} row {row} (query block {row // QBLOCK}) targets key {t} (tile {t // TILE}, byte {t * p['stride_bytes']} of its head"
            f"{', hidden by the mask' if not bool(seen(p)[h, row]) else ''})")


def check_forward(what, p, O, lse, exp=None):
    """asserts O bit for bit over every row and the LSE within lse_bound; prints and returns the worst LSE error / bound"""
    expO, expL, e = exp if exp is not None else expected_forward(p, O.dtype)
    wrong = (_bits_of(O) != _bits_of(expO)).any(-1)
    if bool(wrong.any()):
        _, h, row = torch.nonzero(wrong)[0].tolist()
        raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.numel()} rows of O differ from V[target]; first: {describe(p, h, row)}: "
                             f"{O[0, h, row, :6].float().tolist()} for {expO[0, h, row, :6].float().tolist()}")
    worst = 0.0
    if lse is not None:
        ratio = (lse.double() - expL).abs() / lse_bound(expL, e)
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
        worst = float(ratio.max())
        if worst > 1.0:
            _, h, row = torch.nonzero(ratio == ratio.max())[0].tolist()
            raise AssertionError(f"{what}: {int((ratio > 1).sum())} LSE entries outside the bound, worst error / bound {worst:.3f}: "
                                 f"{describe(p, h, row)}: {float(lse[0, h, row])!r} for {float(expL[0, h, row])!r}")
    print(f"{what}: all {wrong.numel()} rows of O equal V[target] bit for bit, worst LSE error / bound {worst:.3f}")
    return worst


def largest_accepted(accepted, hi, within=4096):
    """the largest n with accepted(n) below a refused `hi`, for a call that is accepted up to a limit and refused above it.  A refusal
    comes before any launch and costs nothing, an accepted probe runs the call over all its keys (a single workgroup walking 2^23 keys
    takes a good part of a second): so the lengths are tried one by one downwards from hi, and the first accepted one is the only
    launch.  The limit must lie within `within` of hi."""
    assert not accepted(hi)
    for n in range(hi - 1, hi - within, -1):
        if accepted(n):
            return n
    raise AssertionError(f"no length in ({hi - within}, {hi}) was accepted")


# ---- the documented arithmetic in fp32, and what a wrong kernel would return -----------------------------------------------------------
MUTANTS = ("key_minus_2^16", "key_minus_2^21", "key_minus_2^(31-log2 row bytes)", "tile_skipped", "last_partial_tile_dropped", "mask_plus_64",
           "mask_minus_64", "kv_rows_one_tile_short", "v_of_the_next_key", "rows_alias_mod_2^16")


def emulate(p, h, rows, tracked=False, mutant=None, arg=None):
    """O [len(rows), d] (fp32) of head h's rows as the forward kernels compute it (tests/forward_routes.py): the optimistic pass -- weights
    relative to tile 0's row maximum, rounded to bf16, fp32 sums tile by tile -- or the tracked pass (running maximum, rescale by
    exp2(m_old - m_new)).  mutant: one of MUTANTS, `arg` its tile / shift where it has one."""
    G = p["Q"].shape[1] // p["K"].shape[1]
    rows = torch.as_tensor(rows)
    K, V = p["K"][0, h // G].to(f32), p["V"][0, h // G].to(f32)
    Sk, d = K.shape
    nb, base = p["nb"], p["base"]
    qrows = rows % 2 ** 16 if mutant == "rows_alias_mod_2^16" else rows
    Q = p["Q"][0, h].to(f32)[qrows]
    if mutant and mutant.startswith("key_minus"):             # the row 2^k keys below: its code is 2^k less (that is what base is for)
        code = base + torch.arange(Sk) - 2 ** arg
        K, V = K.clone(), V.clone()
        K[1:, :nb], V[1:] = bits(code, nb)[1:].float(), v_rows(code, h // G, d)[1:].float()
    if mutant == "v_of_the_next_key":
        V = V.roll(-1, 0)
    x = (Q @ K.T) * float(p["c"])
    assert bool((x == x.round()).all())
    key = torch.arange(Sk)[None]
    live = torch.ones(len(rows), Sk, dtype=torch.bool)
    if p["causal"]:
        live = key <= rows[:, None] + {"mask_plus_64": TILE, "mask_minus_64": -TILE}.get(mutant, 0)
    if mutant == "tile_skipped":
        live = live & (key // TILE != arg)
    if mutant == "last_partial_tile_dropped":
        live = live & (key < Sk // TILE * TILE)
    if mutant == "kv_rows_one_tile_short":                  # the unit's descriptors end one tile below min(Sk, its diagonal's tile end)
        n_tiles = torch.minimum(torch.tensor(-(-Sk // TILE)), (rows // QBLOCK + 1) * (QBLOCK // TILE))[:, None]
        live = live & (key < TILE * (n_tiles - 1))
    x = x.masked_fill(~live, float("-inf"))
    acc, l = torch.zeros(len(rows), d), torch.zeros(len(rows))
    m = x[:, :TILE].max(-1).values
    for k0 in range(0, Sk, TILE):
        xt = x[:, k0:k0 + TILE]
        if tracked:
            m_new = torch.maximum(m, xt.max(-1).values)
            r = torch.exp2(m - m_new)
            acc, l, m = acc * r[:, None], l * r, m_new
        w = torch.exp2(xt - m[:, None])
        l = l + w.sum(-1)
        acc = acc + w.to(bf).float() @ V[k0:k0 + TILE]
    return acc * (1.0 / l)[:, None]


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def _shared_direction(n, d, r, g, device):
    """[n, d] fp32: +-(0.5 + |N|) r + N / 4 (weight_probe.build_backward)"""
    out = torch.empty((n, d), dtype=f32, device=device)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        x = torch.randn((m, 1), generator=g, device=device)
        out[r0:r0 + m] = torch.sign(x) * (0.5 + x.abs()) * r + 0.25 * torch.randn((m, d), generator=g, device=device)
    return out


def build_backward(Sq, Sk, d, H=1, Hkv=1, causal=True, base=0, seed=0, device="cpu"):
    """build(pairs=True) with V (bf16, V[0] = 0) and dO (bf16-exact fp32) drawn along a shared direction"""
    p = build(Sq, Sk, d, "bf16", H, Hkv, causal, base, seed, device, pairs=True)
    g = torch.Generator(device=device).manual_seed(7000 + seed)
    r = torch.randn(d, generator=g, device=device)
    for h in range(Hkv):
        p["V"][0, h] = _shared_direction(Sk, d, r, g, device).to(bf)
    p["V"][0, :, 0] = 0
    p["dO"] = torch.stack([_shared_direction(Sq, d, r, g, device).to(bf).float() for _ in range(H)])[None]
    return p


def backward_closed_form(p):
    """float64, O(S d): dict(O, lse, dQ, mag_dQ [1, H, Sq, ...]; per K/V head: keys (sorted, the targeted keys and the anchor), dK, dV,
    mag_dK, mag_dV [len(keys), d]).  Every key not in `keys` has dK = dV = 0."""
    t = p["target"]
    H, Sq = t.shape
    Hkv, Sk, d = p["K"].shape[1:]
    G, dev, scale = H // Hkv, t.device, p["scale"]
    i = torch.arange(Sq, device=dev)[None, :, None]
    idx = torch.stack([t & ~1, t | 1, torch.zeros_like(t)], -1)                       # [H, Sq, 3]
    live = (idx <= i) if p["causal"] else torch.ones_like(idx, dtype=torch.bool)
    x = (UNIT * p["live"] - torch.tensor([0.0, 0.0, E], dtype=f64, device=dev)).expand(H, Sq, 3)
    s = (LN2 * x).masked_fill(~live, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])                                                  # [H, Sq, 3]
    kvh = torch.arange(H, device=dev) // G
    Kr, Vr = p["K"][0][kvh[:, None, None], idx].double(), p["V"][0][kvh[:, None, None], idx].double()      # [H, Sq, 3, d]
    Q, dO = p["Q"][0].double(), p["dO"][0].double()
    O = (P[..., None] * Vr).sum(2)
    dP = (dO[:, :, None] * Vr).sum(-1)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    A = P * ((dO.abs()[:, :, None] * Vr.abs()).sum(-1) + delta.abs())
    out = dict(O=O[None], lse=lse[None], dQ=(scale * (dS[..., None] * Kr).sum(2))[None], mag_dQ=(scale * (A[..., None] * Kr.abs()).sum(2))[None], heads=[])
    for hk in range(Hkv):
        hs = slice(hk * G, hk * G + G)
        pairs, inv = torch.unique(idx[hs][..., :2], return_inverse=True)              # every pair key is >= 2: the anchor is none of them
        keys, inv = torch.cat([torch.zeros(1, dtype=i64, device=dev), pairs]), inv.reshape(-1) + 1

        def add(w, X):
            """sum over the rows of w[row, slot] X[row] into the slot's key (the anchor's slot, which every row has, by a plain sum)"""
            acc = torch.zeros((len(keys), d), dtype=f64, device=dev)
            acc.index_add_(0, inv, (w[hs][..., :2, None] * X[hs][:, :, None]).reshape(-1, d))
            acc[0] = (w[hs][..., 2, None] * X[hs]).sum((0, 1))
            return acc

        out["heads"].append(dict(keys=keys, dK=scale * add(dS, Q), dV=add(P, dO), mag_dK=scale * add(A, Q.abs()), mag_dV=add(P, dO.abs())))
    return out


def dense(p, ref, name):
    """[1, Hkv, Sk, d] float64 of a per-head gradient of backward_closed_form (small problems)"""
    Hkv, Sk, d = p["K"].shape[1:]
    out = torch.zeros((1, Hkv, Sk, d), dtype=f64, device=p["target"].device)
    for hk, r in enumerate(ref["heads"]):
        out[0, hk, r["keys"]] = r[name]
    return out


def grad_bound(ref, mag, grad_dtype):
    """weight_probe's element-wise bound of the backward"""
    return 1e-2 * ref.abs() + 2.0 ** -7 * mag + 1e-5 + (2.0 ** -8 * ref.abs() if grad_dtype == bf else 0.0)


def check_backward(what, p, ref, dQ, dK, dV):
    """asserts the three gradients against the closed form and exact zeros on every untargeted key; -> {name: worst error / bound}"""
    worst = {}
    r = (dQ.double() - ref["dQ"]).abs() / grad_bound(ref["dQ"], ref["mag_dQ"], dQ.dtype)
    worst["dQ"] = float(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max())
    worst["dK"] = worst["dV"] = 0.0
    stray = {}
    for hk, h in enumerate(ref["heads"]):
        for name, g in (("dK", dK), ("dV", dV)):
            got = g[0, hk, h["keys"]].double()
            r = (got - h[name]).abs() / grad_bound(h[name], h["mag_" + name], g.dtype)
            worst[name] = max(worst[name], float(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max()))
            rest = torch.ones(g.shape[2], dtype=torch.bool, device=g.device)
            rest[h["keys"]] = False
            bad = rest & (_bits_of(g[0, hk]) != 0).any(-1)                                # -0 and NaN are not the exact 0 either
            if bool(bad.any()):
                stray[(name, hk)] = (int(bad.sum()), int(torch.nonzero(bad)[0]))
    print(f"{what}: worst error / bound dQ {worst['dQ']:.3f} dK {worst['dK']:.3f} dV {worst['dV']:.3f}; "
          f"untargeted keys with a bit set: {sum(n for n, _ in stray.values())}")
    assert not stray, f"{what}: untargeted keys are not exactly 0: " + ", ".join(f"{n} K/V head {hk}: {c} keys, first key {k} (byte {k * p['stride_bytes']})"
                                                                                for (n, hk), (c, k) in stray.items())
    assert max(worst.values()) <= 1.0, f"{what}: gradients outside the bound: {worst}"
    return worst
