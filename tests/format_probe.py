"""Exact single-key probes of the fp8 (OCP e4m3fn) and bf16 input paths (no tests in here; tests/test_format_probe.py proves the
instrument on the CPU, tests/test_exact_formats.py uses it on the GPU).

The per-pair probes (tests/weight_probe.py) make every output element depend on one (query, key) pair.  Here the pair's softmax weight
is forced to exactly 1 as well, which turns the outputs into read-outs of single input elements:

    O[row, :] = fp32(V[key, :] * v_descale)                 (a bf16 / fp16 output: that value rounded once)
    LSE[row]  = scale * Q[row, c] * K[key, c] * k_descale     (the row's query is one-hot at column c)

so the conversions of the five fp8 input paths (decode K and V, prefill Q / K, prefill V, the weights kernel) and the "any finite bf16
V" claim are checked bit for bit, code by code, instead of through a tolerance sized for sums over keys.

How a row comes to see one key with weight exactly 1.
  structural   decode with window = 1 under the bottom-right mask (row i sees key L - Sq + i only), decode with kv_lens = 1, a prefill
               cross call with Sk = 1;
  by score     (a key anywhere in a prefill K tile) key k holds +448 at column k and -448 at every other column, and the row that
               probes key j is one-hot at column j: the probed score is +448 q, every other -448 q.  With scale = 2 ln 2 the gap is
               1242 natural-log units: exp of it is 0 in fp32, fp16, bf16 and float64 alike.

Scales.  Decode subtracts the row maximum from scores that were rounded the same way (x - m with x = m: exactly 0), so any scale gives
a weight of exactly 1 there; its families use powers of two, and one uses descales that are not.  The prefill kernels take the
exponential of fma(s, c, -m) with c = fp32(scale * log2 e) and m = fp32(s c): the fma returns the rounding residual of s c, which is
0 only if s c is exact.  Their families therefore use scale = fp32(ln 2) * 2^k, for which c is exactly 2^k (PREFILL_SCALE; asserted
in tests/test_format_probe.py): every product on the path is then exact up to the final * ln 2.

Sign of zero.  Every output element is a sum that starts from a +0 accumulator, and (+0) + (-0) = +0 in round-to-nearest: V = -0 reads
out as +0.  expected() pins that (ZERO_OUT); it is arithmetic, not a tolerance -- a -0 in O fails the check.  An explicit
float64 sum from +0 behaves so (tests/test_format_probe.py) and so do the kernels (tests/test_exact_formats.py).

LSE bound.  LSE_REL = 2 * 4 * 2^-24: the kernels' path from the exact fp32 score s to the LSE is fp32(scale * log2 e), * k_descale,
* s, * ln 2 -- four roundings of at most 2^-24 relative each (log2 of a sum of exactly 1 is exactly 0) -- with a factor 2 over it, which
also covers the fp32 roundings of the constants log2 e and ln 2 themselves (2^-25 each).  No absolute term: an expected LSE of 0 must
read 0.  The bound is derived, not measured; what the kernels reach of it is in profiles/exact_formats_gpu.log (at most 0.17).
"""
import math

import numpy as np
import torch

import __graft_entry__ as entry

fa = entry.load_package()
import kv_cache_check as kv  # noqa: E402  (reference, visible: the float64 ground truth and the rule it masks with)
from weight_probe import paged  # noqa: E402,F401  (the seeded page scatter of the decode probes: tests/test_exact_formats.py)

bf, f32, f16, u8 = torch.bfloat16, torch.float32, torch.float16, torch.uint8
FP8 = getattr(torch, "float8_e4m3fn", None)
LSE_REL = 2.0 * 4.0 * 2.0 ** -24
LN2_F32 = float(np.float32(math.log(2.0)))


def PREFILL_SCALE(k):
    """fp32(ln 2) * 2^k: the library's c = fp32(scale * fp32(log2 e)) is then exactly 2^k"""
    return LN2_F32 * 2.0 ** k


# ---- OCP e4m3fn, from the definition: S.EEEE.MMM, bias 7, subnormals at E = 0, no infinities, NaN = S.1111.111 only ----------------
def decode_e4m3fn(code):
    """one byte -> float (NaN for 0x7F / 0xFF); the sign of zero is kept"""
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return float("nan")
    mag = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)      # m/8 2^(1-7)  |  (1 + m/8) 2^(e-7)
    return -mag if s else mag


CODES = [c for c in range(256) if c & 0x7F != 0x7F]                    # the 254 finite codes
TABLE = torch.tensor([decode_e4m3fn(c) for c in range(256)], dtype=torch.float64)


def finite_codes():
    """{code: value} of the 254 finite codes, float64"""
    return {c: decode_e4m3fn(c) for c in CODES}


def code_of_slot(n):
    """uint8 tensor: slot n (any int64 tensor) -> a finite code; 254 consecutive slots hold every finite code"""
    return torch.tensor(CODES, dtype=u8)[n % 254]


def pow2_code(e):
    """the e4m3fn byte of 2^e, -6 <= e <= 8"""
    return 0x38 + 8 * e


# bf16 classes of the bf16-cache family, as bit patterns: +-0, +-2^-126 (min normal), +-1, +-max finite
BF16_CLASSES = [0x0000, 0x8000, 0x0080, 0x8080, 0x3F80, 0xBF80, 0x7F7F, 0xFF7F]


def bf16_of_slot(n):
    return torch.tensor(BF16_CLASSES, dtype=torch.int32)[n % len(BF16_CLASSES)].to(torch.int16).view(bf)


def values(t, table=TABLE):
    """float64 values of an input tensor: e4m3fn bytes (uint8) through `table`, anything else as it is"""
    return table[t.long()] if t.dtype == u8 else t.double()


# ---- families ----------------------------------------------------------------------------------------------------------------------
# A family is a dict: kind ("decode" / "prefill"), Q, K, V (CPU tensors; uint8 = e4m3fn bytes), kd, vd (fp32 [Hkv] or None), scale,
# causal, window, lens, and the read-out maps key, col (int64 [B, H, Sq]): row (b, h, i) sees key[b, h, i] of its K/V head alone and
# its query is one-hot at col[b, h, i].  fp8: the tensors whose every finite code is probed at every column ("K", "V", "Q").
DEC_B, DEC_SQ, DEC_CAP = 16, 16, 256


def _slots(*shape_and_strides):
    """sum of stride * arange over broadcast axes: _slots((n0, s0), (n1, s1), ...) -> int64 [n0, n1, ...]"""
    out = torch.zeros([n for n, _ in shape_and_strides], dtype=torch.int64)
    for ax, (n, s) in enumerate(shape_and_strides):
        shape = [1] * len(shape_and_strides)
        shape[ax] = n
        out = out + s * torch.arange(n).reshape(shape)
    return out


def _one_hot_q(B, H, Sq, d, col, val, dtype):
    """Q[b, h, i, col[b, h, i]] = val[b, h, i], 0 elsewhere"""
    Q = torch.zeros(B, H, Sq, d, dtype=dtype)
    Q.scatter_(3, col[..., None], val.to(dtype)[..., None])
    return Q


def decode_family(d, Hkv=1, kd=(0.25,), vd=(8.0,), cache="fp8", scale=0.125):
    """window = 1 under the mask: B = 16 sequences of 16, 32, ..., 256 keys, 16 rows each -- row i of sequence b sees key
    16 b + i alone, so the 16 sequences probe every key 0 .. 255 of a 256-key cache (two 128-key tiles, every row of a page of 16 or
    128).  G = d query heads per K/V head, head g one-hot at column g: one call reads all of K through the LSE and all of V through O.
    Slot k + 7 c (+ offsets per head and tensor) makes every column meet 256 consecutive slots: every finite code.
    cache "bf16": BF16_CLASSES instead of codes, the query a power of two that keeps q K inside fp32's normal range."""
    B, Sq, cap, G = DEC_B, DEC_SQ, DEC_CAP, d
    H = Hkv * G
    lens = [Sq * (b + 1) for b in range(B)]
    slot = _slots((B, 0), (Hkv, 97), (cap, 1), (d, 7))
    make = code_of_slot if cache == "fp8" else bf16_of_slot
    K, V = make(slot), make(slot + 131)
    key = (torch.tensor(lens)[:, None, None] - Sq + torch.arange(Sq)[None, None, :]).expand(B, H, Sq).contiguous()
    col = (torch.arange(H) % G)[None, :, None].expand(B, H, Sq).contiguous()
    if cache == "fp8":
        qv = (2.0 ** (torch.arange(H) % 5 - 2))[None, :, None].expand(B, H, Sq)
    else:   # |K| = max finite: q = 2^-64; |K| = 2^-126: q = 2^64; else 1
        kel = K[torch.arange(B)[:, None, None], (torch.arange(H) // G)[None, :, None], key, col].double().abs()
        qv = torch.where(kel > 2.0 ** 100, 2.0 ** -64, torch.where((kel > 0) & (kel < 2.0 ** -100), 2.0 ** 64, 1.0))
    Q = _one_hot_q(B, H, Sq, d, col, qv, bf)
    t = lambda x: torch.tensor(x, dtype=f32) if cache == "fp8" else None
    return dict(name=f"decode {cache} d {d} Hkv {Hkv} kd {kd} vd {vd}", kind="decode", Q=Q, K=K, V=V, kd=t(kd), vd=t(vd), scale=scale, causal=True,
                window=1, lens=lens, key=key, col=col, fp8=("K", "V") if cache == "fp8" else ())


def decode_key0_family(d, causal, kd=(0.5, 4.0), vd=(2.0, 0.125), scale=0.25):
    """no window: kv_lens = 1, every row sees key 0.  B = 128 sequences x 2 K/V heads = 256 caches, one row each: every finite code
    at every column of key 0.  (The capacity is 16: one page.)"""
    B, Hkv, G, cap = 128, 2, d, 16
    H = Hkv * G
    slot = _slots((B, 2), (Hkv, 1), (cap, 37), (d, 7))
    K, V = code_of_slot(slot), code_of_slot(slot + 131)
    key = torch.zeros(B, H, 1, dtype=torch.int64)
    col = (torch.arange(H) % G)[None, :, None].expand(B, H, 1).contiguous()
    qv = (2.0 ** (torch.arange(H) % 5 - 2))[None, :, None].expand(B, H, 1)
    t = lambda x: torch.tensor(x, dtype=f32)
    return dict(name=f"decode fp8 d {d} key 0 mask {causal}", kind="decode", Q=_one_hot_q(B, H, 1, d, col, qv, bf), K=K, V=V, kd=t(kd), vd=t(vd),
                scale=scale, causal=causal, window=0, lens=[1] * B, key=key, col=col, fp8=("K", "V"))


def _prefill(name, Q, K, V, key, col, scale, causal, fp8):
    return dict(name=name, kind="prefill", Q=Q, K=K, V=V, kd=None, vd=None, scale=scale, causal=causal, window=0, lens=None, key=key, col=col, fp8=fp8)


def prefill_k_family(causal, d=128):
    """Sk = 1: every row sees key 0.  H = 256 heads hold 256 consecutive slots at every column of K (and V); row i is one-hot at
    column i with q = 1/2, 1, 2 in turn.  scale = ln 2 / 512: |LSE| <= 1.22 (what the weights kernel's 2 ulp are derived for)."""
    H, Sq = 256, d
    slot = _slots((1, 0), (H, 1), (1, 0), (d, 7))
    K, V = code_of_slot(slot), code_of_slot(slot + 131)
    col = torch.arange(Sq)[None, None, :].expand(1, H, Sq).contiguous()
    qb = torch.tensor([pow2_code(-1), pow2_code(0), pow2_code(1)], dtype=u8)[torch.arange(Sq) % 3][None, None, :].expand(1, H, Sq)
    Q = _one_hot_q(1, H, Sq, d, col, qb, u8)
    return _prefill(f"prefill K mask {causal}", Q, K, V, torch.zeros(1, H, Sq, dtype=torch.int64), col, PREFILL_SCALE(-9), causal, ("K", "V"))


def prefill_q_family(causal, d=128):
    """Sk = 1, K of head h one-hot at column h (value 1): LSE[h, i] = scale Q[h, i, h].  Sq = 256 rows hold 256 consecutive slots
    at every column of Q (V rides along: O is
    checked, but 128 heads do not hold every code)."""
    H, Sq = d, 256
    Q = code_of_slot(_slots((1, 0), (H, 1), (Sq, 1), (d, 7)))
    K = torch.zeros(1, H, 1, d, dtype=u8)
    K[0, torch.arange(H), 0, torch.arange(H)] = pow2_code(0)
    V = code_of_slot(_slots((1, 0), (H, 1), (1, 0), (d, 7)) + 131)
    col = torch.arange(H)[None, :, None].expand(1, H, Sq).contiguous()
    return _prefill(f"prefill Q mask {causal}", Q, K, V, torch.zeros(1, H, Sq, dtype=torch.int64), col, PREFILL_SCALE(-9), causal, ("Q",))


V_SK, V_SQ = 65, 320


def prefill_v_family(H, causal, d=128):
    """by score, Sk = 65: a whole 64-key tile and the first key of the next (the staging ring's slot change, both halves of the fp8
    widening).  Row i < 256 probes key i % 65 (under the mask: a key it sees), row i >= 256 key i - 256: the first 256-row query block
    meets key 64 beyond tile 0 -- the optimistic pass overflows, the tracked pass answers --, the second stays within tile 0 and in
    the optimistic pass.  V[h, k, c]: slot 65 h + k + 7 c, 260 consecutive slots at every column from four heads on."""
    Sk, Sq = V_SK, V_SQ
    K = torch.full((1, H, Sk, d), 0xFE, dtype=u8)                         # -448 ...
    K[0, :, torch.arange(Sk), torch.arange(Sk)] = 0x7E                     # ... but K[k, k] = +448
    V = code_of_slot(_slots((1, 0), (H, Sk), (Sk, 1), (d, 7)))
    i = torch.arange(Sq)
    key = torch.where(i < 256, i % Sk, i - 256)[None, None, :].expand(1, H, Sq).contiguous()
    Q = _one_hot_q(1, H, Sq, d, key, torch.full((1, H, Sq), pow2_code(0)), u8)
    return _prefill(f"prefill V H {H} mask {causal}", Q, K, V, key, key.clone(), PREFILL_SCALE(1), causal, ("V",))


def cpu_families():
    """every family the GPU tests run, by name (tests/test_format_probe.py walks them all; prefill_v_family(132, ...) is the same
    construction over more heads than the chip has compute units: a persistent walk)"""
    fams = [decode_family(64), decode_family(128), decode_family(128, 2, (0.25, 2.0), (8.0, 0.5)), decode_family(128, 2, (0.0123, 3.7), (3.7, 0.0123)),
            decode_family(64, cache="bf16"), decode_family(128, cache="bf16")]
    for causal in (False, True):
        fams += [decode_key0_family(64, causal), decode_key0_family(128, causal), prefill_k_family(causal), prefill_q_family(causal),
                 prefill_v_family(4, causal)]
    return fams


# ---- expected values, the float64 reference, the checker -----------------------------------------------------------------------------
ZERO_OUT = 0.0      # what a V of -0 reads out as: +0 (module docstring)


def _gather(p, Q, K, V):
    B, H, Sq = p["key"].shape
    G = H // K.shape[1]
    b, h, i = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None], torch.arange(Sq)[None, None, :]
    return Q[b, h, i, p["col"]], K[b, h // G, p["key"], p["col"]], V[b, h // G, p["key"]], h // G


def expected(p, table=TABLE, Q=None, K=None, V=None, kd=None, vd=None):
    """(O fp32 [B, H, Sq, d], LSE float64 [B, H, Sq]) of the family's read-out maps.  The keyword arguments replace the decoder, the
    tensors or the descales: that is how tests/test_format_probe.py emulates a wrong conversion."""
    q, k, v, kvh = _gather(p, *(values(x if x is not None else p[n], table) for n, x in (("Q", Q), ("K", K), ("V", V))))
    kd = kd if kd is not None else p["kd"]
    vd = vd if vd is not None else p["vd"]
    one = torch.ones(p["K"].shape[1], dtype=torch.float64)
    kdv, vdv = (one if kd is None else kd.double())[kvh], (one if vd is None else vd.double())[kvh]
    O = (v * vdv[..., None]).to(f32)                 # exact in float64 (4 x 24 bits): one rounding
    O = torch.where(O == 0, torch.full_like(O, ZERO_OUT), O)
    return O, p["scale"] * q * k * kdv


def logical(p, table=TABLE):
    """(Q, K, V) in float64 with the descales applied: what the float64 reference takes"""
    s = lambda t: 1.0 if t is None else t.double()[None, :, None, None]
    return values(p["Q"], table), values(p["K"], table) * s(p["kd"]), values(p["V"], table) * s(p["vd"])


def visible(p, b):
    """bool [Sq, keys]: what the rows of sequence b see"""
    Sq, Sk = p["Q"].shape[2], p["K"].shape[2]
    if p["kind"] == "decode":
        L = p["lens"][b]
        vis = torch.zeros(Sq, Sk, dtype=torch.bool)
        vis[:, :L] = kv.visible(L, Sq, p["causal"], p["window"])
        return vis
    k, q = torch.arange(Sk)[None, :], torch.arange(Sq)[:, None]
    return (k <= q) if p["causal"] else torch.ones(Sq, Sk, dtype=torch.bool)


def weights(p, b):
    """float64 softmax weights [H, Sq, keys] of sequence b: the explicit softmax"""
    Q, K, _ = logical(p)
    G = Q.shape[1] // K.shape[1]
    S = (Q[b] @ K[b].repeat_interleave(G, 0).transpose(-1, -2)) * p["scale"]
    return torch.softmax(S.masked_fill(~visible(p, b)[None], float("-inf")), -1)


def reference(p):
    """(O, LSE) float64: decode through kv_cache_check.reference (under the window: the same softmax over the window's
    keys), prefill through the explicit softmax"""
    Q, K, V = logical(p)
    if p["kind"] == "decode":
        return kv.reference(Q, K, V, p["lens"], p["causal"], p["window"], scale=p["scale"])
    G = Q.shape[1] // K.shape[1]
    S = ((Q[0] @ K[0].repeat_interleave(G, 0).transpose(-1, -2)) * p["scale"]).masked_fill(~visible(p, 0)[None], float("-inf"))
    return (torch.softmax(S, -1) @ V[0].repeat_interleave(G, 0))[None], torch.logsumexp(S, -1)[None]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def verdict(O, lse, expO, expL):
    """(elements of O whose bits differ from expO rounded once to O's type, LSE entries outside the bound, worst LSE error / bound)
    O: fp32 / bf16 / fp16 CPU tensor; lse: CPU tensor or None"""
    bad_o = int((_bits(O) != _bits(expO.to(O.dtype))).sum())
    if lse is None:
        return bad_o, 0, 0.0
    got = lse.double()
    zero = expL == 0
    ratio = torch.where(zero, torch.zeros_like(got), (got - expL).abs() / (LSE_REL * expL.abs()).clamp(min=1e-300))
    bad = ~torch.isfinite(got) | torch.where(zero, got != 0, ratio > 1.0)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    return bad_o, int(bad.sum()), float(ratio.max())


def check(what, O, lse, expO, expL):
    """asserts the read-outs; prints and returns the worst LSE error / bound"""
    bad_o, bad_l, worst = verdict(O.cpu(), None if lse is None else lse.cpu(), expO, expL)
    print(f"{what}: {bad_o} of {O.numel()} elements of O differ, worst LSE error / bound {worst:.3f} ({bad_l} outside)")
    if bad_o:
        at = torch.nonzero(_bits(O.cpu()) != _bits(expO.to(O.dtype)))[0].tolist()
        raise AssertionError(f"{what}: {bad_o} elements of O differ from the probed V; first at {at}: {O.cpu()[tuple(at)].item()!r} "
                             f"for {expO[tuple(at)].item()!r}")
    assert bad_l == 0, f"{what}: {bad_l} LSE entries outside {LSE_REL:.3g} |ref|, worst ratio {worst:.3f}"
    return worst


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def probed_codes(p, which):
    """{column: set of bytes} probed in tensor `which` ("K", "Q": the one element under the LSE; "V": the whole row under O)"""
    q, k, v, _ = _gather(p, p["Q"], p["K"], p["V"])
    d = p["Q"].shape[3]
    if which == "V":
        return {c: set(v[..., c].reshape(-1).tolist()) for c in range(d)}
    el, col = (q if which == "Q" else k).reshape(-1), p["col"].reshape(-1)
    return {c: set(el[col == c].tolist()) for c in range(d)}


def probed_keys(p):
    """the (sequence, key) pairs some row reads out"""
    B = p["key"].shape[0]
    return {(b, int(k)) for b in range(B) for k in p["key"][b].unique()}


# ---- wrong conversions, emulated: each returns the keyword arguments of expected() ---------------------------------------------------
def _fnuz(code):
    """e4m3fnuz: bias 8, 0x80 = NaN, no -0, no other NaN"""
    if code == 0x80:
        return float("nan")
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    mag = m * 2.0 ** -10 if e == 0 else (8 + m) * 2.0 ** (e - 11)
    return -mag if s else mag


def _halves_swapped(t):
    """the two 8-byte halves of every 16-byte chunk of a row exchanged"""
    return t.reshape(*t.shape[:-1], -1, 2, 8).flip(-2).reshape(t.shape)


def _table(f):
    return torch.tensor([f(c) for c in range(256)], dtype=torch.float64)


def mutants(p):
    """{name: keyword arguments of expected()} of the wrong conversions that can show in family p (descales: where it has them;
    another head's: where it has another head)"""
    swapped = {n: _halves_swapped(p[n]) for n in p["fp8"]}
    out = {
        "subnormals_flushed": dict(table=_table(lambda c: decode_e4m3fn(c) if c & 0x78 else math.copysign(0.0, decode_e4m3fn(c)))),
        "fnuz": dict(table=_table(_fnuz)),
        "minus_zero_nan": dict(table=_table(lambda c: float("nan") if c == 0x80 else decode_e4m3fn(c))),
        "max_saturated": dict(table=_table(lambda c: decode_e4m3fn(c - 1 if c & 0x7F == 0x7E else c))),
        "halves_swapped": swapped,
    }
    if p["kd"] is not None:
        out["v_descale_dropped"] = dict(vd=torch.ones_like(p["vd"]))
        if len(p["kd"]) > 1:
            out["next_heads_descale"] = dict(kd=p["kd"].roll(-1), vd=p["vd"].roll(-1))
    return out
