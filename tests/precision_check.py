"""Checker of the K/V-cache calls' OWN precision (no tests in here; tests/test_precision_check.py proves the instrument on the CPU,
tests/test_kv_precision.py uses it on the GPU).  Plain torch on the CPU for everything but `run`; rule, float64 reference, cache forms
and fronts are kv_cache_check's, the sinks sink_check's, the tree masks tree_check's.

Why.  split_kv_kernel spends its spare MFMAs on precision (csrc/decode_bf16.hip.h): the softmax weights enter
P.V as a bf16 hi + lo pair, the row sum is taken over the unrounded fp32 weights, the partial results and the combine are fp32.  The
stated tolerance (1e-3 + 1e-3 |ref|) is two orders of magnitude wider than that arithmetic, so a kernel that lost one of the three
would pass every test that asserts the stated tolerance alone.  This module holds fp32 outputs to the bound of the arithmetic itself.

The bound (`bounds`; fp32 outputs only).  ref, ref_abs: kv_cache_check.reference on V and on |V| (sinks applied to both: linear, the
sink's value is 0); smax: the largest |scale * score| over the pairs the case's mask, window and tree words show.
    O:    1e-5 + 1e-5 |ref| + (2^-17 + 8 max(smax, 4) 2^-23) ref_abs
    LSE:  1e-5 + 16 max(smax, 4) 2^-23 + 2^-22 |ref|
The floor, the |ref| term and the score-noise terms are the fp32 lines of tests/fuzz_gpu.py, the LSE line is
kv_cache_check.assert_close_with_score_noise's.  The one new term is 2^-17 ref_abs: hi = RN_bf16(p) leaves |p - hi| <= 2^-9 p,
lo = RN_bf16(p - hi) leaves <= 2^-18 p, and the bound takes twice that.

The emulation (`emulate`): the documented arithmetic on the same CPU tensors.  Per row block and split -- a split is a whole number
of 128-key tiles of the block's range, divided as the kernel divides them -- scores = the fp32 rounding of the exact dot product times
fp32(scale log2 e); p = exp2(x - m) in fp32; hi, lo as above; l from the unrounded p; O from (hi + lo) V accumulated wide, rounded to
fp32 and normalised; LSE = (m + log2 l) ln 2; the combine of decode_combine_kernel in fp32; the sinks where the kernels add them (one
split: the epilogue; more: the combine).  `MUTANTS` are four wrong kernels, switched by name: the lo term dropped, l summed over the hi
weights, the partial O rounded to bf16 under more than one split, the scores rounded to bf16 before the exponential.

Cases (`cases`): the shapes no other file uses -- B = 3 (the ragged call: 4), Hkv in {1, 3}, G in {1, 3, 7} and one G = 4, capacity 640,
lengths {1, Sq, 127, 129, 300, 640} (the middle three are the lengths at Sq = 1: the prefix is kept, like tests/test_extend.py does) --
N(0, 1) data with Q and K x 3 on one d of a family and V x 8 on the other, window 0 and 100, both masks, and `long_cases`: 2^15 keys.
A paged form holds the same logical cache as the contiguous form of its element type (`twin`), so the CPU tests run one of the two.
"""
import functools
import itertools
import math
from collections import namedtuple

import torch

import kv_cache_check as kv
import sink_check as sc
import tree_check as tc
from kv_cache_check import CAP, DEV, TILE, fa

bf16, f32 = torch.bfloat16, torch.float32
NEG = float("-inf")
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
MUTANTS = ("no_lo", "l_over_hi", "partial_bf16", "scores_bf16")
EMULATION_AT_MOST, MUTANT_AT_LEAST = 0.5, 4.0          # tests/test_precision_check.py: conditions on the instrument, not measurements
FORMS, FORM_IDS = sc.FORMS, sc.FORM_IDS
CAPACITY, WINDOWS, SPLITS = 640, (0, 100), (1, 3, CAP, 0)
LONG_KEYS = 1 << 15
RAGGED_ROWS = (0, 1, 33, 70)
# descales that are no powers of two, for the caches whose bytes are e4m3fn numbers as they stand (the paged fp8 tree cases)
ODD_DESCALES = (torch.tensor([0.7, 1.3, 0.9]), torch.tensor([1.1, 0.6, 1.7]))

# family: "decode", "extend", "varlen" (the ragged call), "tree"; form: (page or None, fp8); rows: Sq, or the ragged call's tuple;
# boost: "qk3" (Q and K x 3), "q3" (Q x 3), "v8" (V x 8) or None; sinks: with sink_check.sinks_for(H); masks: the tree family of every sequence
Case = namedtuple("Case", "family form d Hkv G rows lens causal W boost sinks masks cap odd")


def name_of(c):
    return (f"{c.family} d{c.d} Hkv{c.Hkv} G{c.G} rows{c.rows} lens{c.lens} causal{int(c.causal)} window{c.W} {c.boost}"
            f"{' sinks' if c.sinks else ''}{' ' + '/'.join(c.masks) if c.masks else ''} {FORM_IDS[FORMS.index(c.form)]}")


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def lengths(Sq):
    """the two length triples of a row count: {1, Sq, 127, 129, 300, 640}, the middle three shifted by Sq - 1 (the prefix is kept)"""
    return (1, 128 + Sq, CAPACITY), (Sq, 126 + Sq, 299 + Sq)


RAGGED_LENS = ((300, 1, 128 + 33, CAPACITY), (1, 127, 33, 299 + 70))      # (an idle slot's length is not read)
SHAPES = {"decode": ((3, 7, 1), (1, 3, 5), (3, 1, 16), (1, 7, 16)),            # (Hkv, G, rows)
          "extend": ((3, 3, 17), (1, 7, 65), (3, 1, 65)),
          "varlen": ((1, 7, RAGGED_ROWS), (3, 1, RAGGED_ROWS), (3, 3, RAGGED_ROWS)),
          "tree": ((3, 3, 16), (1, 7, 33), (3, 1, 33))}
SINK_SHAPES = {"decode": (1, 4, 5), "extend": (3, 3, 17), "varlen": (1, 7, RAGGED_ROWS), "tree": (3, 3, 16)}
QK3_AT = {"decode": 128, "extend": 64, "varlen": 128, "tree": 64}             # the d whose Q and K are x 3; the other d has V x 8
TREE_FORMS = (FORMS[0], FORMS[3])                                             # contiguous bf16 and paged fp8
TREE_MASKS = (("binary", "random", "binary"), ("random", "binary", "random"))


def lens_of(family, rows):
    return RAGGED_LENS if family == "varlen" else lengths(rows)


def cases(family, form, d):
    """the cases of one GPU test: every shape of the family x two length sets x both masks x window 0 / 100 (a tree call is causal)"""
    boost = "qk3" if QK3_AT[family] == d else "v8"
    odd = family == "tree" and form == FORMS[3]
    out = []
    for Hkv, G, rows in SHAPES[family]:
        for n, lens in enumerate(lens_of(family, rows)):
            for causal, W in itertools.product((True,) if family == "tree" else (False, True), WINDOWS):
                out.append(Case(family, form, d, Hkv, G, rows, lens, causal, W, boost, False, TREE_MASKS[n] if family == "tree" else None,
                                CAPACITY, odd))
    return out


def sink_cases():
    """each family once with sinks_for(H): contiguous bf16, d = 128, the causal mask, both windows; decode's is the G = 4 case"""
    out = []
    for family, (Hkv, G, rows) in SINK_SHAPES.items():
        for W in WINDOWS:
            out.append(Case(family, FORMS[0], 128, Hkv, G, rows, lens_of(family, rows)[0], True, W, "qk3" if QK3_AT[family] == 128 else "v8",
                            True, TREE_MASKS[0] if family == "tree" else None, CAPACITY, False))
    return out


def long_cases():
    """2^15 keys under the planned split count: the many-tile fp32 accumulation and a many-split combine.  Q x 3 (scores of deviation
    3): the largest dozen weights of a row carry 13 to 56 % of it and thousands of keys the rest.  Over N(0, 1) scores the roundings of
    12 000 effective weights average out an order of magnitude below the bound and no mutant of a weight could be told from the kernel;
    Q and K x 3 leave a row little more than one key of weight 1, which is exact in bf16 (tests/test_precision_check.py, test_long_case)"""
    return [Case("decode", form, 128, 1, 7, 5, (LONG_KEYS,), True, 0, "q3", False, None, LONG_KEYS, False) for form in (FORMS[0], FORMS[3])]


PLAIN_KEYS = 2048


def plain_cases():
    """CPU only: N(0, 1) with no factor, one case per family and d -- what nearly every other cache test uses -- with sequences of 640
    and of 2048 keys.  There the stated tolerance admits the first two mutants: the gap this module closes, written down as a test"""
    out = []
    for f in SHAPES:
        Hkv, G, rows = SHAPES[f][0]
        lens = (300, 1, CAPACITY, PLAIN_KEYS) if f == "varlen" else (1, CAPACITY, PLAIN_KEYS)
        out += [Case(f, FORMS[0], d, Hkv, G, rows, lens, True, 0, None, False, TREE_MASKS[0] if f == "tree" else None, PLAIN_KEYS, False)
                for d in (64, 128)]
    return out


def twin(c):
    """the case whose logical tensors are this one's: the contiguous form of the same element type (paged caches hold the same rows)"""
    return c if c.odd else c._replace(form=(None, c.form[1]))


# ---- data ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cache_class(B, Hkv, rows):
    """kv_cache_check.Cache at another batch, K/V head count and capacity"""
    return type(f"Cache{B}x{Hkv}x{rows}", (kv.Cache,), dict(B=B, HKV=Hkv, ROWS=rows))


@functools.lru_cache(maxsize=8)
def cache_of(form, d, B, Hkv, cap, boost, odd):
    """the case's cache: the logical rows depend on the element type alone, not on the page size"""
    seed = 5000 + d + 10 * Hkv + B + (1 if boost == "qk3" else 0)
    K = kv.randn((B, Hkv, cap, d), seed, f32) * (3.0 if boost == "qk3" else 1.0)
    V = kv.randn((B, Hkv, cap, d), seed + 1, f32) * (8.0 if boost == "v8" else 1.0)
    descales = tuple(t[:Hkv] for t in ODD_DESCALES) if odd else None
    return cache_class(B, Hkv, cap)(d, form[0], form[1], seed, K=K.to(bf16), V=V.to(bf16), descales=descales)


def sequences(c):
    """(sq_b, len_b) of every sequence"""
    rows = c.rows if c.family == "varlen" else (c.rows,) * len(c.lens)
    return list(zip(rows, c.lens))


@functools.lru_cache(maxsize=64)
def data(c):
    """dict(cache, Q: bf16 on the CPU -- [B, H, Sq, d], the ragged call's [T, H, d] --, sinks: fp32 [H] or None, words: [B][Sq] or None)"""
    B, H = len(c.lens), c.Hkv * c.G
    total = sum(c.rows) if c.family == "varlen" else c.rows
    shape = (total, H, c.d) if c.family == "varlen" else (B, H, c.rows, c.d)
    Q = (kv.randn(shape, 6000 + c.d + 7 * H + total, f32) * (3.0 if c.boost in ("qk3", "q3") else 1.0)).to(bf16)
    words = [tc.words_of(m, c.rows, seed=b) for b, m in enumerate(c.masks)] if c.masks else None
    return dict(cache=cache_of(c.form, c.d, B, c.Hkv, c.cap, c.boost, c.odd), Q=Q, sinks=sc.sinks_for(H) if c.sinks else None, words=words)


def rows_of(c, Q, b):
    """sequence b's query rows [H, sq_b, d]"""
    if c.family != "varlen":
        return Q[b]
    cu = kv.cu_of(c.rows)
    return Q[cu[b]:cu[b + 1]].transpose(0, 1)


def plan_of(c, ns):
    """(num_splits, rows_per_block) of the case's call under num_splits = ns (0: the library's choice), from the family's plan"""
    B, H, odt = len(c.lens), c.Hkv * c.G, fa.FA_DTYPE_F32
    if c.family == "varlen":
        p = fa.extend_varlen_plan(B, H, c.Hkv, sum(c.rows), c.cap, c.d, odt, ns, c.W)
    else:
        p = {"decode": fa.decode_plan, "extend": fa.extend_plan, "tree": fa.tree_plan}[c.family](B, H, c.Hkv, c.rows, c.cap, c.d, odt, ns, c.W)
    assert p["kv_block_rows"] == TILE
    return p["num_splits"], p["rows_per_block"]


# ---- the truth and the bound ---------------------------------------------------------------------------------------------------------
def bounds(refO, ref_abs, refL, smax):
    """(bound on O, bound on the LSE) of the module docstring"""
    s = max(smax, 4.0)
    return (1e-5 + 1e-5 * refO.abs() + (2.0 ** -17 + 8.0 * s * 2.0 ** -23) * ref_abs,
            1e-5 + 16.0 * s * 2.0 ** -23 + 2.0 ** -22 * refL.abs())


def raw_scores(c, d, b):
    """float64 Q K^T [H, sq, L] of sequence b (not scaled, not masked) and the bool [sq, L] of what its rows see"""
    sq, L = sequences(c)[b]
    S = rows_of(c, d["Q"], b).double() @ d["cache"].refK[b, :, :L].repeat_interleave(c.G, 0).transpose(-1, -2)
    return S, kv.visible(L, sq, c.causal, c.W, d["words"][b] if d["words"] else None)


@functools.lru_cache(maxsize=64)
def truth(c):
    """dict(O, lse: the float64 reference in the call's layout; o_bound, l_bound; owned: bool [T] or None; smax)"""
    d = data(c)
    cache, scale = d["cache"], 1.0 / math.sqrt(c.d)
    smax = 0.0
    for b, (sq, L) in enumerate(sequences(c)):
        if sq:
            S, vis = raw_scores(c, d, b)
            smax = max(smax, (S.abs() * scale).masked_fill(~vis[None], 0.0).max().item())
    owned = None
    if c.family == "varlen":
        refO, refL, owned = kv.reference_ragged(d["Q"], cache.refK, cache.refV, c.rows, c.lens, c.causal, c.W, d["sinks"])
        ref_abs = kv.reference_ragged(d["Q"], cache.refK, cache.refV.abs(), c.rows, c.lens, c.causal, c.W, d["sinks"])[0]
    else:
        kw = dict(words=d["words"], sinks=d["sinks"])
        refO, refL = kv.reference(d["Q"], cache.refK, cache.refV, c.lens, c.causal, c.W, **kw)
        ref_abs = kv.reference(d["Q"], cache.refK, cache.refV.abs(), c.lens, c.causal, c.W, **kw)[0]
    ob, lb = bounds(refO, ref_abs, refL, smax)
    return dict(O=refO, lse=refL, o_bound=ob, l_bound=lb, owned=owned, smax=smax)


def worst(c, O, lse, t=None):
    """(worst O error / bound, worst LSE error / bound) over the rows a sequence owns; a NaN counts as inf"""
    t = t or truth(c)
    r, lr = (O.double().cpu() - t["O"]).abs() / t["o_bound"], (lse.double().cpu() - t["lse"]).abs() / t["l_bound"]
    if t["owned"] is not None:
        r, lr = r[t["owned"]], lr[:, t["owned"]]
    r, lr = (torch.nan_to_num(x, nan=float("inf")).max().item() for x in (r, lr))
    return r, lr


def check(c, O, lse, what):
    """every element of an fp32 O and of the LSE within the bound; prints the worst ratios like kv_cache_check.assert_close"""
    r, lr = worst(c, O, lse)
    print(f"{what}: smax {truth(c)['smax']:.1f}, worst O error / bound {r:.3f}, worst LSE error / bound {lr:.3f}")
    assert r <= 1.0, f"{what}: O outside 1e-5 + 1e-5 |ref| + (2^-17 + 8 max(smax, 4) 2^-23) ref_abs, worst ratio {r:.3f}"
    assert lr <= 1.0, f"{what}: LSE outside 1e-5 + 16 max(smax, 4) 2^-23 + 2^-22 |ref|, worst ratio {lr:.3f}"
    return r, lr


def stated(c, O, lse, at_least=0):
    """(worst O, worst LSE error / the STATED tolerance) over the sequences of at least `at_least` keys that have rows"""
    t = truth(c)
    r, lr = kv.ratios(O, lse, t["O"], t["lse"])
    keep = [b for b, (sq, L) in enumerate(sequences(c)) if L >= at_least and sq]
    assert keep, "no sequence of that length"
    if c.family == "varlen":
        cu = kv.cu_of(c.rows)
        tok = [i for b in keep for i in range(cu[b], cu[b + 1])]
        return r[tok].max().item(), lr[:, tok].max().item()
    return r[keep].max().item(), lr[keep].max().item()


# ---- the emulation -------------------------------------------------------------------------------------------------------------------
def block_ranges(L, Sq, G, rpb, causal, W):
    """(first packed row, one past the last, first tile, one past the last tile) of every row block of one (sequence, K/V head): the
    tiles one of the block's rows can see (csrc/decode_bf16.hip.h: limb, firstb; 16-row blocks -- RT = 1 -- walk [first, len))"""
    nrows, first = G * Sq, kv.first_visible(L, Sq, W)
    for pr0 in range(0, nrows, rpb):
        prl = min(pr0 + rpb, nrows) - 1
        g0, gl = pr0 // Sq, prl // Sq
        qmax = Sq - 1 if g0 != gl else prl - gl * Sq
        limb = max(L - Sq + qmax + 1, 1) if rpb > 16 and causal else L
        firstb = first
        if rpb > 16 and W > 0 and Sq > fa.FA_DECODE_MAX_Q:
            qmin = 0 if g0 != gl else pr0 - g0 * Sq
            firstb = max(max(L - Sq + qmin + 1, 1) - W, 0)
        yield pr0, prl + 1, firstb // TILE, -(-limb // TILE)


def f32_(v):
    return torch.tensor(v, dtype=f32)


def _pair(p, mutant):
    hi = p.to(bf16).float()
    lo = torch.zeros_like(hi) if mutant == "no_lo" else (p - hi).to(bf16).float()
    return hi, lo


def emulate_sequence(x, V, G, rpb, L, Sq, causal, W, ns, sink, mutant):
    """x: fp32 log2-domain scores [H, Sq, L] with -inf where hidden; V float64 [Hkv, L, d]; sink: fp32 [H] or None -> (O [H, Sq, d],
    LSE [H, Sq]) fp32"""
    H, d = x.shape[0], V.shape[-1]
    X = x.reshape(H * Sq, L)
    acc, m, l = torch.zeros(ns, H * Sq, d), torch.full((ns, H * Sq), NEG), torch.zeros(ns, H * Sq)
    for kvh in range(H // G):
        for pr0, pr1, tlo, ntb in block_ranges(L, Sq, G, rpb, causal, W):
            r0, r1 = kvh * G * Sq + pr0, kvh * G * Sq + pr1
            for s in range(ns):
                t0, t1 = tlo + (ntb - tlo) * s // ns, tlo + (ntb - tlo) * (s + 1) // ns
                k0, k1 = t0 * TILE, min(t1 * TILE, L)
                if k0 >= k1:
                    continue
                xs = X[r0:r1, k0:k1]
                ms = xs.max(-1).values
                p = torch.exp2(xs - torch.where(ms == NEG, torch.zeros_like(ms), ms)[:, None])
                hi, lo = _pair(p, mutant)
                m[s, r0:r1], l[s, r0:r1] = ms, (hi if mutant == "l_over_hi" else p).sum(-1)
                acc[s, r0:r1] = ((hi.double() + lo.double()) @ V[kvh, k0:k1]).float()
    seen = m != NEG
    sinkr = None if sink is None else sink.float().repeat_interleave(Sq)              # per (head, row)
    if ns == 1:                                                                       # the split kernel's own epilogue
        m, l, acc, seen = m[0], l[0], acc[0], seen[0]
        inv, lse = torch.where(seen, 1.0 / l, torch.zeros_like(l)), torch.where(seen, (m + torch.log2(l)) * f32_(LN2), m)
        if sinkr is not None:
            sk = sinkr * f32_(LOG2E)
            M2 = torch.maximum(m, sk)
            ok = M2 != NEG
            e = torch.exp2(m - torch.where(ok, M2, torch.zeros_like(M2)))
            L2 = l * e + torch.exp2(sk - torch.where(ok, M2, torch.zeros_like(M2)))
            inv, lse = torch.where(ok, 1.0 / L2 * e, inv), torch.where(ok, (M2 + torch.log2(L2)) * f32_(LN2), lse)
        O = acc * inv[:, None]
    else:                                                                             # normalised fp32 slabs, then decode_combine_kernel
        po = acc * torch.where(seen, 1.0 / l, torch.zeros_like(l))[..., None]
        pl = torch.where(seen, (m + torch.log2(torch.where(seen, l, torch.ones_like(l)))) * f32_(LN2), m)
        if mutant == "partial_bf16":
            po = po.to(bf16).float()
        M = pl.max(0).values
        if sinkr is not None:
            M = torch.maximum(M, sinkr)
        w = torch.exp(pl - M)
        Wt = w.sum(0) + (torch.exp(sinkr - M) if sinkr is not None else 0.0)
        O, lse = (w[..., None] * po).sum(0) * (1.0 / Wt)[:, None], M + torch.log(Wt)
    return O.reshape(H, Sq, d), lse.reshape(H, Sq)


def emulate(c, ns=0, mutant=None):
    """(O, LSE) fp32 in the call's layout: the documented arithmetic (module docstring) under the plan of num_splits = ns, or one of
    MUTANTS"""
    assert mutant is None or mutant in MUTANTS
    d = data(c)
    n, rpb = plan_of(c, ns)
    H, scale_log2 = c.Hkv * c.G, f32_((1.0 / math.sqrt(c.d)) * LOG2E)
    outs = []
    for b, (sq, L) in enumerate(sequences(c)):
        if sq == 0:
            outs.append(None)
            continue
        S, vis = raw_scores(c, d, b)
        x = S.float() * scale_log2
        if mutant == "scores_bf16":
            x = x.to(bf16).float()
        x = x.masked_fill(~vis[None], NEG)
        outs.append(emulate_sequence(x, d["cache"].refV[b, :, :L], c.G, rpb, L, sq, c.causal, c.W, n, d["sinks"], mutant))
    if c.family == "varlen":
        O, lse, _ = kv.packed(outs, c.rows, sum(c.rows), H, c.d)
        return O.float(), lse.float()
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


# ---- the GPU call --------------------------------------------------------------------------------------------------------------------
def run(c, dev, ns):
    """(O fp32, LSE) of the case's call on the GPU under num_splits = ns; dev: data(c)["cache"].device()"""
    d = data(c)
    kw = dict(window=c.W, num_splits=ns, out_dtype=f32)
    if d["sinks"] is not None:
        kw["sinks"] = d["sinks"].to(DEV)
    if c.family == "tree":
        return tc.attend(dev, d["Q"].to(DEV), kv.i32(c.lens), kv.words_tensor(d["words"]).to(DEV), **kw)
    cu = kv.i32(kv.cu_of(c.rows)) if c.family == "varlen" else None
    return kv.attend(c.family, dev, d["Q"].to(DEV), kv.i32(c.lens), cu, is_causal=c.causal, **kw)
