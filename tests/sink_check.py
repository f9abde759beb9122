"""Checker shared by the attention-sink tests (tests/test_sink_abi.py, test_sink.py, test_sink_extend.py, test_sink_memory_contract.py):
the float64 ground truth of a K/V-cache call with ``sinks``, derived from the existing references, and the data the tests build alike.
Plain torch on the CPU; rule, reference, criterion, the four cache forms (`Cache`) and the fronts (`attend`) are kv_cache_check's.

Reference.  A sink is one more key of score ``sinks[h]`` (natural log, not scaled) and value 0 in the softmax of every row of query head
h.  So with (O, LSE) the reference WITHOUT sinks -- kv_cache_check.reference, or reference_ragged for the ragged call --

    LSE' = logaddexp(LSE, sink_h)        O' = O * exp(LSE - LSE')

(`apply_sinks`: what kv_cache_check.reference does with its ``sinks`` argument).  `brute_force` is the same thing the long way round --
an explicit softmax in float64 over the visible keys (`scores`: kv_cache_check.visible, never its reference) and one extra column of
score sink_h whose value row is 0 -- and test_sink_abi.py holds the two against each other.

Sink vector.  `SINKS8` is the vector of the parity cases at H = 8.  `sinks_for(H)` cycles it for H > 8.  For H < 8 it takes every
(8 / H)-th element from index 1 on (H = 2: 0 and 5.5; H = 4: 0, 3, 5.5, 8), not the first H: the first two, (-inf, 0), would
leave an un-windowed 300-key sequence (LSE about ln 300 + 1/2 = 6.2) with sink weights of 0 and e^-6.2 = 0.002 and the case would test
nothing, which `assert_sinks_matter` refuses.  With 0 and 5.5 one head's sink is in reach of a one-key or 7-key row (LSE about 0 and
2.4) and the other's of a 129- to 300-key row (5.4 to 6.2): half of the rows.  -inf at H = 2 is covered by the bit-equality tests.

`assert_sinks_matter`: on the reference, at least ONE THIRD of the (sequence, head, row) triples of a case have a sink weight
exp(sink_h - LSE') in [0.05, 0.95].  A case whose sinks change nothing, or swamp everything, tests nothing.
"""
import itertools
import math

import torch

from kv_cache_check import (DEV, Cache, assert_close, attend, cu_of, fa, first_visible, i32, lse_ratio, poisoned_ff, ratios, reference,
                            reference_ragged, same_bits, visible)

NEG_INF = float("-inf")
SINKS8 = (NEG_INF, 0.0, 1.5, 3.0, 4.5, 5.5, 6.5, 8.0)
B, HKV, CAP = Cache.B, Cache.HKV, Cache.ROWS  # every case: two sequences, two K/V heads, three 128-key tiles of capacity
WINDOWS = (0, 7, 130)


def sinks_for(H):
    """the fp32 sink vector [H] of the parity cases (module docstring)"""
    n = len(SINKS8)
    if H >= n:
        return torch.tensor([SINKS8[h % n] for h in range(H)], dtype=torch.float32)
    step = n // H
    return torch.tensor([SINKS8[(1 + h * step) % n] for h in range(H)], dtype=torch.float32)


def _per_head(sinks, lse, ragged):
    """sinks [H] broadcast against an LSE: uniform [B, H, Sq], ragged (token-packed) [H, T]"""
    return sinks.double()[:, None] if ragged else sinks.double()[None, :, None]


def apply_sinks(O, lse, sinks, ragged=False):
    """(O', LSE') of the module docstring.  Uniform: O [B, H, Sq, d], lse [B, H, Sq]; ragged: O [T, H, d], lse [H, T]"""
    lse2 = torch.logaddexp(lse.double(), _per_head(sinks, lse, ragged))
    w = torch.exp(lse.double() - lse2)
    return O.double() * (w.transpose(0, 1) if ragged else w)[..., None], lse2


def sink_weights(lse2, sinks, ragged=False):
    """exp(sink_h - LSE'): the share of the row's softmax that the sink takes"""
    return torch.exp(_per_head(sinks, lse2, ragged) - lse2)


def assert_sinks_matter(lse2, sinks, ragged=False, owned=None, what=""):
    """at least a third of the case's (sequence, head, row) triples have a sink weight in [0.05, 0.95] (``owned``: bool [T], the tokens
    of a ragged case that a sequence owns); returns the share"""
    w = sink_weights(lse2, sinks, ragged)
    if owned is not None:
        w = w[:, owned]
    share = ((w >= 0.05) & (w <= 0.95)).double().mean().item()
    assert share >= 1.0 / 3.0, f"{what}: only {share:.2f} of the rows have a sink weight in [0.05, 0.95]"
    return share


def reference_sinks(Q, K, V, lens, causal, W, sinks, scale=None):
    """the uniform calls' reference with sinks: kv_cache_check.reference, then apply_sinks.  Returns (O' [B, H, Sq, d],
    LSE' [B, H, Sq], O, LSE) -- the last two without sinks"""
    O, lse = reference(Q, K, V, lens, causal, W, scale=scale)
    O2, lse2 = apply_sinks(O, lse, sinks)
    return O2, lse2, O, lse


def scores(Q, K, L, causal, W, scale=None):
    """float64 scores [H, Sq, L] of ONE sequence (Q [H, Sq, d], K [Hkv, cap, d]) with -inf where the row does not see the key"""
    H, Sq, d = Q.shape
    G = H // K.shape[0]
    S = (Q.double() @ K[:, :L].double().repeat_interleave(G, 0).transpose(-1, -2)) * (scale or 1.0 / d ** 0.5)
    return S.masked_fill(~visible(L, Sq, causal, W)[None], NEG_INF)


def brute_force(Q, K, V, lens, causal, W, sinks, scale=None):
    """float64 explicit softmax over the visible keys AND one extra column of score sinks[h] whose value row is 0: (O, LSE)"""
    Bq, H, Sq, d = Q.shape
    G = H // K.shape[1]
    O, lse = torch.zeros(Bq, H, Sq, d, dtype=torch.float64), torch.zeros(Bq, H, Sq, dtype=torch.float64)
    for b in range(Bq):
        L = int(lens[b])
        S = torch.cat([scores(Q[b], K[b], L, causal, W, scale), sinks.double()[:, None, None].expand(H, Sq, 1)], -1)
        v = torch.cat([V[b, :, :L].double().repeat_interleave(G, 0), torch.zeros(H, 1, d, dtype=torch.float64)], 1)
        lse[b] = torch.logsumexp(S, -1)
        O[b] = torch.softmax(S, -1) @ v
    return O, lse


def data(d, G, Sq, seed):
    """(Q [B, H, Sq, d], K, V [B, HKV, CAP, d]) bf16 N(0, 1) on the CPU"""
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(B, HKV * G, Sq, d, generator=g).to(torch.bfloat16)
    K, V = (torch.randn(B, HKV, CAP, d, generator=g).to(torch.bfloat16) for _ in range(2))
    return Q, K, V


def excess(O, lse, refO, refL):
    """(worst O error / tolerance, worst LSE error / tolerance) under kv_cache_check.assert_close's bounds: > 1 is a refusal"""
    r, lr = ratios(O, lse, refO, refL)
    return r.max().item(), lr.max().item()


LN2 = math.log(2.0)


# ---- what the GPU tests (test_sink.py, test_sink_extend.py) build and run alike ---------------------------------------------------
FORMS = ((None, False), (16, False), (None, True), (128, True))      # (page size or None, fp8): the four cache forms
FORM_IDS = ("contig-bf16", "paged16-bf16", "contig-fp8", "paged128-fp8")
LENS = ((1, 300), (129, 300))
f32, bf16 = torch.float32, torch.bfloat16


def queries(family, d, G, rows, seed):
    """bf16 N(0, 1) rows on the CPU: uniform [B, H, rows, d]; "varlen": rows is the per-sequence tuple, Q [T, H, d] packed by token"""
    g = torch.Generator().manual_seed(seed)
    shape = (sum(rows), HKV * G, d) if family == "varlen" else (B, HKV * G, rows, d)
    return torch.randn(*shape, generator=g).to(bf16)


def reference_of(family, cache, Q, rows, lens, causal, W, sinks):
    """(O', LSE', owned or None) of a case: uniform or ragged"""
    if family == "varlen":
        return reference_ragged(Q, cache.refK, cache.refV, rows, lens, causal, W, sinks)
    O2, lse2, _, _ = reference_sinks(Q, cache.refK, cache.refV, lens, causal, W, sinks)
    return O2, lse2, None


def close(O, lse, refO, refL, owned, what):
    """kv_cache_check.assert_close on the rows a sequence owns (all of them in a uniform call)"""
    if owned is None:
        assert_close(O, lse, refO, refL, what)
    else:
        assert_close(O.cpu()[owned], lse.cpu()[:, owned], refO[owned], refL[:, owned], what)


def run_parity(family, d, G, form, rows_list, run=True):
    """test 1: every case against the float64 reference -- causal and not, windows 0 / 7 / 130, forced splits 1 and 3 and the library's
    own choice, fp32 O held to the reference and bf16 O to the fp32 O rounded once.  run = False: the references and
    assert_sinks_matter alone (no GPU)"""
    page, fp8 = form
    cache = Cache(d, page, fp8, 900 + d + 7 * G)
    c = cache.device() if run else None
    sinks = sinks_for(HKV * G)
    for rows in rows_list:
        Q = queries(family, d, G, rows, 7 * d + 1000 * G + (sum(rows) if family == "varlen" else rows))
        cu = i32(cu_of(rows)) if family == "varlen" and run else None
        for lens, causal, W in itertools.product(LENS, (False, True), WINDOWS):
            what = f"{family} d{d} G{G} rows{rows} lens{lens} causal{int(causal)} window{W} {FORM_IDS[FORMS.index(form)]}"
            refO, refL, owned = reference_of(family, cache, Q, rows, lens, causal, W, sinks)
            assert_sinks_matter(refL, sinks, ragged=family == "varlen", owned=owned, what=what)
            if not run:
                continue
            for ns in (1, 3, 0):
                kw = dict(is_causal=causal, window=W, num_splits=ns, sinks=sinks.to(DEV))
                O, lse = attend(family, c, Q.to(DEV), i32(lens), cu, out_dtype=f32, **kw)
                close(O, lse, refO, refL, owned, f"{what} splits{ns}")
                Ob, lseb = attend(family, c, Q.to(DEV), i32(lens), cu, out_dtype=bf16, **kw)
                assert torch.equal(Ob, O.to(bf16)) and same_bits(lseb, lse), f"{what} splits{ns}: the bf16 O is not the fp32 O rounded once"


def run_neg_inf(family, d, G, form, rows):
    """test 2: sinks = -inf everywhere is the call without sinks, bit for bit: one split and three, windows 0 and 7, both masks, fp32
    and bf16 O.  (Chunked prefill at window 0: the WINDOW = true kernel at window 0 against the WINDOW = false one.)"""
    page, fp8 = form
    cache = Cache(d, page, fp8, 930 + d + G)
    c = cache.device()
    Q = queries(family, d, G, rows, 31 * d + G).to(DEV)
    cu = i32(cu_of(rows)) if family == "varlen" else None
    none = torch.full((HKV * G,), NEG_INF, dtype=f32, device=DEV)
    for lens, causal, W, ns, odt in itertools.product(LENS, (False, True), (0, 7), (1, 3), (f32, bf16)):
        kw = dict(is_causal=causal, window=W, num_splits=ns, out_dtype=odt)
        O, lse = attend(family, c, Q, i32(lens), cu, **kw)
        Os, lses = attend(family, c, Q, i32(lens), cu, sinks=none, **kw)
        what = f"{family} d{d} G{G} rows{rows} lens{lens} causal{int(causal)} window{W} splits{ns} {odt}"
        assert same_bits(Os, O), f"{what}: O with sinks = -inf is not the O without sinks"
        assert same_bits(lses, lse), f"{what}: LSE with sinks = -inf is not the LSE without sinks"


def probe_values(d):
    """index-coded V [B, HKV, CAP, d]: row k of (b, kvh) spells k, b and kvh in small integers (<= 11: exact in e4m3fn, and so are
    their halves in bf16 and fp32)"""
    k = torch.arange(CAP)
    V = torch.zeros(B, HKV, CAP, d)
    V[..., 0], V[..., 1], V[..., 2] = k // 32, (k // 4) % 8, k % 4
    V[..., 3] = torch.arange(B)[:, None, None] + 1.0
    V[..., 4] = torch.arange(HKV)[None, :, None] + 1.0
    for j in range(5, d):
        V[..., j] = (k + j) % 5
    return V.to(bf16)


def run_probe(family, d, G, form, causal, rows, lens_list, splits):
    """test 3: Q = 0, sinks = 0, window = 1 -- every row sees one key with score 0 and a sink of equal weight, so O is exactly half of
    that key's V row (fp32: bit for bit; bf16: its rounding, exact here) and LSE = ln 2.  Under the mask row i of Sq sees key
    max(len - Sq + i, 0); without it (Sq = 1) the sequence's last"""
    page, fp8 = form
    g = torch.Generator().manual_seed(77 + d)
    K = torch.randn(B, HKV, CAP, d, generator=g).to(bf16)
    cache = Cache(d, page, fp8, 950 + d, K=K, V=probe_values(d), descales=(torch.tensor([1.0, 0.5]), torch.tensor([0.5, 2.0])))
    assert torch.equal(cache.refV, probe_values(d).double() * (cache.vd.double()[None, :, None, None] if fp8 else 1.0))
    c = cache.device()
    H = HKV * G
    ragged = family == "varlen"
    Q = torch.zeros((sum(rows), H, d) if ragged else (B, H, rows, d), dtype=bf16, device=DEV)
    cu = cu_of(rows) if ragged else None
    zeros = torch.zeros(H, dtype=f32, device=DEV)
    for lens, ns, odt in itertools.product(lens_list, splits, (f32, bf16)):
        O, lse = attend(family, c, Q, i32(lens), i32(cu) if ragged else None, is_causal=causal, window=1, num_splits=ns, out_dtype=odt,
                        sinks=zeros)
        O, lse = O.cpu(), lse.cpu()
        for b in range(B):
            sq = rows[b] if ragged else rows
            for i in range(sq):
                key = max(lens[b] - sq + i, 0) if causal else lens[b] - 1
                want = (cache.refV[b, :, key] * 0.5).repeat_interleave(G, 0)                    # [H, d]
                got = (O[cu[b] + i] if ragged else O[b, :, i]).double()
                if not torch.equal(got, want.to(odt).double()):
                    h = int((got != want).any(-1).nonzero()[0])
                    named = (cache.refV[b, h // G] * 0.5 == got[h]).all(-1).nonzero().flatten().tolist()
                    raise AssertionError(f"{family} d{d} G{G} causal{int(causal)} lens{lens} splits{ns} {odt}: sequence {b} head {h} row {i} "
                                         f"should hold half of key {key}'s V row and holds that of key(s) {named}: {got[h, :6].tolist()}")
                l = (lse[:, cu[b] + i] if ragged else lse[b, :, i]).double()
                assert (lse_ratio(l, LN2) <= 1).all(), (family, lens, ns, b, i, l.tolist())


def run_range(family, d, G, form, rows):
    """test 4: sinks of +1e4, -1e4 and +-80 beside ordinary data, one split and three"""
    page, fp8 = form
    cache = Cache(d, page, fp8, 970 + d + G)
    c = cache.device()
    H = HKV * G
    Qc = queries(family, d, G, rows, 41 * d + G)
    Q = Qc.to(DEV)
    ragged = family == "varlen"
    cu = i32(cu_of(rows)) if ragged else None
    lens = LENS[1]
    for (causal, W), ns in itertools.product(((True, 0), (False, 130)), (1, 3)):
        kw = dict(is_causal=causal, window=W, num_splits=ns, out_dtype=f32)
        plain = attend(family, c, Q, i32(lens), cu, **kw)
        owned = reference_of(family, cache, Qc, rows, lens, causal, W, torch.zeros(H))[2]
        for value in (1e4, -1e4, 80.0, -80.0):
            sinks = torch.full((H,), value, dtype=f32)
            what = f"{family} d{d} G{G} rows{rows} causal{int(causal)} window{W} splits{ns} sinks {value:g}"
            O, lse = attend(family, c, Q, i32(lens), cu, sinks=sinks.to(DEV), **kw)
            assert torch.isfinite(O).all() and torch.isfinite(lse).all(), what
            refO, refL, _ = reference_of(family, cache, Qc, rows, lens, causal, W, sinks)
            close(O, lse, refO, refL, owned, what)
            lo, ll = O.cpu(), lse.cpu()
            if owned is not None:
                lo, ll = lo[owned], ll[:, owned]
            if value == 1e4:
                assert not lo.any(), f"{what}: O is not 0"
                assert (lse_ratio(ll, 1e4) <= 1).all(), f"{what}: LSE is not the sink"
            if value == -1e4:
                po, pl = plain[0].cpu(), plain[1].cpu()
                if owned is not None:
                    po, pl = po[owned], pl[:, owned]
                assert_close(lo, ll, po.double(), pl.double(), what + " against the call without sinks")


def run_paged_equal(family, d, rows, page, fp8, seed):
    """test 5: the paged call equals the contiguous call on the same bytes, bit for bit, with sinks"""
    G = 4
    cache = Cache(d, page, fp8, seed)
    paged, contig = cache.device(), cache.device(contiguous=True)
    Q = queries(family, d, G, rows, seed + 1).to(DEV)
    cu = i32(cu_of(rows)) if family == "varlen" else None
    sinks = sinks_for(HKV * G).to(DEV)
    for lens, causal, W, ns in itertools.product(LENS, (False, True), (0, 130), (1, 3)):
        kw = dict(is_causal=causal, window=W, num_splits=ns, sinks=sinks, out_dtype=f32)
        a, b = attend(family, paged, Q, i32(lens), cu, **kw), attend(family, contig, Q, i32(lens), cu, **kw)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), (lens, causal, W, ns)


def run_poison(family, d, rows, form, seed):
    """test 5: NaN bytes at and beyond every length and below the window (130 keys: a whole tile of the 300-key sequence) change no bit"""
    G, W = 4, 130
    cache = Cache(d, *form, seed)
    Q = queries(family, d, G, rows, seed + 1).to(DEV)
    cu = i32(cu_of(rows)) if family == "varlen" else None
    sinks = sinks_for(HKV * G).to(DEV)
    for lens in LENS:
        firsts = [first_visible(L, sq, W) for L, sq in zip(lens, rows if family == "varlen" else (rows,) * B)]
        assert max(firsts) > 128
        clean = cache.device()
        dirty = cache.device(poisoned_ff(cache.cK, lens, firsts), poisoned_ff(cache.cV, lens, firsts))
        for causal, ns in itertools.product((False, True), (1, 3)):
            kw = dict(is_causal=causal, window=W, num_splits=ns, sinks=sinks, out_dtype=f32)
            a, b = attend(family, clean, Q, i32(lens), cu, **kw), attend(family, dirty, Q, i32(lens), cu, **kw)
            assert torch.isfinite(b[0]).all() and same_bits(a[0], b[0]) and same_bits(a[1], b[1]), (lens, causal, ns)


def run_graph(step, lens, start, Sq, sinks, reference, O):
    """test 6: `step` (kv_lens += Sq; append; attend with sinks -> (O, LSE)) captured once -- a single chain of kernels -- and replayed
    three times; the sinks tensor is overwritten between the replays and each replay is held to reference(lens now, sinks now)"""
    H = sinks.shape[0]
    step()                                     # every kernel of the step has run once before the capture
    torch.cuda.synchronize()
    lens.copy_(i32(start))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse = step()
    lens.copy_(i32(start))
    seen = []
    for r, vec in enumerate([sinks_for(H), torch.full((H,), NEG_INF), sinks_for(H).flip(0) + 1.0]):
        sinks.copy_(vec)
        graph.replay()
        torch.cuda.synchronize()
        now = lens.tolist()
        assert now == [s + (r + 1) * Sq for s in start]
        refO, refL = reference(now, vec)
        assert_close(O, lse, refO, refL, f"replay {r}")
        seen.append(O.clone())
    assert not torch.equal(seen[0], seen[2])


class Recorder:
    """``fa.lib()`` as the fronts see it: the real library, every attribute fetched from it noted by name"""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)


def run_routing(monkeypatch, front, args, kw, sinks, plan, launch):
    """test 7: with sinks the front fetches [plan, workspace size, launch]; without them the same two and no sink entry point"""
    rec = Recorder(fa.lib())
    monkeypatch.setattr(fa, "lib", lambda: rec)
    O, lse = getattr(fa, front)(*args, sinks=sinks, return_lse=True, **kw)
    assert rec.names == [plan, "flash_attention_decode_workspace_size", launch]
    del rec.names[:]
    getattr(fa, front)(*args, return_lse=True, **kw)
    assert len(rec.names) == 3 and rec.names[:2] == [plan, "flash_attention_decode_workspace_size"] and "sink" not in rec.names[2]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(O.float()).all()) and bool(torch.isfinite(lse).all())
