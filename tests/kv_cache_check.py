"""Checker shared by every test of the K/V-cache calls' read side (decode, chunked prefill, the ragged call, windows, fp8 and paged
caches, sinks, tree masks): the visibility rule, the project's float64 ground truth under it, the element-wise criterion, and the data
and cache layouts the tests build alike.  Plain torch on the CPU for everything but `assert_close`, `Cache.device()` and `attend`.

Rule.  `visible(L, Sq, causal, W, words)` is the contract of include/flash_attention.h, written once.  The Sq rows are the last rows of
the L keys (bottom-right aligned).  With base = L - Sq, lim_i = max(base + i + 1, 1) and lo_i = max(lim_i - W, 0) (W = 0: no window,
lo_i = 0), row i sees key k iff lo_i <= k < lim_i (causal) or lo_i <= k < L (not causal: the left edge still follows the row's own
position).  Under a tree mask (`words`: the sequence's Sq unsigned 64-bit patterns; the call is causal) a visible key is also one of
the prefix (k < base), or names a node whose bit k - base is set in the row's word, or is the row's own (k == lim_i - 1).
`first_visible` is lo_0, the lowest key any row sees: keys below it are outside the library's contract and the tests poison them.

Reference.  `reference()`: the explicit softmax in float64 over the keys each row sees, grouped-query attention by
`repeat_interleave` of the K/V heads.  K and V may be bf16, fp32 or float64 -- an fp8 cache comes in dequantised (`dequantise()`: exact
in float64), so the error of quantising is never part of a comparison.  `sinks` go on at the end (sink_check.apply_sinks);
`vis(b, h, L)` replaces the rule by a visibility of the caller's own per (sequence, head).  `reference_ragged()`: the same on every
sequence of a token-packed batch as a batch of one.

Criterion.  `ratios()`: every element's error over the project's stated bound, 1e-3 + 1e-3 |ref| on O and 2e-4 + 2e-6 |ref| on the LSE
(`lse_ratio()`); a ratio that is not <= 1 -- a NaN included -- is a refusal.  `assert_close()` asserts it of every element, both
results finite, and prints the worst ratio of each (and the worst absolute LSE error, the figure the logs under profiles/ carry).
`assert_close_with_score_noise()` is the wider bound of the custom-scale cases.
"""
import torch

import __graft_entry__ as entry

fa = entry.load_package()

DEV = "cuda:0"
CAP = fa.FA_DECODE_MAX_SPLITS
TILE = 128   # fa_decode_plan.kv_block_rows
F8 = getattr(torch, "float8_e4m3fn", None)   # (the bf16 tests do not need it)


def randn(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def i32(v):
    """a list of ints (or None) as the int32 device tensor the calls take"""
    return None if v is None else torch.tensor(list(v), dtype=torch.int32).to(DEV)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def cu_of(sq):
    cu = [0]
    for s in sq:
        cu.append(cu[-1] + s)
    return cu


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def first_visible(L, Sq, W):
    """lo_0: the lowest key any of the Sq rows sees of a sequence of L keys under the window W (0: none)"""
    return max(max(L - Sq + 1, 1) - W, 0) if W > 0 else 0


def words_tensor(words):
    """rows of unsigned 64-bit patterns (Python ints) -> the int64 tensor (CPU) of the same bits"""
    return torch.tensor([[w - (1 << 64) if w >> 63 else w for w in row] for row in words], dtype=torch.int64)


def visible(L, Sq, causal, W=0, words=None):
    """bool [Sq, L]: row i sees key k (module docstring); at least key 0"""
    k = torch.arange(L)[None, :]
    if W <= 0 and not causal:
        vis = torch.ones(Sq, L, dtype=torch.bool) & (k >= 0)
    elif W <= 0:
        last = (L - Sq + torch.arange(Sq)).clamp(min=0)[:, None]
        vis = k <= last
    else:
        limc = (L - Sq + 1 + torch.arange(Sq)).clamp(min=1)[:, None]
        lo = (limc - W).clamp(min=0)
        vis = (k >= lo) & (k < (limc if causal else L))
    if words is None:
        return vis
    assert causal, "a tree call is causal"
    base = L - Sq
    own = (base + torch.arange(Sq)).clamp(min=0)[:, None]                         # lim_i - 1
    node = (k - base).clamp(min=0, max=63)                                        # (a visible key's node is below Sq <= 64)
    bit = ((words_tensor([words])[0][:, None] >> node) & 1).bool()
    return vis & ((k < base) | bit | (k == own))


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _with_sinks(O, lse, sinks, ragged=False):
    if sinks is None:
        return O, lse
    from sink_check import apply_sinks      # (sink_check is built on this module)
    return apply_sinks(O, lse, sinks, ragged)


def reference(Q, K, V, lens, causal, W=0, *, words=None, sinks=None, vis=None, scale=None):
    """float64 explicit softmax over the visible keys of each sequence (CPU tensors; K, V [B, Hkv, capacity, d] in bf16, fp32 or
    float64: a paged cache gathered, an fp8 one dequantised), then the sinks: O [B, H, Sq, d], LSE [B, H, Sq].  lens None: every
    sequence fills the capacity; words [B][Sq]: tree masks; vis(b, h, L) -> bool [Sq, L]: another visibility than the rule's"""
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
        if vis is None:
            M = visible(L, Sq, causal, W, None if words is None else words[b])[None]
        else:
            M = torch.stack([vis(b, h, L) for h in range(H)])
        S = S.masked_fill(~M, float("-inf"))
        lse[b] = torch.logsumexp(S, -1)
        O[b] = torch.softmax(S, -1) @ v
    return _with_sinks(O, lse, sinks)


def packed(refs, sq, T, H, d):
    """per-sequence references [(O [H, sq_b, d], LSE [H, sq_b]) or None] as packed (O [T, H, d], LSE [H, T], owned bool [T])"""
    O, lse, owned = torch.zeros(T, H, d, dtype=torch.float64), torch.zeros(H, T, dtype=torch.float64), torch.zeros(T, dtype=torch.bool)
    cu = cu_of(sq)
    for b, r in enumerate(refs):
        if r is not None:
            O[cu[b]:cu[b + 1]] = r[0].transpose(0, 1)
            lse[:, cu[b]:cu[b + 1]] = r[1]
            owned[cu[b]:cu[b + 1]] = True
    return O, lse, owned


def reference_ragged(Q, K, V, sq, lens, causal, W=0, sinks=None, scale=None):
    """the ragged call's: `reference` on every sequence as a batch of one -- its length clamped into [1, capacity] as the library
    clamps it, None for an idle slot (sq_b = 0) -- packed by token, then the sinks.  Q [T, H, d] packed by token, K / V
    [B, Hkv, capacity, d]; returns (O [T, H, d], LSE [H, T], owned bool [T]: the tokens a sequence owns)"""
    T, H, d = Q.shape
    cu, refs = cu_of(sq), []
    for b, s in enumerate(sq):
        if s == 0:
            refs.append(None)
            continue
        L = min(max(int(lens[b]), 1), K.shape[2])
        O, lse = reference(Q[cu[b]:cu[b + 1]].transpose(0, 1)[None], K[b:b + 1], V[b:b + 1], [L], causal, W, scale=scale)
        refs.append((O[0], lse[0]))
    O, lse, owned = packed(refs, sq, T, H, d)
    return _with_sinks(O, lse, sinks, ragged=True) + (owned,)


# ---- the criterion -------------------------------------------------------------------------------------------------------------------
def lse_ratio(lse, refL):
    """|LSE - ref| / (2e-4 + 2e-6 |ref|), float64; refL a tensor or a number"""
    refL = torch.as_tensor(refL, dtype=torch.float64)
    return (lse.double() - refL).abs() / (2e-4 + 2e-6 * refL.abs())


def ratios(O, lse, refO, refL):
    """(|O - ref| / (1e-3 + 1e-3 |ref|), |LSE - ref| / (2e-4 + 2e-6 |ref|)), float64 tensors of the shapes of O and of the LSE: an
    element is within the project's stated bound iff its ratio is <= 1 (a NaN is not)"""
    return (O.double() - refO).abs() / (1e-3 + 1e-3 * refO.abs()), lse_ratio(lse, refL)


def assert_close(O, lse, refO, refL, what=""):
    O, lse = O.double().cpu(), lse.double().cpu()
    assert torch.isfinite(O).all() and torch.isfinite(lse).all(), what
    r, lr = ratios(O, lse, refO, refL)
    lerr = (lse - refL).abs()
    print(f"{what}: worst O error / tolerance {r.max().item():.3f}, worst LSE error / tolerance {lr.max().item():.3f}"
          f" ({lerr.max().item():.2e})")
    assert (r <= 1).all(), f"{what}: {int((r > 1).sum())} elements outside 1e-3 + 1e-3|ref|, worst ratio {r.max().item():.3f}"
    assert (lr <= 1).all(), f"{what}: LSE error {lerr.max().item():.3e}"


def scores_max(Q, K, lens, causal, scale):
    """largest |scale * score| over the visible (row, key) pairs"""
    B, H, Sq, d = Q.shape
    G = H // K.shape[1]
    worst = 0.0
    for b in range(B):
        L = K.shape[2] if lens is None else int(lens[b])
        S = (Q[b].double() @ K[b, :, :L].double().repeat_interleave(G, 0).transpose(-1, -2)) * scale
        worst = max(worst, S.abs().masked_fill(~visible(L, Sq, causal)[None], 0.0).max().item())
    return worst


def assert_close_with_score_noise(O, lse, Q, K, V, lens, causal, scale, what):
    """the stated 1e-3 + 1e-3 |ref| plus the fp32 score noise through exp(), 8 max(smax, 4) 2^-23 ref_abs (ref_abs: the reference on
    |V|); the LSE within 1e-5 + 16 max(smax, 4) 2^-23 + 2^-22 |LSE| -- the fp32 terms of tests/fuzz_gpu.py"""
    refO, refL = reference(Q, K, V, lens, causal, scale=scale)
    ref_abs, _ = reference(Q, K, V.abs(), lens, causal, scale=scale)
    smax = max(scores_max(Q, K, lens, causal, scale), 4.0)
    O, lse = O.double().cpu(), lse.double().cpu()
    assert torch.isfinite(O).all() and torch.isfinite(lse).all(), what
    err, tol = (O - refO).abs(), 1e-3 + 1e-3 * refO.abs() + 8 * smax * 2.0 ** -23 * ref_abs
    lerr, ltol = (lse - refL).abs(), 1e-5 + 16 * smax * 2.0 ** -23 + 2.0 ** -22 * refL.abs()
    print(f"{what}: smax {smax:.1f}, LSE up to {refL.abs().max().item():.1f}, worst O error / tolerance {(err / tol).max().item():.3f}, "
          f"worst LSE error / tolerance {(lerr / ltol).max().item():.3f}")
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} elements of O out, worst ratio {(err / tol).max().item():.3f}"
    assert (lerr <= ltol).all(), f"{what}: LSE worst ratio {(lerr / ltol).max().item():.3f}"


# the (scale, factor on Q and K) of the custom-scale cases: 0.02, 3/sqrt(d), 1 with the scores kept O(1); Q and K times 3 and times 12
SCALES = {"small": lambda d: (0.02, 1.0), "large": lambda d: (3.0 / d ** 0.5, 1.0), "one": lambda d: (1.0, d ** -0.25),
          "boost3": lambda d: (1.0 / d ** 0.5, 3.0), "boost12": lambda d: (1.0 / d ** 0.5, 12.0)}


# ---- paged caches --------------------------------------------------------------------------------------------------------------------
def gather(pool, table):
    """[P, Hkv, page, d] pool, [B, max_pages] table (in range) -> the contiguous cache [B, Hkv, max_pages * page, d]"""
    B, n = table.shape
    P, Hkv, page, d = pool.shape
    return pool[table.long()].permute(0, 2, 1, 3, 4).reshape(B, Hkv, n * page, d).contiguous()


def scatter(cache, table, page, spare=5):
    """the pool [P, Hkv, page, d] that `table` [B, n] gathers back into `cache` [B, Hkv, n * page, d]; P = B * n + spare"""
    B, Hkv, cap, d = cache.shape
    n = cap // page
    pool = torch.zeros((B * n + spare, Hkv, page, d), dtype=cache.dtype, device=cache.device)
    pool[table.long().reshape(-1)] = cache.reshape(B, Hkv, n, page, d).permute(0, 2, 1, 3, 4).reshape(B * n, Hkv, page, d)
    return pool


def random_table(B, n, seed, spare=5):
    return torch.randperm(B * n + spare, generator=torch.Generator().manual_seed(seed))[:B * n].reshape(B, n).to(torch.int32)


def boundary_lengths(page, cap):
    """around every boundary: the page, the 128-key tile, the capacity"""
    return sorted({max(1, min(L, cap)) for L in (1, page - 1, page, page + 1, 127, 128, 129, cap - 3, cap)})


def max_pages_of(page):
    return max(3, 320 // page)     # capacities 320, 320, 384, 768: more than one tile, more than two pages


def paged_layout(page, d, spare=7):
    """(P, table, lens) of the paged sweeps: one sequence per boundary length, pools of P pages -- `spare` more than the sequences
    use -- and a random permutation as the table.  The pools are randn((P, Hkv, page, d), 1000 / 2000 + page + d) in the caller's type"""
    n = max_pages_of(page)
    lens = boundary_lengths(page, n * page)
    B = len(lens)
    P = B * n + spare
    g = torch.Generator().manual_seed(3000 + page + d)
    table = torch.randperm(P, generator=g)[:B * n].reshape(B, n).to(torch.int32)
    return P, table, lens


# ---- fp8 caches, handled as uint8 tensors and viewed as float8_e4m3fn at the call ------------------------------------------------------
def quantise(x):
    """x fp32 [*, Hkv, rows, d] (K/V heads in dimension 1) -> (bytes uint8 of the same shape, descale fp32 [Hkv] = amax / 448).
    torch's cast gives NaN beyond 448, not saturation: clamp, and check"""
    ds = (x.abs().amax(dim=(0, 2, 3)) / 448.0).float()
    b = (x / ds[None, :, None, None]).clamp(-448, 448).to(F8).view(torch.uint8)
    assert ((b & 0x7F) != 0x7F).all(), "NaN among the quantised bytes"
    return b, ds


def dequantise(b, ds):
    return b.view(F8).float().double() * ds.double()[None, :, None, None]


# ---- poison: what a call must never read ---------------------------------------------------------------------------------------------
def poisoned_ff(stored, lens, firsts):
    """a copy of a stored contiguous cache with 0xFF bytes (NaN in bf16 and in e4m3fn) at and beyond every sequence's length and below
    its first visible key"""
    out = stored.clone()
    raw = out.view(torch.uint8)
    for b, (L, first) in enumerate(zip(lens, firsts)):
        raw[b, :, L:] = 0xFF
        raw[b, :, :first] = 0xFF
    return out


def poisoned_nan_inf(K, V, lens, firsts, fp8):
    """copies of a contiguous K and V with alternating NaN / inf keys (fp8, as uint8: the NaN bytes 0x7F / 0xFF) below every sequence's
    first visible key and at and beyond its length"""
    nan, inf = float("nan"), float("inf")
    Kp, Vp = K.clone(), V.clone()
    for b, (L, f) in enumerate(zip(lens, firsts)):
        for lo, hi in ((0, f), (L, K.shape[2])):
            if fp8:
                Kp[b, :, lo:hi:2], Kp[b, :, lo + 1:hi:2] = 0x7F, 0xFF
                Vp[b, :, lo:hi:2], Vp[b, :, lo + 1:hi:2] = 0xFF, 0x7F
            else:
                Kp[b, :, lo:hi:2], Kp[b, :, lo + 1:hi:2] = nan, inf
                Vp[b, :, lo:hi:2], Vp[b, :, lo + 1:hi:2] = -inf, nan
    return Kp, Vp


# ---- the four cache forms and the fronts that read them --------------------------------------------------------------------------------
class Cache:
    """A K/V cache [B, HKV, ROWS, d] of N(0, 1) data in one of the four forms.  cK, cV: what is stored, contiguous, on the CPU (bf16, or
    the e4m3fn bytes as uint8 with the descales kd, vd = amax / 448); refK, refV: the float64 logical cache the references read"""
    B, HKV, ROWS = 2, 2, 384                  # every case: two sequences, two K/V heads, three 128-key tiles of capacity

    def __init__(self, d, page, fp8, seed, K=None, V=None, descales=None):
        B, HKV, ROWS, bf16 = self.B, self.HKV, self.ROWS, torch.bfloat16
        g = torch.Generator().manual_seed(seed)
        K = torch.randn(B, HKV, ROWS, d, generator=g).to(bf16) if K is None else K
        V = torch.randn(B, HKV, ROWS, d, generator=g).to(bf16) if V is None else V
        self.d, self.page, self.fp8, self.kd, self.vd = d, page, fp8, None, None
        if fp8:
            if descales is None:
                (self.cK, self.kd), (self.cV, self.vd) = quantise(K.float()), quantise(V.float())
            else:       # values that are e4m3fn numbers as they stand
                self.kd, self.vd = descales
                self.cK, self.cV = K.float().to(F8).view(torch.uint8), V.float().to(F8).view(torch.uint8)
            self.refK, self.refV = dequantise(self.cK, self.kd), dequantise(self.cV, self.vd)
        else:
            self.cK, self.cV, self.refK, self.refV = K, V, K.double(), V.double()
        self.table = random_table(B, ROWS // page, seed + 2) if page else None

    def device(self, cK=None, cV=None, contiguous=False):
        """the device tensors the fronts take, of the stored bytes (or of cK, cV in their place: a poisoned copy): K, V -- the cache,
        or its pools under the table -- table, and the descales as keywords.  contiguous: the contiguous form of the same bytes"""
        out = dict(table=None, ds={})
        kv = [self.cK if cK is None else cK, self.cV if cV is None else cV]
        if self.page and not contiguous:
            flat = kv
            kv = [scatter(t, self.table, self.page) for t in flat]
            assert all(same_bits(gather(p, self.table), t) for p, t in zip(kv, flat))      # (bits: a poisoned copy holds NaNs)
            out["table"] = self.table.to(DEV)
        out["K"], out["V"] = ((t.view(F8) if self.fp8 else t).to(DEV) for t in kv)
        if self.fp8:
            out["ds"] = dict(k_descale=self.kd.to(DEV), v_descale=self.vd.to(DEV))
        return out


def attend(family, c, Q, lens, cu=None, **kw):
    """(O, LSE) of one call through the Python fronts: family "decode", "extend" (the _window fronts: window None / 0 is the plain call)
    or "varlen" (Q packed by token, cu the offsets); c: Cache.device()"""
    paged = c["table"] is not None
    name = {"decode": "flash_attention_decode", "extend": "flash_attention_extend", "varlen": "flash_attention_extend"}[family] \
        + ("_paged" if paged else "") + ("_varlen" if family == "varlen" else "") + ("" if family == "decode" else "_window")
    args = [Q, c["K"], c["V"]] + ([c["table"]] if paged else []) + ([cu] if family == "varlen" else [])
    return getattr(fa, name)(*args, lens, return_lse=True, **c["ds"], **kw)
