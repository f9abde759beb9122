"""long_probe.py's index-coded problems for the K/V-CACHE calls -- flash_attention_decode*, flash_attention_extend*, the ragged *_varlen
calls and the _window forms, on contiguous or paged, bf16 or e4m3fn caches (no tests in here; tests/test_long_cache_probe.py proves the
instrument on the CPU, tests/test_long_cache.py uses it on the GPU).

The coding is long_probe.build's: key j holds +1 / -1 at column b < nb by bit b of code(j) = base + j, a bf16 query holds +-128 by the
bits of its target's code and 128 nb - 64 at column nb, the scale is format_probe.PREFILL_SCALE(0) (c = 1: every score an exact integer
in exp2 units), V comes from long_probe.v_rows.  What this family adds:

  anchors   key 0 and every key j with j % A == 37 % A (A = 64; 37 is no tile, page or 16-key-group edge) are ANCHORS: K is 0 but for a
            1 at column nb, V is 0, never a target.  Every window of W >= A keys and every row's range then holds one.  In exp2 units the
            target scores 128 nb, an anchor 128 nb - 64, every other key <= 128 nb - 256.
  ranges    row i of a sequence of `len` keys and Sq rows sees lo_i <= k < lim_i with limC_i = max(len - Sq + i + 1, 1),
            lo_i = max(limC_i - W, 0) (W = 0: 0), lim_i = limC_i (causal) or len: ranges(), which tests/test_long_cache_probe.py holds
            to kv_cache_check.visible (that one builds a [Sq, len] matrix: not at 2^20 keys).
  closed    a row whose target is visible: the target weighs 1 and the k anchors 2^-64 each: l = 1 in fp32, O = V[target] BIT FOR BIT,
  forms     LSE = ln 2 * 128 nb.  A row whose target is hidden -- above lim_i, below lo_i, at or beyond len -- has the anchors for its
            best keys: O = +0 exactly, LSE = ln 2 * (128 nb - 64) + ln k, k the anchors in [lo_i, lim_i) (anchors_below()).  Every row has
            one of the two: plan_targets() asserts that the range holds the target or an anchor.
  why it    the kernel (csrc/decode_bf16.hip.h) keeps a running maximum per wave: after the target every earlier sum is scaled by
  is exact  2^-64 and l = 1 + k 2^-64 = 1; a wave or a split without target and anchor has a maximum <= 128 nb - 256 and merges with weight
            exp2(<= -192) = 0 against finite V; a split with anchors alone has O = 0 (V = 0) and the combine weight 2^-64 k, which
            vanishes next to the target's 1.  emulate() is that arithmetic in fp32.
  fp8       the cache holds K8 = +-2^j (j by K/V head) and k_descale = 2^-j, V8 = the integers of v_rows and v_descale a power of two,
            neither 1, different per K/V head: the logical K is +-1 as above, the expected O is fp32(V8) * v_descale[kvh] rounded once.
  V salt    V[j] of sequence b, K/V head kvh is v_rows(code(j), kvh + Hkv * owner): a row read from another sequence, head or page
            differs in about 16 columns of 17.  V at and beyond len (inside the capacity) is NaN, K there is coded: a row that targets
            such a key reads +0 only if the length is respected by the mask AND by the record count.
  paged     the block table is a seeded permutation into a pool with more pages than any sequence uses; pages no sequence owns hold NaN
            bytes, table entries at and beyond the length's last page hold out-of-range values, and under a window the entries of pages
            wholly below row 0's left edge hold arbitrary int32 (those pages are not in the pool at all).  Contiguous caches hold NaN
            below row 0's left edge.
  targets   plan_targets(): seeded; half within NEAR keys of the row's diagonal, half uniform over its range, about every seventh hidden
            (alternating: 1 .. NEAR above lim_i, 1 .. NEAR below lo_i, at or beyond len).  Forced places (forced_places(); each one that
            exists in a case is in `named` and in the failure text): first and last key of the length, lo_i and lim_i - 1 of the first and
            last row of every row block (and lo_i - 1, lim_i as hidden targets), both sides of every split boundary
            t0 = tlo + (ntb - tlo) s / ns of every row block (extend_window_check.block_range), both sides of a page seam, first and last
            page of the table, both sides of byte 2^30 and 2^31 - 2^20 of a contiguous head, a page on each side of byte 2^32 of a pool.
            A forced place needs a row that sees it (a split boundary: a row of THAT block); decode has H Sq rows per sequence, so the
            places are dealt over as many ROUNDS (one Q, one call each) as it takes.
"""
import dataclasses
import math

import numpy as np
import torch

import long_probe as lp
import extend_window_check as ewc

fa, fp = lp.fa, lp.fp
bf, f32 = torch.bfloat16, torch.float32
FP8 = fp.FP8
TILE, A, E, UNIT, NEAR, CHUNK = 128, 64, 64, 128, 300, 2 ** 18
LN2 = fp.LN2_F32
KD, VD = (0.25, 2.0, 0.5, 8.0), (0.5, 4.0, 2.0, 0.25)        # descales by K/V head: powers of two, none of them 1
CANARY = 12352.0                                               # bf16-exact; no V * descale reaches it
BYTE_LINES = lp.BYTE_LINES


@dataclasses.dataclass(frozen=True)
class Spec:
    """one problem: `seqs` = ((rows, length), ...) per sequence against caches of `cap` keys.  kind: decode / extend (uniform: every
    sequence has the same row count) / varlen (token-packed, `pad` trailing rows of total_q that no sequence owns).  page > 0: paged with
    `spare` pages more than the sequences use (or `pool_pages` in all); share: sequence 1 names the first `share` pages of sequence 0."""
    kind: str
    seqs: tuple
    cap: int
    d: int = 128
    H: int = 8
    Hkv: int = 2
    causal: bool = True
    W: int = 0
    fp8: bool = False
    page: int = 0
    spare: int = 64
    pool_pages: int = 0
    share: int = 0
    pad: int = 0
    base: int = 0
    A: int = A
    seed: int = 0

    @property
    def G(self):
        return self.H // self.Hkv

    @property
    def total_q(self):
        return sum(s for s, _ in self.seqs) + self.pad

    @property
    def esz(self):
        return 1 if self.fp8 else 2

    @property
    def nb(self):
        return max(2, (self.base + self.cap - 1).bit_length())

    def length(self, b):
        return min(max(self.seqs[b][1], 1), self.cap)

    def first(self, b):
        """the lowest key any row of sequence b sees (row 0's left edge)"""
        sq, L = self.seqs[b][0], self.length(b)
        return max(max(L - sq + 1, 1) - self.W, 0) if self.W > 0 and sq > 0 else 0

    def form(self):
        return f"{self.kind}{'_window' if self.W else ''} {'paged' if self.page else 'contiguous'} {'fp8' if self.fp8 else 'bf16'} d {self.d}"


def residue(a):
    return 37 % a


def is_anchor(j, a=A):
    return (j == 0) | (j % a == residue(a))


def anchors_below(x, a=A):
    """the anchors among the keys [0, x) (numpy or torch integers)"""
    return (x > 0) * 1 + ((x - residue(a) + a - 1) // a) * (x > residue(a))


def ranges(L, Sq, causal, W):
    """(lo, lim) int64 numpy [Sq]: row i sees lo_i <= k < lim_i (module docstring; the header's rule)"""
    limc = np.maximum(L - Sq + np.arange(Sq, dtype=np.int64) + 1, 1)
    return (np.maximum(limc - W, 0) if W > 0 else np.zeros(Sq, dtype=np.int64)), (limc if causal else np.full(Sq, L, dtype=np.int64))


def owner(spec, b, j):
    """the sequence whose data key j of sequence b holds (shared pages: sequence 0's)"""
    return np.where((b == 1) & (j < spec.share * spec.page), 0, b) if spec.share else b


# ---- the caches ----------------------------------------------------------------------------------------------------------------------
def _nan_like(shape, spec, device):
    if spec.fp8:
        return torch.full(shape, 0x7F, dtype=torch.uint8, device=device).view(FP8)
    return torch.full(shape, float("nan"), dtype=bf, device=device)


def _store(T, idx, rows, spec):
    """T[idx] = rows (fp32, exact in the cache's type; NaN allowed), fp8 through the bytes"""
    if spec.fp8:
        b = rows.clamp(-448, 448).to(FP8).view(torch.uint8)
        T.view(torch.uint8)[idx] = torch.where(torch.isnan(rows), torch.full_like(b, 0x7F), b)
    else:
        T[idx] = rows.to(bf)


def key_rows(spec, j, kvh, own, L, device):
    """(K, V) fp32 [len(j), d] as the CACHE holds them for the keys j (int64 tensor) of a sequence of L keys: K8 / V8 for fp8"""
    d, nb = spec.d, spec.nb
    code = spec.base + j
    K = torch.zeros((len(j), d), dtype=f32, device=device)
    K[:, :nb] = lp.bits(code, nb).float()
    anc = is_anchor(j, spec.A)
    K[anc] = 0
    K[anc, nb] = 1
    V = lp.v_rows(code, kvh + spec.Hkv * own, d).float()
    V[anc] = 0
    V[j >= L] = float("nan")
    if spec.fp8:
        K = K / KD[kvh % 4]
    return K, V


def layout(spec):
    """paged: (P, table int64 numpy [B, max_pages] with -1 where no page is owned, (first page, pages used) per sequence)"""
    B, page = len(spec.seqs), spec.page
    n = spec.cap // page
    used = []
    for b, (sq, _) in enumerate(spec.seqs):
        used.append((spec.first(b) // page, -(-spec.length(b) // page)) if (sq > 0 or spec.kind != "varlen") else (0, 0))
    need = sum(u1 - u0 for u0, u1 in used)
    P = spec.pool_pages or need + spec.spare
    assert P >= need + 1
    perm = np.random.RandomState(7000 + spec.seed).permutation(P)
    table, at = -np.ones((B, n), dtype=np.int64), 0
    for b, (u0, u1) in enumerate(used):
        table[b, u0:u1] = perm[at:at + u1 - u0]
        at += u1 - u0
    if spec.share:
        assert used[0][0] == 0 == used[1][0] and spec.share <= min(used[0][1], used[1][1])
        table[1, :spec.share] = table[0, :spec.share]
    return P, table, used


def build_cache(spec, device="cpu"):
    """-> dict(K, V: [B, Hkv, cap, d] or pools [P, Hkv, page, d]; table int32 [B, max_pages] or None; phys (the table with -1 at unowned
    entries, numpy); kv_lens int32 [B]; kd, vd fp32 [Hkv] or None)"""
    assert spec.cap % TILE == 0 or not spec.page
    assert spec.nb <= 24 and spec.nb + 1 <= spec.d and spec.base % 2 == 0 and (not spec.fp8 or FP8 is not None)
    B, Hkv, d = len(spec.seqs), spec.Hkv, spec.d
    out = dict(kv_lens=torch.tensor([L for _, L in spec.seqs], dtype=torch.int32, device=device), table=None, phys=None, kd=None, vd=None)
    if spec.fp8:
        out["kd"] = torch.tensor([KD[h % 4] for h in range(Hkv)], dtype=f32, device=device)
        out["vd"] = torch.tensor([VD[h % 4] for h in range(Hkv)], dtype=f32, device=device)
    if spec.page:
        P, phys, used = layout(spec)
        K, V = _nan_like((P, Hkv, spec.page, d), spec, device), _nan_like((P, Hkv, spec.page, d), spec, device)
        g = np.random.RandomState(7100 + spec.seed)
        junk = np.where(g.randint(0, 2, phys.shape) == 0, g.randint(P, 2 ** 31 - 1, phys.shape), -g.randint(1, 2 ** 31 - 1, phys.shape))
        for b, (u0, u1) in enumerate(used):
            junk[b, u1:] = np.where(np.arange(u1, phys.shape[1]) % 2 == 0, P + np.arange(u1, phys.shape[1]), -1 - np.arange(u1, phys.shape[1]))
        out["table"] = torch.tensor(np.where(phys >= 0, phys, junk), dtype=torch.int32, device=device)
        out["phys"], out["P"] = phys, P
    else:
        K, V = _nan_like((B, Hkv, spec.cap, d), spec, device), _nan_like((B, Hkv, spec.cap, d), spec, device)
    for b, (sq, _) in enumerate(spec.seqs):
        if sq == 0 and spec.kind == "varlen":
            continue                                            # an idle slot: neither its length nor its table row is read
        L = spec.length(b)
        if spec.page:
            u0, u1 = used[b]
            if spec.share and b == 1:
                u0 = spec.share                                 # (sequence 0 wrote the shared pages)
            r0, r1 = u0 * spec.page, u1 * spec.page
        else:
            r0, r1 = spec.first(b), spec.cap
        for c0 in range(r0, r1, CHUNK):
            j = torch.arange(c0, min(c0 + CHUNK, r1), device=device)
            for kvh in range(Hkv):
                Kr, Vr = key_rows(spec, j, kvh, b, L, device)
                if spec.page:
                    pages = torch.as_tensor(phys[b, c0 // spec.page:(c0 + len(j)) // spec.page], device=device)
                    _store(K, (pages, kvh), Kr.view(-1, spec.page, d), spec)
                    _store(V, (pages, kvh), Vr.view(-1, spec.page, d), spec)
                else:
                    _store(K, (b, kvh, slice(c0, c0 + len(j))), Kr, spec)
                    _store(V, (b, kvh, slice(c0, c0 + len(j))), Vr, spec)
    out["K"], out["V"] = K, V
    return out


# ---- targets --------------------------------------------------------------------------------------------------------------------------
def _free_of_anchor(k, a, step=1):
    while is_anchor(k, a):
        k += step
    return k


def pool_line_pages(spec, phys_row):
    """the logical pages of a table row whose pool pages lie closest below and at / above byte 2^32 of the pool ({} if it has no such)"""
    line = 2 ** 32 // (spec.Hkv * spec.page * spec.d * spec.esz)
    own = np.nonzero(phys_row >= 0)[0]
    below, above = own[phys_row[own] < line], own[phys_row[own] >= line]
    out = {}
    if len(below) and len(above):
        out["pool page below byte 2^32"] = int(below[np.argmax(phys_row[below])])
        out["pool page past byte 2^32"] = int(above[np.argmin(phys_row[above])])
    return out


def forced_places(spec, b, ns, rpb, phys=None):
    """[(name, key, K/V head or None, row block or None, hidden)] of sequence b under `ns` splits and row blocks of `rpb` packed rows.
    A place bound to a row block wants a row of that block."""
    sq, L, a = spec.seqs[b][0], spec.length(b), spec.A
    lo, lim = ranges(L, sq, spec.causal, spec.W)
    first = spec.first(b)
    out = [("first key of the length", _free_of_anchor(max(first, 1), a), None, None, False),
           ("last key of the length", _free_of_anchor(L - 1, a, -1), None, None, False)]
    if spec.page:
        mid = (first // spec.page + (L - 1) // spec.page + 1) // 2
        out += [("last key below a page seam", mid * spec.page - 1, None, None, False), ("first key past a page seam", mid * spec.page, None, None, False),
                ("first page of the table", _free_of_anchor(max(first, 1), a) + 1, None, None, False),
                ("last page of the table", max((L - 1) // spec.page * spec.page, first), None, None, False)]
        if phys is not None:
            out += [(name, p * spec.page + 3, None, None, False) for name, p in pool_line_pages(spec, phys[b]).items()]
    else:
        for line in BYTE_LINES:
            k = line // (spec.d * spec.esz)
            out += [(f"last key below byte {line}", k - 1, None, None, False), (f"first key past byte {line}", k, None, None, False)]
    nrows = spec.G * sq
    for rb in range(-(-nrows // rpb)):
        pr0, prl = rb * rpb, min((rb + 1) * rpb, nrows) - 1
        for which, i in (("first", pr0 % sq), ("last", prl % sq)):
            out += [(f"lo of the {which} row", int(lo[i]), None, rb, False), (f"lim - 1 of the {which} row", int(lim[i]) - 1, None, rb, False),
                    (f"lo - 1 of the {which} row (hidden)", int(lo[i]) - 1, None, rb, True), (f"lim of the {which} row (hidden)", int(lim[i]), None, rb, True)]
        tlo, ntb = ewc.block_range(rpb, spec.G, sq, L, spec.W, spec.causal, rb)
        for s in range(1, ns):
            t0 = tlo + (ntb - tlo) * s // ns
            out += [(f"last key below split {s}", t0 * TILE - 1, None, rb, False), (f"first key of split {s}", t0 * TILE, None, rb, False)]
    ok = [p for p in out if 1 <= p[1] < spec.cap and not is_anchor(p[1], a) and (p[4] or first <= p[1] < L)]
    return [(n, k, kvh, rb, h) for n, k, kv, rb, h in ok for kvh in ([None] if rb is None else range(spec.Hkv))]


def plan_targets(spec, ns, rpb, phys=None):
    """-> list over ROUNDS of dict(target: per sequence int64 numpy [H, sq] (None: no rows), named: {(b, h, i): name}); plus the places
    no row can see ({(b, name, kvh, rb)}: a gap between two heads' windows in a straddling block).  Round 0 carries the seeded targets,
    every round its share of the forced places."""
    H, G, a, cap = spec.H, spec.G, spec.A, spec.cap
    base_t, info = [], []
    for b, (sq, _) in enumerate(spec.seqs):
        if sq == 0:
            base_t.append(None)
            info.append(None)
            continue
        L = spec.length(b)
        lo, lim = ranges(L, sq, spec.causal, spec.W)
        i = np.arange(sq, dtype=np.int64)
        t = np.empty((H, sq), dtype=np.int64)
        for h in range(H):
            r = np.random.RandomState((1000003 * spec.seed + 7919 * b + h) % 2 ** 31).randint(0, 2 ** 31 - 1, (3, sq)).astype(np.int64)
            th = np.where(r[2] % 2 == 0, np.maximum(lim - 1 - r[0] % NEAR, lo), lo + r[1] % (lim - lo))
            n = i * H + h
            hid, kind = n % 7 == 3, (n // 7) % 3
            th = np.where(hid & (kind == 0), lim + r[0] % NEAR, th)
            th = np.where(hid & (kind == 1) & (lo > 0), lo - 1 - r[0] % NEAR, th)
            th = np.where(hid & (kind == 2) & (L < cap), L + r[0] % max(cap - L, 1), th)
            t[h] = th
        t = np.clip(t, 1, cap - 1)
        t = np.where(is_anchor(t, a), t + 1, t)
        t = np.where(t > cap - 1, cap - 2, t)
        assert not is_anchor(t, a).any()
        base_t.append(t)
        info.append((lo, lim, L))
    rounds, missing = [dict(target=[None if t is None else t.copy() for t in base_t], named={})], set()
    for b, (sq, _) in enumerate(spec.seqs):
        if sq == 0:
            continue
        lo, lim, L = info[b]
        nrows = G * sq
        for name, k, kvh, rb, hidden in forced_places(spec, b, ns, rpb, phys):
            if rb is None:                                  # any row that sees it: from the diagonal row on, over the heads
                i0 = int(np.clip(k - (L - sq), 0, sq - 1))
                cand = ((h, i) for i in list(range(i0, min(i0 + 4, sq))) + list(range(max(i0 - 4, 0), i0)) for h in range(H))
            else:
                cand = ((kvh * G + pr // sq, pr % sq) for pr in range(rb * rpb, min((rb + 1) * rpb, nrows)))
            cand = [(h, i) for h, i in cand if hidden or lo[i] <= k < lim[i]]
            if hidden:
                i_own = (rb * rpb if "first" in name else min((rb + 1) * rpb, nrows) - 1) % sq
                cand = [(h, i) for h, i in cand if i == i_own]
            if not cand:
                missing.add((b, name, kvh, rb))
                continue
            for n in range(10 ** 6):
                if n == len(rounds):
                    rounds.append(dict(target=[None if t is None else t.copy() for t in base_t], named={}))
                free = [c for c in cand if (b, *c) not in rounds[n]["named"]]
                if free:
                    h, i = free[(7 * len(rounds[n]["named"])) % len(free)] if rb is None else free[0]
                    rounds[n]["target"][b][h, i] = k
                    rounds[n]["named"][(b, h, i)] = f"{name}{'' if rb is None else f' of row block {rb}'} (key {k})"
                    break
    for rnd in rounds:                                      # every row has a closed form
        for b, t in enumerate(rnd["target"]):
            if t is not None:
                lo, lim, L = info[b]
                vis = (t >= lo[None]) & (t < lim[None])
                assert (vis | (anchors_below(lim, a) - anchors_below(lo, a) >= 1)[None]).all(), (b, "a row with neither target nor anchor")
    return rounds, missing


def build_queries(spec, rnd, device="cpu"):
    """-> dict(Q: [B, H, Sq, d] or (varlen) [total_q, H, d] bf16, cu int32 [B + 1] or None, target, named)"""
    d, nb, H = spec.d, spec.nb, spec.H
    uniform = spec.kind != "varlen"
    sq0 = spec.seqs[0][0]
    assert not uniform or all(s == sq0 for s, _ in spec.seqs)
    Q = torch.zeros((len(spec.seqs), H, sq0, d) if uniform else (spec.total_q, H, d), dtype=bf, device=device)
    cu = np.concatenate([[0], np.cumsum([s for s, _ in spec.seqs])])
    for b, t in enumerate(rnd["target"]):
        if t is None:
            continue
        tt = torch.as_tensor(t, device=device)
        rows = torch.zeros((H, t.shape[1], d), dtype=f32, device=device)
        rows[..., :nb] = UNIT * lp.bits(spec.base + tt, nb).float()
        rows[..., nb] = UNIT * nb - E
        if uniform:
            Q[b] = rows.to(bf)
        else:
            Q[cu[b]:cu[b + 1]] = rows.to(bf).transpose(0, 1)
    assert UNIT * nb - E == float(torch.tensor(float(UNIT * nb - E)).to(bf))
    return dict(Q=Q, cu=None if uniform else torch.tensor(cu, dtype=torch.int32, device=device), target=rnd["target"], named=rnd["named"])


def expected(spec, q, o_dtype=bf, device="cpu"):
    """per sequence (None: no rows) dict(O [H, sq, d] in o_dtype, lse float64 [H, sq], log2k [H, sq], vis bool [H, sq])"""
    out = []
    for b, t in enumerate(q["target"]):
        if t is None:
            out.append(None)
            continue
        sq, L = t.shape[1], spec.length(b)
        lo, lim = ranges(L, sq, spec.causal, spec.W)
        vis = (t >= lo[None]) & (t < lim[None])
        k = (anchors_below(lim, spec.A) - anchors_below(lo, spec.A))[None].repeat(spec.H, 0)
        tt, own = torch.as_tensor(t, device=device), torch.as_tensor(owner(spec, b, t) * np.ones_like(t), device=device)
        O = torch.empty((spec.H, sq, spec.d), dtype=f32, device=device)
        for h in range(spec.H):
            kvh = h // spec.G
            O[h] = lp.v_rows(spec.base + tt[h], kvh + spec.Hkv * own[h][:, None], spec.d).float() * (VD[kvh % 4] if spec.fp8 else 1.0)
        O = torch.where(torch.as_tensor(vis, device=device)[..., None], O, torch.zeros((), device=device)).to(o_dtype)
        O = torch.where(O == 0, torch.full_like(O, fp.ZERO_OUT), O)
        with np.errstate(divide="ignore"):
            lse = np.where(vis, LN2 * UNIT * spec.nb, LN2 * (UNIT * spec.nb - E) + np.log(np.maximum(k, 1).astype(np.float64)))
            log2k = np.where(vis, 0.0, np.log2(np.maximum(k, 1)))
        out.append(dict(O=O, lse=torch.as_tensor(lse, device=device), log2k=torch.as_tensor(log2k, device=device), vis=vis))
    return out


def lse_bound(ref, log2k):
    """fp.LSE_REL |ref| plus one ulp of the hardware log at log2 k (hidden rows: the row sum is k, not 1): long_probe.lse_bound's e"""
    return fp.LSE_REL * ref.abs() + log2k * 2.0 ** -23 * LN2


# ---- the call and the check -------------------------------------------------------------------------------------------------------------
def plan_of(spec, ns=0, o_dtype=bf, W=None):
    """the library's plan of the call (num_splits, rows_per_block, ...): a host function, no GPU"""
    W = spec.W if W is None else W
    code = {bf: fa.FA_DTYPE_BF16, f32: fa.FA_DTYPE_F32}[o_dtype]
    B, sq = len(spec.seqs), spec.seqs[0][0]
    if spec.kind == "decode":
        return fa.decode_plan(B, spec.H, spec.Hkv, sq, spec.cap, spec.d, code, ns, W)
    if spec.kind == "extend":
        return fa.extend_plan(B, spec.H, spec.Hkv, sq, spec.cap, spec.d, code, ns, W or None)
    return fa.extend_varlen_plan(B, spec.H, spec.Hkv, spec.total_q, spec.cap, spec.d, code, ns, W or None)


def kernel_name(spec, W=None):
    """the split-KV form a call of this spec runs: the flags of its row in csrc/split_forms.hip.h, under the label profiles/long_cache_gpu.log uses"""
    W = spec.W if W is None else W
    ext = spec.kind != "decode"
    return (f"split_kernel_of<EXTEND={int(ext)}, VARLEN={int(spec.kind == 'varlen')}, WINDOW={int(bool(W) or not ext)}, PAGED={int(bool(spec.page))}, "
            f"KV8={int(spec.fp8)}>(d={spec.d})")


def call(spec, cache, q, ns, o_dtype=bf, W=None, O=None):
    """the front of spec.kind with return_lse -> (O, LSE)"""
    W = spec.W if W is None else W
    K, V = (cache["K"], cache["V"])
    kw = dict(kv_lens=cache["kv_lens"], scale=fp.PREFILL_SCALE(0), is_causal=spec.causal, num_splits=ns, return_lse=True, O=O,
              k_descale=cache["kd"], v_descale=cache["vd"])
    if O is None:
        kw["out_dtype"] = o_dtype
    if spec.kind == "decode":
        kw["window"] = W or None
        return fa.flash_attention_decode_paged(q["Q"], K, V, cache["table"], **kw) if spec.page else fa.flash_attention_decode(q["Q"], K, V, **kw)
    name = "flash_attention_extend" + ("_paged" if spec.page else "") + ("_varlen" if spec.kind == "varlen" else "") + ("_window" if W else "")
    args = (q["Q"], K, V) + ((cache["table"],) if spec.page else ()) + ((q["cu"],) if spec.kind == "varlen" else ())
    if W:
        kw["window"] = W
    return getattr(fa, name)(*args, **kw)


def canary_output(spec, o_dtype, device):
    """a ragged call's O, prefilled: the rows no sequence owns must keep the pattern"""
    return torch.full((spec.total_q, spec.H, spec.d), CANARY, dtype=o_dtype, device=device)


def describe(spec, q, b, h, i, ns, rpb, cache=None):
    t = int(q["target"][b][h, i])
    sq, L = spec.seqs[b][0], spec.length(b)
    rb = ((h % spec.G) * sq + i) // rpb
    tlo, ntb = ewc.block_range(rpb, spec.G, sq, L, spec.W, spec.causal, rb)
    split = next((s for s in range(ns) if tlo + (ntb - tlo) * s // ns <= t // TILE < tlo + (ntb - tlo) * (s + 1) // ns), None)
    page = ""
    if spec.page:
        lp_ = t // spec.page
        page = f", page {lp_}" + (f" = pool page {int(cache['phys'][b, lp_])}" if cache is not None and cache.get("phys") is not None and lp_ < cache["phys"].shape[1] else "")
    lo, lim = ranges(L, sq, spec.causal, spec.W)
    seen = lo[i] <= t < lim[i]
    forced = q["named"].get((b, h, i))
    return (f"sequence {b} (length {L}, {sq} rows) head {h} row {i} (row block {rb} of K/V head {h // spec.G}, tiles [{tlo}, {ntb})) targets key {t} "
            f"(tile {t // TILE}{page}, split {split} of {ns}){'' if seen else f', hidden: the row sees [{int(lo[i])}, {int(lim[i])})'}"
            f"{f'; forced: {forced}' if forced else ''}")


def check(what, spec, q, exp, O, lse, ns, rpb, cache=None):
    """asserts O bit for bit on every row of every sequence, the canary on the rows no sequence owns, the LSE within lse_bound; returns
    dict(rows, hidden, worst): rows compared, rows with a hidden target, worst LSE error / bound"""
    cu = np.concatenate([[0], np.cumsum([s for s, _ in spec.seqs])])
    rows = hidden = 0
    worst = 0.0
    for b, e in enumerate(exp):
        if e is None:
            continue
        if spec.kind == "varlen":
            Ob, Lb = O[cu[b]:cu[b + 1]].transpose(0, 1), lse[:, cu[b]:cu[b + 1]]
        else:
            Ob, Lb = O[b], lse[b]
        wrong = (lp._bits_of(Ob) != lp._bits_of(e["O"])).any(-1)
        if bool(wrong.any()):
            h, i = torch.nonzero(wrong)[0].tolist()
            raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.numel()} rows of sequence {b} differ from the closed form; first: "
                                 f"{describe(spec, q, b, h, i, ns, rpb, cache)}: {Ob[h, i, :6].float().tolist()} for {e['O'][h, i, :6].float().tolist()}")
        ratio = (Lb.double() - e["lse"]).abs() / lse_bound(e["lse"], e["log2k"])
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
        if float(ratio.max()) > 1.0:
            h, i = torch.nonzero(ratio == ratio.max())[0].tolist()
            raise AssertionError(f"{what}: {int((ratio > 1).sum())} LSE entries of sequence {b} outside the bound, worst error / bound "
                                 f"{float(ratio.max()):.3f}: {describe(spec, q, b, h, i, ns, rpb, cache)}: {float(Lb[h, i])!r} for {float(e['lse'][h, i])!r}")
        worst = max(worst, float(ratio.max()))
        rows += wrong.numel()
        hidden += int((~e["vis"]).sum())
    if spec.kind == "varlen" and spec.pad:
        tail = O[cu[-1]:]
        assert bool((tail.float() == CANARY).all()), f"{what}: rows of O that no sequence owns were written"
    return dict(rows=rows, hidden=hidden, worst=worst)


# ---- the documented arithmetic of csrc/decode_bf16.hip.h in fp32, and what a wrong kernel would return ----------------------------------
MUTANTS = ("split_one_tile_short", "split_one_tile_long", "limb_of_the_last_row", "firstb_one_tile_high", "lo_plus_1", "lo_minus_1",
           "records_of_the_capacity", "page_plus_1", "table_row_0", "page_shift_minus_1", "key_minus_2^16", "key_minus_2^(31-log2 row bytes)",
           "slab_row_of_the_next_token", "q0_of_the_next_sequence", "descale_of_the_next_head")


def logical_cache(spec, cache, b, kvh, mutant=None):
    """(K, V) fp32 [cap, d] of sequence b's K/V head as the kernel's loads return them: rows at and beyond the length 0 (the record
    count), V below row 0's left edge 0 (the prologue's cut), unowned pages as the memory holds them (clamped entries)"""
    L, cap, d = spec.length(b), spec.cap, spec.d
    j = torch.arange(cap)
    if spec.page:
        shift = int(math.log2(spec.page)) - (mutant == "page_shift_minus_1")
        P = cache["K"].shape[0]
        lpage = (j >> shift).clamp(max=(L - 1) >> shift).clamp(min=spec.first(b) >> shift) + (mutant == "page_plus_1")
        tb = cache["table"][0 if mutant == "table_row_0" else b].long()
        entry = tb[lpage.clamp(max=len(tb) - 1)].clamp(0, P - 1)
        row = j & ((1 << shift) - 1)
        K, V = cache["K"][entry, kvh, row].float(), cache["V"][entry, kvh, row].float()
    elif mutant and mutant.startswith("key_minus"):
        shift = 16 if mutant.endswith("16") else 31 - int(math.log2(d * spec.esz))
        K, V = key_rows(dataclasses.replace(spec, base=spec.base - 2 ** shift), j, kvh, b, L, "cpu")   # (an anchor's row 2^k below is an anchor)
        K[:spec.first(b)] = float("nan")
    else:
        K, V = cache["K"][b, kvh].float(), cache["V"][b, kvh].float()
    if mutant != "records_of_the_capacity":
        K, V = K.clone(), V.clone()
        K[L:], V[L:] = 0, 0
    V[:spec.first(b)] = 0
    return K, V


def emulate(spec, cache, q, b, ns, rpb, mutant=None):
    """(O fp32 [H, sq, d] before the rounding to the output type, LSE fp32 [H, sq]) of sequence b as split_kv_kernel and
    decode_combine_kernel compute them: per (K/V head, row block, split) the tiles [t0, t1); per tile four waves of 32 keys with a running
    maximum each, weights as a bf16 hi + lo pair; the four-wave merge; normalised slabs; the combine's weights exp(lse_s - m)."""
    sq, L, G, d, W = spec.seqs[b][0], spec.length(b), spec.G, spec.d, spec.W
    NEG = float("-inf")
    cu = np.concatenate([[0], np.cumsum([s for s, _ in spec.seqs])])
    bq = b + 1 if mutant == "q0_of_the_next_sequence" else b
    Qb = (q["Q"][b] if spec.kind != "varlen" else q["Q"][cu[bq]:cu[bq] + sq].transpose(0, 1)).float()
    lo_all, lim_all = ranges(L, sq, spec.causal, W)
    lo_all = lo_all + {"lo_plus_1": 1, "lo_minus_1": -1}.get(mutant, 0) * (lo_all > 0)
    O, LSE = torch.zeros((spec.H, sq, d), dtype=f32), torch.zeros((spec.H, sq), dtype=f32)
    nrows = G * sq
    for kvh in range(spec.Hkv):
        K, V = logical_cache(spec, cache, b, kvh, mutant)
        dh = (kvh + 1) % spec.Hkv if mutant == "descale_of_the_next_head" else kvh
        c = f32_(1.0) * (KD[dh % 4] if spec.fp8 else 1.0)                       # fp32(scale log2 e) = 1, times k_descale
        vd = VD[dh % 4] if spec.fp8 else 1.0
        part_o, part_l = torch.zeros((ns, nrows, d), dtype=f32), torch.full((ns, nrows), NEG, dtype=f32)
        for rb in range(-(-nrows // rpb)):
            pr = torch.arange(rb * rpb, min((rb + 1) * rpb, nrows))
            g, i = pr // sq, pr % sq
            tlo, ntb = ewc.block_range(rpb, G, sq, L, W, spec.causal, rb)
            if mutant == "limb_of_the_last_row" and spec.causal:
                ntb = -(-max(L - sq + int(i[-1]) + 1, 1) // TILE)
            if mutant == "firstb_one_tile_high" and W > 0:
                tlo = min(tlo + 1, ntb)
            Qr = Qb[kvh * G + g, i]
            lo, lim = torch.as_tensor(lo_all)[i][:, None], torch.as_tensor(lim_all)[i][:, None]
            for s in range(ns):
                t0, t1 = tlo + (ntb - tlo) * s // ns, tlo + (ntb - tlo) * (s + 1) // ns
                if s == 0 and ns > 1:
                    t1 += {"split_one_tile_short": -1, "split_one_tile_long": 1}.get(mutant, 0)
                R = len(pr)
                m, l, o = torch.full((R, 4), NEG), torch.zeros((R, 4)), torch.zeros((R, 4, d))
                for t in range(t0, t1):
                    key = torch.arange(t * TILE, (t + 1) * TILE)
                    Kt, Vt = torch.zeros((TILE, d)), torch.zeros((TILE, d))
                    n = max(min(spec.cap - t * TILE, TILE), 0)
                    Kt[:n], Vt[:n] = K[t * TILE:t * TILE + n], V[t * TILE:t * TILE + n]
                    x = (Qr @ Kt.T) * c
                    x = torch.where((key[None] >= lo) & (key[None] < lim), x, torch.full_like(x, NEG)).view(R, 4, 32)
                    m_new = torch.maximum(m, x.max(-1).values)
                    m_use = torch.where(m_new == NEG, torch.zeros_like(m_new), m_new)
                    alpha = torch.exp2(m - m_use)
                    p = torch.exp2(x - m_use[..., None])
                    hi = p.to(bf).float()
                    low = (p - hi).to(bf).float()
                    l = l * alpha + p.sum(-1)
                    o = o * alpha[..., None] + torch.einsum("rwk,wkd->rwd", hi, Vt.view(4, 32, d)) + torch.einsum("rwk,wkd->rwd", low, Vt.view(4, 32, d))
                    m = m_new
                M = m.max(-1).values
                ok = M != NEG
                wgt = torch.where(ok[:, None], torch.exp2(m - torch.where(ok, M, torch.zeros_like(M))[:, None]), torch.zeros_like(m))
                Ls = (wgt * l).sum(-1)
                acc = (wgt[..., None] * o).sum(1)
                inv = torch.where(ok, 1.0 / Ls, torch.zeros_like(Ls)) * vd
                part_o[s, pr] = acc * inv[:, None]
                part_l[s, pr] = torch.where(ok, (M + torch.log2(Ls)) * f32_(LN2), torch.full_like(M, NEG))
        if ns == 1:
            Oh, Lh = part_o[0], part_l[0]
        else:
            if mutant == "slab_row_of_the_next_token":
                part_o[1:] = part_o[1:].roll(-1, 1)
            M = part_l.max(0).values
            w = torch.exp(part_l - M[None])
            Wsum = w.sum(0)
            Oh, Lh = (w[..., None] * part_o).sum(0) * (1.0 / Wsum)[:, None], M + torch.log(Wsum)
        O[kvh * G:(kvh + 1) * G], LSE[kvh * G:(kvh + 1) * G] = Oh.view(G, sq, d), Lh.view(G, sq)
    return O, LSE


def f32_(x):
    return float(np.float32(x))


# ---- the cases tests/test_long_cache.py runs on the GPU (tests/test_long_cache_probe.py asserts their coverage on the CPU) ---------------
def _ragged_batch(seed, n=70, cap=2 ** 20):
    """70 sequences (two steps of the kernel's 64-sequence scan): row counts from {0, 1, 3, 16, 17, 64, 1000, 4099}, lengths 1 .. 2^20 --
    a few long ones, the rest spread, some shorter than their row count"""
    g = np.random.RandomState(seed)
    rows = g.choice([0, 1, 3, 16, 17, 64], n)
    lens = (2.0 ** g.uniform(0, 13, n)).astype(np.int64) + 1
    for at, (r, L) in {0: (4099, cap), 3: (1000, 2 ** 19 + 5), 7: (17, cap - 129), 20: (1000, 700), 41: (64, 2 ** 17 + 77), 63: (1, 1), 64: (4099, 2 ** 18 + 1),
                       65: (0, 5), 66: (16, cap), 69: (3, 70001)}.items():
        rows[at], lens[at] = r, L
    return tuple((int(r), int(L)) for r, L in zip(rows, lens))


def gpu_cases():
    """{id: (Spec, split counts)} from cheap to large"""
    M = 2 ** 20
    L17 = 2 ** 17 + 77
    c = {}
    for sq in (1, 16):
        for causal in (True, False):
            c[f"decode_bf16_sq{sq}_{'causal' if causal else 'full'}"] = (
                Spec("decode", ((sq, M), (sq, M - 129), (sq, 70001)), M, causal=causal, seed=1), (0, 1, 3, 64))
    for d in (128, 64):
        for causal in (True, False):
            tag = f"d{d}_{'causal' if causal else 'full'}"
            if d == 128:
                c[f"extend_sq4096_{tag}"] = (Spec("extend", ((4096, L17),), 2 ** 17 + 128, d, causal=causal, seed=2), (0, 1, 3))
            c[f"extend_sq1000_{tag}"] = (Spec("extend", ((1000, L17),), 2 ** 17 + 128, d, causal=causal, seed=3), (0, 1, 3))
            if (d == 128) == causal:
                c[f"extend_sq5000_short_{tag}"] = (Spec("extend", ((5000, L17), (5000, 3000)), 2 ** 17 + 128, d, causal=causal, seed=4), (0, 1, 3))
    for fp8, page, d in ((True, 0, 64), (False, 64, 64), (True, 128, 128)):      # the other three cache forms of the un-windowed call
        c[f"extend_sq1000_{'fp8' if fp8 else 'bf16'}_{'paged' if page else 'contiguous'}_d{d}"] = (
            Spec("extend", ((1000, L17),), 2 ** 17 + 128, d, fp8=fp8, page=page, seed=3), (0, 3))
    for W in (4096, 100):
        for fp8, page, d, causal in ((False, 0, 128, True), (True, 0, 64, True), (False, 64, 64, False), (True, 128, 128, True)):
            c[f"extend_window{W}_{'fp8' if fp8 else 'bf16'}_{'paged' if page else 'contiguous'}_d{d}"] = (
                Spec("extend", ((5000, M - 3),), M, d, causal=causal, W=W, fp8=fp8, page=page, seed=5), (0, 3))
    for fp8 in (False, True):
        for W in (0, 4096):
            c[f"ragged_paged_{'fp8' if fp8 else 'bf16'}_W{W}"] = (
                Spec("varlen", _ragged_batch(11), M, 128, W=W, fp8=fp8, page=128, pad=50, seed=6), (0, 1, 3))
    for W in (0, 100):
        for fp8, d in ((False, 64), (True, 128)):
            c[f"ragged_contiguous_{'fp8' if fp8 else 'bf16'}_W{W}"] = (
                Spec("varlen", ((1000, 2 ** 18), (17, 2 ** 18 - 129), (0, 9), (4099, 70001)), 2 ** 18, d, W=W, fp8=fp8, pad=50, seed=7), (0, 3))
    for fp8 in (False, True):
        line = 2 ** 32 // (2 * 128 * 128 * (1 if fp8 else 2))
        c[f"decode_pool_past_4GiB_{'fp8' if fp8 else 'bf16'}"] = (
            Spec("decode", ((16, M), (16, 300000)), M, 128, fp8=fp8, page=128, pool_pages=line * 5 // 4, share=100, seed=8), (0, 3, 64))
    for W in (0, 4096):
        c[f"decode_fp8_at_the_capacity_limit_W{W}"] = (Spec("decode", ((4, 2 ** 24),), 2 ** 24, 64, 4, 1, W=W, fp8=True, seed=9), (0, 64))
        c[f"decode_paged_at_the_capacity_limit_W{W}"] = (Spec("decode", ((4, 2 ** 24),), 2 ** 24, 64, 4, 1, W=W, page=16, seed=10), (0, 64))
    return c
