"""Checker of the MLA decode tests (flash_attention_mla_decode, _mla_decode_paged): the float64 ground truth, the
data in both cache forms, an fp32 emulation of the kernel's arithmetic, and a by-name caller of the C entry points.

Rule.  One latent cache row per token, DL = 512 latent columns then DR = 64 rotary columns, shared by every head.  Row i of head h sees
the keys `kv_cache_check.visible(len_b, Sq, causal)` shows it (len_b clamped into [1, capacity] as the library clamps it); its score
against key k is scale * <Q[b, h, i, :576], KV[b, k, :576]> and its value is KV[b, k, :512].

Reference.  `reference()`: the explicit softmax in float64 over those keys, O [B, H, Sq, 512], LSE [B, H, Sq].  Criterion:
`kv_cache_check.assert_close`, unchanged (1e-3 + 1e-3 |ref| on O, 2e-4 + 2e-6 |ref| on the LSE).

Emulation.  `emulate()`: what the kernel computes, in torch fp32 on the CPU -- fp32 scores of the bf16 inputs, the online softmax over
tiles of KT keys in the log2 domain, weights as a bf16 hi + lo pair against the bf16 values, fp32 sums, normalised slabs per split and
the LSE-weighted combine in split order.  It differs from the kernel in summation order only; the CPU test holds it to half the tolerance
on every GPU case's inputs, so those inputs are known admissible before the GPU run.
"""
import math

import torch

import kv_cache_check as kc
from abi_decl import declared_parameters
from kv_cache_check import DEV, fa

DL, DR = fa.MLA_D_LATENT, fa.MLA_D_ROPE
D = DL + DR
CAPACITY = 384
PAGES = (16, 128)
KT = 32                      # the kernel's key tile: fa.mla_decode_plan(...)["kv_block_rows"] (asserted in test_mla_abi.py)
ROWS = 64                    # ... and its row block
DEFAULT_SCALE = D ** -0.5
# the packed-row shapes (H, Sq) of the GPU parity tests: one row; 15 rows, a partial tile; 16 rows; 65 rows, head 12 across the block seam;
# two blocks; four blocks
SHAPES = ((1, 1), (5, 3), (16, 1), (13, 5), (128, 1), (16, 16))
B = 3


def clamp(n, cap=CAPACITY):
    return min(max(int(n), 1), cap)


def lengths(Sq, page):
    """three batches of B lengths, mixed: around the 16-key group, the kernel's key tile, the page and the capacity; one below Sq"""
    around = lambda n: [clamp(n - 1), clamp(n), clamp(n + 1)]
    out = [around(16), around(KT), around(page or 128), [CAPACITY - 3, CAPACITY, 2 * KT + 1], [max(Sq - 1, 1), 1, 3 * KT]]
    return out


def data(H, Sq, seed, batch=B):
    """(Q [B, H, Sq, 576], KV [B, CAPACITY, 576]) bf16 N(0, 1) on the CPU"""
    return kc.randn((batch, H, Sq, D), seed, torch.bfloat16), kc.randn((batch, CAPACITY, D), seed + 1, torch.bfloat16)


SPLITS = (1, 2, 3, 64, 0)    # forced counts, and the library's choice


def parity_cases():
    """every input of the GPU parity tests, (H, Sq, Q, KV, lens, causal, page): per packed-row shape one data set, every batch of
    `lengths`, the mask both ways; the cache form cycles through contiguous, page 16 and page 128 (all three at every shape).  The CPU
    test holds the emulation to half the tolerance on exactly these"""
    for (H, Sq) in SHAPES:
        Q, KV = data(H, Sq, 4000 + 10 * H + Sq)
        n = 0
        for causal in (False, True):
            for page in (0,) + PAGES:
                for lens in lengths(Sq, page)[n % 2::2] if H * Sq > 64 else lengths(Sq, page):
                    yield H, Sq, Q, KV, lens, causal, page
                n += 1


def scale_cases():
    """the custom-scale inputs, (name, scale, Q, KV, lens): kv_cache_check.SCALES at d = 576 (Q and the cache times the factor)"""
    for name in ("small", "large", "one", "boost3"):
        scale, f = kc.SCALES[name](D)
        Q, KV = data(8, 2, 4700 + len(name))
        yield name, scale, (Q.float() * f).to(torch.bfloat16), (KV.float() * f).to(torch.bfloat16), [CAPACITY, 100, 33]


def reference(Q, KV, lens, causal, scale=None, score_cols=D, v_lo=0, vis=None):
    """float64 (O [B, H, Sq, 512], LSE [B, H, Sq]); score_cols / v_lo / vis(b, L) -> bool [Sq, L]: the columns and the visibility a
    WRONG implementation would use, or those of a part of the keys (test_mla_abi.py); a row that sees no key: O = NaN, LSE = -inf"""
    Bq, H, Sq, _ = Q.shape
    scale = DEFAULT_SCALE if scale is None else scale
    O = torch.zeros(Bq, H, Sq, DL, dtype=torch.float64)
    lse = torch.zeros(Bq, H, Sq, dtype=torch.float64)
    for b in range(Bq):
        L = clamp(KV.shape[1] if lens is None else lens[b], KV.shape[1])
        kv = KV[b, :L].double()
        S = (Q[b, :, :, :score_cols].double() @ kv[:, :score_cols].T) * scale
        S = S.masked_fill(~(kc.visible(L, Sq, causal) if vis is None else vis(b, L))[None], float("-inf"))
        lse[b] = torch.logsumexp(S, -1)
        O[b] = torch.softmax(S, -1) @ kv[:, v_lo:v_lo + DL]
    return O, lse


def as_kv_cache(Q, KV):
    """(K, V) [B, 1, capacity, 576] with V's rope columns zeroed: the tensors kv_cache_check's own functions take"""
    V = KV.clone()
    V[..., DL:] = 0
    return KV[:, None], V[:, None]


def assert_close_with_score_noise(O, lse, Q, KV, lens, causal, scale, what):
    """kv_cache_check's wider bound of the custom-scale cases, on the 576-wide problem (its O has 64 zero columns more)"""
    K, V = as_kv_cache(Q, KV)
    pad = torch.zeros(*O.shape[:-1], DR, dtype=O.dtype, device=O.device)
    kc.assert_close_with_score_noise(torch.cat([O, pad], -1), lse, Q, K, V, [clamp(L) for L in lens], causal, scale, what)


# ---- the two cache forms ----
def table_for(batch, page, seed):
    return kc.random_table(batch, CAPACITY // page, seed)


def pool_of(KV, table, page, spare=5):
    """[P, page, 576] with P = B n + spare pages, which `table` gathers back into KV"""
    return kc.scatter(KV[:, None], table, page, spare)[:, 0].contiguous()


def gathered(pool, table):
    return kc.gather(pool[:, None], table)[:, 0].contiguous()


def attend(Q, KV, lens, page=0, table=None, pool=None, **kw):
    """(O, LSE) -- or O alone under return_lse=False -- through the Python fronts; page > 0: the paged front on a pool built here (or
    `pool` / `table` as given)"""
    kw.setdefault("return_lse", True)
    lens = kc.i32(lens)
    if not page:
        return fa.flash_attention_mla_decode(Q.to(DEV), KV.to(DEV), lens, **kw)
    table = table_for(Q.shape[0], page, 77) if table is None else table
    pool = pool_of(KV, table, page) if pool is None else pool
    return fa.flash_attention_mla_decode_paged(Q.to(DEV), pool.to(DEV), table.to(DEV), lens, **kw)


# ---- the kernel's arithmetic in fp32 ----
def _bf16(x):
    return x.to(torch.bfloat16).float()


def emulate(Q, KV, lens, causal, scale=None, ns=1, single_weights=False):
    """fp32 (O [B, H, Sq, 512], LSE [B, H, Sq]) as the kernel and the combine compute them under `ns` splits"""
    Bq, H, Sq, _ = Q.shape
    scale = DEFAULT_SCALE if scale is None else scale
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    ln2 = torch.tensor(0.6931471805599453, dtype=torch.float32)
    O = torch.zeros(Bq, H, Sq, DL)
    lse = torch.zeros(Bq, H, Sq)
    ninf = float("-inf")
    for b in range(Bq):
        L = clamp(KV.shape[1] if lens is None else lens[b], KV.shape[1])
        vis = kc.visible(L, Sq, causal)[None]                                         # [1, Sq, L]
        q, kv = Q[b].float(), KV[b, :L].float()
        nt = -(-L // KT)
        po, pl = [], []
        for s in range(ns):
            t0, t1 = nt * s // ns, nt * (s + 1) // ns
            m = torch.full((H, Sq), ninf)
            l = torch.zeros(H, Sq)
            acc = torch.zeros(H, Sq, DL)
            for t in range(t0, t1):
                k0, k1 = t * KT, min(t * KT + KT, L)
                x = ((q @ kv[k0:k1].T) * sl2).masked_fill(~vis[:, :, k0:k1], ninf)
                m_new = torch.maximum(m, x.max(-1).values)
                m_use = torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
                alpha = torch.exp2(m - m_use)
                p = torch.exp2(x - m_use[..., None])
                hi = _bf16(p)
                w = hi if single_weights else hi + _bf16(p - hi)                       # (the two MFMAs' fp32 products, summed in fp32)
                acc = acc * alpha[..., None] + w @ kv[k0:k1, :DL]
                l = l * alpha + p.sum(-1)
                m = m_new
            some = m != ninf
            inv = torch.where(some, 1.0 / l, torch.zeros_like(l))
            po.append(acc * inv[..., None])
            pl.append(torch.where(some, (m + torch.log2(l)) * ln2, torch.full_like(m, ninf)))
        if ns == 1:
            O[b], lse[b] = po[0], pl[0]
        else:
            ls = torch.stack(pl)
            M = ls.max(0).values
            w = torch.exp(ls - M)
            W = w.sum(0)
            O[b] = sum(w[s][..., None] * po[s] for s in range(ns)) / W[..., None]
            lse[b] = M + torch.log(W)
    return O, lse


# ---- the C entry points by name ----
# short key -> the header's names (the keys of abi_decl.KEYS where the parameter is one of its, the new ones beside them)
KEYS = {"Q": ("Q",), "KV": ("KV", "KVpool"), "O": ("O",), "LSE": ("LSE",), "lens": ("kvLens",), "table": ("blockTable",), "ws": ("workspace",),
        "B": ("batchSize",), "H": ("numHeads",), "Sq": ("seqLenQ",), "Sk": ("seqLenK",), "P": ("numPages",), "page": ("pageSize",),
        "maxp": ("maxPagesPerSeq",), "ts": ("tableStride",), "dl": ("dLatent",), "dr": ("dRope",), "scale": ("scale",), "causal": ("is_causal",),
        "dtype": ("dtype",), "o": ("o_dtype",), "ns": ("numSplits",), "sQ": ("sQ",), "sKV": ("sKV",), "sO": ("sO",), "stream": ("stream",),
        "plan": ("plan",)}
SYMBOLS = {False: "flash_attention_mla_decode", True: "flash_attention_mla_decode_paged"}


def c_call(symbol, values):
    """`symbol` on the arguments `values` names, the positional list built from include/flash_attention.h: a declared parameter without
    exactly one value is an error; keys the symbol does not declare are ignored (one dict serves both cache forms)"""
    unknown = set(values) - set(KEYS)
    assert not unknown, (symbol, sorted(unknown))
    params = declared_parameters(symbol)
    found = {}
    for key, value in values.items():
        for n in KEYS[key]:
            if n in params:
                found.setdefault(n, []).append(value)
    args = []
    for n in params:
        if len(found.get(n, ())) != 1:
            raise KeyError(f"{symbol}: {len(found.get(n, ()))} values for the declared parameter {n}")
        args.append(found[n][0])
    return getattr(fa.lib(), symbol)(*args)


def sqrt_scale():
    """a model's scale: mscale^2 / sqrt(192) with mscale = 1"""
    return 1.0 / math.sqrt(192.0)
