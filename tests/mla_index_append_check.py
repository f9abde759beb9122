"""Reference of the MLA index-cache append (mla_index_append / _paged; no tests in here): the eight pinned steps of
include/flash_attention.h in plain elementwise numpy fp32 -- rope_check's rotation, the seven butterfly stages, the two roundings to
bf16, the scale in both forms, torch's CPU cast to e4m3fn -- and the cache such an append leaves, on test_mla_append's pattern."""
import numpy as np
import torch

import mla_check as mc
import rope_check as rc
from kv_cache_check import F8

B, CAP, PAGES, table_for = mc.B, mc.CAPACITY, mc.PAGES, mc.table_for
H, D = 64, 128
C0, C1 = np.float32(2.0 ** -3.5), np.float32(1.0 / 448.0)
SENTINEL, SCALE_SENTINEL = 0xA5, -7.0


def hadamard(x):
    """the in-place fast Walsh-Hadamard transform of fp32 [..., 128]: strides 1, 2, ..., 64, (a, b) -> (a + b, a - b)"""
    t = np.ascontiguousarray(x, dtype=np.float32).copy()
    st = 1
    while st < D:
        v = t.reshape(t.shape[:-1] + (D // (2 * st), 2, st))
        a, b = v[..., 0, :].copy(), v[..., 1, :].copy()
        v[..., 0, :], v[..., 1, :] = a + b, a - b
        st *= 2
    return t


def scale_of(amax, pow2):
    """fp32 amax (floored at 1e-4) -> the row's scale"""
    s = (np.maximum(amax, np.float32(1e-4)) * C1).astype(np.float32)
    if pow2:
        u = s.view(np.uint32)
        s = (((u >> 23) + ((u & 0x7FFFFF) != 0)) << 23).astype(np.uint32).view(np.float32)
    return s


def transform(x, pow2, table=None, pos=None, interleaved=False):
    """x bf16 [B, heads, R, 128], rotated at pos int64 [B, R] under `table` (None: not rotated) -> (codes uint8, scales fp32 [B, heads, R])"""
    if table is not None:
        x = rc.rotate(x, table, pos, interleaved)
    r = torch.from_numpy(hadamard(x.float().numpy()) * C0).to(torch.bfloat16).float().numpy()
    s = scale_of(np.abs(r).max(-1), pow2)
    q = np.clip(r / s[..., None], np.float32(-448), np.float32(448))
    return torch.from_numpy(q).to(F8).view(torch.uint8), torch.from_numpy(s)


def positions(lens, Sq):
    """int64 [B, Sq]: where row i of sequence b is rotated -- its cache position where it is written, the Q rule's everywhere"""
    return torch.tensor([rc.q_positions(L, Sq, CAP) for L in lens], dtype=torch.int64)


def expected(cache, scales, codes, s, lens, table=None, page=0, skip=()):
    """(cache, scales) -- uint8 [B, CAP, 128] / fp32 [B, CAP] or the pools -- after the append of codes [B, Sq, 128], s [B, Sq];
    skip: (b, table column) pairs whose rows are dropped"""
    out, so, Sq = cache.clone(), scales.clone(), codes.shape[1]
    for b, L in enumerate(lens):
        L = min(L, CAP)
        for i in range(max(Sq - L, 0), Sq if L > 0 else 0):
            p = L - Sq + i
            if table is None:
                out[b, p], so[b, p] = codes[b, i], s[b, i]
            elif (b, p // page) not in skip:
                out[table[b, p // page], p % page], so[table[b, p // page], p % page] = codes[b, i], s[b, i]
    return out, so


def blank(page, spare=5):
    """a sentinel-filled (cache, scales), contiguous (page 0) or pools of B CAP / page + spare pages"""
    shape = (B * (CAP // page) + spare, page) if page else (B, CAP)
    return torch.full(shape + (D,), SENTINEL, dtype=torch.uint8), torch.full(shape, SCALE_SENTINEL)


def same(got, want):
    """bytes for bytes, fp32 bit for bit"""
    return all(torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)) and g.shape == w.shape for g, w in zip(got, want))
