"""Helpers shared by the tests of windowed chunked prefill (tests/test_extend_window_abi.py, test_extend_window.py,
test_extend_varlen_window.py).  The criterion stays decode_check.assert_close against decode_window_check.reference_window (float64);
what is added here is

* `block_range()`: a Python model of the tile range [tlo_b, ntb) a row block of the windowed split-KV kernel walks (the per-row-block
  start documented in include/flash_attention.h), and `block_hull()`: the brute-force hull of the 128-key tiles that hold a key some
  row of the block sees, straight from decode_window_check.visible_window;
* `per_sequence_reference_window()` / `packed()`: the float64 reference of a ragged batch, every sequence as a batch of one;
* `scatter()`: a contiguous cache laid out as a paged pool behind a given table.
"""
import torch

from decode_window_check import reference_window, visible_window

TILE = 128
MAX_Q = 16   # FA_DECODE_MAX_Q


def row_edges(L, Sq, causal, W):
    """(lowest, highest) visible key of each of the Sq rows, from visible_window: two int lists"""
    vis = visible_window(L, Sq, causal, W)
    assert bool(vis.any(1).all()), "every row sees a key"
    lo = vis.int().argmax(1)
    hi = L - 1 - vis.flip(1).int().argmax(1)
    return lo.tolist(), hi.tolist()


def block_rows(RPB, G, Sq, rb):
    """the query rows i of the packed rows g * Sq + i of row block rb (blocks are not head-aligned)"""
    return [pr % Sq for pr in range(rb * RPB, min((rb + 1) * RPB, G * Sq))]


def block_hull(edges, RPB, G, Sq, rb):
    """[first tile, one past the last tile) that hold a key some row of block rb sees; `edges` = row_edges(...)"""
    lo, hi = edges
    rows = block_rows(RPB, G, Sq, rb)
    return min(lo[i] for i in rows) // TILE, max(hi[i] for i in rows) // TILE + 1


def block_range(RPB, G, Sq, L, W, causal, rb):
    """The kernel's rule.  ntb: the tiles below the largest limit of the block's rows.  tlo_b = firstb / 128 with
    firstb = max(max(L - Sq + qmin + 1, 1) - W, 0), qmin = 0 when the block reaches into the next head, else the query row of its first
    packed row; Sq <= 16: qmin = 0 (decode's range)"""
    nrows, pr0 = G * Sq, rb * RPB
    prl = min(pr0 + RPB, nrows) - 1
    g0, gl = pr0 // Sq, prl // Sq
    qmax = Sq - 1 if g0 != gl else prl - gl * Sq
    limb = max(L - Sq + qmax + 1, 1) if causal else L
    qmin = 0 if (g0 != gl or Sq <= MAX_Q) else pr0 - g0 * Sq
    firstb = max(max(L - Sq + qmin + 1, 1) - W, 0) if W > 0 else 0
    return firstb // TILE, -(-limb // TILE)


def decode_range(Sq, L, W):
    """flash_attention_decode_window's range of a sequence: [first / 128, ceil(L / 128))"""
    first = max(max(L - Sq + 1, 1) - W, 0) if W > 0 else 0
    return first // TILE, -(-L // TILE)


def cu_of(sq):
    cu = [0]
    for s in sq:
        cu.append(cu[-1] + s)
    return cu


def per_sequence_reference_window(Q, K, V, sq, lens, causal, W, scale=None):
    """[(refO [H, sq_b, d], refL [H, sq_b]) or None for an idle slot]: reference_window on every sequence as a batch of one; Q [T, H, d]
    packed by token, K / V [B, Hkv, cap, d]"""
    cu, out = cu_of(sq), []
    for b, s in enumerate(sq):
        if s == 0:
            out.append(None)
            continue
        L = min(max(int(lens[b]), 1), K.shape[2])
        O, lse = reference_window(Q[cu[b]:cu[b + 1]].transpose(0, 1)[None], K[b:b + 1], V[b:b + 1], [L], causal, W, scale)
        out.append((O[0], lse[0]))
    return out


def packed(refs, sq, T, H, d):
    """the per-sequence references as packed (O [T, H, d], LSE [H, T], owned bool [T])"""
    O, lse, owned = torch.zeros(T, H, d, dtype=torch.float64), torch.zeros(H, T, dtype=torch.float64), torch.zeros(T, dtype=torch.bool)
    cu = cu_of(sq)
    for b, r in enumerate(refs):
        if r is not None:
            O[cu[b]:cu[b + 1]] = r[0].transpose(0, 1)
            lse[:, cu[b]:cu[b + 1]] = r[1]
            owned[cu[b]:cu[b + 1]] = True
    return O, lse, owned


def scatter(cache, table, page, spare=5):
    """the pool [P, Hkv, page, d] that `table` [B, n] gathers back into `cache` [B, Hkv, n * page, d]; P = B * n + spare"""
    B, Hkv, cap, d = cache.shape
    n = cap // page
    pool = torch.zeros((B * n + spare, Hkv, page, d), dtype=cache.dtype, device=cache.device)
    pool[table.long().reshape(-1)] = cache.reshape(B, Hkv, n, page, d).permute(0, 2, 1, 3, 4).reshape(B * n, Hkv, page, d)
    return pool


def random_table(B, n, seed, spare=5):
    return torch.randperm(B * n + spare, generator=torch.Generator().manual_seed(seed))[:B * n].reshape(B, n).to(torch.int32)
