"""The Python model of the windowed split-KV kernel's tile range (tests/test_extend_window_abi.py, test_extend_window.py,
test_long_cache_probe.py, test_memory_contract.py).  Rule, reference and criterion are tests/kv_cache_check.py's; what is here is

* `block_range()`: the tile range [tlo_b, ntb) a row block of the windowed split-KV kernel walks (the per-row-block start documented
  in include/flash_attention.h), and `decode_range()`: flash_attention_decode_window's range of a sequence;
* `block_hull()`: the brute-force hull of the 128-key tiles that hold a key some row of the block sees, straight from
  kv_cache_check.visible.
"""
from kv_cache_check import TILE, visible

MAX_Q = 16   # FA_DECODE_MAX_Q


def row_edges(L, Sq, causal, W):
    """(lowest, highest) visible key of each of the Sq rows, from kv_cache_check.visible: two int lists"""
    vis = visible(L, Sq, causal, W)
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
