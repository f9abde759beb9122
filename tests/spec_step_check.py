"""Reference shared by the tests of the speculative step's write side -- flash_attention_rope_append_pos* (the fused rotary append with
per-row position offsets) and flash_attention_kv_accept* (in-cache acceptance); tests/test_spec_step_abi.py on the CPU,
tests/test_rope_append_pos.py, test_kv_accept.py, test_spec_step_rotary.py and test_spec_memory_contract.py on the GPU; no tests in
here.  Plain torch on the CPU, BIT EXACT: the contract of include/flash_attention.h spelled out.

* `pos_positions()`: the table row of every new row -- max(first + clamp(off, 0, Sq - 1), 0), first = clamp(L, 1, cap) - Sq.
* `rope_append_pos()`: `rope_check.rotate` at those rows for Q and K, then `kv_append_check.append` for the slots, which do not move.
* `accept()`: the sequential rule on a contiguous cache or a pool, clamps and skips as the header states them.
* `tree_path()`: the ancestor walk, on the host.  `binary()`, `star()`, `random_tree()`: parent arrays.
Each takes `wrong=`: a named wrong kernel, emulated, for tests/test_spec_step_abi.py to refuse.
"""
import torch

import kv_append_check as kc
import rope_check as rc

WRONG_ROPE = ("offsets by cache position", "offsets of batch 0", "offset moves the slot", "Q at base + i")
WRONG_ACCEPT = ("descending t", "parallel moves", "destination j_t", "lens of the other sequence", "V not moved")


def clamp(x, lo, hi):
    return min(max(int(x), lo), hi)


def pos_positions(L, Sq, cap, offs):
    """[table row] of the Sq new rows of a sequence whose length (the new rows counted) is L; offs: its Sq offsets (any int32)"""
    first = clamp(L, 1, cap) - Sq
    return [max(first + clamp(o, 0, Sq - 1), 0) for o in offs]


def rope_append_pos(Q, Kn, Vn, Kc, Vc, table, lens, offs, interleaved, kds=None, vds=None, block_table=None, wrong=None):
    """-> (Qout bf16, K cache, V cache): rope_check.rope_append with row i rotated by offs[b][i] (int, [B][Sq]) instead of i"""
    B, _, Sq, _ = Kn.shape
    cap = Kc.shape[2] * (block_table.shape[1] if block_table is not None else 1)
    assert table.shape[0] >= cap and wrong in (None,) + WRONG_ROPE
    L = [cap if lens is None else int(lens[b]) for b in range(B)]
    offs = [[int(o) for o in row] for row in offs]
    use = offs
    if wrong == "offsets of batch 0":
        use = [offs[0]] * B
    if wrong == "offsets by cache position":       # the offset looked up under the row's cache position, not its index
        use = [[offs[b][clamp(clamp(L[b], 1, cap) - Sq + i, 0, Sq - 1)] for i in range(Sq)] for b in range(B)]
    pos = torch.tensor([pos_positions(L[b], Sq, cap, use[b]) for b in range(B)], dtype=torch.int64)
    qpos = torch.tensor([rc.q_positions(L[b], Sq, cap) for b in range(B)], dtype=torch.int64) if wrong == "Q at base + i" else pos
    Qout, Krot = rc.rotate(Q, table, qpos, interleaved), rc.rotate(Kn, table, pos, interleaved)
    if wrong == "offset moves the slot":           # row i stored where row clamp(off) belongs
        Kperm, Vperm = Krot.clone(), Vn.clone()
        for b in range(B):
            for i in range(Sq):
                Kperm[b, :, clamp(offs[b][i], 0, Sq - 1)] = Krot[b, :, i]
                Vperm[b, :, clamp(offs[b][i], 0, Sq - 1)] = Vn[b, :, i]
        Krot, Vn = Kperm, Vperm
    return Qout, kc.append(Krot, Kc, lens, kds, block_table), kc.append(Vn, Vc, lens, vds, block_table)


def accept(Kc, Vc, lens, idx, nacc, Sq, block_table=None, wrong=None):
    """-> (K cache, V cache) after the acceptance: caches int16 / uint8 [B, Hkv, cap, d] or (block_table: int [B, max_pages], any
    values) pools [P, Hkv, page, d]; lens: B ints or None; idx [B][Sq], nacc [B]: any int32"""
    assert wrong in (None,) + WRONG_ACCEPT
    B = len(nacc)
    page = Kc.shape[2]
    cap = page * block_table.shape[1] if block_table is not None else Kc.shape[2]
    out = [Kc.clone(), Vc.clone()]

    def row(c, b, p):
        """the [Hkv, d] view of position p of sequence b in cache c, or None: negative, or its page entry out of range"""
        if p < 0:
            return None
        if block_table is None:
            return c[b, :, p]
        e = int(block_table[b, p // page])
        return c[e, :, p % page] if 0 <= e < c.shape[0] else None

    for b in range(B):
        L = min(cap if lens is None else int(lens[b]), cap)
        if L <= 0:
            continue
        base = L - Sq
        n = clamp(nacc[(b + 1) % B] if wrong == "lens of the other sequence" else nacc[b], 0, Sq)
        order = list(range(n))
        if wrong == "descending t":
            order.reverse()
        if wrong == "parallel moves":                # a lane per move, in an order of the hardware's: the odd moves land first and
            order = order[1::2] + order[0::2]        # the even ones read the cache they have already written
        for ci, c in enumerate(out):
            if wrong == "V not moved" and ci == 1:
                continue
            for t in order:
                j = clamp(idx[b][t], 0, Sq - 1)
                to = j if wrong == "destination j_t" else t
                src = row(c, b, base + j)
                dst = row(c, b, base + to)
                if src is None or dst is None or (j == t and wrong is None):
                    continue
                dst.copy_(src.clone())
    return out[0], out[1]


def tree_path(parents, leaf):
    """(accept_idx [Sq], n) of ONE sequence by an ancestor walk: root first, the tail padded with Sq - 1"""
    Sq = len(parents)
    path, node = [], clamp(leaf, 0, Sq - 1)
    while node >= 0:
        path.append(node)
        node = int(parents[node])
    path.reverse()
    return path + [Sq - 1] * (Sq - len(path)), len(path)


def depths(parents):
    d = []
    for i, p in enumerate(parents):
        d.append(0 if p < 0 else d[p] + 1)
    return d


def binary(Sq):
    """a complete binary tree in level order: node i's parent is (i - 1) // 2"""
    return [(i - 1) // 2 if i else -1 for i in range(Sq)]


def star(Sq):
    """one root, every other node its child"""
    return [-1] + [0] * (Sq - 1)


def chain(Sq):
    return [i - 1 for i in range(Sq)]


def random_tree(Sq, seed):
    g = torch.Generator().manual_seed(seed)
    return [-1] + [int(torch.randint(0, i, (1,), generator=g)) for i in range(1, Sq)]


def first_difference(name, got, want):
    """None, or 'name[b, head, row, col]: ...' of the first element that differs (rope_check.assert_same's message)"""
    try:
        rc.assert_same(name, got, want)
    except AssertionError as e:
        return str(e)
    return None
