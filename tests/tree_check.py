"""Checker shared by the tree-masked verification tests (tests/test_tree_abi.py, test_tree.py, test_tree_memory_contract.py): the mask
families, the condition that a case's mask matters, the read-back probe and the calls the GPU tests make alike; the visibility rule of
flash_attention_tree as include/flash_attention.h states it and the float64 ground truth under it are kv_cache_check's.  Plain torch on the CPU for everything but the calls; the criterion is kv_cache_check.assert_close,
unchanged (1e-3 + 1e-3 |ref| on O, 2e-4 + 2e-6 |ref| on the LSE).

Rule.  With len the sequence's length, base = len - Sq, lim_i = max(base + i + 1, 1) and lo_i = max(lim_i - W, 0) (W = 0: 0), row i sees
key k iff lo_i <= k < lim_i (the causal mask under the window) AND (k < base, or bit k - base of the row's word is set, or
k == lim_i - 1): kv_cache_check.visible with ``words``, and kv_cache_check.reference with ``words`` is the explicit float64 softmax over
it, then the sinks (its ``vis``: a visibility of the caller's own per (sequence, head) -- the wrong kernels test_tree_abi.py emulates).

Masks.  A case's words are a list [B][Sq] of Python ints (unsigned 64-bit patterns); kv_cache_check.words_tensor makes the int64
tensor the call takes.  Families: "chain" (bits 0 .. i), "ones" (every bit), "star" (the self bit alone: every node hangs off the
prefix), "binary" (the heap-shaped tree, parent (i - 1) // 2) and "random" (a seeded parent array, parent uniform in [-1, i));
`words_of_parents` is the brute-force ancestor walk.  The first two are the causal twin.

`assert_masks_matter`: a case whose mask changes nothing tests nothing.  On the reference, for every sequence of a non-chain case whose
prefix base is in [0, 120] and that has rows i >= 2: at least HALF of the (head, row i >= 2) pairs differ from the causal reference by
more than 4 x the tolerance in some element of O or in the LSE.  (Measured on the CPU, N(0, 1) data, scale d^-1/2: the share is 1.0 for
star and binary masks at Sq 5 / 16 / 33 / 64 and prefixes 0 / 3 / 120; at prefix 300 and Sq = 5 it falls to 1/3, hence the cap.)
"""
import itertools

import torch

import kv_cache_check as kv
import sink_check as sc
from kv_cache_check import DEV, Cache, assert_close, fa, i32, ratios, reference, visible, words_tensor

FULL = (1 << 64) - 1
FAMILIES = ("chain", "ones", "star", "binary", "random")
TWINS = ("chain", "ones")                    # the families that are the causal mask
B, HKV, CAP = sc.B, sc.HKV, sc.CAP
f32, bf16 = torch.float32, torch.bfloat16
MAX_Q = fa.FA_TREE_MAX_Q


# ---- masks ------------------------------------------------------------------------------------------------------------------------
def parents_of(family, Sq, seed=0):
    """the parent array of a family that is a tree: -1 for a root"""
    if family == "chain":
        return [i - 1 for i in range(Sq)]
    if family == "star":
        return [-1] * Sq
    if family == "binary":
        return [(i - 1) // 2 if i else -1 for i in range(Sq)]
    assert family == "random", family
    g = torch.Generator().manual_seed(4000 + 97 * Sq + seed)
    return [int(torch.randint(-1, i, (1,), generator=g)) if i else -1 for i in range(Sq)]


def words_of_parents(parents):
    """brute force: word i = the bits of i and of every node on the walk from i to its root"""
    out = []
    for i in range(len(parents)):
        w, j = 0, i
        while j >= 0:
            w |= 1 << j
            j = parents[j]
        out.append(w)
    return out


def words_of(family, Sq, seed=0):
    return [FULL] * Sq if family == "ones" else words_of_parents(parents_of(family, Sq, seed))


def effective(words, Sq):
    """what the rule reads of a sequence's words: bits 0 .. i of word i, the self bit forced"""
    return [(w & ((1 << (i + 1)) - 1)) | (1 << i) for i, w in enumerate(words[:Sq])]


# ---- when a mask matters --------------------------------------------------------------------------------------------------------
def differing_rows(O, lse, refO, refL, factor=4.0):
    """bool [B, H, Sq]: the row is off the reference by more than `factor` x the tolerance in some element of O, or in the LSE"""
    r, lr = ratios(O, lse, refO, refL)
    return (r > factor).any(-1) | (lr > factor)


def assert_masks_matter(refO, refL, causalO, causalL, lens, families, what=""):
    """module docstring; returns the shares of the sequences it applies to"""
    Sq = refO.shape[2]
    shares = []
    for b, L in enumerate(lens):
        if families[b] in TWINS or Sq < 3 or not 0 <= L - Sq <= 120:
            continue
        share = differing_rows(refO[b:b + 1, :, 2:], refL[b:b + 1, :, 2:], causalO[b:b + 1, :, 2:], causalL[b:b + 1, :, 2:]).double().mean().item()
        assert share >= 0.5, f"{what}: only {share:.2f} of sequence {b}'s rows i >= 2 ({families[b]}, prefix {L - Sq}) differ from the causal reference"
        shares.append(share)
    return shares


# ---- what the GPU tests build and run alike -------------------------------------------------------------------------------------------
def lengths(Sq):
    """the length pairs of a row count: the draft's keys [len - Sq, len) inside one tile (prefixes 3 and 120: the cases that must
    matter; 300 and the full capacity), across the 128- and the 256-key tile starts, at len == Sq (no prefix) and at len < Sq"""
    return ((Sq + 3, 300), (128 + (Sq + 1) // 2, 256 + Sq // 2), (Sq, max(Sq - 3, 1)), (Sq + 120, CAP))


def case_words(Sq, n, families=("star", "binary", "random")):
    """the words of the two sequences of the n-th case: two different families of the rotation -> (words [B][Sq], names [B])"""
    names = [families[(n + b) % len(families)] for b in range(B)]
    return [words_of(f, Sq, seed=n + b) for b, f in enumerate(names)], names


def attend(c, Q, lens, words, **kw):
    """(O, LSE) of one tree call through the Python fronts; c: kv_cache_check.Cache.device(); words: the int64 device tensor"""
    if c["table"] is not None:
        return fa.flash_attention_tree_paged(Q, c["K"], c["V"], c["table"], words, lens, return_lse=True, **c["ds"], **kw)
    return fa.flash_attention_tree(Q, c["K"], c["V"], words, lens, return_lse=True, **c["ds"], **kw)


def twin(c, Q, lens, **kw):
    """the causal twin on the same tensors: flash_attention_sink_decode* up to FA_DECODE_MAX_Q rows, flash_attention_sink_extend* above"""
    return kv.attend("decode" if Q.shape[2] <= fa.FA_DECODE_MAX_Q else "extend", c, Q, lens, is_causal=True, **kw)


def run_parity(d, G, form, rows, run=True):
    """every case of (row count, length pair, window) against the float64 reference, under forced splits 1, 2, 3 and the library's own
    choice; the masks rotate through star / binary / random, two different ones per case.  run = False: the references and
    assert_masks_matter alone (no GPU).  Returns the number of sequences assert_masks_matter applied to"""
    page, fp8 = form
    cache = Cache(d, page, fp8, 1400 + d + 7 * G)
    c = cache.device() if run else None
    sinks = sc.sinks_for(HKV * G)
    mattered = 0
    for n, (Sq, W) in enumerate(itertools.product(rows, sc.WINDOWS)):
        Q = sc.queries("decode", d, G, Sq, 11 * d + 1000 * G + Sq)
        for m, lens in enumerate(lengths(Sq)):
            words, names = case_words(Sq, n + m)
            what = f"tree d{d} G{G} Sq{Sq} lens{lens} window{W} {'/'.join(names)} {sc.FORM_IDS[sc.FORMS.index(form)]}"
            refO, refL = reference(Q, cache.refK, cache.refV, lens, True, W, words=words, sinks=sinks)
            chain = [words_of("chain", Sq)] * B
            mattered += len(assert_masks_matter(refO, refL, *reference(Q, cache.refK, cache.refV, lens, True, W, words=chain, sinks=sinks), lens, names, what))
            if not run:
                continue
            wt = words_tensor(words).to(DEV)
            for ns in (1, 2, 3, 0):
                O, lse = attend(c, Q.to(DEV), i32(lens), wt, window=W, num_splits=ns, sinks=sinks.to(DEV), out_dtype=f32)
                assert_close(O, lse, refO, refL, f"{what} splits{ns}")
    return mattered


def probe_values(Sq, lens, d):
    """V [B, HKV, CAP, d] bf16 of the read-back probe: V[base + j][j] = 1 for every node j whose key exists, 0 elsewhere"""
    V = torch.zeros(B, HKV, CAP, d)
    for b, L in enumerate(lens):
        for j in range(Sq):
            if L - Sq + j >= 0:
                V[b, :, L - Sq + j, j] = 1.0
    return V.to(bf16)


def expected_bits(Sq, L, W, words):
    """(bits float64 [Sq, Sq], n [Sq]) of one sequence: bits[i, j] = row i sees node j (0 where the node's key does not exist), n_i =
    the keys row i sees"""
    vis = visible(L, Sq, True, W, words)
    bits = torch.zeros(Sq, Sq, dtype=torch.float64)
    for j in range(Sq):
        if L - Sq + j >= 0:
            bits[:, j] = vis[:, L - Sq + j].double()
    return bits, vis.sum(-1).double()


def assert_read_back(O, lens, W, words, what):
    """O [B, H, Sq, d] fp32 of a probe call (Q = 0, probe_values): O[i][j] n_i is bit j of row i's effective word, every row, head and
    sequence within 1e-3 of 0 or 1 and equal to the rule's bit; the columns beyond Sq hold 0"""
    O = O.double().cpu()
    Sq = O.shape[2]
    for b, L in enumerate(lens):
        bits, n = expected_bits(Sq, int(L), W, words[b])
        got = O[b, :, :, :Sq] * n[None, :, None]
        near = torch.minimum(got.abs(), (got - 1.0).abs())
        assert (near <= 1e-3).all(), f"{what}: sequence {b}: a read-back value {near.max().item():.3e} away from 0 and 1"
        wrong = (got.round() != bits[None]).nonzero()
        assert not len(wrong), f"{what}: sequence {b} (len {L}): head {int(wrong[0][0])} row {int(wrong[0][1])} node {int(wrong[0][2])} " \
                               f"reads {got[tuple(wrong[0])].item():.3f}, the rule says {bits[wrong[0][1], wrong[0][2]].item():.0f}"
        assert not O[b, :, :, Sq:].any(), f"{what}: sequence {b}: a column beyond the nodes is not 0"
