"""GPU tests of the MLA indexer (mla_index_topk / mla_index_topk_paged) against a few lines of float64 torch:
the logit formula, then a stable sort by (-logit, position), the first n sorted ascending, -1 after them."""
import functools

import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
from kv_cache_check import DEV, F8, fa

pytestmark = pytest.mark.gpu
CAP, B, PAGE = mc.CAPACITY, mc.B, 16
LENS = ([1, 31, 127], [32, 128, CAP], [33, 129, PAGE], [2, PAGE + 1, CAP - 1])
TOPKS = (1, 32, 33, 200, 2048)


def ref_logits(Q, W, K, ks):
    """float64 [B, Sq, capacity] of the fp8 tensors' values"""
    s = torch.einsum("bihd,bkd->bihk", Q.double(), K.double()).clamp(min=0)
    return (s * W.double()[..., None]).sum(2) * ks.double()[:, None, :]


def below_limit(lens, Sq, causal, cap=CAP):
    """bool [B, Sq, capacity]: k < lim_i"""
    lim = torch.tensor([[max(mc.clamp(L, cap) - Sq + i + 1, 1) if causal else mc.clamp(L, cap) for i in range(Sq)] for L in lens])
    return torch.arange(cap)[None, None] < lim[..., None]


def select(logits, vis, topk):
    """the contract's indices of float64 logits: per row the n = min(topk, lim) largest, ties to the lower position, ascending, then -1"""
    out = torch.full(vis.shape[:2] + (topk,), -1, dtype=torch.int32)
    for b, i in torch.cartesian_prod(torch.arange(vis.shape[0]), torch.arange(vis.shape[1])).tolist():
        lim = int(vis[b, i].sum())
        order = torch.sort(-logits[b, i, :lim].double(), stable=True).indices[:topk]
        out[b, i, :len(order)] = order.sort().values
    return out


def run(page, Q, W, K, ks, lens, topk, causal, table=None, pool=None, ks_pool=None, **kw):
    """(indices, logits) on the CPU through the front of the form; K: e4m3fn values as fp32, stored as their bytes"""
    bytes_ = K.to(F8).view(torch.uint8) if K.dtype != torch.uint8 else K
    q = Q.to(F8).to(DEV)
    if not page:
        got = fa.mla_index_topk(q, W.to(DEV), bytes_.view(F8).to(DEV), ks.to(DEV), topk, kc.i32(lens), causal, return_logits=True, **kw)
    else:
        table = kc.random_table(Q.shape[0], K.shape[1] // page, 91) if table is None else table
        pool = kc.scatter(bytes_[:, None], table, page)[:, 0] if pool is None else pool
        ks_pool = kc.scatter(ks[:, None, :, None], table, page)[:, 0, :, 0] if ks_pool is None else ks_pool
        got = fa.mla_index_topk_paged(q, W.to(DEV), pool.contiguous().view(F8).to(DEV), ks_pool.contiguous().to(DEV), table.to(DEV), topk,
                                      kc.i32(lens), causal, return_logits=True, **kw)
    return got[0].cpu(), got[1].cpu()


@functools.lru_cache(maxsize=None)
def exact_data(Sq):
    """integers: every logit a multiple of 0.5 below 2^19, exact in fp32 in any order (128 * 9 * 2 * 64 * 2 < 2^24); ties are plentiful"""
    g = torch.Generator().manual_seed(7000 + Sq)
    Q = torch.randint(-3, 4, (B, Sq, 64, 128), generator=g).float()
    K = torch.randint(-3, 4, (B, CAP, 128), generator=g).float()
    W = torch.randint(-2, 3, (B, Sq, 64), generator=g).float()
    ks = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B, CAP), generator=g)]
    return Q, W, K, ks, ref_logits(Q, W, K, ks)


@functools.lru_cache(maxsize=None)
def random_data(Sq, cap, batch=B):
    """N(0, 1) rounded to e4m3fn, random W of both signs, positive scales"""
    g = torch.Generator().manual_seed(7100 + Sq + cap)
    Q = torch.randn((batch, Sq, 64, 128), generator=g).to(F8).float()
    K = torch.randn((batch, cap, 128), generator=g).to(F8).float()
    return Q, torch.randn((batch, Sq, 64), generator=g), K, torch.rand((batch, cap), generator=g) + 0.25


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Sq", [1, 3, 16])
@pytest.mark.parametrize("page", [0, PAGE])
def test_exact_data_logits_and_indices_equal_the_reference(page, Sq, causal):
    Q, W, K, ks, ref = exact_data(Sq)
    for lens in LENS:
        vis = below_limit(lens, Sq, causal)
        for topk in TOPKS:
            idx, logits = run(page, Q, W, K, ks, lens, topk, causal)
            assert torch.equal(logits.double()[vis], ref[vis]) and not (logits[vis] == 0).logical_and(logits[vis].signbit()).any(), (lens, topk)
            assert torch.equal(idx, select(ref, vis, topk)), (lens, topk)


@pytest.mark.parametrize("page", [0, PAGE])
def test_random_data_within_the_derived_bound_and_the_selection_exact(page):
    """|logit - ref| <= 2^-16 A, A = kScale sum_h |W_h| sum_d |q k|: n u with n = 256 >= 128 products + 64 heads + two multiplies,
    u = 2^-24.  One row of 5000 keys under topk 2048: all three radix passes discriminate"""
    Sq, cap, lens, topk = 2, 5008, [5000, 777], 2048
    Q, W, K, ks = random_data(Sq, cap, 2)
    vis = below_limit(lens, Sq, True, cap)
    idx, logits = run(page, Q, W, K, ks, lens, topk, True)
    A = torch.einsum("bihd,bkd->bihk", Q.double().abs(), K.double().abs())
    A = (A * W.double().abs()[..., None]).sum(2) * ks.double()[:, None, :]
    ratio = ((logits.double() - ref_logits(Q, W, K, ks)).abs() / (2.0 ** -16 * A))[vis]
    print(f"page {page}: worst |logit - ref| / (2^-16 A) = {ratio.max().item():.4f}")
    assert (ratio <= 1).all()
    assert torch.equal(idx, select(logits, vis, topk))


@pytest.mark.parametrize("page", [0, PAGE])
def test_poison_beyond_the_lengths_and_equal_bits_across_forms_and_runs(page):
    """NaN bytes and NaN scales in every row at or beyond the lengths and in the spare pages, wild entries for the unread pages: the
    bits of the clean run; paged equals contiguous on the gathered copy; two runs are equal"""
    Sq, lens, topk = 3, [130, 33, CAP - 1], 100
    Q, W, K, ks = random_data(Sq, CAP)
    vis = below_limit(lens, Sq, True)
    idx, logits = run(0, Q, W, K, ks, lens, topk, True)
    again = run(page, Q, W, K, ks, lens, topk, True)
    assert torch.equal(idx, again[0]) and kc.same_bits(logits[vis], again[1][vis])
    bad, bad_ks = K.to(F8).view(torch.uint8).clone(), ks.clone()
    for b, L in enumerate(lens):
        bad[b, L:], bad_ks[b, L:] = 0x7F, float("nan")
    extra = {}
    if page:
        table = kc.random_table(B, CAP // page, 91)
        pool, ks_pool = kc.scatter(bad[:, None], table, page)[:, 0], kc.scatter(bad_ks[:, None, :, None], table, page)[:, 0, :, 0]
        used = torch.zeros(pool.shape[0], dtype=torch.bool)
        used[table.long().reshape(-1)] = True
        pool[~used], ks_pool[~used] = 0x7F, float("nan")
        wild = table.clone()
        for b, L in enumerate(lens):
            wild[b, -(-L // page):] = torch.tensor([-1, 2 ** 31 - 1, pool.shape[0]], dtype=torch.int32).repeat(CAP)[:CAP // page - -(-L // page)]
        extra = dict(table=wild, pool=pool, ks_pool=ks_pool)
    dirty = run(page, Q, W, bad, bad_ks, lens, topk, True, **extra)
    assert torch.isfinite(logits[vis]).all() and torch.equal(idx, dirty[0]) and kc.same_bits(logits[vis], dirty[1][vis])


def sparse_step(Qi, W, Ki, ks, Q, KV, ld, **kw):
    idx = fa.mla_index_topk(Qi, W, Ki, ks, CAP, ld, True, **kw)
    return fa.flash_attention_mla_sparse_decode(Q, KV, idx, ld, is_causal=True, num_splits=2, return_lse=True, out_dtype=torch.float32)


def step_inputs(Sq):
    Qi, W, Ki, ks = random_data(Sq, CAP)
    Q, KV = mc.data(16, Sq, 7200)
    return [Qi.to(F8).to(DEV), W.to(DEV), Ki.to(F8).to(DEV), ks.to(DEV), Q.to(DEV), KV.to(DEV)]


def test_end_to_end_topk_above_every_length_is_the_dense_decode():
    args, lens = step_inputs(3), [CAP, 100, 3]
    O, lse = sparse_step(*args, kc.i32(lens))
    dO, dlse = fa.flash_attention_mla_decode(args[4], args[5], kc.i32(lens), is_causal=True, return_lse=True, out_dtype=torch.float32)
    kc.assert_close(O, lse, dO.double().cpu(), dlse.double().cpu(), "indexer + sparse decode against the dense decode")


def test_one_graph_of_indexer_and_sparse_decode_reads_the_lengths_of_the_moment():
    args, states = step_inputs(2), ([300, 77, CAP], [64, CAP, 31], [200, 1, 200])
    ld = kc.i32(states[0])
    bufs = dict(logits=torch.empty((B, 2, CAP), device=DEV), indices=torch.empty((B, 2, CAP), dtype=torch.int32, device=DEV))
    sparse_step(*args, ld, **bufs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        O, lse = sparse_step(*args, ld, **bufs)
    for lens in states:
        ld.copy_(kc.i32(lens))
        graph.replay()
        torch.cuda.synchronize()
        idx = bufs["indices"].clone()
        eager = sparse_step(*args, ld)
        assert torch.equal(O, eager[0]) and torch.equal(lse, eager[1]), lens
        assert torch.equal(idx, fa.mla_index_topk(*args[:4], CAP, ld, True)), lens
