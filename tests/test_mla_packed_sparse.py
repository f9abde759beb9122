"""GPU tests of sparse MLA decode on the packed latent row: bit identity with the bf16 sparse call on the dequantised
cache and float64 parity, single-key probes of the scale map and the rope offset, poison in what no key names, one replayed graph."""
import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
import mla_sparse_check as sc
from kv_cache_check import DEV, fa
from test_mla_packed_append import FORMS, ROW, write

pytestmark = pytest.mark.gpu
BLOCK_SCALES = torch.tensor([1.0, 8.0, 1.0 / 64, 300.0]).repeat_interleave(128)   # the four scales differ by orders of magnitude
# the softmax scale that keeps that data's scores at the N(0, 1) the tolerance is stated for: (the sum of the columns' variances) ** -0.5
SCALE = float((BLOCK_SCALES ** 2).sum() + mc.DR) ** -0.5
packed_cache = lambda KV: write((KV[..., :mc.DL].float() * BLOCK_SCALES).bfloat16(), KV[..., mc.DL:])


def logical(rows):
    codes, scales = rows[..., :512].contiguous(), rows[..., 512:528].contiguous().view(torch.float32)
    latent = (codes.view(kc.F8).float() * scales.repeat_interleave(128, -1)).bfloat16()
    return torch.cat([latent, rows[..., 528:].contiguous().view(torch.bfloat16)], -1)


def attend(Q, rows, idx, lens, page, table=None, pool=None, **kw):
    """(O, LSE) of the packed sparse call on the cache `rows` [B, CAPACITY, 656] in the form `page` (0: contiguous)"""
    kw = dict(dict(return_lse=True, out_dtype=torch.float32), **kw)
    if not page:
        return fa.flash_attention_mla_sparse_decode_packed(Q.to(DEV), rows.to(DEV), idx.to(DEV), kc.i32(lens), **kw)
    table = mc.table_for(Q.shape[0], page, 77) if table is None else table
    pool = mc.pool_of(rows, table, page) if pool is None else pool
    return fa.flash_attention_mla_sparse_decode_paged_packed(Q.to(DEV), pool.to(DEV), table.to(DEV), idx.to(DEV), kc.i32(lens), **kw)


@pytest.mark.parametrize("page", FORMS)
@pytest.mark.parametrize("H,Sq", [(1, 1), (65, 3), (128, 2)])
def test_the_bf16_sparse_call_on_the_dequantised_cache_bit_for_bit_and_float64_parity(H, Sq, page):
    Q, KV = mc.data(H, Sq, 7000 + 10 * H + Sq)
    rows = packed_cache(KV)
    twin = sc.Cache(logical(rows), False, page)
    for k, topk in enumerate((1, 33, 200)):
        lens = mc.lengths(Sq, page)[(k + 2) % 5]
        idx = sc.index_lists(Sq, topk, lens, 7100 + topk)
        for causal in (False, True):
            ref = sc.reference(Q, twin.logical, idx, lens, causal, SCALE)
            for ns in (1, 3, 0):
                what = f"H {H} Sq {Sq} page {page} topk {topk} lens {lens} causal {causal} splits {ns}"
                kw = dict(is_causal=causal, num_splits=ns, scale=SCALE, out_dtype=torch.float32)
                (O, lse), (tO, tl) = attend(Q, rows, idx, lens, page, **kw), sc.attend(Q, twin, idx, lens, **kw)
                assert kc.same_bits(O, tO) and kc.same_bits(lse, tl), what
                sc.assert_close(O, lse, *ref, what)


@pytest.mark.parametrize("page", FORMS)
def test_single_key_probes_of_the_scale_map_and_the_rope_offset(page):
    """topk = 1.  (1) Q = 0 against column-coded codes under four distinct scales, no powers of two: the weight is exactly 1, so O is the
    dequantised row bit for bit and LSE = 0.  (2) zero codes, an index-coded rope and a rope-only Q: head h reads rope column h alone"""
    H, pos, col = 64, torch.tensor([5, 200, mc.CAPACITY - 1]), torch.arange(512)
    rows = torch.zeros(mc.B, mc.CAPACITY, ROW, dtype=torch.uint8)
    rows[..., :512] = ((col * 7 + 3) % 126 + 128 * (col % 2)).to(torch.uint8)                         # (no NaN code)
    rows[..., 512:528] = torch.tensor([0.3, 1.7, 0.011, 23.0]).view(torch.uint8)
    rope = (((torch.arange(mc.CAPACITY)[:, None] * 64 + torch.arange(64)) % 251 - 125) / 16.0).bfloat16()
    rows[..., 528:] = rope.view(torch.uint8)
    idx = pos.to(torch.int32).reshape(mc.B, 1, 1)
    Q = torch.zeros(mc.B, H, 1, mc.D, dtype=torch.bfloat16)
    O, lse = attend(Q, rows, idx, None, page)
    bad = (O.cpu() != logical(rows)[torch.arange(mc.B), pos][:, None, None, :512].float()).nonzero()
    assert not len(bad) and (lse == 0).all(), f"first wrong (b, h, i, column): {bad[:1].tolist()}"

    rows[..., :512] = 0
    Q[:, torch.arange(H), 0, mc.DL + torch.arange(H)] = 1.0
    O, lse = attend(Q, rows, idx, None, page, scale=1.0)                                            # LSE[b, h] = rope[pos_b, h]
    assert (O == 0).all()
    sc.assert_close(O, lse, *sc.reference(Q, logical(rows), idx, [mc.CAPACITY] * mc.B, False, 1.0), "rope probe")


@pytest.mark.parametrize("page", FORMS)
def test_poison_in_every_row_no_key_names_never_enters_the_result(page):
    """NaN codes, scales and rope in every row no valid slot names, 0xFF in spare pages, wild table entries for pages without a key"""
    H, Sq, lens = 16, 3, [33, 130, mc.CAPACITY - 1]
    Q, KV = mc.data(H, Sq, 7300)
    rows = packed_cache(KV)
    idx = sc.index_lists(Sq, 96, lens, 7301)
    lim = torch.tensor([[sc.limit(L, Sq, i, True) for i in range(Sq)] for L in lens])[..., None]
    named = torch.zeros(mc.B, mc.CAPACITY + 1, dtype=torch.bool)                   # (the last column takes the slots that are no keys)
    named = named.scatter_(1, torch.where((idx >= 0) & (idx < lim), idx, mc.CAPACITY).long().flatten(1), True)[:, :-1]
    nan_row = torch.cat([torch.tensor([0x7F, 0xFF], dtype=torch.uint8).repeat(256), torch.full((4,), float("nan")).view(torch.uint8),
                         torch.full((64,), float("nan"), dtype=torch.bfloat16).view(torch.uint8)])
    junk = torch.where(named[..., None], rows, nan_row)
    table = mc.table_for(mc.B, page or 16, 77)                                     # (the contiguous form reads neither table nor pool)
    keyless = ~named.reshape(mc.B, -1, page or 16).any(-1)
    wild = torch.where(keyless, torch.tensor([[-1], [2 ** 31 - 1], [table.numel() + 5]], dtype=torch.int32), table)
    pool = mc.pool_of(junk ^ 0xFF, table, page) ^ 0xFF if page else None           # (pool_of leaves the spare pages zero: here 0xFF)
    kw = dict(is_causal=True, num_splits=2, scale=SCALE)
    clean, dirty = attend(Q, rows, idx, lens, page, **kw), attend(Q, junk, idx, lens, page, table=wild, pool=pool, **kw)
    assert keyless.any() and torch.isfinite(clean[0]).all() and kc.same_bits(clean[0], dirty[0]) and kc.same_bits(clean[1], dirty[1])


def test_one_replayed_graph_of_the_append_and_the_read():
    """kv_lens += 1; append; read -- captured once, replayed twice after kv_lens and indices changed in place"""
    H, page, topk = 16, 16, 96
    Q, KV = mc.data(H, 1, 7400)
    table = mc.table_for(mc.B, page, 84)
    pool = mc.pool_of(packed_cache(KV), table, page)
    new = kc.randn((mc.B, 1, mc.D), 7403, torch.bfloat16).to(DEV)
    Qd, td = Q.to(DEV), table.to(DEV)
    ws = torch.empty(fa.decode_workspace_size(mc.B, H, 1, mc.DL, 3), dtype=torch.uint8, device=DEV)

    def step(pool_d, lens_d, idx_d, O):
        lens_d += 1
        fa.mla_cache_append_paged_packed(new[..., :mc.DL], new[..., mc.DL:], pool_d, td, lens_d, scale_fmt="pow2")
        return fa.flash_attention_mla_sparse_decode_paged_packed(Qd, pool_d, td, idx_d, lens_d, SCALE, True, num_splits=3, return_lse=True,
                                                                 O=O, workspace=ws)[1]

    state = lambda: (pool.to(DEV), kc.i32([30, 15, 100]), torch.zeros(mc.B, 1, topk, dtype=torch.int32, device=DEV),
                     torch.zeros((mc.B, H, 1, mc.DL), dtype=torch.float32, device=DEV))
    g, e = state(), state()
    step(*e)                                               # (first calls outside the capture; the first replay writes the same rows again)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_lse = step(*g)
    for lens, seed in (([30, 15, 100], 7401), ([200, 63, 300], 7402)):
        now = [L + 1 for L in lens]
        idx = sc.index_lists(1, topk, now, seed)
        idx[:, 0, 0] = torch.tensor(lens, dtype=torch.int32)                  # (the row this step appends is a key)
        for s in (g, e):
            s[1].copy_(kc.i32(lens))
            s[2].copy_(idx.to(DEV))
        graph.replay()
        e_lse = step(*e)
        torch.cuda.synchronize()
        assert g[1].tolist() == e[1].tolist() == now and torch.equal(g[0], e[0]) and kc.same_bits(g[3], e[3]) and kc.same_bits(g_lse, e_lse)
        ref = sc.reference(Q, logical(mc.gathered(g[0].cpu(), table)), idx, now, True, SCALE)
        sc.assert_close(g[3], g_lse, *ref, f"replay with lens {lens}")
