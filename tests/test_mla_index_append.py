"""GPU tests of the MLA index-cache append (mla_index_append / _paged): whole tensors compared for equality of
bytes and of fp32 bits with mla_index_append_check's elementwise reference, a sentinel everywhere else; exact probes that pin the
transform without the reference; and the one-graph step append -> indexer -> sparse decode."""
import functools

import numpy as np
import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
import mla_index_append_check as ic
from kv_cache_check import DEV, F8, fa

pytestmark = pytest.mark.gpu
B, CAP, H, D = ic.B, ic.CAP, ic.H, ic.D
ROPES = {"none": None, "neox": False, "gptj": True}       # name -> interleaved
W_SCALE = 128 ** -0.5 * 64 ** -0.5


@functools.lru_cache(maxsize=None)
def rope_table():
    return fa.rope_table(CAP, 64).cpu()


def new_rows(shape, seed):
    """bf16 rows [.., 128] as a strided slice of a wider projection: N(0, 9) with an all-zero row (the amax floor), a row of -0, a tiny
    and a huge one"""
    proj = kc.randn(shape[:-1] + (D + 32,), seed, torch.bfloat16) * 3
    flat = proj.view(-1, D + 32)
    flat[0], flat[-1, 16:80] = 0.0, -0.0
    if len(flat) > 2:
        flat[1] *= 1e-9
        flat[2] *= 1e28
    return proj, (lambda t: t[..., 16:16 + D])


def append(page, k, cache, scales, lens, table=None, **kw):
    """the front of the form on device copies -> ((cache bytes, scales) on the host, what the front returned)"""
    cd, sd = cache.to(DEV), scales.to(DEV)
    if page:
        out = fa.mla_index_append_paged(k, cd.view(F8), sd, table.to(DEV), kc.i32(lens), **kw)
    else:
        out = fa.mla_index_append(k, cd.view(F8), sd, kc.i32(lens), **kw)
    torch.cuda.synchronize()
    return (cd.cpu(), sd.cpu()), out


def rope_kw(rope):
    il = ROPES[rope]
    return {} if il is None else dict(cos_sin=rope_table().to(DEV), interleaved=il)


def reference(x, lens, rope, fmt):
    """x bf16 [B, heads, Sq, 128] -> (codes, scales) under the rotation of the case"""
    il = ROPES[rope]
    return ic.transform(x, fmt == "pow2", None if il is None else rope_table(), ic.positions(lens, x.shape[2]), bool(il))


@pytest.mark.parametrize("rope", list(ROPES))
@pytest.mark.parametrize("fmt", ["f32", "pow2"])
@pytest.mark.parametrize("Sq", [1, 5, 16, 70])           # 70: across a 64-position block and the 16-position waves, from an unaligned start
@pytest.mark.parametrize("page", [0, 16])
def test_every_byte_of_the_cache_and_every_scale(page, Sq, fmt, rope):
    proj, part = new_rows((B, Sq, D), 8000 + Sq)
    kd = part(proj.to(DEV))
    assert not kd.is_contiguous()
    pg = page or 128
    for lens in ([0, max(Sq - 1, 1), CAP + 5], [pg - 1, pg, pg + 1], [-3, CAP, 2 * pg + 7]):
        table = ic.table_for(B, page, 85 + Sq) if page else None
        before = ic.blank(page)
        got, out = append(page, kd, *before, lens, table, scale_fmt=fmt, **rope_kw(rope))
        codes, s = reference(part(proj)[:, None], lens, rope, fmt)
        want = ic.expected(*before, codes[:, 0], s[:, 0], lens, table, page)
        assert out is None and not ic.same(want, before) and ic.same(got, want), (lens, int((got[0] != want[0]).sum()))


@pytest.mark.parametrize("rope", list(ROPES))
@pytest.mark.parametrize("Sq", [1, 3, 16])
def test_the_q_side_writes_every_row_of_qidx_and_w(Sq, rope):
    """Qraw a permuted, sliced view; negative weights; sequences whose K rows are not written (L < Sq, L <= 0) still get their Q rows"""
    proj, part = new_rows((B, Sq, D), 8100 + Sq)
    store, _ = new_rows((B, H, Sq, D), 8200 + Sq)
    q = lambda t: t[..., 8:8 + D].permute(0, 2, 1, 3)          # [B, Sq, 64, 128], strides (B, S, H) all in play
    w = kc.randn((B, Sq, H), 8300 + Sq, torch.float32) - 0.25
    qd, wd = q(store.to(DEV)), w.to(DEV)
    assert not qd.is_contiguous() and (w < 0).any()
    for fmt, lens in (("pow2", [0, max(Sq - 1, 1), CAP + 5]), ("f32", [-3, 100, 17])):
        before = ic.blank(0)
        Qidx = torch.full((B, Sq, H, D), ic.SENTINEL, dtype=torch.uint8, device=DEV).view(F8)
        Wout = torch.full((B, Sq, H), ic.SCALE_SENTINEL, device=DEV)
        got, out = append(0, part(proj.to(DEV)), *before, lens, q=qd, w=wd, w_scale=W_SCALE, scale_fmt=fmt, Qidx=Qidx, W=Wout, **rope_kw(rope))
        assert out[0] is Qidx and out[1] is Wout
        codes, s = reference(part(proj)[:, None], lens, rope, fmt)
        assert ic.same(got, ic.expected(*before, codes[:, 0], s[:, 0], lens)), lens
        qc, qs = reference(q(store).permute(0, 2, 1, 3), lens, rope, fmt)                      # [B, 64, Sq, ..]
        want_w = (w.numpy() * qs.permute(0, 2, 1).numpy()).astype(np.float32) * np.float32(W_SCALE)
        assert ic.same((Qidx.cpu().view(torch.uint8), Wout.cpu()), (qc.permute(0, 2, 1, 3), torch.from_numpy(want_w))), (fmt, lens)


@pytest.mark.parametrize("fmt", ["f32", "pow2"])
def test_exact_probes_one_hot_rows_and_constant_rows(fmt):
    """row j = c e_j: every code has one magnitude, the signs are sign(c) times row j of the Sylvester matrix, and the scale is that of
    |c| 2^-3.5 rounded to bf16; a constant row: column 0 alone is not zero.  c a power of two: every product here is exact"""
    n = D + 2
    c = torch.where(torch.arange(D) % 2 == 0, 4.0, -0.5)
    x = torch.zeros(1, n, D)
    x[0, torch.arange(D), torch.arange(D)] = c
    x[0, D], x[0, D + 1] = 0.25, -2.0
    cache, scales = torch.full((1, n, D), ic.SENTINEL, dtype=torch.uint8, device=DEV), torch.full((1, n), ic.SCALE_SENTINEL, device=DEV)
    fa.mla_index_append(x.to(torch.bfloat16).to(DEV), cache.view(F8), scales, scale_fmt=fmt)
    codes, s = cache.cpu()[0], scales.cpu()[0].numpy()
    m = torch.cat([c.abs() * 2.0 ** -3.5, torch.tensor([0.25 * D, 2.0 * D]) * 2.0 ** -3.5]).to(torch.bfloat16).float().numpy()
    s0 = m * np.float32(1.0 / 448.0)
    want_s = np.array([2.0 ** np.ceil(np.log2(float(v))) for v in s0], dtype=np.float32) if fmt == "pow2" else s0
    assert s.tobytes() == want_s.tobytes()
    mag = torch.from_numpy(np.minimum(m / want_s, np.float32(448))).to(F8).view(torch.uint8)               # [n]
    j, k = torch.arange(D)[:, None], torch.arange(D)[None, :]
    parity = torch.zeros(D, D, dtype=torch.int64)
    for bit in range(7):
        parity ^= ((j & k) >> bit) & 1
    negative = (parity == 1) ^ (c < 0)[:, None]
    assert torch.equal(codes[:D], mag[:D, None] | (negative.to(torch.uint8) << 7)) and (mag[:D] & 0x7F).min() >= 0x70
    assert codes[D:, 0].tolist() == [int(mag[D]), int(mag[D + 1]) | 0x80] and (codes[D:, 1:] == 0).all()


def test_a_table_entry_outside_the_pool_skips_its_rows_and_nothing_else():
    page, Sq, lens = 16, 40, [100, 100, 100]               # positions 60 .. 99: pages 3 .. 6 of every sequence
    proj, part = new_rows((B, Sq, D), 8400)
    table = ic.table_for(B, page, 86)
    before = ic.blank(page)
    wild = table.clone()
    wild[0, 4], wild[1, 5] = -1, before[0].shape[0]
    got, _ = append(page, part(proj.to(DEV)), *before, lens, wild, scale_fmt="pow2", **rope_kw("neox"))
    codes, s = reference(part(proj)[:, None], lens, "neox", "pow2")
    assert ic.same(got, ic.expected(*before, codes[:, 0], s[:, 0], lens, table, page, skip={(0, 4), (1, 5)}))
    assert (got[0][table[0, 4]] == ic.SENTINEL).all() and (got[0][table[1, 5]] == ic.SENTINEL).all() and (got[0][table[2, 4]] != ic.SENTINEL).any()


def test_one_graph_append_indexer_sparse_decode():
    """kv_lens += 1; mla_index_append_paged; mla_index_topk_paged; flash_attention_mla_sparse_decode_paged: captured once, replayed twice,
    equal to the eager steps bit for bit (pools, scales, indices, O) and to the indexer run on the reference-built cache"""
    page, topk, start, heads = 16, 12, [30, 15, 100], 16
    table = ic.table_for(B, page, 87)
    td, cs = table.to(DEV), rope_table().to(DEV)
    fill = kc.randn((B, 100, D), 8500, torch.bfloat16)
    kn, qn = kc.randn((B, 1, D), 8501, torch.bfloat16), kc.randn((B, 1, H, D), 8502, torch.bfloat16)
    wn = kc.randn((B, 1, H), 8503, torch.float32)
    Q, KV = mc.data(heads, 1, 8504)
    Qd, KVd, knd, qnd, wnd = Q.to(DEV), mc.pool_of(KV, table, page).to(DEV), kn.to(DEV), qn.to(DEV), wn.to(DEV)
    ref = lambda x, lens: ic.transform(x, True, rope_table(), ic.positions(lens, x.shape[2]), False)
    codes, s = ref(fill[:, None], start)
    pool0 = ic.expected(*ic.blank(page), codes[:, 0], s[:, 0], start, table, page)

    def state():
        pool, sc = (t.to(DEV) for t in ic.blank(page))
        lens = kc.i32(start)
        fa.mla_index_append_paged(fill.to(DEV), pool.view(F8), sc, td, lens, cos_sin=cs)             # the cache fill: the K side alone
        bufs = dict(Qidx=torch.empty((B, 1, H, D), dtype=F8, device=DEV), W=torch.empty((B, 1, H), device=DEV),
                    logits=torch.empty((B, 1, CAP), device=DEV), indices=torch.empty((B, 1, topk), dtype=torch.int32, device=DEV),
                    O=torch.zeros((B, heads, 1, mc.DL), dtype=torch.float32, device=DEV))
        return pool, sc, lens, bufs

    def step(pool, sc, lens, bufs):
        lens += 1
        qi, w = fa.mla_index_append_paged(knd, pool.view(F8), sc, td, lens, q=qnd, w=wnd, cos_sin=cs, w_scale=W_SCALE, Qidx=bufs["Qidx"], W=bufs["W"])
        idx = fa.mla_index_topk_paged(qi, w, pool.view(F8), sc, td, topk, lens, True, logits=bufs["logits"], indices=bufs["indices"])
        fa.flash_attention_mla_sparse_decode_paged(Qd, KVd, td, idx, lens, is_causal=True, num_splits=1, O=bufs["O"])

    step(*state())                                         # (first calls outside the capture, on a state of their own)
    torch.cuda.synchronize()
    g, e = state(), state()
    assert ic.same((g[0].cpu(), g[1].cpu()), pool0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*g)
    want = pool0
    for n in (1, 2):
        graph.replay()
        step(*e)
        torch.cuda.synchronize()
        lens = [L + n for L in start]
        assert g[2].tolist() == e[2].tolist() == lens and torch.equal(g[0], e[0]) and kc.same_bits(g[1], e[1]), n
        assert all(kc.same_bits(g[3][k], e[3][k]) for k in ("Qidx", "W", "O", "indices")), n
        codes, s = ref(kn[:, None], lens)
        want = ic.expected(*want, codes[:, 0], s[:, 0], lens, table, page)
        assert ic.same((g[0].cpu(), g[1].cpu()), want), n
        qc, qs = ref(qn.permute(0, 2, 1, 3), lens)
        w_ref = torch.from_numpy((wn.numpy() * qs.permute(0, 2, 1).numpy()).astype(np.float32) * np.float32(W_SCALE))
        idx = fa.mla_index_topk_paged(qc.permute(0, 2, 1, 3).contiguous().view(F8).to(DEV), w_ref.to(DEV), want[0].view(F8).to(DEV),
                                      want[1].to(DEV), td, topk, kc.i32(lens), True)
        assert torch.equal(idx, g[3]["indices"]) and (idx >= 0).all(), n
