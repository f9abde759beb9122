"""GPU tests of the MLA latent-cache append (mla_cache_append / _paged): WHOLE caches compared, byte for byte, with
an expectation built on the host -- the bits for a bf16 cache, kv_cache_check.quantise's arithmetic (fp32 quotient, clamp, one cast)
under a descale of the test's own for an fp8 one -- and the one-graph decode step against mla_check's reference."""
import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
from kv_cache_check import DEV, fa

pytestmark = pytest.mark.gpu
CAP, B, DS, SENTINEL = mc.CAPACITY, mc.B, 0.37, 0xA5


def new_rows(Sq, seed):
    """(c_kv [B, Sq, 512], k_pe [B, Sq, 64]): strided slices of one bf16 projection [B, Sq, 576 + 32], the special values in both --
    +-448 descale, beyond it, +-0, a NaN, a bf16 subnormal"""
    proj = kc.randn((B, Sq, mc.D + 32), seed, torch.bfloat16)
    special = torch.tensor([448 * DS, -448 * DS, 1000.0, -3e38, 0.0, -0.0, float("nan"), 1e-40, -1e-40], dtype=torch.bfloat16)
    proj[:, 0, 3:3 + len(special)] = special
    proj[:, -1, mc.DL + 16 + 5:mc.DL + 16 + 5 + len(special)] = special
    return proj, (lambda t: (t[..., :mc.DL], t[..., mc.DL + 16:mc.DL + 16 + mc.DR]))


def stored(rows, fp8):
    """the bytes of cache rows: bf16 [.., 576] -> uint8 [.., 576 (fp8) or 1152]"""
    if not fp8:
        return rows.contiguous().view(torch.uint8)
    return (rows.float() / torch.tensor(DS, dtype=torch.float32)).clamp(-448, 448).to(kc.F8).view(torch.uint8)


def one_nan(b, fp8):
    """fp8: both NaN codes as one (which of 0x7F / 0xFF a NaN stores is not specified)"""
    return torch.where((b & 0x7F) == 0x7F, torch.full_like(b, 0x7F), b) if fp8 else b


def expected(cache, c, r, lens, fp8, table=None, page=0, skip=()):
    """`cache` (uint8: [B, CAP, bytes] or the pool [P, page, bytes]) after the append; skip: (b, table column) pairs whose rows are dropped"""
    out, new, Sq = cache.clone(), stored(torch.cat([c, r], -1), fp8), c.shape[1]
    for b, L in enumerate(lens):
        L = min(L, CAP)
        for i in range(max(Sq - L, 0), Sq if L > 0 else 0):
            p = L - Sq + i
            if table is None:
                out[b, p] = new[b, i]
            elif (b, p // page) not in skip:
                out[table[b, p // page], p % page] = new[b, i]
    return out


def append(cache, c, r, lens, fp8, table=None):
    """the front on device copies; returns the cache's bytes on the host"""
    dev = cache.to(DEV)
    view = dev.view(kc.F8) if fp8 else dev.view(torch.bfloat16)
    ds = torch.tensor([DS], device=DEV) if fp8 else None
    if table is None:
        fa.mla_cache_append(c, r, view, kc.i32(lens), kv_descale=ds)
    else:
        fa.mla_cache_append_paged(c, r, view, table.to(DEV), kc.i32(lens), kv_descale=ds)
    torch.cuda.synchronize()
    return dev.cpu()


@pytest.mark.parametrize("Sq", [1, 5, 16, 70])           # 70: across a 64-position block and the 16-position waves, from an unaligned start
@pytest.mark.parametrize("page", (0,) + mc.PAGES)
@pytest.mark.parametrize("fp8", [False, True])
def test_every_byte_of_the_cache_after_the_append(fp8, page, Sq):
    proj, parts = new_rows(Sq, 6000 + Sq)
    c, r = parts(proj)
    cd, rd = parts(proj.to(DEV))
    assert not cd.is_contiguous() and not rd.is_contiguous()
    width = mc.D * (1 if fp8 else 2)
    pg = page or 128
    for lens in ([0, max(Sq - 1, 1), CAP + 5], [pg - 1, pg, pg + 1], [-3, CAP, 2 * pg + 7]):
        if page:
            table = mc.table_for(B, page, 81 + Sq)
            cache = torch.full((B * (CAP // page) + 5, page, width), SENTINEL, dtype=torch.uint8)
        else:
            table, cache = None, torch.full((B, CAP, width), SENTINEL, dtype=torch.uint8)
        got, want = append(cache, cd, rd, lens, fp8, table), expected(cache, c, r, lens, fp8, table, page)
        assert not torch.equal(want, cache) and torch.equal(one_nan(got, fp8), one_nan(want, fp8)), (lens, int((got != want).sum()))
        if fp8:      # a NaN went in as a NaN code, and only there
            assert torch.equal((got & 0x7F) == 0x7F, (want & 0x7F) == 0x7F) and ((got & 0x7F) == 0x7F).any()


@pytest.mark.parametrize("fp8", [False, True])
def test_a_table_entry_outside_the_pool_skips_its_rows_and_nothing_else(fp8):
    page, Sq, lens = 16, 40, [100, 100, 100]               # positions 60 .. 99: pages 3 .. 6 of every sequence
    proj, parts = new_rows(Sq, 6100)
    c, r = parts(proj)
    table = mc.table_for(B, page, 82)
    P = B * (CAP // page) + 5
    wild = table.clone()
    wild[0, 4], wild[1, 5] = -1, P
    cache = torch.full((P, page, mc.D * (1 if fp8 else 2)), SENTINEL, dtype=torch.uint8)
    got = append(cache, *parts(proj.to(DEV)), lens, fp8, wild)
    want = expected(cache, c, r, lens, fp8, table, page, skip={(0, 4), (1, 5)})
    assert torch.equal(one_nan(got, fp8), one_nan(want, fp8))
    assert (got[table[0, 4]] == SENTINEL).all() and (got[table[1, 5]] == SENTINEL).all() and (got[table[2, 4]] != SENTINEL).any()


def test_one_graph_decode_step_on_an_fp8_paged_cache():
    """kv_lens += 1; mla_cache_append_paged; flash_attention_mla_decode_paged: captured once, replayed twice, equal to the eager steps bit
    for bit (O and every byte of the pool) and to the float64 reference on the dequantised cache"""
    H, page, ns, start = 16, 16, 2, [30, 15, 100]
    Q, KV = mc.data(H, 1, 6200)
    b8, ds = kc.quantise(KV.float()[:, None])
    table = mc.table_for(B, page, 83)
    pool = mc.pool_of(b8[:, 0], table, page)
    proj, parts = new_rows(1, 6201)
    proj[:] = kc.randn(proj.shape, 6202, torch.bfloat16)   # (plain rows: the reference must stay finite)
    cd, rd = parts(proj.to(DEV))
    Qd, td, dsd = Q.to(DEV), table.to(DEV), ds.to(DEV)
    ws = torch.empty(fa.decode_workspace_size(B, H, 1, mc.DL, ns), dtype=torch.uint8, device=DEV)

    def step(pool_d, lens_d, O):
        lens_d += 1
        fa.mla_cache_append_paged(cd, rd, pool_d.view(kc.F8), td, lens_d, kv_descale=dsd)
        fa.flash_attention_mla_decode_paged(Qd, pool_d.view(kc.F8), td, lens_d, is_causal=True, num_splits=ns, kv_descale=dsd, O=O, workspace=ws)

    state = lambda: (pool.to(DEV), kc.i32(start), torch.zeros((B, H, 1, mc.DL), dtype=torch.float32, device=DEV))
    step(*state())                                         # (first calls outside the capture, on a state of their own)
    torch.cuda.synchronize()
    (pool_g, lens_g, O_g), (pool_e, lens_e, O_e) = state(), state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(pool_g, lens_g, O_g)
    for n in (1, 2):
        graph.replay()
        step(pool_e, lens_e, O_e)
        torch.cuda.synchronize()
        lens = [L + n for L in start]
        assert lens_g.tolist() == lens_e.tolist() == lens and torch.equal(pool_g, pool_e) and kc.same_bits(O_g, O_e), n
        assert not torch.equal(pool_g.cpu(), pool)
        logical = kc.dequantise(mc.gathered(pool_g.cpu(), table)[:, None], ds)[:, 0]
        refO, _ = mc.reference(Q, logical, lens, True)
        err = (O_g.double().cpu() - refO).abs() / (1e-3 + 1e-3 * refO.abs())
        print(f"step {n}: worst O error / tolerance {err.max().item():.3f}")
        assert (err <= 1).all()
