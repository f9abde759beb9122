"""GPU tests of MLA decode against an fp8 latent cache (flash_attention_mla_decode / _paged with a float8_e4m3fn cache and `kv_descale`;
DESIGN.md section 37), on mla_check's data, reference and cache forms and kv_cache_check's criterion.  The cache is one quantised copy
of mla_check's bf16 cache, handled as uint8 and viewed as float8_e4m3fn at the call; the reference sees it DEQUANTISED, so the error of
quantising is never part of a comparison."""
import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
from kv_cache_check import DEV, fa

pytestmark = pytest.mark.gpu
f8 = lambda t: t.view(kc.F8)


def quantised(H, Sq, seed):
    """(Q bf16, the cache as uint8 [B, CAPACITY, 576], its descale fp32 [1] = amax / 448: no power of two)"""
    Q, KV = mc.data(H, Sq, seed)
    b, ds = kc.quantise(KV.float()[:, None])
    assert abs(torch.log2(ds).item() % 1) > 1e-3
    return Q, b[:, 0].contiguous(), ds


def attend(Q, KV8, lens, ds, page=0, table=None, pool=None, **kw):
    """(O, LSE) of the fp8 call; page > 0: the paged front on a pool built here (or `pool` / `table` as given, on the device)"""
    kw.setdefault("return_lse", True)
    ds = torch.as_tensor(ds, dtype=torch.float32).reshape(1).to(DEV)
    if not page:
        return fa.flash_attention_mla_decode(Q.to(DEV), f8(KV8.to(DEV)), kc.i32(lens), kv_descale=ds, **kw)
    table = mc.table_for(Q.shape[0], page, 77) if table is None else table
    pool = mc.pool_of(KV8, table, page) if pool is None else pool
    return fa.flash_attention_mla_decode_paged(Q.to(DEV), f8(pool.to(DEV)), table.to(DEV), kc.i32(lens), kv_descale=ds, **kw)


@pytest.mark.parametrize("page", (0,) + mc.PAGES)
@pytest.mark.parametrize("H,Sq", [(1, 1), (13, 5), (128, 1)])
def test_float64_parity_on_the_dequantised_cache(H, Sq, page):
    Q, KV8, ds = quantised(H, Sq, 5100 + 10 * H + Sq)
    logical = kc.dequantise(KV8[:, None], ds)[:, 0]
    Qd, table = Q.to(DEV), mc.table_for(mc.B, page, 78) if page else None
    cache = (mc.pool_of(KV8, table, page) if page else KV8).to(DEV)
    for lens in mc.lengths(Sq, page):
        for causal in (False, True):
            refO, refL = mc.reference(Q, logical, lens, causal)
            for ns in (1, 3, 0):
                O, lse = attend(Qd, cache, lens, ds, page, table=table, pool=cache, is_causal=causal, num_splits=ns, out_dtype=torch.float32)
                kc.assert_close(O, lse, refO, refL, f"H {H} Sq {Sq} page {page} lens {lens} causal {causal} splits {ns}")


@pytest.mark.parametrize("ds", [1.0, 0.5])
def test_equal_bits_with_the_bf16_call_on_the_dequantised_cache(ds):
    """e4m3fn -> bf16 is exact and a power-of-two descale commutes with every rounding: the fp8 call IS the bf16 call on bytes * descale,
    O and LSE, under 1 and 3 splits; and the paged call is the contiguous one on the gathered copy"""
    H, Sq = 13, 5
    Q, KV8, _ = quantised(H, Sq, 5200)
    as_bf16 = (f8(KV8).float() * ds).to(torch.bfloat16)
    assert torch.equal(as_bf16.double(), kc.dequantise(KV8[:, None], torch.tensor([ds]))[:, 0])
    for lens in ([mc.CAPACITY - 3, mc.CAPACITY, 65], [4, 17, 96]):
        for ns in (1, 3):
            kw = dict(is_causal=True, num_splits=ns, out_dtype=torch.float32)
            O, lse = attend(Q, KV8, lens, ds, **kw)
            refO, refL = mc.attend(Q, as_bf16, lens, **kw)
            assert torch.isfinite(O).all() and kc.same_bits(O, refO) and kc.same_bits(lse, refL), (lens, ns)
            for page in mc.PAGES:
                table = mc.table_for(mc.B, page, 79)
                pool = mc.pool_of(KV8, table, page)
                assert torch.equal(mc.gathered(pool, table), KV8)
                Op, lp = attend(Q, KV8, lens, ds, page, table=table, pool=pool, **kw)
                assert kc.same_bits(Op, O) and kc.same_bits(lp, lse), (lens, ns, page)


@pytest.mark.parametrize("page", (0,) + mc.PAGES)
def test_poison_beyond_the_length_and_in_pages_not_read_never_enters_the_result(page):
    H, Sq, lens = 16, 2, [33, 128, mc.CAPACITY - 1]
    Q, KV8, ds = quantised(H, Sq, 5300)
    junk = KV8.clone()
    for b, L in enumerate(lens):
        junk[b, L:] = torch.tensor([0x7F, 0xFF], dtype=torch.uint8).repeat(mc.D // 2)
    kw = dict(is_causal=True, num_splits=2, out_dtype=torch.float32)
    if not page:
        clean, dirty = attend(Q, KV8, lens, ds, **kw), attend(Q, junk, lens, ds, **kw)
    else:
        table = mc.table_for(mc.B, page, 80)
        pool, bad = mc.pool_of(KV8, table, page), mc.pool_of(junk, table, page)
        used = torch.zeros(pool.shape[0], dtype=torch.bool)
        used[table.long().reshape(-1)] = True
        bad[~used] = 0xFF                                            # the spare pages
        wild = table.clone()
        for b, L in enumerate(lens):                                 # entries of pages that hold no key below the length
            n = -(-L // page)
            wild[b, n:] = torch.tensor([-1, pool.shape[0]] * table.shape[1], dtype=torch.int32)[:table.shape[1] - n]
        assert not torch.equal(wild, table) and (~used).any()
        clean, dirty = attend(Q, KV8, lens, ds, page, table=table, pool=pool, **kw), attend(Q, KV8, lens, ds, page, table=wild, pool=bad, **kw)
    assert torch.isfinite(clean[0]).all() and kc.same_bits(clean[0], dirty[0]) and kc.same_bits(clean[1], dirty[1])


def test_graph_replay_reads_the_descale_of_the_moment():
    H, Sq, lens = 16, 1, [300, 77, mc.CAPACITY]
    Q, KV8, ds = quantised(H, Sq, 5400)
    Qd, KVd, dsd, ld = Q.to(DEV), f8(KV8.to(DEV)), ds.to(DEV), kc.i32(lens)
    ns = 3
    ws = torch.empty(fa.decode_workspace_size(mc.B, H, Sq, mc.DL, ns), dtype=torch.uint8, device=DEV)
    O = torch.zeros((mc.B, H, Sq, mc.DL), dtype=torch.float32, device=DEV)
    call = lambda **kw: fa.flash_attention_mla_decode(Qd, KVd, ld, is_causal=True, num_splits=ns, kv_descale=dsd, **kw)
    call(O=O, workspace=ws)            # (first call outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(O=O, workspace=ws)
    results = []
    for factor in (1.0, 1.75, 0.3):
        dsd.copy_(ds.to(DEV) * factor)
        O.zero_()
        graph.replay()
        torch.cuda.synchronize()
        results.append(O.clone())
        assert torch.equal(O, call(out_dtype=torch.float32)), factor           # the eager call of the moment
        refO, _ = mc.reference(Q, kc.dequantise(KV8[:, None], dsd.cpu())[:, 0], lens, True)
        err = (O.double().cpu() - refO).abs() / (1e-3 + 1e-3 * refO.abs())
        print(f"replay under descale x {factor}: worst O error / tolerance {err.max().item():.3f}")
        assert (err <= 1).all()
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])
