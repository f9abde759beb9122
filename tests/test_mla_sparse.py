"""GPU tests of sparse MLA decode (flash_attention_mla_sparse_decode / _paged, bf16 and fp8 caches) on
mla_sparse_check's reference, index lists and cache forms: float64 parity, bit identity with the dense call on the identity list,
poison in everything no key names, equal bits across forms, a pool above 2^32 bytes, graph replay."""
import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
import mla_sparse_check as sc
from kv_cache_check import DEV, fa

pytestmark = pytest.mark.gpu
F32 = dict(out_dtype=torch.float32)


@pytest.mark.parametrize("fp8,page", sc.FORMS)
@pytest.mark.parametrize("H,Sq", [(1, 1), (16, 1), (65, 3), (128, 2)])
def test_float64_parity(H, Sq, fp8, page):
    """every kind of slot in one batch (mla_sparse_check.index_lists), topk around the tile, every split count, both masks; the row
    without a key is O = 0, LSE = -inf under every split count"""
    Q, KV = mc.data(H, Sq, 6000 + 10 * H + Sq)
    c = sc.Cache(KV, fp8, page)
    Qd = Q.to(DEV)
    for k, topk in enumerate((1, 31, 32, 33, 96, 200)):
        lens = mc.lengths(Sq, page)[k % 5]
        idx = sc.index_lists(Sq, topk, lens, 6100 + topk)
        for causal in (False, True):
            refO, refL = sc.reference(Q, c.logical, idx, lens, causal)
            assert (refL[1, :, 0] == float("-inf")).all()
            for ns in mc.SPLITS:
                O, lse = sc.attend(Qd, c, idx, lens, is_causal=causal, num_splits=ns, **F32)
                sc.assert_close(O, lse, refO, refL, f"H {H} Sq {Sq} fp8 {fp8} page {page} topk {topk} lens {lens} causal {causal} splits {ns}")


@pytest.mark.parametrize("fp8", [False, True])
def test_the_identity_list_is_the_dense_call_bit_for_bit(fp8):
    """indices = 0 .. capacity - 1 and every length the capacity: the same tiles in the same splits, and the per-tile arithmetic is the
    dense kernel's -- with H = 65, Sq = 3 this also pins the packing of the rows (head blocks per query row, not h * Sq + i)"""
    H, Sq = 65, 3
    Q, KV = mc.data(H, Sq, 6200)
    c = sc.Cache(KV, fp8, 0)
    idx = torch.arange(mc.CAPACITY, dtype=torch.int32).expand(mc.B, Sq, mc.CAPACITY).contiguous()
    dense_kv = c.stored.view(kc.F8) if fp8 else c.stored
    extra = dict(kv_descale=c.ds.reshape(1).to(DEV)) if fp8 else {}
    for causal in (False, True):
        for ns in (1, 3):
            O, lse = sc.attend(Q, c, idx, None, is_causal=causal, num_splits=ns, **F32)
            dO, dlse = fa.flash_attention_mla_decode(Q.to(DEV), dense_kv.to(DEV), None, is_causal=causal, num_splits=ns, return_lse=True,
                                                     **F32, **extra)
            assert torch.isfinite(O).all() and kc.same_bits(O, dO) and kc.same_bits(lse, dlse), (causal, ns)


@pytest.mark.parametrize("fp8,page", sc.FORMS)
def test_poison_in_every_row_no_key_names_never_enters_the_result(fp8, page):
    """NaN / inf (fp8: 0x7F / 0xFF) in every cache row no valid slot names -- rows at and beyond the length that slots DO name among
    them -- and in the spare pages; wild table entries for the pages no key lies in"""
    H, Sq, topk, lens = 16, 3, 96, [33, 130, mc.CAPACITY - 1]
    Q, KV = mc.data(H, Sq, 6300)
    c = sc.Cache(KV, fp8, page)
    idx = sc.index_lists(Sq, topk, lens, 6301)
    named = torch.zeros(mc.B, mc.CAPACITY, dtype=torch.bool)
    for b in range(mc.B):
        for i in range(Sq):
            p = idx[b, i].long()
            named[b, p[(p >= 0) & (p < sc.limit(lens[b], Sq, i, True))]] = True
    assert (idx[0] == mc.clamp(lens[0])).any() and not named[0, lens[0]:].any()
    junk = c.stored.clone()
    if fp8:
        junk[~named] = torch.tensor([0x7F, 0xFF], dtype=torch.uint8).repeat(mc.D // 2)
    else:
        junk[~named] = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=torch.bfloat16).repeat(mc.D // 3)
    kw = dict(is_causal=True, num_splits=2, **F32)
    clean = sc.attend(Q, c, idx, lens, **kw)
    if not page:
        dirty = sc.attend(Q, c, idx, lens, stored=junk, **kw)
    else:
        bad = mc.pool_of(junk, c.table, page)
        used = torch.zeros(bad.shape[0], dtype=torch.bool)
        used[c.table.long().reshape(-1)] = True
        bad[~used] = 0xFF if fp8 else float("nan")
        wild = c.table.clone()
        keyless = ~named.reshape(mc.B, -1, page).any(-1)
        wild[keyless] = torch.tensor([-1, 2 ** 31 - 1, bad.shape[0]], dtype=torch.int32).repeat(keyless.sum().item())[:keyless.sum().item()]
        assert keyless.any() and (~used).any()
        dirty = sc.attend(Q, c, idx, lens, table=wild, pool=bad, **kw)
    assert torch.isfinite(clean[0]).all() and kc.same_bits(clean[0], dirty[0]) and kc.same_bits(clean[1], dirty[1])


@pytest.mark.parametrize("fp8", [False, True])
def test_equal_bits_across_forms(fp8):
    """paged is contiguous on the gathered copy; a BF16 / F16 O is the F32 one rounded once; with the LSE or without; run to run"""
    H, Sq, topk, lens = 65, 2, 200, [mc.CAPACITY, 100, 47]
    Q, KV = mc.data(H, Sq, 6400)
    idx = sc.index_lists(Sq, topk, lens, 6401)
    c = sc.Cache(KV, fp8, 0)
    for ns in (1, 3):
        kw = dict(is_causal=True, num_splits=ns)
        O, lse = sc.attend(Q, c, idx, lens, **kw, **F32)
        assert kc.same_bits(O, sc.attend(Q, c, idx, lens, **kw, **F32)[0])
        assert kc.same_bits(O, sc.attend(Q, c, idx, lens, return_lse=False, **kw, **F32))
        for dt in (torch.bfloat16, torch.float16):
            assert kc.same_bits(O.to(dt), sc.attend(Q, c, idx, lens, out_dtype=dt, **kw)[0]), (ns, dt)
        for page in mc.PAGES:
            cp = sc.Cache(KV, fp8, page, seed=79)
            assert torch.equal(mc.gathered(cp.pool, cp.table), c.stored)
            Op, lp = sc.attend(Q, cp, idx, lens, **kw, **F32)
            assert kc.same_bits(Op, O) and kc.same_bits(lp, lse), (ns, page)


def test_a_pool_above_4_gib_with_the_named_pages_at_its_far_end():
    """the row addresses are 64-bit: a bf16 pool of more than 2^32 bytes, allocated and not filled but for the sequences' pages, which
    are its last ones, against the same rows in a small pool"""
    H, Sq, topk, page, lens = 16, 1, 96, 128, [mc.CAPACITY, 300, 129]
    Q, KV = mc.data(H, Sq, 6500)
    idx = sc.index_lists(Sq, topk, lens, 6501)
    c = sc.Cache(KV, False, page)
    n = c.table.numel()
    P = 2 ** 32 // (page * mc.D * 2) + n + 1
    big = torch.empty((P, page, mc.D), dtype=torch.bfloat16, device=DEV)
    assert big.numel() * 2 > 2 ** 32 + n * page * mc.D * 2
    far = (P - n + torch.randperm(n, generator=torch.Generator().manual_seed(6502))).to(torch.int32).reshape(c.table.shape)
    big[far.long().reshape(-1)] = c.pool[c.table.long().reshape(-1)].to(DEV)
    for ns in (1, 2):
        kw = dict(is_causal=False, num_splits=ns, **F32)
        O, lse = sc.attend(Q, c, idx, lens, **kw)
        Ob, lb = fa.flash_attention_mla_sparse_decode_paged(Q.to(DEV), big, far.to(DEV), idx.to(DEV), kc.i32(lens), return_lse=True, **kw)
        assert torch.isfinite(O[0]).all() and kc.same_bits(O, Ob) and kc.same_bits(lse, lb), ns


def test_graph_replay_reads_the_indices_and_the_lengths_of_the_moment():
    H, Sq, topk, ns = 16, 2, 96, 3
    Q, KV = mc.data(H, Sq, 6600)
    c = sc.Cache(KV, False, 0)
    states = [([300, 77, mc.CAPACITY], 6601), ([64, 384, 31], 6602), ([200, 200, 200], 6603)]
    Qd, KVd = Q.to(DEV), KV.to(DEV)
    ld, idxd = kc.i32(states[0][0]), sc.index_lists(Sq, topk, *states[0]).to(DEV)
    ws = torch.empty(fa.decode_workspace_size(mc.B, H, Sq, mc.DL, ns), dtype=torch.uint8, device=DEV)
    O = torch.zeros((mc.B, H, Sq, mc.DL), dtype=torch.float32, device=DEV)
    call = lambda **kw: fa.flash_attention_mla_sparse_decode(Qd, KVd, idxd, ld, is_causal=True, num_splits=ns, **kw)
    call(O=O, workspace=ws)            # (first call outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(O=O, workspace=ws)
    results = []
    for lens, seed in states:
        idx = sc.index_lists(Sq, topk, lens, seed)
        ld.copy_(kc.i32(lens))
        idxd.copy_(idx.to(DEV))
        O.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        results.append(O.clone())
        eager, lse = call(return_lse=True, **F32)
        assert torch.equal(O, eager), lens
        sc.assert_close(O, lse, *sc.reference(Q, c.logical, idx, lens, True), f"replay with lens {lens}")
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])
