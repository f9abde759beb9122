"""GPU tests of sparse MLA prefill (flash_attention_mla_sparse_prefill / _paged, bf16 and fp8 caches) on
mla_sparse_check's reference, index lists and cache forms: float64 parity on one ragged batch, bit identity with the sparse decode call
token by token, poison in everything no key names and sentinels in the rows no sequence owns, graph replay."""
import pytest
import torch

import kv_cache_check as kc
import mla_check as mc
import mla_sparse_check as sc
from kv_cache_check import DEV, fa

pytestmark, F32 = pytest.mark.gpu, dict(out_dtype=torch.float32)
ROWS = (1, 17, 0, 5)                       # new rows per sequence: a decoding one, a chunk above 16 rows, an idle one, a short one
CU = [0, 1, 18, 18, 23]
USED, TOTAL = CU[-1], CU[-1] + 3           # totalQ is a bound: three rows no sequence owns
LENS = [[31, 33, 200, 64], [32, mc.CAPACITY, 1, 17], [95, 65, 300, 4]]   # around the 32-slot tile; the last one below its row count
FORMS = [(fp8, page) for fp8 in (False, True) for page in (0, 16)]
SEQ = [b for b, n in enumerate(ROWS) for _ in range(n)]           # the sequence of an owned token
ROW = [j for n in ROWS for j in range(n)]                         # ... and its row in it


def batch(H, topk, lens, seed):
    """(Q [TOTAL, H, 576], KV [4, CAPACITY, 576], indices [TOTAL, topk]); token (1, 0) has no key, the unowned rows hold NaN queries"""
    Q = kc.randn((TOTAL, H, mc.D), seed, torch.bfloat16)
    KV = kc.randn((len(ROWS), mc.CAPACITY, mc.D), seed + 1, torch.bfloat16)
    per_seq = sc.index_lists(max(ROWS), topk, lens, seed + 2, batch=len(ROWS))
    idx = torch.zeros(TOTAL, topk, dtype=torch.int32)
    idx[:USED] = torch.stack([per_seq[b, j] for b, j in zip(SEQ, ROW)])
    Q[USED:] = float("nan")
    return Q, KV, idx


def reference(Q, c, idx, lens, causal):
    """float64 (O [USED, H, 512], LSE [H, USED]): mla_sparse_check.reference on each sequence alone, with its own row count"""
    O = torch.zeros(USED, Q.shape[1], mc.DL, dtype=torch.float64)
    lse = torch.zeros(Q.shape[1], USED, dtype=torch.float64)
    for b, n in enumerate(ROWS):
        if n:
            t = slice(CU[b], CU[b + 1])
            o, l = sc.reference(Q[t].transpose(0, 1)[None], c.logical[b:b + 1], idx[t][None], [lens[b]], causal)
            O[t], lse[:, t] = o[0].transpose(0, 1), l[0]
    return O, lse


def prefill(Q, c, idx, lens, cu=CU, stored=None, table=None, pool=None, **kw):
    kw.setdefault("return_lse", True)
    dev = lambda t: (t.view(kc.F8) if c.fp8 else t).to(DEV)
    if c.fp8:
        kw["kv_descale"] = c.ds.reshape(1).to(DEV)
    if not c.page:
        return fa.flash_attention_mla_sparse_prefill(Q.to(DEV), dev(c.stored if stored is None else stored), idx.to(DEV), kc.i32(cu),
                                                     kc.i32(lens), **kw)
    return fa.flash_attention_mla_sparse_prefill_paged(Q.to(DEV), dev(c.pool if pool is None else pool),
                                                       (c.table if table is None else table).to(DEV), idx.to(DEV), kc.i32(cu),
                                                       kc.i32(lens), **kw)


@pytest.mark.parametrize("fp8,page", FORMS)
@pytest.mark.parametrize("H", [1, 65, 128, 129])
def test_float64_parity_on_a_ragged_batch(H, fp8, page):
    """every kind of slot, topk around the tile, both masks; the keyless token is O = 0, LSE = -inf; H = 129 is two head blocks"""
    for k, topk in enumerate((1, 33, 96)):
        lens = LENS[k]
        Q, KV, idx = batch(H, topk, lens, 7000 + 10 * H + topk)
        c = sc.Cache(KV, fp8, page)
        for causal in (False, True):
            refO, refL = reference(Q, c, idx, lens, causal)
            assert (refL[:, CU[1]] == float("-inf")).all()
            O, lse = prefill(Q, c, idx, lens, is_causal=causal, **F32)
            sc.assert_close(O[:USED].transpose(0, 1), lse[:, :USED], refO.transpose(0, 1), refL,
                            f"H {H} fp8 {fp8} page {page} topk {topk} lens {lens} causal {causal}")


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H", [65, 128])
def test_every_token_is_the_sparse_decode_call_on_it_alone_bit_for_bit(H, fp8):
    """B = 1, Sq = 1, one split, not causal, kv_lens = the token's lim: pins the row packing, the lane map and the column ownership"""
    topk, lens = 96, LENS[0]
    Q, KV, idx = batch(H, topk, lens, 7100 + H)
    c = sc.Cache(KV, fp8, 0)
    O, lse = prefill(Q, c, idx, lens, is_causal=True, **F32)
    stored = (c.stored.view(kc.F8) if fp8 else c.stored).to(DEV)
    extra = dict(kv_descale=c.ds.reshape(1).to(DEV)) if fp8 else {}
    for t, (b, j) in enumerate(zip(SEQ, ROW)):
        lim = sc.limit(lens[b], ROWS[b], j, True)
        dO, dl = fa.flash_attention_mla_sparse_decode(Q[t][None, :, None].to(DEV), stored[b:b + 1], idx[t][None, None].to(DEV), kc.i32([lim]),
                                                      num_splits=1, return_lse=True, **F32, **extra)
        assert kc.same_bits(O[t], dO[0, :, 0]) and kc.same_bits(lse[:, t], dl[0, :, 0]), (t, b, j)


@pytest.mark.parametrize("fp8,page", FORMS)
def test_poison_never_enters_and_unowned_rows_keep_their_sentinel(fp8, page):
    """NaN / inf in every cache row, spare page and table entry no key names; O beyond cu[B] keeps its sentinel (the LSE its zero)"""
    H, topk, lens = 16, 96, LENS[2]
    Q, KV, idx = batch(H, topk, lens, 7200)
    c = sc.Cache(KV, fp8, page)
    named = torch.zeros(len(ROWS), mc.CAPACITY, dtype=torch.bool)
    for t, (b, j) in enumerate(zip(SEQ, ROW)):
        p = idx[t].long()
        named[b, p[(p >= 0) & (p < sc.limit(lens[b], ROWS[b], j, True))]] = True
    junk = c.stored.clone()
    if fp8:
        junk[~named] = torch.tensor([0x7F, 0xFF], dtype=torch.uint8).repeat(mc.D // 2)
    else:
        junk[~named] = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=torch.bfloat16).repeat(mc.D // 3)
    sentinel = lambda: torch.full((TOTAL, H, mc.DL), 7.0, dtype=torch.float32, device=DEV)
    clean = prefill(Q, c, idx, lens, is_causal=True, O=sentinel())
    if not page:
        dirty = prefill(Q, c, idx, lens, is_causal=True, O=sentinel(), stored=junk)
    else:
        bad = mc.pool_of(junk, c.table, page)
        used = torch.zeros(bad.shape[0], dtype=torch.bool)
        used[c.table.long().reshape(-1)] = True
        bad[~used] = 0xFF if fp8 else float("nan")
        wild = c.table.clone()
        keyless = ~named.reshape(len(ROWS), -1, page).any(-1)
        wild[keyless] = torch.tensor([-1, 2 ** 31 - 1, bad.shape[0]], dtype=torch.int32).repeat(keyless.sum().item())[:keyless.sum().item()]
        assert keyless.any() and (~used).any()
        dirty = prefill(Q, c, idx, lens, is_causal=True, O=sentinel(), table=wild, pool=bad)
        flat = prefill(Q, sc.Cache(KV, fp8, 0), idx, lens, is_causal=True, O=sentinel())
        assert kc.same_bits(clean[0], flat[0]) and kc.same_bits(clean[1], flat[1])
    assert torch.isfinite(clean[0]).all() and kc.same_bits(clean[0], dirty[0]) and kc.same_bits(clean[1], dirty[1])
    assert (dirty[0][USED:] == 7.0).all() and (dirty[1][:, USED:] == 0).all() and (dirty[0][:USED] != 7.0).any()


def test_graph_replay_reads_indices_offsets_and_lengths_of_the_moment():
    H, topk, states = 16, 96, [(CU, LENS[0], 7301), ([0, 5, 5, 20, 23], LENS[1], 7302), ([0, 0, 9, 9, 26], LENS[2], 7303)]
    Q, KV, _ = batch(H, topk, LENS[0], 7300)
    Q[USED:] = Q[:TOTAL - USED]            # (every row is owned in the last state)
    c = sc.Cache(KV, False, 0)
    Qd, KVd = Q.to(DEV), KV.to(DEV)
    cud, ld = kc.i32(CU), kc.i32(LENS[0])
    idxd = torch.zeros(TOTAL, topk, dtype=torch.int32, device=DEV)
    O = torch.zeros((TOTAL, H, mc.DL), dtype=torch.float32, device=DEV)
    call = lambda **kw: fa.flash_attention_mla_sparse_prefill(Qd, KVd, idxd, cud, ld, is_causal=True, **kw)
    call(O=O)                              # (first call outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(O=O)
    results = []
    for cu, lens, seed in states:
        rows = [cu[b + 1] - cu[b] for b in range(len(ROWS))]
        per_seq = sc.index_lists(max(rows), topk, lens, seed, batch=len(ROWS))
        idx = torch.zeros(TOTAL, topk, dtype=torch.int32)
        idx[:cu[-1]] = torch.stack([per_seq[b, j] for b, n in enumerate(rows) for j in range(n)])
        for dst, src in ((cud, kc.i32(cu)), (ld, kc.i32(lens)), (idxd, idx.to(DEV))):
            dst.copy_(src)
        for _ in range(2):                 # (several replays against the eager result)
            O.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            eager = torch.full_like(O, 7.0)
            call(O=eager)
            assert torch.equal(O, eager) and (O[cu[-1]:] == 7.0).all(), cu
        results.append(O.clone())
        for b, n in enumerate(rows):
            if n:
                t = slice(cu[b], cu[b + 1])
                ref = sc.reference(Q[t].transpose(0, 1)[None], c.logical[b:b + 1], idx[t][None], [lens[b]], True)[0][0].transpose(0, 1)
                assert ((O[t].cpu().double() - ref).abs() <= 1e-3 + 1e-3 * ref.abs()).all(), (cu, b)     # (kv_cache_check's bound on O)
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])
