"""GPU tests of MLA decode (flash_attention_mla_decode, flash_attention_mla_decode_paged) through the Python fronts,
against mla_check.py's float64 reference under kv_cache_check.assert_close (1e-3 + 1e-3 |ref| on O, 2e-4 + 2e-6 |ref| on the LSE).

Capacity 384, pages 16 and 128, B = 3.  Parity over the packed-row shapes of mla_check.SHAPES -- one row, a partial 16-row tile, a full
one, 65 rows with a head across the block seam, two and four row blocks -- with lengths around the 16-key group, the kernel's 32-key
tile, the page and the capacity mixed in one batch and one length below Sq, the mask both ways, 1, 2, 3, 64 and the library's own split
count; custom scales under the score-noise bound.  Probes with a known answer, poison where the call must not read, the bit-for-bit
equalities of the contract, a replayed graph and the fronts' refusals.  mla_check.parity_cases() are the inputs test_mla_abi.py has held
the emulation to half the tolerance on.
"""
import math

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import kv_cache_check as kc  # noqa: E402
import mla_check as mc  # noqa: E402
from abi_decl import BAD_DTYPE, BAD_SCALE, BAD_SHAPE  # noqa: E402
from kv_cache_check import DEV, i32, same_bits  # noqa: E402
from mla_check import B, CAPACITY, D, DL, DR, KT  # noqa: E402

pytestmark = pytest.mark.gpu
bf, f32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("H,Sq", mc.SHAPES)
def test_parity_with_the_float64_reference(H, Sq):
    n = 0
    for h, sq, Q, KV, lens, causal, page in mc.parity_cases():
        if (h, sq) != (H, Sq):
            continue
        refO, refL = mc.reference(Q, KV, lens, causal)
        q, kv_dev = Q.to(DEV), KV.to(DEV)
        table = mc.table_for(B, page, 31 + page) if page else None
        pool = mc.pool_of(KV, table, page).to(DEV) if page else None
        for ns in mc.SPLITS:
            if page:
                O, lse = fa.flash_attention_mla_decode_paged(q, pool, table.to(DEV), i32(lens), is_causal=causal, num_splits=ns,
                                                             out_dtype=f32, return_lse=True)
            else:
                O, lse = fa.flash_attention_mla_decode(q, kv_dev, i32(lens), is_causal=causal, num_splits=ns, out_dtype=f32, return_lse=True)
            kc.assert_close(O, lse, refO, refL, f"H {H} Sq {Sq} lens {lens} causal {causal} page {page} splits {ns}")
            n += 1
    assert n >= 30


def test_the_plan_is_what_the_parity_tests_ran():
    """the library's own split count at capacity 384 is above one for every shape of the parity tests (the combine runs under
    num_splits = 0 too), and the key tile is the one the lengths were chosen around"""
    for H, Sq in mc.SHAPES:
        plan = fa.mla_decode_plan(B, H, Sq, CAPACITY)
        assert plan["kv_block_rows"] == KT and plan["rows_per_block"] == mc.ROWS and plan["num_splits"] == CAPACITY // KT // 2, plan


@pytest.mark.parametrize("name", ["small", "large", "one", "boost3"])
def test_custom_scales(name):
    for case, scale, Q, KV, lens in mc.scale_cases():
        if case != name:
            continue
        for causal, page, ns in ((False, 0, 0), (True, 16, 1), (True, 0, 3), (False, 128, 2)):
            O, lse = mc.attend(Q, KV, lens, page, scale=scale, is_causal=causal, num_splits=ns, out_dtype=f32)
            mc.assert_close_with_score_noise(O, lse, Q, KV, lens, causal, scale, f"scale {name} causal {causal} page {page} splits {ns}")


def test_the_default_scale_is_576_to_the_minus_half():
    Q, KV = mc.data(8, 2, 4800)
    lens = [CAPACITY, 100, 33]
    a = mc.attend(Q, KV, lens, num_splits=2, out_dtype=f32)
    b = mc.attend(Q, KV, lens, num_splits=2, out_dtype=f32, scale=576 ** -0.5)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    O, lse = mc.attend(Q, KV, lens, num_splits=2, out_dtype=f32, scale=mc.sqrt_scale())      # a model's: mscale^2 / sqrt(192)
    mc.assert_close_with_score_noise(O, lse, Q, KV, lens, False, mc.sqrt_scale(), "scale 1 / sqrt(192)")


# ---- probes with a known answer ----
LENS = [1, 47, CAPACITY]


def visible_counts(lens, Sq, causal):
    return torch.stack([kc.visible(mc.clamp(L), Sq, causal).sum(-1) for L in lens]).double()      # [B, Sq]


@pytest.mark.parametrize("page", [0, 16])
def test_zero_queries_give_the_count_and_the_mean(page):
    """Q = 0: every visible key has weight 1 / n_i, LSE = ln n_i, and with the key index in every latent column (exact in bf16 up to 256,
    even above) O is the mean of the visible indices"""
    H, Sq = 5, 3
    Q = torch.zeros(B, H, Sq, D, dtype=bf)
    idx = torch.arange(CAPACITY)
    idx = torch.where(idx < 256, idx, idx // 2 * 2).float()
    KV = idx[None, :, None].expand(B, CAPACITY, D).to(bf).contiguous()
    for causal, ns in ((False, 1), (True, 1), (True, 3), (False, 0)):
        O, lse = mc.attend(Q, KV, LENS, page, is_causal=causal, num_splits=ns, out_dtype=f32)
        n = visible_counts(LENS, Sq, causal)
        assert (kc.lse_ratio(lse.cpu(), n.log()[:, None, :].expand(B, H, Sq)) <= 1).all()
        mean = torch.stack([torch.stack([idx[:mc.clamp(L)].double()[kc.visible(mc.clamp(L), Sq, causal)[i]].mean() for i in range(Sq)])
                            for L in LENS])
        want = mean[:, None, :, None].expand(B, H, Sq, DL)
        assert ((O.double().cpu() - want).abs() <= 1e-3 + 1e-3 * want.abs()).all(), (causal, ns)


def test_zero_latent_columns_give_exactly_zero():
    """latent columns 0, rope columns random: V = 0, so O is exactly 0 whatever the weights, and the LSE is the reference's"""
    Q, KV = mc.data(13, 5, 4900)
    KV[..., :DL] = 0
    for causal, ns, page in ((True, 1, 0), (False, 3, 16), (True, 0, 128)):
        O, lse = mc.attend(Q, KV, LENS, page, is_causal=causal, num_splits=ns, out_dtype=f32)
        assert (O == 0).all()
        _, refL = mc.reference(Q, KV, LENS, causal)
        assert (kc.lse_ratio(lse.cpu(), refL) <= 1).all()


def test_zero_rope_columns_give_the_512_column_reference():
    Q, KV = mc.data(16, 1, 4910)
    KV[..., DL:] = 0
    for causal, ns, page in ((True, 1, 16), (False, 2, 0)):
        O, lse = mc.attend(Q, KV, LENS, page, is_causal=causal, num_splits=ns, out_dtype=f32)
        refO, refL = mc.reference(Q, KV, LENS, causal, score_cols=DL)
        kc.assert_close(O, lse, refO, refL, f"rope columns zero, causal {causal} splits {ns} page {page}")
    Q[..., :DL] = 0        # ... and a query without latent columns then scores 0 everywhere: the count again
    O, lse = mc.attend(Q, KV, LENS, 0, num_splits=1, out_dtype=f32)
    assert (kc.lse_ratio(lse.cpu(), visible_counts(LENS, 1, False).log()[:, None, :].expand(B, 16, 1)) <= 1).all()


@pytest.mark.parametrize("H,Sq", [(16, 1), (13, 5), (128, 1)])
def test_a_column_coded_cache_comes_back_column_by_column(H, Sq):
    """every key's row equal to the pattern ((c % 64) - 32) / 32: whatever the weights (they sum to 1), O[..., c] is that value up to the
    rounding of the weights' hi + lo pair (each weight within 2^-18 of itself: two roundings to 8 bits) and of the fp32 sums and rescales
    of at most 12 tiles and 64 slabs (2^-18 together): within 2^-17 |value|, and exactly 0 where the value is 0 -- any column permutation
    among the waves' quarters or inside the transposed read is an error of 1 / 32 or more"""
    pattern = ((torch.arange(D) % 64) - 32).float() / 32
    pattern[DL:] = torch.linspace(-1, 1, DR)        # (the rope columns take part in the score only)
    KV = pattern[None, None].expand(B, CAPACITY, D).to(bf).contiguous()
    Q = kc.randn((B, H, Sq, D), 4920 + H, bf)
    want = pattern[:DL].double()
    for causal, ns, page in ((False, 1, 0), (True, 3, 16), (False, 0, 128)):
        O, _ = mc.attend(Q, KV, LENS, page, is_causal=causal, num_splits=ns, out_dtype=f32)
        err = (O.double().cpu() - want).abs()
        assert (err <= 2.0 ** -17 * want.abs()).all(), (causal, ns, page, err.max().item())
    # a pattern that tells the 128-column quarters and the 16-column groups apart as well: the column's index, exact in bf16 below 256
    KV2 = (torch.arange(D) % 256).float()[None, None].expand(B, CAPACITY, D).to(bf).contiguous()
    O, _ = mc.attend(Q * 0, KV2, LENS, 0, num_splits=1, out_dtype=f32)
    col = torch.arange(DL).double() % 256
    assert ((O.double().cpu() - col).abs() <= 8 * 2.0 ** -23 * col.clamp(min=1)).all()
    KV3 = (torch.arange(D) // 256).float()[None, None].expand(B, CAPACITY, D).to(bf).contiguous()
    O, _ = mc.attend(Q * 0, KV3, LENS, 0, num_splits=1, out_dtype=f32)
    assert ((O.double().cpu() - (torch.arange(DL) // 256).double()).abs() <= 1e-6).all()


# ---- poison: what the call must never read ----
POISON_LENS = [1, 33, 200]


def poisoned(KV, lens):
    out = KV.clone()
    for b, L in enumerate(lens):
        out[b, L::2] = float("nan")
        out[b, L + 1::2] = float("inf")
    return out


@pytest.mark.parametrize("H,Sq", [(5, 3), (128, 1)])
def test_poison_beyond_the_lengths_and_in_unused_pages(H, Sq):
    Q, KV = mc.data(H, Sq, 5000 + H)
    dirty = poisoned(KV, POISON_LENS)
    assert not torch.isfinite(dirty.float()).all()
    for causal, ns in ((True, 1), (False, 3), (True, 0)):
        kw = dict(is_causal=causal, num_splits=ns, out_dtype=f32)
        clean = mc.attend(Q, KV, POISON_LENS, 0, **kw)
        got = mc.attend(Q, dirty, POISON_LENS, 0, **kw)
        assert same_bits(got[0], clean[0]) and same_bits(got[1], clean[1]), ("contiguous", causal, ns)
        for page in mc.PAGES:
            table = mc.table_for(B, page, 51 + page)
            pool = mc.pool_of(dirty, table, page)
            used = set(table.reshape(-1).tolist())
            for pg in set(range(pool.shape[0])) - used:                       # the spare pages
                pool[pg] = float("nan")
            # table entries of pages no visible key lies in: -1, 2^31 - 1, numPages
            bad = table.clone()
            junk = [-1, 2 ** 31 - 1, pool.shape[0]]
            for b, L in enumerate(POISON_LENS):
                for j in range(-(-L // page), bad.shape[1]):
                    bad[b, j] = junk[(b + j) % 3]
            assert (bad != table).any()
            got = mc.attend(Q, None, POISON_LENS, page, table=bad, pool=pool, **kw)
            assert same_bits(got[0], clean[0]) and same_bits(got[1], clean[1]), (page, causal, ns)


# ---- bit-for-bit equalities ----
@pytest.mark.parametrize("H,Sq", [(13, 5), (128, 1)])
def test_bit_for_bit_equalities(H, Sq):
    Q, KV = mc.data(H, Sq, 5100 + H)
    lens = [KT + 1, CAPACITY, 4]
    for causal, ns in ((True, 1), (False, 2), (True, 64), (False, 0)):
        kw = dict(is_causal=causal, num_splits=ns)
        O, lse = mc.attend(Q, KV, lens, 0, out_dtype=f32, **kw)
        again = mc.attend(Q, KV, lens, 0, out_dtype=f32, **kw)
        assert same_bits(O, again[0]) and same_bits(lse, again[1]), "two runs"
        for page in mc.PAGES:                                                 # paged = contiguous on the gathered copy
            table = mc.table_for(B, page, 61 + page)
            pool = mc.pool_of(KV, table, page)
            assert same_bits(mc.gathered(pool, table), KV)
            got = mc.attend(Q, None, lens, page, table=table, pool=pool, out_dtype=f32, **kw)
            assert same_bits(got[0], O) and same_bits(got[1], lse), (page, causal, ns)
        for dt in (bf, torch.float16):                                        # BF16 / F16 = F32 rounded once
            got = mc.attend(Q, KV, lens, 0, out_dtype=dt, **kw)
            assert got[0].dtype == dt and same_bits(got[0], O.to(dt)) and same_bits(got[1], lse), (dt, causal, ns)
        alone = mc.attend(Q, KV, lens, 0, out_dtype=f32, return_lse=False, **kw)   # the LSE asked for or not
        assert same_bits(alone, O)
    # strided views: Q and O as [B, Sq, H, *] buffers, the cache as a row slice of a wider one
    wide = torch.zeros(B, CAPACITY, D + 64, dtype=bf)
    wide[..., :D] = KV
    q = Q.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    out = torch.empty(B, Sq, H, DL, dtype=f32, device=DEV).transpose(1, 2)
    got = fa.flash_attention_mla_decode(q, wide.to(DEV)[..., :D], i32(lens), is_causal=True, num_splits=1, O=out, return_lse=True)
    want = mc.attend(Q, KV, lens, 0, out_dtype=f32, is_causal=True, num_splits=1)
    assert got[0].data_ptr() == out.data_ptr() and same_bits(got[0], want[0]) and same_bits(got[1], want[1])


# ---- a decode step as one captured graph ----
def test_a_replayed_graph_sees_the_lengths_and_the_cache_of_the_moment():
    """kv_lens += 1; a torch write of the new cache row; mla_decode -- one captured single-stream graph, replayed after the lengths
    changed on the device: every replay equals the eager step on the same state, bit for bit, and the reference"""
    H, Sq = 16, 1
    Q, KV = mc.data(H, Sq, 5200)
    q, row = Q.to(DEV), kc.randn((B, D), 5201, bf).to(DEV)
    plan = fa.mla_decode_plan(B, H, Sq, CAPACITY)
    ws = torch.empty(fa.decode_workspace_size(B, H, Sq, DL, plan["num_splits"]), dtype=torch.uint8, device=DEV)
    assert plan["num_splits"] > 1 and ws.numel() > 0
    batch = torch.arange(B, device=DEV)

    def step(kv, lens, O):
        lens.add_(1)
        kv[batch, (lens - 1).long()] = row
        return fa.flash_attention_mla_decode(q, kv, lens, is_causal=True, O=O, workspace=ws, return_lse=True)

    kv, lens, O = KV.to(DEV), i32([1] * B), torch.empty(B, H, Sq, DL, dtype=f32, device=DEV)
    step(kv, lens, O)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse = step(kv, lens, O)
    seen = []
    for r, start in enumerate(([KT - 2, 100, 2 * KT - 1], [CAPACITY - 1, 1, 15], [KT, 16, 200])):
        kv.copy_(KV.to(DEV))
        lens.copy_(i32(start))
        graph.replay()
        torch.cuda.synchronize()
        now = lens.tolist()
        assert now == [L + 1 for L in start]
        got = O.clone(), lse.clone()
        ekv, elens, eO = KV.to(DEV), i32(start), torch.empty_like(O)
        _, eager_lse = step(ekv, elens, eO)
        torch.cuda.synchronize()
        assert same_bits(kv, ekv) and same_bits(got[0], eO) and same_bits(got[1], eager_lse), f"replay {r}"
        refO, refL = mc.reference(Q, kv.cpu(), now, True)
        kc.assert_close(got[0], got[1], refO, refL, f"replay {r}")
        seen.append(got[0])
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- the fronts' refusals that need a device ----
def test_front_refusals():
    q = torch.zeros(2, 8, 3, D, dtype=bf, device=DEV)
    kv = torch.zeros(2, 64, D, dtype=bf, device=DEV)
    pool = torch.zeros(9, 16, D, dtype=bf, device=DEV)
    table = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_mla_decode(q.cpu(), kv)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_mla_decode_paged(q, pool, table.cpu())
    for front, cache in ((lambda Q, C, **kw: fa.flash_attention_mla_decode(Q, C, **kw), kv),
                         (lambda Q, C, **kw: fa.flash_attention_mla_decode_paged(Q, C, table, **kw), pool)):
        with pytest.raises(fa.FlashAttentionError) as e:                      # a dtype the kernel does not take: the library's refusal
            front(q.half(), cache.half())
        assert e.value.code == BAD_DTYPE
        with pytest.raises(fa.FlashAttentionError) as e:
            front(q, cache, scale=0.0)
        assert e.value.code == BAD_SCALE
        with pytest.raises(ValueError, match=r"O must be a device tensor \[B, H, Sq, 512\]"):
            front(q, cache, O=torch.empty_like(q))
        with pytest.raises(ValueError, match="workspace must be a device tensor of at least"):
            front(q, cache, num_splits=2, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="kv_lens must be a dense int32 device tensor"):
            front(q, cache, kv_lens=torch.zeros(2, dtype=torch.int32))
        O = front(q, cache, num_splits=1)                                     # zeros in, zeros out: the mean of zero rows
        assert O.dtype == bf and tuple(O.shape) == (2, 8, 3, DL) and (O == 0).all()
    with pytest.raises(fa.FlashAttentionError) as e:                          # page 8
        fa.flash_attention_mla_decode_paged(q, torch.zeros(9, 8, D, dtype=bf, device=DEV), table)
    assert e.value.code == BAD_SHAPE
    assert math.isclose(mc.DEFAULT_SCALE, 1 / 24)
