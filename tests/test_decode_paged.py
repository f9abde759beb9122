"""GPU tests of flash_attention_decode_paged (split-KV decode against K/V pools of fixed-size pages behind a block table): parity
with the float64 explicit softmax over the gathered keys of each sequence (every element of the fp32 output within the stated
1e-3 + 1e-3 |ref|; the LSE within 2e-4 + 2e-6 |ref|), the same bits as flash_attention_decode on a gathered contiguous copy, poison
in the rows beyond the length and in the pages not used, out-of-range table entries, shared prefixes, strided pools and tables, graph
replay with a table that changes in place, and a pool above 2^32 bytes.

The tests are ordered so that a kernel that ignores the lengths meets NaN (a valid page full of it) before it meets a bad index."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from kv_cache_check import CAP, DEV, assert_close, gather, max_pages_of, paged_layout, randn, reference  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
PAGES = [16, 32, 128, 256]
NAN = float("nan")


@functools.lru_cache(maxsize=2)
def paged_case(page, d, Hkv=2):
    """CPU pools with more pages than any sequence uses, a random permutation as the table, one sequence per boundary length"""
    P, table, lens = paged_layout(page, d)
    Kp, Vp = randn((P, Hkv, page, d), 1000 + page + d, BF16), randn((P, Hkv, page, d), 2000 + page + d, BF16)
    return Kp, Vp, table, lens


@functools.lru_cache(maxsize=2)
def device_case(page, d):
    Kp, Vp, table, lens = paged_case(page, d)
    return Kp.to(DEV), Vp.to(DEV), table.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


# ---- 1. parity sweep ----
@pytest.mark.parametrize("Sq,G", [(1, 1), (1, 4), (5, 8), (16, 16), (2, 2)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", PAGES)
def test_sweep_against_float64(page, d, Sq, G):
    Kp, Vp, table, lens = paged_case(page, d)
    Kd, Vd, td, ld = device_case(page, d)
    B, Hkv = len(lens), Kp.shape[1]
    H = G * Hkv
    Q = randn((B, H, Sq, d), 4000 + Sq + G, BF16)
    Kg, Vg = gather(Kp, table), gather(Vp, table)
    Qd = Q.to(DEV)
    for causal in (False, True):
        refO, refL = reference(Q, Kg, Vg, lens, causal)
        for splits in (0, 1, 2, 3, CAP):
            O, lse = fa.flash_attention_decode_paged(Qd, Kd, Vd, td, ld, is_causal=causal, out_dtype=torch.float32, num_splits=splits,
                                                     return_lse=True)
            torch.cuda.synchronize()
            assert_close(O, lse, refO, refL, f"page {page} d {d} Sq {Sq} G {G} causal {causal} splits {splits} lens {lens}")
            # bf16 / fp16 output: the fp32 result of the same call rounded once
            for dt in (torch.bfloat16, torch.float16):
                Ol = fa.flash_attention_decode_paged(Qd, Kd, Vd, td, ld, is_causal=causal, out_dtype=dt, num_splits=splits)
                assert Ol.dtype == dt and torch.equal(Ol, O.to(dt)), dt
    # kv_lens = None: the capacity
    refO, refL = reference(Q, Kg, Vg, None, True)
    O, lse = fa.flash_attention_decode_paged(Qd, Kd, Vd, td, None, is_causal=True, out_dtype=torch.float32, return_lse=True)
    torch.cuda.synchronize()
    assert_close(O, lse, refO, refL, f"page {page} d {d} Sq {Sq} G {G} no lengths")


# ---- 2. the same bits as the contiguous path ----
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", PAGES)
def test_bitwise_equal_to_the_contiguous_path_on_a_gathered_copy(page, d):
    Kd, Vd, td, ld = device_case(page, d)
    B, Hkv = td.shape[0], Kd.shape[1]
    Kg, Vg = gather(Kd, td), gather(Vd, td)
    for Sq, G in ((1, 4), (5, 8)):
        Q = randn((B, G * Hkv, Sq, d), 5000 + Sq, BF16).to(DEV)
        for causal in (False, True):
            for splits in (0, 1, 2, 3, CAP):
                kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True)
                O, lse = fa.flash_attention_decode_paged(Q, Kd, Vd, td, ld, **kw)
                Oc, lsec = fa.flash_attention_decode(Q, Kg, Vg, ld, **kw)
                torch.cuda.synchronize()
                assert torch.equal(O, Oc) and torch.equal(lse, lsec), (Sq, G, causal, splits)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", PAGES)
def test_identity_table_over_a_contiguous_cache_viewed_as_pages(page, d):
    Hkv, G, Sq, n = 3, 4, 2, max_pages_of(page) + 2
    cap = n * page
    K, V = randn((1, Hkv, cap, d), 51, BF16).to(DEV), randn((1, Hkv, cap, d), 52, BF16).to(DEV)
    Q = randn((1, G * Hkv, Sq, d), 53, BF16).to(DEV)
    pool = lambda t: t[0].view(Hkv, n, page, d).transpose(0, 1)      # [n, Hkv, page, d]: no copy
    assert pool(K).data_ptr() == K.data_ptr() and not pool(K).is_contiguous()
    table = torch.arange(n, dtype=torch.int32, device=DEV)[None]
    for L in (cap, cap - page - 5, 1):
        ld = torch.tensor([L], dtype=torch.int32, device=DEV)
        for splits in (0, 2):
            kw = dict(is_causal=True, out_dtype=torch.float32, num_splits=splits, return_lse=True)
            O, lse = fa.flash_attention_decode_paged(Q, pool(K), pool(V), table, ld, **kw)
            Oc, lsec = fa.flash_attention_decode(Q, K, V, ld, **kw)
            torch.cuda.synchronize()
            assert torch.equal(O, Oc) and torch.equal(lse, lsec), (L, splits)


# ---- 3. and 4.: poison, then out-of-range entries ----
POISON_SPLITS = (0, 1, 3, CAP)


@functools.lru_cache(maxsize=2)
def poison_case(page, d):
    """Pools whose pages 0 and P - 1 are NaN; the tables name neither.  Returns the device tensors (rows beyond each length and the
    unused table entries still clean: zero rows, entries naming a zero page) and the clean results per (causal, splits)"""
    Hkv, G, Sq, n = 2, 4, 3, max_pages_of(page)
    cap = n * page
    lens = [1, page + 1, cap - page - 3, cap - 3]      # a last page half full; whole pages unused behind it
    B = len(lens)
    P = B * n + 3
    Kp, Vp = randn((P, Hkv, page, d), 61 + page, BF16), randn((P, Hkv, page, d), 62 + page, BF16)
    zero_page = P - 2
    Kp[zero_page], Vp[zero_page] = 0, 0
    g = torch.Generator().manual_seed(63 + page)
    table = (1 + torch.randperm(B * n, generator=g)).reshape(B, n).to(torch.int32)     # pages 1 .. B n
    used = [-(-L // page) for L in lens]
    for b, L in enumerate(lens):
        last = int(table[b, used[b] - 1])
        Kp[last, :, L - (used[b] - 1) * page:], Vp[last, :, L - (used[b] - 1) * page:] = 0, 0
        table[b, used[b]:] = zero_page
    Kp[0], Vp[0], Kp[P - 1], Vp[P - 1] = NAN, NAN, NAN, NAN
    Q = randn((B, G * Hkv, Sq, d), 64, BF16).to(DEV)
    Kd, Vd, td, ld = Kp.to(DEV), Vp.to(DEV), table.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    clean = {}
    for causal in (False, True):
        for splits in POISON_SPLITS:
            clean[causal, splits] = fa.flash_attention_decode_paged(Q, Kd, Vd, td, ld, is_causal=causal, out_dtype=torch.float32,
                                                                    num_splits=splits, return_lse=True)
    torch.cuda.synchronize()
    refO, refL = reference(Q.cpu(), gather(Kp, table), gather(Vp, table), lens, True)
    assert_close(*clean[True, 0], refO, refL, f"poison case, clean, page {page} d {d}")
    return Q, Kd, Vd, td, ld, lens, used, clean


def dirty_pools(page, d):
    """the pools of poison_case with NaN / 1e30 in the rows at and beyond each length of the last used page"""
    Q, Kd, Vd, td, ld, lens, used, clean = poison_case(page, d)
    Kg, Vg = Kd.clone(), Vd.clone()
    for b, L in enumerate(lens):
        last, r = int(td[b, used[b] - 1]), L - (used[b] - 1) * page
        Kg[last, :, r::2], Kg[last, :, r + 1::2] = NAN, 1e30
        Vg[last, :, r::2], Vg[last, :, r + 1::2] = 1e30, NAN
    return Kg, Vg


def assert_same_bits_as_clean(page, d, Kg, Vg, table):
    Q, Kd, Vd, td, ld, lens, used, clean = poison_case(page, d)
    for causal in (False, True):
        for splits in POISON_SPLITS:
            O, lse = fa.flash_attention_decode_paged(Q, Kg, Vg, table, ld, is_causal=causal, out_dtype=torch.float32, num_splits=splits,
                                                     return_lse=True)
            torch.cuda.synchronize()
            assert torch.isfinite(O).all() and torch.isfinite(lse).all(), (causal, splits)
            assert torch.equal(O, clean[causal, splits][0]) and torch.equal(lse, clean[causal, splits][1]), (causal, splits)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", PAGES)
def test_poison_beyond_the_length_and_in_unused_pages_never_enters_the_result(page, d):
    Q, Kd, Vd, td, ld, lens, used, clean = poison_case(page, d)
    Kg, Vg = dirty_pools(page, d)
    table = td.clone()
    for b in range(len(lens)):
        table[b, used[b]:] = 0 if b % 2 else Kd.shape[0] - 1      # valid pages, full of NaN
    assert_same_bits_as_clean(page, d, Kg, Vg, table)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", PAGES)
def test_out_of_range_unused_entries_are_never_followed(page, d):
    Q, Kd, Vd, td, ld, lens, used, clean = poison_case(page, d)
    Kg, Vg = dirty_pools(page, d)
    table = td.clone()
    bad = [-1, 2 ** 31 - 1, Kd.shape[0]]
    for b in range(len(lens)):
        for j in range(used[b], table.shape[1]):
            table[b, j] = bad[(b + j) % 3]
    assert int((table < 0).sum()) and int((table >= Kd.shape[0]).sum())
    assert_same_bits_as_clean(page, d, Kg, Vg, table)


# ---- 5. shared prefix ----
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [16, 128])
def test_sequences_that_share_their_first_pages(page, d):
    Hkv, G, Sq, n, shared = 2, 4, 2, max_pages_of(page) + 1, 2
    P = 3 * n
    Kp, Vp = randn((P, Hkv, page, d), 71, BF16), randn((P, Hkv, page, d), 72, BF16)
    table = torch.stack([torch.arange(n), torch.arange(n) + n, torch.arange(n) + 2 * n]).to(torch.int32)
    table[1, :shared] = table[0, :shared]
    table[2, :shared + 1] = table[0, :shared + 1]
    lens = [n * page - 1, shared * page + 3, shared * page]       # the third sequence is its shared prefix and nothing else
    Q = randn((3, G * Hkv, Sq, d), 73, BF16)
    refO, refL = reference(Q, gather(Kp, table), gather(Vp, table), lens, True)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for splits in (0, 3):
        O, lse = fa.flash_attention_decode_paged(Q.to(DEV), Kp.to(DEV), Vp.to(DEV), table.to(DEV), ld, is_causal=True,
                                                 out_dtype=torch.float32, num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close(O, lse, refO, refL, f"shared prefix, page {page} d {d} splits {splits}")


# ---- 6. strided pool and table ----
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [16, 256])
def test_page_major_pool_view_and_a_row_slice_of_a_wider_table(page, d):
    Hkv, G, Sq, n = 2, 4, 3, max_pages_of(page)
    B, P = 3, 3 * max_pages_of(page) + 5
    kp, vp = randn((P, page, Hkv, d), 81, BF16).to(DEV), randn((P, page, Hkv, d), 82, BF16).to(DEV)      # [P, page, Hkv, d] storage
    Kp, Vp = kp.transpose(1, 2), vp.transpose(1, 2)
    assert not Kp.is_contiguous() and Kp.shape == (P, Hkv, page, d)
    g = torch.Generator().manual_seed(83)
    wide = torch.full((B, n + 6), -7, dtype=torch.int32)
    wide[:, 2:2 + n] = torch.randperm(P, generator=g)[:B * n].reshape(B, n).to(torch.int32)
    wide = wide.to(DEV)
    table = wide[:, 2:2 + n]
    assert table.stride(0) == n + 6 and not table.is_contiguous()
    lens = [n * page, page + 1, n * page - page + 2]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    Q = randn((B, G * Hkv, Sq, d), 84, BF16).to(DEV)
    O, lse = fa.flash_attention_decode_paged(Q, Kp, Vp, table, ld, is_causal=True, out_dtype=torch.float32, return_lse=True)
    Od, lsed = fa.flash_attention_decode_paged(Q, Kp.contiguous(), Vp.contiguous(), table.contiguous(), ld, is_causal=True,
                                               out_dtype=torch.float32, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(O, Od) and torch.equal(lse, lsed)
    refO, refL = reference(Q.cpu(), gather(Kp.cpu(), table.cpu()), gather(Vp.cpu(), table.cpu()), lens, True)
    assert_close(O, lse, refO, refL, f"strided pool and table, page {page} d {d}")


# ---- 7. graph capture, a side stream, determinism ----
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [16, 128])
def test_graph_replay_reads_the_table_and_the_lengths_of_the_moment(page, d):
    """one captured call (a linear chain: split kernel, combine kernel); a sequence then grows across a page boundary: the new
    page's entry is written into the table in place, the length advanced in place"""
    B, H, Hkv, Sq, n = 2, 8, 2, 1, 4096 // page
    P = B * n + 4
    Kp, Vp = randn((P, Hkv, page, d), 91, BF16).to(DEV), randn((P, Hkv, page, d), 92, BF16).to(DEV)
    Q = randn((B, H, Sq, d), 93, BF16).to(DEV)
    lens = [3 * page, 1000]
    table = torch.full((B, n), P - 1, dtype=torch.int32)             # entries not yet in use name a page full of NaN
    g = torch.Generator().manual_seed(94)
    perm = torch.randperm(P - 1, generator=g).to(torch.int32)
    for b, L in enumerate(lens):
        table[b, :-(-L // page)] = perm[b * n:b * n + -(-L // page)]
    Kp[P - 1], Vp[P - 1] = NAN, NAN
    td, ld = table.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    plan = fa.decode_plan(B, H, Hkv, Sq, n * page, d, fa.FA_DTYPE_F32)
    assert plan["num_splits"] > 1
    ws = torch.empty(fa.decode_workspace_size(B, H, Sq, d, plan["num_splits"]), dtype=torch.uint8, device=DEV)
    O = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
    eager = lambda: fa.flash_attention_decode_paged(Q, Kp, Vp, td, ld, is_causal=True, out_dtype=torch.float32).clone()
    fa.flash_attention_decode_paged(Q, Kp, Vp, td, ld, is_causal=True, O=O, workspace=ws)   # (first call outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.flash_attention_decode_paged(Q, Kp, Vp, td, ld, is_causal=True, O=O, workspace=ws)
    O.zero_()
    graph.replay()
    torch.cuda.synchronize()
    first = eager()
    assert torch.isfinite(O).all() and torch.equal(O, first) and torch.equal(first, eager())      # (run-to-run determinism)
    # one decode step later: sequence 0 was at a page boundary, so its next key opens a new page
    new_page = int(perm[B * n])
    td[0, 3] = new_page
    ld += 1
    graph.replay()
    torch.cuda.synchronize()
    second = eager()
    assert torch.isfinite(O).all() and torch.equal(O, second) and not torch.equal(first[0], second[0])
    table[0, 3] = new_page
    live = [3 * page + 1, 1001]
    tb = table.clone()
    for b, L in enumerate(live):
        tb[b, -(-L // page):] = 0                                    # (the reference's gather needs entries it can follow)
    refO, _ = reference(Q.cpu(), gather(Kp.cpu(), tb), gather(Vp.cpu(), tb), live, True)
    assert ((O.double().cpu() - refO).abs() <= 1e-3 + 1e-3 * refO.abs()).all()


@pytest.mark.parametrize("d", [64, 128])
def test_on_a_side_stream_keeps_its_workspace(d):
    """stream=: the kernels run on a side stream while the current stream goes on allocating blocks of the workspace's size and
    overwriting them; the workspace released at return must not be one of them while the kernels still use it"""
    B, H, Hkv, Sq, page, n = 4, 32, 8, 4, 128, 64
    P = B * n
    Kp, Vp = randn((P, Hkv, page, d), 95, BF16).to(DEV), randn((P, Hkv, page, d), 96, BF16).to(DEV)
    Q = randn((B, H, Sq, d), 97, BF16).to(DEV)
    td = torch.randperm(P, generator=torch.Generator().manual_seed(98)).reshape(B, n).to(torch.int32).to(DEV)
    ns = fa.decode_plan(B, H, Hkv, Sq, n * page, d, fa.FA_DTYPE_F32)["num_splits"]
    nbytes = fa.decode_workspace_size(B, H, Sq, d, ns)
    assert ns > 1 and nbytes > 0
    ref = fa.flash_attention_decode_paged(Q, Kp, Vp, td, out_dtype=torch.float32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        got = fa.flash_attention_decode_paged(Q, Kp, Vp, td, out_dtype=torch.float32, stream=side)
        junk = [torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV) for _ in range(4)]   # NaN bytes, on the current stream
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
        del junk, got


# ---- 8. a pool above 2^32 bytes ----
@pytest.mark.parametrize("d", [64, 128])
def test_a_pool_above_four_gibibytes(d):
    """Page bases are 64-bit: a sequence whose table names pages on both sides of byte 2^32 of each pool, with its softmax mass on a
    page above it.  The pages that a base wrapped to 32 bits would reach instead hold other data."""
    Hkv, page, G, Sq = 1, 256, 4, 2
    page_bytes = page * d * 2
    wrap = (1 << 32) // page_bytes                 # the page that starts at byte 2^32: 65 536 at d = 128
    P = wrap + 64 * (128 // d)
    assert P >= 65600 and P * page_bytes > (1 << 32)
    Kp = torch.empty((P, Hkv, page, d), dtype=torch.bfloat16, device=DEV)
    Vp = torch.empty((P, Hkv, page, d), dtype=torch.bfloat16, device=DEV)
    pages = [5, wrap + 9, wrap - 1, P - 1, wrap, 17]
    aliases = [p - wrap for p in pages if p >= wrap]               # where a 32-bit page base would land
    assert not set(aliases) & set(pages)
    Q = randn((1, G * Hkv, Sq, d), 101, BF16)
    for j, pg in enumerate(pages + aliases):
        Kp[pg], Vp[pg] = randn((Hkv, page, d), 110 + j, BF16).to(DEV), randn((Hkv, page, d), 130 + j, BF16).to(DEV)
    # the mass: on page P - 1 (the fourth of the sequence) a few keys line up with the queries
    heavy = (Q[0, :, -1].float().mean(0) * 6).to(torch.bfloat16)
    Kp[P - 1, 0, 40:44] = heavy.to(DEV)
    table = torch.tensor([pages], dtype=torch.int32)
    L = 5 * page + 77
    Kg = torch.stack([Kp[pg].cpu() for pg in pages], 1).reshape(1, Hkv, len(pages) * page, d)
    Vg = torch.stack([Vp[pg].cpu() for pg in pages], 1).reshape(1, Hkv, len(pages) * page, d)
    refO, refL = reference(Q, Kg, Vg, [L], True)
    S = (Q[0].double() @ Kg[0, 0, :L].double().T) / d ** 0.5
    w = torch.softmax(S[:, -1], -1)
    assert (w[:, 3 * page:4 * page].sum(-1) > 0.5).all()           # (most of the last row's weight lies above byte 2^32)
    ld = torch.tensor([L], dtype=torch.int32, device=DEV)
    for splits in (0, 1):
        O, lse = fa.flash_attention_decode_paged(Q.to(DEV), Kp, Vp, table.to(DEV), ld, is_causal=True, out_dtype=torch.float32,
                                                 num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close(O, lse, refO, refL, f"pool of {P * page_bytes / 2 ** 30:.2f} GiB, d {d}, splits {splits}")
