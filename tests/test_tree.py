"""GPU tests of tree-masked verification (flash_attention_tree, flash_attention_tree_paged): B = 2, Hkv = 2, capacity 384 (three 128-key
tiles), as the attention-sink tests; the helper, the mask families and the reference are tests/tree_check.py's.

1. float64 parity: d 64 / 128, G 1 / 4, Sq 1 / 5 / 16 / 17 / 33 / 64, star / binary / random-parent masks (two different ones per
   case), the draft's keys inside one tile, across the 128- and 256-key tile starts, at len == Sq and at len < Sq, forced splits 1 / 2 /
   3 and the library's own, the four cache forms (pages of 16 and of 128, the draft's keys across a page boundary), windows 0 / 7 / 130,
   sinks of sink_check.sinks_for -- and tree_check.assert_masks_matter on every reference.
2. exact mask read-back: Q = 0 and V[base + j][j] = 1 make O[i][j] n_i bit j of row i's effective word -- on the parity lengths, and
   on a 2^15-key cache under the planned split count (contiguous bf16, paged fp8), at Sq = 64, d = 128.
3. bit-for-bit seams, O and LSE: chain and all-ones words are the causal sink twin; paged is contiguous on a gathered copy; garbage in
   the ignored bits changes nothing; sinks = NULL is a vector of -inf.
4. non-leakage: invisible sibling nodes holding huge K and V leave a row's bits those of the run with those rows zeroed.
5. one step end to end: append a tree, verify, accept a path, rewind, re-append it; and a captured graph replayed on other words.
"""
import itertools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import kv_cache_check as kv  # noqa: E402
import sink_check as sc  # noqa: E402
import tree_check as tc  # noqa: E402
from kv_cache_check import DEV, Cache, i32, same_bits  # noqa: E402
from sink_check import FORM_IDS, FORMS, HKV  # noqa: E402
from tree_check import B, CAP, bf16, f32  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = (1, 5, 16, 17, 33, 64)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("d", [64, 128])
def test_parity_against_the_float64_reference(d, G, form):
    assert tc.run_parity(d, G, form, ROWS) >= 30


def probe_cache(d, form, Sq, lens, seed):
    """a cache in `form` whose V is tree_check.probe_values (exact in e4m3fn: descales 1) and whose K is N(0, 1) -- Q = 0 makes it moot"""
    g = torch.Generator().manual_seed(seed)
    K = torch.randn(B, HKV, CAP, d, generator=g).to(bf16)
    return Cache(d, *form, seed, K=K, V=tc.probe_values(Sq, lens, d), descales=(torch.tensor([1.0, 0.5]), torch.tensor([1.0, 1.0])))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d,G", [(64, 4), (128, 1), (128, 4)])
def test_exact_read_back_of_the_effective_words(d, G, form):
    H = HKV * G
    for n, Sq in enumerate(ROWS):
        Q = torch.zeros(B, H, Sq, d, dtype=bf16, device=DEV)
        for m, lens in enumerate(tc.lengths(Sq)):
            c = probe_cache(d, form, Sq, lens, 1500 + d).device()
            W = sc.WINDOWS[(n + m) % 3]
            words, names = tc.case_words(Sq, n + m, tc.FAMILIES)
            wt = tc.words_tensor(words).to(DEV)
            for ns in (1, 3, 0):
                O, lse = tc.attend(c, Q, i32(lens), wt, window=W, num_splits=ns, out_dtype=f32)
                tc.assert_read_back(O, lens, W, words, f"read-back d{d} G{G} Sq{Sq} lens{lens} window{W} {'/'.join(names)} splits{ns}")
                # Q = 0: every visible key has weight 1 / n_i, so the LSE is ln n_i
                n_i = torch.stack([tc.expected_bits(Sq, L, W, words[b])[1] for b, L in enumerate(lens)])
                assert ((lse.double().cpu() - n_i.log()[:, None, :]).abs() <= 2e-4 + 2e-6 * n_i.log()[:, None, :]).all()


@pytest.mark.parametrize("paged_fp8", [False, True], ids=["contig-bf16", "paged128-fp8"])
def test_exact_read_back_on_a_long_cache_under_the_planned_splits(paged_fp8):
    """2^15 keys of capacity, Sq = 64, d = 128: the plan splits the keys many times, and the split boundaries lie far from the draft's keys"""
    d, G, Sq, cap, lens = 128, 4, 64, 1 << 15, (1 << 15, 20011)
    H = HKV * G
    plan = fa.tree_plan(B, H, HKV, Sq, cap, d, fa.FA_DTYPE_F32)
    assert plan["num_splits"] > 2 and plan == fa.extend_plan(B, H, HKV, Sq, cap, d, fa.FA_DTYPE_F32), plan
    words = [tc.words_of("binary", Sq), tc.words_of("random", Sq, 5)]
    wt = tc.words_tensor(words).to(DEV)
    Q = torch.zeros(B, H, Sq, d, dtype=bf16, device=DEV)
    if not paged_fp8:
        K = torch.zeros(B, HKV, cap, d, dtype=bf16, device=DEV)
        V = torch.zeros(B, HKV, cap, d, dtype=bf16, device=DEV)
        for b, L in enumerate(lens):
            V[b, :, torch.arange(L - Sq, L), torch.arange(Sq)] = 1.0
        O = fa.flash_attention_tree(Q, K, V, wt, i32(lens), out_dtype=f32)
    else:
        page, n = 128, cap // 128
        table = torch.randperm(B * n, generator=torch.Generator().manual_seed(9)).reshape(B, n).to(torch.int32)
        V = torch.zeros(B * n, HKV, page, d, dtype=torch.uint8)
        for b, L in enumerate(lens):
            for j in range(Sq):
                key = L - Sq + j
                V[int(table[b, key // page]), :, key % page, j] = 0x38                     # 1.0 in e4m3fn
        K = torch.zeros(B * n, HKV, page, d, dtype=torch.uint8)
        O = fa.flash_attention_tree_paged(Q, K.view(kv.F8).to(DEV), V.view(kv.F8).to(DEV), table.to(DEV), wt, i32(lens), out_dtype=f32)
    tc.assert_read_back(O, lens, 0, words, f"long cache, {plan['num_splits']} splits")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d,G", [(64, 4), (128, 1)])
def test_chain_and_all_ones_words_are_the_causal_twin_bit_for_bit(d, G, form):
    cache = Cache(d, *form, 1600 + d)
    c = cache.device()
    H = HKV * G
    sinks = sc.sinks_for(H).to(DEV)
    for n, Sq in enumerate(ROWS):
        Q = sc.queries("decode", d, G, Sq, 13 * d + Sq).to(DEV)
        for (m, lens), ns in itertools.product(enumerate(tc.lengths(Sq)), (1, 3)):
            W = sc.WINDOWS[(n + m) % 3]
            for odt, with_sinks in ((f32, True), (bf16, False)):
                kw = dict(window=W, num_splits=ns, out_dtype=odt, sinks=sinks if with_sinks else None)
                want = tc.twin(c, Q, i32(lens), **kw)
                for family in tc.TWINS:
                    got = tc.attend(c, Q, i32(lens), tc.words_tensor([tc.words_of(family, Sq)] * B).to(DEV), **kw)
                    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), \
                        f"d{d} G{G} Sq{Sq} lens{lens} window{W} splits{ns} {odt} {family}: not the causal twin"


@pytest.mark.parametrize("page,fp8", [(16, False), (128, False), (16, True), (128, True)])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_equals_contiguous_and_ignored_bits_and_null_sinks_change_nothing(d, page, fp8):
    G = 4
    H = HKV * G
    cache = Cache(d, page, fp8, 1700 + d)
    paged, contig = cache.device(), cache.device(contiguous=True)
    sinks = sc.sinks_for(H).to(DEV)
    none = torch.full((H,), sc.NEG_INF, dtype=f32, device=DEV)
    for n, Sq in enumerate(ROWS):
        Q = sc.queries("decode", d, G, Sq, 17 * d + Sq).to(DEV)
        for (m, lens), ns in itertools.product(enumerate(tc.lengths(Sq)), (1, 3)):
            W = sc.WINDOWS[(n + m) % 3]
            words, _ = tc.case_words(Sq, n + m)
            wt = tc.words_tensor(words).to(DEV)
            what = f"d{d} Sq{Sq} lens{lens} window{W} splits{ns}"
            kw = dict(window=W, num_splits=ns, out_dtype=f32)
            a, b = tc.attend(paged, Q, i32(lens), wt, sinks=sinks, **kw), tc.attend(contig, Q, i32(lens), wt, sinks=sinks, **kw)
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), f"{what}: paged is not contiguous on a gathered copy"
            # garbage above i and at or beyond Sq, and the self bit cleared: the rule reads none of it
            dirty = [[(w & ~(1 << i)) | (tc.FULL << (i + 1) & tc.FULL) for i, w in enumerate(row)] for row in words]
            g = tc.attend(paged, Q, i32(lens), tc.words_tensor(dirty).to(DEV), sinks=sinks, **kw)
            assert same_bits(g[0], a[0]) and same_bits(g[1], a[1]), f"{what}: the ignored bits were read"
            x, y = tc.attend(paged, Q, i32(lens), wt, sinks=None, **kw), tc.attend(paged, Q, i32(lens), wt, sinks=none, **kw)
            assert same_bits(x[0], y[0]) and same_bits(x[1], y[1]), f"{what}: sinks = NULL is not a vector of -inf"


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d,Sq", [(64, 16), (128, 33)])
def test_invisible_siblings_do_not_leak(d, Sq, form):
    """A binary tree.  The nodes of the root's right subtree are invisible to the root and to every node of its left subtree.  Their K
    rows are scaled by 1e4 and their V rows set to +-1e30 (an fp8 cache: K and V to +-448, the largest e4m3fn
    values): the rows that do not see them keep, bit for bit, the O and LSE of the run with those K / V rows zeroed."""
    page, fp8 = form
    G = 4
    parents = tc.parents_of("binary", Sq)
    side = [0] * Sq                                            # 0 the root, 1 its left subtree, 2 its right one
    for i in range(1, Sq):
        side[i] = i if i <= 2 else side[parents[i]]
    hidden, watched = [i for i in range(Sq) if side[i] == 2], [i for i in range(Sq) if side[i] != 2]
    words = [tc.words_of("binary", Sq)] * B
    assert all(not words[0][i] >> j & 1 for i in watched for j in hidden)
    wt = tc.words_tensor(words).to(DEV)
    g = torch.Generator().manual_seed(1800 + d)
    K, V = (torch.randn(B, HKV, CAP, d, generator=g).to(bf16) for _ in range(2))
    Q = sc.queries("decode", d, G, Sq, 19 * d + Sq).to(DEV)
    for lens, W, ns in itertools.product(((Sq + 3, 300), (128 + Sq // 2, 256 + Sq // 2)), (0, 130), (1, 3)):
        runs = []
        for poison in (True, False):
            k, v = K.clone().float(), V.clone().float()
            for b, L in enumerate(lens):
                rows = torch.tensor([L - Sq + j for j in hidden])
                sign = torch.where(torch.arange(len(hidden)) % 2 == 0, 1.0, -1.0)[None, :, None].expand(HKV, -1, d)
                if poison:
                    k[b, :, rows] = sign * 448.0 if fp8 else k[b, :, rows] * 1e4
                    v[b, :, rows] = sign * (448.0 if fp8 else 1e30)
                else:
                    k[b, :, rows], v[b, :, rows] = 0.0, 0.0
            ds = (torch.tensor([1.0, 0.5]), torch.tensor([1.0, 1.0])) if fp8 else None        # (the stored values are e4m3fn numbers as they stand)
            cache = Cache(d, page, fp8, 1801, K=k.to(bf16), V=v.to(bf16), descales=ds)
            runs.append(tc.attend(cache.device(), Q, i32(lens), wt, window=W, num_splits=ns, out_dtype=f32, sinks=sc.sinks_for(HKV * G).to(DEV)))
        (Op, lp), (Oz, lz) = runs
        assert torch.isfinite(Op[:, :, watched]).all() and torch.isfinite(lp[:, :, watched]).all()
        assert same_bits(Op[:, :, watched], Oz[:, :, watched]) and same_bits(lp[:, :, watched], lz[:, :, watched]), \
            f"d{d} Sq{Sq} lens{lens} window{W} splits{ns}: a row that does not see the right subtree changed with it"
        assert not same_bits(Op[:, :, hidden], Oz[:, :, hidden])                              # (the rows that see them did change)


@pytest.mark.parametrize("d,Sq", [(64, 7), (128, 31)])
def test_one_speculative_step_end_to_end(d, Sq):
    """kv_lens += Sq; kv_cache_append of a binary tree; flash_attention_tree; accept one root-to-leaf path; rewind kv_lens to base and
    re-append the accepted rows with kv_cache_append_varlen.  Each accepted node's row of the tree call is the reference of the linear
    sequence up to it, and a plain flash_attention_decode of a further token is the reference on the accepted sequence."""
    G, start = 4, (100, 250)
    H = HKV * G
    g = torch.Generator().manual_seed(1900 + d)
    K0, V0 = (torch.randn(B, HKV, CAP, d, generator=g).to(bf16) for _ in range(2))
    Kn, Vn = (torch.randn(B, HKV, Sq, d, generator=g).to(bf16) for _ in range(2))
    Qc = torch.randn(B, H, Sq, d, generator=g).to(bf16)
    K, V, lens = K0.to(DEV), V0.to(DEV), i32(start)
    parents = tc.parents_of("binary", Sq)
    mask = fa.tree_mask_from_parents(torch.tensor([parents] * B, device=DEV))
    lens += Sq
    fa.kv_cache_append(Kn.to(DEV), Vn.to(DEV), K, V, lens)
    O, lse = fa.flash_attention_tree(Qc.to(DEV), K, V, mask, lens, return_lse=True, out_dtype=f32)
    # the whole call against the rule's reference on the cache as the append left it
    refO, refL = kv.reference(Qc, K.cpu(), V.cpu(), [s + Sq for s in start], True, 0, words=[tc.words_of_parents(parents)] * B)
    kv.assert_close(O, lse, refO, refL, "the tree call")
    path = [Sq - 1]                                            # the last node's walk to the root, root first
    while parents[path[0]] >= 0:
        path.insert(0, parents[path[0]])
    assert path[0] == 0 and len(path) >= 3
    # the linear sequence: the prefix, then the accepted rows
    Kl, Vl = K0.clone(), V0.clone()
    for b, s in enumerate(start):
        Kl[b, :, s:s + len(path)], Vl[b, :, s:s + len(path)] = Kn[b][:, path], Vn[b][:, path]
    for t, node in enumerate(path):
        wantO, wantL = kv.reference(Qc[:, :, node:node + 1], Kl, Vl, [s + t + 1 for s in start], True)
        kv.assert_close(O[:, :, node:node + 1], lse[:, :, node:node + 1], wantO, wantL, f"accepted node {node} (depth {t})")
    assert fa.tree_depths([parents])[0, path].tolist() == list(range(len(path)))
    # rewind and re-append the accepted rows, packed by token
    lens -= Sq
    lens += len(path)
    cu = i32([0, len(path), 2 * len(path)])
    pack = lambda T: T[:, :, path].permute(0, 2, 1, 3).reshape(B * len(path), HKV, d).contiguous().to(DEV)
    fa.kv_cache_append_varlen(pack(Kn), pack(Vn), K, V, cu, lens)
    for b, s in enumerate(start):
        assert torch.equal(K[b, :, :s + len(path)].cpu(), Kl[b, :, :s + len(path)]) and torch.equal(V[b, :, :s + len(path)].cpu(), Vl[b, :, :s + len(path)])
    # a further token, plain decode
    k1, v1 = (torch.randn(B, HKV, 1, d, generator=g).to(bf16) for _ in range(2))
    q1 = torch.randn(B, H, 1, d, generator=g).to(bf16)
    lens += 1
    fa.kv_cache_append(k1.to(DEV), v1.to(DEV), K, V, lens)
    for b, s in enumerate(start):
        Kl[b, :, s + len(path)], Vl[b, :, s + len(path)] = k1[b, :, 0], v1[b, :, 0]
    O1, lse1 = fa.flash_attention_decode(q1.to(DEV), K, V, lens, is_causal=True, return_lse=True, out_dtype=f32)
    assert lens.tolist() == [s + len(path) + 1 for s in start]
    kv.assert_close(O1, lse1, *kv.reference(q1, Kl, Vl, [s + len(path) + 1 for s in start], True), "the next token")


@pytest.mark.parametrize("Sq,ns", [(5, 1), (16, 2), (33, 1), (64, 3)])
def test_graph_replays_see_the_words_of_the_moment(Sq, ns):
    d, G, W, lens = 64, 4, 130, (Sq + 40, 300)
    cache = Cache(d, None, False, 2000)
    c = cache.device()
    sinks = sc.sinks_for(HKV * G)
    Qc = sc.queries("decode", d, G, Sq, 2001 + Sq)
    Q, L, sk = Qc.to(DEV), i32(lens), sinks.to(DEV)
    wt = tc.words_tensor([tc.words_of("chain", Sq)] * B).to(DEV)
    step = lambda: tc.attend(c, Q, L, wt, window=W, num_splits=ns, sinks=sk, out_dtype=f32)
    step()                                                     # every kernel of the step has run once before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        O, lse = step()
    seen = []
    for r, families in enumerate((("binary", "star"), ("random", "binary"), ("star", "chain"))):
        words = [tc.words_of(f, Sq, r) for f in families]
        wt.copy_(tc.words_tensor(words).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        kv.assert_close(O, lse, *kv.reference(Qc, cache.refK, cache.refV, lens, True, W, words=words, sinks=sinks), f"replay {r} {families}")
        seen.append(O.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
