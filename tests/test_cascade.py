"""GPU tests of shared-prefix (cascade) decode: flash_attention_cascade_decode / _paged through the Python fronts, shared capacity 384
and unique capacity 256, against the float64 reference of cascade_check.py under kv_cache_check.assert_close, unchanged.

1. parity: both d, all four cache forms (pages 16 and 128), four batch shapes whose B * G * Sq packed rows meet every seam of the
   64-row (d = 128) / 32-row (d = 64) row block, shared lengths around the tile, suffix lengths mixed in one batch (one below Sq),
   forced and chosen split counts, is_causal both ways;
2. the Q = 0 count probe: LSE = ln(ls + visible_i), O the mean of the visible rows of an index-coded V;
3. poison: NaN / inf (fp8: the NaN bytes) at and beyond ls, beyond every len_b and in unused pages, table entries of pages not read
   set to -1, 2^31 - 1 and numPages: the clean run bit for bit;
4. bit-for-bit seams: paged = contiguous on gathered copies, BF16 output = the F32 result rounded once, the LSE asked or not, two runs,
   sinks = -inf = no sinks; finite sinks, +-1e4 included, against the reference with sink_check.apply_sinks;
5. one captured graph of kv_lens += 1, kv_cache_append, cascade_decode, replayed after sharedLen, kvLens and the sinks changed on the device;
6. what the fronts refuse.
"""
import itertools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import cascade_check as cc  # noqa: E402
import kv_cache_check as kc  # noqa: E402
import sink_check as sc  # noqa: E402
from abi_decl import BAD_SHAPE  # noqa: E402
from kv_cache_check import DEV, i32, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
bf, f32 = torch.bfloat16, torch.float32

# (B, H, Hkv, Sq): 6 packed rows, one partial block; 60: one block with idle rows at d = 128, two at d = 64 with sequence 2 across the
# seam; 72: a second block at d = 128; 80
SHAPES = ((3, 4, 2, 1), (5, 8, 2, 3), (9, 8, 1, 1), (5, 2, 2, 16))
FORMS = ((0, False), (0, True), (16, False), (128, False), (16, True), (128, True))      # (page or 0, fp8)
FORM_IDS = ("contig-bf16", "contig-fp8", "paged16-bf16", "paged128-bf16", "paged16-fp8", "paged128-fp8")
FOUR = ((0, False), (16, False), (0, True), (128, True))
FOUR_IDS = ("contig-bf16", "paged16-bf16", "contig-fp8", "paged128-fp8")
LS = (1, 127, 128, 129, 384)
SPLITS = ((1, 2), (3, 2), (2, 5), (32, 32), (0, 0))


def suffix_lengths(B, Sq):
    """mixed in one batch from {Sq, Sq + 1, 128, 129, 256}; the Sq = 3 shape holds one len_b = 1 < Sq (the clamp to key 0)"""
    pick = (Sq, Sq + 1, 128, 129, 256)
    lens = [pick[(b + Sq) % 5] for b in range(B)]
    if Sq == 3:
        lens[lens.index(128)] = 1
    return lens


def queries(B, H, Sq, d, seed):
    return kc.randn((B, H, Sq, d), seed, bf)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-H%d-Hkv%d-Sq%d" % s)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d", [64, 128])
def test_parity(d, form, shape):
    (page, fp8), (B, H, Hkv, Sq) = form, shape
    if fp8 and kc.F8 is None:
        pytest.skip("this torch has no float8_e4m3fn")
    caches = cc.Caches(B, Hkv, d, page, fp8, seed=500 + d + page + 3 * fp8 + B)
    args, ds = caches.device()
    Q = queries(B, H, Sq, d, 900 + d + B)
    lens = suffix_lengths(B, Sq)
    assert any(L < Sq for L in lens) == (Sq == 3) and all(1 <= L <= cc.LU_CAP for L in lens)
    at = SHAPES.index(shape)
    for j, ls in enumerate(LS):
        for causal in ((False, True) if Sq > 1 else (False,)):
            ns = SPLITS[(j + at + causal) % len(SPLITS)]
            refO, refL = caches.reference(Q, ls, lens, causal)
            O, lse = cc.attend(args, ds, Q.to(DEV), ls, lens, is_causal=causal, num_splits=ns, out_dtype=f32)
            kc.assert_close(O, lse, refO, refL, f"d {d} {FORM_IDS[FORMS.index(form)]} {shape} ls {ls} lens {lens} causal {causal} splits {ns}")
    # every split pair at one length each, and the capacities through shared_len = kv_lens = None
    for ns in SPLITS:
        refO, refL = caches.reference(Q, 129, lens, True)
        O, lse = cc.attend(args, ds, Q.to(DEV), 129, lens, is_causal=True, num_splits=ns, out_dtype=f32)
        kc.assert_close(O, lse, refO, refL, f"d {d} {shape} ls 129 splits {ns}")
    refO, refL = caches.reference(Q, cc.LS_CAP, [cc.LU_CAP] * B, True)
    O, lse = cc.attend(args, ds, Q.to(DEV), None, None, is_causal=True, out_dtype=f32)
    kc.assert_close(O, lse, refO, refL, f"d {d} {shape} at the capacities")


@pytest.mark.parametrize("page", [0, 16, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_count_probe(d, page):
    """Q = 0: every visible key weighs the same, so LSE = ln(ls + visible_i) -- the tolerance 2e-4 + 2e-6 |ref| resolves one key up to
    about 5000 -- and O is the mean of the visible rows of V, index-coded: shared row k holds ((k + 3 j + kvh) % 128 - 64) / 16 at
    column j, row k of suffix b ((5 k + j + 11 b) % 128 - 64) / 16 + b, all exact in bf16"""
    B, H, Hkv, Sq = 5, 8, 2, 3
    k, j = torch.arange(cc.LS_CAP)[:, None], torch.arange(d)[None, :]
    sV = torch.stack([((k + 3 * j + h) % 128 - 64) / 16.0 for h in range(Hkv)])
    k = torch.arange(cc.LU_CAP)[:, None]
    uV = torch.stack([torch.stack([((5 * k + j + 11 * b) % 128 - 64) / 16.0 + b for _ in range(Hkv)]) for b in range(B)])
    assert torch.equal(sV.to(bf).float(), sV) and torch.equal(uV.to(bf).float(), uV)
    caches = cc.Caches(B, Hkv, d, page, False, seed=77 + d + page, sV=sV.to(bf), uV=uV.to(bf))
    args, ds = caches.device()
    Q = torch.zeros(B, H, Sq, d, dtype=bf)
    lens = suffix_lengths(B, Sq)
    for ls, causal, ns in ((1, True, (1, 2)), (127, False, (3, 2)), (129, True, (2, 5)), (384, True, (32, 32)), (384, False, (0, 0))):
        refO, refL = caches.reference(Q, ls, lens, causal)
        count = torch.stack([ls + kc.visible(L, Sq, causal).sum(-1) for L in lens]).double()          # [B, Sq]
        assert torch.allclose(refL, count.log()[:, None, :].expand(B, H, Sq), rtol=0, atol=1e-12)
        O, lse = cc.attend(args, ds, Q.to(DEV), ls, lens, is_causal=causal, num_splits=ns, out_dtype=f32)
        kc.assert_close(O, lse, refO, refL, f"count probe d {d} page {page} ls {ls} causal {causal} splits {ns}")
        worst = kc.lse_ratio(lse.cpu(), count.log()[:, None, :]).max().item()
        assert worst <= 1, f"LSE against ln(count): {worst:.3f} of the tolerance"


def poisoned(t, keep, fp8, flip):
    """a copy of a stored cache [..., rows, d] with the rows at and beyond `keep` alternating NaN / inf (fp8 bytes: 0x7F / 0xFF)"""
    out = t.clone()
    a, b = ((0x7F, 0xFF) if fp8 else (float("nan"), float("inf")))
    if flip:
        a, b = (b, a) if fp8 else (float("-inf"), float("nan"))
    out[..., keep::2, :] = a
    out[..., keep + 1::2, :] = b
    return out


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("d", [64, 128])
def test_poison(d, form):
    page, fp8 = form
    if fp8 and kc.F8 is None:
        pytest.skip("this torch has no float8_e4m3fn")
    B, H, Hkv, Sq = 5, 8, 2, 3
    caches = cc.Caches(B, Hkv, d, page, fp8, seed=1300 + d + page + fp8)
    Q = queries(B, H, Sq, d, 1301 + d).to(DEV)
    lens = suffix_lengths(B, Sq)
    clean_args, ds = caches.device()
    for ls, ns in ((1, (1, 2)), (129, (3, 2)), (300, (0, 0))):
        sK, sV = poisoned(caches.sK, ls, fp8, False), poisoned(caches.sV, ls, fp8, True)
        uK, uV = caches.uK.clone(), caches.uV.clone()
        for b, L in enumerate(lens):
            uK[b], uV[b] = poisoned(caches.uK[b], L, fp8, True), poisoned(caches.uV[b], L, fp8, False)
        tables = {}
        if page:       # the entries of the pages that hold no key below the length: freed by the engine, any int32
            junk = (-1, 2 ** 31 - 1, caches.shared_table.numel() + caches.block_table.numel() + caches.spare)
            st, bt = caches.shared_table.clone(), caches.block_table.clone()
            for n in range(-(-ls // page), st.numel()):
                st[n] = junk[n % 3]
            for b, L in enumerate(lens):
                for n in range(-(-L // page), bt.shape[1]):
                    bt[b, n] = junk[(n + b) % 3]
            tables = dict(shared_table=st, block_table=bt)
        dirty_args, _ = caches.device(sK, sV, uK, uV, fill=0xFF, **tables)        # (0xFF bytes: NaN in bf16 and in e4m3fn, in the unused pages)
        for causal in (False, True):
            kw = dict(is_causal=causal, num_splits=ns, out_dtype=f32)
            a, b = cc.attend(clean_args, ds, Q, ls, lens, **kw), cc.attend(dirty_args, ds, Q, ls, lens, **kw)
            assert torch.isfinite(b[0]).all() and torch.isfinite(b[1]).all(), (ls, ns, causal)
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), (ls, ns, causal)


@pytest.mark.parametrize("form", FOUR, ids=FOUR_IDS)
@pytest.mark.parametrize("d", [64, 128])
def test_bit_for_bit_seams(d, form):
    page, fp8 = form
    if fp8 and kc.F8 is None:
        pytest.skip("this torch has no float8_e4m3fn")
    B, H, Hkv, Sq = 5, 8, 2, 3
    caches = cc.Caches(B, Hkv, d, page, fp8, seed=1400 + d + page + fp8)
    Q = queries(B, H, Sq, d, 1401 + d).to(DEV)
    lens = suffix_lengths(B, Sq)
    args, ds = caches.device()
    flat, _ = caches.device(contiguous=True)
    for ls, ns, causal in ((129, (3, 2), True), (384, (2, 5), False), (127, (0, 0), True)):
        kw = dict(is_causal=causal, num_splits=ns)
        O, lse = cc.attend(args, ds, Q, ls, lens, out_dtype=f32, **kw)
        again = cc.attend(args, ds, Q, ls, lens, out_dtype=f32, **kw)
        assert same_bits(O, again[0]) and same_bits(lse, again[1]), "two runs"
        assert same_bits(O, cc.attend(args, ds, Q, ls, lens, out_dtype=f32, return_lse=False, **kw)), "O with and without the LSE"
        Ob, lseb = cc.attend(args, ds, Q, ls, lens, out_dtype=bf, **kw)
        assert Ob.dtype == bf and same_bits(Ob, O.to(bf)) and same_bits(lseb, lse), "BF16 output = the F32 result rounded once"
        assert same_bits(Ob, cc.attend(args, ds, Q, ls, lens, out_dtype=bf, return_lse=False, **kw))
        if page:
            Oc, lsec = cc.attend(flat, ds, Q, ls, lens, out_dtype=f32, **kw)
            assert same_bits(O, Oc) and same_bits(lse, lsec), "paged = contiguous on gathered copies"
        none = torch.full((H,), float("-inf"), dtype=f32, device=DEV)
        On, lsen = cc.attend(args, ds, Q, ls, lens, out_dtype=f32, sinks=none, **kw)
        assert same_bits(O, On) and same_bits(lse, lsen), "sinks = -inf = no sinks"


@pytest.mark.parametrize("form", FOUR, ids=FOUR_IDS)
@pytest.mark.parametrize("d", [64, 128])
def test_finite_sinks(d, form):
    page, fp8 = form
    if fp8 and kc.F8 is None:
        pytest.skip("this torch has no float8_e4m3fn")
    B, H, Hkv, Sq = 5, 8, 2, 3
    caches = cc.Caches(B, Hkv, d, page, fp8, seed=1500 + d + page + fp8)
    Q = queries(B, H, Sq, d, 1501 + d)
    lens = suffix_lengths(B, Sq)
    args, ds = caches.device()
    wide = sc.sinks_for(H)
    wide[1], wide[2] = 1e4, -1e4
    for sinks, (ls, ns, causal) in itertools.product((sc.sinks_for(H), wide), ((129, (3, 2), True), (1, (1, 2), False), (384, (0, 0), True))):
        refO, refL = caches.reference(Q, ls, lens, causal, sinks=sinks)
        plainO, plainL = caches.reference(Q, ls, lens, causal)
        assert (refL - plainL).abs().max() > 1.0                                      # the sinks matter
        O, lse = cc.attend(args, ds, Q.to(DEV), ls, lens, is_causal=causal, num_splits=ns, out_dtype=f32, sinks=sinks.to(DEV))
        kc.assert_close(O, lse, refO, refL, f"sinks d {d} ls {ls} splits {ns} causal {causal} max {sinks.max().item():.0f}")


@pytest.mark.parametrize("page", [0, 16])
@pytest.mark.parametrize("d", [64, 128])
def test_one_graph_follows_the_values_of_the_moment(d, page):
    """kv_lens += 1; kv_cache_append; cascade_decode captured as one graph and replayed after sharedLen, kvLens and the sinks changed"""
    B, H, Hkv, Sq = 5, 8, 2, 1
    caches = cc.Caches(B, Hkv, d, page, False, seed=1600 + d + page)
    args, ds = caches.device()
    Q = queries(B, H, Sq, d, 1601 + d)
    Kn, Vn = kc.randn((B, Hkv, 1, d), 1602 + d, bf), kc.randn((B, Hkv, 1, d), 1603 + d, bf)
    q, kn, vn = Q.to(DEV), Kn.to(DEV), Vn.to(DEV)
    lens, sl, sinks = i32([1] * B), i32([1]), torch.zeros(H, dtype=f32, device=DEV)
    O = torch.empty(B, H, Sq, d, dtype=f32, device=DEV)
    need = fa.decode_workspace_size(B, H, Sq, d, fa.cascade_plan(B, H, Hkv, Sq, cc.LS_CAP, cc.LU_CAP, d)["num_splits"])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def step():
        lens.add_(1)
        if page:
            fa.kv_cache_append_paged(kn, vn, args[0], args[1], args[3], lens)
            return fa.flash_attention_cascade_decode_paged(q, *args, sl, lens, is_causal=True, return_lse=True, O=O, workspace=ws, sinks=sinks)
        fa.kv_cache_append(kn, vn, args[2], args[3], lens)
        return fa.flash_attention_cascade_decode(q, *args, sl, lens, is_causal=True, return_lse=True, O=O, workspace=ws, sinks=sinks)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse = step()
    uK, uV = caches.refuK.clone(), caches.refuV.clone()
    uK[:, :, 1], uV[:, :, 1] = Kn[:, :, 0].double(), Vn[:, :, 0].double()             # (the step before the capture: lengths 1 -> 2)
    seen = []
    for r, (start, ls, vec) in enumerate((([3, 127, 128, 200, 9], 129, sc.sinks_for(H)), ([254, 1, 30, 128, 129], 384, torch.full((H,), float("-inf"))),
                                          ([7, 8, 9, 10, 11], 1, sc.sinks_for(H).flip(0) + 1.0))):
        lens.copy_(i32(start))
        sl.copy_(i32([ls]))
        sinks.copy_(vec.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        now = lens.tolist()
        assert now == [s + 1 for s in start]
        for b, L in enumerate(now):                                                   # what the append of this replay wrote
            uK[b, :, L - 1], uV[b, :, L - 1] = Kn[b, :, 0].double(), Vn[b, :, 0].double()
        refO, refL = cc.reference(Q, caches.refsK, caches.refsV, uK, uV, ls, now, True, sinks=vec)
        kc.assert_close(O, lse, refO, refL, f"replay {r}")
        seen.append(O.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_refused_by_the_front():
    B, H, Hkv, d = 2, 4, 2, 64
    caches = cc.Caches(B, Hkv, d, 0, False, seed=5)
    args, _ = caches.device()
    q = queries(B, H, 17, d, 6).to(DEV)
    with pytest.raises(fa.FlashAttentionError) as e:                                  # Sq = 17: chunked prefill, not this call
        fa.flash_attention_cascade_decode(q, *args)
    assert e.value.code == BAD_SHAPE
    q = q[:, :, :4].contiguous()
    with pytest.raises(TypeError, match="window"):                                    # there is no window argument
        fa.flash_attention_cascade_decode(q, *args, window=16)
    with pytest.raises(TypeError, match="share a dtype"):                             # mismatched shared and unique dtypes
        fa.flash_attention_cascade_decode(q, args[0].half(), args[1].half(), args[2], args[3])
    if kc.F8 is not None:
        with pytest.raises(TypeError, match="share a dtype"):
            fa.flash_attention_cascade_decode(q, args[0].to(kc.F8), args[1].to(kc.F8), args[2], args[3])
    O = fa.flash_attention_cascade_decode(q, *args)                                   # and the call as it should be goes through
    assert O.shape == q.shape and torch.isfinite(O.float()).all()
