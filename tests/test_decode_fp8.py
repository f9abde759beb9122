"""GPU tests of split-KV decode against fp8 (e4m3fn) K/V caches, contiguous and paged: flash_attention_decode and
flash_attention_decode_paged with float8_e4m3fn K/V under a bf16 Q and per-K/V-head descales.

Data: K, V ~ N(0, 1), quantised per K/V head with descale = amax / 448.  The reference is the float64 explicit softmax over the
DEQUANTISED values K8 * k_descale, V8 * v_descale, so the error of quantising is not part of the comparison: every element of the
fp32 output within the project's stated 1e-3 + 1e-3 |ref|, the LSE within 2e-4 + 2e-6 |ref|.  The bounds need no new margin: the
fp8 -> bf16 conversion is exact, the dequantised data is N(0, 1)-scale and the arithmetic after the conversion is the bf16 decode
kernel's, whose worst element over its own sweep is 0.036 of that tolerance.  Every case prints its worst ratio.

The caches are handled as uint8 tensors here (indexing, gathering, poisoning) and viewed as float8_e4m3fn at the call."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from kv_cache_check import CAP, DEV, F8, assert_close, dequantise, gather, max_pages_of, paged_layout, quantise, randn, reference  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
SPLITS = (0, 1, 2, 3, CAP)
SHAPES = [(1, 1), (1, 4), (5, 8), (16, 16), (2, 2)]      # (Sq, G)


def f8(t):
    return t.view(F8)


# ---- 1. contiguous sweep ----
LENS = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 317, 320]


@functools.lru_cache(maxsize=2)
def contiguous_case(d, Hkv=2, cap=320):
    """one sequence per length; returns CPU bytes and descales, their dequantised float64 values, and the device tensors"""
    B = len(LENS)
    K8, kd = quantise(randn((B, Hkv, cap, d), 100 + d, F32))
    V8, vd = quantise(randn((B, Hkv, cap, d), 200 + d, F32))
    assert len({float(x) for x in (*kd, *vd)}) == 4         # different for K and V and for the two heads
    dev = tuple(t.to(DEV) for t in (K8, V8, kd, vd, torch.tensor(LENS, dtype=torch.int32)))
    return K8, V8, kd, vd, dequantise(K8, kd), dequantise(V8, vd), dev


@pytest.mark.parametrize("Sq,G", SHAPES)
@pytest.mark.parametrize("d", [64, 128])
def test_contiguous_sweep_against_float64(d, Sq, G):
    K8, V8, kd, vd, Kf, Vf, (Kd, Vd, kdd, vdd, ld) = contiguous_case(d)
    B, Hkv = K8.shape[:2]
    Q = randn((B, G * Hkv, Sq, d), 300 + Sq + G, torch.bfloat16)
    Qd = Q.to(DEV)
    for causal in (False, True):
        refO, refL = reference(Q, Kf, Vf, LENS, causal)
        for splits in SPLITS:
            kw = dict(is_causal=causal, num_splits=splits, k_descale=kdd, v_descale=vdd)
            O, lse = fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, out_dtype=torch.float32, return_lse=True, **kw)
            torch.cuda.synchronize()
            assert_close(O, lse, refO, refL, f"contiguous d {d} Sq {Sq} G {G} causal {causal} splits {splits}")
            for dt in (torch.bfloat16, torch.float16):      # the fp32 result of the same call rounded once
                Ol = fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, out_dtype=dt, **kw)
                assert Ol.dtype == dt and torch.equal(Ol, O.to(dt)), dt
    refO, refL = reference(Q, Kf, Vf, None, True)
    O, lse = fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), None, is_causal=True, out_dtype=torch.float32, return_lse=True,
                                       k_descale=kdd, v_descale=vdd)
    torch.cuda.synchronize()
    assert_close(O, lse, refO, refL, f"contiguous d {d} Sq {Sq} G {G} no lengths")
    assert fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, k_descale=kdd, v_descale=vdd).dtype == torch.bfloat16   # the default: Q's


# ---- 2. paged sweep ----
@functools.lru_cache(maxsize=2)
def paged_case(page, d, Hkv=2):
    """pools with more pages than any sequence uses, a random permutation as the table, one sequence per boundary length"""
    P, table, lens = paged_layout(page, d)
    Kp, kd = quantise(randn((P, Hkv, page, d), 1000 + page + d, F32))
    Vp, vd = quantise(randn((P, Hkv, page, d), 2000 + page + d, F32))
    dev = tuple(t.to(DEV) for t in (Kp, Vp, kd, vd, table, torch.tensor(lens, dtype=torch.int32)))
    Kf, Vf = dequantise(gather(Kp, table), kd), dequantise(gather(Vp, table), vd)
    return lens, Kf, Vf, dev


@pytest.mark.parametrize("Sq,G", SHAPES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [16, 128])
def test_paged_sweep_against_float64(page, d, Sq, G):
    lens, Kf, Vf, (Kd, Vd, kdd, vdd, td, ld) = paged_case(page, d)
    B, Hkv = len(lens), Kd.shape[1]
    Q = randn((B, G * Hkv, Sq, d), 4000 + Sq + G, torch.bfloat16)
    Qd = Q.to(DEV)
    for causal in (False, True):
        refO, refL = reference(Q, Kf, Vf, lens, causal)
        for splits in SPLITS:
            kw = dict(is_causal=causal, num_splits=splits, k_descale=kdd, v_descale=vdd)
            O, lse = fa.flash_attention_decode_paged(Qd, f8(Kd), f8(Vd), td, ld, out_dtype=torch.float32, return_lse=True, **kw)
            torch.cuda.synchronize()
            assert_close(O, lse, refO, refL, f"paged {page} d {d} Sq {Sq} G {G} causal {causal} splits {splits} lens {lens}")
            for dt in (torch.bfloat16, torch.float16):
                Ol = fa.flash_attention_decode_paged(Qd, f8(Kd), f8(Vd), td, ld, out_dtype=dt, **kw)
                assert Ol.dtype == dt and torch.equal(Ol, O.to(dt)), dt
    refO, refL = reference(Q, Kf, Vf, None, True)
    O, lse = fa.flash_attention_decode_paged(Qd, f8(Kd), f8(Vd), td, None, is_causal=True, out_dtype=torch.float32, return_lse=True,
                                             k_descale=kdd, v_descale=vdd)
    torch.cuda.synchronize()
    assert_close(O, lse, refO, refL, f"paged {page} d {d} Sq {Sq} G {G} no lengths")


# ---- 3. paged = contiguous on a gathered copy, bit for bit ----
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [16, 32, 128, 256])
def test_paged_is_bitwise_the_contiguous_path_on_a_gathered_copy(page, d):
    lens, Kf, Vf, (Kd, Vd, kdd, vdd, td, ld) = paged_case(page, d)
    B, Hkv = td.shape[0], Kd.shape[1]
    Kg, Vg = gather(Kd, td), gather(Vd, td)
    for Sq, G in ((1, 4), (5, 8)):
        Q = randn((B, G * Hkv, Sq, d), 5000 + Sq, torch.bfloat16).to(DEV)
        for causal in (False, True):
            for splits in SPLITS:
                kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, k_descale=kdd, v_descale=vdd)
                O, lse = fa.flash_attention_decode_paged(Q, f8(Kd), f8(Vd), td, ld, **kw)
                Oc, lsec = fa.flash_attention_decode(Q, f8(Kg), f8(Vg), ld, **kw)
                torch.cuda.synchronize()
                assert torch.isfinite(O).all() and torch.equal(O, Oc) and torch.equal(lse, lsec), (Sq, G, causal, splits)


# ---- 4. the descales: per head, read by the kernel ----
@pytest.mark.parametrize("d", [64, 128])
def test_descales_are_applied_per_head(d):
    K8, V8, kd, vd, Kf, Vf, (Kd, Vd, kdd, vdd, ld) = contiguous_case(d)
    B, Hkv, G, Sq = K8.shape[0], 2, 4, 3
    Q = randn((B, G * Hkv, Sq, d), 400, torch.bfloat16)
    Qd = Q.to(DEV)
    run = lambda k, v, splits: fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, is_causal=True, out_dtype=torch.float32,
                                                         num_splits=splits, return_lse=True, k_descale=k, v_descale=v)
    kf, vf = torch.tensor([0.5, 2.0]), torch.tensor([4.0, 0.25])       # powers of two, different per head
    k2, v2 = (kd * kf).to(DEV), (vd * vf).to(DEV)
    for splits in (1, 3):
        base = run(kdd, vdd, splits)
        # the same bytes under other descales: the result moves as the reference does
        refO, refL = reference(Q, dequantise(K8, kd * kf), dequantise(V8, vd * vf), LENS, True)
        assert_close(*run(k2, v2, splits), refO, refL, f"descales x {kf.tolist()} / {vf.tolist()}, d {d} splits {splits}")
        # V's descale alone by a power of two, per head: O scales exactly, the LSE does not move
        O, lse = run(kdd, v2, splits)
        per_head = vf.repeat_interleave(G).to(DEV)[None, :, None, None]
        assert torch.equal(O, base[0] * per_head) and torch.equal(lse, base[1])
        # K's alone: head 0 and head 1 differ from the base, each as the reference says
        O, lse = run(k2, vdd, splits)
        assert not torch.equal(O[:, :G], base[0][:, :G]) and not torch.equal(O[:, G:], base[0][:, G:])
        refO, refL = reference(Q, dequantise(K8, kd * kf), Vf, LENS, True)
        assert_close(O, lse, refO, refL, f"K descales x {kf.tolist()}, d {d} splits {splits}")
    # None = ones, bit for bit, for each (the bytes taken at face value are large: a small softmax scale keeps the scores in range)
    ones = torch.ones(Hkv, device=DEV)
    kw = dict(is_causal=True, out_dtype=torch.float32, num_splits=2, return_lse=True, scale=1e-3)
    want = fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, k_descale=ones, v_descale=ones, **kw)
    for k, v in ((None, None), (ones, None), (None, ones)):
        got = fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, k_descale=k, v_descale=v, **kw)
        assert torch.isfinite(got[0]).all() and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_graph_replay_reads_the_descales_and_the_lengths_of_the_moment(d, paged):
    B, Hkv, G, Sq, page, n = 2, 2, 4, 1, 128, 32
    cap, H = n * page, G * Hkv
    K8, kd = quantise(randn((B, Hkv, cap, d), 500 + d, F32))
    V8, vd = quantise(randn((B, Hkv, cap, d), 501 + d, F32))
    Q = randn((B, H, Sq, d), 502, torch.bfloat16)
    lens = [1000, 3 * page]
    Kd, Vd, kdd, vdd, Qd = (t.to(DEV) for t in (K8, V8, kd, vd, Q))
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    if paged:     # the same data as pages [B n, Hkv, page, d] behind a reversed table
        pool = lambda t: t.view(B, Hkv, n, page, d).transpose(1, 2).reshape(B * n, Hkv, page, d).flip(0).contiguous()
        td = torch.arange(B * n - 1, -1, -1, dtype=torch.int32, device=DEV).reshape(B, n)
        Kp, Vp = pool(Kd), pool(Vd)
        call = lambda **kw: fa.flash_attention_decode_paged(Qd, f8(Kp), f8(Vp), td, ld, is_causal=True, k_descale=kdd, v_descale=vdd, **kw)
    else:
        call = lambda **kw: fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, is_causal=True, k_descale=kdd, v_descale=vdd, **kw)
    plan = fa.decode_plan(B, H, Hkv, Sq, cap, d, fa.FA_DTYPE_F32)
    assert plan["num_splits"] > 1
    ws = torch.empty(fa.decode_workspace_size(B, H, Sq, d, plan["num_splits"]), dtype=torch.uint8, device=DEV)
    O = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
    call(O=O, workspace=ws)            # (first call outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(O=O, workspace=ws)
    O.zero_()
    graph.replay()
    torch.cuda.synchronize()
    first = call(out_dtype=torch.float32).clone()
    assert torch.isfinite(O).all() and torch.equal(O, first)
    # in place: another K descale for head 0, another V descale for head 1, every sequence one key longer
    kdd[0] *= 0.75
    vdd[1] *= 1.5
    ld += 1
    graph.replay()
    torch.cuda.synchronize()
    second = call(out_dtype=torch.float32).clone()
    assert torch.equal(O, second) and not torch.equal(first[:, :G], second[:, :G]) and not torch.equal(first[:, G:], second[:, G:])
    refO, _ = reference(Q, dequantise(K8, kdd.cpu()), dequantise(V8, vdd.cpu()), [L + 1 for L in lens], True)
    err, tol = (O.double().cpu() - refO).abs(), 1e-3 + 1e-3 * refO.abs()
    print(f"graph replay d {d} paged {paged}: worst O error / tolerance {(err / tol).max().item():.3f}")
    assert (err <= tol).all()


# ---- 5. poison ----
def poison(t, seed):
    """bytes 0x7F, 0xFF (the NaNs of e4m3fn) and random ones, in turn along the last dimension"""
    g = torch.Generator().manual_seed(seed)
    junk = torch.randint(0, 256, t.shape, generator=g, dtype=torch.uint8)
    pos = torch.arange(t.shape[-1]) % 3
    junk[..., pos == 0] = 0x7F
    junk[..., pos == 1] = 0xFF
    return junk


@pytest.mark.parametrize("d", [64, 128])
def test_poison_beyond_the_length_never_enters_the_contiguous_result(d):
    K8, V8, kd, vd, Kf, Vf, (Kd, Vd, kdd, vdd, ld) = contiguous_case(d)
    B, Hkv, G, Sq = K8.shape[0], 2, 4, 3
    Q = randn((B, G * Hkv, Sq, d), 600, torch.bfloat16).to(DEV)
    Kc, Vc, Kx, Vx = K8.clone(), V8.clone(), K8.clone(), V8.clone()
    for b, L in enumerate(LENS):
        Kc[b, :, L:], Vc[b, :, L:] = 0, 0
        Kx[b, :, L:], Vx[b, :, L:] = poison(Kx[b, :, L:], 601 + b), poison(Vx[b, :, L:], 701 + b)
    assert int(((Kx & 0x7F) == 0x7F).sum()) and int(((Vx & 0x7F) == 0x7F).sum())
    for causal in (False, True):
        for splits in (0, 1, 3, CAP):
            kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, k_descale=kdd, v_descale=vdd)
            clean = fa.flash_attention_decode(Q, f8(Kc.to(DEV)), f8(Vc.to(DEV)), ld, **kw)
            dirty = fa.flash_attention_decode(Q, f8(Kx.to(DEV)), f8(Vx.to(DEV)), ld, **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(dirty[0]).all() and torch.isfinite(dirty[1]).all(), (causal, splits)
            assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1]), (causal, splits)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [16, 128])
def test_poison_in_unused_rows_and_pages_and_bad_unused_entries_never_enter_the_paged_result(page, d):
    Hkv, G, Sq, n = 2, 4, 3, max_pages_of(page)
    cap = n * page
    lens = [1, page + 1, cap - page - 3, cap - 3]      # a last page half full; whole pages unused behind it
    B = len(lens)
    P = B * n + 3
    Kp, kd = quantise(randn((P, Hkv, page, d), 61 + page, F32))
    Vp, vd = quantise(randn((P, Hkv, page, d), 62 + page, F32))
    g = torch.Generator().manual_seed(63 + page)
    table = (1 + torch.randperm(B * n, generator=g)).reshape(B, n).to(torch.int32)     # pages 1 .. B n; 0, P - 2, P - 1 are named by nobody
    used = [-(-L // page) for L in lens]
    Kx, Vx, bad_table = Kp.clone(), Vp.clone(), table.clone()
    bad = [-1, 2 ** 31 - 1, P]
    for b, L in enumerate(lens):
        last, r = int(table[b, used[b] - 1]), L - (used[b] - 1) * page
        Kp[last, :, r:], Vp[last, :, r:] = 0, 0
        Kx[last, :, r:], Vx[last, :, r:] = poison(Kx[last, :, r:], 64 + b), poison(Vx[last, :, r:], 74 + b)
        for j in range(used[b], n):
            pg = int(table[b, j])
            Kx[pg], Vx[pg] = poison(Kx[pg], 84 + j), poison(Vx[pg], 94 + j)          # pages not named any more
            bad_table[b, j] = bad[(b + j) % 3]
            table[b, j] = 0 if (b + j) % 2 else P - 1                                   # valid pages, full of poison
    for pg in (0, P - 2, P - 1):
        Kx[pg], Vx[pg] = poison(Kx[pg], 104 + pg), poison(Vx[pg], 114 + pg)
    assert int((bad_table < 0).sum()) and int((bad_table >= P).sum())
    Q = randn((B, G * Hkv, Sq, d), 64, torch.bfloat16)
    Qd, kdd, vdd, ld = Q.to(DEV), kd.to(DEV), vd.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    dev = lambda t: t.to(DEV)
    for causal in (False, True):
        for splits in (0, 1, 3, CAP):
            kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, k_descale=kdd, v_descale=vdd)
            clean = fa.flash_attention_decode_paged(Qd, f8(dev(Kp)), f8(dev(Vp)), dev(table), ld, **kw)
            torch.cuda.synchronize()
            for tb in (table, bad_table):
                dirty = fa.flash_attention_decode_paged(Qd, f8(dev(Kx)), f8(dev(Vx)), dev(tb), ld, **kw)
                torch.cuda.synchronize()
                assert torch.isfinite(dirty[0]).all() and torch.isfinite(dirty[1]).all(), (causal, splits)
                assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1]), (causal, splits)
    tb = table.clone()
    for b in range(B):
        tb[b, used[b]:] = 1
    refO, refL = reference(Q, dequantise(gather(Kp, tb), kd), dequantise(gather(Vp, tb), vd), lens, True)
    assert_close(*clean, refO, refL, f"poison case, clean, page {page} d {d}")


# ---- 6. layouts ----
@pytest.mark.parametrize("d", [64, 128])
def test_sequence_major_cache_view_and_a_row_stride_larger_than_d(d):
    B, Hkv, G, Sq, cap = 3, 2, 4, 3, 333
    K8, kd = quantise(randn((B, Hkv, cap, d), 800, F32))
    V8, vd = quantise(randn((B, Hkv, cap, d), 801, F32))
    lens = [cap, 130, 17]
    Q = randn((B, G * Hkv, Sq, d), 802, torch.bfloat16)
    Kd, Vd, kdd, vdd, Qd = (t.to(DEV) for t in (K8, V8, kd, vd, Q))
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(is_causal=True, out_dtype=torch.float32, return_lse=True, k_descale=kdd, v_descale=vdd)
    want = fa.flash_attention_decode(Qd, f8(Kd), f8(Vd), ld, **kw)
    assert_close(*want, *reference(Q, dequantise(K8, kd), dequantise(V8, vd), lens, True), f"dense, d {d}")
    # [B, S, Hkv, d] storage
    Ks, Vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (Kd, Vd))
    assert not Ks.is_contiguous() and Ks.stride(2) == Hkv * d
    # rows of d + 16 and d + 48 bytes: strides that are multiples of 16 and not of d
    Kw = torch.full((B, Hkv, cap, d + 16), 0x7F, dtype=torch.uint8, device=DEV)
    Vw = torch.full((B, Hkv, cap, d + 48), 0xFF, dtype=torch.uint8, device=DEV)
    Kw[..., :d], Vw[..., :d] = Kd, Vd
    for K, V in ((Ks, Vs), (Kw[..., :d], Vw[..., :d])):
        got = fa.flash_attention_decode(Qd, f8(K), f8(V), ld, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [16, 128])
def test_page_major_pool_view_a_wider_table_and_a_wide_row_stride(page, d):
    Hkv, G, Sq, n = 2, 4, 3, max_pages_of(page)
    B, P = 3, 3 * n + 5
    Kp, kd = quantise(randn((P, Hkv, page, d), 81, F32))
    Vp, vd = quantise(randn((P, Hkv, page, d), 82, F32))
    g = torch.Generator().manual_seed(83)
    wide = torch.full((B, n + 6), -7, dtype=torch.int32)
    wide[:, 2:2 + n] = torch.randperm(P, generator=g)[:B * n].reshape(B, n).to(torch.int32)
    wide = wide.to(DEV)
    table = wide[:, 2:2 + n]
    assert table.stride(0) == n + 6 and not table.is_contiguous()
    lens = [n * page, page + 1, n * page - page + 2]
    Q = randn((B, G * Hkv, Sq, d), 84, torch.bfloat16)
    Kd, Vd, kdd, vdd, Qd = (t.to(DEV) for t in (Kp, Vp, kd, vd, Q))
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(is_causal=True, out_dtype=torch.float32, return_lse=True, k_descale=kdd, v_descale=vdd)
    want = fa.flash_attention_decode_paged(Qd, f8(Kd), f8(Vd), table.contiguous(), ld, **kw)
    refO, refL = reference(Q, dequantise(gather(Kp, table.cpu()), kd), dequantise(gather(Vp, table.cpu()), vd), lens, True)
    assert_close(*want, refO, refL, f"dense pool, page {page} d {d}")
    # [P, page, Hkv, d] storage; rows of d + 32 bytes
    Ks, Vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (Kd, Vd))
    assert not Ks.is_contiguous() and Ks.stride(2) == Hkv * d
    Kw = torch.full((P, Hkv, page, d + 32), 0xFF, dtype=torch.uint8, device=DEV)
    Vw = torch.full((P, Hkv, page, d + 32), 0x7F, dtype=torch.uint8, device=DEV)
    Kw[..., :d], Vw[..., :d] = Kd, Vd
    for K, V in ((Ks, Vs), (Kw[..., :d], Vw[..., :d])):
        got = fa.flash_attention_decode_paged(Qd, f8(K), f8(V), table, ld, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 7. byte arithmetic at size ----
def heavy_keys(Q, kd_head, factor=6.0):
    """bytes of a key that lines up with the last query row of every head: the softmax mass goes where it is stored"""
    key = Q[0, :, -1].float().mean(0) * factor
    return (key / kd_head).clamp(-448, 448).to(F8).view(torch.uint8)


@pytest.mark.parametrize("d", [64, 128])
def test_a_pool_above_two_to_the_32_bytes(d):
    """Page bases are 64-bit and counted at one byte per element: a sequence whose table names pages on both sides of byte 2^32 of
    each pool, with its softmax mass on a page above it.  Other data lies where a base wrapped to 32 bits, a base counted at two
    bytes per element, or both, would land"""
    Hkv, page, G, Sq = 1, 256, 4, 2
    page_bytes = page * d
    wrap = (1 << 32) // page_bytes                 # the page that starts at byte 2^32: 131 072 at d = 128
    P = wrap + 64
    assert P * page_bytes > (1 << 32) and (P - 64) * page_bytes <= (1 << 32)
    Kp = torch.empty((P, Hkv, page, d), dtype=torch.uint8, device=DEV)
    Vp = torch.empty((P, Hkv, page, d), dtype=torch.uint8, device=DEV)
    pages = [5, wrap + 9, wrap - 1, P - 1, wrap, 17]
    aliases = sorted({p - wrap for p in pages if p >= wrap} | {2 * p for p in pages if 2 * p < P}
                     | {2 * (p - wrap) for p in pages if p >= wrap})
    assert not set(aliases) & set(pages)
    Q = randn((1, G * Hkv, Sq, d), 101, torch.bfloat16)
    data = {}
    for j, pg in enumerate(pages + aliases):
        k8, _ = quantise(randn((1, Hkv, page, d), 110 + j, F32))
        v8, _ = quantise(randn((1, Hkv, page, d), 130 + j, F32))
        data[pg] = (k8[0], v8[0])
    kd, vd = torch.tensor([4.5 / 448]), torch.tensor([4.25 / 448])
    data[P - 1][0][0, 40:44] = heavy_keys(Q, kd[0])            # the mass: on page P - 1, the fourth of the sequence
    for pg, (k8, v8) in data.items():
        Kp[pg], Vp[pg] = k8.to(DEV), v8.to(DEV)
    L = 5 * page + 77
    Kg = torch.stack([data[pg][0] for pg in pages], 1).reshape(1, Hkv, len(pages) * page, d)
    Vg = torch.stack([data[pg][1] for pg in pages], 1).reshape(1, Hkv, len(pages) * page, d)
    Kf, Vf = dequantise(Kg, kd), dequantise(Vg, vd)
    refO, refL = reference(Q, Kf, Vf, [L], True)
    w = torch.softmax((Q[0].double() @ Kf[0, 0, :L].T)[:, -1] / d ** 0.5, -1)
    assert (w[:, 3 * page:4 * page].sum(-1) > 0.5).all()           # (most of the last row's weight lies above byte 2^32)
    table = torch.tensor([pages], dtype=torch.int32, device=DEV)
    ld = torch.tensor([L], dtype=torch.int32, device=DEV)
    for splits in (0, 1):
        O, lse = fa.flash_attention_decode_paged(Q.to(DEV), f8(Kp), f8(Vp), table, ld, is_causal=True, out_dtype=torch.float32,
                                                 num_splits=splits, return_lse=True, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
        torch.cuda.synchronize()
        assert_close(O, lse, refO, refL, f"pool of {P * page_bytes / 2 ** 30:.3f} GiB, d {d}, splits {splits}")


@pytest.mark.parametrize("d", [64, 128])
def test_a_head_extent_between_two_to_the_30_and_two_to_the_31_bytes(d):
    """1536 keys in rows 2^20 bytes apart: (1536 + 192) x 2^20 bytes, which the bf16 call refuses and a byte count doubled in the
    kernel would misplace.  The mass sits on the last keys, beyond byte 2^30"""
    Hkv, G, Sq, cap, stride = 1, 4, 2, 1536, 1 << 20
    K8, _ = quantise(randn((1, Hkv, cap, d), 900, F32))
    V8, _ = quantise(randn((1, Hkv, cap, d), 901, F32))
    kd, vd = torch.tensor([4.5 / 448]), torch.tensor([4.25 / 448])
    Q = randn((1, G * Hkv, Sq, d), 902, torch.bfloat16)
    K8[0, 0, cap - 4:] = heavy_keys(Q, kd[0])
    Kf, Vf = dequantise(K8, kd), dequantise(V8, vd)
    w = torch.softmax((Q[0].double() @ Kf[0, 0].T)[:, -1] / d ** 0.5, -1)
    assert (w[:, cap - 4:].sum(-1) > 0.5).all() and (cap - 4) * stride > (1 << 30) and (cap + 192) * stride < (1 << 31)
    views = []
    for t in (K8, V8):
        store = torch.empty((1, Hkv, cap, stride), dtype=torch.uint8, device=DEV)
        store[..., :d] = t.to(DEV)
        store[..., d:2 * d] = 0x7F       # what follows a row is not a row
        views.append(store[..., :d])
    for causal in (False, True):
        refO, refL = reference(Q, Kf, Vf, None, causal)
        for splits in (0, 1):
            O, lse = fa.flash_attention_decode(Q.to(DEV), f8(views[0]), f8(views[1]), None, is_causal=causal, out_dtype=torch.float32,
                                               num_splits=splits, return_lse=True, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
            torch.cuda.synchronize()
            assert_close(O, lse, refO, refL, f"head extent {(cap + 192) * stride / 2 ** 30:.2f} GiB, d {d}, causal {causal}, splits {splits}")


# ---- 8. determinism, a side stream ----
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_two_runs_give_the_same_bits_and_a_side_stream_keeps_its_workspace(d, paged):
    B, H, Hkv, Sq, page, n = 4, 32, 8, 4, 128, 64
    P = B * n
    g = torch.Generator().manual_seed(95 + d)
    Kp = torch.randint(0, 0x78, (P, Hkv, page, d), generator=g, dtype=torch.uint8).to(DEV)       # finite, positive bytes ...
    Vp = (torch.randint(0, 0x78, (P, Hkv, page, d), generator=g, dtype=torch.uint8) | 0x80 * (torch.arange(d) % 2).to(torch.uint8)).to(DEV)
    kdd, vdd = torch.full((Hkv,), 1 / 64, device=DEV), torch.full((Hkv,), 1 / 32, device=DEV)
    Q = randn((B, H, Sq, d), 97, torch.bfloat16).to(DEV)
    td = torch.randperm(P, generator=g).reshape(B, n).to(torch.int32).to(DEV)
    if paged:
        call = lambda **kw: fa.flash_attention_decode_paged(Q, f8(Kp), f8(Vp), td, out_dtype=torch.float32, k_descale=kdd, v_descale=vdd, **kw)
    else:
        Kc, Vc = gather(Kp, td), gather(Vp, td)
        call = lambda **kw: fa.flash_attention_decode(Q, f8(Kc), f8(Vc), out_dtype=torch.float32, k_descale=kdd, v_descale=vdd, **kw)
    ns = fa.decode_plan(B, H, Hkv, Sq, n * page, d, fa.FA_DTYPE_F32)["num_splits"]
    nbytes = fa.decode_workspace_size(B, H, Sq, d, ns)
    assert ns > 1 and nbytes > 0
    ref = call()
    again = call()
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and torch.equal(ref, again)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        got = call(stream=side)
        junk = [torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV) for _ in range(4)]   # NaN bytes, on the current stream
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
        del junk, got
