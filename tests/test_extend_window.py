"""GPU tests of windowed chunked prefill (flash_attention_extend_window / flash_attention_extend_paged_window, the Python fronts and the
C entry points of those names) over all four cache forms: contiguous / paged x bf16 / fp8.

Criterion: kv_cache_check.assert_close against kv_cache_check.reference (float64 explicit softmax over the keys
kv_cache_check.visible lets each row see) -- every element of the fp32 O within 1e-3 + 1e-3 |ref|, the LSE within 2e-4 + 2e-6 |ref|.
Capacity 640 = five 128-key tiles, H = 8 / Hkv = 2 plus G = 1 cases, one sequence per length.  Beside parity: the per-row-block tile
start (single softmax weights on both sides of a row's left edge in every row block; poison below first(b) and beyond the length), the
seams bit for bit (decode for Sq <= 16; the un-windowed call for no window and a window no shorter than the capacity; paged against
contiguous), pages wholly below first(b) behind out-of-range table entries, fp8 against the dequantised reference, output types, the
LSE on and off, and run-to-run determinism."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from extend_window_check import block_range  # noqa: E402
from kv_cache_check import (DEV, F8, assert_close, dequantise, first_visible, gather, i32 as dev_lens, poisoned_nan_inf, quantise,  # noqa: E402
                            randn, random_table, reference, scatter)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CAPACITY, TILE = 640, 128
H, HKV = 8, 2
SQS = (17, 40, 64, 65, 130, 200)
WINDOWS = (1, 16, 17, 127, 128, 129, 300, 640)
SPLITS = (0, 1, 2, 3, 5)          # 0: the library's choice; 5: more than most windows here have tiles, so some splits are empty
NAN = float("nan")
BMAX = 6


def lengths(W, Sq):
    """one sequence per length: fewer keys than query rows, as many, the window behind the chunk, around tile starts, the capacity"""
    return sorted({min(max(L, 1), CAPACITY) for L in (Sq - 3, Sq, Sq + W, 257, 511, 640)})


@functools.lru_cache(maxsize=None)
def cache(d, hkv=HKV):
    """(K, V) on the CPU, [BMAX, hkv, CAPACITY, d] bf16: the tests use the first B sequences"""
    return randn((BMAX, hkv, CAPACITY, d), 8100 + d + hkv, BF16), randn((BMAX, hkv, CAPACITY, d), 8200 + d + hkv, BF16)


@functools.lru_cache(maxsize=None)
def device_cache(d, hkv=HKV):
    K, V = cache(d, hkv)
    return K.to(DEV), V.to(DEV)


@functools.lru_cache(maxsize=None)
def fp8_cache(d):
    """(K bytes, V bytes, k_descale, v_descale) on the CPU: the bf16 cache quantised per K/V head"""
    K, V = cache(d)
    (K8, kd), (V8, vd) = quantise(K.float()), quantise(V.float())
    return K8, V8, kd, vd


def queries(B, Sq, d, heads=H):
    return randn((B, heads, Sq, d), 8300 + 16 * Sq + d + heads, BF16)


def run(Q, K, V, ld, **kw):
    O, lse = fa.flash_attention_extend_window(Q, K, V, ld, out_dtype=torch.float32, return_lse=True, **kw)
    torch.cuda.synchronize()
    return O, lse


def run_paged(Q, Kp, Vp, table, ld, **kw):
    O, lse = fa.flash_attention_extend_paged_window(Q, Kp, Vp, table, ld, out_dtype=torch.float32, return_lse=True, **kw)
    torch.cuda.synchronize()
    return O, lse


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 1. parity ----
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Sq", SQS)
@pytest.mark.parametrize("d", [64, 128])
def test_parity_against_float64(d, Sq, causal):
    K, V = cache(d)
    Kd, Vd = device_cache(d)
    for W in WINDOWS:
        lens = lengths(W, Sq)
        B = len(lens)
        assert B <= BMAX
        Q = queries(B, Sq, d)
        refO, refL = reference(Q, K[:B], V[:B], lens, causal, W)
        Qd, ld = Q.to(DEV), dev_lens(lens)
        for splits in SPLITS:
            O, lse = run(Qd, Kd[:B], Vd[:B], ld, is_causal=causal, num_splits=splits, window=W)
            assert_close(O, lse, refO, refL, f"d {d} Sq {Sq} causal {causal} W {W} splits {splits} lens {lens}")


@pytest.mark.parametrize("d", [64, 128])
def test_parity_with_one_query_head_per_kv_head(d):
    """G = 1: a row block never reaches into a next head before the last one"""
    K, V = cache(d)
    Kd, Vd = device_cache(d)
    for Sq in (65, 200):
        for W in (17, 100, 300):
            lens = lengths(W, Sq)
            B = len(lens)
            Q = queries(B, Sq, d, HKV)
            Qd, ld = Q.to(DEV), dev_lens(lens)
            for causal in (False, True):
                refO, refL = reference(Q, K[:B], V[:B], lens, causal, W)
                for splits in SPLITS:
                    O, lse = run(Qd, Kd[:B], Vd[:B], ld, is_causal=causal, num_splits=splits, window=W)
                    assert_close(O, lse, refO, refL, f"G 1 d {d} Sq {Sq} causal {causal} W {W} splits {splits}")


# ---- 2. the per-row-block tile start ----
BLOCK_CASES = [(1, 200, 640, 100), (4, 130, 600, 100)]       # (G, Sq, L, W)


@pytest.mark.parametrize("G,Sq,L,W", BLOCK_CASES)
@pytest.mark.parametrize("d", [64, 128])
def test_single_weights_on_both_sides_of_the_left_edge_in_every_row_block(d, G, Sq, L, W):
    """V is one-hot over d consecutive keys that straddle lo_i: O[i, j] is the single weight of the pair (row i, key w0 + j) -- exactly
    0.0 for a hidden key, > 0 and within the bound of the reference for a visible one.  Rows 0, 63, 64, 65 and Sq - 1 lie in
    different row blocks, whose tile ranges start at different tiles"""
    heads = HKV * G
    rpb = fa.extend_plan(1, heads, HKV, Sq, CAPACITY, d, window=W)["rows_per_block"]
    starts = {block_range(rpb, G, Sq, L, W, True, rb)[0] for rb in range(-(-G * Sq // rpb))}
    assert len(starts) > 1, "the blocks of this case start at different tiles"
    K, _ = cache(d)
    Kd, _ = device_cache(d)
    Q = queries(1, Sq, d, heads)
    Qd, ld = Q.to(DEV), dev_lens([L])
    for i in (0, 63, 64, 65, Sq - 1):
        limc = max(L - Sq + i + 1, 1)
        lo = max(limc - W, 0)
        w0 = lo - d // 2
        assert w0 >= 0 and w0 + d <= CAPACITY
        V = torch.zeros((1, HKV, CAPACITY, d), dtype=BF16)
        V[0, :, w0 + torch.arange(d), torch.arange(d)] = 1.0
        Vd = V.to(DEV)
        for causal in (False, True):
            refO, refL = reference(Q, K[:1], V, [L], causal, W)
            keys = torch.arange(w0, w0 + d)
            hidden = (keys < lo) | (keys >= (limc if causal else L))
            assert hidden[:d // 2].all() and not hidden[d // 2] and (refO[0, :, i, hidden] == 0).all() and (refO[0, :, i, ~hidden] > 0).all()
            for splits in SPLITS:
                O, lse = run(Qd, Kd[:1], Vd, ld, is_causal=causal, num_splits=splits, window=W)
                assert (O[0, :, i, hidden.to(DEV)] == 0.0).all(), (i, causal, splits)
                assert (O[0, :, i, (~hidden).to(DEV)] > 0.0).all(), (i, causal, splits)
                assert_close(O, lse, refO, refL, f"pairs: d {d} G {G} Sq {Sq} W {W} L {L} row {i} causal {causal} splits {splits}")


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("d", [64, 128])
def test_poison_below_first_and_beyond_the_length_never_enters_the_result(d, kv):
    """NaN / inf (fp8: the NaN bytes 0x7F / 0xFF) in every key below first(b) = lo_0 and at and beyond the length: not a bit changes.
    The cases include the two of the per-block starts"""
    fp8 = kv == "fp8"
    if fp8:
        K8, V8, kd, vd = fp8_cache(d)
        K, V = K8.to(DEV), V8.to(DEV)
        extra = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    else:
        K, V = device_cache(d)
        extra = {}
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t)
    for heads, Sq, W, lens in ((HKV, 200, 100, [640, 500, 203]), (H, 130, 100, [640, 387, 259]), (H, 17, 1, lengths(1, 17)),
                               (H, 65, 128, lengths(128, 65)), (H, 40, 300, lengths(300, 40))):
        firsts = [first_visible(L, Sq, W) for L in lens]
        assert any(f > 0 for f in firsts)
        B, ld = len(lens), dev_lens(lens)
        Kp, Vp = poisoned_nan_inf(K[:B], V[:B], lens, firsts, fp8)
        Qd = queries(B, Sq, d, heads).to(DEV)
        for causal in (False, True):
            for splits in (0, 1, 3, 5):
                kw = dict(is_causal=causal, num_splits=splits, window=W, **extra)
                clean = run(Qd, view(K[:B]), view(V[:B]), ld, **kw)
                got = run(Qd, view(Kp), view(Vp), ld, **kw)
                assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), (Sq, W, causal, splits)
                assert same(got, clean), (Sq, W, causal, splits)


# ---- 3. seams ----
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("G", [1, 4, 16])
@pytest.mark.parametrize("d", [64, 128])
def test_up_to_sixteen_rows_the_result_is_decodes_bit_for_bit(d, G, kv):
    heads = HKV * G
    if kv == "fp8":
        K8, V8, kd, vd = fp8_cache(d)
        K, V = K8.to(DEV).view(F8), V8.to(DEV).view(F8)
        extra = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    else:
        (K, V), extra = device_cache(d), {}
    lens = [1, 9, 130, 257, 511, 640]
    B, ld = len(lens), dev_lens(lens)
    for Sq in (1, 5, 16):
        Qd = queries(B, Sq, d, heads).to(DEV)
        for W in (7, 130):
            for causal in (False, True):
                for splits in (1, 3):
                    kw = dict(is_causal=causal, num_splits=splits, window=W, out_dtype=torch.float32, return_lse=True, **extra)
                    got = fa.flash_attention_extend_window(Qd, K[:B], V[:B], ld, **kw)
                    want = fa.flash_attention_decode(Qd, K[:B], V[:B], ld, **kw)
                    torch.cuda.synchronize()
                    assert same(got, want), (Sq, W, causal, splits)


@pytest.mark.parametrize("d", [64, 128])
def test_no_window_and_a_window_no_shorter_than_the_capacity_are_the_unwindowed_call(d):
    Kd, Vd = device_cache(d)
    lens = [1, 127, 129, 300, 639, 640]
    B, ld = len(lens), dev_lens(lens)
    for Sq in (5, 17, 65, 200):
        Qd = queries(B, Sq, d).to(DEV)
        for causal in (False, True):
            for splits in (0, 1, 3):
                kw = dict(is_causal=causal, num_splits=splits)
                plain = fa.flash_attention_extend(Qd, Kd[:B], Vd[:B], ld, out_dtype=torch.float32, return_lse=True, **kw)
                for W in (None, 0, CAPACITY, CAPACITY + 1, 1 << 20):
                    assert same(run(Qd, Kd[:B], Vd[:B], ld, window=W, **kw), plain), (Sq, causal, splits, W)


# ---- 4. the four cache forms ----
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("page", [16, 64, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_is_contiguous_and_pages_below_first_are_never_read(d, page, kv):
    """paged equals contiguous on the gathered copy; every page wholly below first(b) holds NaN behind a table entry nobody can
    follow (-1, 2^31 - 1, P + 5): bit-equal to the clean run"""
    if kv == "bf16":
        K, V = device_cache(d)
        extra, nan = {}, NAN
    else:
        K8, V8, kd, vd = fp8_cache(d)
        K, V = K8.to(DEV), V8.to(DEV)
        extra, nan = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)), 0x7F
    view = (lambda t: t) if kv == "bf16" else (lambda t: t.view(F8))
    n = CAPACITY // page
    for Sq, W in ((17, 17), (65, 128), (130, 100), (200, 1)):
        lens = lengths(W, Sq)
        firsts = [first_visible(L, Sq, W) for L in lens]
        B, ld = len(lens), dev_lens(lens)
        P = B * n + 5
        table = random_table(B, n, 8400 + page + W).to(DEV)
        Kp, Vp = scatter(K[:B], table, page), scatter(V[:B], table, page)
        assert torch.equal(gather(Kp, table), K[:B])
        Kn, Vn = Kp.clone(), Vp.clone()
        below = torch.zeros((B, n), dtype=torch.bool)
        for b, f in enumerate(firsts):
            below[b, :f // page] = True
        assert below.any()
        below = below.to(DEV)
        Kn[table[below].long()], Vn[table[below].long()] = nan, nan
        tables = [torch.where(below, torch.full_like(table, bad), table) for bad in (-1, 2 ** 31 - 1, P + 5)]
        Qd = queries(B, Sq, d).to(DEV)
        for causal in (False, True):
            for splits in (0, 1, 3):
                kw = dict(is_causal=causal, num_splits=splits, window=W, **extra)
                clean = run_paged(Qd, view(Kp), view(Vp), table, ld, **kw)
                assert same(clean, run(Qd, view(K[:B]), view(V[:B]), ld, **kw)), (Sq, W, causal, splits)
                for t in tables:
                    got = run_paged(Qd, view(Kn), view(Vn), t, ld, **kw)
                    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), (Sq, W, causal, splits, int(t.min()), int(t.max()))
                    assert same(got, clean), (Sq, W, causal, splits, int(t.min()), int(t.max()))


@pytest.mark.parametrize("descales", [True, False])
@pytest.mark.parametrize("d", [64, 128])
def test_fp8_against_the_dequantised_reference(d, descales):
    K8, V8, kd, vd = fp8_cache(d)
    ones = torch.ones(HKV)
    Kf, Vf = (dequantise(K8, kd), dequantise(V8, vd)) if descales else (dequantise(K8, ones), dequantise(V8, ones))
    extra = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)) if descales else {}
    scale = None if descales else 1e-3        # (the bytes taken at face value are large: a small softmax scale keeps the scores in range)
    Kd, Vd = K8.to(DEV).view(F8), V8.to(DEV).view(F8)
    n = CAPACITY // 64
    for Sq in (17, 65, 200):
        for W in (16, 129, 300):
            lens = lengths(W, Sq)
            B, ld = len(lens), dev_lens(lens)
            Q = queries(B, Sq, d)
            Qd = Q.to(DEV)
            table = random_table(B, n, 8500 + W).to(DEV)
            Kp, Vp = scatter(K8.to(DEV)[:B], table, 64).view(F8), scatter(V8.to(DEV)[:B], table, 64).view(F8)
            for causal in (False, True):
                refO, refL = reference(Q, Kf[:B], Vf[:B], lens, causal, W, scale=scale)
                for splits in (0, 1, 3):
                    kw = dict(is_causal=causal, num_splits=splits, window=W, scale=scale, **extra)
                    got = run(Qd, Kd[:B], Vd[:B], ld, **kw)
                    assert_close(*got, refO, refL, f"fp8 d {d} Sq {Sq} descales {descales} causal {causal} W {W} splits {splits}")
                    assert same(run_paged(Qd, Kp, Vp, table, ld, **kw), got), (W, causal, splits)


# ---- 5. outputs, determinism ----
@pytest.mark.parametrize("d", [64, 128])
def test_output_types_the_lse_and_two_runs(d):
    Sq, W = 130, 100
    lens = lengths(W, Sq)
    B, ld = len(lens), dev_lens(lens)
    Kd, Vd = device_cache(d)
    Qd = queries(B, Sq, d).to(DEV)
    for causal in (False, True):
        for splits in (0, 1, 3):
            kw = dict(is_causal=causal, num_splits=splits, window=W)
            O, lse = run(Qd, Kd[:B], Vd[:B], ld, **kw)
            assert same(run(Qd, Kd[:B], Vd[:B], ld, **kw), (O, lse)), "two runs differ"
            assert torch.equal(fa.flash_attention_extend_window(Qd, Kd[:B], Vd[:B], ld, out_dtype=torch.float32, **kw), O), "O depends on the LSE"
            # bf16 / fp16 output: the fp32 result of the same call rounded once; a caller's O is written in place
            for dt in (torch.bfloat16, torch.float16):
                Ol = fa.flash_attention_extend_window(Qd, Kd[:B], Vd[:B], ld, out_dtype=dt, **kw)
                assert Ol.dtype == dt and torch.equal(Ol, O.to(dt)), dt
            out = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
            assert fa.flash_attention_extend_window(Qd, Kd[:B], Vd[:B], ld, O=out, **kw) is out and torch.equal(out, O)
