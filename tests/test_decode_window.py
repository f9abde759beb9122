"""GPU tests of sliding-window decode (flash_attention_decode / flash_attention_decode_paged with window=W; the C entry points
flash_attention_decode_window and flash_attention_decode_paged_window) over all four cache forms: contiguous / paged x bf16 / fp8.

Criterion: kv_cache_check.assert_close against the float64 explicit softmax over the keys kv_cache_check.visible lets each
row see -- every element of the fp32 O within 1e-3 + 1e-3 |ref|, the LSE within 2e-4 + 2e-6 |ref|.  Capacity 640 = five 128-key
tiles, one sequence per length, lengths placed so that `first` (row 0's left edge: the lowest key any row sees) falls on, one before
and one after a tile start.  Beside parity: bitwise identities (no window, a window no shorter than the capacity, paged against
contiguous, run to run), single softmax weights on both sides of a row's left edge, poison below `first` (NaN / inf, fp8 NaN bytes,
NaN pages behind out-of-range table entries), layouts and output types, and graph replay with `first` moving across a tile start."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from kv_cache_check import (DEV, F8, assert_close, dequantise, first_visible, gather, i32 as dev_lens, poisoned_nan_inf, quantise,  # noqa: E402
                            randn, random_table, reference, scatter)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CAPACITY, TILE = 640, 128
H, HKV = 8, 2
WINDOWS = (1, 2, 15, 16, 17, 127, 128, 129, 300, 640)
SPLITS = (0, 1, 2, 3, 5, 8)          # 0: the library's choice; 8: more than any window here has tiles, so some splits are empty
NAN = float("nan")


def lengths(W, Sq):
    """one sequence per length: `first` on, one before and one after the starts of tiles 1 and 2 (where the capacity allows), fewer
    keys than query rows, one key, W and its neighbours, the capacity"""
    want = {f + W + Sq - 1 for f in (127, 128, 129, 255, 256, 257)} | {max(Sq - 1, 1), 1, W - 1, W, W + 1, CAPACITY}
    return sorted(L for L in want if 1 <= L <= CAPACITY)


BMAX = 12


@functools.lru_cache(maxsize=None)
def cache(d):
    """(K, V) on the CPU, [BMAX, HKV, CAPACITY, d] bf16: the tests use the first B sequences"""
    return randn((BMAX, HKV, CAPACITY, d), 7100 + d, BF16), randn((BMAX, HKV, CAPACITY, d), 7200 + d, BF16)


@functools.lru_cache(maxsize=None)
def device_cache(d):
    K, V = cache(d)
    return K.to(DEV), V.to(DEV)


@functools.lru_cache(maxsize=None)
def fp8_cache(d):
    """(K bytes, V bytes, k_descale, v_descale) on the CPU: the bf16 cache quantised per K/V head"""
    K, V = cache(d)
    (K8, kd), (V8, vd) = quantise(K.float()), quantise(V.float())
    return K8, V8, kd, vd


def queries(B, Sq, d):
    return randn((B, H, Sq, d), 7300 + 16 * Sq + d, BF16)


def run(Q, K, V, ld, **kw):
    O, lse = fa.flash_attention_decode(Q, K, V, ld, out_dtype=torch.float32, return_lse=True, **kw)
    torch.cuda.synchronize()
    return O, lse


def run_paged(Q, Kp, Vp, table, ld, **kw):
    O, lse = fa.flash_attention_decode_paged(Q, Kp, Vp, table, ld, out_dtype=torch.float32, return_lse=True, **kw)
    torch.cuda.synchronize()
    return O, lse


# ---- 1. boundary sweep ----
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Sq", [1, 3, 16])
@pytest.mark.parametrize("d", [64, 128])
def test_boundary_sweep_against_float64(d, Sq, causal):
    K, V = cache(d)
    Kd, Vd = device_cache(d)
    seen = set()
    for W in WINDOWS:
        lens = lengths(W, Sq)
        B = len(lens)
        assert B <= BMAX
        seen |= {first_visible(L, Sq, W) for L in lens}
        Q = queries(B, Sq, d)
        refO, refL = reference(Q, K[:B], V[:B], lens, causal, W)
        Qd, ld = Q.to(DEV), dev_lens(lens)
        for splits in SPLITS:
            O, lse = run(Qd, Kd[:B], Vd[:B], ld, is_causal=causal, num_splits=splits, window=W)
            assert_close(O, lse, refO, refL, f"d {d} Sq {Sq} causal {causal} W {W} splits {splits} lens {lens}")
    assert {127, 128, 129, 255, 256, 257} <= seen


# ---- 2. identities ----
@pytest.mark.parametrize("d", [64, 128])
def test_no_window_and_a_window_no_shorter_than_the_capacity_are_the_unwindowed_call(d):
    Kd, Vd = device_cache(d)
    lens = [1, 2, 127, 128, 129, 300, 639, 640]
    B, ld = len(lens), dev_lens(lens)
    for Sq in (1, 3, 16):
        Qd = queries(B, Sq, d).to(DEV)
        for causal in (False, True):
            for splits in SPLITS:
                kw = dict(is_causal=causal, num_splits=splits)
                plain = run(Qd, Kd[:B], Vd[:B], ld, **kw)
                for W in (None, 0, CAPACITY, CAPACITY + 1, 1 << 20):
                    O, lse = run(Qd, Kd[:B], Vd[:B], ld, window=W, **kw)
                    assert torch.equal(O, plain[0]) and torch.equal(lse, plain[1]), (Sq, causal, splits, W)


# ---- 3. single weights on both sides of a row's left edge ----
@pytest.mark.parametrize("Sq,W,L", [(3, 128, 300),       # lo_0 = 170, lo_2 = 172: one tile
                                    (16, 128, 263),      # first = lo_0 = 120 in tile 0, lo_15 = 135 in tile 1
                                    (16, 17, 400),       # lo_0 = 368, lo_15 = 383 in tile 2, 384 opens tile 3
                                    (3, 300, 640)])      # lo_0 = 338, lo_2 = 340; the sequence fills the capacity
@pytest.mark.parametrize("d", [64, 128])
def test_single_weights_on_both_sides_of_the_left_edge(d, Sq, W, L):
    """V is one-hot over d consecutive keys that straddle lo_i: O[i, j] is the single weight of the pair (row i, key w0 + j) -- exactly
    0.0 for a hidden key, within the bound of the reference for a visible one"""
    K, _ = cache(d)
    Kd, _ = device_cache(d)
    Q = queries(1, Sq, d)
    Qd, ld = Q.to(DEV), dev_lens([L])
    for i in (0, Sq - 1):
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
                assert_close(O, lse, refO, refL, f"pairs: d {d} Sq {Sq} W {W} L {L} row {i} causal {causal} splits {splits}")


# ---- 4. poison below the window: contiguous ----
POISON_W = (1, 17, 128, 300)
POISON_SPLITS = (0, 1, 3, 8)


def poison_case(W, Sq):
    lens = lengths(W, Sq)
    return lens, [first_visible(L, Sq, W) for L in lens]


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("d", [64, 128])
def test_poison_below_the_window_and_beyond_the_length_never_enters_the_result(d, kv):
    if kv == "bf16":
        K, V = device_cache(d)
        extra = {}
    else:
        K8, V8, kd, vd = fp8_cache(d)
        K, V = K8.to(DEV), V8.to(DEV)
        extra = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    view = (lambda t: t) if kv == "bf16" else (lambda t: t.view(F8))
    for Sq in (1, 3, 16):
        for W in POISON_W:
            lens, firsts = poison_case(W, Sq)
            B, ld = len(lens), dev_lens(lens)
            Kp, Vp = poisoned_nan_inf(K[:B], V[:B], lens, firsts, kv == "fp8")
            assert any(f > 0 for f in firsts)
            Qd = queries(B, Sq, d).to(DEV)
            for causal in (False, True):
                for splits in POISON_SPLITS:
                    kw = dict(is_causal=causal, num_splits=splits, window=W, **extra)
                    clean = run(Qd, view(K[:B]), view(V[:B]), ld, **kw)
                    O, lse = run(Qd, view(Kp), view(Vp), ld, **kw)
                    assert torch.isfinite(O).all() and torch.isfinite(lse).all(), (Sq, W, causal, splits)
                    assert torch.equal(O, clean[0]) and torch.equal(lse, clean[1]), (Sq, W, causal, splits)


# ---- 5. poison below the window: paged; the same bits as the contiguous path ----
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("page", [16, 64, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_pages_below_the_window_are_never_read_and_neither_are_their_table_entries(d, page, kv):
    if kv == "bf16":
        K, V = device_cache(d)
        extra, nan = {}, NAN
    else:
        K8, V8, kd, vd = fp8_cache(d)
        K, V = K8.to(DEV), V8.to(DEV)
        extra, nan = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)), 0x7F
    view = (lambda t: t) if kv == "bf16" else (lambda t: t.view(F8))
    n = CAPACITY // page
    for Sq, W in ((1, 17), (3, 128), (16, 1), (3, 300)):
        lens, firsts = poison_case(W, Sq)
        B, ld = len(lens), dev_lens(lens)
        P = B * n + 5
        table = random_table(B, n, 7400 + page + W).to(DEV)
        Kp, Vp = scatter(K[:B], table, page), scatter(V[:B], table, page)
        assert torch.equal(gather(Kp, table), K[:B])
        # every page wholly below first(b): NaN contents, and an entry nobody can follow
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
            for splits in POISON_SPLITS:
                kw = dict(is_causal=causal, num_splits=splits, window=W, **extra)
                clean = run_paged(Qd, view(Kp), view(Vp), table, ld, **kw)
                contiguous = run(Qd, view(K[:B]), view(V[:B]), ld, **kw)
                assert torch.equal(clean[0], contiguous[0]) and torch.equal(clean[1], contiguous[1]), (Sq, W, causal, splits)
                for t in tables:
                    O, lse = run_paged(Qd, view(Kn), view(Vn), t, ld, **kw)
                    assert torch.isfinite(O).all() and torch.isfinite(lse).all(), (Sq, W, causal, splits, int(t.min()), int(t.max()))
                    assert torch.equal(O, clean[0]) and torch.equal(lse, clean[1]), (Sq, W, causal, splits, int(t.min()), int(t.max()))


# ---- 6. fp8 caches against the dequantised reference ----
@pytest.mark.parametrize("descales", [True, False])
@pytest.mark.parametrize("Sq", [1, 3, 16])
@pytest.mark.parametrize("d", [64, 128])
def test_fp8_sweep_against_the_dequantised_reference(d, Sq, descales):
    K8, V8, kd, vd = fp8_cache(d)
    ones = torch.ones(HKV)
    Kf, Vf = (dequantise(K8, kd), dequantise(V8, vd)) if descales else (dequantise(K8, ones), dequantise(V8, ones))
    extra = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)) if descales else {}
    scale = None if descales else 1e-3        # (the bytes taken at face value are large: a small softmax scale keeps the scores in range)
    Kd, Vd = K8.to(DEV).view(F8), V8.to(DEV).view(F8)
    n = CAPACITY // 64
    for W in POISON_W:
        lens = lengths(W, Sq)
        B, ld = len(lens), dev_lens(lens)
        Q = queries(B, Sq, d)
        Qd = Q.to(DEV)
        table = random_table(B, n, 7500 + W).to(DEV)
        Kp, Vp = scatter(K8.to(DEV)[:B], table, 64).view(F8), scatter(V8.to(DEV)[:B], table, 64).view(F8)
        for causal in (False, True):
            refO, refL = reference(Q, Kf[:B], Vf[:B], lens, causal, W, scale=scale)
            for splits in SPLITS:
                kw = dict(is_causal=causal, num_splits=splits, window=W, scale=scale, **extra)
                O, lse = run(Qd, Kd[:B], Vd[:B], ld, **kw)
                assert_close(O, lse, refO, refL, f"fp8 d {d} Sq {Sq} descales {descales} causal {causal} W {W} splits {splits}")
                Op, lsep = run_paged(Qd, Kp, Vp, table, ld, **kw)
                assert torch.equal(Op, O) and torch.equal(lsep, lse), (W, causal, splits)


# ---- 7. layouts and outputs ----
@pytest.mark.parametrize("d", [64, 128])
def test_a_strided_cache_and_every_output_type(d):
    Sq, W = 3, 128
    lens = lengths(W, Sq)
    B, ld = len(lens), dev_lens(lens)
    K, V = cache(d)
    Q = queries(B, Sq, d)
    Qd = Q.to(DEV)
    ks, vs = K[:B].transpose(1, 2).contiguous().to(DEV), V[:B].transpose(1, 2).contiguous().to(DEV)        # [B, S, Hkv, d] storage
    Kd, Vd = ks.transpose(1, 2), vs.transpose(1, 2)
    assert not Kd.is_contiguous() and Kd.shape == (B, HKV, CAPACITY, d)
    for causal in (False, True):
        refO, refL = reference(Q, K[:B], V[:B], lens, causal, W)
        for splits in (0, 1, 3):
            kw = dict(is_causal=causal, num_splits=splits, window=W)
            O, lse = run(Qd, Kd, Vd, ld, **kw)
            assert_close(O, lse, refO, refL, f"[B, S, Hkv, d] cache, d {d} causal {causal} splits {splits}")
            dense = run(Qd, Kd.contiguous(), Vd.contiguous(), ld, **kw)
            assert torch.equal(O, dense[0]) and torch.equal(lse, dense[1])
            # bf16 / fp16 output: the fp32 result of the same call rounded once; a caller's O is written in place
            for dt in (torch.bfloat16, torch.float16):
                Ol = fa.flash_attention_decode(Qd, Kd, Vd, ld, out_dtype=dt, **kw)
                assert Ol.dtype == dt and torch.equal(Ol, O.to(dt)), dt
            out = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
            assert fa.flash_attention_decode(Qd, Kd, Vd, ld, O=out, **kw) is out and torch.equal(out, O)


# ---- 8. graph replay, determinism ----
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_graph_replay_follows_the_lengths_as_first_crosses_a_tile_start(d, paged):
    """one captured call (a linear chain: split kernel, combine kernel), replayed as the sequences grow a key at a time: `first` of
    sequence 0 goes 127, 128, 129 -- the tile range starts one tile later from the second replay on"""
    Sq, W, splits, page = 1, 128, 2, 16
    K, V = cache(d)
    Kd, Vd = device_cache(d)
    lens = [254, 400, 639]
    B = len(lens)
    Q = queries(B, Sq, d)
    Qd, ld = Q.to(DEV), dev_lens(lens)
    if paged:
        n = CAPACITY // page
        table = random_table(B, n, 7600).to(DEV)
        Kp, Vp = scatter(Kd[:B], table, page), scatter(Vd[:B], table, page)
        call = lambda **kw: fa.flash_attention_decode_paged(Qd, Kp, Vp, table, ld, is_causal=True, num_splits=splits, window=W, **kw)
    else:
        call = lambda **kw: fa.flash_attention_decode(Qd, Kd[:B], Vd[:B], ld, is_causal=True, num_splits=splits, window=W, **kw)
    ws = torch.empty(fa.decode_workspace_size(B, H, Sq, d, splits), dtype=torch.uint8, device=DEV)
    O = torch.zeros((B, H, Sq, d), dtype=torch.float32, device=DEV)
    call(O=O, workspace=ws)                     # (first call outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(O=O, workspace=ws)
    firsts = []
    for step in range(4):
        ld += 1
        live = [L + step + 1 for L in lens[:2]] + [CAPACITY]      # (the library clamps a length beyond the capacity)
        firsts.append(first_visible(live[0], Sq, W))
        O.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = call(out_dtype=torch.float32)
        torch.cuda.synchronize()
        assert torch.equal(O, eager), step
        refO, _ = reference(Q, K[:B], V[:B], live, True, W)
        assert ((O.double().cpu() - refO).abs() <= 1e-3 + 1e-3 * refO.abs()).all(), step
    assert firsts == [127, 128, 129, 130]


@pytest.mark.parametrize("d", [64, 128])
def test_two_runs_give_the_same_bits(d):
    Kd, Vd = device_cache(d)
    Sq, W = 3, 300
    lens = lengths(W, Sq)
    B, ld = len(lens), dev_lens(lens)
    Qd = queries(B, Sq, d).to(DEV)
    for splits in (0, 3, 8):
        a = run(Qd, Kd[:B], Vd[:B], ld, is_causal=True, num_splits=splits, window=W)
        b = run(Qd, Kd[:B], Vd[:B], ld, is_causal=True, num_splits=splits, window=W)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), splits
