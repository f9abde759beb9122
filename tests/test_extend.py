"""GPU tests of flash_attention_extend / flash_attention_extend_paged: chunked prefill against the decode K/V caches, all four forms.
Reference, mask, criterion (1e-3 + 1e-3 |ref| on O, 2e-4 + 2e-6 |ref| on the LSE, every element) and the paged / fp8 data are those of
tests/kv_cache_check.py, the score-noise criterion of the scale cases included."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from kv_cache_check import (CAP, DEV, F8, SCALES, assert_close, assert_close_with_score_noise, dequantise, gather, i32, paged_layout,  # noqa: E402
                            quantise, randn, reference)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SPLITS = (0, 1, 2, 3, CAP)
# (G, Sq): packed rows g * Sq + i across 16, across rows_per_block, row blocks that straddle heads
SHAPES = [(1, 17), (4, 17), (8, 33), (1, 64), (2, 65), (4, 100), (1, 200), (8, 200)]
LENS_200 = (200, 201, 256, 257, 383, 384, 385, 700, 1024)   # at Sq = 200, capacity 1024; other Sq shift them (and the capacity) alike


def lens_of(Sq):
    return [L - 200 + Sq for L in LENS_200]


def dev(*ts):
    return [t.to(DEV) for t in ts]


@functools.lru_cache(maxsize=None)
def sweep_case(d, G, Sq):
    """(Q, K, V, lens) on the CPU and the two references (not causal, causal), computed once"""
    lens = lens_of(Sq)
    B, Hkv, cap = len(lens), 2, lens[-1]
    Q, K, V = randn((B, Hkv * G, Sq, d), 11 + Sq, BF16), randn((B, Hkv, cap, d), 12 + G, BF16), randn((B, Hkv, cap, d), 13 + d, BF16)
    return Q, K, V, lens, {c: reference(Q, K, V, lens, c) for c in (False, True)}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("G,Sq", SHAPES)
@pytest.mark.parametrize("d", [64, 128])
def test_parity_sweep(d, G, Sq, causal):
    Q, K, V, lens, refs = sweep_case(d, G, Sq)
    Qd, Kd, Vd = dev(Q, K, V)
    for splits in SPLITS:
        O, lse = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close(O, lse, *refs[causal], f"extend d {d} G {G} Sq {Sq} causal {causal} splits {splits}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_lengths_below_the_chunk(d, causal):
    """len < Sq: every row keeps key 0, nothing is NaN"""
    Sq, lens, cap, Hkv, G = 40, [1, 5, 39], 300, 2, 4
    Q, K, V = randn((3, Hkv * G, Sq, d), 21, BF16), randn((3, Hkv, cap, d), 22, BF16), randn((3, Hkv, cap, d), 23, BF16)
    ref = reference(Q, K, V, lens, causal)
    Qd, Kd, Vd = dev(Q, K, V)
    for splits in (0, 1, 3):
        O, lse = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close(O, lse, *ref, f"len < Sq, d {d} causal {causal} splits {splits}")
        if causal:   # rows 0 .. Sq - len see key 0 alone (weight 1, l = 1): O = V[0] exactly, for every length and split count
            first = V[:, :, 0].float().repeat_interleave(G, 1)      # [B, H, d]
            for b, L in enumerate(lens):
                n = Sq - L + 1
                assert torch.equal(O.cpu()[b, :, :n], first[b][:, None, :].expand(-1, n, -1)), (b, L, splits)


def paged_case(page, d, Sq, G, fp8):
    """paged_layout's pools and table with the lengths raised to at least 1 (any length is legal against Sq); the contiguous twin; the
    dequantised (or plain) K/V for the reference"""
    P, table, lens = paged_layout(page, d)
    Hkv = 2
    Kp, Vp = randn((P, Hkv, page, d), 1000 + page + d, torch.float32), randn((P, Hkv, page, d), 2000 + page + d, torch.float32)
    Q = randn((len(lens), Hkv * G, Sq, d), 31 + page, BF16)
    if fp8:
        (Kb, kd), (Vb, vd) = quantise(Kp), quantise(Vp)
        refK, refV = gather(dequantise(Kb, kd), table), gather(dequantise(Vb, vd), table)
        return Q, Kb, Vb, kd, vd, table, lens, refK, refV
    Kb, Vb = Kp.to(BF16), Vp.to(BF16)
    return Q, Kb, Vb, None, None, table, lens, gather(Kb, table), gather(Vb, table)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [16, 128, 256])
@pytest.mark.parametrize("d", [64, 128])
def test_all_four_cache_forms(d, page, fp8, causal):
    Sq, G = 50, 4
    Q, Kb, Vb, kd, vd, table, lens, refK, refV = paged_case(page, d, Sq, G, fp8)
    ref = reference(Q, refK, refV, lens, causal)
    view = (lambda t: t.view(F8)) if fp8 else (lambda t: t)
    Qd, Kp, Vp, td = dev(Q, Kb, Vb, table)
    Kc, Vc = gather(Kb, table).to(DEV), gather(Vb, table).to(DEV)
    ds = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)) if fp8 else {}
    # strided views of the same data: a [P, page, Hkv, d] pool, a [B, S, Hkv, d] cache
    Kps, Vps = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (Kp, Vp))
    Kcs, Vcs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (Kc, Vc))
    assert not Kps.is_contiguous() and not Kcs.is_contiguous()
    for splits in (0, 1, 3):
        kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, **ds)
        Op, lp = fa.flash_attention_extend_paged(Qd, view(Kp), view(Vp), td, i32(lens), **kw)
        Oc, lc = fa.flash_attention_extend(Qd, view(Kc), view(Vc), i32(lens), **kw)
        Ops, lps = fa.flash_attention_extend_paged(Qd, view(Kps), view(Vps), td, i32(lens), **kw)
        Ocs, lcs = fa.flash_attention_extend(Qd, view(Kcs), view(Vcs), i32(lens), **kw)
        torch.cuda.synchronize()
        assert_close(Op, lp, *ref, f"paged d {d} page {page} fp8 {fp8} causal {causal} splits {splits}")
        assert torch.equal(Op, Oc) and torch.equal(lp, lc), "paged != contiguous"
        assert torch.equal(Op, Ops) and torch.equal(lp, lps) and torch.equal(Oc, Ocs) and torch.equal(lc, lcs), "strided views"


@pytest.mark.parametrize("d", [64, 128])
def test_poison_beyond_the_length_contiguous(d):
    """NaN and 1e30 (bf16) / 0x7F bytes (fp8) at and beyond each length do not change a bit"""
    Q, K, V, lens, _ = sweep_case(d, 4, 100)
    Qd = Q.to(DEV)
    Kb, kd = quantise(K.float())
    Vb, vd = quantise(V.float())
    for fp8 in (False, True):
        Kc, Vc = (Kb.clone(), Vb.clone()) if fp8 else (K.clone(), V.clone())
        Kx, Vx = Kc.clone(), Vc.clone()
        for b, L in enumerate(lens):
            Kx[b, :, L:] = 0x7F if fp8 else float("nan")
            Vx[b, :, L:] = 0x7F if fp8 else 1e30
            if not fp8:
                Vx[b, :, L + 1::2] = float("nan")
        view = (lambda t: t.to(DEV).view(F8)) if fp8 else (lambda t: t.to(DEV))
        ds = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)) if fp8 else {}
        for causal in (False, True):
            for splits in (1, 3):
                kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, **ds)
                O, lse = fa.flash_attention_extend(Qd, view(Kc), view(Vc), i32(lens), **kw)
                Ox, lx = fa.flash_attention_extend(Qd, view(Kx), view(Vx), i32(lens), **kw)
                torch.cuda.synchronize()
                assert torch.isfinite(O).all()
                assert torch.equal(O, Ox) and torch.equal(lse, lx), (fp8, causal, splits)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [16, 128])
def test_poison_in_pages_and_table(page, fp8):
    """rows beyond the length, pages no sequence names, and table entries beyond the last visible page (any int32) are never read"""
    d, Sq, G = 128, 50, 2
    Q, Kb, Vb, kd, vd, table, lens, _, _ = paged_case(page, d, Sq, G, fp8)
    P, B, n = Kb.shape[0], *table.shape
    Kx, Vx, tx = Kb.clone(), Vb.clone(), table.clone()
    named = torch.zeros(P, dtype=torch.bool)
    for b, L in enumerate(lens):
        last = (L - 1) // page
        named[table[b, :last + 1].long()] = True
        tx[b, last + 1:] = torch.tensor([2 ** 31 - 1, -2 ** 31, P, -1] * n, dtype=torch.int32)[:n - last - 1]
    bad = 0x7F if fp8 else float("nan")
    for b, L in enumerate(lens):   # the tail of the last visible page (sequences share no pages here)
        last = (L - 1) // page
        Kx[table[b, last].long(), :, L - last * page:] = bad
        Vx[table[b, last].long(), :, L - last * page:] = bad if fp8 else 1e30
    Kx[~named], Vx[~named] = bad, bad
    view = (lambda t: t.to(DEV).view(F8)) if fp8 else (lambda t: t.to(DEV))
    ds = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV)) if fp8 else {}
    Qd = Q.to(DEV)
    for causal in (False, True):
        for splits in (1, 3):
            kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, **ds)
            O, lse = fa.flash_attention_extend_paged(Qd, view(Kb), view(Vb), table.to(DEV), i32(lens), **kw)
            Ox, lx = fa.flash_attention_extend_paged(Qd, view(Kx), view(Vx), tx.to(DEV), i32(lens), **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(O).all()
            assert torch.equal(O, Ox) and torch.equal(lse, lx), (causal, splits)


@pytest.mark.parametrize("G", [1, 4, 16])
@pytest.mark.parametrize("Sq", [1, 5, 16])
def test_seam_to_decode_bit_for_bit(Sq, G):
    """Sq <= FA_DECODE_MAX_Q: extend equals decode of the same arguments and forced num_splits, O and LSE, contiguous bf16 and paged fp8"""
    d, Hkv, page = 128, 2, 16
    lens = [Sq, 127, 128, 129, 700]
    B, n = len(lens), 48
    Q = randn((B, Hkv * G, Sq, d), 41 + Sq, BF16).to(DEV)
    K, V = randn((B, Hkv, n * page, d), 42, BF16), randn((B, Hkv, n * page, d), 43, BF16)
    P = B * n + 3
    table = torch.randperm(P, generator=torch.Generator().manual_seed(44))[:B * n].reshape(B, n).to(torch.int32)
    (Kb, kd), (Vb, vd) = quantise(randn((P, Hkv, page, d), 45, torch.float32)), quantise(randn((P, Hkv, page, d), 46, torch.float32))
    Kd, Vd, Kp, Vp, td = K.to(DEV), V.to(DEV), Kb.to(DEV).view(F8), Vb.to(DEV).view(F8), table.to(DEV)
    ds = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    for causal in (False, True):
        for splits in (1, 2, 5, CAP):
            kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True)
            got = fa.flash_attention_extend(Q, Kd, Vd, i32(lens), **kw) + fa.flash_attention_extend_paged(Q, Kp, Vp, td, i32(lens), **kw, **ds)
            want = fa.flash_attention_decode(Q, Kd, Vd, i32(lens), **kw) + fa.flash_attention_decode_paged(Q, Kp, Vp, td, i32(lens), **kw, **ds)
            torch.cuda.synchronize()
            for name, a, b in zip(("O", "LSE", "paged fp8 O", "paged fp8 LSE"), got, want):
                assert torch.equal(a, b), f"{name} differs from decode: Sq {Sq} G {G} causal {causal} splits {splits}, " \
                                          f"{int((a != b).sum())} elements, worst {(a - b).abs().max().item():.3e}"


def test_seam_to_prefill():
    """len == Sq, one length for the batch: the bottom-right and the top-left masks agree; both kernels meet the float64 criterion"""
    B, Hkv, G, Sq, d = 2, 2, 4, 256, 128
    Q, K, V = randn((B, Hkv * G, Sq, d), 51, BF16), randn((B, Hkv, Sq, d), 52, BF16), randn((B, Hkv, Sq, d), 53, BF16)
    ref = reference(Q, K, V, None, True)
    Qd, Kd, Vd = dev(Q, K, V)
    O, lse = fa.flash_attention_extend(Qd, Kd, Vd, None, is_causal=True, out_dtype=torch.float32, return_lse=True)
    Op, lp = fa.flash_attention(Qd, Kd, Vd, is_causal=True, out_dtype=torch.float32, return_lse=True)
    torch.cuda.synchronize()
    assert_close(O, lse, *ref, "extend, len == Sq")
    assert_close(Op, lp, *ref, "flash_attention (gqa), causal")


def test_chunked_prefill_then_decode_end_to_end():
    """3 chunks (96, 160, 64), each `kv_lens += chunk; kv_cache_append_paged; flash_attention_extend_paged` into a page-16 fp8 pool,
    then 2 decode steps; sequence 1 sits behind a cached prefix of 37 keys.  The chunk-64 step is a captured graph, replayed first on
    the two sequences swapped (lengths and table changed in place), then on the real state."""
    B, Hkv, G, d, page, n = 2, 2, 4, 128, 16, 24
    H, prefix, chunks = Hkv * G, [0, 37], [96, 160, 64, 1, 1]
    T, P = sum(chunks), B * n + 5
    Qa = randn((B, H, T, d), 61, BF16).to(DEV)
    Ka, Va = randn((B, Hkv, 37 + T, d), 62, BF16).to(DEV), randn((B, Hkv, 37 + T, d), 63, BF16).to(DEV)   # keys by position
    kd, vd = (Ka.float().abs().amax(dim=(0, 2, 3)) / 448).contiguous(), (Va.float().abs().amax(dim=(0, 2, 3)) / 448).contiguous()
    Kp, Vp = torch.zeros((P, Hkv, page, d), dtype=torch.uint8, device=DEV), torch.zeros((P, Hkv, page, d), dtype=torch.uint8, device=DEV)
    table = torch.randperm(P, generator=torch.Generator().manual_seed(64))[:B * n].reshape(B, n).to(torch.int32).to(DEV)
    lens = i32([0, 0])
    ds = dict(k_descale=kd, v_descale=vd)

    def new_rows(pos, c):   # the c new K/V rows of each sequence: positions prefix[b] + pos ..
        return [torch.stack([t[b, :, prefix[b] + pos:prefix[b] + pos + c] for b in range(B)]).contiguous() for t in (Ka, Va)]

    lens += i32(prefix)     # the cached prefix of sequence 1 (kv_lens 0: nothing is written for sequence 0)
    fa.kv_cache_append_paged(Ka[:, :, :37].contiguous(), Va[:, :, :37].contiguous(), Kp.view(F8), Vp.view(F8), table, lens, **ds)
    outs, pos = [], 0
    for c in chunks[:2]:
        lens += c
        Kn, Vn = new_rows(pos, c)
        fa.kv_cache_append_paged(Kn, Vn, Kp.view(F8), Vp.view(F8), table, lens, **ds)
        outs.append(fa.flash_attention_extend_paged(Qa[:, :, pos:pos + c].contiguous(), Kp.view(F8), Vp.view(F8), table, lens, is_causal=True,
                                                    out_dtype=torch.float32, **ds))
        pos += c
    # the chunk-64 step as a graph over static tensors
    c = chunks[2]
    Qs, (Kn, Vn) = Qa[:, :, pos:pos + c].contiguous(), new_rows(pos, c)
    Os = torch.empty((B, H, c, d), dtype=torch.float32, device=DEV)
    ws = torch.empty(fa.decode_workspace_size(B, H, c, d, 2), dtype=torch.uint8, device=DEV)
    # (every kernel of the step has run once before the capture: the two-split form and its combine here, into Os)
    fa.flash_attention_extend_paged(Qs, Kp.view(F8), Vp.view(F8), table, lens, is_causal=True, num_splits=2, O=Os, workspace=ws, **ds)
    torch.cuda.synchronize()
    saved = (Kp.clone(), Vp.clone(), lens.clone(), table.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lens += c
        fa.kv_cache_append_paged(Kn, Vn, Kp.view(F8), Vp.view(F8), table, lens, **ds)
        fa.flash_attention_extend_paged(Qs, Kp.view(F8), Vp.view(F8), table, lens, is_causal=True, num_splits=2, O=Os, workspace=ws, **ds)
    for t, s in zip((Kp, Vp, lens, table), saved):   # (capture runs nothing, but the state is restored the same way both times)
        t.copy_(s)
    # replay 1: the two sequences swapped -- lengths, table rows and inputs changed in place
    lens.copy_(saved[2].flip(0)); table.copy_(saved[3].flip(0))
    for t in (Qs, Kn, Vn):
        t.copy_(t.flip(0))
    graph.replay()
    swapped = Os.clone()
    # replay 2: the real state
    for t, s in zip((Kp, Vp, lens, table), saved):
        t.copy_(s)
    for t in (Qs, Kn, Vn):
        t.copy_(t.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(swapped.flip(0), Os), "the replayed graph did not follow the lengths and the table"
    outs.append(Os.clone())
    pos += c
    for c in chunks[3:]:
        lens += c
        Kn, Vn = new_rows(pos, c)
        fa.kv_cache_append_paged(Kn, Vn, Kp.view(F8), Vp.view(F8), table, lens, **ds)
        outs.append(fa.flash_attention_decode_paged(Qa[:, :, pos:pos + c].contiguous(), Kp.view(F8), Vp.view(F8), table, lens, is_causal=True,
                                                    out_dtype=torch.float32, **ds))
        pos += c
    torch.cuda.synchronize()
    final = [p + T for p in prefix]
    assert lens.tolist() == final
    K64, V64 = gather(dequantise(Kp.cpu(), kd.cpu()), table.cpu()), gather(dequantise(Vp.cpu(), vd.cpu()), table.cpu())
    refO, _ = reference(Qa.cpu(), K64, V64, final, True)
    O = torch.cat(outs, dim=2).double().cpu()
    err, tol = (O - refO).abs(), 1e-3 + 1e-3 * refO.abs()
    print(f"end to end: worst O error / tolerance {(err / tol).max().item():.3f}")
    assert torch.isfinite(O).all() and (err <= tol).all(), f"worst ratio {(err / tol).max().item():.3f}"


@pytest.mark.parametrize("splits", [1, 3])
def test_outputs_streams_and_determinism(splits):
    Q, K, V, lens, _ = sweep_case(128, 4, 100)
    Qd, Kd, Vd = dev(Q, K, V)
    kw = dict(is_causal=True, num_splits=splits)
    O32, lse = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), out_dtype=torch.float32, return_lse=True, **kw)
    again, lse2 = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), out_dtype=torch.float32, return_lse=True, **kw)
    no_lse = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), out_dtype=torch.float32, **kw)
    Ob = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), out_dtype=torch.bfloat16, **kw)
    Oh = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), out_dtype=torch.float16, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Oside, lside = fa.flash_attention_extend(Qd, Kd, Vd, i32(lens), out_dtype=torch.float32, return_lse=True, stream=side, **kw)
    side.synchronize()
    assert torch.equal(O32, again) and torch.equal(lse, lse2), "two runs differ"
    assert torch.equal(O32, no_lse), "O depends on whether the LSE was requested"
    assert torch.equal(O32, Oside) and torch.equal(lse, lside), "side stream"
    assert torch.equal(Ob, O32.to(torch.bfloat16)) and torch.equal(Oh, O32.to(torch.float16)), "not the fp32 result rounded once"


@pytest.mark.parametrize("kind", ["one", "boost3"])
@pytest.mark.parametrize("d", [64, 128])
def test_scale_cases(d, kind):
    """scale 1 (scores kept O(1)) and Q, K x 3, at Sq 64 and length 700: the criterion with the fp32 score-noise term"""
    scale, mul = SCALES[kind](d)
    B, Hkv, G, Sq, cap, lens = 2, 2, 4, 64, 1000, [700, 1000]
    Q, K, V = (randn((B, Hkv * G, Sq, d), 81, BF16) * mul).bfloat16(), (randn((B, Hkv, cap, d), 82, BF16) * mul).bfloat16(), randn((B, Hkv, cap, d), 83, BF16)
    for splits in (0, 1, 5):
        O, lse = fa.flash_attention_extend(*dev(Q, K, V), i32(lens), scale=scale, is_causal=True, out_dtype=torch.float32,
                                           num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close_with_score_noise(O, lse, Q, K, V, lens, True, scale, f"extend {kind} d {d} splits {splits}")
