"""GPU tests of the ragged call with a sliding window (flash_attention_extend_varlen_window / flash_attention_extend_paged_varlen_window,
the Python fronts and the C entry points of those names), all four cache forms.  Reference: kv_cache_check.reference_ragged (every
sequence as a batch of one); criterion: kv_cache_check.assert_close.  The seam carries most of the weight: a sequence's bits are those
of flash_attention_extend_window(window=W) on that sequence alone (and, up to 16 rows, flash_attention_decode(window=W)) under the same
forced splits."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from kv_cache_check import (DEV, F8, assert_close, cu_of, dequantise, first_visible, gather, i32, quantise, randn, random_table,  # noqa: E402
                            reference_ragged, scatter)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
HKV, G = 2, 4
H = HKV * G
CAPACITY = 640
# the mixed batch: decode rows, an idle slot, rows across 16 and across the row blocks of 32 / 64 packed rows
SQ = [1, 5, 0, 16, 17, 130, 200]
# mixed lengths around the 128-key tile seams; the idle slot's is garbage; sequence 5 fills the capacity
LENS = [129, 300, -77, 257, 511, 640, 600]
WINDOWS = (16, 100, 300)
PAD = 23                                        # totalQ = cu[-1] + PAD: rows no sequence owns
SENTINEL = -123456.75


@functools.lru_cache(maxsize=None)
def batch(d):
    """(Q [T, H, d], K, V [B, HKV, CAPACITY, d]) of the mixed batch on the CPU"""
    T = sum(SQ) + PAD
    return (randn((T, H, d), 9100 + d, BF16), randn((len(SQ), HKV, CAPACITY, d), 9200 + d, BF16),
            randn((len(SQ), HKV, CAPACITY, d), 9300 + d, BF16))


@functools.lru_cache(maxsize=None)
def references(d, fp8, causal, W):
    """the packed float64 reference (O, LSE, owned) of the batch against the bf16 cache or the dequantised fp8 one"""
    Q, refK, refV = forms(d, None, fp8)[-3:]
    return reference_ragged(Q, refK, refV, SQ, LENS, causal, W)


@functools.lru_cache(maxsize=None)
def forms(d, page, fp8):
    """the batch against a cache form: contiguous (page None) or paged, bf16 or fp8 with non-unit descales.  Returns the device tensors
    (Q, K, V, table or None, descale kwargs), the contiguous twin (Kc, Vc), and on the CPU Q and the K / V the reference reads"""
    Q, K, V = batch(d)
    B = len(SQ)
    if fp8:
        (Kb, kd), (Vb, vd) = quantise(K.float() * 3.0), quantise(V.float() * 0.5)      # descales well away from 1
        refK, refV = dequantise(Kb, kd), dequantise(Vb, vd)
        ds = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
        view = lambda t: t.view(F8)
    else:
        Kb, Vb, refK, refV, ds, view = K, V, K, V, {}, (lambda t: t)
    Kc, Vc = Kb.to(DEV), Vb.to(DEV)
    if page is None:
        return Q.to(DEV), view(Kc), view(Vc), None, ds, view(Kc), view(Vc), Q, refK, refV
    table = random_table(B, CAPACITY // page, 9400 + page + d).to(DEV)
    Kp, Vp = scatter(Kc, table, page), scatter(Vc, table, page)
    assert torch.equal(gather(Kp, table), Kc)
    return Q.to(DEV), view(Kp), view(Vp), table, ds, view(Kc), view(Vc), Q, refK, refV


def call(Q, K, V, table, cu, lens, **kw):
    if table is None:
        return fa.flash_attention_extend_varlen_window(Q, K, V, cu, lens, **kw)
    return fa.flash_attention_extend_paged_varlen_window(Q, K, V, table, cu, lens, **kw)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_parity_mixed_batch_and_rows_no_sequence_owns(d, causal):
    Qd, Kd, Vd, _, _, _, _, Q, _, _ = forms(d, None, False)
    T = Q.shape[0]
    cu, lens = i32(cu_of(SQ)), i32(LENS)
    for W in WINDOWS:
        refO, refL, owned = references(d, False, causal, W)
        for splits in (0, 1, 2, 3, 5):
            O = torch.full((T, H, d), SENTINEL, dtype=torch.float32, device=DEV)
            out, lse = fa.flash_attention_extend_varlen_window(Qd, Kd, Vd, cu, lens, is_causal=causal, num_splits=splits, window=W, O=O,
                                                        return_lse=True)
            torch.cuda.synchronize()
            assert out.data_ptr() == O.data_ptr() and lse.shape == (H, T)
            Oc, lc = O.cpu(), lse.cpu()
            # the rows no sequence owns come back as they went in, bit for bit (the LSE was allocated zero-filled)
            assert bool((Oc[~owned] == SENTINEL).all()) and not lc[:, ~owned].any(), (W, splits)
            assert_close(Oc[owned], lc[:, owned], refO[owned], refL[:, owned], f"varlen d {d} causal {causal} W {W} splits {splits}")


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_seam_every_sequence_is_the_windowed_extend_on_that_sequence_alone(d, page, fp8):
    """all four cache forms: O and LSE of every sequence equal flash_attention_extend*_window(window=W) on that sequence alone (batch of
    one) at forced splits 1 and 3, for sq_b <= 16 flash_attention_decode*(window=W) as well; paged equals contiguous; the float64
    criterion holds"""
    Q, K, V, table, ds, Kc, Vc, _, _, _ = forms(d, page, fp8)
    cu_l, cu, lens = cu_of(SQ), i32(cu_of(SQ)), i32(LENS)
    for W in WINDOWS:
        refO, refL, _ = references(d, fp8, True, W)
        for splits in (1, 3):
            kw = dict(is_causal=True, out_dtype=torch.float32, num_splits=splits, return_lse=True, window=W, **ds)
            O, lse = call(Q, K, V, table, cu, lens, **kw)
            if table is not None:
                Oc, lc = fa.flash_attention_extend_varlen_window(Q, Kc, Vc, cu, lens, **kw)
                torch.cuda.synchronize()
                assert torch.equal(O, Oc) and torch.equal(lse, lc), "paged != contiguous on the gathered copy"
            for b, s in enumerate(SQ):
                if s == 0:
                    continue
                q = Q[cu_l[b]:cu_l[b + 1]].transpose(0, 1)[None].contiguous()              # [1, H, sq_b, d]
                one = i32([LENS[b]])
                if table is None:
                    Ob, lb = fa.flash_attention_extend_window(q, K[b:b + 1], V[b:b + 1], one, **kw)
                else:
                    Ob, lb = fa.flash_attention_extend_paged_window(q, K, V, table[b:b + 1], one, **kw)
                torch.cuda.synchronize()
                got, gl = O[cu_l[b]:cu_l[b + 1]].transpose(0, 1), lse[:, cu_l[b]:cu_l[b + 1]]
                assert torch.equal(got, Ob[0]) and torch.equal(gl, lb[0]), f"sequence {b} ({s} rows) differs from extend alone, W {W} splits {splits}"
                if s <= fa.FA_DECODE_MAX_Q:
                    if table is None:
                        Od, ld = fa.flash_attention_decode(q, K[b:b + 1], V[b:b + 1], one, **kw)
                    else:
                        Od, ld = fa.flash_attention_decode_paged(q, K, V, table[b:b + 1], one, **kw)
                    torch.cuda.synchronize()
                    assert torch.equal(got, Od[0]) and torch.equal(gl, ld[0]), f"sequence {b} ({s} rows) differs from decode, W {W} splits {splits}"
                assert_close(got, gl, refO[cu_l[b]:cu_l[b + 1]].transpose(0, 1), refL[:, cu_l[b]:cu_l[b + 1]],
                             f"form page {page} fp8 {fp8} d {d} W {W} sequence {b} splits {splits}")


@pytest.mark.parametrize("fp8,page", [(False, None), (True, 16)])
def test_no_window_is_the_unwindowed_call_and_poison_below_first_changes_nothing(fp8, page):
    d = 128
    Q, K, V, table, ds, _, _, _, _, _ = forms(d, page, fp8)
    cu, lens = i32(cu_of(SQ)), i32(LENS)
    kw = dict(is_causal=True, out_dtype=torch.float32, return_lse=True, **ds)
    for splits in (0, 1, 3):
        plain = (fa.flash_attention_extend_varlen(Q, K, V, cu, lens, num_splits=splits, **kw) if table is None else
                 fa.flash_attention_extend_paged_varlen(Q, K, V, table, cu, lens, num_splits=splits, **kw))
        for W in (None, 0, CAPACITY, 1 << 20):
            got = call(Q, K, V, table, cu, lens, num_splits=splits, window=W, **kw)
            torch.cuda.synchronize()
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), (splits, W)
    # NaN (fp8: 0x7F) in every key below first(b) and beyond the length; paged: in the pages wholly below first(b), entries -1
    W = 100
    bad = 0x7F if fp8 else float("nan")
    raw = (lambda t: t.view(torch.uint8)) if fp8 else (lambda t: t)
    back = (lambda t: t.view(F8)) if fp8 else (lambda t: t)
    Kx, Vx = raw(K).clone(), raw(V).clone()
    tx = None if table is None else table.clone()
    hit = 0
    for b, s in enumerate(SQ):
        if s == 0:
            continue
        f = first_visible(LENS[b], s, W)
        if table is None:
            Kx[b, :, :f], Vx[b, :, :f] = bad, bad
            Kx[b, :, LENS[b]:], Vx[b, :, LENS[b]:] = bad, bad
            hit += f
        else:
            gone = table[b, :f // page].long()
            Kx[gone], Vx[gone] = bad, bad
            tx[b, :f // page] = -1
            hit += f // page
    assert hit > 0
    for splits in (1, 3):
        clean = call(Q, K, V, table, cu, lens, num_splits=splits, window=W, **kw)
        got = call(Q, back(Kx), back(Vx), tx, cu, lens, num_splits=splits, window=W, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
        assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1]), splits


def test_outputs_and_determinism():
    d, W = 128, 100
    Q, K, V, _, _, _, _, _, _, _ = forms(d, None, False)
    cu, lens = i32(cu_of(SQ)), i32(LENS)
    for splits in (1, 3):
        kw = dict(is_causal=True, num_splits=splits, window=W)
        O32, lse = fa.flash_attention_extend_varlen_window(Q, K, V, cu, lens, out_dtype=torch.float32, return_lse=True, **kw)
        again, lse2 = fa.flash_attention_extend_varlen_window(Q, K, V, cu, lens, out_dtype=torch.float32, return_lse=True, **kw)
        no_lse = fa.flash_attention_extend_varlen_window(Q, K, V, cu, lens, out_dtype=torch.float32, **kw)
        Ob = fa.flash_attention_extend_varlen_window(Q, K, V, cu, lens, out_dtype=torch.bfloat16, **kw)
        Oh = fa.flash_attention_extend_varlen_window(Q, K, V, cu, lens, out_dtype=torch.float16, **kw)
        torch.cuda.synchronize()
        assert torch.equal(O32, again) and torch.equal(lse, lse2), "two runs differ"
        assert torch.equal(O32, no_lse), "O depends on whether the LSE was requested"
        assert torch.equal(Ob, O32.to(torch.bfloat16)) and torch.equal(Oh, O32.to(torch.float16)), "not the fp32 result rounded once"


def test_three_steps_as_one_replayed_graph_with_first_crossing_a_tile_start():
    """`kv_lens += q_lens; kv_cache_append_varlen; flash_attention_extend_varlen_window`: one linear graph on one stream, captured once
    at a fixed totalQ and replayed for three steps with cu_seqlens_q and the lengths changed in place.  Sequence 0 decodes a row per
    step behind 254 keys: its first goes 127, 128, 129 -- across the start of tile 1.  Sequence 1 prefills in chunks, sequence 2 joins
    at step 1 and then decodes"""
    B, d, T, W = 3, 128, 128, 128
    steps = [[1, 40, 0], [1, 30, 65], [1, 17, 1]]
    start = [254, 300, 100]
    Kall, Vall = randn((B, HKV, CAPACITY, d), 9501, BF16), randn((B, HKV, CAPACITY, d), 9502, BF16)      # keys by position
    Kc, Vc = (torch.zeros((B, HKV, CAPACITY, d), dtype=BF16, device=DEV) for _ in range(2))
    for b, n in enumerate(start):
        Kc[b, :, :n], Vc[b, :, :n] = Kall[b, :, :n].to(DEV), Vall[b, :, :n].to(DEV)
    lens = i32(start)
    Qs = torch.zeros((T, H, d), dtype=BF16, device=DEV)
    Kn, Vn = (torch.zeros((T, HKV, d), dtype=BF16, device=DEV) for _ in range(2))
    cu, q_lens = i32([0] * (B + 1)), i32([0] * B)
    Os = torch.zeros((T, H, d), dtype=torch.float32, device=DEV)
    ws = torch.empty(fa.decode_workspace_size(1, H, T, d, 2), dtype=torch.uint8, device=DEV)

    def step():
        lens.add_(q_lens)
        fa.kv_cache_append_varlen(Kn, Vn, Kc, Vc, cu, lens)
        fa.flash_attention_extend_varlen_window(Qs, Kc, Vc, cu, lens, is_causal=True, num_splits=2, window=W, O=Os, workspace=ws)

    step()                                                       # every kernel has run once before the capture (all slots idle)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    pos, firsts = list(start), []
    for it, sq in enumerate(steps):
        c = cu_of(sq)
        q = randn((T, H, d), 9510 + it, BF16)
        kn, vn = torch.zeros((T, HKV, d), dtype=BF16), torch.zeros((T, HKV, d), dtype=BF16)
        for b, s in enumerate(sq):
            kn[c[b]:c[b + 1]] = Kall[b, :, pos[b]:pos[b] + s].transpose(0, 1)
            vn[c[b]:c[b + 1]] = Vall[b, :, pos[b]:pos[b] + s].transpose(0, 1)
            pos[b] += s
        Qs.copy_(q); Kn.copy_(kn); Vn.copy_(vn); cu.copy_(i32(c)); q_lens.copy_(i32(sq))
        Os.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert lens.tolist() == pos
        firsts.append(first_visible(pos[0], sq[0], W))
        refO, _, owned = reference_ragged(q, Kc.cpu(), Vc.cpu(), sq, pos, True, W)
        O = Os.double().cpu()
        err, tol = (O - refO).abs()[owned], (1e-3 + 1e-3 * refO.abs())[owned]
        print(f"step {it}: rows {sq}, worst O error / tolerance {(err / tol).max().item():.3f}")
        assert torch.isfinite(O[owned]).all() and (err <= tol).all(), f"step {it}: worst ratio {(err / tol).max().item():.3f}"
        assert bool((Os.cpu()[~owned] == SENTINEL).all()), f"step {it}: a row no sequence owns was written"
    assert firsts == [127, 128, 129]
