"""GPU tests of flash_attention_extend_varlen / flash_attention_extend_paged_varlen: ragged chunked prefill against the decode K/V
caches -- every sequence its own number of new rows, Q / O packed by token.  Reference (per sequence, as a batch of one), mask and
criterion (1e-3 + 1e-3 |ref| on O, 2e-4 + 2e-6 |ref| on the LSE, every element) are those of tests/kv_cache_check.py, the score-noise
criterion of the scale cases included.  The property most tests lean on is the seam: a sequence's bits are
those of flash_attention_extend* (and, up to 16 rows, flash_attention_decode*) on that sequence alone under the same forced splits."""
import ctypes
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from abi_decl import c_call  # noqa: E402
from kv_cache_check import (CAP, DEV, F8, SCALES, assert_close, assert_close_with_score_noise, cu_of, dequantise, gather, i32,  # noqa: E402
                            quantise, randn, reference_ragged)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
HKV = 2
# the mixed batch: decode rows, an idle slot, rows across 16 and across the row blocks of 32 / 64 packed rows
SQ = [1, 0, 5, 16, 17, 64, 65, 130, 1, 200]
# lengths around the 128-key tile seams; the idle slot's is garbage; sequence 7 has fewer keys than rows (100 < 130)
LENS = [129, -77, 128, 127, 256, 257, 385, 100, 1024, 640]
CAPACITY = 1024
PAD = 37                                        # totalQ = cu[-1] + PAD: rows no sequence owns
SENTINEL = -123456.75


@functools.lru_cache(maxsize=None)
def mixed_case(d, G):
    """(Q [T, H, d], K, V, packed references {causal: (O, LSE, owned)}) of the mixed batch on the CPU, computed once"""
    T, H = sum(SQ) + PAD, HKV * G
    Q = randn((T, H, d), 101 + G, BF16)
    K, V = randn((len(SQ), HKV, CAPACITY, d), 102 + d, BF16), randn((len(SQ), HKV, CAPACITY, d), 103 + d, BF16)
    refs = {c: reference_ragged(Q, K, V, SQ, LENS, c) for c in (False, True)}
    return Q, K, V, refs


def raw_varlen(Q, K, V, O, lse, cu, lens, splits, causal):
    """the C entry point on caller-owned O and LSE (the front allocates the LSE itself): contiguous bf16 cache, dense tensors.
    Returns the workspace, to be kept until the stream is synchronised"""
    T, H, d = Q.shape
    B, Hkv, Sk = K.shape[:3]
    ns = fa.extend_varlen_plan(B, H, Hkv, T, Sk, d, fa.FA_DTYPE_F32, splits)["num_splits"]
    need = fa.decode_workspace_size(1, H, T, d, ns)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    rc = c_call("flash_attention_extend_varlen", dict(
        Q=Q.data_ptr(), K=K.data_ptr(), V=V.data_ptr(), O=O.data_ptr(), LSE=lse.data_ptr(), cu=cu.data_ptr(), lens=lens.data_ptr(), kd=None,
        vd=None, ws=ws.data_ptr() if need else None, B=B, H=H, Hkv=Hkv, T=T, Sk=Sk, d=d, scale=1.0 / d ** 0.5, causal=causal,
        dtype=fa.FA_DTYPE_BF16, kv=fa.FA_DTYPE_BF16, o=fa.FA_DTYPE_F32, ns=ns, strides=[None] * 4,
        stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert rc == 0, rc
    return ws


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("d", [64, 128])
def test_parity_mixed_batch(d, G, causal):
    Q, K, V, refs = mixed_case(d, G)
    refO, refL, owned = refs[causal]
    T, H = Q.shape[:2]
    Qd, Kd, Vd, cu, lens = Q.to(DEV), K.to(DEV), V.to(DEV), i32(cu_of(SQ)), i32(LENS)
    for splits in (0, 1, 3, CAP):
        O = torch.full((T, H, d), SENTINEL, dtype=torch.float32, device=DEV)
        lse = torch.full((H, T), SENTINEL, dtype=torch.float32, device=DEV)
        keep = raw_varlen(Qd, Kd, Vd, O, lse, cu, lens, splits, causal)
        torch.cuda.synchronize()
        del keep
        Oc, lc = O.cpu(), lse.cpu()
        # the rows no sequence owns come back as they went in, bit for bit
        assert torch.equal(Oc[~owned].view(torch.int32), torch.full_like(Oc[~owned], SENTINEL).view(torch.int32)), splits
        assert torch.equal(lc[:, ~owned].view(torch.int32), torch.full_like(lc[:, ~owned], SENTINEL).view(torch.int32)), splits
        assert_close(Oc[owned], lc[:, owned], refO[owned], refL[:, owned], f"varlen d {d} G {G} causal {causal} splits {splits}")
        # the front: the same bits, and zeros where nothing is written
        Of, lf = fa.flash_attention_extend_varlen(Qd, Kd, Vd, cu, lens, is_causal=causal, out_dtype=torch.float32, num_splits=splits,
                                                  return_lse=True)
        torch.cuda.synchronize()
        assert Of.shape == (T, H, d) and lf.shape == (H, T)
        assert torch.equal(Of.cpu()[owned], Oc[owned]) and torch.equal(lf.cpu()[:, owned], lc[:, owned]), splits
        assert not Of.cpu()[~owned].any() and not lf.cpu()[:, ~owned].any(), splits


# ---- the four cache forms ----
def forms_case(d, G, page, fp8):
    """the mixed batch against a cache form: contiguous (page None) or paged, bf16 or fp8 with non-unit descales.  Returns the device
    tensors (Q, K, V, table or None, descale kwargs), the contiguous twin (Kc, Vc) and the CPU K / V the reference reads"""
    Q, K, V, _ = mixed_case(d, G)
    B = len(SQ)
    if fp8:
        (Kb, kd), (Vb, vd) = quantise(K.float() * 3.0), quantise(V.float() * 0.5)      # descales well away from 1
        refK, refV = dequantise(Kb, kd), dequantise(Vb, vd)
        ds = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
        view = lambda t: t.to(DEV).view(F8)
    else:
        Kb, Vb, refK, refV, ds, view = K, V, K, V, {}, (lambda t: t.to(DEV))
    if page is None:
        return Q.to(DEV), view(Kb), view(Vb), None, ds, view(Kb), view(Vb), refK, refV
    n = CAPACITY // page
    P = B * n + 5
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(page + d))[:B * n]
    pools = []
    for t in (Kb, Vb):
        pool = torch.zeros((P, HKV, page, d), dtype=t.dtype)
        pool[perm] = t.view(B, HKV, n, page, d).transpose(1, 2).reshape(B * n, HKV, page, d)
        pools.append(pool)
    table = perm.reshape(B, n).to(torch.int32)
    assert torch.equal(gather(pools[0], table), Kb)
    return Q.to(DEV), view(pools[0]), view(pools[1]), table.to(DEV), ds, view(Kb), view(Vb), refK, refV


def call(Q, K, V, table, cu, lens, **kw):
    if table is None:
        return fa.flash_attention_extend_varlen(Q, K, V, cu, lens, **kw)
    return fa.flash_attention_extend_paged_varlen(Q, K, V, table, cu, lens, **kw)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_seam_every_sequence_is_extend_on_that_sequence_alone(d, page, fp8):
    """all four cache forms: O and LSE of every sequence equal flash_attention_extend* on that sequence alone (batch of one) at forced
    splits 1 and 3, for sq_b <= 16 flash_attention_decode* as well; paged equals contiguous; the float64 criterion holds"""
    G = 4
    Q, K, V, table, ds, Kc, Vc, refK, refV = forms_case(d, G, page, fp8)
    cu_l, cu, lens = cu_of(SQ), i32(cu_of(SQ)), i32(LENS)
    refO, refL, _ = reference_ragged(Q.cpu(), refK, refV, SQ, LENS, True)
    for splits in (1, 3):
        kw = dict(is_causal=True, out_dtype=torch.float32, num_splits=splits, return_lse=True, **ds)
        O, lse = call(Q, K, V, table, cu, lens, **kw)
        if table is not None:
            Oc, lc = fa.flash_attention_extend_varlen(Q, Kc, Vc, cu, lens, **kw)
            torch.cuda.synchronize()
            assert torch.equal(O, Oc) and torch.equal(lse, lc), "paged != contiguous on the gathered copy"
        for b, s in enumerate(SQ):
            if s == 0:
                continue
            q = Q[cu_l[b]:cu_l[b + 1]].transpose(0, 1)[None].contiguous()              # [1, H, sq_b, d]
            one = i32([LENS[b]])
            if table is None:
                Ob, lb = fa.flash_attention_extend(q, K[b:b + 1], V[b:b + 1], one, **kw)
            else:
                Ob, lb = fa.flash_attention_extend_paged(q, K, V, table[b:b + 1], one, **kw)
            torch.cuda.synchronize()
            got, gl = O[cu_l[b]:cu_l[b + 1]].transpose(0, 1), lse[:, cu_l[b]:cu_l[b + 1]]
            assert torch.equal(got, Ob[0]) and torch.equal(gl, lb[0]), f"sequence {b} ({s} rows) differs from extend alone, splits {splits}"
            if s <= fa.FA_DECODE_MAX_Q:
                if table is None:
                    Od, ld = fa.flash_attention_decode(q, K[b:b + 1], V[b:b + 1], one, **kw)
                else:
                    Od, ld = fa.flash_attention_decode_paged(q, K, V, table[b:b + 1], one, **kw)
                torch.cuda.synchronize()
                assert torch.equal(got, Od[0]) and torch.equal(gl, ld[0]), f"sequence {b} ({s} rows) differs from decode, splits {splits}"
            assert_close(got, gl, refO[cu_l[b]:cu_l[b + 1]].transpose(0, 1), refL[:, cu_l[b]:cu_l[b + 1]],
                         f"form page {page} fp8 {fp8} d {d} sequence {b} splits {splits}")


@pytest.mark.parametrize("fp8,page", [(False, None), (True, 16)])
@pytest.mark.parametrize("d", [64, 128])
def test_a_uniform_batch_is_the_batched_extend(d, fp8, page):
    """cu = [0, Sq, 2 Sq, ..]: the result equals flash_attention_extend* over a token-major strided view of the same Q"""
    G, Sq = 4, 50
    _, K, V, table, ds, _, _, _, _ = forms_case(d, G, page, fp8)
    B, H = len(SQ), HKV * G
    Q = randn((B * Sq, H, d), 111, BF16).to(DEV)
    lens = i32([max(L, 1) for L in LENS])
    cu = i32([b * Sq for b in range(B + 1)])
    Qb = Q.view(B, Sq, H, d).permute(0, 2, 1, 3)                 # [B, H, Sq, d], strided
    for causal in (False, True):
        for splits in (1, 3):
            kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, **ds)
            O, lse = call(Q, K, V, table, cu, lens, **kw)
            Ob, lb = (fa.flash_attention_extend(Qb, K, V, lens, **kw) if table is None else
                      fa.flash_attention_extend_paged(Qb, K, V, table, lens, **kw))
            torch.cuda.synchronize()
            assert torch.equal(O.view(B, Sq, H, d).permute(0, 2, 1, 3), Ob), (causal, splits)
            assert torch.equal(lse.view(H, B, Sq).permute(1, 0, 2), lb), (causal, splits)


# ---- the unit lookup ----
def lookup_case(sq, d=64, G=4, cap=256, seed=121, extra=0):
    """a batch with the row counts `sq`, every sequence at a length of its own; returns device inputs and the packed reference"""
    B, H, T = len(sq), HKV * G, max(sum(sq), 1) + extra
    lens = [1 + (37 * b + 11) % cap for b in range(B)]
    Q, K, V = randn((T, H, d), seed, BF16), randn((B, HKV, cap, d), seed + 1, BF16), randn((B, HKV, cap, d), seed + 2, BF16)
    ref = reference_ragged(Q, K, V, sq, lens, True)
    return Q.to(DEV), K.to(DEV), V.to(DEV), i32(cu_of(sq)), i32(lens), ref


@pytest.mark.parametrize("name", ["130 sequences", "one sequence", "all but the last empty", "three empty between"])
def test_lookup_edges(name):
    """the scan of the per-sequence block counts: across its 64- and 128-sequence steps, a single sequence, leading idle slots;
    cu[-1] == totalQ exactly in every case (no padding rows)"""
    sq = {"130 sequences": [(b * 7 + 3) % 4 for b in range(64)] + [70] + [(b * 5 + 1) % 4 for b in range(65)],
          "one sequence": [45],
          "all but the last empty": [0] * 69 + [33],
          "three empty between": [3, 0, 0, 0, 40, 0, 1]}[name]
    Q, K, V, cu, lens, (refO, refL, owned) = lookup_case(sq)
    assert bool(owned.all()) and int(cu[-1]) == Q.shape[0]
    for splits in (1, 3):
        O, lse = fa.flash_attention_extend_varlen(Q, K, V, cu, lens, is_causal=True, out_dtype=torch.float32, num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close(O, lse, refO, refL, f"lookup: {name}, splits {splits}")


def test_offsets_beyond_total_q_are_clamped():
    """cu[-1] = totalQ + 1000: q1 = clamp(cu[b + 1], q0, totalQ) cuts the last sequence at totalQ -- it then HAS totalQ - q0 rows, the
    last rows of its length -- and everything else stands"""
    sq = [20, 0, 7, 60]
    T = sum(sq)
    cut = sq[:-1] + [60 - 25]                                   # what the kernel sees once totalQ is 25 rows short
    Q, K, V, cu, lens, (refO, refL, owned) = lookup_case(cut, seed=131)
    assert Q.shape[0] == T - 25
    beyond = i32(cu_of(sq)[:-1] + [T - 25 + 1000])
    for splits in (1, 3):
        kw = dict(is_causal=True, out_dtype=torch.float32, num_splits=splits, return_lse=True)
        O, lse = fa.flash_attention_extend_varlen(Q, K, V, beyond, lens, **kw)
        Oc, lc = fa.flash_attention_extend_varlen(Q, K, V, cu, lens, **kw)
        torch.cuda.synchronize()
        assert torch.equal(O, Oc) and torch.equal(lse, lc), splits
        assert_close(O, lse, refO, refL, f"clamped offsets, splits {splits}")


# ---- what is never read ----
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16, 128])
def test_poison(page, fp8):
    """NaN beyond every length and in pages no table names, out-of-range table entries beyond the last visible page, and garbage in
    the length and the table row of the idle slot: not a bit changes"""
    d, G = 128, 4
    Q, K, V, table, ds, _, _, _, _ = forms_case(d, G, page, fp8)
    cu, lens = i32(cu_of(SQ)), i32(LENS)
    bad = 0x7F if fp8 else float("nan")
    raw = (lambda t: t.view(torch.uint8)) if fp8 else (lambda t: t)
    Kx, Vx = raw(K).clone(), raw(V).clone()
    lens_x = lens.clone()
    idle = SQ.index(0)
    lens_x[idle] = 2 ** 31 - 1
    if table is None:
        for b, L in enumerate(LENS):
            L = CAPACITY if SQ[b] == 0 else L
            Kx[b, :, L:] = bad
            Vx[b, :, L:] = bad
        Kx[idle], Vx[idle], tx = bad, bad, None
    else:
        P, n = K.shape[0], table.shape[1]
        tx = table.clone()
        named = torch.zeros(P, dtype=torch.bool, device=DEV)
        garbage = i32([2 ** 31 - 1, -2 ** 31, P, -1] * n)
        for b, L in enumerate(LENS):
            if SQ[b] == 0:
                tx[b] = garbage[:n]
                continue
            last = (L - 1) // page
            named[table[b, :last + 1].long()] = True
            tx[b, last + 1:] = garbage[:n - last - 1]
            Kx[table[b, last].long(), :, L - last * page:] = bad
            Vx[table[b, last].long(), :, L - last * page:] = bad
        Kx[~named], Vx[~named] = bad, bad
    back = (lambda t: t.view(F8)) if fp8 else (lambda t: t)
    for causal in (False, True):
        for splits in (1, 3):
            kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True, **ds)
            O, lse = call(Q, K, V, table, cu, lens, **kw)
            Ox, lx = call(Q, back(Kx), back(Vx), tx, cu, lens_x, **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(O).all() and torch.isfinite(lse).all()
            assert torch.equal(O, Ox) and torch.equal(lse, lx), (causal, splits)


@pytest.mark.parametrize("splits", [1, 3])
def test_views_outputs_streams_and_determinism(splits):
    d, G = 128, 4
    Q, K, V, _ = mixed_case(d, G)
    T, H = Q.shape[:2]
    Qd, Kd, Vd, cu, lens = Q.to(DEV), K.to(DEV), V.to(DEV), i32(cu_of(SQ)), i32(LENS)
    kw = dict(is_causal=True, num_splits=splits)
    O32, lse = fa.flash_attention_extend_varlen(Qd, Kd, Vd, cu, lens, out_dtype=torch.float32, return_lse=True, **kw)
    again, lse2 = fa.flash_attention_extend_varlen(Qd, Kd, Vd, cu, lens, out_dtype=torch.float32, return_lse=True, **kw)
    no_lse = fa.flash_attention_extend_varlen(Qd, Kd, Vd, cu, lens, out_dtype=torch.float32, **kw)
    Ob = fa.flash_attention_extend_varlen(Qd, Kd, Vd, cu, lens, out_dtype=torch.bfloat16, **kw)
    Oh = fa.flash_attention_extend_varlen(Qd, Kd, Vd, cu, lens, out_dtype=torch.float16, **kw)
    # Q as the slice of a fused [T, (H + 2 Hkv) d] projection, O as a slice of a wider buffer, the cache as a [B, S, Hkv, d] view
    fused = torch.zeros((T, (H + 2 * HKV) * d), dtype=BF16, device=DEV)
    fused[:, :H * d] = Qd.reshape(T, H * d)
    Qs = fused[:, :H * d].view(T, H, d)
    wide = torch.zeros((T, H, 2 * d), dtype=torch.float32, device=DEV)
    Ks, Vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (Kd, Vd))
    assert not Qs.is_contiguous() and not Ks.is_contiguous()
    Os = fa.flash_attention_extend_varlen(Qs, Ks, Vs, cu, lens, O=wide[:, :, d:], **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Oside, lside = fa.flash_attention_extend_varlen(Qd, Kd, Vd, cu, lens, out_dtype=torch.float32, return_lse=True, stream=side, **kw)
    side.synchronize()
    assert torch.equal(O32, again) and torch.equal(lse, lse2), "two runs differ"
    assert torch.equal(O32, no_lse), "O depends on whether the LSE was requested"
    assert torch.equal(O32, Oside) and torch.equal(lse, lside), "side stream"
    assert torch.equal(Ob, O32.to(torch.bfloat16)) and torch.equal(Oh, O32.to(torch.float16)), "not the fp32 result rounded once"
    assert Os.data_ptr() == wide[:, :, d:].data_ptr() and torch.equal(Os, O32) and not wide[:, :, :d].any(), "strided views"


@pytest.mark.parametrize("kind", ["one", "boost3"])
@pytest.mark.parametrize("d", [64, 128])
def test_scale_cases(d, kind):
    """scale 1 (scores kept O(1)) and Q, K x 3, on a decode row, a 20-row and a 64-row chunk: the criterion with the fp32 score-noise
    term, per sequence"""
    scale, mul = SCALES[kind](d)
    G, sq, lens, cap = 4, [1, 20, 64], [1000, 333, 700], 1000
    cu = cu_of(sq)
    Q = (randn((sum(sq), HKV * G, d), 141, BF16) * mul).bfloat16()
    K, V = (randn((3, HKV, cap, d), 142, BF16) * mul).bfloat16(), randn((3, HKV, cap, d), 143, BF16)
    for splits in (0, 1, 5):
        O, lse = fa.flash_attention_extend_varlen(Q.to(DEV), K.to(DEV), V.to(DEV), i32(cu), i32(lens), scale=scale, is_causal=True,
                                                  out_dtype=torch.float32, num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        for b in range(3):
            assert_close_with_score_noise(O[cu[b]:cu[b + 1]].transpose(0, 1)[None], lse[None, :, cu[b]:cu[b + 1]],
                                          Q[cu[b]:cu[b + 1]].transpose(0, 1)[None], K[b:b + 1], V[b:b + 1], [lens[b]], True, scale,
                                          f"varlen {kind} d {d} splits {splits} sequence {b}")


def test_mixed_batch_steps_as_one_graph():
    """`kv_lens += q_lens; kv_cache_append_paged_varlen; flash_attention_extend_paged_varlen` into a page-16 fp8 pool: one linear graph
    on one stream, captured once at a fixed totalQ and replayed for three steps with cu_seqlens_q, the lengths and the table changed in
    place.  Sequence 0 goes from a 96-row chunk to a 40-row chunk to 1-row decode; sequence 1 decodes and then goes idle; sequence 2
    joins at step 1; slot 3 stays idle.  Every step against one float64 attention over the dequantised cache"""
    B, G, d, page, n, T = 4, 4, 128, 16, 16, 128
    H, P = HKV * G, B * n + 3
    steps = [[96, 1, 0, 0], [40, 1, 30, 0], [1, 0, 2, 0]]
    start = [0, 57, 0, 0]                                        # sequence 1 sits behind 57 cached keys
    Kall, Vall = randn((B, HKV, 256, d), 151, BF16), randn((B, HKV, 256, d), 152, BF16)      # keys by position
    kd = (Kall.float().abs().amax(dim=(0, 2, 3)) / 448).to(DEV)
    vd = (Vall.float().abs().amax(dim=(0, 2, 3)) / 448).to(DEV)
    Kp, Vp = (torch.zeros((P, HKV, page, d), dtype=torch.uint8, device=DEV) for _ in range(2))
    table = torch.randperm(P, generator=torch.Generator().manual_seed(153))[:B * n].reshape(B, n).to(torch.int32).to(DEV)
    ds = dict(k_descale=kd, v_descale=vd)
    # the cached prefix of sequence 1, by the uniform append
    lens = i32(start)
    fa.kv_cache_append_paged(Kall[:, :, :57].contiguous().to(DEV), Vall[:, :, :57].contiguous().to(DEV), Kp.view(F8), Vp.view(F8), table, lens, **ds)
    # static tensors of the graph
    Qs = torch.zeros((T, H, d), dtype=BF16, device=DEV)
    Kn, Vn = (torch.zeros((T, HKV, d), dtype=BF16, device=DEV) for _ in range(2))
    cu, q_lens = i32([0] * (B + 1)), i32([0] * B)
    Os = torch.zeros((T, H, d), dtype=torch.float32, device=DEV)
    ws = torch.empty(fa.decode_workspace_size(1, H, T, d, 2), dtype=torch.uint8, device=DEV)

    def step():
        lens.add_(q_lens)
        fa.kv_cache_append_paged_varlen(Kn, Vn, Kp.view(F8), Vp.view(F8), table, cu, lens, **ds)
        fa.flash_attention_extend_paged_varlen(Qs, Kp.view(F8), Vp.view(F8), table, cu, lens, is_causal=True, num_splits=2, O=Os, workspace=ws, **ds)

    step()                                                       # every kernel has run once before the capture (all slots idle)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    pos = list(start)
    for it, sq in enumerate(steps):
        c = cu_of(sq)
        q = randn((T, H, d), 160 + it, BF16)
        kn, vn = torch.zeros((T, HKV, d), dtype=BF16), torch.zeros((T, HKV, d), dtype=BF16)
        for b, s in enumerate(sq):
            kn[c[b]:c[b + 1]] = Kall[b, :, pos[b]:pos[b] + s].transpose(0, 1)
            vn[c[b]:c[b + 1]] = Vall[b, :, pos[b]:pos[b] + s].transpose(0, 1)
            pos[b] += s
        if it == 1:                                              # the joining sequence gets fresh pages: its table row changes in place
            table[2] = table[2].flip(0)
        Qs.copy_(q); Kn.copy_(kn); Vn.copy_(vn); cu.copy_(i32(c)); q_lens.copy_(i32(sq))
        Os.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert lens.tolist() == pos
        K64, V64 = gather(dequantise(Kp.cpu(), kd.cpu()), table.cpu()), gather(dequantise(Vp.cpu(), vd.cpu()), table.cpu())
        refO, _, owned = reference_ragged(q, K64, V64, sq, pos, True)
        O = Os.double().cpu()
        err, tol = (O - refO).abs()[owned], (1e-3 + 1e-3 * refO.abs())[owned]
        print(f"step {it}: rows {sq}, worst O error / tolerance {(err / tol).max().item():.3f}")
        assert torch.isfinite(O[owned]).all() and (err <= tol).all(), f"step {it}: worst ratio {(err / tol).max().item():.3f}"
        assert bool((Os.cpu()[~owned] == SENTINEL).all()), f"step {it}: a row no sequence owns was written"
