"""CPU tests of MLA decode (flash_attention_mla_decode, _mla_decode_paged, _mla_decode_plan, _mla_decode_workspace_size) at the C ABI, in
the binding and in the tests' own reference and emulation (mla_check.py):

* the four symbols are exported with the declared signatures;
* every refusal of flash_attention_decode / _paged comes back from the MLA call of the same cache form with the twin's code (fake aligned
  host pointers: no GPU is touched; no call here is valid as a whole), and the refusals the calls add stand at their places: the latent
  and rotary widths where dHead stands, sKV's head stride not read;
* plan properties and the workspace size;
* the Python fronts' refusals;
* the fp32 emulation of the kernel's arithmetic is within HALF the tolerance on every input of the GPU parity tests, so those inputs are
  known admissible before the GPU run, and it REFUSES nothing the hi + lo weights are there for (single weights miss a short cache);
* five wrong implementations emulated in float64, each refused on a named row.
"""
import ctypes
import itertools

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

import abi_decl  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, aligned_host_pointer, declared_parameters)

TWINS = {"flash_attention_mla_decode": "flash_attention_decode", "flash_attention_mla_decode_paged": "flash_attention_decode_paged"}


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    vp, i, f, b, sp = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_bool, ctypes.POINTER(fa.FaStrides)
    want = {
        "flash_attention_mla_decode": [
            ("Q", vp), ("KV", vp), ("O", vp), ("LSE", vp), ("kvLens", vp), ("workspace", vp), ("batchSize", i), ("numHeads", i),
            ("seqLenQ", i), ("seqLenK", i), ("dLatent", i), ("dRope", i), ("scale", f), ("is_causal", b), ("dtype", i), ("o_dtype", i),
            ("numSplits", i), ("sQ", sp), ("sKV", sp), ("sO", sp), ("stream", vp)],
        "flash_attention_mla_decode_paged": [
            ("Q", vp), ("KVpool", vp), ("O", vp), ("LSE", vp), ("kvLens", vp), ("blockTable", vp), ("workspace", vp), ("batchSize", i),
            ("numHeads", i), ("seqLenQ", i), ("numPages", i), ("pageSize", i), ("maxPagesPerSeq", i), ("tableStride", ctypes.c_int64),
            ("dLatent", i), ("dRope", i), ("scale", f), ("is_causal", b), ("dtype", i), ("o_dtype", i), ("numSplits", i), ("sQ", sp),
            ("sKV", sp), ("sO", sp), ("stream", vp)],
        "flash_attention_mla_decode_plan": [(n, i) for n in ("batchSize", "numHeads", "seqLenQ", "seqLenK", "dLatent", "dRope", "o_dtype",
                                                              "numSplits")] + [("plan", ctypes.POINTER(fa.FaDecodePlan))],
        "flash_attention_mla_decode_workspace_size": [(n, i) for n in ("batchSize", "numHeads", "seqLenQ", "dLatent", "numSplits")],
    }
    assert sorted(fa._MLA_SYMBOLS.values()) == sorted(TWINS)
    for name, params in want.items():
        assert name in fa.EXPORTS and getattr(L, name) is not None
        assert declared_parameters(name) == [n for n, _ in params], name
        assert list(getattr(L, name).argtypes) == [t for _, t in params], name
        assert getattr(L, name).restype is (ctypes.c_size_t if "workspace" in name else i)
    # what distinguishes a call from its twin: one cache tensor and its strides, no K/V head count, two widths for dHead
    for name, twin in TWINS.items():
        mine, theirs = set(declared_parameters(name)), set(declared_parameters(twin))
        assert theirs - mine == {"K", "V", "Kpool", "Vpool", "numHeadsKV", "dHead", "sK", "sV"} & theirs, name
        assert mine - theirs == {"KV", "KVpool", "dLatent", "dRope", "sKV"} & mine, name


def calls():
    """{MLA entry point: call(twin=False, **overrides)} on an aligned host pointer p, and p.  Every call is valid but for its workspace
    (two forced splits), so that passing every other check ends at NULL_POINTER.  twin=True: flash_attention_decode / _paged on the
    twin's share of the arguments -- K = V = the cache, one K/V head, d = 128 unless the override says otherwise"""
    import mla_check as mc
    host = aligned_host_pointer()
    p = host[1]
    ok = dict(Q=p, KV=p, O=p, LSE=None, lens=None, table=p, ws=None, B=2, H=8, Sq=4, Sk=1024, P=64, page=64, maxp=16, ts=16, dl=512, dr=64,
              scale=0.125, causal=True, dtype=BF16, o=F32, ns=2, stream=None)

    def make(name):
        def call(twin=False, _keep=host, **kw):
            v = dict(ok, **kw)
            st = v.pop("strides", [None] * 3)            # Q, KV, O
            if twin:
                d = v.pop("d", 128)
                t = {k: x for k, x in v.items() if k not in ("KV", "dl", "dr")}
                return abi_decl.c_call(TWINS[name], dict(t, K=v["KV"], V=v["KV"], Hkv=1, d=d, strides=[st[0], st[1], st[1], st[2]]))
            v.pop("d", None)
            return mc.c_call(name, dict(v, sQ=st[0], sKV=st[1], sO=st[2]))

        return call

    return {name: make(name) for name in TWINS}, p


def ladder(p, paged):
    """the arguments the twins refuse (and a few they accept up to the workspace check), as keyword overrides"""
    out = [dict()]
    for name in ("Q", "KV", "O"):
        out += [{name: None}, {name: p + 8}]
    out += [dict(LSE=p + 4), dict(ws=p + 8), dict(lens=p + 2), dict(lens=p + 2, Sq=0), dict(Q=None, O=p + 8)]
    out += [dict(ws=p, **kw) for kw in (dict(Sq=0), dict(Sq=-1), dict(Sq=17), dict(B=0), dict(H=0), dict(H=-3), dict(ns=-1), dict(ns=CAP + 1),
                                        dict(B=1 << 16, H=1 << 15))]
    out += [dict(Sq=s) for s in (1, 16)] + [dict(ns=CAP), dict(ws=p, ns=1, Q=None)]
    out += [dict(o=FP8), dict(o=7), dict(dtype=F32), dict(dtype=FP8), dict(dtype=F16), dict(dtype=9), dict(dtype=F32, ns=-1), dict(o=7, scale=0.0)]
    out += [dict(scale=s) for s in (0.0, -0.5, float("nan"), float("inf"))]
    if paged:
        out += [dict(table=None), dict(table=p + 2), dict(table=p + 2, Sq=0)]
        out += [dict(ws=p, **kw) for kw in (dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),
                                            dict(ts=15), dict(ts=-16))]
        out += [dict(page=16, maxp=4, ts=4), dict(page=1 << 12, maxp=1 << 12, ts=1 << 12)]
    else:
        out += [dict(ws=p, **kw) for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1))]
        out += [dict(Sk=1 << 20), dict(Sk=1)]
    return out


def test_the_decode_twins_ladder_with_the_twins_codes():
    fns, p = calls()
    bad = fa.FaStrides(64, 16, 8)                 # strideS below either width
    mis = fa.FaStrides(1 << 20, 1 << 20, 1030)    # rows that are no multiples of 16 bytes, in bf16 or fp32
    for name, call in fns.items():
        paged = "paged" in name
        assert call() == call(twin=True) == NULL_POINTER, name                         # valid but for the workspace
        for kw in ladder(p, paged):
            want = call(twin=True, **kw)
            assert NULL_POINTER >= want >= BAD_STRIDE, (name, kw, want)
            assert call(**kw) == want, (name, kw, want)
        for i, s in itertools.product(range(3), (bad, mis)):
            st = [None] * 3
            st[i] = ctypes.byref(s)
            assert call(strides=st) == call(twin=True, strides=st) == BAD_STRIDE, (name, i)
            assert call(strides=st, scale=0.0) == call(twin=True, strides=st, scale=0.0) == BAD_SCALE, (name, i)
        # the extent of one sequence's cache (contiguous: capacity + 192 rows; paged: one page), after the strides
        wide = fa.FaStrides(0, 0, 1 << 25)
        st = [None, ctypes.byref(wide), None]
        assert call(strides=st, ws=p) == call(twin=True, strides=st, ws=p) == BAD_SHAPE, name
        assert call(Q=None) == NULL_POINTER and call(KV=p + 8) == MISALIGNED and call(ws=p, ns=CAP + 1) == BAD_SHAPE
        assert call(dtype=F32) == BAD_DTYPE and call(scale=0.0) == BAD_SCALE


def test_the_new_refusals_at_their_places():
    fns, p = calls()
    for name, call in fns.items():
        paged = "paged" in name
        # the widths: where the twin refuses its dHead -- behind the pointers, the arrays, the geometry, the shape and the types, ahead
        # of the scale, the strides and the workspace
        for kw in (dict(dl=256), dict(dl=576, dr=0 + 64), dict(dr=32), dict(dr=128), dict(dl=128, dr=64), dict(dl=64, dr=512)):
            assert call(**kw) == call(ws=p, **kw) == call(twin=True, d=96) == BAD_DHEAD, (name, kw)
            assert call(scale=0.0, **kw) == BAD_DHEAD and call(strides=[ctypes.byref(fa.FaStrides(64, 16, 8)), None, None], **kw) == BAD_DHEAD
            assert call(Q=None, **kw) == NULL_POINTER and call(lens=p + 2, **kw) == MISALIGNED and call(Sq=17, **kw) == BAD_SHAPE
            assert call(dtype=F32, **kw) == BAD_DTYPE and call(o=7, **kw) == BAD_DTYPE and call(ns=CAP + 1, **kw) == BAD_SHAPE
            assert call(**kw, **(dict(page=24) if paged else dict(Sk=0))) == BAD_SHAPE, (name, kw)
        # a width that is no width: the shape step, as the twin's dHead <= 0
        for kw in (dict(dl=0), dict(dr=0), dict(dl=-512), dict(dl=512, dr=-64)):
            assert call(**kw) == call(twin=True, d=0) == BAD_SHAPE, (name, kw)
            assert call(dtype=F32, **kw) == BAD_SHAPE and call(Q=None, **kw) == NULL_POINTER
        # sKV: strideH is not read (decode refuses a head stride that is no multiple of 16 bytes)
        odd = fa.FaStrides(1 << 20, 7, 576)
        st = [None, ctypes.byref(odd), None]
        assert call(strides=st) == NULL_POINTER and call(twin=True, strides=st) == BAD_STRIDE, name
        neg = fa.FaStrides(1 << 20, -5, 640)
        assert call(strides=[None, ctypes.byref(neg), None]) == NULL_POINTER, name
        # ... strideB and strideS are: 16-byte multiples, a row of at least 576 elements
        for s in (fa.FaStrides(1 << 20, 0, 575), fa.FaStrides(1 << 20, 0, 580), fa.FaStrides(1028, 0, 576), fa.FaStrides(-576, 0, 576)):
            assert call(strides=[None, ctypes.byref(s), None]) == BAD_STRIDE, (name, s.strideB, s.strideS)
        # O's rows are 512 wide, Q's 576
        assert call(strides=[None, None, ctypes.byref(fa.FaStrides(1 << 20, 1 << 12, 512))]) == NULL_POINTER
        assert call(strides=[None, None, ctypes.byref(fa.FaStrides(1 << 20, 1 << 12, 504))]) == BAD_STRIDE
        assert call(strides=[ctypes.byref(fa.FaStrides(1 << 20, 1 << 12, 512)), None, None]) == BAD_STRIDE
        # a NULL workspace is the last rung, and only under more than one split
        assert call(ns=1, Q=None) == NULL_POINTER and call(ns=2) == NULL_POINTER and call(ns=2, scale=0.0) == BAD_SCALE
        # the grid limit: 2^18 sequences x 1 row block x 64 splits = 2^24 workgroups; the rows of O under two splits
        assert call(B=1 << 18, H=1, Sq=1, ns=64, ws=p) == BAD_SHAPE and call(B=1 << 18, H=1, Sq=1, ns=32) == NULL_POINTER
        assert call(B=1 << 20, H=16, Sq=1, ns=2, ws=p) == BAD_SHAPE and call(B=1 << 19, H=16, Sq=1, ns=2) == NULL_POINTER


def test_plan_properties_and_the_workspace_size():
    import mla_check as mc
    L = fa.lib()
    for B, H, Sq, Sk in itertools.product((1, 3, 32, 128, 1024), (1, 13, 16, 64, 128), (1, 2, 5, 16), (1, 31, 32, 64, 384, 4096, 32768, 1 << 20)):
        auto = fa.mla_decode_plan(B, H, Sq, Sk)
        blocks = -(-H * Sq // 64)
        tiles = -(-Sk // auto["kv_block_rows"])
        assert auto["rows_per_block"] == mc.ROWS == 64 and auto["kv_block_rows"] == mc.KT and auto["threads"] == 256
        assert auto["row_blocks"] == blocks and auto["grid"] == B * blocks * auto["num_splits"]
        assert 0 < auto["lds_bytes"] <= 160 * 1024
        # decode_route's formula: units = B * row blocks, one workgroup per CU, no split shorter than two key tiles
        units = B * blocks
        assert 1 <= auto["num_splits"] <= max(1, min(CAP, tiles // 2)), auto
        if units >= 256 or tiles < 4:
            assert auto["num_splits"] == 1, auto
        assert (auto["combine_grid"], auto["combine_threads"]) == ((B * H * Sq, 256) if auto["num_splits"] > 1 else (0, 0))
        for ns in (1, 2, 3, CAP):
            got = fa.mla_decode_plan(B, H, Sq, Sk, num_splits=ns)
            assert got["num_splits"] == ns and got["grid"] == units * ns and got["row_blocks"] == blocks
            need = int(L.flash_attention_mla_decode_workspace_size(B, H, Sq, 512, ns))
            assert need == fa.decode_workspace_size(B, H, Sq, 512, ns)
            rows = B * H * Sq
            assert need == (0 if ns == 1 else -(-rows * ns * 512 * 4 // 16) * 16 + -(-rows * ns * 4 // 16) * 16)
        for o in (F32, BF16, F16):
            assert fa.mla_decode_plan(B, H, Sq, Sk, o_dtype=o) == auto
    # the benchmark's shapes on 256 CUs (the count the plan assumes without a device)
    assert fa.mla_decode_plan(1, 16, 1, 32768)["num_splits"] == 64 and fa.mla_decode_plan(128, 128, 1, 4096)["num_splits"] == 1
    assert fa.mla_decode_plan(32, 16, 1, 8192)["num_splits"] in (8, 16)
    p = fa.FaDecodePlan()
    rc = lambda *a, plan=p: L.flash_attention_mla_decode_plan(*a, ctypes.byref(plan) if plan is not None else None)
    assert rc(2, 8, 4, 384, 512, 64, F32, 0) == 0 and rc(2, 8, 4, 384, 512, 64, F32, 0, plan=None) == NULL_POINTER
    for a in ((0, 8, 4, 384, 512, 64, F32, 0), (2, 0, 4, 384, 512, 64, F32, 0), (2, 8, 0, 384, 512, 64, F32, 0), (2, 8, 17, 384, 512, 64, F32, 0),
              (2, 8, 4, 0, 512, 64, F32, 0), (2, 8, 4, (1 << 24) + 1, 512, 64, F32, 0), (2, 8, 4, 384, 0, 64, F32, 0),
              (2, 8, 4, 384, 512, 64, F32, -1), (2, 8, 4, 384, 512, 64, F32, CAP + 1), (1 << 16, 256, 1, 384, 512, 64, F32, 64)):
        assert rc(*a) == BAD_SHAPE, a
    assert rc(2, 8, 4, 384, 256, 64, F32, 0) == BAD_DHEAD and rc(2, 8, 4, 384, 512, 128, F32, 0) == BAD_DHEAD
    assert rc(2, 8, 4, 384, 512, 64, FP8, 0) == BAD_DTYPE and rc(2, 8, 4, 384, 256, 64, 7, 0) == BAD_DTYPE


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    bf = torch.bfloat16
    q = torch.zeros(2, 8, 3, 576, dtype=bf)
    kv = torch.zeros(2, 64, 576, dtype=bf)
    pool = torch.zeros(9, 16, 576, dtype=bf)
    table = torch.zeros(2, 3, dtype=torch.int32)
    contig = lambda **kw: fa.flash_attention_mla_decode(kw.pop("Q", T(q)), kw.pop("KV", T(kv)), **kw)
    paged = lambda **kw: fa.flash_attention_mla_decode_paged(kw.pop("Q", T(q)), kw.pop("KV", T(pool)), kw.pop("table", T(table)), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_mla_decode(q, kv)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_mla_decode_paged(T(q), T(pool), table)
    for wrong in (T(torch.zeros(2, 8, 3, 512, dtype=bf)), T(torch.zeros(2, 8, 576, dtype=bf)), T(torch.zeros(3, 8, 3, 576, dtype=bf))):
        with pytest.raises(ValueError, match=r"Q must be \[B, H, Sq, 576\] and KV \[B, capacity, 576\]"):
            contig(Q=wrong)
    for wrong in (T(torch.zeros(2, 64, 512, dtype=bf)), T(torch.zeros(2, 1, 64, 576, dtype=bf)), T(torch.zeros(3, 64, 576, dtype=bf))):
        with pytest.raises(ValueError, match=r"Q must be \[B, H, Sq, 576\]"):
            contig(KV=wrong)
    with pytest.raises(ValueError, match=r"KV_pool \[P, page, 576\]"):
        paged(KV=T(torch.zeros(9, 1, 16, 576, dtype=bf)))
    for wrong in (torch.float16, torch.float32):
        with pytest.raises(TypeError, match="Q, KV must share a dtype"):
            contig(KV=T(kv.to(wrong)))
    with pytest.raises(ValueError, match="last dimension must be contiguous"):
        contig(KV=T(torch.zeros(2, 576, 64, dtype=bf).transpose(1, 2)))
    for t in (T(table.long()), T(torch.zeros(3, 3, dtype=torch.int32)), T(torch.zeros(2, 0, dtype=torch.int32)), T(torch.zeros(6, dtype=torch.int32))):
        with pytest.raises(ValueError, match="block_table must be an int32 device tensor"):
            paged(table=t)
    for front in (contig, paged):
        for lens in (torch.zeros(2, dtype=torch.int32), T(torch.zeros(2, dtype=torch.int64)), T(torch.zeros(3, dtype=torch.int32))):
            with pytest.raises(ValueError, match="kv_lens must be a dense int32 device tensor"):
                front(kv_lens=lens)
        for ns in (-1, CAP + 1):
            with pytest.raises(fa.FlashAttentionError) as e:
                front(num_splits=ns)
            assert e.value.code == BAD_SHAPE
        with pytest.raises(TypeError, match="window"):                     # not done: windows, sinks
            front(window=16)
        with pytest.raises(TypeError, match="sinks"):
            front(sinks=None)
        with pytest.raises(fa.FlashAttentionError) as e:
            front(Q=T(torch.zeros(2, 8, 17, 576, dtype=bf)))
        assert e.value.code == BAD_SHAPE
    assert fa.MLA_D_LATENT == 512 and fa.MLA_D_ROPE == 64
    assert "576 ** -0.5" in fa.flash_attention_mla_decode.__doc__ and "576 ** -0.5" in fa.flash_attention_mla_decode_paged.__doc__


# ---- the emulation and the reference ----
def test_the_emulation_is_within_half_the_tolerance_on_every_gpu_input():
    """mla_check.parity_cases() are the GPU parity tests' inputs: the emulation -- the kernel's arithmetic up to summation order --
    at half of 1e-3 + 1e-3 |ref| (O) and of 2e-4 + 2e-6 |ref| (LSE) on every one, under every split count the GPU test forces."""
    torch = pytest.importorskip("torch")
    import kv_cache_check as kc
    import mla_check as mc
    worst, n = [0.0, 0.0], 0
    for H, Sq, Q, KV, lens, causal, page in mc.parity_cases():
        refO, refL = mc.reference(Q, KV, lens, causal)
        for ns in (1, 3) if H * Sq > 64 else (1, 2, 3, 64):
            O, lse = mc.emulate(Q, KV, lens, causal, ns=ns)
            assert torch.isfinite(O).all() and torch.isfinite(lse).all()
            r, lr = kc.ratios(O, lse, refO, refL)
            worst = [max(worst[0], r.max().item()), max(worst[1], lr.max().item())]
            assert r.max() <= 0.5 and lr.max() <= 0.5, (H, Sq, lens, causal, ns, r.max().item(), lr.max().item())
            n += 1
    print(f"{n} emulations, worst O ratio {worst[0]:.4f}, worst LSE ratio {worst[1]:.4f}")
    assert n >= 100
    for name, scale, Q, KV, lens in mc.scale_cases():
        for causal in (False, True):
            O, lse = mc.emulate(Q, KV, lens, causal, scale=scale, ns=2)
            mc.assert_close_with_score_noise(O, lse, Q, KV, lens, causal, scale, f"emulation, scale {name}, causal {causal}")


def test_single_weights_miss_the_tolerance_on_a_short_cache():
    """why the lo product stays: with the weights rounded to bf16 once (FA_MLA_SINGLE_WEIGHTS) the emulation misses 1e-3 + 1e-3 |ref| on
    caches of a handful of keys -- with the hi + lo pair it is within a hundredth of it"""
    torch = pytest.importorskip("torch")
    import kv_cache_check as kc
    import mla_check as mc
    Q, KV = mc.data(16, 1, 4300)
    lens = [2, 3, 5]
    refO, refL = mc.reference(Q, KV, lens, False)
    r2, _ = kc.ratios(*mc.emulate(Q, KV, lens, False), refO, refL)
    r1, _ = kc.ratios(*mc.emulate(Q, KV, lens, False, single_weights=True), refO, refL)
    print(f"hi + lo: worst ratio {r2.max().item():.4f}; single weights: {r1.max().item():.3f}")
    assert r2.max() < 0.05 and r1.max() > 1


NAMED_ROWS = {"rope columns left out of the score": (0, 0, 0), "V taken from columns 64 to 575": (1, 1, 1), "a top-left mask": (2, 2, 0),
              "packed rows as i * H + h": (0, 1, 0), "a split's LSE ignored in the combine": (1, 3, 2)}


def test_the_reference_refuses_five_wrong_implementations_each_on_a_named_row():
    """B = 3, H = 4, Sq = 3, lengths (40, 129, 300), causal, N(0, 1) bf16 data, the default scale.  Each emulation is one wrong way to
    compute the call in float64 and must miss kv_cache_check.assert_close's bounds on the row named here (sequence, head, query row)."""
    torch = pytest.importorskip("torch")
    import kv_cache_check as kc
    import mla_check as mc
    H, Sq, lens = 4, 3, [40, 129, 300]
    Q, KV = mc.data(H, Sq, 4242)
    refO, refL = mc.reference(Q, KV, lens, True)

    def repacked():
        O, lse = refO.clone(), refL.clone()
        for h, i in itertools.product(range(H), range(Sq)):
            pr = h * Sq + i
            O[:, h, i], lse[:, h, i] = refO[:, pr % H, pr // H], refL[:, pr % H, pr // H]
        return O, lse

    def halves_averaged():
        part = lambda lo, hi: mc.reference(Q, KV, lens, True, vis=lambda b, L: kc.visible(L, Sq, True) & (torch.arange(L)[None] * 2 >= lo * L)
                                           & (torch.arange(L)[None] * 2 < hi * L))
        (O0, l0), (O1, l1) = part(0, 1), part(1, 2)
        return (O0 + O1) / 2, torch.logsumexp(torch.stack([l0, l1]), 0)

    # the two halves merged WITH their LSEs are the reference: the emulation below differs from it by the weights alone
    (O0, l0), (O1, l1) = (mc.reference(Q, KV, lens, True, vis=lambda b, L, s=s: kc.visible(L, Sq, True) & ((torch.arange(L)[None] * 2 >= L) == s))
                          for s in (False, True))
    lse = torch.logsumexp(torch.stack([l0, l1]), 0)
    merged = O0 * (l0 - lse).exp()[..., None] + O1 * (l1 - lse).exp()[..., None]
    assert (merged - refO).abs().max() < 1e-12 and (lse - refL).abs().max() < 1e-12
    wrong = {
        "rope columns left out of the score": lambda: mc.reference(Q, KV, lens, True, score_cols=mc.DL),
        "V taken from columns 64 to 575": lambda: mc.reference(Q, KV, lens, True, v_lo=mc.DR),
        "a top-left mask": lambda: mc.reference(Q, KV, lens, True, vis=lambda b, L: torch.arange(L)[None] <= torch.arange(Sq)[:, None]),
        "packed rows as i * H + h": repacked,
        "a split's LSE ignored in the combine": halves_averaged,
    }
    assert sorted(wrong) == sorted(NAMED_ROWS) and len(wrong) == 5
    for name, run in wrong.items():
        O, lse = run()
        r, lr = kc.ratios(O, lse, refO, refL)
        off = (r > 1).any(-1) | (lr > 1)
        print(f"{name}: {int(off.sum())} of {off.numel()} rows outside the bounds; worst O {r.max().item():.0f} x, LSE {lr.max().item():.0f} x;"
              f" first {tuple(off.nonzero()[0].tolist()) if off.any() else None}")
        with pytest.raises(AssertionError):
            kc.assert_close(O, lse, refO, refL, name)
        b, h, i = NAMED_ROWS[name]
        with pytest.raises(AssertionError):
            kc.assert_close(O[b, h, i], lse[b, h, i], refO[b, h, i], refL[b, h, i], f"{name}, row {NAMED_ROWS[name]}")
