"""CPU tests of attention sinks in the K/V-cache calls (flash_attention_sink_decode, _decode_paged, _extend, _extend_paged, _extend_varlen,
_extend_paged_varlen) at the C ABI, in the binding and in the tests' own reference (sink_check.py):

* the six symbols are exported and declared, each with the parameter list of its _window twin and ``sinks`` directly after vDescale, and
  none of them starts with flash_attention_decode or flash_attention_extend;
* every refusal of the twin comes back with the twin's code, with sinks NULL and with a valid pointer (fake aligned host pointers: no GPU
  is touched; no call here is valid as a whole), and a sinks pointer that is not 4-byte aligned is FA_ERR_MISALIGNED at its stated place;
* the Python fronts raise on a sinks tensor that is on the CPU, not fp32, of the wrong shape, or strided;
* sink_check.apply_sinks (the closed form on top of the existing references) equals a brute-force float64 softmax with one explicit extra
  zero-value column;
* the helper REFUSES four wrong implementations emulated in float64 -- by how much, as measured here, is in each test's docstring.
"""
import ctypes
import itertools

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, aligned_host_pointer, declared_parameters, host_call)

# the sink entry point -> its _window twin
TWINS = {
    "flash_attention_sink_decode": "flash_attention_decode_window",
    "flash_attention_sink_decode_paged": "flash_attention_decode_paged_window",
    "flash_attention_sink_extend": "flash_attention_extend_window",
    "flash_attention_sink_extend_paged": "flash_attention_extend_paged_window",
    "flash_attention_sink_extend_varlen": "flash_attention_extend_varlen_window",
    "flash_attention_sink_extend_paged_varlen": "flash_attention_extend_paged_varlen_window",
}
UNSET = object()


def test_the_six_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    assert sorted(fa._SINK_SYMBOLS.values()) == sorted(TWINS)
    for name, twin in TWINS.items():
        assert name in fa.EXPORTS and getattr(L, name) is not None
        assert not name.startswith(("flash_attention_decode", "flash_attention_extend"))
        want = declared_parameters(twin)
        at = want.index("vDescale") + 1
        want.insert(at, "sinks")
        assert declared_parameters(name) == want, name
        types = list(getattr(L, twin).argtypes)
        types.insert(at, ctypes.c_void_p)
        assert list(getattr(L, name).argtypes) == types, name
        assert getattr(L, name).restype is ctypes.c_int
    # the count that tests/test_split_fronts.py pins is untouched
    split = [s for s in fa.EXPORTS if s.startswith(("flash_attention_decode", "flash_attention_extend")) and "plan" not in s
             and "workspace" not in s]
    assert len(split) == 14


def calls(kv):
    """{sink entry point: call(W, sinks, **overrides)} on an aligned host pointer.  sinks = UNSET calls the _window twin.  Every call is
    valid but for its workspace: two splits and none given, so that passing every other check ends at NULL_POINTER"""
    host = aligned_host_pointer()
    ok = dict(B=2, H=8, Hkv=2, Sk=1024, P=64, page=64, maxp=16, ts=16, d=128, scale=0.125, causal=True, dtype=BF16, kv=kv, o=F32, ns=2)

    def make(name):
        sink = host_call(name, dict(ok, Sq=4 if "decode" in name else 300), host)[0]
        return lambda W, sinks, **kw: sink(symbol=TWINS[name], W=W, **kw) if sinks is UNSET else sink(W=W, sinks=sinks, **kw)

    return {name: make(name) for name in TWINS}, host[1]


def ladder(p, paged, ragged, decode):
    """the arguments the twins refuse (and a few they accept up to the workspace check), as keyword overrides"""
    out = [dict()]
    for name in ("Q", "K", "V", "O"):
        out += [{name: None}, {name: p + 8}]
    out += [dict(LSE=p + 4), dict(ws=p + 8), dict(lens=p + 2), dict(lens=p + 2, Sq=0), dict(Q=None, O=p + 8)]
    out += [dict(ws=p, **kw) for kw in (dict(Sq=0), dict(Sq=-1), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0),
                                        dict(Hkv=16), dict(ns=-1), dict(ns=CAP + 1), dict(Sq=(1 << 31) - 1))]
    # (a workspace is only ever passed with an argument that is invalid in that form: nothing here may reach a launch)
    if ragged:      # totalQ is not capped by the capacity; the batch is
        out += [dict(Sq=1025), dict(Sq=5000), dict(ws=p, B=fa.FA_VARLEN_MAX_BATCH + 1)]
    else:
        out += [dict(ws=p, Sq=1025), dict(ws=p, Sq=5000)]
    out += [dict(ws=p, Sq=17)] if decode else [dict(Sq=17), dict(Sq=1024)]
    out += [dict(Sq=s) for s in (1, 16)]
    out += [dict(o=FP8), dict(o=7), dict(dtype=F32), dict(dtype=FP8), dict(dtype=9), dict(kv=F32), dict(kv=F16), dict(kv=-1),
            dict(kv=F16, d=96), dict(dtype=F32, ns=-1)]
    out += [dict(d=d) for d in (96, 32, 256)]
    out += [dict(scale=s) for s in (0.0, -0.5, float("nan"), float("inf"))]
    out += [dict(kd=p), dict(vd=p + 8), dict(kd=p + 4, vd=p + 12), dict(kd=p + 1), dict(vd=p + 2), dict(kd=p, Q=None)]
    if ragged:
        out += [dict(cu=None), dict(cu=p + 2), dict(cu=p + 1)]
    if paged:
        out += [dict(table=None), dict(table=p + 2)]
        out += [dict(ws=p, **kw) for kw in (dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),
                                            dict(ts=15), dict(ts=-16))]
    else:
        out += [dict(ws=p, **kw) for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1))]
        out += [dict(Sk=1 << 24)]
    return out


@pytest.mark.parametrize("W", [0, 128])
@pytest.mark.parametrize("kv", [BF16, FP8])
def test_the_twins_ladder_with_the_twins_codes(kv, W):
    """every rung through the twin, through the sink entry point with sinks = NULL, and with a valid sinks pointer: one code"""
    # (the pointers are host memory and there may be no device: anything but a validation code would mean a launch was tried)
    fns, p = calls(kv)
    bad = fa.FaStrides(64, 16, 8)            # strideS < d
    mis = fa.FaStrides(1024, 66, 66)         # d = 64: rows that are no multiples of 16 bytes
    for name, call in fns.items():
        assert call(W, UNSET) == call(W, None) == call(W, p + 64) == NULL_POINTER, name     # valid but for the workspace of its two splits
        for kw in ladder(p, "paged" in name, "varlen" in name, "decode" in name):
            want = call(W, UNSET, **kw)
            assert NULL_POINTER >= want >= BAD_STRIDE, (name, kw, want)
            assert call(W, None, **kw) == want and call(W, p + 64, **kw) == want, (name, kw)
        for i in range(4):
            for s in (bad, mis):
                st = [None] * 4
                st[i] = ctypes.byref(s)
                assert call(W, p + 64, strides=st, d=64) == call(W, UNSET, strides=st, d=64) == BAD_STRIDE, (name, i)
        # a few of the ladder's codes spelled out, and the window's own
        assert call(W, p + 64, Q=None) == NULL_POINTER and call(W, p + 64, K=p + 8) == MISALIGNED
        assert call(W, p + 64, ws=p, ns=CAP + 1) == BAD_SHAPE and call(-1, p + 64, ws=p) == BAD_SHAPE
        assert call(W, p + 64, d=96) == BAD_DHEAD and call(W, p + 64, dtype=F32) == BAD_DTYPE and call(W, p + 64, scale=0.0) == BAD_SCALE
        assert call(W, p + 64, kd=p) == (NULL_POINTER if kv == FP8 else BAD_DTYPE)


@pytest.mark.parametrize("kv", [BF16, FP8])
def test_a_misaligned_sinks_pointer_is_refused_at_its_place(kv):
    """FA_ERR_MISALIGNED, directly after the alignment checks of kvLens, cuSeqlensQ, blockTable and the descales: behind the entry
    point's own descale check and the NULL checks, ahead of the paging geometry, the shape, the types, the scale and the strides"""
    fns, p = calls(kv)
    bad = fa.FaStrides(64, 16, 8)
    for name, call in fns.items():
        for r in range(1, 8):
            assert call(0, p + 64 + r) == (MISALIGNED if r % 4 else NULL_POINTER), (name, r)
        s = p + 66
        assert call(128, s) == MISALIGNED and call(128, s, ws=p) == MISALIGNED, name
        # behind ...
        assert call(128, s, Q=None) == NULL_POINTER and call(128, s, V=None) == NULL_POINTER, name
        if kv == BF16:
            assert call(128, s, kd=p) == BAD_DTYPE, name
        if "paged" in name:
            assert call(128, s, table=None) == NULL_POINTER, name
        if "varlen" in name:
            assert call(128, s, cu=None) == NULL_POINTER, name
        # ... ahead of
        for kw in (dict(Sq=0), dict(B=0), dict(Hkv=3), dict(ns=-1), dict(dtype=F32), dict(o=7), dict(d=96), dict(kv=F16 if kv == FP8 else F32),
                   dict(scale=0.0), dict(strides=[ctypes.byref(bad), None, None, None], d=64)):
            if kv == BF16 and "kv" in kw:
                continue
            assert call(128, s, ws=p, **kw) == MISALIGNED, (name, kw)
        if "paged" in name:
            assert call(128, s, ws=p, page=24) == MISALIGNED and call(128, s, ws=p, ts=15) == MISALIGNED, name
        else:
            assert call(128, s, ws=p, Sk=0) == MISALIGNED, name
        assert call(-1, s, ws=p) == MISALIGNED, name


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    H = 8
    qd = torch.zeros(2, H, 4, 64, dtype=torch.bfloat16)
    q = torch.zeros(2, H, 40, 64, dtype=torch.bfloat16)
    qt = torch.zeros(40, H, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 64, 64, dtype=torch.bfloat16)
    pool = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 3, dtype=torch.int32)
    cu = torch.tensor([0, 30, 40], dtype=torch.int32)
    fronts = {
        "flash_attention_decode": (T(qd), T(k), T(k)),
        "flash_attention_decode_paged": (T(qd), T(pool), T(pool), T(table)),
        "flash_attention_extend": (T(q), T(k), T(k)),
        "flash_attention_extend_window": (T(q), T(k), T(k)),
        "flash_attention_extend_paged": (T(q), T(pool), T(pool), T(table)),
        "flash_attention_extend_paged_window": (T(q), T(pool), T(pool), T(table)),
        "flash_attention_extend_varlen": (T(qt), T(k), T(k), T(cu)),
        "flash_attention_extend_varlen_window": (T(qt), T(k), T(k), T(cu)),
        "flash_attention_extend_paged_varlen": (T(qt), T(pool), T(pool), T(table), T(cu)),
        "flash_attention_extend_paged_varlen_window": (T(qt), T(pool), T(pool), T(table), T(cu)),
    }
    good = torch.zeros(H)
    wrong = {
        "on the CPU": good,
        "bf16": T(good.to(torch.bfloat16)),
        "float64": T(good.double()),
        "[H + 1]": T(torch.zeros(H + 1)),
        "[Hkv]": T(torch.zeros(2)),
        "[1, H]": T(good[None]),
        "strided": T(torch.zeros(2 * H)[::2]),
        "on another device": T(good, device="cuda:1"),
        "a list": [0.0] * H,
    }
    for front, args in fronts.items():
        for what, sinks in wrong.items():
            with pytest.raises(ValueError, match="sinks"):
                getattr(fa, front)(*args, sinks=sinks)
            if front.endswith("_window") or "decode" in front:
                with pytest.raises(ValueError, match="sinks"):
                    getattr(fa, front)(*args, window=16, sinks=sinks)
    # the tensors' own checks come first, as without sinks
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_decode(qd, k, k, sinks=T(good))
    with pytest.raises(ValueError, match="window"):
        fa.flash_attention_decode(T(qd), T(k), T(k), window=-1, sinks=T(good))


# ---- the reference ----
LENGTHS = ((1, 300), (129, 300), (127, 128))
ROWS = (1, 16, 40)


def test_the_closed_form_is_a_softmax_with_one_more_zero_valued_column():
    torch = pytest.importorskip("torch")
    import sink_check as sc
    worst = 0.0
    for (d, G), Sq in itertools.product(((64, 4), (128, 1)), ROWS):
        Q, K, V = sc.data(d, G, Sq, 100 + d + Sq)
        sinks = sc.sinks_for(sc.HKV * G)
        for lens, causal, W in itertools.product(LENGTHS, (False, True), sc.WINDOWS):
            O2, lse2, O, lse = sc.reference_sinks(Q, K, V, lens, causal, W, sinks)
            bO, bL = sc.brute_force(Q, K, V, lens, causal, W, sinks)
            assert torch.isfinite(O2).all() and torch.isfinite(lse2).all()
            worst = max(worst, (O2 - bO).abs().max().item(), (lse2 - bL).abs().max().item())
            share = sc.assert_sinks_matter(lse2, sinks, what=f"d{d} G{G} Sq{Sq} {lens} causal{causal} W{W}")
            assert share <= 0.95
            # -inf is no sink: the head keeps the reference's own values
            gone = torch.isinf(sinks)
            assert torch.equal(O2[:, gone], O[:, gone]) and torch.equal(lse2[:, gone], lse[:, gone])
    print(f"closed form against brute force: worst difference {worst:.2e}")
    assert worst < 1e-12        # float64 against float64: rounding only


def wrong_implementations(sc, torch, Q, K, V, lens, causal, W, sinks, G):
    """{name: (O, LSE)} of four wrong ways to add a sink, in float64"""
    out = {}
    scale = 1.0 / Q.shape[-1] ** 0.5
    # the sink counted once per split: three splits of whole 128-key tiles, each with the sink in its partial result, combined by LSE
    Bq, H, Sq, d = Q.shape
    O, lse = torch.zeros(Bq, H, Sq, d, dtype=torch.float64), torch.zeros(Bq, H, Sq, dtype=torch.float64)
    for b in range(Bq):
        L = int(lens[b])
        S = sc.scores(Q[b], K[b], L, causal, W)
        v = V[b, :, :L].double().repeat_interleave(G, 0)
        nt = -(-L // 128)
        parts = []
        for s in range(3):
            k0, k1 = min(128 * (nt * s // 3), L), min(128 * (nt * (s + 1) // 3), L)
            Ss = torch.cat([S[..., k0:k1], sinks.double()[:, None, None].expand(H, Sq, 1)], -1)
            m = torch.logsumexp(Ss, -1)
            parts.append((m, (torch.exp(Ss[..., :-1] - m[..., None]) @ v[:, k0:k1])))
        lse[b] = torch.logsumexp(torch.stack([m for m, _ in parts]), 0)
        O[b] = sum(torch.exp(m - lse[b])[..., None] * o for m, o in parts)
    out["the sink counted once per split (3 splits)"] = (O, lse)
    out["the sink multiplied by scale"] = sc.reference_sinks(Q, K, V, lens, causal, W, sinks * scale)[:2]
    out["the sink indexed by K/V head"] = sc.reference_sinks(Q, K, V, lens, causal, W, sinks[:sc.HKV].repeat_interleave(G))[:2]
    plain = sc.reference_sinks(Q, K, V, lens, causal, W, sinks)
    out["the sink dropped when a window is set"] = plain[2:] if W > 0 else plain[:2]
    return out


def test_the_helper_refuses_four_wrong_implementations():
    """Worst error / tolerance (kv_cache_check.assert_close's: O 1e-3 + 1e-3 |ref|, LSE 2e-4 + 2e-6 |ref|) of each emulation against the
    reference, the SMALLEST over the cases below (Sq 1 / 16 / 40, the three length pairs, causal and not, windows 0 / 7 / 130; the windowed ones only
    for the last) -- measured here, d = 64,
    G = 4, N(0, 1) bf16 data, scale 1/8, SINKS8:
        the sink counted once per split (3 splits)    O 71 x,   LSE 4803 x the tolerance
        the sink multiplied by scale                  O 307 x,  LSE 11209 x
        the sink indexed by K/V head                  O 309 x,  LSE 11236 x
        the sink dropped when a window is set         O 328 x,  LSE 13060 x
    The test asks for 10 x on both, far below any of them and far above rounding."""
    torch = pytest.importorskip("torch")
    import sink_check as sc
    d, G = 64, 4
    least = {}
    for Sq in ROWS:
        Q, K, V = sc.data(d, G, Sq, 200 + Sq)
        sinks = sc.sinks_for(sc.HKV * G)
        for lens, causal, W in itertools.product(LENGTHS, (False, True), sc.WINDOWS):
            refO, refL = sc.reference_sinks(Q, K, V, lens, causal, W, sinks)[:2]
            for name, (O, lse) in wrong_implementations(sc, torch, Q, K, V, lens, causal, W, sinks, G).items():
                if "window" in name and W == 0:
                    assert sc.excess(O, lse, refO, refL) == (0.0, 0.0)      # (the mistake cannot show without a window)
                    continue
                eo, el = sc.excess(O, lse, refO, refL)
                lo = least.setdefault(name, [eo, el])
                lo[0], lo[1] = min(lo[0], eo), min(lo[1], el)
    assert len(least) == 4
    for name, (eo, el) in least.items():
        print(f"{name}: O {eo:.0f} x, LSE {el:.0f} x the tolerance at the least")
        assert eo > 10 and el > 10, name
