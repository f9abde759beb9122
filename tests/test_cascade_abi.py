"""CPU tests of shared-prefix (cascade) decode (flash_attention_cascade_decode, _cascade_decode_paged, flash_attention_cascade_plan) at
the C ABI, in the binding and in the tests' own reference (cascade_check.py):

* the three symbols are exported with the declared signatures;
* every refusal of flash_attention_decode_window / _paged_window comes back from the cascade call of the same form with the twin's code
  (fake aligned host pointers: no GPU is touched; no call here is valid as a whole), and the refusals the calls add stand at their
  places: NULL Kshared / Vshared / sharedTable with the other pointers, a NULL workspace where decode asks for its own, sharedLen and
  sinks not 4-byte aligned with the arrays, the shared capacity, maxSharedPages and the split counts in the shape step;
* plan properties: unique.num_splits >= 2, the sum <= FA_DECODE_MAX_SPLITS, forced values returned as given, the workspace size is
  flash_attention_decode_workspace_size at the sum;
* the Python fronts' refusals;
* the reference equals kv_cache_check.reference(causal=True) on the concatenation whenever len_b >= Sq, and it REFUSES five wrong
  implementations emulated in float64, each on a named row.
"""
import ctypes
import itertools

import pytest

import __graft_entry__ as entry

fa = entry.load_package()

import kv_cache_check as kv  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SCALE, BAD_SHAPE, BAD_STRIDE, BF16, CAP, F16, F32, FP8, MISALIGNED,  # noqa: E402
                      NULL_POINTER, MetaTensor as T, aligned_host_pointer, c_call, declared_parameters)

TWINS = {"flash_attention_cascade_decode": "flash_attention_decode_window",
         "flash_attention_cascade_decode_paged": "flash_attention_decode_paged_window"}
# short key -> the header's name, for what the cascade calls declare beyond their twins (the twins' keys: abi_decl.KEYS)
NEW = {"Ks": "Kshared", "Vs": "Vshared", "sl": "sharedLen", "st": "sharedTable", "Ls": "seqLenShared", "maxsp": "maxSharedPages",
       "nss": "numSplitsShared", "ns": "numSplitsUnique", "sKs": "sKshared", "sVs": "sVshared"}
OLD = {"Q": "Q", "K": ("K", "Kpool"), "V": ("V", "Vpool"), "O": "O", "LSE": "LSE", "lens": "kvLens", "table": "blockTable", "kd": "kDescale",
       "vd": "vDescale", "sinks": "sinks", "ws": "workspace", "B": "batchSize", "H": "numHeads", "Hkv": "numHeadsKV", "Sq": "seqLenQ",
       "Sk": "seqLenK", "P": "numPages", "page": "pageSize", "maxp": "maxPagesPerSeq", "ts": "tableStride", "d": "dHead", "scale": "scale",
       "causal": "is_causal", "dtype": "dtype", "kv": "kv_dtype", "o": "o_dtype", "sQ": "sQ", "sK": "sK", "sV": "sV", "sO": "sO",
       "stream": "stream"}


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    vp, i, f, b, sp = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_bool, ctypes.POINTER(fa.FaStrides)
    assert sorted(fa._CASCADE_SYMBOLS.values()) == sorted(TWINS)
    want = {
        "flash_attention_cascade_decode": [
            ("Q", vp), ("Kshared", vp), ("Vshared", vp), ("K", vp), ("V", vp), ("O", vp), ("LSE", vp), ("sharedLen", vp), ("kvLens", vp),
            ("kDescale", vp), ("vDescale", vp), ("sinks", vp), ("workspace", vp), ("batchSize", i), ("numHeads", i), ("numHeadsKV", i),
            ("seqLenQ", i), ("seqLenShared", i), ("seqLenK", i), ("dHead", i), ("scale", f), ("is_causal", b), ("dtype", i), ("kv_dtype", i),
            ("o_dtype", i), ("numSplitsShared", i), ("numSplitsUnique", i), ("sQ", sp), ("sKshared", sp), ("sVshared", sp), ("sK", sp),
            ("sV", sp), ("sO", sp), ("stream", vp)],
        "flash_attention_cascade_decode_paged": [
            ("Q", vp), ("Kpool", vp), ("Vpool", vp), ("O", vp), ("LSE", vp), ("sharedLen", vp), ("kvLens", vp), ("sharedTable", vp),
            ("blockTable", vp), ("kDescale", vp), ("vDescale", vp), ("sinks", vp), ("workspace", vp), ("batchSize", i), ("numHeads", i),
            ("numHeadsKV", i), ("seqLenQ", i), ("numPages", i), ("pageSize", i), ("maxSharedPages", i), ("maxPagesPerSeq", i),
            ("tableStride", ctypes.c_int64), ("dHead", i), ("scale", f), ("is_causal", b), ("dtype", i), ("kv_dtype", i), ("o_dtype", i),
            ("numSplitsShared", i), ("numSplitsUnique", i), ("sQ", sp), ("sK", sp), ("sV", sp), ("sO", sp), ("stream", vp)],
        "flash_attention_cascade_plan": [(n, i) for n in ("batchSize", "numHeads", "numHeadsKV", "seqLenQ", "seqLenShared", "seqLenK", "dHead",
                                                           "o_dtype", "numSplitsShared", "numSplitsUnique")]
        + [("plan", ctypes.POINTER(fa.FaCascadePlan))],
    }
    for name, params in want.items():
        assert name in fa.EXPORTS and getattr(L, name) is not None
        assert declared_parameters(name) == [n for n, _ in params], name
        assert list(getattr(L, name).argtypes) == [t for _, t in params], name
        assert getattr(L, name).restype is i
    # what distinguishes a call from its _window twin: the shared tensors, sharedLen, the shared table, sinks, two split counts, no window
    for name, twin in TWINS.items():
        gone = set(declared_parameters(twin)) - set(declared_parameters(name))
        assert gone == {"numSplits", "windowSize"}, (name, gone)
    assert [k for k, _ in fa.FaCascadePlan._fields_] == ["shared", "unique", "num_splits"]
    # the count that tests/test_split_fronts.py pins is untouched
    split = [s for s in fa.EXPORTS if s.startswith(("flash_attention_decode", "flash_attention_extend")) and "plan" not in s
             and "workspace" not in s]
    assert len(split) == 14


def calls(kvt):
    """{cascade entry point: call(twin=False, **overrides)} on an aligned host pointer p, and p.  Every call is valid but for its workspace,
    so that passing every other check ends at NULL_POINTER.  twin=True: the _window twin on the twin's share of the arguments (ns is
    numSplitsUnique / numSplits; windowSize 0)"""
    host = aligned_host_pointer()
    p = host[1]
    ok = dict(Q=p, Ks=p, Vs=p, K=p, V=p, O=p, LSE=None, sl=None, lens=None, st=p, table=p, kd=None, vd=None, sinks=None, ws=None,
              B=2, H=8, Hkv=2, Sq=4, Ls=2048, Sk=1024, P=64, page=64, maxsp=32, maxp=16, ts=16, d=128, scale=0.125, causal=True, dtype=BF16,
              kv=kvt, o=F32, nss=0, ns=2, stream=None)

    def make(name):
        params = declared_parameters(name)

        def call(twin=False, _keep=host, **kw):
            v = dict(ok, **kw)
            strides = v.pop("strides", None)
            if twin:      # (its four strides: Q, K, V, O)
                return c_call(TWINS[name], dict({k: x for k, x in v.items() if k not in NEW or k == "ns"}, W=0,
                                                strides=[None] * 4 if strides is None else strides))
            by_name = {}
            for k, x in v.items():
                names = NEW[k] if k in NEW else OLD[k]
                for n in (names,) if isinstance(names, str) else names:
                    by_name[n] = x
            names = [n for n in params if n in ("sQ", "sKshared", "sVshared", "sK", "sV", "sO")]
            for n, s in zip(names, strides or [None] * len(names)):
                by_name.setdefault(n, s)
            return getattr(fa.lib(), name)(*[by_name[n] for n in params])

        return call

    return {name: make(name) for name in TWINS}, p


def ladder(p, paged):
    """the arguments the _window twins refuse (and a few they accept up to the workspace check), as keyword overrides"""
    out = [dict()]
    for name in ("Q", "K", "V", "O"):
        out += [{name: None}, {name: p + 8}]
    out += [dict(LSE=p + 4), dict(ws=p + 8), dict(lens=p + 2), dict(lens=p + 2, Sq=0), dict(Q=None, O=p + 8)]
    out += [dict(ws=p, **kw) for kw in (dict(Sq=0), dict(Sq=-1), dict(Sq=17), dict(B=0), dict(H=0, Hkv=0), dict(d=0), dict(Hkv=3), dict(Hkv=0),
                                        dict(Hkv=16), dict(ns=-1), dict(ns=CAP + 1))]
    out += [dict(Sq=s) for s in (1, 16)]
    out += [dict(o=FP8), dict(o=7), dict(dtype=F32), dict(dtype=FP8), dict(dtype=9), dict(kv=F32), dict(kv=F16), dict(kv=-1),
            dict(kv=F16, d=96), dict(dtype=F32, ns=-1)]
    out += [dict(d=d) for d in (96, 32, 256)]
    out += [dict(scale=s) for s in (0.0, -0.5, float("nan"), float("inf"))]
    out += [dict(kd=p), dict(vd=p + 8), dict(kd=p + 4, vd=p + 12), dict(kd=p + 1), dict(vd=p + 2), dict(kd=p, Q=None)]
    if paged:
        out += [dict(table=None), dict(table=p + 2)]
        out += [dict(ws=p, **kw) for kw in (dict(P=0), dict(maxp=0), dict(page=8), dict(page=24), dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),
                                            dict(ts=15), dict(ts=-16))]
    else:
        out += [dict(ws=p, **kw) for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1))]
        out += [dict(Sk=1 << 24)]
    return out


@pytest.mark.parametrize("kvt", [BF16, FP8])
def test_the_window_twins_ladder_with_the_twins_codes(kvt):
    fns, p = calls(kvt)
    bad = fa.FaStrides(64, 16, 8)            # strideS < d
    mis = fa.FaStrides(1024, 66, 66)         # d = 64: rows that are no multiples of 16 bytes
    for name, call in fns.items():
        paged = "paged" in name
        assert call() == call(twin=True) == NULL_POINTER, name                         # valid but for the workspace
        for kw in ladder(p, paged):
            want = call(twin=True, **kw)
            assert NULL_POINTER >= want >= BAD_STRIDE, (name, kw, want)
            assert call(**kw) == want, (name, kw, want)
        for i, s in itertools.product(range(4), (bad, mis)):                            # the twin's four strides: Q, K, V, O
            st = [None] * 4
            st[i] = ctypes.byref(s)
            mine = st if paged else [st[0], None, None, st[1], st[2], st[3]]
            assert call(strides=mine, d=64) == call(twin=True, strides=st, d=64) == BAD_STRIDE, (name, i)
        assert call(Q=None) == NULL_POINTER and call(K=p + 8) == MISALIGNED and call(ws=p, ns=CAP + 1) == BAD_SHAPE
        assert call(d=96) == BAD_DHEAD and call(dtype=F32) == BAD_DTYPE and call(scale=0.0) == BAD_SCALE
        assert call(kd=p) == (NULL_POINTER if kvt == FP8 else BAD_DTYPE)


@pytest.mark.parametrize("kvt", [BF16, FP8])
def test_the_new_refusals_at_their_places(kvt):
    fns, p = calls(kvt)
    bad = fa.FaStrides(64, 16, 8)
    for name, call in fns.items():
        paged = "paged" in name
        shape_faults = (dict(Sq=0), dict(B=0), dict(Hkv=3), dict(ns=-1), dict(dtype=F32), dict(o=7), dict(d=96), dict(scale=0.0))
        # NULL shared tensors / table: with the other pointers -- behind the entry point's own descale check, ahead of everything else
        for kw in (dict(st=None),) if paged else (dict(Ks=None), dict(Vs=None)):
            assert call(**kw) == call(ws=p, **kw) == NULL_POINTER, (name, kw)
            assert call(K=p + 8, **kw) == NULL_POINTER and call(lens=p + 2, **kw) == NULL_POINTER, (name, kw)
            for more in shape_faults:
                assert call(ws=p, **kw, **more) == NULL_POINTER, (name, kw, more)
            if kvt == BF16:
                assert call(kd=p, **kw) == BAD_DTYPE, (name, kw)
        # the shared tensors' base alignment: with the other tensors'
        if not paged:
            for kw in (dict(Ks=p + 8), dict(Vs=p + 4)):
                assert call(**kw) == MISALIGNED and call(Q=None, **kw) == NULL_POINTER and call(ws=p, Sq=0, **kw) == MISALIGNED, (name, kw)
        # sharedLen, the shared table and sinks not 4-byte aligned: with the int32 / fp32 arrays, ahead of the geometry and the shape
        arrays = [("sl", p + 64), ("sinks", p + 96)] + ([("st", p + 32)] if paged else [])
        for key, at in arrays:
            for r in range(8):
                assert call(**{key: at + r}) == (MISALIGNED if r % 4 else NULL_POINTER), (name, key, r)
            kw = {key: at + 2}
            assert call(ws=p, **kw) == MISALIGNED and call(Q=None, **kw) == NULL_POINTER and call(O=p + 8, **kw) == MISALIGNED, (name, key)
            for more in shape_faults + ((dict(page=24), dict(maxsp=0)) if paged else (dict(Sk=0), dict(Ls=0))):
                assert call(ws=p, **kw, **more) == MISALIGNED, (name, key, more)
            if kvt == BF16:
                assert call(kd=p, **kw) == BAD_DTYPE, (name, key)
        # the shape step: the shared capacity, maxSharedPages, the split counts -- behind the pointers and the arrays, ahead of the types,
        # the scale and the strides
        shapes = [dict(ns=1), dict(nss=-1), dict(nss=CAP - 1), dict(nss=CAP - 1, ns=0), dict(nss=0, ns=CAP), dict(nss=33, ns=32), dict(nss=CAP + 1)]
        shapes += [dict(maxsp=0), dict(maxsp=-3), dict(maxsp=(1 << 18) + 1)] if paged else [dict(Ls=0), dict(Ls=-5), dict(Ls=(1 << 24) + 1)]
        for kw in shapes:
            assert call(**kw) == call(ws=p, **kw) == BAD_SHAPE, (name, kw)
            assert call(Q=None, **kw) == NULL_POINTER and call(lens=p + 2, **kw) == MISALIGNED, (name, kw)
            for more in (dict(dtype=F32), dict(o=7), dict(d=96), dict(kv=F16), dict(scale=0.0)):
                assert call(ws=p, **kw, **more) == BAD_SHAPE, (name, kw, more)
        # accepted up to the workspace: the largest counts, the largest shared capacity; a shared grid at FA_DECODE_MAX_WORKGROUPS is not
        for kw in (dict(nss=CAP - 2, ns=2), dict(nss=32, ns=32), dict(nss=1, ns=CAP - 1), dict(nss=CAP - 2, ns=0), dict(nss=0, ns=CAP - 1),
                   dict(maxsp=1 << 18) if paged else dict(Ls=1 << 22)):
            assert call(**kw) == NULL_POINTER, (name, kw)
        # the shared grid alone at or above FA_DECODE_MAX_WORKGROUPS: 256 heads x 1280 row blocks x 62 splits (the suffixes' 2 x 20480 x 256
        # workgroups and the 2^23.3 rows of O are below it)
        assert call(B=20480, H=256, Hkv=256, Sq=2, d=64, nss=62) == call(B=20480, H=256, Hkv=256, Sq=2, d=64, nss=62, ws=p) == BAD_SHAPE
        assert call(B=20480, H=256, Hkv=256, Sq=2, d=64, nss=32) == NULL_POINTER
        # a NULL workspace: decode's place for its own, the last rung -- under ANY split counts, the shared part's one split included
        for kw in (dict(nss=1, ns=2), dict(nss=0, ns=0)):
            assert call(**kw) == NULL_POINTER, (name, kw)
            assert call(**kw, strides=[ctypes.byref(bad)] + [None] * (3 if paged else 5), d=64) == BAD_STRIDE, (name, kw)
        # the shared tensors' strides and extents are those of K / V
        if not paged:
            for at in (1, 2):
                st = [None] * 6
                st[at] = ctypes.byref(bad)
                assert call(strides=st, d=64) == BAD_STRIDE and call(strides=st, d=64, scale=0.0) == BAD_SCALE, (name, at)
            wide = fa.FaStrides(0, 1 << 32, 1 << 21)       # 1024 rows x 2^21 elements: 2^31 bytes in one head even at one byte each
            for at in (1, 2, 3, 4):
                st = [None] * 6
                st[at] = ctypes.byref(wide)
                assert call(strides=st, ws=p) == BAD_SHAPE, (name, at)


def test_plan_properties():
    L = fa.lib()
    for (B, H, Hkv), Sq, d, Ls, Sk in itertools.product(((2, 8, 2), (1, 32, 8), (32, 32, 8), (7, 4, 4), (256, 64, 8)), (1, 5, 16), (64, 128),
                                                        (128, 384, 8192, 1 << 20), (128, 256, 32768)):
        auto = fa.cascade_plan(B, H, Hkv, Sq, Ls, Sk, d)
        rpb = 64 if d == 128 else 32
        assert auto["unique"]["num_splits"] >= 2 and auto["shared"]["num_splits"] >= 1
        assert auto["unique"]["num_splits"] <= 32
        assert auto["num_splits"] == auto["shared"]["num_splits"] + auto["unique"]["num_splits"] <= CAP
        assert auto["shared"]["rows_per_block"] == rpb and auto["unique"]["rows_per_block"] == 16
        assert auto["shared"]["row_blocks"] == -(-B * (H // Hkv) * Sq // rpb)
        assert auto["shared"]["grid"] == Hkv * auto["shared"]["row_blocks"] * auto["shared"]["num_splits"]               # no batch factor
        assert auto["shared"]["num_splits"] <= max(1, -(-Ls // 128) // 2)                                                 # extend's min tiles
        assert auto["unique"] == fa.decode_plan(B, H, Hkv, Sq, Sk, d, num_splits=auto["unique"]["num_splits"])
        for forced in ((1, 2), (3, 2), (2, 5), (32, 32), (62, 2), (1, 63)):
            got = fa.cascade_plan(B, H, Hkv, Sq, Ls, Sk, d, num_splits=forced)
            assert (got["shared"]["num_splits"], got["unique"]["num_splits"], got["num_splits"]) == (*forced, sum(forced))
        for ns_s in (1, 40, 62):                      # a chosen unique count makes room for a forced shared one
            got = fa.cascade_plan(B, H, Hkv, Sq, Ls, Sk, d, num_splits=(ns_s, 0))
            assert got["shared"]["num_splits"] == ns_s and 2 <= got["unique"]["num_splits"] <= min(32, CAP - ns_s)
        got = fa.cascade_plan(B, H, Hkv, Sq, Ls, Sk, d, num_splits=(0, 60))
        assert got["unique"]["num_splits"] == 60 and 1 <= got["shared"]["num_splits"] <= 4
        # the workspace is the decode function's at the sum, and never 0
        need = fa.decode_workspace_size(B, H, Sq, d, auto["num_splits"])
        assert need == int(L.flash_attention_decode_workspace_size(B, H, Sq, d, auto["num_splits"])) > 0
    # the benchmark's shape: 32 x 4 packed rows per K/V head are 2 row blocks, 16 units; one workgroup on each of 256 CUs: 16 splits
    big = fa.cascade_plan(32, 32, 8, 1, 8192, 256, 128)
    assert big["shared"]["row_blocks"] == 2 and big["unique"]["num_splits"] == 2 and big["shared"]["num_splits"] in (16, 32)
    # refusals of the plan: the shape step's, with the codes of the calls
    p = fa.FaCascadePlan()
    rc = lambda *a, plan=p: L.flash_attention_cascade_plan(*a, ctypes.byref(plan) if plan is not None else None)
    assert rc(2, 8, 2, 4, 384, 256, 128, F32, 0, 0) == 0
    assert rc(2, 8, 2, 4, 384, 256, 128, F32, 0, 0, plan=None) == NULL_POINTER
    for a in ((2, 8, 2, 4, 0, 256, 128, F32, 0, 0), (2, 8, 2, 4, (1 << 24) + 1, 256, 128, F32, 0, 0), (2, 8, 2, 4, 384, 0, 128, F32, 0, 0),
              (2, 8, 2, 17, 384, 256, 128, F32, 0, 0), (2, 8, 3, 4, 384, 256, 128, F32, 0, 0), (2, 8, 2, 4, 384, 256, 128, F32, 0, 1),
              (2, 8, 2, 4, 384, 256, 128, F32, -1, 0), (2, 8, 2, 4, 384, 256, 128, F32, 0, -1), (2, 8, 2, 4, 384, 256, 128, F32, 33, 32),
              (2, 8, 2, 4, 384, 256, 128, F32, 63, 0), (2, 8, 2, 4, 384, 256, 128, F32, 0, 64), (2, 8, 2, 4, 384, 256, 96, F32, 0, 1)):
        assert rc(*a) == BAD_SHAPE, a
    assert rc(2, 8, 2, 4, 384, 256, 96, F32, 0, 0) == BAD_DHEAD and rc(2, 8, 2, 4, 384, 256, 128, FP8, 0, 0) == BAD_DTYPE


def test_binding_refusals():
    torch = pytest.importorskip("torch")
    bf = torch.bfloat16
    H, Sq, d = 8, 5, 64
    q = torch.zeros(2, H, Sq, d, dtype=bf)
    k = torch.zeros(2, 2, 64, d, dtype=bf)
    ks = torch.zeros(2, 128, d, dtype=bf)
    pool = torch.zeros(9, 2, 16, d, dtype=bf)
    table, stable = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    contig = lambda **kw: fa.flash_attention_cascade_decode(T(q), kw.pop("Ks", T(ks)), kw.pop("Vs", T(ks)), kw.pop("K", T(k)), T(k), **kw)
    paged = lambda **kw: fa.flash_attention_cascade_decode_paged(T(q), T(pool), T(pool), kw.pop("st", T(stable)), T(table), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.flash_attention_cascade_decode(q, ks, ks, k, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contig(Ks=ks)
    with pytest.raises(ValueError, match="Hkv dividing H"):
        contig(K=T(k[:, :, :, :32]))
    for wrong in (T(torch.zeros(3, 128, d, dtype=bf)), T(torch.zeros(2, 128, 32, dtype=bf)), T(torch.zeros(1, 2, 128, d, dtype=bf)),
                  T(torch.zeros(2, 0, d, dtype=bf))):
        with pytest.raises(ValueError, match="K_shared, V_shared must be"):
            contig(Ks=wrong, Vs=wrong)
    with pytest.raises(ValueError, match="K_shared, V_shared must be"):
        contig(Vs=T(torch.zeros(2, 64, d, dtype=bf)))
    # mismatched shared and unique dtypes
    for wrong in (torch.float16, torch.float32) + ((kv.F8,) if kv.F8 is not None else ()):
        with pytest.raises(TypeError, match="K_shared, V_shared, K, V must share a dtype"):
            contig(Ks=T(ks.to(wrong)), Vs=T(ks.to(wrong)))
    for st in (stable, T(stable.long()), T(torch.zeros(1, 3, dtype=torch.int32)), T(torch.zeros(6, dtype=torch.int32)[::2]),
               T(stable, device="cuda:1"), T(torch.zeros(0, dtype=torch.int32)), None):
        with pytest.raises(ValueError, match="shared_table must be a dense int32 device tensor"):
            paged(st=st)
    for front in (contig, paged):
        for sl in (torch.zeros(1, dtype=torch.int32), T(torch.zeros(1, dtype=torch.int64)), T(torch.zeros(2, dtype=torch.int32)),
                   T(torch.zeros(1, dtype=torch.int32), device="cuda:1"), 5):
            with pytest.raises(ValueError, match="shared_len must be an int32 device tensor"):
                front(shared_len=sl)
        with pytest.raises(ValueError, match="kv_lens must be a dense int32 device tensor"):
            front(kv_lens=T(torch.zeros(3, dtype=torch.int32)))
        with pytest.raises(ValueError, match="sinks must be a dense fp32 tensor"):
            front(sinks=T(torch.zeros(H + 1)))
        with pytest.raises(ValueError, match="k_descale belongs to an fp8"):
            front(k_descale=T(torch.zeros(2)))
        for ns in (3, (1,), (1, 2, 3), None, ("a", 2)):
            with pytest.raises(ValueError, match="num_splits must be a pair"):
                front(num_splits=ns)
        for ns in ((0, 1), (-1, 0), (40, 30)):
            with pytest.raises(fa.FlashAttentionError) as e:
                front(num_splits=ns)
            assert e.value.code == BAD_SHAPE
        with pytest.raises(TypeError, match="window"):                     # there is no window argument
            front(window=16)
    q17 = torch.zeros(2, H, 17, d, dtype=bf)
    with pytest.raises(fa.FlashAttentionError) as e:
        fa.flash_attention_cascade_decode(T(q17), T(ks), T(ks), T(k), T(k))
    assert e.value.code == BAD_SHAPE


# ---- the reference ----
def data(torch, B, H, Hkv, Sq, d, Ls, Lu, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g).to(torch.bfloat16)
    return r(B, H, Sq, d), r(Hkv, Ls, d), r(Hkv, Ls, d), r(B, Hkv, Lu, d), r(B, Hkv, Lu, d)


def test_the_reference_is_causal_decode_on_the_concatenation():
    torch = pytest.importorskip("torch")
    import cascade_check as cc
    worst = 0.0
    for (B, H, Hkv, Sq), d in itertools.product(((3, 4, 2, 1), (2, 4, 2, 3), (2, 2, 2, 16)), (64, 128)):
        Q, Ks, Vs, K, V = data(torch, B, H, Hkv, Sq, d, 160, 140, 11 + Sq + d)
        for ls, lens in itertools.product((1, 127, 160), ([Sq, Sq + 1, 140][:B], [129, Sq, 128][:B])):
            O, lse = cc.reference(Q, Ks, Vs, K, V, ls, lens, True)
            Kc, Vc, lens_c = cc.concatenated(Ks, Vs, K, V, ls, lens)
            assert lens_c == [ls + L for L in lens]
            refO, refL = kv.reference(Q, Kc, Vc, lens_c, True)
            worst = max(worst, (O - refO).abs().max().item(), (lse - refL).abs().max().item())
            # not causal: every key of both parts
            O, lse = cc.reference(Q, Ks, Vs, K, V, ls, lens, False)
            refO, refL = kv.reference(Q, Kc, Vc, lens_c, False)
            worst = max(worst, (O - refO).abs().max().item(), (lse - refL).abs().max().item())
    assert worst == 0.0
    # len_b < Sq: the rows clamped to key 0 of the suffix still see the whole prefix -- which causal decode on the concatenation cuts
    Q, Ks, Vs, K, V = data(torch, 2, 4, 2, 3, 64, 160, 140, 5)
    vis = cc.visibility(7, [1, 3], 3, True)
    assert vis(0, 0, 8).tolist() == [[True] * 8] * 3 and vis(1, 0, 10)[:, 7:].tolist() == [[True, False, False], [True, True, False], [True] * 3]
    O, lse = cc.reference(Q, Ks, Vs, K, V, 7, [1, 3], True)
    Kc, Vc, lens_c = cc.concatenated(Ks, Vs, K, V, 7, [1, 3])
    refO, refL = kv.reference(Q, Kc, Vc, lens_c, True)
    assert torch.equal(O[1], refO[1]) and torch.equal(O[0, :, 2], refO[0, :, 2]) and not torch.allclose(lse[0, :, 0], refL[0, :, 0])
    # the clamps of the lengths: 0 and negative are 1, beyond the capacity is the capacity
    a = cc.reference(Q, Ks, Vs, K, V, 0, [-4, 999], False)
    b = cc.reference(Q, Ks, Vs, K, V, 1, [1, 140], False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def merge(torch, parts):
    """the LSE-weighted merge of (O, LSE) partial results, float64"""
    lse = torch.logsumexp(torch.stack([p[1] for p in parts]), 0)
    return sum(p[0] * (p[1] - lse).exp()[..., None] for p in parts), lse


def test_the_reference_refuses_five_wrong_implementations_each_on_a_named_row():
    """B = 3, H = 4, Hkv = 2, Sq = 3, d = 64, ls = 130 of 160, suffix lengths (5, 129, 40), causal, N(0, 1) bf16 data, sinks of
    sink_check.  The two parts' float64 partial results merged with LSE weights ARE the reference (checked first); each emulation is
    one wrong way to make or merge them, and must miss kv_cache_check.assert_close's bounds on the row named here (sequence, head, row)."""
    torch = pytest.importorskip("torch")
    import cascade_check as cc
    import sink_check as sc
    B, H, Hkv, Sq, d, ls, lens = 3, 4, 2, 3, 64, 130, [5, 129, 40]
    Q, Ks, Vs, K, V = data(torch, B, H, Hkv, Sq, d, 160, 140, 4242)
    sinks = sc.sinks_for(H)
    refO, refL = cc.reference(Q, Ks, Vs, K, V, ls, lens, True, sinks=sinks)
    shared = lambda q, causal=False, s=None: kv.reference(q, Ks[None].expand(B, -1, -1, -1), Vs[None].expand(B, -1, -1, -1), [ls] * B, causal, sinks=s)
    unique = lambda s=None: kv.reference(Q, K, V, lens, True, sinks=s)
    O, lse = sc.apply_sinks(*merge(torch, [shared(Q), unique()]), sinks)
    assert (O - refO).abs().max() < 1e-12 and (lse - refL).abs().max() < 1e-12
    half = lambda parts: ((parts[0][0] + parts[1][0]) / 2, torch.logsumexp(torch.stack([parts[0][1], parts[1][1]]), 0))
    twice = shared(Q)
    wrong = {
        "the prefix masked causally": lambda: sc.apply_sinks(*merge(torch, [shared(Q, causal=True), unique()]), sinks),
        "the prefix counted twice": lambda: sc.apply_sinks(*merge(torch, [twice, twice, unique()]), sinks),
        "the two parts averaged without LSE weights": lambda: sc.apply_sinks(*half([shared(Q), unique()]), sinks),
        "shared rows handed to sequence b + 1": lambda: sc.apply_sinks(*merge(torch, [tuple(t.roll(1, 0) for t in shared(Q)), unique()]), sinks),
        "a sink applied in both parts": lambda: merge(torch, [shared(Q, s=sinks), unique(s=sinks)]),
    }
    named = NAMED_ROWS
    assert sorted(wrong) == sorted(named) and len(wrong) == 5
    for name, run in wrong.items():
        O, lse = run()
        r, lr = kv.ratios(O, lse, refO, refL)
        off = (r > 1).any(-1) | (lr > 1)
        print(f"{name}: {int(off.sum())} of {off.numel()} rows outside the bounds; worst O {r.max().item():.0f} x, LSE {lr.max().item():.0f} x;"
              f" first {tuple(off.nonzero()[0].tolist()) if off.any() else None}")
        with pytest.raises(AssertionError):
            kv.assert_close(O, lse, refO, refL, name)
        b, h, i = named[name]
        with pytest.raises(AssertionError):
            kv.assert_close(O[b, h, i], lse[b, h, i], refO[b, h, i], refL[b, h, i], f"{name}, row {named[name]}")


NAMED_ROWS = {"the prefix masked causally": (0, 0, 0), "the prefix counted twice": (1, 1, 1),
              "the two parts averaged without LSE weights": (2, 2, 2), "shared rows handed to sequence b + 1": (0, 3, 1),
              "a sink applied in both parts": (1, 0, 2)}
