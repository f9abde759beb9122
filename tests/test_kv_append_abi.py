"""CPU tests of flash_attention_kv_append and flash_attention_kv_append_paged (the write side of the decode caches) at the C ABI and
in the binding, and of the reference the GPU tests compare with (tests/kv_append_check.py): the symbols exist with the declared
parameter lists and argtypes; every invalid argument is refused with the decode calls' code before anything is launched (fake aligned
host pointers: no GPU is touched), for both cache types; the reference's value rule is round-to-nearest-even with the sign kept on
every bf16 bit pattern; its position rule is the header's; the binding's own refusals."""
import ctypes

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

import kv_append_check as kc  # noqa: E402
from abi_decl import (BAD_DHEAD, BAD_DTYPE, BAD_SHAPE, BAD_STRIDE, BF16, F16, F32, FP8, MISALIGNED, NULL_POINTER,  # noqa: E402
                      MetaTensor as T, declared_parameters, host_calls)


def test_the_symbols_are_exported_with_the_declared_signatures():
    L = fa.lib()
    sp, vp, i = ctypes.POINTER(fa.FaStrides), ctypes.c_void_p, ctypes.c_int
    of = {"int": i, "int64": ctypes.c_int64}
    want = {
        "flash_attention_kv_append": [
            ("Knew", vp), ("Vnew", vp), ("K", vp), ("V", vp), ("kvLens", vp), ("kDescale", vp), ("vDescale", vp), ("batchSize", i),
            ("numHeadsKV", i), ("seqLenNew", i), ("seqLenK", i), ("dHead", i), ("dtype", i), ("kv_dtype", i), ("sKnew", sp), ("sVnew", sp),
            ("sK", sp), ("sV", sp), ("stream", vp)],
        "flash_attention_kv_append_paged": [
            ("Knew", vp), ("Vnew", vp), ("Kpool", vp), ("Vpool", vp), ("kvLens", vp), ("blockTable", vp), ("kDescale", vp), ("vDescale", vp),
            ("batchSize", i), ("numHeadsKV", i), ("seqLenNew", i), ("numPages", i), ("pageSize", i), ("maxPagesPerSeq", i),
            ("tableStride", of["int64"]), ("dHead", i), ("dtype", i), ("kv_dtype", i), ("sKnew", sp), ("sVnew", sp), ("sK", sp), ("sV", sp),
            ("stream", vp)],
    }
    for name, params in want.items():
        assert name in fa.EXPORTS and getattr(L, name) is not None
        assert declared_parameters(name) == [n for n, _ in params], name
        assert list(getattr(L, name).argtypes) == [t for _, t in params], name
        assert getattr(L, name).restype is i
    # the paged list is the contiguous one with blockTable after kvLens and the paging geometry in the place of seqLenK, as in decode
    c, p = declared_parameters("flash_attention_kv_append"), declared_parameters("flash_attention_kv_append_paged")
    c[c.index("seqLenK"):c.index("seqLenK") + 1] = ["numPages", "pageSize", "maxPagesPerSeq", "tableStride"]
    c.insert(c.index("kvLens") + 1, "blockTable")
    assert [x.replace("pool", "") for x in p] == c


def calls(kv):
    """(contiguous call, paged call, an aligned host pointer) for cache type kv; keyword arguments override a valid call"""
    okc = dict(B=2, Hkv=2, Sq=3, Sk=1024, d=128, dtype=BF16, kv=kv)
    okp = dict(B=2, Hkv=2, Sq=3, P=64, page=64, maxp=16, ts=16, d=128, dtype=BF16, kv=kv)
    return host_calls(("flash_attention_kv_append", okc), ("flash_attention_kv_append_paged", okp))


# A call that passes every check would LAUNCH (on a machine with a device: write through the host pointers).  So there is no "valid
# call" probe here: each case below is wrong in exactly one way, or in two ways whose order of detection is the decode calls' order
# (pointers, alignment, paging, shape, types, dHead, strides, extent), and the code says which check spoke.
@pytest.mark.parametrize("kv", [BF16, FP8])
def test_what_the_decode_calls_refuse_is_refused_with_the_same_codes(kv):
    contiguous, paged, p = calls(kv)
    esz = 2 if kv == BF16 else 1
    for call in (contiguous, paged):
        for name in ("Kn", "Vn", "K", "V"):
            assert call(**{name: None}) == NULL_POINTER, name
            assert call(**{name: p + 8}, d=96) == MISALIGNED, name
        assert call(lens=p + 2, d=96) == MISALIGNED and call(lens=p + 1, d=96) == MISALIGNED
        assert call(lens=p + 4, d=96) == BAD_DHEAD                     # (4-byte alignment is enough for the lengths)
        for name in ("kd", "vd"):
            for off in (1, 2, 3, 6):
                assert call(**{name: p + off}, d=96) == MISALIGNED, (name, off)
        # seqLenNew: at least 1, at most the capacity (1024 either way) -- and NOT capped at FA_DECODE_MAX_Q: 17 and the capacity itself
        # pass on to the dHead check
        for kw in (dict(Sq=0), dict(Sq=-1), dict(Sq=1025), dict(Sq=1 << 30), dict(B=0), dict(B=-1), dict(Hkv=0), dict(Hkv=-2), dict(d=0),
                   dict(B=1 << 16, Hkv=1 << 15)):
            assert call(**kw) == BAD_SHAPE, kw
        for Sq in (1, fa.FA_DECODE_MAX_Q + 1, 1024):
            assert call(Sq=Sq, d=96) == BAD_DHEAD, Sq
        for dt in (F32, FP8, F16, 9, -1):
            assert call(dtype=dt, d=96) == BAD_DTYPE, dt
        for other in (F32, F16, 9, -1):
            assert call(kv=other, d=96) == BAD_DTYPE, other
        for d in (96, 32, 256, 120, 8):
            assert call(d=d) == BAD_DHEAD, d
        bad = fa.FaStrides(1 << 20, 1 << 16, 56)           # strideS < d
        mis = fa.FaStrides(1 << 20, 1 << 16, 66)           # 132-byte bf16 rows, 66-byte fp8 rows: no multiples of 16
        misH = fa.FaStrides(1 << 20, (1 << 16) + 4, 64)
        misB = fa.FaStrides((1 << 20) + 4, 1 << 16, 64)
        neg = fa.FaStrides(-(1 << 20), 1 << 16, 64)
        for i in range(4):
            for s in (bad, mis, misH, misB, neg):
                st = [None] * 4
                st[i] = ctypes.byref(s)
                assert call(strides=st, d=64) == BAD_STRIDE, i
        # 8 elements are 16 bytes of bf16 and only 8 bytes of e4m3fn: fine for the new rows, and for the caches only if they are bf16.
        # (The stride is accepted where the extent check speaks next: one head of 2^24 rows does not fit)
        eight = fa.FaStrides(1 << 40, 1 << 36, 136)
        for i in (0, 1):
            st = [None] * 4
            st[i] = ctypes.byref(eight)
            huge = dict(Sk=1 << 24) if call is contiguous else dict(page=1 << 24, maxp=1, ts=1)
            assert call(strides=st, **huge) == BAD_SHAPE, i
        for i in (2, 3):
            st = [None] * 4
            st[i] = ctypes.byref(eight)
            huge = dict(Sk=1 << 24) if call is contiguous else dict(page=1 << 24, maxp=1, ts=1)
            assert call(strides=st, **huge) == (BAD_SHAPE if kv == BF16 else BAD_STRIDE), i
    for kw in (dict(Sk=0), dict(Sk=-128), dict(Sk=(1 << 24) + 1)):
        assert contiguous(**kw) == BAD_SHAPE, kw
    assert paged(table=None) == NULL_POINTER
    assert paged(table=p + 2, d=96) == MISALIGNED and paged(table=p + 1, d=96) == MISALIGNED
    for kw in (dict(P=0), dict(P=-1), dict(maxp=0, ts=16), dict(maxp=-3), dict(page=8), dict(page=0), dict(page=-16), dict(page=1),
               dict(page=24), dict(page=48), dict(page=100), dict(page=(1 << 20) + 16),
               dict(page=16, maxp=(1 << 20) + 1, ts=1 << 21),        # capacity 2^24 + 16: the cap stays
               dict(page=1 << 16, maxp=1 << 16, ts=1 << 16),         # capacity 2^32: no 32-bit wrap-around
               dict(page=1 << 30, maxp=4, ts=4),
               dict(ts=15), dict(ts=0), dict(ts=-16), dict(page=16, maxp=2, ts=2, Sq=33)):
        assert paged(**kw) == BAD_SHAPE, kw
    # the extent limits are decode's, counted in bytes: (seqLenK + 192) x row stride, or pageSize x row stride, below 2^31
    rows = (1 << 31) // (128 * esz)                       # dense d = 128 rows that make 2^31 bytes
    assert contiguous(Sk=rows - 192) == BAD_SHAPE
    assert paged(page=rows, maxp=1, ts=1) == BAD_SHAPE
    wide = fa.FaStrides(1 << 40, 128, (1 << 25) // esz)   # 64 rows x 2^25 bytes = 2^31
    for i in (2, 3):
        st = [None] * 4
        st[i] = ctypes.byref(wide)
        assert paged(strides=st) == BAD_SHAPE, i
        assert contiguous(strides=st) == BAD_SHAPE, i


def test_descales_belong_to_an_fp8_cache():
    contiguous, paged, p = calls(BF16)
    for call in (contiguous, paged):
        # (as in the _window calls: a bf16 cache is what lies in memory; the type check speaks before the dHead check)
        assert call(kd=p, d=96) == BAD_DTYPE and call(vd=p + 4, d=96) == BAD_DTYPE and call(kd=p, vd=p, d=96) == BAD_DTYPE
    contiguous, paged, p = calls(FP8)
    for call in (contiguous, paged):
        assert call(kd=p, vd=p + 4, d=96) == BAD_DHEAD and call(kd=p + 8, d=96) == BAD_DHEAD


# ---- the reference of the GPU tests ----
DESCALES = (1.0, 0.25, 0.0123, 3.7)


def test_the_reference_rounds_every_bf16_pattern_to_the_nearest_even_code():
    x = kc.all_bf16_patterns()
    finite = torch.isfinite(x.float())
    for ds in DESCALES:
        got = kc.encode(x.reshape(1, 1, 512, 128), torch.tensor([ds]), True).reshape(-1)
        want, nan = kc.nearest_even_code(kc.quotient(x, ds))
        assert torch.equal(nan, torch.isnan(x.float()))
        assert torch.equal((got & 0x7F) == 0x7F, nan), ds          # a NaN code for NaN, none from a finite input or an infinity
        assert torch.equal(got[~nan], want[~nan]), ds               # nearest, ties to even, saturated, the sign of zero included
        assert torch.equal(got[~nan] >> 7, (x.view(torch.int16)[~nan].int() >> 15 & 1).to(torch.uint8)), ds   # the sign is the input's
        assert int(got[0x7F80]) == 0x7E and int(got[0xFF80]) == 0xFE                                         # +-inf -> +-448
        assert int(got[0x0000]) == 0x00 and int(got[0x8000]) == 0x80 and int(got[0x8001]) == 0x80            # -0, negative underflow
        assert int(finite.sum()) == 65536 - 256
    # ... and a NULL descale is 1.0; a bf16 cache stores the pattern itself
    assert torch.equal(kc.encode(x.reshape(1, 1, 512, 128), None, True), kc.encode(x.reshape(1, 1, 512, 128), torch.ones(1), True))
    assert torch.equal(kc.encode(x.reshape(1, 1, 512, 128), None, False).reshape(-1).int() & 0xFFFF, torch.arange(65536, dtype=torch.int32))


def test_the_search_itself_on_hand_made_quotients():
    q = torch.tensor([0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 2.0 ** -10 * 1.01, 3 * 2.0 ** -10, 1.0, 1.0625, 1.1875, 432.0, 431.9, 447.0, 448.0,
                      500.0, float("inf"), -float("inf"), float("nan"), -1e-30], dtype=torch.float64)
    want = [0x00, 0x80, 0x00, 0x80, 0x01, 0x02, 0x38, 0x38, 0x3A, 0x7E, 0x7D, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0x7F, 0x80]
    got, nan = kc.nearest_even_code(q)
    assert got.tolist() == want and nan.tolist() == [False] * 16 + [True, False]


def test_the_position_rule_is_the_headers():
    cap = 32
    for L in range(-2, 41):
        for Sq in range(1, 7):
            want = []
            for i in range(Sq):
                for p in range(cap):
                    if L > 0 and p == min(L, cap) - Sq + i:
                        want.append((i, p))
            assert kc.positions(L, Sq, cap) == want, (L, Sq)
            # through the writer: contiguous, and paged behind a table with one entry out of range
            new = (torch.arange(Sq * 8).reshape(1, 1, Sq, 8) + 1).to(torch.bfloat16)
            out = kc.append(new, torch.zeros(1, 1, cap, 8, dtype=torch.int16), [L])
            exp = torch.zeros(1, 1, cap, 8, dtype=torch.int16)
            for i, p in want:
                exp[0, 0, p] = new[0, 0, i].view(torch.int16)
            assert torch.equal(out, exp), (L, Sq)
            table = torch.tensor([[1, 7]])
            pool = kc.append(new, torch.zeros(3, 1, 16, 8, dtype=torch.int16), [L], table=table)
            assert torch.equal(pool[1, 0], exp[0, 0, :16]) and not pool[0].any() and not pool[2].any(), (L, Sq)


def test_binding_refusals():
    f8, bf = torch.float8_e4m3fn, torch.bfloat16
    new = torch.zeros(2, 2, 3, 64, dtype=bf)
    k, k8 = torch.zeros(2, 2, 32, 64, dtype=bf), torch.zeros(2, 2, 32, 64, dtype=f8)
    pool, pool8 = torch.zeros(6, 2, 16, 64, dtype=bf), torch.zeros(6, 2, 16, 64, dtype=f8)
    table = torch.zeros(2, 2, dtype=torch.int32)
    ones = torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.kv_cache_append(new, new, k, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.kv_cache_append_paged(new, new, pool8, pool8, table, k_descale=ones)

    def both(Kn, Vn, K, V, Kp, Vp, tab=table, **kw):
        yield lambda: fa.kv_cache_append(T(Kn), T(Vn), T(K), T(V), **kw)
        yield lambda: fa.kv_cache_append_paged(T(Kn), T(Vn), T(Kp), T(Vp), T(tab), **kw)

    # Sq: at least one row, at most the capacity (32 both ways) -- before the C call
    for Sq in (0, 33, 100):
        n = torch.zeros(2, 2, Sq, 64, dtype=bf)
        for call in both(n, n, k, k, pool, pool):
            with pytest.raises(ValueError, match="new rows"):
                call()
    # shapes: K_new and V_new alike, the caches' K/V heads, K and V alike, d alike
    for Kn, Vn, K, V, Kp, Vp in ((new, new[:, :, :2], k, k, pool, pool), (new[:, :1], new[:, :1], k, k, pool, pool),
                                 (new[0], new[0], k, k, pool, pool), (new, new, k, k[:, :, :16], pool, pool[:4]),
                                 (new, new, k[..., :32], k[..., :32], pool[..., :32], pool[..., :32])):
        for call in both(Kn, Vn, K, V, Kp, Vp):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        fa.kv_cache_append(T(new), T(new), T(k[:1]), T(k[:1]))          # the batch of a contiguous cache
    # dtypes: bf16 new rows under a bf16 or an fp8 cache; everything else is "share a dtype"
    for Kn, Vn, K, V, Kp, Vp in ((new, new, k.float(), k.float(), pool.float(), pool.float()), (new, new, k8, k, pool8, pool),
                                 (new.half(), new.half(), k8, k8, pool8, pool8), (new.float(), new.float(), k, k, pool, pool)):
        for call in both(Kn, Vn, K, V, Kp, Vp):
            with pytest.raises(TypeError, match="share a dtype"):
                call()
    for call in both(new, new.half(), k, k, pool, pool):
        with pytest.raises(ValueError, match="one dtype"):
            call()
    # descales belong to an fp8 cache and are dense fp32 [Hkv] on the device of the new rows
    for kw in (dict(k_descale=T(ones)), dict(v_descale=T(ones))):
        for call in both(new, new, k, k, pool, pool, **kw):
            with pytest.raises(ValueError, match="descale"):
                call()
    for bad in (T(ones.double()), T(torch.ones(3)), T(torch.ones(4)[::2]), T(ones, device="cpu"), ones, 1.0):
        for name in ("k_descale", "v_descale"):
            for call in both(new, new, k8, k8, pool8, pool8, **{name: bad}):
                with pytest.raises(ValueError, match=name):
                    call()
    # lengths: dense int32 [B] on the device (good descales pass: the next check speaks)
    for lens in (T(torch.zeros(3, dtype=torch.int32)), T(torch.zeros(2, dtype=torch.int64)), T(torch.zeros(4, dtype=torch.int32)[::2]),
                 torch.zeros(2, dtype=torch.int32)):
        for call in both(new, new, k8, k8, pool8, pool8, k_descale=T(ones), v_descale=T(ones), kv_lens=lens):
            with pytest.raises(ValueError, match="kv_lens"):
                call()
    # the table: int32 [B, max_pages], last dimension contiguous
    for tab in (table.long(), table[:1], torch.zeros(2, 4, dtype=torch.int32)[:, ::2], torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="block_table"):
            fa.kv_cache_append_paged(T(new), T(new), T(pool), T(pool), T(tab))
