"""GPU tests of flash_attention_decode at its edges: lengths out of range (clamped on the device into [1, capacity]), custom scales and
a sharp softmax, splits whose partial log-sum-exps differ by hundreds, |V| = 1e30, and the largest head extent the ABI accepts
(one K/V head just under 2^31 bytes).  Reference, mask and the element-wise check are those of tests/kv_cache_check.py."""
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()

from kv_cache_check import CAP, DEV, SCALES, TILE, assert_close, assert_close_with_score_noise, randn, reference  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_lengths_out_of_range_are_clamped_on_the_device(d, causal):
    B, H, Hkv, Sq, cap = 8, 8, 2, 2, 1000
    raw = [0, -1, -2 ** 31, cap + 1, 2 ** 31 - 1, 5, cap, 300]
    clamped = [min(max(x, 1), cap) for x in raw]
    assert clamped == [1, 1, 1, cap, cap, 5, cap, 300]
    Q, K, V = randn((B, H, Sq, d), 71, BF16), randn((B, Hkv, cap, d), 72, BF16), randn((B, Hkv, cap, d), 73, BF16)
    refO, refL = reference(Q, K, V, clamped, causal)
    Qd, Kd, Vd = Q.to(DEV), K.to(DEV), V.to(DEV)
    raw_d, clamped_d = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in (raw, clamped))
    for splits in (0, 1, 3, CAP):
        kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True)
        O, lse = fa.flash_attention_decode(Qd, Kd, Vd, raw_d, **kw)
        Oc, lsec = fa.flash_attention_decode(Qd, Kd, Vd, clamped_d, **kw)
        torch.cuda.synchronize()
        assert torch.equal(O, Oc) and torch.equal(lse, lsec), splits
        assert_close(O, lse, refO, refL, f"clamped lengths, d {d} causal {causal} splits {splits}")


@pytest.mark.parametrize("kind", list(SCALES))
@pytest.mark.parametrize("d", [64, 128])
def test_custom_scale_and_sharp_softmax(d, kind):
    """(scale, factor on Q and K): 0.02, 3/sqrt(d), 1 with the scores kept O(1); Q and K times 3 and times 12"""
    scale, mul = SCALES[kind](d)
    B, H, Hkv, Sq, cap, lens = 2, 8, 2, 4, 3000, [777, 3000]
    Q, K, V = (randn((B, H, Sq, d), 81, BF16) * mul).bfloat16(), (randn((B, Hkv, cap, d), 82, BF16) * mul).bfloat16(), randn((B, Hkv, cap, d), 83, BF16)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for splits in (0, 1, 5):
        O, lse = fa.flash_attention_decode(Q.to(DEV), K.to(DEV), V.to(DEV), lens_d, scale=scale, is_causal=True, out_dtype=torch.float32,
                                           num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close_with_score_noise(O, lse, Q, K, V, lens, True, scale, f"{kind} d {d} splits {splits}")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("d", [64, 128])
def test_one_tile_hundreds_above_every_other(d, where):
    """every query has the component 3 in each coordinate, the keys of ONE 128-key tile the component 10: their scores stand
    30 sqrt(d) (240 / 339) above all others.  Every split but one gets the weight exp(-hundreds) = exactly 0 in the combine kernel"""
    B, H, Hkv, Sq, tiles = 2, 8, 2, 2, 14
    cap = tiles * TILE
    hot = {"first": 0, "middle": 6, "last": tiles - 1}[where]
    Q, K, V = randn((B, H, Sq, d), 91, BF16).float() + 3.0, randn((B, Hkv, cap, d), 92, BF16).float(), randn((B, Hkv, cap, d), 93, BF16)
    K[:, :, hot * TILE:(hot + 1) * TILE] += 10.0
    Q, K = Q.bfloat16(), K.bfloat16()
    scale = 1.0 / d ** 0.5
    for splits in (2, 7, CAP):
        O, lse = fa.flash_attention_decode(Q.to(DEV), K.to(DEV), V.to(DEV), None, is_causal=False, out_dtype=torch.float32,
                                           num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        assert_close_with_score_noise(O, lse, Q, K, V, None, False, scale, f"hot tile {where} d {d} splits {splits}")
    # the mass really is in that tile alone: the float64 weights outside it sum to less than the smallest fp32 subnormal
    S = (Q[0, 0].double() @ K[0, 0].double().T) * scale
    P = torch.softmax(S, -1)
    P[:, hot * TILE:(hot + 1) * TILE] = 0
    assert P.sum(-1).max().item() < 1e-45


@pytest.mark.parametrize("d", [64, 128])
def test_v_of_1e30_on_the_keys_that_carry_weight(d):
    """|V| ~ 1e30 (one sign per column, so that no element of the reference is a cancellation) on every valid key; NaN and inf in K and
    V beyond the length only.  Finite, and every element within 1e-3 |ref|"""
    B, H, Hkv, Sq, cap, lens = 2, 8, 2, 3, 1024, [100, 1000]
    g = torch.Generator().manual_seed(95)
    sign = torch.where(torch.arange(d) % 2 == 0, 1.0, -1.0)
    Q, K = randn((B, H, Sq, d), 96, BF16), randn((B, Hkv, cap, d), 97, BF16)
    V = ((0.5 + torch.rand((B, Hkv, cap, d), generator=g)) * 1e30 * sign).bfloat16()
    for b, L in enumerate(lens):
        K[b, :, L::2], K[b, :, L + 1::2] = float("nan"), float("inf")
        V[b, :, L::2], V[b, :, L + 1::2] = float("-inf"), float("nan")
    refO, refL = reference(Q, K, V, lens, True)
    assert refO.abs().min().item() > 1e29
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for splits in (0, 1, 3, CAP):
        O, lse = fa.flash_attention_decode(Q.to(DEV), K.to(DEV), V.to(DEV), lens_d, is_causal=True, out_dtype=torch.float32,
                                           num_splits=splits, return_lse=True)
        torch.cuda.synchronize()
        O, lse = O.double().cpu(), lse.double().cpu()
        assert torch.isfinite(O).all() and torch.isfinite(lse).all(), splits
        ratio = ((O - refO).abs() / (1e-3 * refO.abs())).max().item()
        print(f"V of 1e30, d {d} splits {splits}: worst error / (1e-3 |ref|) {ratio:.3f}")
        assert ratio <= 1.0 and ((lse - refL).abs() <= 2e-4 + 2e-6 * refL.abs()).all(), splits


def test_the_largest_head_extent_the_abi_accepts():
    """A [1, capacity, Hkv = 8, d = 128] cache view (row stride 2048 bytes) at the largest capacity flash_attention_decode accepts --
    one K/V head's extent just under 2^31 bytes, where the kernel's 32-bit buffer offsets end.  The softmax mass and a distinctive V
    sit on the last keys, and on the keys just past byte offsets 2^30 and 2^31 - 2^20 of a head.  Needs ~4.5 GiB of device memory
    for the cache, ~6 GiB with the temporaries."""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * 2 ** 30:
        pytest.skip("needs ~6 GiB of device memory")
    H, Hkv, d, rows = 16, 8, 128, 2 ** 20
    G = H // Hkv
    gen = torch.Generator(device=DEV).manual_seed(99)
    Kb, Vb = (torch.empty((1, rows, Hkv, d), dtype=torch.bfloat16, device=DEV) for _ in range(2))
    for t in (Kb, Vb):
        for r0 in range(0, rows, 2 ** 16):
            t[0, r0:r0 + 2 ** 16] = torch.randn((2 ** 16, Hkv, d), generator=gen, device=DEV).bfloat16()
    Q = torch.randn((1, H, 1, d), generator=gen, device=DEV).bfloat16()
    view = lambda t, c: t[:, :c].transpose(1, 2)                     # [1, Hkv, c, d], strides (., d, Hkv d, 1)

    def accepted(c):
        try:
            fa.flash_attention_decode(Q, view(Kb, c), view(Vb, c), out_dtype=torch.float32)
            return True
        except fa.FlashAttentionError as e:
            assert e.code == -3, e                                   # FA_ERR_BAD_SHAPE, before any launch
            return False

    lo, hi = 2 ** 19, rows                                           # accepted, refused
    assert accepted(lo) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    cap = lo
    torch.cuda.synchronize()
    print(f"largest accepted capacity at a 2048-byte row stride: {cap} keys, head extent {cap * 2048} bytes = 2^31 - {2 ** 31 - cap * 2048}")
    assert accepted(cap) and not accepted(cap + 1)
    assert (cap + 1 + 192) * 2048 >= 2 ** 31 > cap * 2048             # include/flash_attention.h: one head's extent below 2^31 bytes
    K, V = view(Kb, cap), view(Vb, cap)
    places = {"the last keys": cap - 8, "past byte 2^30": 2 ** 30 // 2048, "past byte 2^31 - 2^20": (2 ** 31 - 2 ** 20) // 2048}
    assert places["past byte 2^31 - 2^20"] + 8 <= cap - 8
    marks = torch.arange(8, device=DEV, dtype=torch.float32)[:, None, None]
    for what, k0 in places.items():
        keepK, keepV = Kb[0, k0:k0 + 8].clone(), Vb[0, k0:k0 + 8].clone()
        # the FIRST query head of every group gets its mass there (score 3 |q|^2 / sqrt(d) ~ 34 above the rest); the second does not
        Kb[0, k0:k0 + 8] = (3.0 * Q[0, ::G, 0].float())[None].expand(8, Hkv, d).bfloat16()
        Vb[0, k0:k0 + 8] = (100.0 + 8.0 * marks + torch.arange(Hkv, device=DEV)[None, :, None]).expand(8, Hkv, d).bfloat16()
        for L in (cap, cap - 3):
            lens_d = torch.tensor([L], dtype=torch.int32, device=DEV)
            outs = {}
            for splits in (1, 0):
                outs[splits] = fa.flash_attention_decode(Q, K, V, lens_d, is_causal=True, out_dtype=torch.float32, num_splits=splits,
                                                         return_lse=True)
            torch.cuda.synchronize()
            for kvh in (0, Hkv - 1):
                hs = slice(kvh * G, kvh * G + G)
                refO, refL = reference(Q[:, hs].cpu(), K[:, kvh:kvh + 1].cpu(), V[:, kvh:kvh + 1].cpu(), [L], True)
                assert refO[0, 0, 0].min().item() > 99.0              # the marked V is what the first head of the group returns
                for splits, (O, lse) in outs.items():
                    assert_close(O[:, hs], lse[:, hs], refO, refL, f"{what}, length {L}, K/V head {kvh}, splits {splits or 'chosen'}")
        Kb[0, k0:k0 + 8], Vb[0, k0:k0 + 8] = keepK, keepV
