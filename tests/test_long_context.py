"""GPU: the prefill forward on long heads -- up to 2^18 rows per head, up to the largest K/V head extent the library accepts (just under
2^31 bytes) -- against the exact O(S d) closed form of tests/long_probe.py (CPU proof of the instrument: tests/test_long_probe.py).
Every row of every case sees one key with all the softmax weight: O is that key's V row BIT FOR BIT on every row (a row whose target
the mask hides reads +0), the LSE is held to long_probe.lse_bound.  Data is built and compared on the device; the kernel family is
asserted from plan_ex.  The cases run from moderate sizes to the extent limit, so that a defect shows first where it is cheapest to
read; a failure names the row, its target, the target's tile and byte offset, and the row's query block.  What each case reached is in
profiles/long_context_gpu.log."""
import time

import numpy as np
import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import forward_routes as fr  # noqa: E402
import long_probe as lp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf, f32, f16 = torch.bfloat16, torch.float32, torch.float16
CODE = {bf: fa.FA_DTYPE_BF16, f32: fa.FA_DTYPE_F32, "bf16": fa.FA_DTYPE_BF16, "f32": fa.FA_DTYPE_F32, "fp8": fa.FA_DTYPE_FP8_E4M3}
FLAG = {None: 0, f16: fa.FA_FLAG_F16_WEIGHTS}
GIB = 2 ** 30


def need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"needs ~{gib} GiB of device memory")


def run_and_check(what, family, p, odt, lse=True, wdt=None, layout="dense", t0=None):
    if p["fmt"] == "fp8" and lp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")
    t0 = t0 or time.time()
    H, Sq, d = p["Q"].shape[1:]
    Hkv, Sk = p["K"].shape[1:3]
    got = fr.family(1, H, Sq, Sk, d, p["causal"], CODE[p["fmt"]], CODE[odt], FLAG[wdt])
    assert got == family, (what, got)
    O = lp._alloc(H, Sq, d, odt, DEV, layout)
    out = fa.flash_attention(p["Q"], p["K"], p["V"], O=O, scale=p["scale"], is_causal=p["causal"], return_lse=lse, weights_dtype=wdt)
    torch.cuda.synchronize()
    L = out[1] if lse else None
    worst = lp.check_forward(what, p, O, L)
    hidden = int((~lp.seen(p)).sum())
    print(f"    family {family}, Q [1, {H}, {Sq}, {d}] K/V [1, {Hkv}, {Sk}, {d}] {p['fmt']} -> {str(odt)[6:]}, mask {p['causal']}, layout {layout}, "
          f"head extent {p['extent']} bytes = 2^31 - {2 ** 31 - p['extent']}, codes of {p['nb']} bits, {hidden} rows with a hidden target, "
          f"{time.time() - t0:.2f} s, worst LSE error / bound {worst:.3f}")
    return O, L


# ---- self-attention ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lse", [True, False], ids=["lse", "no_lse"])
def test_bf16_without_the_mask_at_2_pow_16(lse):
    need(4)
    t0 = time.time()
    p = lp.build(2 ** 16, 2 ** 16, 128, "bf16", causal=False, seed=11, device=DEV)
    run_and_check(f"bf16, no mask, S 2^16, LSE {lse}", "bf16", p, f32, lse, t0=t0)


@pytest.mark.parametrize("causal", [False, True], ids=["no_mask", "causal"])
def test_padded_head_dimension_at_2_pow_16(causal):
    need(4)
    t0 = time.time()
    p = lp.build(2 ** 16, 2 ** 16, 96, "bf16", causal=causal, seed=12, device=DEV)
    run_and_check(f"bf16_padded d 96, S 2^16, mask {causal}", "bf16_padded", p, f32, t0=t0)


def test_fp16_weights_at_2_pow_16():
    """FA_FLAG_F16_WEIGHTS: fp16 ends at 65504, so a row whose target lies beyond tile 0 (a weight of 2^64 relative to tile 0) overflows
    the fp16 optimistic pass and is answered by a tracked pass, where the target weighs 1 and the anchor's 2^-64 is 0: exact either way.
    The pass is predicted from the inputs (forward_routes.row_excess) on sampled rows and printed, not asserted from a result."""
    need(4)
    t0 = time.time()
    S = 2 ** 16
    p = lp.build(S, S, 128, "bf16", causal=True, seed=13, device=DEV)
    rows = np.unique(np.concatenate([np.arange(0, S, S // 64), np.array(sorted(p["named"].values()))]))
    e = fr.row_excess(p["Q"][0, 0].float().cpu(), p["K"][0, 0].float().cpu(), p["scale"], True, rows)
    over = int((e >= fr.OVER["f16"]).sum())
    assert ((e >= fr.OVER["f16"]) | (e <= fr.UNDER["f16"])).all()
    print(f"fp16 weights: of {len(rows)} sampled rows {over} have e >= {fr.OVER['f16']} (their units leave the fp16 optimistic pass for a tracked "
          f"one), {len(rows) - over} have e <= {fr.UNDER['f16']} (a unit of such rows alone would stay); e in [{e.min():.0f}, {e.max():.0f}]")
    run_and_check("fp16 weights, causal, S 2^16", "f16_weights", p, f32, wdt=f16, t0=t0)


@pytest.mark.parametrize("fmt,family", [("fp8", "fp8"), ("f32", "f32")])
def test_fp8_and_fp32_inputs_at_2_pow_17(fmt, family):
    need(4)
    t0 = time.time()
    if fmt == "fp8" and lp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")
    p = lp.build(2 ** 17, 2 ** 17, 128, fmt, causal=True, seed=14, device=DEV)
    run_and_check(f"{fmt} inputs, causal, S 2^17", family, p, f32, t0=t0)
    if fmt == "fp8":
        run_and_check(f"{fmt} inputs, causal, S 2^17, bf16 output", family, p, bf)


@pytest.mark.parametrize("S", [2 ** 18, 2 ** 18 - 77], ids=["2_pow_18", "ragged"])
@pytest.mark.parametrize("d", [128, 64])
def test_causal_mix_at_2_pow_18(d, S):
    """one head of 2^18 rows: 1024 query blocks (4 of them with fp16 weights), units whose diagonal lies up to 4096 tiles in; 2^18 - 77:
    the last query block and the last tile are ragged"""
    need(4)
    t0 = time.time()
    p = lp.build(S, S, d, "bf16", causal=True, seed=15 + d, device=DEV)
    run_and_check(f"causal_mix d {d}, S {S}", "causal_mix", p, f32, t0=t0)
    if S % 256:
        run_and_check(f"causal_mix d {d}, S {S}, bf16 output", "causal_mix", p, bf)


@pytest.mark.parametrize("Hkv", [32, 4], ids=["mha", "grouped"])
def test_model_layout_views_with_a_head_extent_just_under_2_pow_31(Hkv):
    """[1, S, H * 128] buffers with H = 32 and S = 2^18 - 256, viewed as [1, H, S, 128] (Q, O; K, V with Hkv heads): the row stride of
    K / V is Hkv * 256 bytes.  With 32 K/V heads one head extends over 2^31 - 2^21 - 7936 bytes -- (S + 192) rows are the last that
    stay below 2^31 -- and byte 2^30 of a head lies at key 2^17; grouped (Hkv = 4) the same rows span 2^28 bytes"""
    need(24)
    t0 = time.time()
    H, S, d = 32, 2 ** 18 - 256, 128
    p = lp.build(S, S, d, "bf16", H, Hkv, True, seed=17, device=DEV, layout="model")
    assert p["K"].stride(2) == Hkv * d and p["Q"].stride(2) == H * d
    if Hkv == H:
        assert (S + 192 + 64) * p["stride_bytes"] >= 2 ** 31 > (S + 192) * p["stride_bytes"] and "first key past byte 1073741824" in p["named"]
    run_and_check(f"model layout, H {H} Hkv {Hkv}, S {S}", "causal_mix", p, bf, layout="model", t0=t0)


# ---- cross-attention at the largest extent the library accepts ----------------------------------------------------------------------------
CROSS_SQ = 512
PERSISTENT_SQ = 130 * 256               # more query blocks than half the compute units: past the pair kernel's reach (forward_routes)


def largest_accepted(fmt, d, H, layout, hi):
    """the largest Sk flash_attention accepts for [1, H, Sk, d] K / V (dense, or views of [1, Sk, H d]): long_probe.largest_accepted
    with 64 rows of zeros; a refusal must be FA_ERR_BAD_SHAPE, which comes before any launch"""
    dtype = lp.FORMATS[fmt][0]
    Kb, Q = lp._alloc(H, hi, d, dtype, DEV, layout), lp._alloc(H, 64, d, dtype, DEV, layout)

    def accepted(c):
        try:
            fa.flash_attention(Q, Kb[:, :, :c], Kb[:, :, :c], scale=0.125, out_dtype=f32)
            return True
        except fa.FlashAttentionError as e:
            assert e.code == -3, e
            return False

    lo = lp.largest_accepted(accepted, hi)
    torch.cuda.synchronize()
    stride = Kb.stride(2) * Kb.element_size()
    assert (lo + 1 + 192) * stride >= 2 ** 31 > lo * stride                  # include/flash_attention.h: one head's extent below 2^31 bytes
    return lo


@pytest.mark.parametrize("fmt,d,H,layout,hi,Sq,family", [
    ("bf16", 128, 16, "model", 2 ** 19, CROSS_SQ, "pair"), ("bf16", 128, 1, "dense", 2 ** 23, CROSS_SQ, "pair"),
    ("f32", 64, 1, "dense", 2 ** 23, CROSS_SQ, "f32"), ("fp8", 128, 1, "dense", 2 ** 24, CROSS_SQ, "fp8"),
    ("bf16", 64, 1, "dense", 2 ** 24, CROSS_SQ, "pair"), ("bf16", 128, 1, "dense", 2 ** 23, PERSISTENT_SQ, "bf16")],
    ids=["model_layout_d128", "dense_d128", "f32_d64", "fp8_d128", "dense_d64", "dense_d128_persistent"])
def test_cross_attention_at_the_largest_accepted_extent(fmt, d, H, layout, hi, Sq, family):
    """512 rows against the longest K / V the call accepts (found as tests/test_decode_edges.py finds its capacity), not causal: half the
    targets on the keys of the last 300 + Sq, forced ones on the last key and on both sides of byte 2^30 and byte 2^31 - 2^20 of the
    head.  With 512 rows a bf16 call has too few query blocks for the persistent kernels and plan_ex gives it to the pair kernel (the
    family is asserted, whichever it is); the last case has 130 query blocks, which puts the persistent bf16 kernel -- the one the
    benchmark times -- on the same K / V."""
    need(12)
    if fmt == "fp8" and lp.FP8 is None:
        pytest.skip("torch has no float8_e4m3fn")
    t0 = time.time()
    cap = largest_accepted(fmt, d, H, layout, hi)
    p = lp.build(Sq, cap, d, fmt, H, H, False, seed=19, device=DEV, layout=layout)
    print(f"largest accepted Sk at a row stride of {p['stride_bytes']} bytes: {cap} = 2^{int(np.log2(hi))} - {hi - cap}")
    for line in lp.BYTE_LINES:
        assert f"first key past byte {line}" in p["named"] and f"last key below byte {line}" in p["named"]
    assert int((p["target"] >= cap - Sq - lp.NEAR).sum()) >= H * Sq // 3 and int(p["target"][0, -1]) == cap - 1
    run_and_check(f"cross {fmt} d {d} H {H} {layout}, Sq {Sq} Sk {cap}", family, p, f32, layout=layout, t0=t0)
