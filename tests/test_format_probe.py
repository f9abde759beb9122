"""CPU tests of the exact single-key probes (tests/format_probe.py), on every family the GPU tests run (tests/test_exact_formats.py):
the e4m3fn decoder written from the OCP definition agrees with torch's float8_e4m3fn and with oracle.round_e4m3fn code by code; in
every family the float64 reference gives the probed key a weight of exactly 1.0 and every other key exactly 0.0, and its O and LSE
pass the checker with error 0 (the inputs, not the checker, stay inside the conditions); an explicit float64 sum over the keys that
starts from +0 reads a V of -0 as +0, bit for bit what expected() pins; every finite code is probed at every column of every fp8
tensor, every key position of the tiles is probed; and every emulated wrong conversion is refused.  No GPU and no kernel."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import format_probe as fp  # noqa: E402
import oracle  # noqa: E402

FAMILIES = fp.cpu_families()
BY_NAME = {p["name"]: p for p in FAMILIES}
assert len(BY_NAME) == len(FAMILIES)
FP8_FAMILIES = [n for n, p in BY_NAME.items() if p["fp8"]]


@pytest.mark.parametrize("code", fp.CODES)
def test_decoder_agrees_with_torch_and_the_oracle(code):
    mine = fp.decode_e4m3fn(code)
    assert np.isfinite(mine)
    if fp.FP8 is not None:
        theirs = torch.tensor([code], dtype=torch.uint8).view(fp.FP8).double()
        assert theirs.item() == mine and bool(torch.signbit(theirs)) == bool(np.signbit(mine)), hex(code)
    fixed = oracle.round_e4m3fn(np.array([mine], dtype=np.float32))
    assert fixed[0] == mine and np.signbit(fixed[0]) == np.signbit(mine), hex(code)            # every code rounds to itself
    assert oracle.lib().oracle_e4m3fn_to_f32(code) == mine and oracle.lib().oracle_f32_to_e4m3fn(mine) == code


def test_the_table_has_254_finite_codes_and_two_nans():
    assert len(fp.finite_codes()) == 254 and all(np.isnan(fp.decode_e4m3fn(c)) for c in (0x7F, 0xFF))
    v = fp.finite_codes()
    assert v[0x01] == 2.0 ** -9 and v[0x07] == 7 * 2.0 ** -9 and v[0x08] == 2.0 ** -6 and v[0x7E] == 448.0 and v[0xFE] == -448.0
    assert v[0x80] == 0 and np.signbit(v[0x80]) and v[fp.pow2_code(0)] == 1.0 and v[fp.pow2_code(-6)] == 2.0 ** -6 and v[fp.pow2_code(8)] == 256.0


def test_prefill_scales_make_the_log2_factor_a_power_of_two():
    """the library computes c = scale * 1.4426950408889634f in fp32 (flash-attention-cuda-c_amd/csrc/FlashAttention.hip: fill_params for the
    prefill kernels, and the same expression in the decode and backward launchers)"""
    for k in (-9, 0, 1):
        assert np.float32(fp.PREFILL_SCALE(k)) * np.float32(1.4426950408889634) == np.float32(2.0 ** k)
        assert float(np.float32(fp.PREFILL_SCALE(k))) == fp.PREFILL_SCALE(k)


def accumulated(p):
    """O [B, H, Sq, d] float64 as acc = +0; acc += w[k] * V[k] for k = 0, 1, ...: plain elementwise float64 arithmetic"""
    _, _, V = fp.logical(p)
    B, H, Sq = p["key"].shape
    G = H // V.shape[1]
    acc = torch.zeros(B, H, Sq, V.shape[3], dtype=torch.float64)
    for b in range(B):
        W, v = fp.weights(p, b), V[b].repeat_interleave(G, 0)
        for k in range(W.shape[2] if p["lens"] is None else p["lens"][b]):
            acc[b] += W[:, :, k, None] * v[:, None, k, :]
    return acc


@pytest.mark.parametrize("name", list(BY_NAME))
def test_reference_puts_weight_one_on_the_probed_key_and_passes_with_error_zero(name):
    p = BY_NAME[name]
    B, H, Sq = p["key"].shape
    for b in range(B):
        W = fp.weights(p, b)
        at = torch.zeros_like(W, dtype=torch.bool).scatter_(2, p["key"][b][..., None], True)
        assert (W[at] == 1.0).all() and (W[~at] == 0.0).all(), (name, b)
    O, lse = fp.reference(p)
    expO, expL = fp.expected(p)
    # the sign of a zero, independently of expected(): the sum over the keys written out, one key after the other onto an accumulator
    # of +0 -- what every kernel's accumulator is.  It must carry expected()'s bits, signs of zeros included.  (A BLAS is free to
    # return a lone product 1 x -0 = -0 without adding it to anything: the reference's own O is compared by value.)
    acc = accumulated(p)
    assert int(torch.signbit(acc).sum()) < int(torch.signbit(fp._gather(p, *fp.logical(p))[2]).sum())     # some -0 was probed and read +0
    bad_o, bad_l, worst = fp.verdict(acc.to(torch.float32), lse, expO, expL)
    assert (bad_o, bad_l) == (0, 0), (name, bad_o, bad_l, worst)
    assert torch.equal(O, acc), name
    assert float((lse - expL).abs().max()) == 0.0, name
    assert torch.isfinite(expO).all() and torch.isfinite(expL).all()
    # bf16 / fp16 outputs: the fp32 value rounded once
    assert fp.verdict(expO.to(fp.bf), None, expO, expL)[0] == 0 and fp.verdict(expO.clamp(-6e4, 6e4).to(fp.f16), None, expO.clamp(-6e4, 6e4), expL)[0] == 0


@pytest.mark.parametrize("name", FP8_FAMILIES)
def test_every_finite_code_is_probed_at_every_column(name):
    p = BY_NAME[name]
    for which in p["fp8"]:
        seen = fp.probed_codes(p, which)
        assert len(seen) == p["Q"].shape[3]
        for c, codes in seen.items():
            assert codes >= set(fp.CODES), f"{name}: {which} column {c} misses {sorted(set(fp.CODES) - codes)[:8]}"


def test_the_bf16_family_probes_every_class_at_every_column():
    for d in (64, 128):
        p = BY_NAME[fp.decode_family(d, cache="bf16")["name"]]
        q, k, v, _ = fp._gather(p, p["Q"], p["K"], p["V"])
        classes = set(np.array(fp.BF16_CLASSES, dtype=np.uint16).view(np.int16).tolist())
        for c in range(d):
            assert set(v[..., c].reshape(-1).view(torch.int16).tolist()) == classes
            assert set(k.reshape(-1)[p["col"].reshape(-1) == c].view(torch.int16).tolist()) == classes
        score = q.double() * k.double()
        assert ((score == 0) | ((score.abs() > 2.0 ** -100) & (score.abs() < 2.0 ** 100))).all()     # well inside fp32's normal range


@pytest.mark.parametrize("name", list(BY_NAME))
def test_every_key_position_is_probed(name):
    p = BY_NAME[name]
    keys = fp.probed_keys(p)
    if p["kind"] == "decode" and p["window"]:
        # every key 0 .. 255 over the sequences: two 128-key tiles, and every row of a page of 16 and of 128
        assert {k for _, k in keys} == set(range(fp.DEC_CAP))
        for page in (16, 128):
            assert {k % page for _, k in keys} == set(range(page))
    elif name.startswith("prefill V"):
        assert {k for _, k in keys} == set(range(fp.V_SK)) and fp.V_SK == 65       # a 64-key tile and the first key of the next
        i = torch.arange(fp.V_SQ)
        assert (p["key"][0, 0] <= i).all()                                          # under the mask: a key the row sees
        assert 64 in p["key"][0, 0, :256].tolist() and int(p["key"][0, 0, 256:].max()) < 64     # block 0 leaves tile 0, block 1 does not
    else:
        assert {k for _, k in keys} == {0}


CONVERSIONS = ("subnormals_flushed", "fnuz", "minus_zero_nan", "max_saturated", "halves_swapped")
# written out, not derived from the families: every fp8 decode family has descales and must refuse one that is dropped; the four with
# two K/V heads must refuse the other head's.  The fp8 prefill calls take no descales.
BOTH = {"v_descale_dropped", "next_heads_descale"}
DESCALE_MUTANTS = {
    "decode fp8 d 64 Hkv 1 kd (0.25,) vd (8.0,)": {"v_descale_dropped"}, "decode fp8 d 128 Hkv 1 kd (0.25,) vd (8.0,)": {"v_descale_dropped"},
    "decode fp8 d 128 Hkv 2 kd (0.25, 2.0) vd (8.0, 0.5)": BOTH, "decode fp8 d 128 Hkv 2 kd (0.0123, 3.7) vd (3.7, 0.0123)": BOTH,
    "decode fp8 d 64 key 0 mask False": BOTH, "decode fp8 d 128 key 0 mask False": BOTH,
    "decode fp8 d 64 key 0 mask True": BOTH, "decode fp8 d 128 key 0 mask True": BOTH,
    **{f"prefill {t} mask {c}": set() for t in ("K", "Q", "V H 4") for c in (False, True)},
}


def test_every_fp8_family_is_listed_with_its_descale_mutants():
    assert set(DESCALE_MUTANTS) == set(FP8_FAMILIES)
    assert all(BY_NAME[n]["kd"] is not None and BY_NAME[n]["vd"] is not None for n in FP8_FAMILIES if n.startswith("decode"))


@functools.lru_cache(maxsize=None)
def truth(name):
    return fp.expected(BY_NAME[name])


@pytest.mark.parametrize("name", FP8_FAMILIES)
def test_every_wrong_conversion_is_refused(name):
    p = BY_NAME[name]
    expO, expL = truth(name)
    found = fp.mutants(p)
    need = set(CONVERSIONS) | DESCALE_MUTANTS[name]
    assert set(found) == need, name
    for kind, kw in found.items():
        O, lse = fp.expected(p, **kw)
        bad_o, bad_l, _ = fp.verdict(O, lse, expO, expL)
        print(f"{name}: {kind}: {bad_o} elements of O and {bad_l} LSE entries refused")
        assert bad_o + bad_l > 0, (name, kind)
        if kind != "v_descale_dropped":                               # a conversion shows in every probed tensor
            assert (bad_o > 0 or "V" not in p["fp8"]) and (bad_l > 0 or not set(p["fp8"]) & {"K", "Q"}), (name, kind)
        else:
            assert bad_o > 0 and bad_l == 0
    with pytest.raises(AssertionError):
        fp.check(name, *fp.expected(p, **found["fnuz"]), expO, expL)
    # the sign of a zero is compared: -0 where +0 is due is refused
    assert fp.verdict(torch.where(expO == 0, -expO, expO), None, expO, expL)[0] > 0
