"""GPU: the backward pass on long heads -- 2^17 rows per head, thousands of 256-key blocks (FA_BWD_HEAVY_FIRST orders them) whose
workgroups add into the same fp32 dQ rows, and the largest K/V head extent the call accepts -- against the O(S d) closed form of
tests/long_probe.py's backward form (CPU proof: tests/test_long_probe.py).  Every row puts a weight of 1/2 on each key of one pair
(t, t ^ 1) -- or all of it on one where the diagonal runs between them, or on the anchor where the mask hides both.  dQ, dK, dV are held
element by element to the bound tests/weight_probe.py uses for the backward, 1e-2 |ref| + 2^-7 mag + 1e-5 (+ 2^-8 |ref| for bf16
gradients); every key but the anchor that no row targets must hold EXACTLY 0 in dK and dV, over the whole tensors; two runs must give
bitwise equal dK and dV (each is written by one workgroup in a fixed order; dQ is summed by atomics and is not asked that).  The LSE
comes from the library's own forward, as in use.  What each case reached is in profiles/long_context_gpu.log."""
import time

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import long_probe as lp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf, f32 = torch.bfloat16, torch.float32


def need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * 2 ** 30:
        pytest.skip(f"needs ~{gib} GiB of device memory")


def run_and_check(what, p, dtype, t0):
    """forward (O, LSE in `dtype` / fp32), backward twice with gradients in `dtype`"""
    H, Sq, d = p["Q"].shape[1:]
    Hkv, Sk = p["K"].shape[1:3]
    kw = dict(scale=p["scale"], is_causal=p["causal"])
    torch.cuda.synchronize()
    t1 = time.time()
    O, lse = fa.flash_attention(p["Q"], p["K"], p["V"], out_dtype=dtype, return_lse=True, **kw)
    dO = p["dO"].to(dtype)
    runs = []
    for _ in range(2):
        dQ = torch.full((1, H, Sq, d), float("nan"), dtype=dtype, device=DEV)
        dK, dV = (torch.full((1, Hkv, Sk, d), float("nan"), dtype=dtype, device=DEV) for _ in range(2))
        fa.flash_attention_backward(p["Q"], p["K"], p["V"], O, dO, lse, dQ=dQ, dK=dK, dV=dV, **kw)
        torch.cuda.synchronize()
        runs.append((dQ, dK, dV))
    t2 = time.time()
    ref = lp.backward_closed_form(p)
    torch.cuda.synchronize()
    t3 = time.time()
    lse_err = float(((lse.double() - ref["lse"]).abs() / lp.lse_bound(ref["lse"], lp.E + 1)).max())
    worst = lp.check_backward(what, p, ref, *runs[0])
    assert torch.equal(lp._bits_of(runs[0][1]), lp._bits_of(runs[1][1])) and torch.equal(lp._bits_of(runs[0][2]), lp._bits_of(runs[1][2])), \
        f"{what}: two runs differ in dK or dV"
    targeted = sum(len(h["keys"]) - 1 for h in ref["heads"])
    print(f"    backward, Q [1, {H}, {Sq}, {d}] K/V [1, {Hkv}, {Sk}, {d}], O / dO / gradients {str(dtype)[6:]}, mask {p['causal']}, head extent "
          f"{p['extent']} bytes = 2^31 - {2 ** 31 - p['extent']}, {-(-Sk // 256)} key blocks, {targeted} targeted keys, {time.time() - t0:.2f} s "
          f"(data {t1 - t0:.2f}, forward and two backward calls {t2 - t1:.2f}, closed form {t3 - t2:.2f}), "
          f"forward LSE error / bound {lse_err:.3f}, worst gradient error / bound {max(worst.values()):.3f}, dK and dV bitwise equal in two runs")
    assert lse_err <= 1.0, f"{what}: the forward's LSE is outside its bound"


@pytest.mark.parametrize("dtype", [f32, bf], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_backward_at_2_pow_17_rows(d, dtype):
    need(8)
    t0 = time.time()
    S = 2 ** 17
    p = lp.build_backward(S, S, d, 1, 1, True, seed=21 + d, device=DEV)
    run_and_check(f"backward d {d}, S 2^17, causal, {str(dtype)[6:]}", p, dtype, t0)


@pytest.mark.parametrize("dtype", [f32, bf], ids=["fp32", "bf16"])
def test_grouped_backward_at_2_pow_16_rows(dtype):
    """G = 4: dK, dV are the sums over four query heads, each with its own targets"""
    need(8)
    t0 = time.time()
    S = 2 ** 16
    p = lp.build_backward(S, S, 128, 4, 1, True, seed=23, device=DEV)
    run_and_check(f"backward G 4, S 2^16, causal, {str(dtype)[6:]}", p, dtype, t0)


def test_backward_at_the_largest_accepted_extent():
    """256 rows against the longest dense d = 128 K / V flash_attention_backward accepts (long_probe.largest_accepted on zero tensors; a
    refusal is FA_ERR_BAD_SHAPE before any launch), not causal, bf16 gradients: about 2^15 key blocks, of which a few hold a targeted key"""
    need(24)
    t0 = time.time()
    Sq, d, hi = 256, 128, 2 ** 23
    Q, Kb, lse = (torch.zeros(s, dtype=t, device=DEV) for s, t in (((1, 1, Sq, d), bf), ((1, 1, hi, d), bf), ((1, 1, Sq), f32)))
    G = torch.empty((1, 1, hi, d), dtype=bf, device=DEV)

    def accepted(c):
        try:
            fa.flash_attention_backward(Q, Kb[:, :, :c], Kb[:, :, :c], Q, Q, lse, scale=0.125, dQ=torch.empty_like(Q), dK=G[:, :, :c], dV=G[:, :, :c])
            return True
        except fa.FlashAttentionError as e:
            assert e.code == -3, e
            return False

    cap = lp.largest_accepted(accepted, hi)
    torch.cuda.synchronize()
    assert (cap + 1 + 192) * 2 * d >= 2 ** 31 > cap * 2 * d
    print(f"largest accepted Sk of the backward at a row stride of {2 * d} bytes: {cap} = 2^23 - {2 ** 23 - cap}")
    del Q, Kb, G, lse
    p = lp.build_backward(Sq, cap, d, 1, 1, False, seed=25, device=DEV)
    for line in lp.BYTE_LINES:
        assert f"first key past byte {line}" in p["named"]
    run_and_check(f"backward cross, Sq {Sq} Sk {cap}, bf16", p, bf, t0)
