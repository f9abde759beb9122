"""GPU: exact single-key probes of the fp8 (e4m3fn) and bf16 input paths (tests/format_probe.py; CPU proof of the instrument:
tests/test_format_probe.py).  Every row of every call sees one key with a softmax weight of exactly 1, so O is the probed V row times
its descale -- compared BIT FOR BIT, the sign of a zero included -- and the LSE is scale q K k_descale, held to the derived relative
bound fp.LSE_REL with no absolute term.  Every finite e4m3fn code (subnormals, -0, +-448) stands at every column of every fp8 tensor
and at every key position of the tiles:

  decode K (fp8x8_to_bf16x8 into the MFMA operand, the KV8 d order) and V (widened into the LDS image): window = 1 under the mask,
      contiguous and paged (pages of 16 and 128), d = 64 / 128, 1 / 2 / planned splits, two K/V heads with their own descales, descales
      that are no powers of two; kv_lens = 1 without a window, masked and not, through both entry points;
  decode, bf16 cache: +-0, +-2^-126, +-1, +-max finite in the codes' place -- "any finite bf16 V" at the extreme;
  prefill Q / K (raw bytes into the block-scaled MFMA, K staged by LDS-DMA): Sk = 1 read-outs of K and of Q;
  prefill V (loaders.hip.h, widened on its way into LDS): every key of a 64-key tile and the first of the next, by score, one unit per
      workgroup and a persistent walk of several, fp32 and bf16 outputs -- the first query block through the tracked pass, the second
      through the optimistic one;
  the weights kernel (elem_traits<fp8_t>): the single weight of the K read-out is 1 to 2 ulp."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import format_probe as fp  # noqa: E402
import forward_routes as fr  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(fp.FP8 is None, reason="torch has no float8_e4m3fn")]
DEV = "cuda:0"


def dev(t):
    return t.to(DEV).view(fp.FP8) if t.dtype == torch.uint8 else t.to(DEV)


@functools.lru_cache(maxsize=2)
def case(maker, *args):
    p = maker(*args)
    return p, fp.expected(p)


def run_decode(p, page=0, splits=0, out_dtype=torch.float32):
    lens = torch.tensor(p["lens"], dtype=torch.int32, device=DEV)
    kw = dict(scale=p["scale"], is_causal=p["causal"], out_dtype=out_dtype, num_splits=splits, return_lse=True, window=p["window"] or None)
    if p["kd"] is not None:
        kw.update(k_descale=p["kd"].to(DEV), v_descale=p["vd"].to(DEV))
    if page:
        (Kp, table), (Vp, table_v) = fp.paged(p["K"], page), fp.paged(p["V"], page)
        assert torch.equal(table, table_v)
        out = fa.flash_attention_decode_paged(dev(p["Q"]), dev(Kp), dev(Vp), table.to(DEV), lens, **kw)
    else:
        out = fa.flash_attention_decode(dev(p["Q"]), dev(p["K"]), dev(p["V"]), lens, **kw)
    torch.cuda.synchronize()
    return out


def run_prefill(p, out_dtype=torch.float32):
    out = fa.flash_attention(dev(p["Q"]), dev(p["K"]), dev(p["V"]), scale=p["scale"], is_causal=p["causal"], out_dtype=out_dtype, return_lse=True)
    torch.cuda.synchronize()
    return out


def planned_splits(p, splits):
    B, H, Sq, d = p["Q"].shape
    return fa.decode_plan(B, H, p["K"].shape[1], Sq, p["K"].shape[2], d, fa.FA_DTYPE_F32, splits, p["window"])["num_splits"]


@pytest.mark.parametrize("page", [0, 16, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_decode_fp8_cache_reads_out_every_code_at_every_key(d, page):
    p, (expO, expL) = case(fp.decode_family, d)
    first = None
    for splits in (1, 2, 0):
        ns = planned_splits(p, splits)
        assert ns == splits or splits == 0
        O, lse = run_decode(p, page, splits)
        fp.check(f"{p['name']} page {page} splits {ns}", O, lse, expO, expL)
        first = first or (O, lse)
    if page:   # paged equals contiguous bit for bit
        O0, lse0 = run_decode(p, 0, 1)
        assert torch.equal(first[0].view(torch.int32), O0.view(torch.int32)) and torch.equal(first[1].view(torch.int32), lse0.view(torch.int32))
    for odt in (torch.bfloat16, torch.float16):   # the fp32 value rounded once
        Ob, lse = run_decode(p, page, 0, odt)
        fp.check(f"{p['name']} page {page} {odt} output", Ob, lse, expO, expL)


@pytest.mark.parametrize("kd,vd", [((0.25, 2.0), (8.0, 0.5)), ((0.0123, 3.7), (3.7, 0.0123))], ids=["pow2", "not_pow2"])
@pytest.mark.parametrize("page", [0, 16])
def test_decode_fp8_cache_with_a_descale_per_head(page, kd, vd):
    p, (expO, expL) = case(fp.decode_family, 128, 2, kd, vd)
    O, lse = run_decode(p, page, 0)
    fp.check(f"{p['name']} page {page}", O, lse, expO, expL)


@pytest.mark.parametrize("page", [0, 16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_decode_fp8_cache_without_a_window(d, causal, page):
    p, (expO, expL) = case(fp.decode_key0_family, d, causal)
    for splits in (0, 2):
        O, lse = run_decode(p, page, splits)
        fp.check(f"{p['name']} page {page} splits {splits}", O, lse, expO, expL)


@pytest.mark.parametrize("page", [0, 16])
@pytest.mark.parametrize("d", [64, 128])
def test_decode_bf16_cache_reads_out_every_class(d, page):
    p, (expO, expL) = case(fp.decode_family, d, 1, (0.25,), (8.0,), "bf16")
    for splits in (1, 0):
        O, lse = run_decode(p, page, splits)
        fp.check(f"{p['name']} page {page} splits {splits}", O, lse, expO, expL)
        assert torch.equal(O.cpu() + 0.0, fp._gather(p, p["Q"], p["K"], p["V"])[2].float() + 0.0)      # O is V (a -0 reads +0)


def codes(odt):
    return fa.FA_DTYPE_FP8_E4M3, {torch.float32: fa.FA_DTYPE_F32, torch.bfloat16: fa.FA_DTYPE_BF16}[odt]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("maker", [fp.prefill_k_family, fp.prefill_q_family], ids=["K", "Q"])
def test_prefill_fp8_reads_out_k_and_q(maker, causal):
    p, (expO, expL) = case(maker, causal)
    B, H, Sq, d = p["Q"].shape
    for odt in (torch.float32, torch.bfloat16):
        assert fr.family(B, H, Sq, 1, d, causal, *codes(odt), 0) == "fp8"
        O, lse = run_prefill(p, odt)
        fp.check(f"{p['name']} {odt}", O, lse, expO, expL)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,walk", [(4, False), (132, True)], ids=["unit_per_workgroup", "persistent_walk"])
def test_prefill_fp8_reads_out_v_at_every_key_of_a_tile(H, walk, causal):
    """The fp8 prefill has one kernel family and never takes the pair kernel (pair_kernel_applies in csrc/FlashAttention.hip wants bf16
    inputs), so the two routes of the V read-out are the two ways its persistent grid is used: a workgroup per unit (8 units), and
    more units than workgroups (264), where some workgroup walks on to a second unit and fetches its tile 0 under the epilogue."""
    p, (expO, expL) = case(fp.prefill_v_family, H, causal)
    for odt in (torch.float32, torch.bfloat16):
        assert fr.family(1, H, fp.V_SQ, fp.V_SK, 128, causal, *codes(odt), 0) == "fp8"
        units, grid = fr.walks(1, H, fp.V_SQ, fp.V_SK, 128, causal, *codes(odt))
        assert units == 2 * H and (units > grid) == walk, (units, grid)       # some workgroup walks two units, or none does
        O, lse = run_prefill(p, odt)
        fp.check(f"{p['name']} {odt} ({units} units on {grid} workgroups)", O, lse, expO, expL)


@pytest.mark.parametrize("causal", [False, True])
def test_weights_kernel_reads_fp8_exactly(causal):
    """P = expf(fma(s, scale, -LSE)) with s = q K exact.  The forward's LSE is fp32(s 2^k ln 2) (fp.PREFILL_SCALE: c = 2^k, the sum is
    exactly 1), scale is fp32(ln 2) 2^k, so the argument is the rounding residual of one fp32 product, at most 2^-24 |LSE| <= 2^-24 x
    1.22 (|s| <= 896, k = -9) -- or exactly 0 where the compiler does not contract the fma.  exp of it is within 1.22 x 2^-24 of 1, and
    expf adds its documented 1 ulp (2^-23 above 1): under 2 ulp = 2^-22 together."""
    p, (expO, expL) = case(fp.prefill_k_family, causal)
    assert float(expL.abs().max()) <= 1.22 and p["scale"] == fp.PREFILL_SCALE(-9)
    O, lse = run_prefill(p)
    fp.check(f"{p['name']} (for the weights)", O, lse, expO, expL)
    P = fa.attention_weights(dev(p["Q"]), dev(p["K"]), lse, scale=p["scale"], is_causal=causal)
    torch.cuda.synchronize()
    err = (P.double().cpu() - 1.0).abs().max().item()
    print(f"weights kernel, fp8 K read-out, mask {causal}: worst |P - 1| = {err / 2.0 ** -23:.3f} ulp")
    assert P.shape == (1, 256, 128, 1) and err <= 2.0 * 2.0 ** -23
