"""GPU: per-pair probes of the split-KV decode kernels' softmax weights (tests/weight_probe.py: P through V) over contiguous and paged,
bf16 and fp8 caches.  One sequence per length {1, Sq, 127, 128, 129, 640, capacity}, eight K/V heads, every (sequence, head) with a
window of its own: over the end of the length -- which holds the bottom-right diagonal of every packed row -- and over every tile seam
below it, which are the split boundaries of every split count run (1, 3, 64 and the planned one; wp.decode_seams asserts it from
decode_plan) and, for pages of 16 and 128 keys, page seams.  Every element of O is one weight, held to the bf16 line of the fuzz sweep's
bound against kv_cache_check.reference; keys past the length and pairs under the mask must read exactly 0.0.  One long case: 70 000 keys
x 2 rows, windows over the last split boundary and the end.  CPU proof of the instrument: tests/test_weight_probe.py."""
import functools

import pytest

import __graft_entry__ as entry

torch = pytest.importorskip("torch")
fa = entry.load_package()
import weight_probe as wp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CACHES = [("bf16", 0), ("fp8", 0), ("bf16", 16), ("bf16", 128), ("fp8", 16)]      # (cache type, page: 0 = contiguous)


@functools.lru_cache(maxsize=2)
def case(Sq, G, d, fp8, causal):
    p = wp.build_decode(Sq, G, d, fp8)
    return p, wp.decode_truth(p, causal)


def run(p, page, causal, splits):
    Q, lens = p["Q"].to(DEV), torch.tensor(p["lens"], dtype=torch.int32, device=DEV)
    kw = dict(is_causal=causal, out_dtype=torch.float32, num_splits=splits, return_lse=True)
    if p["kd"] is not None:
        kw.update(k_descale=p["kd"].to(DEV), v_descale=p["vd"].to(DEV))
    dev = lambda t: (t.view(torch.uint8).to(DEV).view(wp.FP8) if t.dtype == wp.FP8 else t.to(DEV))
    if page:
        (Kp, table), (Vp, table_v) = wp.paged(p["Kc"], page), wp.paged(p["Vc"], page)
        assert torch.equal(table, table_v)
        out = fa.flash_attention_decode_paged(Q, dev(Kp), dev(Vp), table.to(DEV), lens, **kw)
    else:
        out = fa.flash_attention_decode(Q, dev(p["Kc"]), dev(p["Vc"]), lens, **kw)
    torch.cuda.synchronize()
    return out


def check(p, t, O, lse, what):
    worst, pair = wp.report(what, wp.ratios(O.double().cpu(), t["O"], t["bound"]), p["w0"], p["G"])
    lr = ((lse.double().cpu() - t["lse"]).abs() / t["lse_bound"]).max().item()
    print(f"{what}: worst LSE error / bound {lr:.3f}")
    assert worst <= 1.0, f"{what}: pair (sequence, head, row, k) = {pair} at {worst:.3g} x the bound"
    assert torch.isfinite(lse).all() and lr <= 1.0, what


@pytest.mark.parametrize("cache,page", CACHES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("Sq,G,causal", wp.DEC_SHAPES)
def test_every_weight_of_the_windows(Sq, G, causal, d, cache, page):
    p, t = case(Sq, G, d, cache == "fp8", causal)
    B, H, Hkv = len(p["lens"]), G * wp.DEC_HKV, wp.DEC_HKV
    for splits in wp.DEC_SPLITS:
        ns = fa.decode_plan(B, H, Hkv, Sq, wp.DEC_CAP, d, fa.FA_DTYPE_F32, splits)["num_splits"]
        assert ns == splits or splits == 0
        O, lse = run(p, page, causal, splits)
        check(p, t, O, lse, f"decode {cache} page {page} Sq {Sq} G {G} d {d} mask {causal} splits {ns}")


def test_the_last_split_boundary_of_a_long_sequence():
    p = wp.build_decode_long()
    t = wp.decode_truth(p, True)
    assert fa.decode_plan(1, 2, 2, 2, wp.LONG_KEYS, 128, fa.FA_DTYPE_F32, 0)["num_splits"] > 1
    O, lse = run(p, 0, True, 0)
    check(p, t, O, lse, f"decode bf16 {wp.LONG_LEN} of {wp.LONG_KEYS} keys x 2 rows, windows at {p['w0'][0]}")
