"""GPU tests of the K/V-cache calls' own precision: every element of an fp32 O and of the LSE within the bound of the documented
arithmetic (tests/precision_check.py: 1e-5 + 1e-5 |ref| + (2^-17 + 8 max(smax, 4) 2^-23) ref_abs on O, 1e-5 + 16 max(smax, 4) 2^-23 +
2^-22 |ref| on the LSE), two orders of magnitude inside the stated tolerance that every other test of these calls asserts.  Decode,
chunked prefill and the ragged call on the four cache forms, the tree call on contiguous bf16 and paged fp8 with descales that are no
powers of two, each family once with sinks, d 64 and 128, num_splits 1, 3, the cap and the library's choice, window 0 and 100, at
B = 3 (the ragged call: 4), Hkv 1 and 3, G 1, 3, 7 and once 4, capacity 640; and one cache of 2^15 keys.  tests/test_precision_check.py
proves on the CPU, for every case here, that the bound admits the documented arithmetic and refuses four wrong kernels."""
import pytest

torch = pytest.importorskip("torch")

import precision_check as pc  # noqa: E402

pytestmark = pytest.mark.gpu


def sweep(cases, splits, what):
    """every case under every split count; prints each call's worst ratios and the worst of all"""
    devs, top = {}, [0.0, 0.0]
    for c in cases:
        cache = pc.data(c)["cache"]
        if id(cache) not in devs:
            devs[id(cache)] = (cache, cache.device())
        for ns in splits:
            O, lse = pc.run(c, devs[id(cache)][1], ns)
            r, lr = pc.check(c, O, lse, f"{pc.name_of(c)} splits{ns}")
            top = [max(top[0], r), max(top[1], lr)]
    print(f"WORST {what}: O error / bound {top[0]:.3f}, LSE error / bound {top[1]:.3f} ({len(cases)} cases x {len(splits)} split counts)")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("form", pc.FORMS, ids=pc.FORM_IDS)
@pytest.mark.parametrize("family", ["decode", "extend", "varlen"])
def test_reads_stay_within_the_bound_of_their_arithmetic(family, form, d):
    sweep(pc.cases(family, form, d), pc.SPLITS, f"{family} {pc.FORM_IDS[pc.FORMS.index(form)]} d{d}")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("form", pc.TREE_FORMS, ids=[pc.FORM_IDS[pc.FORMS.index(f)] for f in pc.TREE_FORMS])
def test_tree_reads_stay_within_the_bound(form, d):
    sweep(pc.cases("tree", form, d), pc.SPLITS, f"tree {pc.FORM_IDS[pc.FORMS.index(form)]} d{d}")


@pytest.mark.parametrize("family", list(pc.SINK_SHAPES))
def test_reads_with_sinks_stay_within_the_bound(family):
    sweep([c for c in pc.sink_cases() if c.family == family], pc.SPLITS, f"{family} with sinks")


@pytest.mark.parametrize("c", pc.long_cases(), ids=lambda c: pc.FORM_IDS[pc.FORMS.index(c.form)])
def test_long_cache_under_the_planned_splits(c):
    """2^15 keys x 35 rows: 256 tiles of fp32 accumulation and the combine of the planned split count"""
    n, _ = pc.plan_of(c, 0)
    assert n > 2, n
    sweep([c], (0,), f"2^15 keys {pc.FORM_IDS[pc.FORMS.index(c.form)]}, {n} splits")
