"""CPU tests of the precision checker (tests/precision_check.py), by the protocol of tests/test_weight_probe.py: on every case the GPU
tests run (tests/test_kv_precision.py) -- or its twin on the same logical tensors, where the case is a paged form -- the emulation of
the documented arithmetic stays at or below 0.5 of both bounds, and each of the four mutants (the lo term dropped, l summed over the hi
weights, the partial O rounded to bf16 under more than one split, the scores rounded to bf16) is at least 4 x the O bound or 4 x the
LSE bound in its worst element.  Conditions, not measurements: a case that misses one gets other data, not another threshold.  And the
gap itself, as a test: on plain N(0, 1) data and at least 384 keys the STATED tolerance admits the first two mutants.  No GPU and no
kernel: the library is asked for its plans only."""
import pytest

torch = pytest.importorskip("torch")

import precision_check as pc  # noqa: E402

GPU_CASES = [c for family in pc.SHAPES for form in (pc.TREE_FORMS if family == "tree" else pc.FORMS) for d in (64, 128)
             for c in pc.cases(family, form, d)] + pc.sink_cases()
TWINS = list(dict.fromkeys(pc.twin(c) for c in GPU_CASES))      # in order, each once
FAMILY_FORM_D = list(dict.fromkeys((c.family, c.form, c.d) for c in TWINS))


def prove(c, splits, at_least=None):
    """the conditions on one case under every split count of `splits`; the worst figures.  at_least: a mutant's own threshold, where it
    is not MUTANT_AT_LEAST"""
    seen, emu, least = {}, [0.0, 0.0], {}
    for ns in splits:
        n, _ = pc.plan_of(c, ns)
        if n in seen:                                   # (the same launches: e.g. the library's choice is one split)
            continue
        seen[n] = ns
        r, lr = pc.worst(c, *pc.emulate(c, ns))
        emu = [max(emu[0], r), max(emu[1], lr)]
        assert r <= pc.EMULATION_AT_MOST and lr <= pc.EMULATION_AT_MOST, f"{pc.name_of(c)} splits {n}: the emulation is at {r:.3f} / {lr:.3f} of the bounds"
        for mutant in pc.MUTANTS:
            if mutant == "partial_bf16" and n == 1:
                continue
            reach = max(pc.worst(c, *pc.emulate(c, ns, mutant)))
            least[mutant] = min(least.get(mutant, float("inf")), reach)
            assert reach >= (at_least or {}).get(mutant, pc.MUTANT_AT_LEAST), f"{pc.name_of(c)} splits {n}: mutant {mutant} reaches only {reach:.2f} x a bound"
    return emu, least, seen


@pytest.mark.parametrize("family,form,d", FAMILY_FORM_D, ids=lambda v: pc.FORM_IDS[pc.FORMS.index(v)] if isinstance(v, tuple) else str(v))
def test_bound_admits_the_emulation_and_refuses_every_mutant(family, form, d):
    mine = [c for c in TWINS if (c.family, c.form, c.d) == (family, form, d)]
    assert mine
    emu, least = [0.0, 0.0], {}
    for c in mine:
        e, l, seen = prove(c, pc.SPLITS)
        assert len(seen) >= 2 and 1 in seen, seen         # one split and more than one were both emulated
        emu = [max(a, b) for a, b in zip(emu, e)]
        least = {m: min(least.get(m, float("inf")), v) for m, v in l.items()}
    assert set(least) == set(pc.MUTANTS)
    print(f"{family} {pc.FORM_IDS[pc.FORMS.index(form)]} d{d}: {len(mine)} cases; emulation at most {emu[0]:.3f} (O) {emu[1]:.3f} (LSE) of the bound; "
          "least mutant reach " + ", ".join(f"{m} {v:.1f}" for m, v in least.items()))


def test_every_gpu_case_has_its_twin_among_the_proven():
    assert {pc.twin(c) for c in GPU_CASES} == set(TWINS)
    for c in GPU_CASES:
        a, b = pc.data(c)["cache"], pc.data(pc.twin(c))["cache"]
        assert torch.equal(a.refK, b.refK) and torch.equal(a.refV, b.refV), pc.name_of(c)


def test_long_case():
    """2^15 keys.  Three mutants reach 4 x a bound.  The fourth, l summed over the hi weights, cannot on such a row, whatever the data:
    its error is a relative 2^-8 x 0.3 / sqrt(effective number of weights) of l, against 4 x (1e-5 + 16 max(smax, 4) 2^-23) -- few
    enough weights need scores so far apart that smax takes the bound along (scores of deviation 3, as here, reach about 2 x; wider and
    narrower ones less), and a row of one weight has l = 1 exactly.  It is held to what the GPU test needs to refuse it: outside the
    bound"""
    for c in pc.long_cases():
        n, _ = pc.plan_of(c, 0)
        assert n > 2, n
        emu, least, _ = prove(c, (0,), at_least={"l_over_hi": 1.0 + 1e-9})
        print(f"{pc.name_of(c)}: {n} splits; emulation {emu[0]:.3f} (O) {emu[1]:.3f} (LSE); least mutant reach "
              + ", ".join(f"{m} {v:.1f}" for m, v in least.items()))
        assert set(least) == set(pc.MUTANTS)


@pytest.mark.parametrize("c", pc.plain_cases(), ids=lambda c: f"{c.family}-d{c.d}")
def test_stated_tolerance_admits_the_first_two_mutants(c):
    """plain N(0, 1), the sequences of at least 384 keys (640 and 2048): both mutants' O is within the stated tolerance, and so is the LSE
    of the first.  The LSE of the second -- its error is the relative error of l, which falls with the square root of the keys -- is
    within it at 2048 keys and NOT at 640 (up to 1.5 x 2e-4 in the worst row: printed), so kv_cache_check.assert_close can see that
    mutant through the LSE of a short cache, and through nothing else"""
    for ns in (1, 3):
        for mutant in pc.MUTANTS[:2]:
            O, lse = pc.emulate(c, ns, mutant)
            r, lr = pc.stated(c, O, lse, at_least=384)
            _, lr_long = pc.stated(c, O, lse, at_least=pc.PLAIN_KEYS)
            print(f"{pc.name_of(c)} splits {ns} {mutant}: {r:.3f} (O) {lr:.3f} (LSE; at {pc.PLAIN_KEYS} keys {lr_long:.3f}) of the stated tolerance")
            assert r <= 1.0 and (lr if mutant == "no_lo" else lr_long) <= 1.0


def test_block_ranges_follow_the_kernel():
    # decode (16-row blocks): every block walks [first, len) whatever its rows
    assert list(pc.block_ranges(300, 5, 7, 16, True, 0)) == [(0, 16, 0, 3), (16, 32, 0, 3), (32, 35, 0, 3)]
    assert list(pc.block_ranges(640, 16, 1, 16, True, 100)) == [(0, 16, 4, 5)]
    # chunked prefill (64-row blocks), causal: a block within one head stops at its last row's limit; one that straddles heads does not
    assert list(pc.block_ranges(300, 200, 1, 64, True, 0)) == [(0, 64, 0, 2), (64, 128, 0, 2), (128, 192, 0, 3), (192, 200, 0, 3)]
    assert list(pc.block_ranges(300, 65, 2, 64, True, 0)) == [(0, 64, 0, 3), (64, 128, 0, 3), (128, 130, 0, 3)]
    # ... and under a window starts at its smallest row's left edge
    assert list(pc.block_ranges(640, 65, 1, 64, True, 100)) == [(0, 64, 3, 5), (64, 65, 4, 5)]
