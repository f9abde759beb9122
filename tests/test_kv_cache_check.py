"""CPU tests of tests/kv_cache_check.py itself: what every K/V-cache test now shares.  `visible()` against a literal double loop over
(row, key) written from the sentences of include/flash_attention.h -- windows, both masks, tree words -- and the criterion at its
boundary: an element at 0.99 x the stated tolerance is admitted, one at 1.01 x is refused, a NaN is refused."""
import itertools

import pytest

torch = pytest.importorskip("torch")

import kv_cache_check as kv  # noqa: E402
import tree_check as tc  # noqa: E402

LENGTHS = tuple(range(1, 21)) + (127, 128, 129)


def by_the_header(L, Sq, causal, W, words=None):
    """the header, word for word: limC_i = max(len - Sq + i + 1, 1), lo_i = max(limC_i - W, 0) (W = 0: 0); row i sees lo_i <= k < limC_i
    with is_causal and lo_i <= k < len without; under a tree mask also k < base, or bit k - base of the row's word set, or k == lim_i - 1"""
    base = L - Sq
    want = torch.zeros(Sq, L, dtype=torch.bool)
    for i in range(Sq):
        lim = max(L - Sq + i + 1, 1)
        lo = max(lim - W, 0) if W else 0
        for k in range(L):
            seen = lo <= k < (lim if causal else L)
            if words is not None:
                seen = seen and (k < base or (k - base >= 0 and words[i] >> (k - base) & 1 == 1) or k == lim - 1)
            want[i, k] = seen
    return want


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Sq", [1, 3, 16, 17])
def test_visible_is_the_headers_rule(Sq, causal):
    for L in LENGTHS:
        for W in (0, 1, 2, 7, L):
            got = kv.visible(L, Sq, causal, W)
            assert got.dtype == torch.bool and torch.equal(got, by_the_header(L, Sq, causal, W)), (L, Sq, causal, W)
            assert bool(got.any(1).all()), (L, Sq, causal, W)                                   # every row sees a key
            assert int(got.any(0).nonzero()[0]) == kv.first_visible(L, Sq, W), (L, Sq, causal, W)


@pytest.mark.parametrize("Sq", [3, 5])
def test_visible_under_tree_words_is_the_headers_rule(Sq):
    families = {"chain": tc.words_of("chain", Sq), "star": tc.words_of("star", Sq), "random": tc.words_of("random", Sq, seed=1)}
    assert families["star"] == [1 << i for i in range(Sq)] and families["chain"] == [(2 << i) - 1 for i in range(Sq)]
    for (name, words), L in itertools.product(families.items(), LENGTHS):
        for W in (0, 1, 2, 7, L):
            got = kv.visible(L, Sq, True, W, words)
            assert torch.equal(got, by_the_header(L, Sq, True, W, words)), (name, L, Sq, W)
            assert bool(got.diagonal(L - Sq).all()), (name, L, Sq, W)                               # the own key, always
            if name == "chain":
                assert torch.equal(got, kv.visible(L, Sq, True, W)), (L, Sq, W)                   # the causal twin


def test_the_criterion_at_its_boundary():
    refO = torch.tensor([[0.0, 1.0, -250.0, 1e30]], dtype=torch.float64)
    refL = torch.tensor([0.0, -7.5, 100.0, 1e4], dtype=torch.float64)
    tol, ltol = 1e-3 + 1e-3 * refO.abs(), 2e-4 + 2e-6 * refL.abs()
    for sign in (1.0, -1.0):
        r, lr = kv.ratios(refO + sign * 0.99 * tol, refL + sign * 0.99 * ltol, refO, refL)
        assert (r <= 1).all() and (lr <= 1).all() and (r > 0.98).all() and (lr > 0.98).all()
        kv.assert_close(refO + sign * 0.99 * tol, refL + sign * 0.99 * ltol, refO, refL, "0.99 x the tolerance")
        for j in range(4):
            O, lse = refO.clone(), refL.clone()
            O[0, j] += sign * 1.01 * tol[0, j]
            r, lr = kv.ratios(O, refL, refO, refL)
            assert int((r > 1).sum()) == 1 and r[0, j] > 1 and not (lr > 0).any()
            with pytest.raises(AssertionError, match="1 elements outside"):
                kv.assert_close(O, refL, refO, refL, "one element of O at 1.01 x")
            lse[j] += sign * 1.01 * ltol[j]
            r, lr = kv.ratios(refO, lse, refO, refL)
            assert int((lr > 1).sum()) == 1 and lr[j] > 1 and not (r > 0).any()
            assert torch.equal(lr, kv.lse_ratio(lse, refL)) and kv.lse_ratio(lse[j], float(refL[j])) > 1
            with pytest.raises(AssertionError, match="LSE error"):
                kv.assert_close(refO, lse, refO, refL, "one LSE at 1.01 x")


def test_the_criterion_refuses_a_nan():
    refO, refL = torch.ones(1, 4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    O, lse = refO.clone(), refL.clone()
    O[0, 2], lse[1] = float("nan"), float("nan")
    r, lr = kv.ratios(O, lse, refO, refL)
    assert not (r <= 1).all() and not (lr <= 1).all() and int((r <= 1).sum()) == 3 and int((lr <= 1).sum()) == 3
    for o, l in ((O, refL), (refO, lse), (refO * float("inf"), refL)):
        with pytest.raises(AssertionError):
            kv.assert_close(o, l, refO, refL, "not finite")
