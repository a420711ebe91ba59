"""The selection harness checked on the CPU (tests/selection_cases.py; tests/test_gpu_selection.py runs it against the kernels):
order() against a brute-force minimum extraction, the derived error bounds against a numpy emulation of the device's order of
operations on every node set the GPU tests use -- and against the one-pass variance they must reject --, and the counts of the cases
the builders produce, so that none of them can silently degenerate."""
import math
from fractions import Fraction

import numpy as np
import pytest

import selection_cases as sc


def brute_order(ret, skip=-1):
    """repeated extraction of the minimum, written without a sort and without a key: a finite or infinite return beats a NaN, a
    smaller one beats a larger one, equal ones (-0.0 == +0.0) and two NaN go to the lower index"""
    left = [i for i in range(len(ret)) if i != skip]
    out = []
    while left:
        best = left[0]
        for i in left[1:]:
            a, b = ret[i], ret[best]
            a_nan, b_nan = math.isnan(a), math.isnan(b)
            if (b_nan and not a_nan) or (not a_nan and not b_nan and a < b):
                best = i          # (i > best throughout: a tie keeps the earlier one)
        out.append(best)
        left.remove(best)
    return np.array(out, dtype=np.int32)


def test_order_equals_brute_force_extraction():
    nan, inf = float("nan"), float("inf")
    vectors = [[3.0], [nan], [2.0, 2.0], [nan, 1.0], [0.0, -0.0, 1.0], [-0.0, 0.0, -1.0], [inf, -inf, nan, 0.0], [nan, nan, nan],
               [1e6, 5.0, 1e6, nan, 5.0, -inf, inf, -0.0, 0.0, sc.NEG_NAN, 2.5]]
    rng = np.random.default_rng(3)
    pool = np.array([nan, sc.NEG_NAN, inf, -inf, 0.0, -0.0, 1.0, 1.0, 2.0, 1e6, 1e6, -3.0])
    vectors += [list(rng.choice(pool, size=n)) for n in (2, 3, 5, 8, 13, 21, 34) for _ in range(6)]
    for v in vectors:
        for skip in (-1, 0, len(v) - 1, len(v)):
            assert np.array_equal(sc.order(v, skip), brute_order(v, skip)), (v, skip)
    # the signed zeros tie by index, whichever sign comes first; a NaN never precedes a number
    assert list(sc.order([0.0, -0.0])) == [0, 1] and list(sc.order([-0.0, 0.0])) == [0, 1]
    assert list(sc.order([nan, inf, -inf])) == [2, 1, 0]
    for n in (1, 2, 3, 65):
        for c in sc.plain_cases(n):
            assert np.array_equal(sc.order(c.ret), brute_order(c.ret)), (n, c.name)


def _winner_counts(cases):
    counts = {}
    for c in cases:
        counts[c.winner] = counts.get(c.winner, 0) + 1
    return counts


# (cases, with a NaN, with a tie between numbers, with an infinity, with both zeros, with failed rollouts)
PLAIN_COUNTS = {1: (4, 1, 0, 0, 0, 0), 2: (10, 2, 4, 2, 2, 0), 3: (16, 6, 6, 3, 2, 2), 63: (23, 6, 12, 3, 2, 2), 64: (23, 6, 12, 3, 2, 2),
                65: (26, 6, 14, 3, 2, 2), 1023: (30, 6, 17, 3, 2, 2), 1024: (30, 6, 17, 3, 2, 2), 1025: (33, 6, 19, 3, 2, 2),
                2049: (37, 6, 22, 3, 2, 2)}
SEG_COUNTS = {64: (23, 6, 12, 3, 2, 2), 256: (30, 6, 17, 3, 2, 2), 320: (37, 6, 22, 3, 2, 2), 1024: (37, 6, 22, 3, 2, 2),
              1088: (37, 6, 22, 3, 2, 2)}


@pytest.mark.parametrize("n", sc.PLAIN_N)
def test_plain_cases_are_what_they_say(n):
    cases = sc.plain_cases(n)
    assert len({c.name for c in cases}) == len(cases)
    places = [p for p in sc.PLAIN_PLACES + (n - 1,) if p < n]
    wins = _winner_counts(cases)
    for p in places:                                   # the unique minimum and a tied pair's first at every place that fits
        assert wins.get(p, 0) >= (2 if p < n - 1 else 1), (n, p, wins)
    for a, b in sc.PLAIN_STRADDLES:
        if b < n:                                      # a tie across every boundary that fits, and nothing else as low
            c = next(c for c in cases if c.name == f"tie@{a},{b}")
            assert c.ret[a] == c.ret[b] == c.ret.min() and (c.ret == c.ret.min()).sum() == 2 and c.winner == a
    for c in cases:
        assert c.ret.shape == (n,) and c.ret.dtype == np.float64 and c.fail.shape == (n,) and c.fail.dtype == np.int32
        assert np.array_equal(c.fail != 0, (c.ret == sc.FAILED) | ~np.isfinite(c.ret))
    # how many cases there are, and how many of them have a NaN, a tie between numbers, an infinity, both zeros, failed rollouts
    got = (len(cases), sum(c.nans > 0 for c in cases), sum(c.has_tie for c in cases), sum(c.has_inf for c in cases),
           sum(c.has_signed_zeros for c in cases), sum(c.has_failed for c in cases))
    assert got == PLAIN_COUNTS[n], (n, got)
    assert sum(c.nans == n for c in cases) == 1 and sum(c.name == "all-equal" for c in cases) == 1
    assert any(c.fail.max() > 255 for c in cases) or n < 3    # the diagnostics above the low byte ride along
    # the base of every case is a permutation of distinct values: nothing ties by accident
    assert np.unique(sc.base(n, 1)).size == n


@pytest.mark.parametrize("n_env", sc.SEG_N)
def test_segmented_cases_are_what_they_say(n_env):
    cases = sc.segmented_cases(n_env)
    wins = _winner_counts(cases)
    for p in [p for p in sc.SEG_PLACES + (n_env - 1,) if p < n_env]:
        assert wins.get(p, 0) >= (2 if p < n_env - 1 else 1), (n_env, p, wins)
    for a, b in sc.SEG_STRADDLES:
        if b < n_env:
            assert next(c for c in cases if c.name == f"tie@{a},{b}").winner == a
    rounds = sc.segmented_rounds(n_env)
    assert len(rounds) == len(cases)
    for r in rounds:                                   # a different case in every environment, every case in every environment once
        assert len(r) == sc.SEG_E and len({c.name for c in r}) == sc.SEG_E
    for e in range(sc.SEG_E):
        assert {r[e].name for r in rounds} == {c.name for c in cases}
    got = (len(cases), sum(c.nans > 0 for c in cases), sum(c.has_tie for c in cases), sum(c.has_inf for c in cases),
           sum(c.has_signed_zeros for c in cases), sum(c.has_failed for c in cases))
    assert got == SEG_COUNTS[n_env], (n_env, got)
    ks = sc.elite_counts(n_env)
    assert ks[0] == 1 and ks[-1] == n_env and n_env - 1 in ks
    assert sc.elite_counts(n_env, skip=0)[-1] == n_env - 1
    want = {64: [1, 2, 63, 64], 256: [1, 2, 255, 256], 320: [1, 2, 255, 256, 257, 319, 320], 1024: [1, 2, 255, 256, 257, 513, 1023, 1024],
            1088: [1, 2, 255, 256, 257, 513, 1087, 1088]}[n_env]
    assert ks == want


ELITES = (2, 3, 72, 255, 256, 257, 513, 1087, 8255)    # the elite counts the GPU tests reduce over, both sides of every trip of the stride


@pytest.mark.parametrize("kind", sorted(sc.NODE_SETS))
@pytest.mark.parametrize("precision", [64, 32])
def test_the_device_order_of_operations_stays_inside_the_bounds(kind, precision):
    worst = dict(sum=0.0, mean=0.0, sq=0.0, var=0.0)
    for n in ELITES:
        nodes = sc.as_device(sc.NODE_SETS[kind](n, 1, seed=n), precision)
        elites = np.random.default_rng(n).permutation(n)           # rank order is not index order
        col = nodes[elites, 0]
        total, mean, sq, var = sc.emulate_moments(col)
        ex = sc.exact_moments(nodes, np.zeros(n), elites, mean=[mean], precision=precision)
        worst["sum"] = max(worst["sum"], sc.ratio(total, ex["sum"][0], sc.sum_bound(n, ex["abs_sum"][0])))
        worst["mean"] = max(worst["mean"], sc.ratio(mean, ex["mean"][0], sc.mean_bound(n, ex["abs_sum"][0])))
        worst["sq"] = max(worst["sq"], sc.ratio(sq, ex["sq"][0], sc.square_bound(n) * ex["sq"][0]))
        worst["var"] = max(worst["var"], sc.ratio(var, ex["sq"][0] / (n - 1), sc.square_bound(n) * ex["sq"][0] / (n - 1)))
    print(f"{kind} fp{precision}: worst error / bound {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst


def test_the_one_pass_variance_is_rejected_on_the_ill_conditioned_set():
    """the figures of the module docstring: on 513 elites of the ill-conditioned set (m = 3) the device's order of operations is
    within about 1 u of the sum (15 u allowed) and of the variance (23 u allowed); E[x^2] - E[x]^2 is off by many times the
    variance itself"""
    n = 513
    nodes = sc.ill_nodes(n, 1, seed=7)
    elites = np.arange(n)
    total, mean, sq, var = sc.emulate_moments(nodes[:, 0])
    ex = sc.exact_moments(nodes, np.zeros(n), elites, mean=[mean])
    u = float(sc.U)
    sum_err_u = abs(Fraction(total) - ex["sum"][0]) / ex["abs_sum"][0] / sc.U
    var_exact = ex["sq"][0] / (n - 1)
    var_err_u = abs(Fraction(var) - var_exact) / var_exact / sc.U
    assert sc.trips(n) == 3 and float(sc.sum_bound(n, 1)) == 11 * u and float(sc.square_bound(n)) == 19 * u
    assert sum_err_u <= 11 and var_err_u <= 19
    _, mean1, _, var1 = sc.emulate_moments(nodes[:, 0], one_pass=True)
    assert mean1 == mean
    off = abs(Fraction(var1) - var_exact) / var_exact
    print(f"two-pass: sum {float(sum_err_u):.2f} u, variance {float(var_err_u):.2f} u; one-pass variance off by {float(off):.1f} x the exact value")
    assert off >= 0.5                                              # not a digit of it is right
    assert sc.ratio(var1, var_exact, sc.square_bound(n) * var_exact) > 1e6
    # a lost tail (the stride loop's second trip dropped) and a wrong divisor are far outside the bounds too
    lost = sc.emulate_elite_reduce(nodes[:sc.STRIDE, 0])
    assert sc.ratio(lost, ex["sum"][0], sc.sum_bound(n, ex["abs_sum"][0])) > 1e6
    assert sc.ratio(sq / n, var_exact, sc.square_bound(n) * var_exact) > 1e6


def test_exact_moments_are_exact():
    nodes = np.array([[0.1, 1.0], [0.2, 2.0 ** -60], [0.3, -1.0]])
    ex = sc.exact_moments(nodes, [1.0, np.nan, 2.0], [2, 0])
    assert ex["sum"][0] == Fraction(0.3) + Fraction(0.1) and ex["sum"][1] == 0 and ex["abs_sum"][1] == 2
    assert ex["mean"][0] == (Fraction(0.3) + Fraction(0.1)) / 2 and ex["ret_sum"] == 3 and ex["ret_abs_sum"] == 3
    assert ex["sq"][1] == 2                                        # about the exact mean, 0
    assert sc.exact_moments(nodes, [1.0, np.nan, 2.0], [0, 1, 2], mean=[0.0, 1.0])["sq"][1] == (Fraction(2.0 ** -60) - 1) ** 2 + 4
    assert sc.exact_moments(nodes, [1.0, np.nan, 2.0], [1])["ret_sum"] is None
    third = sc.exact_moments(np.array([[1.0 / 3.0]]), [0.0], [0], precision=32)["sum"][0]
    assert third == Fraction(float(np.float32(1.0 / 3.0))) != Fraction(1.0 / 3.0)
    # the emulation adds in the device's order: 256 partial sums first, so 1 + 2^-53 * 256 terms loses what a running sum keeps
    v = np.concatenate([[1.0], np.full(511, 2.0 ** -53)])
    assert sc.emulate_elite_reduce(v) == 1.0 + 510 * 2.0 ** -53 and sc.emulate_elite_reduce([]) == 0.0
