"""MPPI harness (test infrastructure, like selection_cases.py; not a conftest, no GPU code of its own): the contract of
mjpcx_mppi_update_batched (include/mjpcx.h; mppi_weights_kernel / mppi_mean_kernel, csrc/mppi_update.h) in plain Python, its weights in
mpmath, its sums in exact rational arithmetic FROM THE WEIGHTS THE DEVICE REPORTED (which holds the sums apart from exp), the device's
order of operations in numpy, and the error bounds the device is held to. The return vectors, order(), inject() and the exact-arithmetic
helpers are selection_cases.py's, unchanged.

The contract, per environment over returns R[i], spline parameters p[i][j] and temperature lam:
    winner  order(R)[0] (ascending, ties to the lower index, NaN last), beta = R[winner]; valid = beta is a number below +inf
    w[i]    0 if R[i] is NaN; 1 if R[i] == beta; else exp(-((R[i] - beta) / lam)); all 0 when not valid
    eta = sum w, Q = sum w^2, S[j] = sum w[i] p[i][j], each 256 strided partial sums from zero, then the halving tree (elite_reduce)
    weight_sum = eta, effective_samples = eta^2 / Q, mean[j] = S[j] / eta; not valid: 0, 0, the spline of ref_candidate (NaN without one)

Bounds, derived, not measured. u = 2^-53, n the candidates of the environment, m = ceil(n / 256) (selection_cases.trips).

  weights   x = (R - beta) / lam exactly; the device forms fl(fl(R - beta) / lam) = x (1 + d1)(1 + d2), |d| <= u, so its argument is off by
            at most |x| (2 u + u^2). exp turns an absolute error d of its argument into the relative error |e^d - 1| <= |d| e^|d|; a result
            that is not zero has |x| < 746, so |d| < 2e-13 and that is 2 |x| u (1 + 2e-13). The device's exp adds its own error: ULP_FN
            ulp = 2 ULP_FN u relative, the project's standing ASSUMPTION for device math functions (sampling_policy_cases.py, 4 ulp; the
            same constant, imported). Together (1 + a)(1 + b) - 1 with a <= 2 |x| u, b <= 2 ULP_FN u:
                |w_dev - w| <= (2 |x| + 2 ULP_FN + 1) u w + 2^-1074                                              (weight_bound)
            where the + 1 covers every second-order term (a b < 1e-11 u) and 2^-1074, one subnormal spacing, is the floor for results
            below 2^-1022, whose rounding is absolute. R[i] == beta, NaN and invalid environments are exact (1, 0, 0).
  eta, Q    every term is non-negative, so elite_reduce's bound is relative: a term passes through at most m + 7 rounded additions,
            (1 + u)^(m + 7) - 1 <= (m + 8) u. For Q one more rounding, of the square:
                |eta_dev - eta| <= (m + 8) u eta,   |Q_dev - Q| <= (m + 9) u Q                                   (eta_bound, q_bound)
            about the exact sums of the DEVICE's weights. (A square below 2^-1022 rounds absolutely, by at most 2^-1075 each: n 2^-1075
            against Q >= 1 -- the winner weighs 1 -- is nothing.)
  S[j]      the product w p rounds once, then the m + 7 additions; signs are mixed, so the bound is absolute on A_j = sum |w p|:
                |S_dev - S| <= (m + 9) u A_j                                                                      (s_bound)
  mean      mean_dev = fl(S_dev / eta_dev). S_dev / eta_dev - S / eta = (S_dev - S) / eta_dev + S (1 / eta_dev - 1 / eta): at most
            (m + 9) u A_j / eta + (m + 8) u |S| / eta, and the division adds u |S| / eta:
                |mean_dev - S / eta| <= (m + 9) u (A_j + |S_j|) / eta (1 + 2^-30)                                 (mean_bound)
            (the last factor: the second-order terms, each below (m + 9)^2 u^2).
  effective_samples  fl(fl(eta_dev^2) / Q_dev): twice eta's relative error and one rounding for the square, Q's, one for the division:
                |ess_dev - eta^2 / Q| <= (3 m + 27) u (eta^2 / Q) (1 + 2^-30)                                     (ess_bound)

Nothing here was tuned to the kernel's output. emulate_mppi() repeats the device's operations in numpy (numpy's exp in the place of the
device's); tests/test_mppi_cases.py shows it inside every bound on every data set the GPU test uses (worst shares there: weights 0.50
-- a subnormal's rounding against its floor --, eta 0.21, effective samples 0.17, mean 0.17; the MI355X gives the same figures, see
test_gpu_mppi_update.py), and a variant that does not subtract beta (exp(-R / lam)) far outside them on returns near 1e3 at lam = 0.1:
every weight underflows, eta = 0 where the contract says >= 1."""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

from sampling_policy_cases import ULP_FN
from selection_cases import (FAILED, LOW, NEG_NAN, SEG_E, SEG_N, SEG_PLACES, SEG_STRADDLES, STRIDE, U, Case, _scaled, all_nan,  # noqa: F401
                             as_device, base, bits, emulate_elite_reduce, inject, order, ratio, same_bits, scaled_nodes, segmented_cases,
                             signed_zeros, trips, with_failed, with_inf, with_min, with_nan, with_tie)

TINY = Fraction(1, 2 ** 1074)      # one subnormal spacing
SECOND = 1 + Fraction(1, 2 ** 30)  # room for the second-order terms
N_LARGE = 16384                    # the largest candidate count the planners document
# the temperatures dealt over the cases: moderate ones, one so small that every loser's weight is exactly 0 (x overflows), one so large
# that every weight is 1 - O(1e-298)
LAMBDAS = (0.5, 40.0, 1e4, 1e-300, 1e300, 3.0)


# ------------------------------------------------------------------------------------------------ the contract
def contract(ret, ref=-1):
    """(index, best_return, ref_return, valid) of one environment"""
    ret = np.asarray(ret, dtype=np.float64)
    w = int(order(ret)[0])
    beta = ret[w]
    valid = int(beta == beta and beta < np.inf)
    return w, beta, (ret[ref] if ref >= 0 else np.float64(np.nan)), valid


def contract_weights(ret, lam, shift=True):
    """the weights in the contract's fp64 arithmetic (numpy's exp). shift=False: the formula the kernel must NOT use, exp(-R / lam)"""
    ret = np.asarray(ret, dtype=np.float64)
    _, beta, _, valid = contract(ret)
    w = np.zeros(ret.size)
    if not valid:
        return w
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i, r in enumerate(ret):
            if r != r:
                continue
            if shift:
                w[i] = 1.0 if r == beta else np.exp(-((r - beta) / np.float64(lam)))
            else:
                w[i] = np.exp(-(r / np.float64(lam)))
    return w


def exact_weights(ret, lam):
    """per candidate (w, |x|) with w the contract's weight at 200 bits from the exact x = (R - beta) / lam; exact 0 / 1 where the
    contract says so (NaN, invalid, R == beta, an infinite x)"""
    ret = np.asarray(ret, dtype=np.float64)
    _, beta, _, valid = contract(ret)
    out = []
    with mpmath.workprec(200):
        for r in ret:
            if not valid or r != r:
                out.append((mpmath.mpf(0), 0.0))
            elif r == beta:
                out.append((mpmath.mpf(1), 0.0))
            elif np.isinf(r) or np.isinf(beta):      # (+inf - finite, finite - -inf)
                out.append((mpmath.mpf(0), math.inf))
            else:
                x = (mpmath.mpf(float(r)) - mpmath.mpf(float(beta))) / mpmath.mpf(float(lam))
                out.append((mpmath.exp(-x), float(x)))
    return out


def weight_ratio(got, exact, x):
    """|got - w| / weight_bound, in mpmath (the weights span 1e-320 .. 1)"""
    with mpmath.workprec(200):
        d = abs(mpmath.mpf(float(got)) - exact)
        if d == 0:
            return 0.0
        if math.isinf(x):
            return math.inf                          # the contract's exact 0
        bound = (2 * abs(x) + 2 * ULP_FN + 1) * mpmath.mpf(2) ** -53 * exact + mpmath.mpf(2) ** -1074
        return float(d / bound)


def check_weights(got, ret, lam):
    """the worst |error| / weight_bound over one environment's weights; exact where the contract is"""
    worst = 0.0
    for g, (w, x) in zip(np.asarray(got, dtype=np.float64), exact_weights(ret, lam)):
        assert g == g and 0.0 <= g <= 1.0, g
        worst = max(worst, weight_ratio(g, w, x))
    return worst


# ------------------------------------------------------------------------------------------------ exact sums, bounds
def exact_sums(weights, nodes):
    """eta, Q, and per parameter S[j] and A[j] = sum |w p| as Fractions, from the weights given (the device's) and the nodes as the
    device holds them ([n][np], fp64 values)"""
    w, ws = _scaled(np.asarray(weights, dtype=np.float64))
    out = dict(eta=Fraction(sum(w), 1 << ws), Q=Fraction(sum(x * x for x in w), 1 << (2 * ws)), S=[], A=[])
    nodes = np.asarray(nodes, dtype=np.float64)
    live = [i for i, x in enumerate(w) if x]
    for j in range(nodes.shape[1]):
        p, ps = _scaled(nodes[live, j]) if live else ([], 0)
        out["S"].append(Fraction(sum(w[i] * q for i, q in zip(live, p)), 1 << (ws + ps)))
        out["A"].append(Fraction(sum(w[i] * abs(q) for i, q in zip(live, p)), 1 << (ws + ps)))
    return out


def eta_bound(n, eta):
    return (trips(n) + 8) * U * eta


def q_bound(n, q):
    return (trips(n) + 9) * U * q


def s_bound(n, a):
    return (trips(n) + 9) * U * a


def mean_bound(n, a, s, eta):
    return (trips(n) + 9) * U * (a + abs(s)) / eta * SECOND


def ess_bound(n, ess):
    return (3 * trips(n) + 27) * U * ess * SECOND


def check_outputs(out, ret, nodes, ref, worst):
    """weight_sum, effective_samples and mean of one environment (out: dict with those and `weights`) against the exact sums of the
    weights in `out`; nodes [n][np] as the device holds them. Updates `worst` (share of each bound) and asserts every bound."""
    n = len(ret)
    _, _, _, valid = contract(ret)
    mean = np.asarray(out["mean"], dtype=np.float64).reshape(-1)
    if not valid:
        assert out["weight_sum"] == 0.0 and out["effective_samples"] == 0.0 and not np.any(out["weights"])
        assert same_bits(mean, nodes[ref]) if ref >= 0 else np.isnan(mean).all()
        return
    ex = exact_sums(out["weights"], nodes)
    assert ex["eta"] >= 1 and out["weight_sum"] >= 1.0
    checks = [("eta", out["weight_sum"], ex["eta"], eta_bound(n, ex["eta"])),
              ("ess", out["effective_samples"], ex["eta"] ** 2 / ex["Q"], ess_bound(n, ex["eta"] ** 2 / ex["Q"]))]
    checks += [("mean", mean[j], ex["S"][j] / ex["eta"], mean_bound(n, ex["A"][j], ex["S"][j], ex["eta"])) for j in range(mean.size)]
    for name, got, exact, bound in checks:
        q = ratio(got, exact, bound)
        worst[name] = max(worst.get(name, 0.0), q)
        assert q <= 1.0, (name, float(got), float(exact), q)
    assert 1.0 <= out["effective_samples"] * (1 + 1e-12) and out["effective_samples"] <= n * (1 + 1e-12)
    lo, hi = nodes.min(axis=0), nodes.max(axis=0)
    assert np.all(lo <= mean) and np.all(mean <= hi), "mean outside the convex hull of the nodes"


# ------------------------------------------------------------------------------------------------ the device's order of operations
def emulate_mppi(ret, lam, nodes, ref=-1, shift=True):
    """mppi_weights_kernel + mppi_mean_kernel for one environment in numpy: the same fp64 operations in the same order (numpy's exp for
    the device's). nodes [n][np] as the device holds them. shift=False: the wrong kernel (no subtraction of beta)."""
    ret = np.asarray(ret, dtype=np.float64)
    nodes = np.asarray(nodes, dtype=np.float64)
    index, beta, ref_return, valid = contract(ret, ref)
    w = contract_weights(ret, lam, shift)
    out = dict(index=index, best_return=beta, ref_return=ref_return, valid=valid, weights=w)
    if not valid:
        out.update(weight_sum=0.0, effective_samples=0.0, mean=nodes[ref].copy() if ref >= 0 else np.full(nodes.shape[1], np.nan))
        return out
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        eta = np.float64(emulate_elite_reduce(w))
        q = np.float64(emulate_elite_reduce(w * w))
        s = np.array([emulate_elite_reduce(w * nodes[:, j]) for j in range(nodes.shape[1])])
        out.update(weight_sum=float(eta), effective_samples=float((eta * eta) / q), mean=s / eta)
    return out


# ------------------------------------------------------------------------------------------------ data sets
def spread(n, seed, top):
    """returns LOW .. LOW + top in n even steps, shuffled: at lam = 1 the weights run from 1 through the subnormals (x in 708 .. 745)
    to exact 0 when top is well past 745"""
    return LOW + np.random.default_rng(seed).permutation(n) * (top / (n - 1))


def mppi_cases(n):
    """[(name, returns, temperature)]: every segmented selection case (the unique minimum and tied minima at and across lanes 15/16,
    63/64, 255/256; NaN of both payloads, +inf, -inf as the minimum, signed zeros, failed rollouts' 1e6, all NaN, all equal) with the
    LAMBDAS in turn, and MPPI's own: all +inf, a spread through the subnormals to 0, near-ties at the minimum"""
    cases = [(c.name, c.ret, LAMBDAS[k % len(LAMBDAS)]) for k, c in enumerate(segmented_cases(n))]
    cases.append(("all+inf", np.full(n, np.inf), 1.0))
    cases.append(("spread-800", spread(n, 300 + n, 800.0), 1.0))
    cases.append(("spread-760@.37", spread(n, 301 + n, 760.0 * 0.37), 0.37))
    near = base(n, 302 + n)
    near[[n // 3, n - 1]] = [np.nextafter(2.0, 3.0), 2.0]     # the minimum and its neighbour one ulp above, anywhere
    cases.append(("near-tie", near, 1e-3))
    big = 1e3 + base(n, 303 + n)                              # returns near 1e3 at lam = 0.1: what an unshifted exp cannot do
    cases.append(("offset-1e3", big, 0.1))
    return cases


def mppi_rounds(n, num_envs=SEG_E):
    """the cases dealt once over num_envs environments, a different one (with its own temperature) in each (a wrong `first` offset
    shows): round k puts case k * num_envs + e in environment e; the last round wraps around"""
    cases = mppi_cases(n)
    return [[cases[(r + e) % len(cases)] for e in range(num_envs)] for r in range(0, len(cases), num_envs)]


def large_case():
    """one environment of N_LARGE candidates: ties across the stride, NaN, failures, a spread that reaches 0"""
    n = N_LARGE
    r = spread(n, 77, 900.0)
    r[::7] = FAILED
    r[[0, 64, n - 1]] = [np.nan, NEG_NAN, np.nan]
    r[[255, 256]] = LOW - 0.5
    return ("large", r, 1.0)
