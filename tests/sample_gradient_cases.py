"""Sample-Gradient harness (test infrastructure, like selection_cases.py; no GPU code of its own): the bounds the device's gradient
estimate, its gradient-step candidates and its spline re-sampling are held to, each derived from the operation count, and the spline
sample in exact rational arithmetic.

u = 2^-53. sg_update_kernel (mjpcx.hip) forms, per sorted position i of the m = num_noisy it reads, the term t_i = z_i q_i with
q_i = w_i / m (one rounded product; w_i and q_i are the same bits as planners.sample_gradient_update computes, which divides the same
numbers: the logarithms come from one host table) and adds the terms as elite_reduce does -- 256 strided partial sums from zero, then a
halving tree of 8 levels: a term passes through at most ceil(m / 256) - 1 + 8 rounded additions (selection_cases.sum_bound). With the
product that is ceil(m / 256) + 8 roundings, (1 + u)^k - 1 <= (k + 1) u. The test feeds sample_gradient_update the ORACLE's normals;
the device draws its own from the same counter: u1, u2 are equal bits, log, sqrt, sincos are the device's against libm's. With
r = sqrt(-2 log u1) <= sqrt(2 * 54 log 2) < 8.7 and theta = 2 pi u2 < 6.3: cos(theta) carries at most theta u from the rounded argument
and 2 u from the function on either side, r at most 4 u relatively (log, the product, sqrt; the logarithm's own error is relative to a
value >= u, so divided by 2 under the root), so |dz| <= 8.7 (6.3 + 2 + 4) u < 110 u per side, 220 u = 2.5e-14 between the two. The
repository holds a device normal to the oracle's at 1e-13 * sigma (tests/test_gpu_parity.py, tests/test_gpu_limb.py: candidates at
sigma <= 0.5 to atol 1e-13), which this derivation sits inside; NORMAL_TOL is that figure, absolute (a normal near zero has no
relative accuracy: it is r times a cosine near its root). Hence, for parameter j,
    |g_dev - g_ref| <= (2 ceil(m / 256) + 20) u sum_i |t_ij| + NORMAL_TOL sum_i |q_i|                       (gradient_bound)
(the first term twice: the two sides round different terms; + 2 for the second order), the sums over the positions that carry noise.
A gradient-step candidate is nominal + a g + b g' in two rounded additions, a = -s filter, b = -s (1 - filter), s = step / noise
exploration (four roundings in a, five in b), then the clamp, which is 1-Lipschitz:
    |c_dev - c_ref| <= |a| B + |b| B' + 8 u (|nominal| + |a g| + |b g'|)                                    (candidate_bound)
with B, B' the gradient bounds of this step and the one before, and on a 32-bit context the rounding of the stored node, 2^-24 |c|.

Re-sampling (sg_spline_sample, TimeSpline::Sample): t = (time - tl) / (tu - tl), three roundings; zero: exact. Linear, vl (1 - t) +
vu t: 1 - t one more, two products, one addition: every term at most 6 roundings -> 8 u (|vl| (1 + |t|) + |vu| |t|), |1 - t| <= 1 + |t|.
Cubic: a monomial t^3 or t^2 with its coefficient is at most 3 products of a t of 3 roundings each: 12; two additions in the
polynomial: 14; the span factor of c1, c3: 15; a slope is two terms of (0.5 dv) / dt, subtraction, product, subtraction, division: 4,
and their sum: 5; the product with the value or slope and three additions of the final sum: 4. At most 15 + 5 + 4 = 24 roundings on
any path: 26 u M with M the sum of the absolute values of every monomial times |value| or times the absolute slope terms.
resample_exact returns the exact value and that M."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from mujoco_mpc_amd.planners import log_scale

U = 2.0 ** -53
NORMAL_TOL = 1.0e-13
STRIDE = 256


def gradient_terms(order_used, weights, noise, num_noisy):
    """per parameter: sum_i |z_ij q_i| and sum_i |q_i| over the sorted positions whose candidate carries noise"""
    used = np.asarray(order_used)
    q = np.abs(np.asarray(weights) / num_noisy)
    live = (used > 0) & (used < num_noisy)
    z = np.abs(np.asarray(noise)[used[live]])
    return (z * q[live][:, None]).sum(axis=0) * (1 + 4 * U), float(q[live].sum()) * (1 + 4 * U)


def gradient_bound(order_used, weights, noise, num_noisy):
    abs_terms, abs_q = gradient_terms(order_used, weights, noise, num_noisy)
    return (2 * math.ceil(num_noisy / STRIDE) + 20) * U * abs_terms + NORMAL_TOL * abs_q


def candidate_bound(g, nominal, gradient, gradient_previous, bound, bound_previous, num_gradient, gradient_filter, max_step, min_step, noise_exploration,
                    precision=64):
    s = log_scale(max_step, min_step, num_gradient)[g] / noise_exploration
    a, b = abs(s * gradient_filter), abs(s * (1.0 - gradient_filter))
    value = np.abs(nominal) + a * np.abs(gradient) + b * np.abs(gradient_previous)
    tol = a * bound + b * bound_previous + 8 * U * value
    return tol + (2.0 ** -24 * (value + tol) if precision == 32 else 0.0)


def resample_exact(times, values, interp, time):
    """TimeSpline::Sample of one scalar spline in exact rational arithmetic -> (value, M): M the magnitude the rounding bound scales with"""
    return resample_rational([Fraction(float(t)) for t in times], [Fraction(float(v)) for v in values], interp, Fraction(float(time)))


def resample_weights(times, interp, time):
    """The sample as a linear form of the node values: {node p: (W_p, A_p)} with value = sum_p W_p v_p and M = sum_p A_p |v_p|, from
    resample_rational on the unit splines (the sample is linear in the values, M in their absolute values); nodes with W_p = A_p = 0 are
    left out. tests/sampling_policy_cases.py evaluates many candidates on one grid with it."""
    ts, x = [Fraction(float(t)) for t in times], Fraction(float(time))
    out = {}
    for p in range(len(ts)):
        w, a = resample_rational(ts, [Fraction(int(q == p)) for q in range(len(ts))], interp, x)
        if w != 0 or a != 0:
            out[p] = (w, a)
    return out


def resample_rational(ts, vs, interp, x):
    """resample_exact on Fractions"""
    P = len(ts)
    up = 0
    while up < P and not x < ts[up]:
        up += 1
    if up == P:
        return vs[-1], Fraction(0)
    if up == 0:
        return vs[0], Fraction(0)
    lo = up - 1
    span = ts[up] - ts[lo]
    t = (x - ts[lo]) / span
    if interp == 0:
        return vs[lo], Fraction(0)
    if interp == 1:
        return vs[lo] * (1 - t) + vs[up] * t, abs(vs[lo]) * (1 + abs(t)) + abs(vs[up]) * abs(t)

    def slope(node):
        if node == 0:
            terms = [(vs[1] - vs[0]) / (ts[1] - ts[0])]
        elif node == P - 1:
            terms = [(vs[node] - vs[node - 1]) / (ts[node] - ts[node - 1])]
        else:
            terms = [(vs[node + 1] - vs[node]) / (ts[node + 1] - ts[node]) / 2, (vs[node] - vs[node - 1]) / (ts[node] - ts[node - 1]) / 2]
        return sum(terms), sum(abs(q) for q in terms)
    c0, m0 = 2 * t ** 3 - 3 * t ** 2 + 1, 2 * abs(t) ** 3 + 3 * t ** 2 + 1
    c1, m1 = (t ** 3 - 2 * t ** 2 + t) * span, (abs(t) ** 3 + 2 * t ** 2 + abs(t)) * span
    c2, m2 = -2 * t ** 3 + 3 * t ** 2, 2 * abs(t) ** 3 + 3 * t ** 2
    c3, m3 = (t ** 3 - t ** 2) * span, (abs(t) ** 3 + t ** 2) * span
    (sl, al), (su, au) = slope(lo), slope(up)
    return c0 * vs[lo] + c1 * sl + c2 * vs[up] + c3 * su, m0 * abs(vs[lo]) + m1 * al + m2 * abs(vs[up]) + m3 * au


RESAMPLE_ROUNDINGS = {0: 0, 1: 8, 2: 26}
