"""CMA-ES harness (test infrastructure, like mppi_cases.py; not a conftest, no GPU code of its own): the contract of
mjpcx_rollout_cma_batched and mjpcx_cma_update_batched (include/mjpcx.h; csrc/cma_update.h) restated in exact arithmetic, and the error
bounds the device and the numpy mirror (planners.cma_update) are held to. Written from the header, not from the kernels.

EXACT ARITHMETIC. Every double is an integer over 2^Q (Q = 200; asserted exact), products add their shifts, nothing is rounded. The
standard normals are sampling_policy_cases.normal_pair's: Philox4x32-10 in Python integers, Box-Muller in mpmath at 50 digits (their
2^-166 is nothing against u = 2^-53; kept to 2^-200), with that harness's bound on a double-precision evaluation (ULP_FN-ulp log, sqrt, sincos; its
HEADROOM of 4 included: the project's standing assumption about the device's normals).

WHAT IS COMPARED WITH WHAT. Quantities the device reports are checked against exact functions OF WHAT IT REPORTED UPSTREAM (the way of
mppi_cases.check_outputs), so one stage's error does not eat the next stage's bound:
    nodes, mean, p_sigma', z_w, y_w    from the inputs (state before, nominal, the exact normals)
    norm, h_sigma, sigma'               from the p_sigma' the device reported
    p_c'                                from the inputs and the h_sigma above
    C'                                  from C, the p_c' the device reported and the exact S of the inputs
    A'                                  A' A'^T against the C' the device reported
The h_sigma test is a discrete decision: the cases keep |lhs / rhs - 1| > 1e-9 (asserted), so it is the same on both sides.

BOUNDS, derived, not measured. u = 2^-53, G(k) = k u (1 + 2^-30) (gamma_k with room for the second-order terms), m = ceil(mu / 256),
dz the normals' bound. |.| of a sum means the sum of the absolute values of its terms.
    y[a]      a dot product of a + 1 terms: dY = sum_b |A_ab| dz_b + G(a + 2) sum_b |A_ab| (|z_b| + dz_b)
    node      step = fl(sigma fl(0.5 fl(hi - lo))) is within G(2) of sigma s; the product and the sum round once each:
              dv = step dy + G(4) step (|y| + dy) + G(1) (|m| + step (|y| + dy)); the clamp is 1-Lipschitz; a 32-bit context rounds the
              stored node once more: + 2^-24 |v|. (`step` below is the exact product, so its two roundings are in G(4).)
    z_w[j]    the product, m strided additions, 8 tree levels: dzw = sum_i w_i dz_ij + G(m + 9) sum_i w_i (|z_ij| + dz_ij)
    y_w, mean as y and node, from z_w and dzw
    p_sigma'  two products and a sum: dps = root dzw + G(2) (|(1 - c_sigma) p_sigma| + root (|z_w| + dzw))
    norm      d squares and d additions of non-negative terms, then the root: relative G(d / 2 + 1 + ULP_FN) (the root halves the sum's
              G(d + 1); the function adds ULP_FN ulp = 2 ULP_FN u; G rounds up)
    sigma'    ratio = norm / chi, x = (c_sigma / d_sigma) (ratio - 1): dx = |c| (ratio rel + G(1)) ratio + G(3) |x|; exp turns dx into the
              relative |dx| e^|dx| and adds 2 ULP_FN u; the product one more: dsigma = sigma' (|dx| (1 + 2^-20) + G(2 ULP_FN + 2)); the
              clamp is 1-Lipschitz
    p_c'      as p_sigma' with y_w, dyw and the root of c_c
    S[a][b]   dS = sum_i w_i (|y_a| dy_b + |y_b| dy_a + dy_a dy_b) + G(m + 10) sum_i w_i (|y_a| + dy_a) (|y_b| + dy_b)
    C'[a][b]  three products (one of two factors) and two sums: dC = c_mu dS + G(4) (|decay C| + c_one |p_c p_c| + c_mu (|S| + dS))
    A'        Cholesky's backward error (Higham, Accuracy and Stability, thm 10.3) |C' - A' A'^T| <= gamma_{d+1} |A'| |A'|^T, plus
              the root's ULP_FN ulp on the diagonal, squared: G(d + 1 + 4 ULP_FN) (|A'| |A'|^T)[a][b]
Nothing here was tuned to a kernel's output. tests/test_cma_cases.py holds the numpy mirror to every bound on every data set the GPU
test uses."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import sampling_policy_cases as spc
from mujoco_mpc_amd.planners import cma_parameters
from sampling_policy_cases import HEADROOM, ULP_FN, M, normal_pair, uniform_k
from selection_cases import FAILED, NEG_NAN, U, order, same_bits  # noqa: F401

Q = 200
ONE = 1 << Q
SECOND = 1 + Fraction(1, 2 ** 30)
U32 = Fraction(1, 2 ** 24)
STATE_KEYS = ("sigma", "generation", "C", "A", "p_sigma", "p_c")


def G(k):
    return k * U * SECOND


# ------------------------------------------------------------------------------------------------ fixed point
def _fx1(x):
    n, d = float(x).as_integer_ratio()
    v = n << Q
    assert v % d == 0, f"{x!r} is not a multiple of 2^-{Q}"
    return v // d


def fx(a):
    """doubles -> integers over 2^Q, exactly (object array of the same shape)"""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for i, x in enumerate(a.reshape(-1)):
        flat[i] = _fx1(x)
    return out


def frac(v, shifts=1):
    return Fraction(int(v), 1 << (Q * shifts))


def _abs(a):
    return np.frompyfunc(abs, 1, 1)(a)


_Z = {}


def normals(seed, cand, d, iteration):
    """(z, dz) of one candidate over 2^Q: the exact normals of counter (cand, j >> 1, iteration, 0) under key seed and the bound of a
    double-precision evaluation (rounded up)"""
    key = (seed, cand, d, iteration)
    if key not in _Z:
        z, dz = [], []
        for q in range((d + 1) // 2):
            (z0, z1), (b0, b1) = normal_pair(*uniform_k(seed, cand, q, iteration, 0))
            z += [int(M.floor(z0 * ONE + 0.5)), int(M.floor(z1 * ONE + 0.5))]
            dz += [int(M.ceil(HEADROOM * b0 * ONE)), int(M.ceil(HEADROOM * b1 * ONE))]
        _Z[key] = (np.array(z[:d], dtype=object), np.array(dz[:d], dtype=object))
    return _Z[key]


def normals_f64(seed, cand, d, iteration):
    """the same normals as a double-precision Box-Muller gives them, in the device's order of operations (numpy's functions)"""
    z = []
    for q in range((d + 1) // 2):
        k1, k2 = uniform_k(seed, cand, q, iteration, 0)
        u1, u2 = (np.float64(k1) + 0.5) * (1.0 / 9007199254740992.0), (np.float64(k2) + 0.5) * (1.0 / 9007199254740992.0)
        r, th = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586476925286766559 * u2
        z += [r * np.cos(th), r * np.sin(th)]
    return np.array(z[:d])


def normal_rows(seed, cands, d, iteration, f64=False):
    if f64:
        return np.stack([normals_f64(seed, int(c), d, iteration) for c in cands])
    zs = [normals(seed, int(c), d, iteration) for c in cands]
    return np.stack([z for z, _ in zs]), np.stack([dz for _, dz in zs])


# ------------------------------------------------------------------------------------------------ the contract's stages, exactly
def lower_times(A, absA, z, dz):
    """(y, dy) over 2^2Q of y[., a] = sum_{b <= a} A[a][b] z[., b] (A lower triangular: the entries above the diagonal are zero), with
    dy = sum |A| dz + G(a + 2) sum |A| (|z| + dz)"""
    d = A.shape[0]
    y = z @ A.T
    mag = (_abs(z) + dz) @ absA.T
    g = np.array([G(a + 2) for a in range(d)], dtype=object)
    dy = dz @ absA.T + np.frompyfunc(lambda v, k: -((-v * k.numerator) // k.denominator), 2, 1)(mag, g)
    return y, dy


def half_range(ctrlrange, d):
    b = np.asarray(ctrlrange, dtype=np.float64).reshape(-1, 2)
    lo, hi = np.resize(b[:, 0], d), np.resize(b[:, 1], d)
    return lo, hi, [(Fraction(float(h)) - Fraction(float(l))) / 2 for l, h in zip(lo, hi)]


def moved(m, sigma, half, y, dy, lo, hi, shifts, precision=64):
    """per parameter (clamp(m + sigma s y), bound) as Fractions; y, dy over 2^(shifts Q)"""
    out = []
    for j in range(len(m)):
        step = Fraction(float(sigma)) * half[j]
        yj, dj = frac(y[j], shifts), frac(dy[j], shifts)
        reach = step * (abs(yj) + dj)
        v = Fraction(float(m[j])) + step * yj
        b = step * dj + G(4) * reach + G(1) * (abs(Fraction(float(m[j]))) + reach)
        c = min(max(v, Fraction(float(lo[j]))), Fraction(float(hi[j])))
        if precision == 32:
            b += U32 * abs(c)
        out.append((c, b))
    return out


def ratio(got, exact, bound):
    d = abs(Fraction(float(got)) - exact)
    if d == 0:
        return 0.0
    return float(d / bound) if bound else math.inf


class Worst(dict):
    def take(self, name, got, exact, bound, where=()):
        q = ratio(got, exact, bound)
        self[name] = max(self.get(name, 0.0), q)
        assert q <= 1.0, (name, where, float(got), float(exact), float(bound), q)


def check_candidates(nodes, nominal, state, ctrlrange, seed, iteration, precision, worst, cands=None):
    """nodes [n][d] as the device holds them (fp64 values) against clamp(m + sigma s A z) of candidates `cands` (all but 0 by
    default); candidate 0 must be the mean as the context's type holds it, bit for bit"""
    nodes = np.asarray(nodes, dtype=np.float64)
    n, d = nodes.shape
    m = np.asarray(nominal, dtype=np.float64).reshape(-1)
    held = m.astype(np.float32).astype(np.float64) if precision == 32 else m
    assert same_bits(nodes[0], held), "candidate 0 is not the mean"
    lo, hi, half = half_range(ctrlrange, d)
    held_lo, held_hi = (lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)) if precision == 32 else (lo, hi)
    A = fx(np.tril(state["A"]))
    absA = _abs(A)
    cands = range(1, n) if cands is None else cands
    z, dz = normal_rows(seed, cands, d, iteration)
    y, dy = lower_times(A, absA, z, dz)
    for r, c in enumerate(cands):
        for j, (v, b) in enumerate(moved(m, state["sigma"], half, y[r], dy[r], lo, hi, 2, precision)):
            worst.take("node", nodes[c, j], v, b, (c, j))
            assert held_lo[j] <= nodes[c, j] <= held_hi[j]


def constants(params, d, generation):
    """the doubles the host derives from the parameters, in the header's order of operations"""
    cs, cc, c1, cmu, mueff = (np.float64(params[k]) for k in ("c_sigma", "c_c", "c_one", "c_mu", "mu_eff"))
    decay1 = (1.0 - c1) - cmu
    return dict(one_m_cs=1.0 - cs, cs_root=np.sqrt((cs * (2.0 - cs)) * mueff), one_m_cc=1.0 - cc, cc_root=np.sqrt((cc * (2.0 - cc)) * mueff),
                decay=(decay1 + (c1 * cc) * (2.0 - cc), decay1), cs_ds=cs / np.float64(params["d_sigma"]),
                hs_den=math.sqrt(1.0 - math.pow(1.0 - float(cs), 2.0 * (generation + 1))), hs_rhs=(1.4 + 2.0 / (d + 1.0)) * np.float64(params["chi"]))


def contract_order(ret, mu):
    """(the mu best of candidates 1..n-1, valid, the argmin over all n)"""
    ret = np.asarray(ret, dtype=np.float64)
    ranked = order(ret, skip=0)[:mu]
    return ranked, int(not np.isnan(ret[ranked]).any()), int(order(ret)[0])


def check_update(got, after, ret, nominal, before, params, ctrlrange, seed, iteration, worst, where=()):
    """One environment's outputs `got` (index, best_return, nominal_return, improvement, valid, restarted, sigma, mean, order) and
    its state `after` the update against the contract, from the state `before` (dicts of STATE_KEYS). Asserts every bound, updates
    `worst` (the share of each bound)."""
    ret = np.asarray(ret, dtype=np.float64)
    m = np.asarray(nominal, dtype=np.float64).reshape(-1)
    d, mu = m.size, int(params["mu"])
    ranked, valid, index = contract_order(ret, mu)
    assert got["index"] == index and got["valid"] == valid, where
    assert same_bits(got["best_return"], ret[index]) and same_bits(got["nominal_return"], ret[0]), where
    gain = ret[0] - ret[index]
    assert same_bits(got["improvement"], gain if gain > 0 else 0.0), where
    if got.get("order") is not None:
        assert np.array_equal(got["order"], ranked), where
    mean = np.asarray(got["mean"], dtype=np.float64).reshape(-1)
    if not valid:
        assert got["restarted"] == 0 and same_bits(mean, m) and same_bits(got["sigma"], before["sigma"]), where
        assert all(same_bits(np.asarray(after[k], np.float64), np.asarray(before[k], np.float64)) for k in STATE_KEYS), where
        return
    assert after["generation"] == before["generation"] + 1, where
    k = constants(params, d, int(before["generation"]))
    mtrips = max(1, -(-mu // 256))
    lo, hi, half = half_range(ctrlrange, d)
    w = fx(params["weights"])
    A = fx(np.tril(before["A"]))
    absA = _abs(A)
    z, dz = normal_rows(seed, ranked, d, iteration)
    y, dy = lower_times(A, absA, z, dz)                                  # over 2^2Q
    zw = w @ z                                                            # over 2^2Q
    gz = G(mtrips + 9)
    up = lambda v, g: -((-v * g.numerator) // g.denominator)
    dzw = w @ dz + np.frompyfunc(lambda v: up(v, gz), 1, 1)(w @ (_abs(z) + dz))
    yw, dyw = lower_times(A, absA, zw, dzw)                               # over 2^3Q
    for j, (v, b) in enumerate(moved(m, before["sigma"], half, yw, dyw, lo, hi, 3)):
        worst.take("mean", mean[j], v, b, where + (j,))
    # ---- the sigma path, from the inputs; norm, h_sigma and sigma' from the path as reported
    restarted = int(got["restarted"])
    omc, root = Fraction(float(k["one_m_cs"])), Fraction(float(k["cs_root"]))
    ps_exact = [omc * Fraction(float(p)) + root * frac(zw[j], 2) for j, p in enumerate(before["p_sigma"])]
    ps_bound = [root * frac(dzw[j], 2) + G(2) * (abs(omc * Fraction(float(p))) + root * (abs(frac(zw[j], 2)) + frac(dzw[j], 2)))
                for j, p in enumerate(before["p_sigma"])]
    if restarted:
        assert np.array_equal(after["C"], np.eye(d)) and np.array_equal(after["A"], np.eye(d)), where
        assert not np.any(after["p_sigma"]) and not np.any(after["p_c"]), where
        ps_dev = None
    else:
        ps_dev = np.asarray(after["p_sigma"], dtype=np.float64)
        for j in range(d):
            worst.take("p_sigma", ps_dev[j], ps_exact[j], ps_bound[j], where + (j,))
    # (after a restart the path is gone: norm and h_sigma from the exact path, with its bound as the margin)
    ps_for = [Fraction(float(v)) for v in ps_dev] if ps_dev is not None else ps_exact
    n2 = sum(v * v for v in ps_for)
    norm = M.sqrt(M.mpf(n2.numerator) / M.mpf(n2.denominator))
    norm_f = Fraction(int(M.floor(norm * ONE + 0.5)), ONE)
    norm_rel = G(Fraction(d, 2) + 1 + ULP_FN)
    if ps_dev is None:
        slack = sum(2 * abs(v) * b + b * b for v, b in zip(ps_exact, ps_bound))
        norm_rel += (slack / n2) if n2 else 0
    lhs, rhs = norm_f / Fraction(float(k["hs_den"])), Fraction(float(k["hs_rhs"]))
    assert abs(lhs / rhs - 1) > max(Fraction(1, 10 ** 9), 2 * norm_rel), ("h_sigma is borderline in this case", where)
    h = lhs < rhs
    chi, c = Fraction(float(params["chi"])), Fraction(float(k["cs_ds"]))
    rat = norm_f / chi
    x = c * (rat - 1)
    dx = abs(c) * (norm_rel + G(1)) * rat + G(3) * abs(x)
    grown = Fraction(float(before["sigma"])) * Fraction(int(M.floor(M.exp(M.mpf(x.numerator) / M.mpf(x.denominator)) * ONE + 0.5)), ONE)
    smin, smax = Fraction(float(params["sigma_min"])), Fraction(float(params["sigma_max"]))
    worst.take("sigma", got["sigma"], min(max(grown, smin), smax), grown * (dx * (1 + Fraction(1, 2 ** 20)) + G(2 * ULP_FN + 2)), where)
    assert same_bits(after["sigma"], got["sigma"]) and float(smin) <= got["sigma"] <= float(smax), where
    # ---- the covariance path, from the inputs
    omcc, hc = Fraction(float(k["one_m_cc"])), (Fraction(float(k["cc_root"])) if h else Fraction(0))
    pc_exact = [omcc * Fraction(float(p)) + hc * frac(yw[a], 3) for a, p in enumerate(before["p_c"])]
    pc_bound = [hc * frac(dyw[a], 3) + G(2) * (abs(omcc * Fraction(float(p))) + hc * (abs(frac(yw[a], 3)) + frac(dyw[a], 3)))
                for a, p in enumerate(before["p_c"])]
    # ---- S exactly, over 2^5Q, and C' from the reported p_c'
    wy = y * w[:, None]
    S = wy.T @ y
    ay, adz = _abs(y), dy
    cross = (ay * w[:, None]).T @ adz
    dS = cross + cross.T + (adz * w[:, None]).T @ adz
    magS = ((ay + adz) * w[:, None]).T @ (ay + adz)
    gs = G(mtrips + 10)
    decay, c1, cmu = Fraction(float(k["decay"][1 if h else 0])), Fraction(float(params["c_one"])), Fraction(float(params["c_mu"]))
    if restarted:
        # the restart itself is the claim: with the exact C' (from the exact p_c') the pivot test must fail beyond the bounds -- the cases
        # force it with pivot_floor >= 2, where the first pivot s = C'[0][0] can never exceed pivot_floor C'[0][0] > 0
        assert float(params["pivot_floor"]) >= 2.0, ("a restart without a forcing pivot_floor", where)
        c00 = decay * Fraction(float(before["C"][0][0])) + c1 * pc_exact[0] ** 2 + cmu * frac(S[0, 0], 5)
        assert c00 > 0, where
        return
    pc_dev = np.asarray(after["p_c"], dtype=np.float64)
    for a in range(d):
        worst.take("p_c", pc_dev[a], pc_exact[a], pc_bound[a], where + (a,))
    C_dev, A_dev = np.asarray(after["C"], dtype=np.float64), np.asarray(after["A"], dtype=np.float64)
    assert same_bits(C_dev, C_dev.T) and not np.any(np.triu(A_dev, 1)), where
    for a in range(d):
        for b in range(a + 1):
            s_ab = frac(S[a, b], 5)
            ds_ab = frac(dS[a, b], 5) + gs * frac(magS[a, b], 5)
            old, pp = decay * Fraction(float(before["C"][a][b])), c1 * Fraction(float(pc_dev[a])) * Fraction(float(pc_dev[b]))
            exact = old + pp + cmu * s_ab
            bound = cmu * ds_ab + G(4) * (abs(old) + abs(pp) + cmu * (abs(s_ab) + ds_ab))
            worst.take("C", C_dev[a, b], exact, bound, where + (a, b))
    check_factor(C_dev, A_dev, worst, where)


def check_factor(C, A, worst, where=()):
    """A A^T against C at Cholesky's backward-error bound; A lower triangular with a positive diagonal"""
    C, A = np.asarray(C, dtype=np.float64), np.asarray(A, dtype=np.float64)
    d = C.shape[0]
    assert not np.any(np.triu(A, 1)), where
    Af = fx(A)
    prod, mag = Af @ Af.T, _abs(Af) @ _abs(Af).T
    gf = G(d + 1 + 4 * ULP_FN)
    for a in range(d):
        assert A[a, a] > 0, where
        for b in range(a + 1):
            worst.take("factor", C[a, b], frac(prod[a, b], 2), gf * frac(mag[a, b], 2), where + (a, b))


# ------------------------------------------------------------------------------------------------ data sets
def spd_state(d, seed, sigma, generation=0):
    """a dense SPD covariance from a fixed seed (condition about 1e2, correlations of every sign), non-zero paths; A is left to the
    code under test"""
    rng = np.random.default_rng(seed)
    B = rng.normal(0, 1, (d, d)) / math.sqrt(d)
    C = B @ B.T + np.diag(0.05 + rng.uniform(0, 1, d))
    C = 0.5 * (C + C.T)
    return dict(sigma=float(sigma), C=C, p_sigma=rng.normal(0, 0.4, d), p_c=rng.normal(0, 0.3, d), generation=generation)


def params_for(d, n, **kw):
    return dict(cma_parameters(d, n - 1), sigma_min=1.0e-6, sigma_max=2.0, pivot_floor=kw.pop("pivot_floor", 1.0e-12), **kw)


def return_cases(n, mu, seed):
    """[(name, returns)] over n candidates with mu ranked: plain; ties across the mu boundary; +-0 and +-inf; the 1e6 of failed
    rollouts; NaN (both payloads) outside the mu best; NaN inside the mu best (not valid); candidate 0 the argmin"""
    rng = np.random.default_rng(seed)
    base = lambda: 2.0 + rng.permutation(n) * (3.0 / n)
    cases = [("plain", base())]
    r = base()
    ranked = order(r, skip=0)
    r[ranked[mu - 1]] = r[ranked[mu]] = r[ranked[min(mu + 1, n - 2)]]     # a tie across the boundary: the lower index is ranked
    cases.append(("tie-at-mu", r))
    r = base()
    r[[1, 2, 3, 4]] = [0.0, -0.0, -np.inf, np.inf]
    r[5::7] = FAILED
    cases.append(("zeros-inf-failed", r))
    r = base()
    worst_ones = order(r, skip=0)[mu:]
    r[worst_ones[::2]] = np.nan
    r[worst_ones[1]] = NEG_NAN
    r[0] = 1.0                                                            # the mean is the argmin and still not ranked
    cases.append(("nan-outside", r))
    r = base()
    r[order(r, skip=0)[mu - 1 - mu // 3:]] = np.nan                       # more NaN than n - 1 - mu (NaN sorts last): a rank below mu is one
    cases.append(("nan-inside", r))
    return cases


def emulate(ret, nominal, before, params, ctrlrange, seed, iteration):
    """planners.cma_update on double-precision normals: (got, after) in the shape check_update takes"""
    from mujoco_mpc_amd.planners import cma_factor, cma_update
    ret = np.asarray(ret, dtype=np.float64)
    d = np.asarray(nominal).size
    z = np.zeros((ret.size, d))
    ranked = order(ret, skip=0)[:int(params["mu"])]
    z[ranked] = normal_rows(seed, ranked, d, iteration, f64=True)
    state = dict(before, A=before["A"] if "A" in before else cma_factor(before["C"]))
    out = cma_update(ret, nominal, z, state, params, ctrlrange)
    return out, out["state"], state
