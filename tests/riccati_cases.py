"""Backward-pass harness (test infrastructure, like step_bank.py; not a conftest, no GPU code): problems whose Riccati sweep has an answer
that can be stated without a solver, and that answer in long double.

With B = 0 and A = I a sweep decouples: step t sees Quu = cuu[t] (+ regularisation), Qu = cu[t], Qxu = cxu[t], so du[t] is the solution of
the box-QP (cuu[t] + mu I, cu[t]) on [limits - actions[t]] and K[t] = -H_ff^-1 Qxu' on its free rows. One call with T steps is T - 1 box-QPs
solved in sequence (t = T-2 .. 0) with the warm start carried from one to the next. A strictly convex QP has exactly one KKT point, so a
point that passes the KKT check IS the answer, whoever proposed its active set: exact_boxqp takes the active set from a seed (the CPU
oracle's solution, never the kernel's), solves the free block in long double and verifies.

chain() builds those problems, exact_chain() their answers (du, K, Vx, Vxx, dV), coupled() the generic A, B problems of the shape sweeps."""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

LD = np.longdouble

# the chain set of tests/test_gpu_backward_pass.py (a), (b) and of tests/test_riccati_cases.py: every m on both sides of the <12> / <16>
# instantiations, state widths below, at and above one control, one horizon of 64 problems
CHAIN_M = (1, 2, 3, 11, 12, 13, 15, 16)
CHAIN_N = (1, 3, 17)
CHAIN_T = 65
CHAIN_MU = (0.0, 0.3)
# the coupled shape sweep (c): n on both sides of the 16-wide MFMA tiles, m on both sides of the instantiations, m > n included
COUPLED_N = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48)
COUPLED_M = (1, 12, 13, 16)
COUPLED_T = (2, 4)
COUPLED_REG = ((0, 1), (0, 0), (1, 1), (2, 1), (2, 0))      # (reg_type, use_limits)
COUPLED_MU = (0.0, 0.3)
# ill-conditioned Quu (d) and the pivot threshold (e)
KAPPAS = (1e4, 1e8, 1e11)
KAPPA_M = (12, 16)
KAPPA_T = 17
PIVOT_M = (1, 12, 16)
PIVOT_T = 9


def chain_seed(m, n):
    return 1000 * m + n


def chain_options(m, n):
    """the edge classes of one chain of the set: a zero-width range pins actuator 0 to its bound at every step but one, so the chains with
    n = 3 carry it and the others keep the all-free steps"""
    return dict(zero_width=(n == 3))


def coupled_seed(n, m):
    return n * 100 + m


def coupled_limit_scale(n, m):
    """the control range (and the nominal actions) of coupled() scaled so that the box binds at every shape of the sweep: at 1/2 every cell
    with m >= 12 has a mixed step (at 1 some wide-state cells are nearly free); one control needs 0.12 to clamp at n = 31, 32 and 48
    (tests/test_riccati_cases.py asserts both)"""
    return 0.5 if m >= 2 else 0.12


@dataclass
class Chain:
    n: int
    m: int
    T: int
    args: tuple                 # A, B, cx, cu, cxx, cxu, cuu, actions, limits: what mjpcx_backward_pass / pyoracle.riccati take
    zero_grad_step: int | None  # the step with g = 0 and actions on their limits
    zero_width: bool

    # the T - 1 box-QPs, step t at index t
    @property
    def H(self): return self.args[6][:self.T - 1]
    @property
    def g(self): return self.args[3][:self.T - 1]
    @property
    def Qxu(self): return self.args[5][:self.T - 1]
    @property
    def lo(self): return self.args[8][None, :, 0] - self.args[7][:self.T - 1]      # the subtraction the kernel and the oracle do, in fp64
    @property
    def hi(self): return self.args[8][None, :, 1] - self.args[7][:self.T - 1]


def _spd(rng, T, k, shift):
    M = rng.normal(size=(T, k, k))
    return M @ np.transpose(M, (0, 2, 1)) / k + shift * np.eye(k)


def chain(m, n, T, seed, zero_width=False, on_limit=True, outside=True, zero_grad=True, kappa=None, diagonal=False, wide=False):
    """The B = 0, A = I problem. cuu[t] = M M'/m + 0.2 I (cond < 100); |cu| spread over two decades so that steps come out all free, mixed
    and all clamped; cx / cxx arbitrary (they exercise the Vx / Vxx update and touch neither du nor K).
      zero_width  actuator 0 has the range [0.25, 0.25]
      on_limit    every third step a third of the actions sit exactly on a limit
      outside     every eleventh step a third of the actions lie 0.2 outside the range
      zero_grad   one step has cu = 0 with every action inside the range, actuator 0 at its zero-width value (if any) and actuator
                  min(1, m-1) exactly on its lower limit: x* = 0 exactly, a coordinate on its bound with zero gradient, which the rule counts free
      kappa       cuu[t] = Q diag(lambda) Q', lambda log-spaced from 1 down to 1/kappa
      diagonal    cuu[t] diagonal with entries k/4, k = 4..12: every pivot exact
      wide        a range no solution reaches (everything free); the edge classes above are then off"""
    rng = np.random.default_rng(seed)
    A = np.tile(np.eye(n), (T, 1, 1))
    B = np.zeros((T, n, m))
    if kappa is not None:
        lam = np.logspace(0.0, -np.log10(kappa), m) if m > 1 else np.array([1.0 / kappa])
        Q = np.linalg.qr(rng.normal(size=(T, m, m)))[0]
        cuu = (Q * lam[None, None, :]) @ np.transpose(Q, (0, 2, 1))
        cuu = 0.5 * (cuu + np.transpose(cuu, (0, 2, 1)))
    elif diagonal:
        cuu = np.zeros((T, m, m))
        cuu[:, np.arange(m), np.arange(m)] = rng.integers(4, 13, size=(T, m)) / 4.0
    else:
        cuu = _spd(rng, T, m, 0.2)
    cxx = _spd(rng, T, n, 0.5)
    cxu = 0.3 * rng.normal(size=(T, n, m))
    cx = rng.normal(size=(T, n))
    cu = rng.normal(size=(T, m)) * 10.0 ** rng.uniform(-1.3, 1.5, size=(T, 1))
    actions = rng.uniform(-0.9, 0.9, size=(T, m))
    limits = np.tile([-1.0, 1.0], (m, 1))
    zstep = None
    if wide:
        limits *= 1e15
    else:
        if zero_width:
            limits[0] = [0.25, 0.25]
        for t in range(T):
            pick = rng.random(m) < 1.0 / 3.0
            side = rng.integers(0, 2, size=m)
            if on_limit and t % 3 == 1:
                actions[t] = np.where(pick, limits[:, 0] * (1 - side) + limits[:, 1] * side, actions[t])
            if outside and t % 11 == 5:
                actions[t] = np.where(pick, np.where(side == 1, limits[:, 1] + 0.2, limits[:, 0] - 0.2), actions[t])
        if zero_grad:
            zstep = (T - 1) // 2
            cu[zstep] = 0.0
            actions[zstep] = rng.uniform(-0.5, 0.5, size=m)
            if zero_width:
                actions[zstep, 0] = 0.25
            actions[zstep, min(1, m - 1)] = limits[min(1, m - 1), 0]
    return Chain(n, m, T, (A, B, cx, cu, cxx, cxu, cuu, actions, limits), zstep, zero_width and not wide)


def kappa_chain(kappa, m):
    """cond(cuu[t]) = kappa, a range nothing reaches: every coordinate free, boxed or not"""
    return chain(m, 3, KAPPA_T, 7000 + m, kappa=kappa, wide=True)


def pivot_chain(m, t_bad, smallest):
    """diagonal cuu (entries k/4: every pivot exact), actions 0 on the range [-1, 1]; coordinate j = m // 2 keeps |g| <= 1/2, so it is
    strictly inside the range at every step and free when step t_bad, whose entry j is `smallest`, is factorised. At step t_bad every
    |g| <= 1/2: nothing is clipped there, the first Newton step is taken whole and lands on the answer (after a clipped, shortened step the
    solver's relative-improvement stop would leave a coordinate of curvature 1e-12 wherever it was: it weighs 1e-14 in the value)"""
    ch = chain(m, 3, PIVOT_T, 9000 + m, diagonal=True, on_limit=False, outside=False, zero_grad=False)
    A, B, cx, cu, cxx, cxu, cuu, actions, limits = ch.args
    j = m // 2
    actions[:] = 0.0
    cu[:, j] = np.clip(cu[:, j], -0.5, 0.5)
    cu[t_bad] = np.clip(cu[t_bad], -0.5, 0.5)
    cuu[t_bad, j, j] = smallest
    cu[t_bad, j] = 1e-13                      # x_j = -0.1 when the entry is 1e-12
    return ch


def coupled(n, m, T, seed, limit_scale=1.0):
    """a generic LQ problem (A near I, B dense): everything in a step depends on the steps after it"""
    rng = np.random.default_rng(seed)
    A = np.eye(n)[None] + 0.1 * rng.normal(size=(T, n, n))
    B = 0.3 * rng.normal(size=(T, n, m))
    def spd(k, scale):
        M = rng.normal(size=(T, k, k))
        return scale * (M @ np.transpose(M, (0, 2, 1)) / k + 0.5 * np.eye(k))
    cxx, cuu = spd(n, 1.0), spd(m, 0.5)
    cxu = 0.05 * rng.normal(size=(T, n, m))
    cx, cu = rng.normal(size=(T, n)), rng.normal(size=(T, m))
    actions = limit_scale * rng.uniform(-0.9, 0.9, size=(T, m))
    limits = limit_scale * np.tile([-1.0, 1.0], (m, 1))
    return A, B, cx, cu, cxx, cxu, cuu, actions, limits


def free_rows(K):
    """the free set a backward pass ended each step with, read off its gains: rows of K of clamped controls are exactly zero. (T-1, m) bool"""
    return np.any(np.asarray(K)[:-1] != 0.0, axis=2)


def census(free):
    """(all free, all clamped, mixed, changes): step counts of a (steps, m) free mask; changes = steps whose set differs from the one
    processed before them (the sweep runs from the last step to the first)"""
    nf = free.sum(axis=1)
    m = free.shape[1]
    return int((nf == m).sum()), int((nf == 0).sum()), int(((nf > 0) & (nf < m)).sum()), int(np.any(free[:-1] != free[1:], axis=1).sum())


def _solve_ld(H, rhs):
    """H^-1 rhs: an fp64 solve and three refinement steps with long-double residuals"""
    Hd = np.asarray(H, np.float64)
    Hl = Hd.astype(LD)
    rhs = np.asarray(rhs, LD)
    X = np.linalg.solve(Hd, rhs.astype(np.float64)).astype(LD)
    for _ in range(3):
        X = X + np.linalg.solve(Hd, (rhs - Hl @ X).astype(np.float64)).astype(LD)
    return X


KKT_SLACK = 1e-16       # times 1 + |g|max + |H|max |x|max: a thousand long-double roundings, 1e-7 of the tests' tolerances


def exact_boxqp(H, g, lo, hi, seed_x):
    """min 1/2 x'Hx + g'x on [lo, hi]. The active set is read off seed_x by the solver's rule (x <= lo and grad > 0, x >= hi and grad < 0),
    the free block is solved in long double, and the result is verified: inside the box, outward gradient on the clamped coordinates, zero
    gradient on the free ones. Returns (x, free mask, verdict); with verdict True, x is the solution to the slack."""
    H, g, lo, hi, seed_x = (np.asarray(v, np.float64) for v in (H, g, lo, hi, seed_x))
    grad = H @ seed_x + g
    at_lo, at_hi = (seed_x <= lo) & (grad > 0), (seed_x >= hi) & (grad < 0)
    free = ~(at_lo | at_hi)
    Hl, gl = H.astype(LD), g.astype(LD)
    x = np.where(at_lo, lo, np.where(at_hi, hi, 0.0)).astype(LD)
    if free.any():
        x[free] = _solve_ld(H[np.ix_(free, free)], -(gl[free] + Hl[np.ix_(free, ~free)] @ x[~free]))
    return x, free, kkt_holds(H, g, lo, hi, x, free)


def kkt_holds(H, g, lo, hi, x, free):
    Hl, gl, x = np.asarray(H, np.float64).astype(LD), np.asarray(g, np.float64).astype(LD), np.asarray(x, LD)
    grad = Hl @ x + gl
    xmax = np.max(np.abs(x)) if x.size else 0.0
    slack = KKT_SLACK * (1 + np.max(np.abs(g)) + np.max(np.abs(H)) * xmax)
    inside = np.all(x >= lo - KKT_SLACK * (1 + xmax)) and np.all(x <= hi + KKT_SLACK * (1 + xmax))
    on_lo, on_hi = ~free & (x == lo), ~free & (x == hi)
    clamped = np.all(on_lo | on_hi | free) and np.all(grad[on_lo & ~on_hi] >= -slack) and np.all(grad[on_hi & ~on_lo] <= slack)
    return bool(inside and clamped and np.all(np.abs(grad[free]) <= slack))


def bruteforce_boxqp(H, g, lo, hi):
    """the minimiser over the 3^m active sets (free / at lo / at hi per coordinate): the solution is one of these points, and every one of
    them inside the box costs at least as much. No KKT reasoning; fp64."""
    m = len(g)
    best, best_x = np.inf, None
    for assign in itertools.product((0, 1, 2), repeat=m):
        a = np.array(assign)
        free = a == 0
        x = np.where(a == 1, lo, np.where(a == 2, hi, 0.0))
        if free.any():
            x[free] = np.linalg.solve(H[np.ix_(free, free)], -(g[free] + H[np.ix_(free, ~free)] @ x[~free]))
        if np.all(x >= lo - 1e-12) and np.all(x <= hi + 1e-12):
            v = 0.5 * x @ H @ x + g @ x
            if v < best:
                best, best_x = v, x
    return best_x


def exact_gain(H, free, Qxu):
    """K (m x n) = -H_ff^-1 Qxu' on the free rows, zero on the clamped rows; Qxu is n x m"""
    Qxu = np.asarray(Qxu, np.float64)
    K = np.zeros((len(free), Qxu.shape[0]), LD)
    if free.any():
        K[free] = -_solve_ld(np.asarray(H)[np.ix_(free, free)], Qxu[:, free].T.astype(LD))
    return K


def exact_value_step(Qx, Qxx, Qxu, Quu, Qu, du, K):
    """one step of the cost-to-go in long double: Vx = Qx + K'(Quu du + Qu) + Qxu du, Vxx = sym(Qxx + K' Quu K + Qxu K + (Qxu K)'),
    and the step's (dV0, dV1) = (du'Qu, 1/2 du' Quu du)"""
    Qx, Qxx, Qxu, Quu, Qu, du, K = (np.asarray(v, LD) for v in (Qx, Qxx, Qxu, Quu, Qu, du, K))
    qd = Quu @ du
    Vx = Qx + K.T @ (qd + Qu) + Qxu @ du
    QK = Qxu @ K
    Vxx = Qxx + K.T @ (Quu @ K) + QK + QK.T
    return Vx, 0.5 * (Vxx + Vxx.T), np.array([du @ Qu, 0.5 * (du @ qd)], LD)


def regularised(H, mu):
    """Quu + mu I as the backward pass forms it (reg_type 0): an fp64 addition on the diagonal"""
    Hr = np.array(H, np.float64)
    Hr[np.arange(len(Hr)), np.arange(len(Hr))] += mu
    return Hr


def exact_chain(ch: Chain, mu, use_limits, seed_du=None):
    """The exact outputs of a backward pass over a chain at reg_type 0: dict(du, K, Vx, Vxx, dV, free, rejected), long double.
    seed_du (T x m, the ORACLE's du) proposes each step's active set when use_limits; rejected counts the steps whose KKT check failed."""
    n, m, T = ch.n, ch.m, ch.T
    A, B, cx, cu, cxx, cxu, cuu, actions, limits = ch.args
    du, K = np.zeros((T, m), LD), np.zeros((T, m, n), LD)
    Vx, Vxx, dV = np.zeros((T, n), LD), np.zeros((T, n, n), LD), np.zeros(2, LD)
    free = np.ones((T - 1, m), bool)
    Vx[T - 1], Vxx[T - 1] = cx[T - 1], cxx[T - 1]
    rejected = 0
    lo, hi = ch.lo, ch.hi
    for t in range(T - 2, -1, -1):
        Hr = regularised(cuu[t], mu)
        if use_limits:
            du[t], free[t], good = exact_boxqp(Hr, cu[t], lo[t], hi[t], seed_du[t])
            rejected += not good
        else:
            du[t] = -_solve_ld(Hr, cu[t])
        K[t] = exact_gain(Hr, free[t], cxu[t])
        Vx[t], Vxx[t], d = exact_value_step(cx[t].astype(LD) + Vx[t + 1], cxx[t].astype(LD) + Vxx[t + 1], cxu[t], cuu[t], cu[t], du[t], K[t])
        dV += d
    du[T - 1], K[T - 1] = du[T - 2], K[T - 2]
    return dict(du=du, K=K, Vx=Vx, Vxx=Vxx, dV=dV, free=free, rejected=rejected)


def rel_err(got, exact):
    """max |got - exact| / (1 + |exact|), the measure every tolerance of the backward-pass tests is stated in"""
    exact = np.asarray(exact, LD)
    return float(np.max(np.abs(np.asarray(got, LD) - exact) / (1 + np.abs(exact)))) if exact.size else 0.0
