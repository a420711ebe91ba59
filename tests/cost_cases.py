"""Cost harness (test infrastructure, like riccati_cases.py and selection_cases.py; not a conftest, no GPU code of its own): exact
answers for mjpc::Norm (norm.cc:50-210), CostDerivatives::Compute (cost_derivatives.cc:112-230) and BaseResidualFn::CostValue
(task.cc:71-110), the residual points at which the device kernels are held to them, and the error bounds.

THE REFERENCE IS INDEPENDENT OF THE CODE UNDER TEST. Only each norm's VALUE is written here (value_1d / value_of_c, from the
formula in norm.cc's comment and the line that computes y), in mpmath at 70 digits. The gradient and the Hessian are mpmath.diff of
that value: for the norms that are a sum over the entries, y = sum f(x_i), g_i = f'(x_i), H_ii = f''(x_i); for the two norms of
c = x'x, y = phi(c), g = 2 x phi'(c), H = 2 phi'(c) I + 4 phi''(c) x x'. The second route is the chain rule on the value, not the
reference's hand-derived b and e; tests/test_cost_cases.py checks it against mpmath.diff of the n-variable value itself. Norms of
|x_i| (power loss, smooth-abs2) are differentiated in a = |x_i| and g_i = sign(x_i) f'(a): with an integer exponent f is analytic
at 0 and the even extension has the same second derivative there.

WHERE THE REFERENCE BRANCHES instead of differentiating, the expected result is stated (exact_norm, `branch`):
    null           norm.cc:61-70    y = x[0], g = [1], H = 0
    l2_s0          norm.cc:122-138  s = sqrt(x'x + p^2) == 0 (p = 0 at x = 0): g = 0, H = 0
    smoothabs_s0   norm.cc:170-171  the same per entry
    rectify_p<=0   norm.cc:197-201  y = sum max(x_i, 0), g_i = [x_i > 0], H = 0
    l22_minval     norm.cc:108      0 < c < mjMINVAL: the (q - 2) / c of the Hessian becomes (q - 2) / mjMINVAL, i.e.
                                    H = H_exact + 2 phi'(c) (q - 2) (1 / mjMINVAL - 1 / c) x x'
    l22_zero       norm.cc:96-111   c = 0, q >= 2: d = pow(0, q/2 - 1) is 1 (q = 2) or 0, so g = 0 and H = I / p (q = 2) or 0
    power_zero     norm.cc:157-160  x_i = 0, p >= 2: g_i = 0, H_ii = 2 (p = 2) or 0 (the limits of the derivatives)
    smoothabs2_zero norm.cc:183-185 x_i = 0, q >= 2: g_i = 0, H_ii = 1 / p (q = 2) or 0 (likewise)
and where the reference's own double arithmetic leaves the finite numbers, its pattern is the expectation (`nonfinite`):
    power loss, x_i = 0, p = 1      H_ii = 0 * 1 * pow(0, -1) = 0 * inf = NaN, g_i = 0
    power loss, x_i = 0, 1 < p < 2  H_ii = +inf, g_i = 0
    smooth-abs2, x_i = 0, q < 2     c = s pow(0, q - 2) / e = inf: g_i = inf * 0 = NaN, H_ii = +inf
    L22, x = 0, q < 2               d = pow(0, q/2 - 1) = inf: every g_i = inf * 0 = NaN, every H_ij = NaN; y stays finite
    rectify, x_i / p = 1000         exp overflows: y = +inf, g_i = inf / inf = NaN, H_ii = NaN
    cosh, x_i / p = +-800           cosh overflows: y = +inf, g_i = +-inf, H_ii = +inf

ERROR BOUNDS, derived here and nowhere fitted to a kernel: a running first-order forward-error analysis of the reference's own
formulas (model_norm restates them for this purpose only: it sizes the bound, it does not supply the expected value). Every
quantity is a pair (value, bound on |computed - exact|) in working precision u (2^-53; 2^-24 for the fp32 value path):
    a +- b        e_a + e_b + u |a +- b|                      one correctly rounded operation (IEEE 754)
    a * b, a / b  the product / quotient rule on e_a, e_b, + u |result|
    sqrt          e_a / (2 sqrt a) + 1 ulp                    (1 ulp <= 2 u |result|; correctly rounded in both libraries)
    exp, log      |f'(a)| e_a + ULP ulps of the result        fp64: exp 2, log 2, pow 4, cosh 4, sinh 4 ulps;
    pow, cosh,                                                fp32: exp 4, log 2, pow 8, cosh 4, sinh 6 ulps -- twice the maximum
    sinh                                                      errors the CUDA / HIP programming guides tabulate for these functions
                                                              (exp 1 / 2, log 1 / 1, pow 2 / 4, cosh 2 / 2, sinh 2 / 3 in fp64 / fp32;
                                                              glibc's libm stays within them), as room for another math library
    sum of n      sum e_i + (n - 1) u sum |v_i|               any order of summation (the kernel and the oracle may differ in it)
    dot of n      sum (|a_i| e_b_i + |b_i| e_a_i) + (n + 1) u sum |a_i b_i|     gamma_n of Higham 3.1, any order, fused or not
A fused multiply-add rounds once where the model rounds twice, so contraction stays inside it. The cancellations of the formulas
(s - p for |x| << p, cosh(z) - 1, a - b of two pows) need no special case: the bound of s carries u p into s - p, whatever is left
of the difference. The assembly (bound_cost_derivatives) runs the same analysis through H rx, (H rx)' rx, the weights w_k / T, the
accumulation over the terms (num_term additions per entry) and the risk transform, with the magnitudes of the addends taken from
the double-precision evaluation itself. The model is first order; the final (1 + 2^-10) covers the second-order terms (every
relative error here is below 2^-10 of its operand wherever it is multiplied on) and the double-precision evaluation of the bound.

That analysis is a worst case which an implementation that obeys the model CAN reach: on a formula of three operations the
double-precision oracle comes to half of it. The bound the tests use is HEADROOM = 4 times the worst case, so that an implementation
with another order of operations, another math library or other contractions is not held to the last rounding; a wrong term or a
wrong branch is off by the size of the entry, 2^50 times the bound. tests/test_cost_cases.py holds the oracle to a QUARTER of the
bound, i.e. to the worst case itself: that is the check that the analysis is right, not a tuning of it."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import mpmath
import numpy as np

M = mpmath.mp.clone()      # a context of its own: sympy's global one keeps its precision
M.dps = 70
U64, U32 = 2.0 ** -53, 2.0 ** -24
MINVAL = 1e-15             # mjMINVAL
RISK_TOL = 1.0e-6          # kRiskNeutralTolerance
NORMS = (-1, 0, 1, 2, 3, 5, 6, 7, 8)
NPARAM = {-1: 0, 0: 0, 1: 2, 2: 1, 3: 1, 5: 1, 6: 1, 7: 2, 8: 1}
ULPS64 = dict(sqrt=1, exp=2, log=2, pow=4, cosh=4, sinh=4)
ULPS32 = dict(sqrt=1, exp=4, log=2, pow=8, cosh=4, sinh=6)
HEADROOM = 4
SLACK = HEADROOM * (1 + 2.0 ** -10)
REF_EPS = 1e-45            # the reference's own error: mpmath.diff at 70 digits (a linear f's second derivative comes out as ~1e-80, not 0)
EXP_OVERFLOW, COSH_OVERFLOW = 709.782712893384, 710.4758600739439   # beyond these exp / cosh of a double is +inf
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ the values, in mpmath
def _pw(a, e):
    """a^e; an integer exponent stays an integer, so that a <= 0 stays real (|x|^2 is analytic through 0)"""
    e = M.mpf(e)
    return M.power(a, int(e)) if e == int(e) else M.power(a, e)


def value_1d(t, p, q):
    """f with y = sum_i f(x_i) (types 0, 3, 6, 8) or sum_i f(|x_i|) (types 5, 7): the formulas of norm.cc's comments"""
    p, q = M.mpf(p), M.mpf(q)
    return {0: lambda x: x * x / 2,                                   # 0.5 x'x
            3: lambda x: p * p * (M.cosh(x / p) - 1),                  # p^2 (cosh(x / p) - 1)
            5: lambda a: _pw(a, p),                                    # |x|^p
            6: lambda x: M.sqrt(x * x + p * p) - p,                    # sqrt(x^2 + p^2) - p
            7: lambda a: _pw(_pw(a, q) + _pw(p, q), 1 / q) - p,        # (|x|^q + p^q)^(1/q) - p
            8: lambda x: p * M.log(1 + M.exp(x / p))}[t]               # p log(1 + exp(x / p))


def value_of_c(t, p, q):
    """phi with y = phi(x'x): L22 as norm.cc:92-98 computes it, ((x'x)^(q/2) + p^q)^(1/q) - p, and L2, sqrt(x'x + p^2) - p"""
    p, q = M.mpf(p), M.mpf(q)
    return {1: lambda c: _pw(_pw(c, q / 2) + _pw(p, q), 1 / q) - p, 2: lambda c: M.sqrt(c + p * p) - p}[t]


def norm_value_mp(t, x, p, q):
    """the value alone, of mpmath numbers (what tests differentiate in n variables to check the chain rule of exact_norm)"""
    if t == -1:
        return x[0]
    if t in (1, 2):
        return value_of_c(t, p, q)(sum(v * v for v in x))
    if t == 8 and not p > 0:
        return sum(v if v > 0 else M.mpf(0) for v in x)
    f = value_1d(t, p, q)
    return sum(f(abs(v) if t in (5, 7) else v) for v in x)


@dataclass
class Exact:
    y: object                  # mpf, or a float inf / nan
    g: list                    # n entries: mpf, or a float inf / nan
    H: list                    # n x n
    branches: set = field(default_factory=set)
    nonfinite: bool = False

    def arrays(self):
        """(y, g, H) as doubles (non-finite entries kept)"""
        return float(self.y), np.array([float(v) for v in self.g]), np.array([[float(v) for v in row] for row in self.H])


_EXACT = {}


def exact_norm(t, x, p=0.0, q=0.0):
    """value, gradient and Hessian of norm type t at the doubles x with the doubles p, q: see the module docstring"""
    key = (t, tuple(float(v).hex() for v in x), float(p), float(q))
    if key not in _EXACT:
        _EXACT[key] = _exact_norm(t, [float(v) for v in x], float(p), float(q))
    return _EXACT[key]


def _exact_norm(t, x, p, q):
    n = len(x)
    zero = M.mpf(0)
    X = [M.mpf(v) for v in x]
    g, H, br = [zero] * n, [[zero] * n for _ in range(n)], set()
    if t == -1:                                                                      # norm.cc:61-70
        g[0] = M.mpf(1)
        return Exact(X[0], g, H, {"null"})
    if t in (1, 2):
        c = sum(v * v for v in X)
        phi = value_of_c(t, p, q)
        if t == 2 and c == 0 and p == 0:                                             # norm.cc:122-138
            return Exact(zero, g, H, {"l2_s0"})
        if t == 1 and c == 0:
            y = phi(zero)
            if q < 2:                                                                # d = pow(0, q/2 - 1) = inf
                return Exact(y, [NAN] * n, [[NAN] * n for _ in range(n)], {"l22_zero_q<2"}, True)
            if q == 2:
                for i in range(n):
                    H[i][i] = 1 / M.mpf(p)
            return Exact(y, g, H, {"l22_zero"})
        d1, d2 = M.diff(phi, c, 1), M.diff(phi, c, 2)
        for i in range(n):
            g[i] = 2 * X[i] * d1
            for j in range(n):
                H[i][j] = (2 * d1 if i == j else zero) + 4 * X[i] * X[j] * d2
        if t == 1 and c < M.mpf(MINVAL):                                             # norm.cc:108
            br.add("l22_minval")
            k = 2 * d1 * (M.mpf(q) - 2) * (1 / M.mpf(MINVAL) - 1 / c)
            for i in range(n):
                for j in range(n):
                    H[i][j] += k * X[i] * X[j]
        return Exact(phi(c), g, H, br)
    if t == 8 and not p > 0:                                                         # norm.cc:197-201
        return Exact(sum((v if v > 0 else zero) for v in X), [M.mpf(1) if v > 0 else zero for v in X], H, {"rectify_p<=0"})
    f = value_1d(t, p, q)
    y, nonfinite = zero, False
    for i, v in enumerate(X):
        a = abs(v) if t in (5, 7) else v
        sgn = (1 if v > 0 else (-1 if v < 0 else 0)) if t in (5, 7) else 1
        if t == 6 and v == 0 and p == 0:                                             # norm.cc:170-171
            br.add("smoothabs_s0")
            continue
        if t == 3 and abs(x[i] / p) > COSH_OVERFLOW:
            y, g[i], H[i][i], nonfinite = INF, math.copysign(INF, x[i] / p) * (1 if p > 0 else -1), INF, True
            br.add("cosh_overflow")
            continue
        if t == 8 and x[i] / p > EXP_OVERFLOW:
            y, g[i], H[i][i], nonfinite = INF, NAN, NAN, True
            br.add("rectify_overflow")
            continue
        e = p if t == 5 else q
        if t in (5, 7) and v == 0:
            if e < 2:
                nonfinite = True
                if t == 5:
                    g[i], H[i][i] = zero, (NAN if e == 1 else INF)
                    br.add("power_zero_p=1" if e == 1 else "power_zero_p<2")
                else:
                    g[i], H[i][i] = NAN, INF
                    br.add("smoothabs2_zero_q<2")
                y = y + f(a) if not isinstance(y, float) else y
                continue
            br.add("power_zero" if t == 5 else "smoothabs2_zero")
            if e != int(e):                      # not analytic at 0: the one-sided limits, both 0 for an exponent above 2
                y = y + f(a) if not isinstance(y, float) else y
                continue
        if not isinstance(y, float):
            y = y + f(a)
        g[i] = sgn * M.diff(f, a, 1)
        H[i][i] = M.diff(f, a, 2)
    return Exact(y, g, H, br, nonfinite)


# ------------------------------------------------------------------------------------------------ the running error analysis
class Model:
    def __init__(self, u=U64, ulps=None):
        self.u, self.ulps = u, (ulps or (ULPS64 if u == U64 else ULPS32))

    def const(self, v):
        return V(float(v), 0.0, self)

    def sum(self, terms):
        terms = list(terms)
        if not terms:
            return self.const(0)
        v = math.fsum(t.v for t in terms)
        return V(v, sum(t.e for t in terms) + (len(terms) - 1) * self.u * sum(abs(t.v) for t in terms), self)


class V:
    """a computed quantity: its value (evaluated in double) and a bound on |computed in precision u - exact|"""
    __slots__ = ("v", "e", "m")

    def __init__(self, v, e, m):
        self.v, self.e, self.m = v, e, m

    def _c(self, o):
        return o if isinstance(o, V) else V(float(o), 0.0, self.m)

    def __add__(self, o):
        o = self._c(o)
        v = self.v + o.v
        return V(v, self.e + o.e + self.m.u * abs(v), self.m)

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.e, self.m)

    def __sub__(self, o):
        return self + (-self._c(o))

    def __rsub__(self, o):
        return self._c(o) + (-self)

    def __mul__(self, o):
        o = self._c(o)
        v = self.v * o.v
        return V(v, abs(self.v) * o.e + abs(o.v) * self.e + self.m.u * abs(v), self.m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._c(o)
        v = self.v / o.v
        return V(v, self.e / abs(o.v) + abs(v) * o.e / abs(o.v) + self.m.u * abs(v), self.m)

    def __rtruediv__(self, o):
        return self._c(o) / self

    def _ulp(self, name, v):
        return self.m.ulps[name] * 2 * self.m.u * abs(v)

    def sqrt(self):
        v = math.sqrt(self.v)
        return V(v, (self.e / (2 * v) if v > 0 else math.sqrt(self.e)) + self._ulp("sqrt", v), self.m)

    def exp(self):
        v = math.exp(self.v)
        return V(v, v * self.e + self._ulp("exp", v), self.m)

    def log(self):
        v = math.log(self.v)
        return V(v, self.e / self.v + self._ulp("log", v), self.m)

    def cosh(self):
        v = math.cosh(self.v)
        return V(v, abs(math.sinh(self.v)) * self.e + self._ulp("cosh", v), self.m)

    def sinh(self):
        v = math.sinh(self.v)
        return V(v, math.cosh(self.v) * self.e + self._ulp("sinh", v), self.m)

    def pow(self, ex):
        ex = self._c(ex)
        if self.v == 0:                     # pow(0, e): 1 for e = 0, 0 for e > 0, both exact; the model is asked for no other
            assert self.e == 0 and ex.v >= 0, "pow(0, negative) is a non-finite case: no bound"
            return V(1.0 if ex.v == 0 else 0.0, 0.0, self.m)
        v = self.v ** ex.v
        return V(v, abs(v) * (abs(ex.v) * self.e / self.v + abs(math.log(self.v)) * ex.e) + self._ulp("pow", v), self.m)


def model_norm(m, t, x, p, q, derivatives=True):
    """norm.cc:50-210 as written there, in the arithmetic of V: -> (y, g[n], H[n][n]) of V. Bounds only; see the module docstring."""
    n = len(x)
    X, P, Q = [m.const(v) for v in x], m.const(p), m.const(q)
    zero, one = m.const(0), m.const(1)
    g, H = [zero] * n, [[zero] * n for _ in range(n)]
    if t == -1:
        g[0] = one
        return X[0], g, H
    if t == 0:
        for i in range(n):
            H[i][i] = one
        return m.sum(v * v for v in X) * 0.5, X, H
    if t == 1:
        c = m.sum(v * v for v in X)
        a = c.pow(Q / 2) + P.pow(Q)
        s = a.pow(1 / Q)
        y = s - P
        if derivatives:
            d = c.pow(Q / 2 - 1)
            b = s / a * d
            e = (1 - Q) * d / a + (Q - 2) / (c if c.v > MINVAL else m.const(MINVAL))
            g = [b * v for v in X]
            H = [[b * ((1.0 if i == j else 0.0) + X[i] * X[j] * e) for j in range(n)] for i in range(n)]
        return y, g, H
    if t == 2:
        s = m.sum([v * v for v in X] + [P * P]).sqrt()
        if derivatives and s.v != 0:
            inv = 1 / s
            g = [v * inv for v in X]
            H = [[((1.0 if i == j else 0.0) - g[i] * g[j]) / s for j in range(n)] for i in range(n)]
        return s - P, g, H
    ys = []
    for i, v in enumerate(X):
        if t == 3:
            z = v / P
            ys.append(P * P * (z.cosh() - 1.0))
            g[i], H[i][i] = P * z.sinh(), z.cosh()
        elif t == 5:
            s = m.const(abs(v.v))
            ys.append(s.pow(P))
            if derivatives:
                g[i] = (1.0 if v.v > 0 else (-1.0 if v.v < 0 else 0.0)) * P * s.pow(P - 1)
                H[i][i] = (P - 1) * P * s.pow(P - 2)
        elif t == 6:
            s = (v * v + P * P).sqrt()
            ys.append(s - P)
            if derivatives and s.v != 0:
                g[i] = v / s
                H[i][i] = (1 - g[i] * g[i]) / s
        elif t == 7:
            a = m.const(abs(v.v))
            d = a.pow(Q)
            e = d + P.pow(Q)
            s = e.pow(1 / Q)
            ys.append(s - P)
            if derivatives:
                c = s * a.pow(Q - 2) / e
                g[i], H[i][i] = c * v, c * (Q - 1) * (1 - d / e)
        elif t == 8:
            if p > 0:
                s = (v / P).exp()
                ys.append(P * (1 + s).log())
                g[i], H[i][i] = s / (1 + s), s / (P * (1 + s) * (1 + s))
            else:
                ys.append(v if v.v > 0 else zero)
                g[i] = one if v.v > 0 else zero
        else:
            raise KeyError(t)
    return m.sum(ys), g, H


def bound_norm(t, x, p=0.0, q=0.0, u=U64):
    """bounds on the errors of (y, g, H) computed in precision u, as doubles"""
    y, g, H = model_norm(Model(u), t, [float(v) for v in x], float(p), float(q))
    return y.e * SLACK, np.array([v.e for v in g]) * SLACK, np.array([[v.e for v in row] for row in H]) * SLACK


# ------------------------------------------------------------------------------------------------ the cost of a task
@dataclass
class Spec:
    """a task's cost: term widths, norm types, (p, q) per term, weights, risk"""
    dim: list
    norm: list
    par: list
    weight: list
    risk: float = 0.0

    def shifts(self):
        return np.concatenate([[0], np.cumsum(self.dim)]).astype(int)

    def norm_parameter(self):
        return [float(v) for k, t in enumerate(self.norm) for v in self.par[k][:NPARAM[t]]]

    def num_norm_parameter(self):
        return [NPARAM[t] for t in self.norm]

    def rounded32(self):
        f = lambda v: float(np.float32(v))
        return Spec(list(self.dim), list(self.norm), [(f(p), f(q)) for p, q in self.par], [f(w) for w in self.weight], f(self.risk))

    def terms(self, r):
        sh = self.shifts()
        return [(k, self.norm[k], [float(v) for v in r[sh[k]:sh[k + 1]]], float(self.par[k][0]), float(self.par[k][1])) for k in range(len(self.dim))]


def task_with(task, spec):
    """a copy of `task` with spec's layout, norms, parameters, weights and risk: nothing else changes"""
    import copy
    t2 = copy.copy(task)
    assert sum(spec.dim) == task.num_residual
    t2.num_term, t2.dim_norm_residual, t2.norm = len(spec.dim), list(spec.dim), list(spec.norm)
    t2.num_norm_parameter, t2.norm_parameter = spec.num_norm_parameter(), spec.norm_parameter()
    t2.weight, t2.risk = [float(w) for w in spec.weight], float(spec.risk)
    return t2


def exact_cost_value(spec, r):
    """BaseResidualFn::CostValue (task.cc:71-110) at the doubles r: mpf, or a float inf / nan"""
    c = M.mpf(0)
    for k, t, x, p, q in spec.terms(r):
        y = exact_norm(t, x, p, q).y
        if isinstance(y, float):
            return y
        c += M.mpf(spec.weight[k]) * y
    if abs(spec.risk) < RISK_TOL:
        return c
    return (M.exp(M.mpf(spec.risk) * c) - 1) / M.mpf(spec.risk)


def bound_cost_value(spec, r, u=U64):
    m = Model(u)
    c = m.sum(m.const(spec.weight[k]) * model_norm(m, t, x, p, q, derivatives=False)[0] for k, t, x, p, q in spec.terms(r))
    if not abs(spec.risk) < RISK_TOL:
        c = ((m.const(spec.risk) * c).exp() - 1.0) / m.const(spec.risk)
    return c.e * SLACK


def is_finite_case(spec, r):
    return not any(exact_norm(t, x, p, q).nonfinite for k, t, x, p, q in spec.terms(r))


def running_cost(spec, T, r):
    """c = sum_k (w_k / T) y_k as a double (for the census of risk * c)"""
    return float(sum(M.mpf(spec.weight[k]) / T * exact_norm(t, x, p, q).y for k, t, x, p, q in spec.terms(r)))


NAMES = ("cx", "cu", "cxx", "cxu", "cuu")


def exact_cost_derivatives(spec, T, r, C, D):
    """one time step of CostDerivatives::Compute (cost_derivatives.cc:112-230) at the doubles r[nr], C[nr, ndx], D[nr, nu], in mpmath:
    -> dict of object arrays cx, cu, cxx, cxu, cuu. Finite cases only."""
    C, D = np.asarray(C, float), np.asarray(D, float)
    ndx, nu = C.shape[1], D.shape[1]
    sh = spec.shifts()
    zero = M.mpf(0)
    cx, cu = [zero] * ndx, [zero] * nu
    cxx, cxu, cuu = [[zero] * ndx for _ in range(ndx)], [[zero] * nu for _ in range(ndx)], [[zero] * nu for _ in range(nu)]
    c = zero
    for k, t, x, p, q in spec.terms(r):
        ex = exact_norm(t, x, p, q)
        assert not ex.nonfinite
        n = len(x)
        w = M.mpf(spec.weight[k]) / T                                           # weights[i] / T, cost_derivatives.cc:154
        rx = [[M.mpf(v) for v in row] for row in C[sh[k]:sh[k + 1]]]
        ru = [[M.mpf(v) for v in row] for row in D[sh[k]:sh[k + 1]]]
        rxu = [rx[a] + ru[a] for a in range(n)]                                 # [rx ru]: n x (ndx + nu)
        c += w * ex.y
        full = t in (1, 2)
        Hr = [[(M.fdot(ex.H[a], [rxu[b][j] for b in range(n)]) if full else ex.H[a][a] * rxu[a][j]) for j in range(ndx + nu)] for a in range(n)]
        for i in range(ndx + nu):
            gi = w * M.fdot([rxu[a][i] for a in range(n)], ex.g)
            if i < ndx:
                cx[i] += gi
            else:
                cu[i - ndx] += gi
            col = [Hr[a][i] for a in range(n)]
            for j in range(i, ndx + nu):                                        # the Gauss-Newton block [rx ru]' H [rx ru], upper triangle
                v = w * M.fdot(col, [rxu[a][j] for a in range(n)])
                if j < ndx:
                    cxx[i][j] += v
                    if j != i:
                        cxx[j][i] += v
                elif i < ndx:
                    cxu[i][j - ndx] += v
                else:
                    cuu[i - ndx][j - ndx] += v
                    if j != i:
                        cuu[j - ndx][i - ndx] += v
    if not abs(spec.risk) < RISK_TOL:                                           # cost_derivatives.cc:160-225
        risk = M.mpf(spec.risk)
        s = M.exp(risk * c)
        cx, cu = [v * s for v in cx], [v * s for v in cu]                       # scaled first: the rank-one terms below use THESE
        cxx = [[cxx[i][j] * s + risk * s * cx[i] * cx[j] for j in range(ndx)] for i in range(ndx)]
        cxu = [[cxu[i][j] * s + risk * s * cx[i] * cu[j] for j in range(nu)] for i in range(ndx)]
        cuu = [[cuu[i][j] * s + risk * s * cu[i] * cu[j] for j in range(nu)] for i in range(nu)]
    return dict(cx=np.array(cx, object), cu=np.array(cu, object), cxx=np.array(cxx, object).reshape(ndx, ndx),
                cxu=np.array(cxu, object).reshape(ndx, nu), cuu=np.array(cuu, object).reshape(nu, nu))


def _amul(u, a, b):
    (va, ea), (vb, eb) = a, b
    v = va * vb
    return v, np.abs(va) * eb + np.abs(vb) * ea + u * np.abs(v)


def _aadd(u, a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + u * np.abs(v)


def _adot(u, A, eA, B, eB, n):
    """A @ B of inner length n with entry-wise error bounds eA, eB"""
    return A @ B, eA @ np.abs(B) + np.abs(A) @ eB + (n + 1) * u * (np.abs(A) @ np.abs(B))


def bound_cost_derivatives(spec, T, r, C, D, u=U64):
    """bounds on the errors of one time step's cx, cu, cxx, cxu, cuu computed in precision u -> dict of double arrays"""
    C, D = np.asarray(C, float), np.asarray(D, float)
    ndx, nu = C.shape[1], D.shape[1]
    sh = spec.shifts()
    m = Model(u)
    K = len(spec.dim)
    acc = {k: [] for k in NAMES}
    cterms = []
    for k, t, x, p, q in spec.terms(r):
        n = len(x)
        y, g, H = model_norm(m, t, x, p, q)
        gv, ge = np.array([v.v for v in g]), np.array([v.e for v in g])
        Hv, He = np.array([[v.v for v in row] for row in H]), np.array([[v.e for v in row] for row in H])
        w = m.const(spec.weight[k]) / float(T)
        cterms.append(w * y)
        W = (w.v, w.e)
        rx, ru = C[sh[k]:sh[k + 1]], D[sh[k]:sh[k + 1]]
        zx, zu = np.zeros_like(rx), np.zeros_like(ru)
        Hrx, Hru = _adot(u, Hv, He, rx, zx, n), _adot(u, Hv, He, ru, zu, n)
        acc["cx"].append(_amul(u, W, _adot(u, rx.T, zx.T, gv, ge, n)))
        acc["cu"].append(_amul(u, W, _adot(u, ru.T, zu.T, gv, ge, n)))
        acc["cxx"].append(_amul(u, W, _adot(u, Hrx[0].T, Hrx[1].T, rx, zx, n)))
        acc["cxu"].append(_amul(u, W, _adot(u, Hrx[0].T, Hrx[1].T, ru, zu, n)))
        acc["cuu"].append(_amul(u, W, _adot(u, Hru[0].T, Hru[1].T, ru, zu, n)))
    out = {}
    for name in NAMES:      # cx_t[i] += w * s, once per term: K additions per entry
        v = sum(a[0] for a in acc[name])
        out[name] = (v, sum(a[1] for a in acc[name]) + K * u * sum(np.abs(a[0]) for a in acc[name]))
    if not abs(spec.risk) < RISK_TOL:
        s = (m.const(spec.risk) * m.sum(cterms)).exp()
        S, RS = (s.v, s.e), ((m.const(spec.risk) * s).v, (m.const(spec.risk) * s).e)
        out["cx"], out["cu"] = _amul(u, out["cx"], S), _amul(u, out["cu"], S)
        col = lambda a: (a[0][:, None], a[1][:, None])
        row = lambda a: (a[0][None, :], a[1][None, :])
        for name, a, b in (("cxx", "cx", "cx"), ("cxu", "cx", "cu"), ("cuu", "cu", "cu")):
            out[name] = _aadd(u, _amul(u, out[name], S), _amul(u, _amul(u, RS, col(out[a])), row(out[b])))
    return {k: v[1] * SLACK for k, v in out.items()}


def worst_ratio(got, exact, bound):
    """max over the entries of |got - exact| / bound (0 / 0 counts as 0; an error above a zero bound as inf)"""
    worst = 0.0
    for gv, ev, bv in zip(np.asarray(got, float).reshape(-1), np.asarray(exact, object).reshape(-1), np.asarray(bound, float).reshape(-1)):
        if not math.isfinite(gv):
            return INF
        err = float(abs(M.mpf(float(gv)) - ev)) - REF_EPS * (1 + abs(float(ev)))
        worst = max(worst, 0.0 if err <= 0 else (INF if bv == 0 else err / bv))
    return worst


def pattern(a):
    """which entries are nan, +inf, -inf: what is compared where the reference leaves the finite numbers"""
    a = np.asarray(a, float)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


# ------------------------------------------------------------------------------------------------ residual points
@dataclass
class Point:
    """one residual slice for one norm: `branch` names the branch of exact_norm it is meant to hit (None: a derivative everywhere)"""
    t: int
    x: tuple
    p: float = 0.0
    q: float = 0.0
    branch: str = None
    note: str = ""

    @property
    def nonfinite(self):
        return exact_norm(self.t, self.x, self.p, self.q).nonfinite


GENERIC = ((0.3, -0.7), (1.25, 0.5), (-2.0, 0.125))
ZEROS = ((0.0, 0.4), (0.0, 0.0), (-0.0, 0.0))          # one entry 0, all 0, signed zeros


def points(n=2):
    """the points of every norm type but the null norm, n = 2 entries each (the Particle's terms); wider slices: widen()"""
    P = []
    add = lambda t, xs, p=0.0, q=0.0, branch=None, note="": P.extend(Point(t, tuple(x), p, q, branch, note) for x in xs)
    add(0, GENERIC + ZEROS + ((1e-8, 1e3),))
    for q in (1.5, 2.0, 3.0):                                                        # L22
        add(1, GENERIC + ((0.0, 0.4), (1e-3, 2e-3), (1e3, -5e2)), 0.1, q)
        add(1, ((1e-8, 1e3), (0.5, 1e-8)), 1e-3, q)
        add(1, ((1e-9, 2e-9),), 1.0, q, "l22_minval")                                # c = 5e-18 < mjMINVAL
        add(1, ((0.0, 0.0), (-0.0, 0.0)), 0.1, q, "l22_zero_q<2" if q < 2 else "l22_zero")
    for p in (0.1, 1e-3, 1.0):                                                       # L2
        add(2, GENERIC + ZEROS, p)
    add(2, ((1e-8, 2e-8), (1e-4, 0.0)), 1.0, note="cancelling")                      # |x| << p: s - p loses digits
    add(2, ((1e3, 1e3), (1e-8, 1e3)), 1e-3)
    add(2, ((0.3, -0.7),), 0.0)                                                      # p = 0 away from 0: |x|
    add(2, ((0.0, 0.0), (-0.0, 0.0)), 0.0, branch="l2_s0")
    for p in (0.5, 1.0):                                                             # cosh (|x / p| stays moderate: it is an exponential)
        add(3, GENERIC + ZEROS + ((1e-8, 1e-3), (5.0, -10.0)), p)
    add(3, ((400.0, 0.1), (0.1, -400.0)), 0.5, branch="cosh_overflow")               # x / p = +-800
    for p in (1.0, 1.5, 2.0, 3.0):                                                   # power loss
        add(5, GENERIC + ((1e-8, 1e3),), p)
        add(5, ZEROS, p, branch={1.0: "power_zero_p=1", 1.5: "power_zero_p<2"}.get(p, "power_zero"))
    for p in (0.1, 1e-3, 1.0):                                                       # smooth-abs
        add(6, GENERIC + ZEROS + ((1e-8, 1e3),), p)
    add(6, ((1e-8, 1e-4),), 1.0, note="cancelling")
    add(6, ((0.3, -0.7),), 0.0)
    add(6, ((0.0, 0.4), (0.0, -0.0)), 0.0, branch="smoothabs_s0")
    for q in (1.5, 2.0, 3.0):                                                        # smooth-abs2
        add(7, GENERIC + ((1e-3, 2e-3), (1e3, -5e2)), 0.1, q)
        add(7, ((1e-8, 1e3),), 1e-3, q)
        add(7, ((1e-8, 1e-4),), 1.0, q, note="cancelling")
        add(7, ZEROS, 0.1, q, branch="smoothabs2_zero_q<2" if q < 2 else "smoothabs2_zero")
    for p in (0.3, 1.0):                                                             # rectify
        add(8, GENERIC + ZEROS + ((1e-8, 10.0), (-10.0, 5.0)), p)
    add(8, ((1e-3, -2e-3), (0.02, -0.03)), 1e-3)
    add(8, GENERIC + ZEROS, 0.0, branch="rectify_p<=0")
    add(8, ((0.3, -0.7),), -0.5, branch="rectify_p<=0")
    add(8, ((300.0, 0.1),), 0.3, branch="rectify_overflow")                          # x / p = 1000
    if n != 2:
        P = [widen(pt, n) for pt in P]
    return P


def widen(pt, n):
    """the point's pattern repeated (with the signs alternating) over n entries"""
    if n == 1 and pt.branch:         # the entry that takes the branch: the zero if there is one, else the larger
        zeros = [v for v in pt.x if v == 0]
        return Point(pt.t, (zeros[0] if zeros else max(pt.x, key=abs),), pt.p, pt.q, pt.branch, pt.note)
    x = [pt.x[i % 2] * (1 if (i // 2) % 2 == 0 else -1) * (1 + (i // 2) / 8 if pt.branch is None else 1) for i in range(n)]
    return Point(pt.t, tuple(x), pt.p, pt.q, pt.branch, pt.note)


NULL_POINTS = tuple(Point(-1, (v,), branch="null") for v in (0.3, 0.0, -2.5))       # the null norm is for terms of one residual (task.cc:214)
RISKS = (0.0, 9e-7, -9e-7, 1.1e-6, -1.1e-6, 0.7, -0.7)
RISK_LARGE = 1.0                 # with HEAVY weights on a generic point: risk * c of order 10
HEAVY = (12.0, 9.0)
WEIGHTS = (1.7, 0.6)
PARTNER = Point(6, (0.25, -0.15), 0.2)     # the other term of a Particle case: a free term, so that a branch term never stands alone


def groups(pts):
    """points that share (type, p, q) run as the T steps of one launch"""
    out = {}
    for pt in pts:
        out.setdefault((pt.t, pt.p, pt.q), []).append(pt)
    return out


def dense(rng, shape):
    """no exact zeros, magnitudes in [0.25, 2): a non-finite entry then spreads the same way in any order of summation"""
    return rng.uniform(0.25, 2.0, shape) * rng.choice([-1.0, 1.0], shape)


# ------------------------------------------------------------------------------------------------ the runs of the Particle
@dataclass
class Run:
    """one launch: T steps of one cost specification (risk is set per call)"""
    name: str
    spec: Spec
    r: np.ndarray      # T x nr
    C: np.ndarray      # T x nr x ndx
    D: np.ndarray      # T x nr x nu
    pts: list

    @property
    def T(self):
        return self.r.shape[0]

    def with_risk(self, risk):
        return Spec(self.spec.dim, self.spec.norm, self.spec.par, self.spec.weight, float(risk))

    def finite(self, t, risk=0.0):
        """every norm of step t is finite and, past the risk switch, |risk * c| <= 50 (exp overflows at 709: such a step is compared
        with the oracle's pattern, like the steps whose norms leave the finite numbers)"""
        if not is_finite_case(self.spec, self.r[t]):
            return False
        return abs(risk) < RISK_TOL or abs(risk * running_cost(self.spec, self.T, self.r[t])) <= 50


CHUNKS = (1, 2, 5)       # T of the launches: T = 1 makes w / T = w


def particle_runs(placement, seed=5):
    """every point of points() on term `placement` of the Particle's [2, 2] layout, PARTNER on the other; points of one (type, p, q)
    are the steps of launches of T = 1, 2, 5 in turn. C and D are dense."""
    rng = np.random.default_rng(seed + placement)
    runs, turn = [], 0
    for (t, p, q), pts in groups(points()).items():
        i = 0
        while i < len(pts):
            left = len(pts) - i
            size = CHUNKS[turn % 3] if CHUNKS[turn % 3] <= left else max(c for c in CHUNKS if c <= left)
            chunk = pts[i:i + size]
            i += len(chunk)
            turn += 1
            own, other = (t, (p, q)), (PARTNER.t, (PARTNER.p, PARTNER.q))
            order = (own, other) if placement == 0 else (other, own)
            spec = Spec([2, 2], [order[0][0], order[1][0]], [order[0][1], order[1][1]], list(WEIGHTS))
            r = np.array([(pt.x + PARTNER.x) if placement == 0 else (PARTNER.x + pt.x) for pt in chunk], float)
            T = len(chunk)
            runs.append(Run(f"norm{t}_p{p}_q{q}_T{T}_at{placement}", spec, r, dense(rng, (T, 4, 4)), dense(rng, (T, 4, 2)), chunk))
    return runs


def heavy_run():
    """quadratic terms with HEAVY weights at a generic point, T = 1: with RISK_LARGE, risk * c is 11.3"""
    rng = np.random.default_rng(77)
    return Run("heavy", Spec([2, 2], [0, 0], [(0.0, 0.0)] * 2, list(HEAVY)), np.array([GENERIC[1] + PARTNER.x]), dense(rng, (1, 4, 4)), dense(rng, (1, 4, 2)), [])


def identity_run():
    """C = I, quadratic norms: cx = w r / T, cxx = diag(w / T) by hand (D stays dense)"""
    rng = np.random.default_rng(78)
    r = np.array([GENERIC[0] + PARTNER.x, GENERIC[2] + PARTNER.x])
    return Run("identity", Spec([2, 2], [0, 0], [(0.0, 0.0)] * 2, list(WEIGHTS)), r, np.stack([np.eye(4)] * 2), dense(rng, (2, 4, 2)), [])


# ------------------------------------------------------------------------------------------------ the A1's 42 residuals re-laid-out
def _mix(dims, norms):
    par = {-1: (0.0, 0.0), 0: (0.0, 0.0), 1: (0.1, 3.0), 2: (0.1, 0.0), 3: (1.5, 0.0), 5: (3.0, 0.0), 6: (0.2, 0.0), 7: (0.1, 2.0), 8: (0.3, 0.0)}
    return Spec(list(dims), list(norms), [par[t] for t in norms], [0.5 + 0.25 * (k % 5) for k in range(len(dims))])


CYCLE = (-1, 0, 6, 3, 5, -1, 7, 8, 1, 2)     # norms of the 1-wide terms of the 32-term layout: the null norm on 7 of them
LAYOUTS = {
    "32+10 L22": _mix([32, 10], [1, 6]),
    "32+10 L2": _mix([32, 10], [2, 7]),
    "31x1+11": _mix([1] * 31 + [11], [CYCLE[k % len(CYCLE)] for k in range(31)] + [2]),
    "31+11": _mix([31, 11], [1, 2]),
    "16+16+10": _mix([16, 16, 10], [2, 1, 3]),
}
REFUSED = {
    "32x1+10": (_mix([1] * 32 + [10], [0] * 33), "more than 32 cost terms"),
    "33+9": (_mix([33, 9], [0, 0]), "cost term wider than 32 residuals"),
}


def layout_run(spec, T, ndx, nu, seed):
    rng = np.random.default_rng(seed)
    nr = sum(spec.dim)
    return Run("layout", spec, 0.4 * dense(rng, (T, nr)), dense(rng, (T, nr, ndx)), dense(rng, (T, nr, nu)), [])


def spec_of_task(task):
    par, s = [], 0
    for n in task.num_norm_parameter:
        v = list(task.norm_parameter[s:s + n]) + [0.0, 0.0]
        par.append((float(v[0]), float(v[1])))
        s += n
    return Spec(list(task.dim_norm_residual), list(task.norm), par, [float(w) for w in task.weight], float(task.risk))


def check_run(run, risk, got, ratios=None):
    """the assertions of one launch's outputs `got` (cx, cu, cxx, cxu, cuu, each T x ...) -> worst error / bound of the finite steps.
    Finite steps: every entry within its bound of the exact answer, cxx and cuu symmetric to it. Other steps: returned for the caller
    to compare with the oracle's pattern."""
    spec = run.with_risk(risk)
    worst = 0.0
    for t in range(run.T):
        if not run.finite(t, risk):
            continue
        ex = exact_cost_derivatives(spec, run.T, run.r[t], run.C[t], run.D[t])
        bd = bound_cost_derivatives(spec, run.T, run.r[t], run.C[t], run.D[t])
        for k, name in enumerate(NAMES):
            ratio = worst_ratio(got[k][t], ex[name], bd[name])
            if ratios is not None:
                ratios.append((ratio, run.name, risk, t, name))
            worst = max(worst, ratio)
        for k, name in ((2, "cxx"), (4, "cuu")):
            a = np.asarray(got[k][t], float)
            asym = np.abs(a - a.T)
            assert np.all(asym <= bd[name] + bd[name].T), (run.name, risk, t, name, "asymmetric")
    return worst


# ------------------------------------------------------------------------------------------------ the value path (norm_value, lane_cost)
VALUE_NORMS = (0, 1, 2, 3, 5, 6, 7, 8)      # (the null norm is for terms of one residual; the Particle's have two)
VALUE_RISKS = (0.0, 9e-7, -1.1e-6, 0.7, -0.7)
VALUE_WEIGHTS = (1.7, 0.25)                 # the norm under test on term 0, a quadratic of small weight on term 1
VELOCITY = (0.1, -0.2)
GOAL = (0.5, -0.25)


@dataclass
class ValueCase:
    point: Point
    spec: Spec            # (rounded to fp32 for an fp32 context)
    r: np.ndarray         # the residual the device must store: fl(qpos - goal), velocity -- in the context's precision, as doubles
    qpos: np.ndarray
    goal: np.ndarray


def value_cases(t, precision):
    """every point of norm type t whose VALUE is finite, under every risk of VALUE_RISKS that keeps |risk * cost| below 50; the
    generic points alternately about the goal GOAL and about 0, every other point about 0 (its zeros and magnitudes are then exact)"""
    fl = np.float32 if precision == 32 else np.float64
    out = []
    for i, pt in enumerate(pt for pt in points() if pt.t == t):
        if isinstance(exact_norm(pt.t, pt.x, pt.p, pt.q).y, float):
            continue
        x = np.array(pt.x, fl)
        about = pt.branch is None and pt.note == "" and i % 2 == 0
        goal = np.array(GOAL if about else (0.0, 0.0), fl)
        qpos = (x + goal).astype(fl) if about else x
        r = np.concatenate([(qpos - goal).astype(fl), np.array(VELOCITY, fl)]).astype(float)
        base = Spec([2, 2], [t, 0], [(pt.p, pt.q), (0.0, 0.0)], list(VALUE_WEIGHTS), 0.0)
        if precision == 32:
            base = base.rounded32()
        c = exact_cost_value(base, r)
        for risk in VALUE_RISKS:
            spec = Spec(base.dim, base.norm, base.par, base.weight, float(fl(risk)))
            if abs(spec.risk * float(c)) <= 50:
                out.append(ValueCase(pt, spec, r, qpos.astype(float), goal.astype(float)))
    return out
