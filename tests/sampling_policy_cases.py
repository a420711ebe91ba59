"""Sampling-policy harness (test infrastructure, like feedback_policy_cases.py; not a conftest, no GPU code of its own): exact answers for
the two things every rollout of the sampling planners starts with -- the candidate's spline nodes clamp(nominal + sigma z) and the action
clamp(TimeSpline::Sample(nodes, time)) of every step --, the cases every copy of them is held to those answers at, and the error bounds.

THE METHOD. Both halves are pure functions of what a launch records; neither the physics nor a solver enters.
  nodes    fetch_spline(c) == clamp(nominal + sigma z) of global candidate candidate_offset + c                              (check_nodes)
  actions  actions[t] == clamp(Sample(fetch_spline(c), times[t])) for t < H - 1, from fetch_trajectory(c); row H - 1 repeats row H - 2
           bit for bit (trajectory.cc:189: "copy final action")                                                              (check_actions)

THE REFERENCE IS INDEPENDENT OF THE CODE UNDER TEST.
  noise    written from the text of include/mjpcx.h (mjpcx_noise_spec), not from oracle/rng.c or a kernel: Philox4x32-10 in Python integers
           (philox; pinned by the three Random123 vectors of tests/test_rng.py), key (seed_lo, seed_hi), counter (candidate, pair, iteration,
           stream); u = (k + 1/2) / 2^53 an exact rational, k the top 53 bits of a word pair; z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = ... sin,
           in mpmath at 50 digits with the true pi; parameter j = node nu + actuator takes pair j / 2, z(j % 2); the Bernoulli test u < 0.2 of
           stream 1 is decided on the integer k against the double 0.2; sigma as the header states it for both modes.
  spline   sample_gradient_cases.resample_rational: TimeSpline::Sample in exact rational arithmetic from the reference's spline.cc
           (std::upper_bound, the end nodes held outside the grid, zero / linear / cubic Hermite with Slope per node, one-sided at both
           ends), used as a linear form of the node values (resample_weights).
  INPUTS are what the kernel reads: on a 32-bit context the nominal, the control range and the node times are rounded to float first, and
  the recorded node is a float. std0, std1 and the variance are doubles in the launch arguments (the wave copy rounds them: see below).

ERROR BOUNDS, derived here and nowhere fitted to a kernel; u = 2^-53, or 2^-24 where float arithmetic is involved; gamma_n = n u / (1 - n u).
  spline   gamma_n times M, M the sum of the absolute values of every monomial times |node value| (it holds for any order of summation,
           fused or not). COUNT per copy -- rollout_lane.h, wave_kernel.h (generic and tree), quad_step.h, limb_step.h and sg_spline_sample
           evaluate the same expressions: s = (time - tl) / (tu - tl) 3; s3 = s s s 3 x 3 + 2 = 11; s3 - 2 s2 + s two additions 13; the span
           and the product with it 15; a slope 0.5 (p1 - p0) / dt_mid + 0.5 (...) / (...): difference, span, division, sum 4 (0.5 x is
           exact): 19; coefficient x slope 1, the four-term sum 3: 23 on the longest path. N_CUBIC = 24, the count of
           sample_gradient_cases.py, covers all six. Linear: s 3, 1 - s 1, product 1, sum 1: 6; N_LINEAR = 8. Zero-order hold and both ends
           are copies: bound 0, compared for equality. resample_weights gives sum_p A_p |v_p| >= M.
  normal   device u: ((double) k + 0.5) 2^-53 rounds k + 1/2 to even once k >= 2^52 (u >= 1/2): |du| <= 2^-54 there, 0 below.
           theta = fl(2pi~ u2), 2pi~ the double constant (relative error <= u), one product: |dtheta| <= 2 u theta + 2 pi |du2|.
           cos / sin: 1-Lipschitz in theta, plus the function: ULP_FN = 4 ulp ASSUMED for the device's log, sqrt, sincos, cos and sin (no
           document on the build machine tabulates them; 1 ulp <= 2 u |result|; glibc's are within 1): |dcos| <= |dtheta| + 8 u.
           r = sqrt(-2 log u1): log within 8 u relatively, halved under the root, the root's own 8 u: 12 u r; and |du1| / (u1 r) from the
           rounded uniform (d/du sqrt(-2 ln u) = -1 / (u r)): this term grows as u1 -> 1 (r -> 0) and is why the bound is computed per draw.
           z = r cos: |dz| <= r |dcos| + |cos| |dr| + u |z|.                                                              (normal_pair)
  node     sigma = 0.5 (hi - lo) std: two roundings (CE: the root's 8 u); the product sigma z and the sum: one each:
           |dv| <= sigma |dz| + (s_rel + gamma_2) |sigma z| + gamma_1 (|nominal| + |sigma z|); the clamp is 1-Lipschitz.
           On a 32-bit context the lane, quad and limb copies do this in double and round the stored node once; THE WAVE COPY (generic and
           tree kernels) FORMS THE NODE IN FLOAT: std, hi - lo, their product, z, sigma z and the sum each rounded to float, at most 6
           roundings on a path; gamma_8(2^-24) (|nominal| + |sigma z|) is added on every 32-bit context and covers both.
The bound the tests use is HEADROOM = 4 times that (the margin of the earlier harnesses). The double-precision oracle is held to a quarter
of it on the CPU. CONDITIONS (asserted whenever a bound is computed; not measurements): every fp64 bound <= 1e-11 (hi - lo), every fp32
bound <= 2e-3 (hi - lo).

COMPARISON RULE (compare), for nodes and for actions, x* the exact unclamped value, b its bound:
  clamped    x* outside [lo, hi] by more than b: the recorded value equals that limit bit for bit. A COPY (b = 0) of a node that sits on a
             limit is counted here too: x* = limit exactly, the recorded value must be the limit bit for bit.
  ambiguous  b > 0 and x* within b of a limit: only lo <= got <= hi is required. At most 0.5 % of a family-group's entries (asserted, on
             the CPU for the reference alone and again on every device run).
  interior   everything else: |got - x*| <= b; with b = 0 equal (a zero of either sign: no copy is asked to keep the sign of a zero node).
The census (shares, regimes met) is returned for the tests to assert per family-group.

No product code imports this module."""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

import mpmath
import numpy as np

import feedback_policy_cases as fpc
from sample_gradient_cases import resample_weights

M = mpmath.mp.clone()
M.dps = 50
mpf = M.mpf
U64, U32 = 2.0 ** -53, 2.0 ** -24
ULP_FN = 4               # assumed (see above)
N_LINEAR, N_CUBIC = 8, 24
N_INTERP = {0: 0, 1: N_LINEAR, 2: N_CUBIC}
HEADROOM = 4
SLACK = HEADROOM * (1 + 2.0 ** -10)
CAP = {64: 1e-11, 32: 2e-3}          # times (hi - lo)
AMBIGUOUS_CAP = 0.005
T0, H = 0.25, 12
TWO53 = 1 << 53
REGIMES = ("before_first", "past_end", "on_knot", "left_slope", "right_slope", "mean_slopes", "unequal_spans", "two_knots_in_one_step",
           "all_before", "all_after")
gamma = fpc.gamma
rounded = fpc.rounded


# ------------------------------------------------------------------------------------------------ the noise, from include/mjpcx.h
def philox(ctr, key):
    """Philox4x32-10 (Salmon et al., Random123) in Python integers"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


def uniform_k(seed, candidate, c, iteration, stream):
    """the two 53-bit integers k of counter (candidate, c, iteration, stream): u = (k + 1/2) / 2^53"""
    o = philox([candidate & 0xFFFFFFFF, c & 0xFFFFFFFF, iteration & 0xFFFFFFFF, stream], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return ((o[0] << 32) | o[1]) >> 11, ((o[2] << 32) | o[3]) >> 11


def takes_std1(seed, candidate, iteration):
    """stream 1, c = 0: u1 < 0.2 against the double 0.2, decided in integers"""
    k, _ = uniform_k(seed, candidate, 0, iteration, 1)
    return Fraction(2 * k + 1, 2 * TWO53) < Fraction(0.2)


_PAIRS = {}


def normal_pair(k1, k2):
    """((z0, z1), (bound of z0, bound of z1)) in mpmath: the exact Box-Muller pair of the uniforms (k + 1/2) / 2^53 and the worst case of a
    double-precision evaluation with ULP_FN-ulp functions (before HEADROOM)"""
    if (k1, k2) not in _PAIRS:
        u = mpf(U64)
        u1, u2 = (mpf(k1) + 0.5) / TWO53, (mpf(k2) + 0.5) / TWO53
        du1, du2 = (mpf(2) ** -54 if k1 >= TWO53 // 2 else 0), (mpf(2) ** -54 if k2 >= TWO53 // 2 else 0)
        r, theta = M.sqrt(-2 * M.log(u1)), 2 * M.pi * u2
        d_theta = 2 * u * theta + 2 * M.pi * du2
        d_fn = d_theta + 2 * ULP_FN * u
        d_r = 3 * ULP_FN * u * r + du1 / (u1 * r)
        c, s = M.cos(theta), M.sin(theta)
        z = (r * c, r * s)
        _PAIRS[(k1, k2)] = (z, tuple(r * d_fn + abs(f) * d_r + u * abs(v) for f, v in zip((c, s), z)))
    return _PAIRS[(k1, k2)]


@dataclass
class NoiseCase:
    """one mjpcx_rollout_noise launch (H = 2: only the nodes are read), or one environment of a batched one"""
    name: str
    model: str
    P: int
    N: int
    nominal: np.ndarray            # [P, nu]
    seed: int = 1
    iteration: int = 0
    mode: int = 0
    candidate_offset: int = 0
    nominal_candidate: int = 0
    explore_count: int = 0
    std0: float = 0.1
    std1: float = 0.0
    variance: np.ndarray | None = None     # [P nu], cross-entropy
    t0: float = T0
    rows: tuple | None = None              # the local candidates that are compared (None: all N)
    _ref: dict = field(default_factory=dict, repr=False)

    def checked(self):
        return range(self.N) if self.rows is None else self.rows

    def spec(self):
        from mujoco_mpc_amd import capi
        return capi.make_noise_spec(seed=self.seed, iteration=self.iteration, mode=self.mode, candidate_offset=self.candidate_offset,
                                    nominal_candidate=self.nominal_candidate, explore_count=self.explore_count, std0=self.std0, std1=self.std1,
                                    param_variance=self.variance)

    def node_times(self):
        h = float(fpc.packed(self.model)[0].struct.timestep)
        return self.t0 + h * (np.arange(self.P) + 0.3)

    def reference(self, precision):
        """(x* [N, P, nu], bound [N, P, nu], std1 taken [N]) : the exact unclamped nodes of the local candidates checked()"""
        if precision in self._ref:
            return self._ref[precision]
        j = fpc.Joints.of(fpc.setup(self.model)[0].model)
        nu = j.nu
        rng_ = rounded(j.ctrlrange, precision)
        nom = rounded(self.nominal, precision).reshape(-1)
        want, bound, took = np.zeros((self.N, self.P * nu)), np.zeros((self.N, self.P * nu)), np.zeros(self.N, bool)
        u = mpf(U64)
        for c in self.checked():
            gi = self.candidate_offset + c
            if gi == self.nominal_candidate:
                want[c] = nom
                continue
            std = mpf(self.std0)
            if self.mode == 0 and self.std1 > 0 and takes_std1(self.seed, gi, self.iteration):
                std, took[c] = mpf(self.std1), True
            for jj in range(self.P * nu):
                k = jj % nu
                (z, ez) = normal_pair(*uniform_k(self.seed, gi, jj // 2, self.iteration, 0))
                z, ez = z[jj % 2], ez[jj % 2]
                lo, hi = mpf(float(rng_[k, 0])), mpf(float(rng_[k, 1]))
                if self.mode == 0:
                    sigma, s_rel = mpf(0.5) * (hi - lo) * std, gamma(2, u)
                else:
                    fl = mpf(self.std0 if gi < self.explore_count else self.std1)
                    sd = M.sqrt(mpf(float(self.variance[jj])))
                    sigma, s_rel = (sd if sd > fl else fl), 2 * ULP_FN * u
                n0, sz = mpf(float(nom[jj])), sigma * z
                e = sigma * ez + (s_rel + gamma(2, u)) * abs(sz) + u * (abs(n0) + abs(sz))
                if precision == 32:
                    e += gamma(8, U32) * (abs(n0) + abs(sz))
                want[c, jj], bound[c, jj] = float(n0 + sz), float(SLACK * e)
        self._ref[precision] = (want.reshape(self.N, self.P, nu), bound.reshape(self.N, self.P, nu), took)
        return self._ref[precision]


# ------------------------------------------------------------------------------------------------ census and the comparison rule
@dataclass
class Census:
    interior: int = 0
    clamped: int = 0
    ambiguous: int = 0
    worst: float = 0.0          # max |got - x*| / bound over the entries compared by value
    worst_bound: float = 0.0    # largest bound / (hi - lo)
    regimes: set = field(default_factory=set)
    where: str = ""

    def add(self, o):
        self.interior += o.interior; self.clamped += o.clamped; self.ambiguous += o.ambiguous
        if o.worst > self.worst:
            self.worst, self.where = o.worst, o.where
        self.worst_bound = max(self.worst_bound, o.worst_bound)
        self.regimes |= o.regimes
        return self

    @property
    def total(self):
        return self.interior + self.clamped + self.ambiguous

    @property
    def clamped_share(self):
        return self.clamped / max(self.total, 1)

    def assert_shares(self, what, regimes=(), clamped=(0.10, 0.50)):
        n = self.total
        assert n > 0 and self.ambiguous <= AMBIGUOUS_CAP * n, (what, self)
        if clamped is not None:
            assert clamped[0] * n <= self.clamped <= clamped[1] * n, (what, self)
        assert set(regimes) <= self.regimes, (what, sorted(set(regimes) - self.regimes))

    def __str__(self):
        return (f"{self.total} entries: {self.interior} interior, {self.clamped} clamped ({100 * self.clamped_share:.1f} %), "
                f"{self.ambiguous} ambiguous; regimes {sorted(self.regimes)}")


def same_bits(a, b):
    return a == b and np.signbit(a) == np.signbit(b)


def compare(out: Census, precision, w, b, got, lo, hi, where, scale=1.0, copy_of=None):
    """the comparison rule on one entry; copy_of: the value a bound-0 entry must repeat bit for bit (a held node)"""
    assert b <= CAP[precision] * (hi - lo), (where, b, "the bound exceeds its cap: change the case")
    out.worst_bound = max(out.worst_bound, b / (hi - lo))
    b *= scale
    where = f"{where}: got {got!r}, exact {w!r}, bound {b:.3e}"
    assert np.isfinite(got), where
    if w < lo - b or w > hi + b:
        out.clamped += 1
        assert same_bits(got, lo if w < lo else hi), where
        return
    if b == 0:
        want = fpc.clamp(w if copy_of is None else copy_of, lo, hi)
        if w in (lo, hi):
            out.clamped += 1
        else:
            out.interior += 1
        assert got == want, where
        return
    if abs(w - lo) <= b or abs(w - hi) <= b:
        out.ambiguous += 1
        assert lo <= got <= hi, where
        if got in (lo, hi):
            return
    else:
        out.interior += 1
    ratio = abs(got - w) / b
    if ratio > out.worst:
        out.worst, out.where = ratio, where
    assert ratio <= 1.0, where + f": error {abs(got - w):.3e}"


def ctrlrange(model, precision):
    return rounded(fpc.Joints.of(fpc.setup(model)[0].model).ctrlrange, precision)


def check_nodes(case: NoiseCase, precision, got, scale=1.0) -> Census:
    """got [N, P, nu] (fetch_spline of local candidates 0..N-1; None: the reference alone) against clamp(nominal + sigma z)"""
    want, bound, _ = case.reference(precision)
    r = ctrlrange(case.model, precision)
    out = Census()
    alone = got is None
    for c in case.checked():
        for p in range(case.P):
            for k in range(r.shape[0]):
                w, lo, hi = float(want[c, p, k]), float(r[k, 0]), float(r[k, 1])
                g = fpc.clamp(w, lo, hi) if alone else float(got[c, p, k])
                compare(out, precision, w, float(bound[c, p, k]), g, lo, hi, f"{case.name} fp{precision} candidate {c} node {p} actuator {k}", scale)
    return out


# ------------------------------------------------------------------------------------------------ the spline
class Grid:
    """the exact sample on one knot grid as a linear form of the node values, cached per (interpolation, query time)"""

    def __init__(self, knots, precision):
        self.knots = rounded(knots, precision)
        self.P = len(self.knots)
        self._at = {}

    def weights(self, interp, time):
        key = (interp, float(time))
        if key not in self._at:
            self._at[key] = resample_weights(self.knots, interp, time)
        return self._at[key]

    def up(self, time):
        return int(np.searchsorted(self.knots, time, side="right"))     # (the census only: the sample itself is resample_rational's)

    def regimes(self, interp, times):
        """the regimes the queries times[0 .. H-2] of one rollout meet"""
        kn, P, out = self.knots, self.P, set()
        ups = [self.up(t) for t in times]
        if ups[0] == P:
            out.add("all_before")
        if ups[-1] == 0:
            out.add("all_after")
        for i, (t, up) in enumerate(zip(times, ups)):
            if i and up - ups[i - 1] >= 2:
                out.add("two_knots_in_one_step")
            if up == 0:
                out.add("before_first")
                continue
            if kn[up - 1] == t:
                out.add("on_knot")
            if up == P:
                out.add("past_end")
                continue
            lo = up - 1
            if lo == 0:
                out.add("left_slope")
            if up == P - 1:
                out.add("right_slope")
            if lo > 0 or up < P - 1:
                out.add("mean_slopes")
            span = kn[up] - kn[lo]
            for other in ([kn[lo] - kn[lo - 1]] if lo > 0 else []) + ([kn[up + 1] - kn[up]] if up < P - 1 else []):
                if abs(other - span) > 0.05 * span:
                    out.add("unequal_spans")
        return out


def check_actions(name, model, precision, grid: Grid, interp, nodes, actions, times, scale=1.0) -> Census:
    """nodes [N, P, nu] as fetch_spline gave them, actions [N, H, nu] (None: the reference alone), times [N, H] as fetch_trajectory gave them"""
    r = ctrlrange(model, precision)
    nodes, times = np.asarray(nodes, np.float64), np.asarray(times, np.float64)
    N, Hh = times.shape
    out = Census()
    alone = actions is None
    u = U64 if precision == 64 else U32
    g = gamma(N_INTERP[interp], u)
    fr = {}
    for c in range(N):
        if not alone and Hh >= 2:
            a, b = actions[c, Hh - 1], actions[c, Hh - 2]
            assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)), (name, c, "the last row repeats the one before")
        out.regimes |= grid.regimes(interp, times[c, :Hh - 1])
        for t in range(Hh - 1):
            W = grid.weights(interp, times[c, t])
            for k in range(r.shape[0]):
                lo, hi = float(r[k, 0]), float(r[k, 1])
                val, mag, copy_of = Fraction(0), Fraction(0), None
                for p, (w, a) in W.items():
                    v = float(nodes[c, p, k])
                    if v not in fr:
                        fr[v] = Fraction(v)
                    val += w * fr[v]
                    mag += a * abs(fr[v])
                    if a == 0:
                        copy_of = v
                w_, b_ = float(val), float(SLACK * g * mag)
                got = fpc.clamp(w_ if copy_of is None else copy_of, lo, hi) if alone else float(actions[c, t, k])
                compare(out, precision, w_, b_, got, lo, hi, f"{name} fp{precision} interp {interp} candidate {c} step {t} actuator {k}", scale,
                        copy_of if b_ == 0 else None)
    return out


# ------------------------------------------------------------------------------------------------ spline cases
GRIDS = {   # knot offsets from the start time, in steps
    "S1": [k + 0.3 for k in range(5)],
    "S2": [0, 0.4, 2.1, 3.1, 5.6, 6.2, 7.5],
    "S3": [2.5],
    "S4": [-0.5, 1.5],
    "S5": [-0.2, 1.1, 2.6],
    "S6a": [-3.5, -2.25, -0.5],
    "S6b": [H + 0.5, H + 1.75, H + 3.0],
    "S8": None,     # 0.17 k - 1.75, k < P (about six knots pass per step; P = 70: the last knot at 9.98 steps, so knots 64 .. 69 are read)
}
# S2's knots 5.6 and 6.2 do not share a step (the queries fall on whole steps), so two_knots_in_one_step is S8's (six knots a step) and S6a's
# (every knot passed before the first query); S8 begins 1.75 steps before the start so that with P = 70 the knots past the 64th are read.
GROUPS = {   # group: (grids, regimes the group must meet)
    "S1": (("S1",), {"before_first", "left_slope", "mean_slopes", "right_slope", "past_end"}),
    "S2": (("S2",), {"on_knot", "left_slope", "mean_slopes", "right_slope", "unequal_spans", "past_end"}),
    "S3-S6": (("S3", "S4", "S5", "S6a", "S6b"), {"before_first", "past_end", "left_slope", "right_slope", "mean_slopes", "all_before", "all_after"}),
    "S7": (("S7",), {"on_knot", "mean_slopes"}),
    "S8": (("S8",), {"mean_slopes", "two_knots_in_one_step", "past_end"}),
}
HIT = {"S2": (0,), "S7": (2, 5)}      # knots a query falls on: their nodes stay off the limits (an exact hit of a limit under a bound > 0 is ambiguous)
S7_STEPS = (3, 7)


def step_of(model):
    return float(fpc.packed(model)[0].struct.timestep)


def knots_of(model, grid, P=None, times=None):
    """the knot times of a grid; S7 needs the recorded `times` of a rollout: its knots 2 and 5 are times[3] and times[7] bit for bit"""
    h = step_of(model)
    if grid == "S8":
        return T0 + h * (0.17 * np.arange(P) - 1.75)
    if grid == "S7":
        kn = T0 + h * np.array([-0.6, 1.3, 0.0, 4.2, 5.7, 0.0, 8.4, 9.1])
        kn[2], kn[5] = times[S7_STEPS[0]], times[S7_STEPS[1]]
        return kn
    return T0 + h * np.asarray(GRIDS[grid], float)


def node_values(model, grid, P, N, amplitude=1.0):
    """[N, P, nu] in the control range (scaled by `amplitude` about its middle): node p of candidate c, actuator k sits exactly on a limit
    when (p + c + k) % 3 == 0 -- one third, never two neighbours, so that the cubic overshoots next to it --, the others uniform in the
    range, a signed zero here and there (where 0 is in the range)"""
    j = fpc.Joints.of(fpc.setup(model)[0].model)
    lo, hi = j.ctrlrange[:, 0], j.ctrlrange[:, 1]
    mid, half = 0.5 * (lo + hi), 0.5 * amplitude * (hi - lo)
    rng = np.random.default_rng([11, list(GRIDS).index(grid) if grid in GRIDS else 99, P, N])
    v = mid + half * rng.uniform(-1, 1, size=(N, P, j.nu))
    side = rng.uniform(size=(N, P, j.nu)) < 0.5
    c, p, k = np.meshgrid(np.arange(N), np.arange(P), np.arange(j.nu), indexing="ij")
    on = (p + c + k) % 3 == 0
    for q in HIT.get(grid, ()):
        on[:, q, :] = False
    v = np.where(on, np.where(side, mid - half, mid + half), v)
    zero_ok = (lo < 0) & (hi > 0)
    z = ((p + 2 * c + k) % 7 == 1) & ~on & zero_ok[None, None, :]
    v = np.where(z, np.where(side, -0.0, 0.0), v)
    return v


# ------------------------------------------------------------------------------------------------ noise cases
SEARCHED_SEED, SEARCHED_ITERATION = 0x5EED0001C0FFEE11, 3
SEARCHED = {   # tools/search_noise_counters.py: global candidates whose pair 0 (stream 0) has the property; recomputed in integers by the CPU tests
    "u1_small": 1102855,
    "u1_near_one": 1280230,
    "u2_0": 1443074,
    "u2_quarter": 1205448,
    "u2_half": 1689538,
    "u2_three_quarters": 1191558,
    "u2_1": 1163427,
}
BERNOULLI_WINDOW = dict(seed=0x5EED0001C0FFEE11, iteration=3, candidate=248347307)   # stream-1 uniform in [0.2, (double) 0.2f)
PROPERTY = {
    "u1_small": lambda u1, u2: u1 < Fraction(1, 10 ** 6),
    "u1_near_one": lambda u1, u2: 1 - u1 < Fraction(1, 10 ** 6),
    "u2_0": lambda u1, u2: u2 < Fraction(1, 10 ** 6),
    "u2_quarter": lambda u1, u2: abs(u2 - Fraction(1, 4)) < Fraction(1, 10 ** 6),
    "u2_half": lambda u1, u2: abs(u2 - Fraction(1, 2)) < Fraction(1, 10 ** 6),
    "u2_three_quarters": lambda u1, u2: abs(u2 - Fraction(3, 4)) < Fraction(1, 10 ** 6),
    "u2_1": lambda u1, u2: 1 - u2 < Fraction(1, 10 ** 6),
}


def _nominal(model, P, scale=0.5, seed=3):
    j = fpc.Joints.of(fpc.setup(model)[0].model)
    lo, hi = j.ctrlrange[:, 0], j.ctrlrange[:, 1]
    return 0.5 * (lo + hi) + scale * 0.5 * (hi - lo) * np.random.default_rng([seed, P]).uniform(-1, 1, size=(P, j.nu))


def _nu(model):
    return fpc.Joints.of(fpc.setup(model)[0].model).nu


_NOISE = {}


def noise_cases(model, N, P=5, rows=None):
    """the sampling-mode and cross-entropy cases of one model. P nu is odd on the Cartpole (P = 5): the last pair is half used."""
    if (model, N, P, rows) in _NOISE:
        return _NOISE[(model, N, P, rows)]
    nu = _nu(model)
    big = (1 << 32) + 12345
    nom = _nominal(model, P)
    var = np.random.default_rng([5, P, nu]).uniform(0.01, 0.09, size=P * nu)     # sqrt: 0.1 .. 0.3
    var[0::3] = 1e-4                                                              # below both floors
    var[1::5] = 0.0
    out = [
        # std 0.4 of the half range about a nominal up to half of it out: a fair share of the nodes is clamped
        NoiseCase(f"{model}-ps-plain", model, P, N, nom, seed=7, std0=0.4, nominal_candidate=0),
        NoiseCase(f"{model}-ps-mixture", model, P, N, nom, seed=(0xA5A5A5A5 << 32) | 99, iteration=5, std0=0.1, std1=0.6, nominal_candidate=-1),
        NoiseCase(f"{model}-ps-offset", model, P, N, nom, seed=big, iteration=2, candidate_offset=(1 << 20) + 77, std0=0.15, std1=0.5,
                  nominal_candidate=(1 << 20) + 77 + N // 2),
        NoiseCase(f"{model}-ce-explore", model, P, N, 0.3 * nom, seed=big + 1, iteration=1, mode=1, nominal_candidate=-1, explore_count=N // 2,
                  std0=0.35, std1=0.05, variance=var),
        NoiseCase(f"{model}-ce-offset", model, P, N, 0.3 * nom, seed=11, iteration=4, mode=1, candidate_offset=1000, nominal_candidate=-1,
                  explore_count=1000 + N - 1, std0=0.2, std1=0.12, variance=var),
    ]
    for c in out:
        c.rows = rows
    _NOISE[(model, N, P, rows)] = out
    return out


def searched_cases(model, N=3, P=2):
    """one launch per searched counter: nominal 0, std0 = 0.1 -- nothing clamps and node 0 shows the normal; local candidate 1 is the searched one"""
    nu = _nu(model)
    j = fpc.Joints.of(fpc.setup(model)[0].model)
    mid = np.tile(0.5 * (j.ctrlrange[:, 0] + j.ctrlrange[:, 1]), (P, 1))
    key = ("searched", model, N, P)
    if key not in _NOISE:
        _NOISE[key] = [NoiseCase(f"{model}-{name}", model, P, N, mid, seed=SEARCHED_SEED, iteration=SEARCHED_ITERATION, candidate_offset=gi - 1,
                                 nominal_candidate=-1, std0=0.1, rows=None if N <= 3 else (0, 1, 2)) for name, gi in SEARCHED.items()]
    return _NOISE[key]


def bernoulli_case(model, N=3, P=2):
    """local candidate 1 draws a stream-1 uniform in [0.2, (double) 0.2f): std0 by the header's double comparison, std1 = 4 std0 by a float one"""
    j = fpc.Joints.of(fpc.setup(model)[0].model)
    mid = np.tile(0.5 * (j.ctrlrange[:, 0] + j.ctrlrange[:, 1]), (P, 1))
    w = BERNOULLI_WINDOW
    return NoiseCase(f"{model}-bernoulli-window", model, P, N, mid, seed=w["seed"], iteration=w["iteration"], candidate_offset=w["candidate"] - 1,
                     nominal_candidate=-1, std0=0.05, std1=0.2, rows=None if N <= 3 else (0, 1, 2))


def batched_noise_cases(model, n, P=5, E=3, ce=False, rows=None):
    """E environments of one rollout_noise_batched(_ce) launch: environment e is the plain case with seed + e (and its own variance row)"""
    base = noise_cases(model, n, P, rows)[3 if ce else 2]
    out = []
    for e in range(E):
        var = None if not ce else np.roll(base.variance, e) * (1 + 0.5 * e)
        out.append(NoiseCase(f"{base.name}-env{e}", model, P, n, base.nominal * (1 - 0.2 * e), seed=base.seed + e, iteration=base.iteration, mode=base.mode,
                             candidate_offset=base.candidate_offset, nominal_candidate=base.nominal_candidate, explore_count=base.explore_count,
                             std0=base.std0, std1=base.std1, variance=var, t0=T0 + 0.5 * e, rows=rows))
    return out


# ------------------------------------------------------------------------------------------------ running a case
def run_spline_device(ctx, model, interp, knots, nodes, horizon=H, t0=T0):
    """Context.rollout_splines -> (recorded nodes [N, P, nu], actions [N, H, nu], times [N, H])"""
    _, start, mocap = fpc.setup(model)
    ctx.set_state(start, t0, mocap)
    ctx.rollout_splines(horizon, interp, knots, nodes)
    _, actions, times = fpc.fetch_all(ctx)
    got_nodes = np.stack([ctx.fetch_spline(c) for c in range(ctx.N)])
    want = rounded(nodes, ctx.precision)
    assert np.array_equal(got_nodes, want) and np.array_equal(np.signbit(got_nodes), np.signbit(want)), "fetch_spline returns the nodes it was given"
    return got_nodes, actions, times


def run_spline_oracle(model, interp, knots, nodes, horizon=H, t0=T0):
    from oracle import pyoracle
    pm, pt = fpc.packed(model)
    _, start, mocap = fpc.setup(model)
    nodes = np.asarray(nodes, float)
    ref = pyoracle.rollout_batch(pm, pt, start, t0, mocap, nodes.shape[0], horizon, nodes.shape[1], interp, knots, nodes, num_threads=4)
    assert not ref["failure"].any()
    return nodes, ref["actions"], ref["times"]


def run_noise_device(ctx, case: NoiseCase, interp=0):
    _, start, mocap = fpc.setup(case.model)
    ctx.set_state(start, case.t0, mocap)
    ctx.rollout_noise(case.N, 2, interp, case.node_times(), case.nominal, case.spec())
    ctx.sync()
    got = np.zeros((case.N, case.P, ctx.nu))
    for c in case.checked():
        got[c] = ctx.fetch_spline(c)
    return got


def spline_group(model, group, run, precision, n_lane=70, n_other=5, P8=70, amplitude=1.0, scale=1.0, first_times=None, rows=None):
    """every grid of a group under the three interpolations through `run(interp, knots, nodes) -> (nodes, actions, times)`; actions None:
    the reference alone. S7 runs twice: the first pass (grid S1) only records the step times."""
    lane = model in ("cartpole", "particle")
    N = n_lane if lane else n_other
    total = Census()
    for grid in GROUPS[group][0]:
        times = None
        if grid == "S7":
            times = first_times if first_times is not None else run(0, knots_of(model, "S1"), node_values(model, "S1", 5, N, amplitude))[2][0]
        P = P8 if grid == "S8" else (8 if grid == "S7" else len(GRIDS[grid]))
        knots = knots_of(model, grid, P, times)
        nodes = node_values(model, grid, P, N, amplitude)
        g = Grid(knots, precision)
        for interp in (0, 1, 2):
            got_nodes, actions, tms = run(interp, knots, nodes)
            if grid == "S7":
                kn = rounded(knots, precision)
                assert tms[0, S7_STEPS[0]] == kn[2] and tms[0, S7_STEPS[1]] == kn[5], "S7: the knots sit on the step times bit for bit"
            if rows is not None:     # (a launch of many candidates, a few of them compared)
                got_nodes, actions, tms = got_nodes[list(rows)], None if actions is None else actions[list(rows)], tms[list(rows)]
            total.add(check_actions(f"{model}-{grid}", model, precision, g, interp, got_nodes, actions, tms, scale))
    return total
