"""Selection harness (test infrastructure, like riccati_cases.py; not a conftest, no GPU code of its own): return vectors whose
order is known without running a kernel, the contract of the selection entry points in plain Python, the elites' moments in exact
rational arithmetic, and the error bounds the device sums are held to.

The device chooses candidates by `less_ri` (mjpcx.hip): ascending returns, ties to the lower index, NaN last; -0.0 and +0.0 compare
equal and so tie by index. order() is that contract. inject() overwrites the returns and failure flags a rollout left on the device
(mjpcx_device_buffer hands out their pointers) with values the test chose, so every selection entry point can be held to order() bit
for bit, whatever the rollout computed.

Error bounds of the elite sums (elite_reduce, mjpcx.hip), derived, not measured. u = 2^-53, n the number of elites,
m = ceil(n / 256). Thread t adds the elites t, t + 256, ... into an accumulator that starts at zero (the first addition is exact:
at most m - 1 roundings), then the 256 partial sums go through a halving tree of 8 levels (8 roundings). A term therefore passes
through at most m + 7 rounded additions, each of relative error <= u, and (1 + u)^(m + 7) - 1 <= (m + 8) u for every m a test can
reach (m u < 2^-40). Hence
    |sum_dev - sum_exact| <= (m + 8) u sum|x_i|                                                  (sum_bound)
for the sums of mjpcx_elite_moments and the sum of the returns. The mean is that sum divided by n, one more rounding, and so is
avg_return:
    |mean_dev - mean_exact| <= (m + 10) u sum|x_i| / n                                           (mean_bound)
(m + 9 covers the division; one more for the second-order terms). For the squares every term is non-negative, so the bound is
RELATIVE: d = p - mean_dev (one rounding), d * d (one rounding; an fma contracts it into the addition and rounds less), then the
m + 7 additions, and for `variance` the division by n - 1: at most m + 10 roundings, (1 + u)^(m + 10) (1 + u)^2 - 1 for the error of
d entering squared, <= (m + 16) u with room for the second-order terms. The device's sum of (p - mean_dev)^2 and its variance are
therefore within
    (m + 16) u relative                                                                          (square_bound)
of the exact value ABOUT THE MEAN THE DEVICE REPORTED; that mean is held to mean_bound separately. Nothing here was tuned to the
kernel's output: emulate_elite_reduce() repeats the device's order of operations in numpy, tests/test_selection_cases.py shows it
inside the bounds on every data set the GPU tests use (on 513 elites of the ill-conditioned set: 0.18 u of the 11 u allowed for the
sum, 0.25 u of the 19 u allowed for the variance) and a one-pass E[x^2] - E[x]^2 variance far outside them (it returns rounding
noise on that set: off by the whole of the exact value, 1e14 times the bound)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)   # exact, so the bounds below are rationals too
STRIDE = 256            # elite_reduce's partial sums, best_segmented_kernel's stride
FAILED = 1e6            # what a failed rollout returns
LOW = 1.0               # below every value of base()
NEG_NAN = float(np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0])   # sign and payload set: still a NaN, other bits

# where the reductions change mechanism: a DPP row (row_mirror hands over to __shfl_xor), a wavefront, best_segmented_kernel's
# stride, env_sort_keys' stride and the register / memory split of the bitonic merge
PLAIN_PLACES = (0, 15, 16, 63, 64, 1023, 1024)
PLAIN_STRADDLES = ((15, 16), (63, 64), (1023, 1024))
PLAIN_N = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)
SEG_PLACES = (0, 15, 16, 63, 64, 255, 256)
SEG_STRADDLES = ((15, 16), (63, 64), (255, 256))
SEG_N = (64, 256, 320, 1024, 1088)
SEG_ELITES = (1, 2, 255, 256, 257, 513)
SEG_E = 3
LDS_LAST, SCRATCH_FIRST = 8192, 8256     # the last environment size sorted in LDS, the first sorted in the global slab


# ------------------------------------------------------------------------------------------------ the contract
def order(ret, skip=-1):
    """indices of `ret` in the order the device promises: (isnan, value, index), `skip` left out. -0.0 == +0.0: they tie by index."""
    ret = np.asarray(ret, dtype=np.float64)
    keys = [(True, 0.0, i) if ret[i] != ret[i] else (False, float(ret[i]), i) for i in range(ret.size) if i != skip]
    return np.array([k[2] for k in sorted(keys)], dtype=np.int32)


def bits(a):
    """fp64 values as uint64: equality of these counts NaN payloads and the sign of zero"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ return vectors
@dataclass
class Case:
    name: str
    ret: np.ndarray

    @property
    def nans(self):
        return int(np.isnan(self.ret).sum())

    @property
    def has_tie(self):
        """two candidates that are numbers compare equal (-0.0 == +0.0)"""
        r = self.ret[~np.isnan(self.ret)]
        return bool(r.size != np.unique(r).size)

    @property
    def has_inf(self):
        return bool(np.isinf(self.ret).any())

    @property
    def has_signed_zeros(self):
        z = np.signbit(self.ret[self.ret == 0])
        return bool(z.any() and not z.all())

    @property
    def has_failed(self):
        return bool((self.ret == FAILED).any())

    @property
    def fail(self):
        """the failure flags that go with the returns: FAILED and non-finite ones failed, with the diagnostics some kernels put
        above the low byte on every other of them"""
        bad = (self.ret == FAILED) | ~np.isfinite(self.ret)
        f = np.where(bad, 1, 0).astype(np.int32)
        f[bad & (np.arange(f.size) % 2 == 1)] |= (32 << 8) | (1 << 16)
        return f

    @property
    def winner(self):
        return int(order(self.ret)[0])


def base(n, seed):
    """a seeded permutation of n distinct finite values, all in (LOW, FAILED)"""
    return 2.0 + 0.25 * np.random.default_rng(seed).permutation(n).astype(np.float64)


def with_min(n, seed, at):
    r = base(n, seed)
    r[at] = LOW
    return r


def with_tie(n, seed, a, b):
    r = base(n, seed)
    r[a] = r[b] = LOW
    return r


def with_nan(n, seed, places):
    r = base(n, seed)
    for k, p in enumerate(places):
        r[p] = NEG_NAN if k % 2 else np.nan
    return r


def all_nan(n):
    r = np.full(n, np.nan)
    r[1::2] = NEG_NAN
    return r


def all_equal(n):
    return np.full(n, 3.5)


def with_inf(n, seed, plus, minus):
    r = base(n, seed)
    r[plus], r[minus] = np.inf, -np.inf
    return r


def signed_zeros(n, seed, plus, minus):
    """+0.0 and -0.0 as the two smallest: they are equal, so the lower INDEX goes first whichever sign it carries"""
    r = base(n, seed)
    r[plus], r[minus] = 0.0, -0.0
    return r


def with_failed(n, seed, every=3):
    r = base(n, seed)
    r[::every] = FAILED
    return r


def _fit(places, n):
    return sorted({p for p in tuple(places) + (n - 1,) if 0 <= p < n})


def build_cases(n, places, straddles, seed=0):
    """every builder that fits n candidates: the unique minimum, then a tied pair of minima, at every place and across every
    boundary; NaN, infinities, signed zeros and failed rollouts at and around them"""
    at = _fit(places, n)
    pairs = [(a, b) for a, b in straddles if b < n]
    cases = [Case("base", base(n, seed))]
    for p in at:
        cases.append(Case(f"min@{p}", with_min(n, seed + 1, p)))
    tied = pairs + [(p, n - 1) for p in at if p < n - 1] + [(0, p) for p in at[1:-1]]
    for a, b in sorted(set(tied)):
        cases.append(Case(f"tie@{a},{b}", with_tie(n, seed + 2, a, b)))
    # NaN at the places themselves, the winner next to one of them; then NaN everywhere but two tied candidates
    nan_at = [p for p in at if p % 2 == 0 or p == n - 1]
    if len(nan_at) < n:
        r = with_nan(n, seed + 3, nan_at)
        cases.append(Case("nan@places", r))
        free = [i for i in range(n) if i not in nan_at]
        r = with_nan(n, seed + 3, nan_at)
        r[free[-1]] = LOW
        cases.append(Case(f"nan@places,min@{free[-1]}", r))
    if n >= 3:
        keep = (pairs[-1] if pairs else (0, n - 1))
        r = all_nan(n)
        r[keep[0]] = r[keep[1]] = 7.0
        cases.append(Case(f"nan-but@{keep[0]},{keep[1]}", r))
    if n >= 2:
        r = all_nan(n)
        r[n - 1] = np.inf
        cases.append(Case("nan-but-inf@last", r))
    cases.append(Case("all-nan", all_nan(n)))
    cases.append(Case("all-equal", all_equal(n)))
    if n >= 2:
        cases.append(Case("inf", with_inf(n, seed + 4, 0, n - 1)))
        lo, hi = pairs[0] if pairs else (0, n - 1)
        cases.append(Case(f"zeros+@{lo},-@{hi}", signed_zeros(n, seed + 5, lo, hi)))
        cases.append(Case(f"zeros-@{lo},+@{hi}", signed_zeros(n, seed + 5, hi, lo)))
    if n >= 3:
        r = with_inf(n, seed + 6, 1, 0)
        r[n - 1] = np.nan
        cases.append(Case("inf+nan", r))
        cases.append(Case("failed", with_failed(n, seed + 7)))
        r = np.full(n, FAILED)
        r[n - 1] = FAILED - 1.0
        cases.append(Case("all-failed-but-last", r))
    return cases


def plain_cases(n):
    return build_cases(n, PLAIN_PLACES, PLAIN_STRADDLES, seed=100 + n)


def segmented_cases(n_env):
    return build_cases(n_env, SEG_PLACES, SEG_STRADDLES, seed=200 + n_env)


def segmented_rounds(n_env, num_envs=SEG_E):
    """the segmented cases dealt over num_envs environments, a DIFFERENT one in each (a wrong `first` offset shows): round r puts case
    r + e in environment e. Returns a list of rounds, each a list of num_envs cases."""
    cases = segmented_cases(n_env)
    return [[cases[(r + e) % len(cases)] for e in range(num_envs)] for r in range(len(cases))]


def elite_counts(n_env, skip=-1):
    left = n_env - (1 if 0 <= skip < n_env else 0)
    return sorted({k for k in SEG_ELITES + (n_env - 1, left) if 1 <= k <= left})


# ------------------------------------------------------------------------------------------------ nodes
def scaled_nodes(n, npar, seed):
    """well-scaled spline parameters inside the control range, [n][npar]"""
    return np.clip(np.random.default_rng(seed).normal(0, 0.6, (n, npar)), -1, 1)


def ill_nodes(n, npar, seed):
    """the ill-conditioned set: 0.75 + 1e-9 N(0, 1). The variance (1e-18) is 17 digits below the squares (0.56), so a one-pass
    E[x^2] - E[x]^2 returns rounding noise while the two-pass sum about the mean loses nothing"""
    return 0.75 + 1e-9 * np.random.default_rng(seed).normal(0, 1, (n, npar))


def ill32_nodes(n, npar, seed):
    """the same at the scale a 32-bit context can hold: 0.75 + 1e-6 N(0, 1) survives the rounding to float32 (ill_nodes collapses
    to 0.75 there: every elite equal, the variance exactly zero)"""
    return 0.75 + 1e-6 * np.random.default_rng(seed).normal(0, 1, (n, npar))


NODE_SETS = {"scaled": scaled_nodes, "ill": ill_nodes, "ill32": ill32_nodes}


def as_device(nodes, precision):
    """the node values as a context of that precision holds them, in fp64"""
    nodes = np.asarray(nodes, dtype=np.float64)
    return nodes.astype(np.float32).astype(np.float64) if precision == 32 else nodes


# ------------------------------------------------------------------------------------------------ exact moments, bounds
def _scaled(values):
    """finite floats as integers over one power of two: (ints, shift) with value_i == ints[i] / 2**shift, exactly"""
    pairs = [float(v).as_integer_ratio() for v in values]
    shift = max([d.bit_length() - 1 for _, d in pairs] + [0])
    return [n << (shift - (d.bit_length() - 1)) for n, d in pairs], shift


def exact_moments(nodes, ret, elites, mean=None, precision=64):
    """The elites' moments in exact rational arithmetic from the node values as the device holds them (nodes [n][npar]; rounded to
    float32 first for a 32-bit context). Dict of, per parameter j: sum, abs_sum (sum |p|), mean (sum / n), sq -- the sum of
    (p - m_j)^2 about `mean` (floats, e.g. the mean the device reported) or, without one, about the exact mean -- as Fractions; and
    ret_sum / ret_abs_sum of the elites' returns (None when one of them is not finite: their sum is then no rational number).
    Every double is an integer over a power of two, so the sums are integer sums (fractions.Fraction only carries the results)."""
    nodes = as_device(nodes, precision)
    elites = np.asarray(elites, dtype=np.int64).reshape(-1)
    n, npar = elites.size, nodes.shape[1]
    out = dict(n=n, sum=[], abs_sum=[], mean=[], sq=[])
    for j in range(npar):
        p, shift = _scaled(nodes[elites, j])
        s = Fraction(sum(p), 1 << shift)
        out["sum"].append(s)
        out["abs_sum"].append(Fraction(sum(abs(x) for x in p), 1 << shift))
        out["mean"].append(s / n if n else None)
        m = Fraction(float(np.asarray(mean).reshape(-1)[j])) if mean is not None else (s / n if n else Fraction(0))
        # (p_i / 2^shift - a / b)^2 = (p_i b - a 2^shift)^2 / (b 2^shift)^2
        a, b = m.numerator, m.denominator
        out["sq"].append(Fraction(sum((x * b - (a << shift)) ** 2 for x in p), (b << shift) ** 2))
    r = np.asarray(ret, dtype=np.float64)[elites]
    if np.all(np.isfinite(r)):
        q, shift = _scaled(r)
        out["ret_sum"], out["ret_abs_sum"] = Fraction(sum(q), 1 << shift), Fraction(sum(abs(x) for x in q), 1 << shift)
    else:
        out["ret_sum"] = out["ret_abs_sum"] = None
    return out


def trips(n):
    """m of the docstring: the trips of elite_reduce's stride loop"""
    return max(1, math.ceil(n / STRIDE))


def sum_bound(n, abs_sum):
    return (trips(n) + 8) * U * abs_sum


def mean_bound(n, abs_sum):
    return (trips(n) + 10) * U * abs_sum / n


def square_bound(n):
    """relative"""
    return (trips(n) + 16) * U


def ratio(got, exact, bound):
    """|got - exact| / bound, exactly (got a float, exact and bound rationals); 0 when both are zero"""
    d = abs(Fraction(float(got)) - exact)
    if d == 0:
        return 0.0
    return float(d / Fraction(bound)) if bound else math.inf


# ------------------------------------------------------------------------------------------------ the device's order of operations
def emulate_elite_reduce(values):
    """elite_reduce on the host: 256 strided partial sums in index order, then the halving tree -- the same fp64 additions in the
    same order (numpy adds elementwise, nothing is reassociated)"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    m = max(1, -(-v.size // STRIDE))
    pad = np.zeros(m * STRIDE)
    pad[:v.size] = v
    sm = np.zeros(STRIDE)
    for row in pad.reshape(m, STRIDE):
        sm = sm + row
    s = STRIDE // 2
    while s > 0:
        sm[:s] = sm[:s] + sm[s:2 * s]
        s //= 2
    return float(sm[0])


def emulate_moments(column, one_pass=False):
    """ce_update_kernel's moments of one parameter over the elites' values in rank order: (sum, mean, sum of squares, variance).
    one_pass: the formula the kernel must NOT use, E[x^2] - E[x]^2 from one sweep."""
    p = np.asarray(column, dtype=np.float64).reshape(-1)
    n = p.size
    total = emulate_elite_reduce(p)
    mean = total / n
    if one_pass:
        sq = emulate_elite_reduce(p * p) - n * mean * mean
    else:
        d = p - mean
        sq = emulate_elite_reduce(d * d)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = float(np.float64(sq) / np.float64(n - 1))
    return total, mean, sq, var


# ------------------------------------------------------------------------------------------------ injection
_HIP = None
_H2D = 1   # hipMemcpyHostToDevice


def _hip():
    """hipMemcpy / hipDeviceSynchronize of the HIP runtime libmjpcx.so itself is linked against (resolved through the loaded
    library's dependencies, so the pointers it hands out and these calls belong to one runtime)"""
    global _HIP
    if _HIP is None:
        from mujoco_mpc_amd import capi
        try:
            h = ctypes.CDLL(capi.LIB_PATH)
            h.hipMemcpy
        except (OSError, AttributeError):
            h = ctypes.CDLL("libamdhip64.so")
        h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        h.hipMemcpy.restype = ctypes.c_int
        h.hipDeviceSynchronize.argtypes = []
        h.hipDeviceSynchronize.restype = ctypes.c_int
        _HIP = h
    return _HIP


def inject(ctx, ret, fail=None):
    """Overwrite the returns (and failure flags) of ctx's last rollout on the device. The context's stream does not order behind the
    null stream, so the context is drained first and the device after the copies. Never writes outside the size the context
    reports; reads back through the context's own getter and asserts every bit."""
    ctx.sync()
    hip = _hip()
    payloads = [(0, np.ascontiguousarray(ret, dtype=np.float64))]
    if fail is not None:
        payloads.append((1, np.ascontiguousarray(fail, dtype=np.int32)))
    for which, host in payloads:
        ptr, size = ctx.device_buffer(which)
        assert ptr and host.nbytes == size, (which, host.nbytes, size)
        rc = hip.hipMemcpy(ctypes.c_void_p(ptr), host.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(size), _H2D)
        assert rc == 0, ("hipMemcpy", which, rc)
    rc = hip.hipDeviceSynchronize()
    assert rc == 0, ("hipDeviceSynchronize", rc)
    back, _ = ctx.returns()
    assert same_bits(back, payloads[0][1]), "the injected returns did not arrive"
    if fail is not None:
        assert np.array_equal(ctx.failure_raw, payloads[1][1]), "the injected failure flags did not arrive"
