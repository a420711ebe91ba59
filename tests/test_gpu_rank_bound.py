"""-m gpu: rank_bound_kernel (csrc/rank_bound.h) through mjpcx_rank_bound_batched, held to exact answers on returns and failure words
the test INJECTS (tests/selection_cases.py `inject`), as tests/test_gpu_selection.py does for the selection kernels.

A Cartpole rollout (H = 2) only sizes the buffers; the E x n returns and failure words are then overwritten. The reference is
numpy.partition over the qualifying returns of each environment -- failure word 0, finite, >= 0, with -0.0 counted as 0 -- compared bit for
bit; fewer than K qualifying gives +inf. n = 64, 128, 1024 and 4160: the kernel keeps no keys in LDS, it re-reads them from global memory
in each of its eight passes, so no size is special to it; 4160 = 4096 + 64 is past the 32 KB of keys that an LDS-resident variant would hold
and makes every thread of the 1024 loop more than four times with a ragged last trip."""
from functools import lru_cache

import numpy as np
import pytest

import selection_cases as sc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
H, P = 2, 3
TIMES = np.linspace(0.0, 0.02, P)
SIZES = (64, 128, 1024, 4160)
ENVS = (1, 3)
PARKED, PRUNED, FALLBACK = 0x10000000, 0x20000000, 0x40000000
INF_BITS = np.uint64(0x7FF0000000000000)


def ranks(n):
    return sorted({1, 2, 63, 64, 65, n})


@lru_cache(maxsize=None)
def _task():
    return load_task("Cartpole")


@pytest.fixture(scope="module", params=[(n, E) for n in SIZES for E in ENVS], ids=lambda p: f"n{p[0]}-E{p[1]}")
def fleet(request):
    """a context whose last rollout holds E x n candidates"""
    n, E = request.param
    t = _task()
    ctx = capi.Context(t.packed_model(), t.packed(), 0, 64)
    ctx.set_state([0.0, 0.1, 0.0, 0.0], 0.0, None)
    ctx.rollout_splines(H, capi.SPLINE_CUBIC, TIMES, sc.scaled_nodes(E * n, P * ctx.nu, seed=n).reshape(-1, P, ctx.nu))
    yield ctx, n, E
    ctx.close()


def reference(ret, fail, n, E, K):
    out = np.full(E, np.inf)
    for e in range(E):
        r, f = ret[e * n:(e + 1) * n], fail[e * n:(e + 1) * n]
        with np.errstate(invalid="ignore"):
            q = np.abs(r[(f == 0) & np.isfinite(r) & (r >= 0)])   # (abs: -0.0 counts as 0, and changes nothing else that qualifies)
        if len(q) >= K:
            out[e] = np.partition(q, K - 1)[K - 1]
    return out


def check(ctx, ret, fail, n, E, Ks, what):
    sc.inject(ctx, ret, fail)
    for K in Ks:
        got, want = ctx.rank_bound_batched(E, K), reference(ret, fail, n, E, K)
        assert sc.same_bits(got, want), (what, n, E, K, got, want)
    back, _ = ctx.returns()   # it touches no state: the returns and words stay as injected
    assert sc.same_bits(back, ret) and np.array_equal(ctx.failure_raw, fail), what


def test_distinct_returns(fleet):
    ctx, n, E = fleet
    ret = np.random.default_rng(n + E).uniform(0.5, 40.0, E * n)
    check(ctx, ret, np.zeros(E * n, np.int32), n, E, ranks(n), "distinct")
    # returns that differ only in their lowest bits, and over the whole exponent range: every digit of the radix select decides somewhere
    lo = (np.float64(3.0).view(np.uint64) + np.random.default_rng(1).permutation(E * n).astype(np.uint64)).view(np.float64)
    check(ctx, lo, np.zeros(E * n, np.int32), n, E, ranks(n), "low bits")
    wide = np.exp(np.random.default_rng(2).uniform(-700.0, 700.0, E * n))
    wide[::7] = 5e-324 * np.arange(1, len(wide[::7]) + 1)   # subnormals
    check(ctx, wide, np.zeros(E * n, np.int32), n, E, ranks(n), "wide")


def test_ties_across_the_kth_place(fleet):
    ctx, n, E = fleet
    rng = np.random.default_rng(3 * n + E)
    ret = rng.choice(np.array([0.25, 1.0, 1.0 + 2.0 ** -52, 7.5, 1e6]), E * n)   # long runs of equal returns: every K falls inside one
    check(ctx, ret, np.zeros(E * n, np.int32), n, E, ranks(n), "few values")
    for K in ranks(n):   # exactly three equal returns at places K - 1, K, K + 1 of the order (as far as they exist), at scattered indices
        r = rng.permutation(E * n).astype(np.float64) + 1.0
        for e in range(E):
            seg = r[e * n:(e + 1) * n]
            at = np.argsort(seg)[max(K - 2, 0):min(K + 1, n)]
            seg[at] = seg[at[0]]
        check(ctx, r, np.zeros(E * n, np.int32), n, E, [K], "tie at K")
    check(ctx, np.full(E * n, 2.5), np.zeros(E * n, np.int32), n, E, ranks(n), "all equal")


def test_values_that_do_not_qualify(fleet):
    ctx, n, E = fleet
    rng = np.random.default_rng(5 * n + E)
    ret = rng.uniform(0.5, 40.0, E * n)
    ret[rng.choice(E * n, E * n // 8, replace=False)] = np.inf
    ret[rng.choice(E * n, E * n // 8, replace=False)] = np.nan
    ret[rng.choice(E * n, E * n // 16, replace=False)] = sc.NEG_NAN
    ret[rng.choice(E * n, E * n // 16, replace=False)] = -np.inf
    ret[rng.choice(E * n, E * n // 16, replace=False)] = -1.5
    check(ctx, ret, np.zeros(E * n, np.int32), n, E, ranks(n), "inf, nan, negative")
    # failed, handed-on, parked and retired candidates: their returns (smaller than every completed one here) do not count
    ret = rng.uniform(0.5, 40.0, E * n)
    fail = np.zeros(E * n, np.int32)
    for word, share in ((1, 9), (FALLBACK | 2 | (5 << 8), 7), (PARKED | (3 << 8), 3), (PRUNED | (4 << 8), 5), (1 << 16, 11)):
        at = rng.choice(E * n, E * n // share, replace=False)
        fail[at] = word
        ret[at] = np.where(word == 1, sc.FAILED, rng.uniform(0.0, 0.4, len(at)))
    check(ctx, ret, fail, n, E, ranks(n), "failure words")


def test_signed_zeros(fleet):
    ctx, n, E = fleet
    rng = np.random.default_rng(7 * n + E)
    ret = rng.uniform(0.5, 40.0, E * n)
    ret[rng.choice(E * n, E * n // 4, replace=False)] = -0.0
    ret[rng.choice(E * n, E * n // 4, replace=False)] = 0.0
    ret[rng.choice(E * n, E * n // 8, replace=False)] = 5e-324
    check(ctx, ret, np.zeros(E * n, np.int32), n, E, ranks(n), "signed zeros")
    only = np.full(E * n, -0.0)
    assert (ctx_bits(ctx, only, n, E, 1) == 0).all()   # +0.0, not the bits of -0.0


def ctx_bits(ctx, ret, n, E, K):
    sc.inject(ctx, ret, np.zeros(E * n, np.int32))
    return sc.bits(ctx.rank_bound_batched(E, K))


def test_fewer_than_k_qualify(fleet):
    ctx, n, E = fleet
    rng = np.random.default_rng(11 * n + E)
    ret = rng.uniform(0.5, 40.0, E * n)
    fail = np.ones(E * n, np.int32)
    keep = [3, 1, 0][:E]   # qualifying candidates per environment
    for e, m in enumerate(keep):
        fail[e * n + rng.choice(n, m, replace=False)] = 0
    sc.inject(ctx, ret, fail)
    for K in (1, 2, 3, 4, n):
        got, want = ctx.rank_bound_batched(E, K), reference(ret, fail, n, E, K)
        assert sc.same_bits(got, want), (K, got, want)
        for e, m in enumerate(keep):
            assert (sc.bits(got)[e] == INF_BITS) == (m < K), (K, e)


def test_the_kth_at_every_lane_of_a_wavefront(fleet):
    """the K-th smallest return sits at index p of its environment, for every p of the first two wavefronts' lanes, the last lanes of the
    environment and the places either side of the 1024-thread stride"""
    ctx, n, E = fleet
    rng = np.random.default_rng(13 * n + E)
    places = sorted({p for p in list(range(130)) + [1022, 1023, 1024, 1025, 2047, 2048, n - 65, n - 64, n - 2, n - 1] if 0 <= p < n})
    zeros = np.zeros(E * n, np.int32)
    for K in (2, 64) if n > 64 else (2, 63):
        for p in places:
            ret = rng.permutation(E * n).astype(np.float64) + 1.0
            for e in range(E):
                seg = ret[e * n:(e + 1) * n]
                at = np.argsort(seg)[K - 1]
                seg[at], seg[p] = seg[p], seg[at]
                assert np.argsort(seg)[K - 1] == p
            sc.inject(ctx, ret, zeros)
            got = ctx.rank_bound_batched(E, K)
            assert sc.same_bits(got, ret.reshape(E, n)[:, p]), (K, p, got)


def test_arguments(fleet):
    ctx, n, E = fleet
    for bad in ((0, 1), (E, 0), (E, -3), (7, 1)):   # no environments, rank < 1, a split that does not divide the batch
        with pytest.raises(capi.MjpcxError) as err:
            ctx.rank_bound_batched(*bad)
        assert err.value.code == -1, bad   # MJPCX_EINVAL
