"""-m gpu: rank mode of a plain pruned launch on rollout_quad_kernel (mjpcx_set_prune_rank with mjpcx_set_pruning + mjpcx_set_park_hint).
The bound word stays at +inf through the main launch, rank_bound_kernel writes T = the K-th smallest completed return into it, the
settling pass retires the parked candidates above T and the resume launch continues the others, pruned against T. What a Cross-Entropy
plan step reads -- mjpcx_topk(K), mjpcx_elite_moments of those candidates, mjpcx_best -- and every candidate not marked pruned equal the
unpruned launch bit for bit, whatever the hint. The word does not move while candidates run, so which candidates are parked, T, and what
is retired where are the numpy function of the unpruned costs that tests/test_quad_rank_emulator.py holds the emulator to
(tests/quademu/rank.py `expected`); test_device_equals_the_emulator runs the emulator beside the device.

The shapes and the context of tests/test_gpu_quad_park.py: the bench's initial condition and noise, N = 128, H = 30, fp64, at 4 and at 16
candidates per wavefront, MJPCX_QUAD_MIN_N set before the context is created; K = 13 (a planner with 12 elites and the nominal)."""
import os

import numpy as np
import pytest

from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task
from tests.quademu import rank

pytestmark = pytest.mark.gpu
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
N, H, P, K = 128, 30, 3, 13
TIMES = np.arange(P) * ((H - 1) * 0.01 / P)
NOMINAL = np.zeros((P, 12))
PARKED, PRUNED, FALLBACK = 0x10000000, 0x20000000, 0x40000000
BUFFERS = ("states", "actions", "times", "residual", "costs", "trace")
HINTS = ("inf", "kth", "1.05 kth", "0.5 kth", "second best", "zero")
ESTATE = -5


def hint_value(name, ret):
    s = np.sort(ret)
    return {"inf": np.inf, "kth": s[K - 1], "1.05 kth": 1.05 * s[K - 1], "0.5 kth": 0.5 * s[K - 1], "second best": s[1], "zero": 0.0}[name]


def noise():
    return capi.make_noise_spec(seed=0, iteration=1, mode=capi.NOISE_SAMPLING, std0=0.04)


@pytest.fixture(scope="module")
def quad():
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    return t


def context(t, cpw=None):
    env = {"MJPCX_QUAD_MIN_N": "1"}
    if cpw is not None and cpw != 4:   # (4 is what the library picks for 128 candidates)
        env["MJPCX_QUAD_CPW"] = str(cpw)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = capi.Context(t.packed_model(), t.packed(), 0, 64)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert "rollout_quad_kernel" in ctx.kernel_name
    ctx.set_state(np.concatenate([t.model.keyframes["home"]["qpos"], np.zeros(18)]), 0.0, MOCAP)
    return ctx


def snapshot(ctx):
    ret, _ = ctx.returns()
    out = dict(total_return=ret.copy(), failure=ctx.failure_raw.copy())
    trs = [ctx.fetch_trajectory(c) for c in range(ctx.N)]
    for k in BUFFERS:
        out[k] = np.stack([getattr(tr, k) for tr in trs])
    return out


def elite_reads(ctx, idx):
    """what the Cross-Entropy update reads of the elites: the sums of their parameters, of the squares about a mean, and of their returns"""
    s, sr = ctx.elite_moments(idx)
    q, _ = ctx.elite_moments(idx, mean=s / len(idx))
    return s, sr, q


@pytest.fixture(scope="module")
def full(quad):
    """the unpruned launch: every buffer of every candidate, the candidates' nodes, and what the plan step reads"""
    ctx = context(quad)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    out = snapshot(ctx)
    out["best"] = ctx.best(0)
    out["topk"] = ctx.topk(K)
    out["topk1"] = ctx.topk(K + 1)
    out["elite"] = elite_reads(ctx, out["topk"][0])
    out["stats"] = ctx.quad_stats()
    out["nodes"] = np.stack([ctx.fetch_spline(c) for c in range(N)])
    ctx.close()
    assert not out["failure"].any() and out["costs"].min() > 0 and out["stats"]["handed_on"] == 0
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def same_best(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("cpw", [4, 16])
def test_what_the_plan_step_reads_does_not_depend_on_the_hint(quad, full, cpw):
    ctx = context(quad, cpw=cpw)
    ctx.set_pruning(True)
    ctx.set_prune_rank(K)
    for name in HINTS:
        hint = hint_value(name, full["total_return"])
        want = rank.expected(full["costs"], H, K, hint)
        ctx.set_park_hint(hint)
        ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
        # the plan step's reads
        idx, ret = ctx.topk(K)
        assert np.array_equal(idx, full["topk"][0]) and np.array_equal(ret, full["topk"][1]), name
        for got, ref in zip(elite_reads(ctx, idx), full["elite"]):
            assert np.array_equal(got, ref), name
        assert same_best(ctx.best(0), full["best"]), name
        for k in (1, 2, K - 1):
            i2, r2 = ctx.topk(k)
            assert np.array_equal(i2, idx[:k]) and np.array_equal(r2, ret[:k]), (name, k)
        with pytest.raises(capi.MjpcxError) as e:
            ctx.topk(K + 1)
        assert e.value.code == ESTATE, name
        with pytest.raises(capi.MjpcxError) as e:
            ctx.elite_moments(full["topk1"][0])   # K + 1 candidates
        assert e.value.code == ESTATE, name
        # the candidates: no parked marker is left, every one not marked pruned is the unpruned launch's in all six buffers, every retired
        # one sits at a partial return strictly above T, at the step numpy computes from the unpruned costs
        run = snapshot(ctx)
        st, pk = ctx.prune_stats(), ctx.park_stats()
        assert ((run["failure"] & (PARKED | FALLBACK)) == 0).all(), name
        final = np.where(want["retired"], want["park"], want["late"])
        gone = final >= 0
        assert np.array_equal(run["failure"], np.where(gone, PRUNED | (final << 8), 0)), name
        for k in BUFFERS + ("total_return",):
            assert np.array_equal(run[k][~gone], full[k][~gone]), (name, k)
        assert not gone[idx].any() and not gone[0]
        t = final[gone]
        assert np.array_equal(run["total_return"][gone], want["partial"][gone, t]) and (run["total_return"][gone] > want["T"]).all(), name
        assert (full["total_return"][gone] > want["T"]).all() and want["T"] >= ret[K - 1]
        for c, tc in zip(np.nonzero(gone)[0], t):
            for k in BUFFERS:
                assert np.array_equal(run[k][c, :tc + 1], full[k][c, :tc + 1]), (name, k, c)
        # the counts add up
        assert (pk["parked"], pk["settled_retired"], pk["resumed"]) == ((want["park"] >= 0).sum(), want["retired"].sum(), want["resumed"].sum()), name
        assert pk["parked"] == pk["settled_retired"] + pk["resumed"]
        assert st["retired"] == gone.sum() and st["retire_step_sum"] == t.sum() and not st["negative_cost"], name
        ridx, rstep = ctx.park_resumed()
        assert np.array_equal(ridx, np.nonzero(want["resumed"])[0]) and np.array_equal(rstep, want["park"][want["resumed"]]), name
        assert ctx.quad_stats() == full["stats"]
        if name == "inf":
            assert pk["parked"] == 0
        # what the unpruned costs of this batch give (its returns lie within 10 % of each other, so 1.05 x the K-th parks nothing here)
        if name == "kth":           # at least K complete and what the hint parks is retired
            assert want["completed"] >= K and pk["parked"] > 0 and pk["settled_retired"] == pk["parked"]
        if name == "second best":   # K complete all the same; of the parked some are retired, some resumed, and some of those retired later against T
            assert np.isfinite(want["T"]) and pk["settled_retired"] > 0 and pk["resumed"] > 0 and (want["late"] >= 0).any() and pk["resume_ms"] > 0
        if name in ("0.5 kth", "zero"):   # only the nominal completes: T = +inf, everything parked is resumed and nothing is retired
            assert want["T"] == np.inf and pk["parked"] == N - 1 and pk["resumed"] == N - 1 and not gone.any() and pk["resume_ms"] > 0
    ctx.close()


@pytest.mark.parametrize("name", HINTS)
def test_device_equals_the_emulator(quad, full, name):
    """the same candidates (the device's nodes) through the emulator's four stages: the parked, retired and resumed sets, the park steps
    and the failure words are the device's"""
    hint = hint_value(name, full["total_return"])
    state = np.concatenate([quad.model.keyframes["home"]["qpos"], np.zeros(18)])
    emu = rank.rollout(quad.packed_model(), quad.packed(), state, 0.0, MOCAP, N, H, P, capi.SPLINE_ZERO, TIMES, full["nodes"], rank=K,
                       nominal_candidate=0, hint=hint)
    assert emu["bound_main"] == np.inf
    ctx = context(quad, cpw=16)
    ctx.set_pruning(True)
    ctx.set_prune_rank(K)
    ctx.set_park_hint(hint)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    pk = ctx.park_stats()
    assert (pk["parked"], pk["settled_retired"], pk["resumed"]) == (emu["parked"], emu["settled_retired"], emu["resumed_count"])
    ridx, rstep = ctx.park_resumed()
    assert np.array_equal(ridx, np.nonzero(emu["resumed"])[0]) and np.array_equal(rstep, emu["park_step"][emu["resumed"]])
    ret, _ = ctx.returns()
    assert np.array_equal(ctx.failure_raw, emu["failure"])
    # (against the emulator, whose host compiler rounds differently from the device's fused arithmetic, the flags and steps are exact and
    # the numbers agree closely)
    assert np.allclose(ret, emu["total_return"], rtol=1e-9, atol=0)
    ctx.close()


def test_rank_one_behaves_as_before(quad, full):
    """the default rank, and rank 1 set after a higher one: a pruned launch answers only for the argmin"""
    ctx = context(quad)
    ctx.set_pruning(True)
    for first in (None, K):
        if first:
            ctx.set_prune_rank(first)
            ctx.set_prune_rank(1)
        ctx.set_park_hint(0.5 * full["best"][1])
        ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
        assert same_best(ctx.best(0), full["best"])
        assert ctx.topk(1)[0][0] == full["best"][0]
        assert ctx.prune_stats()["retired"] > 0   # the bound fell with the completions: the argmin's rule retires
        for call in (lambda: ctx.topk(2), lambda: ctx.elite_moments(full["topk"][0][:1])):
            with pytest.raises(capi.MjpcxError) as e:
                call()
            assert e.value.code == ESTATE
    ctx.close()


def test_arguments(quad):
    ctx = context(quad)
    for bad in (0, -2):
        with pytest.raises(capi.MjpcxError) as e:
            ctx.set_prune_rank(bad)
        assert e.value.code == -1   # MJPCX_EINVAL
    # nobody can vouch for a K-th return: a finite initial bound and rank mode exclude each other, whichever comes second
    ctx.set_prune_rank(K)
    with pytest.raises(capi.MjpcxError) as e:
        ctx.set_pruning(True, 3.0)
    assert e.value.code == -1
    ctx.set_prune_rank(1)
    ctx.set_pruning(True, 3.0)
    with pytest.raises(capi.MjpcxError) as e:
        ctx.set_prune_rank(K)
    assert e.value.code == -1
    ctx.close()
