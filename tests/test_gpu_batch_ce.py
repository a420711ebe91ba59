"""-m gpu: Cross-Entropy for several environments in one launch (mjpcx_rollout_noise_batched_ce, mjpcx_ce_update_batched,
GpuBatchCrossEntropyPlanner) on the rollout kernels.

Rollout: a batched CE call with three DIFFERENT variance rows is compared bit for bit with three plain CE calls on the same context
(seed s + e, variance row e) and, per environment, with the oracle at the tolerance of the kernel family listed at the top of
tests/test_gpu_batch.py (the cases, their states and their tolerances are that file's). Update: mjpcx_ce_update_batched against the
same context's sequential path (plain rollout, mjpcx_topk, mjpcx_elite_moments twice, the host's divisions). The elites' sums go
through one __device__ routine in both kernels (elite_reduce, mjpcx.hip), so mean, variance and the mean return are asserted bit for
bit as well as at the tolerances tests/test_cross_entropy.py:95-96 uses."""
import os

import numpy as np
import pytest

import step_bank
from batch_ce_oracle_backend import BatchCeOracleContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchCrossEntropyPlanner
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle
from test_gpu_batch import E, FIELDS, H, HANDED_ON, P, SEED, _states, err, everything, make_case

pytestmark = pytest.mark.gpu
EXPLORE = 6   # the first candidates of every environment keep the std0 floor (explore_fraction_)


class CeCase:
    """a Case of tests/test_gpu_batch.py with cross-entropy noise: three different variance rows, the nominal as the last candidate"""

    def __init__(self, name):
        self.case = c = make_case(name)
        m = c.task.model
        lo, hi = np.asarray(m.arrays["actuator_ctrlrange"], float).reshape(-1, 2).T
        self.scale = 0.5 * (hi - lo) * c.std                      # the sampling cases' sigma, per actuator
        rng = np.random.default_rng(11)
        # row e: its own level (1, 1.5, 2 x the scale) and its own pattern over the parameters
        self.var = np.stack([(self.scale[None, :] * (1 + 0.5 * e) * rng.uniform(0.6, 1.4, (P, m.nu))) ** 2 for e in range(E)])
        self.n = c.n

    def noise(self, e=0, row=None):
        return capi.make_noise_spec(seed=SEED + e, iteration=2, mode=capi.NOISE_CROSS_ENTROPY, nominal_candidate=self.n - 1,
                                    explore_count=EXPLORE, std0=float(self.scale.mean()), std1=0.2 * float(self.scale.mean()),
                                    param_variance=row)

    def set_states(self, ctx, envs):
        c = self.case
        ctx.set_states(np.stack([c.states[e].state for e in envs]), [c.states[e].time for e in envs],
                       np.stack([c.mocap(e) for e in envs]) if c.task.model.nmocap else None)
        c.set_shared_residual(ctx)

    def run_batched(self, ctx, envs, var=None):
        var = self.var if var is None else var
        self.set_states(ctx, envs)
        ctx.rollout_noise_batched_ce(self.n, H, capi.SPLINE_CUBIC, self.case.times[envs], self.case.nominal[envs], var[envs],
                                     self.noise(envs[0]), num_envs=len(envs))

    def run_single(self, ctx, e, var=None):
        c, s = self.case, self.case.states[e]
        c.set_shared_residual(ctx)
        ctx.set_state(s.state, s.time, c.mocap(e) if c.task.model.nmocap else None)
        ctx.rollout_noise(self.n, H, capi.SPLINE_CUBIC, c.times[e], c.nominal[e], self.noise(e, (self.var if var is None else var)[e]))

    def oracle(self, e):
        c, s = self.case, self.case.states[e]
        nodes = pyoracle.noise_candidates(c.pm, self.noise(e, self.var[e]), P, c.nominal[e], np.arange(self.n))
        return pyoracle.rollout_batch(c.pm, c.packed(e), s.state, s.time, c.mocap(e), self.n, H, P, capi.SPLINE_CUBIC, c.times[e], nodes,
                                      num_threads=16)

    def handed_on_mask(self):
        """which candidates of the batched run the quad / limb kernel handed on: the same launch with the hand-on pass switched off"""
        if not ("quad" in self.case.name or "limb" in self.case.name):
            return None
        ctx = self.case.make_context({"MJPCX_QUAD_NO_FALLBACK": "1", "MJPCX_LIMB_NO_FALLBACK": "1"})
        self.run_batched(ctx, list(range(E)))
        ctx.returns()
        mask = (ctx.failure_raw & HANDED_ON) != 0
        ctx.close()
        return mask


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("name", ["cartpole64", "particle32", "quad", "tree_a1", "limb32", "wave"])
def test_batched_ce_rollout_equals_sequential_and_the_oracle(name):
    cc = CeCase(name)
    case, n = cc.case, cc.n
    assert len({tuple(r.ravel()) for r in cc.var}) == E
    handed = cc.handed_on_mask()
    if name == "quad":   # the smallest cap that splits the batch, as tests/test_gpu_batch.py does for the sampling noise
        for cap in (2, 3, 4, 5, 6, 8):
            case.env["MJPCX_QUAD_CON_CAP"] = str(cap)
            handed = cc.handed_on_mask()
            if 0 < handed.sum() < E * n:
                break
        assert 0 < handed.sum() < E * n, int(handed.sum())   # both the kernel's own candidates and its hand-on are in the comparison
    ctx = case.make_context()
    cc.run_batched(ctx, list(range(E)))
    got = everything(ctx)
    assert ctx.N == E * n
    spline1 = ctx.fetch_spline(n + EXPLORE)       # environment 1, a candidate whose noise is scaled by the variance row
    # ---- bit for bit: E plain CE calls with seeds s + e and variance row e on the same context
    for e in range(E):
        cc.run_single(ctx, e)
        one = everything(ctx)
        for k in ("total_return", "failure") + FIELDS:
            assert same(got[k][e * n:(e + 1) * n], one[k]), (name, e, k)
        # the nominal rides along un-noised as the environment's last candidate
        assert np.array_equal(ctx.fetch_spline(n - 1), case.nominal[e].astype(np.float32 if case.precision == 32 else float))
    # the variance rows matter: environment 1 with environment 0's row is another rollout
    swapped = cc.var.copy()
    swapped[1] = cc.var[0]
    cc.run_single(ctx, 1, swapped)
    assert not same(ctx.fetch_spline(EXPLORE), spline1)
    cc.run_single(ctx, 1)
    assert same(ctx.fetch_spline(EXPLORE), spline1)
    # ---- three EQUAL rows: the shared-variance call with that row, bit for bit
    equal = np.stack([cc.var[1]] * E)
    cc.run_batched(ctx, list(range(E)), equal)
    rows = everything(ctx)
    cc.set_states(ctx, list(range(E)))
    ctx.rollout_noise_batched(n, H, capi.SPLINE_CUBIC, case.times, case.nominal, cc.noise(0, cc.var[1]), num_envs=E)
    shared = everything(ctx)
    for k in ("total_return", "failure") + FIELDS:
        assert same(rows[k], shared[k]), (name, "equal rows", k)
    ctx.close()
    # ---- the oracle, per environment, every candidate
    worst = {}
    for e in range(E):
        ref = cc.oracle(e)
        sl = slice(e * n, (e + 1) * n)
        assert np.array_equal(got["failure"][sl] != 0, ref["failure"] != 0), (name, e)
        assert not ref["failure"].any(), (name, e)   # (the oracle completes these rollouts: checked on the CPU)
        tol = np.where(handed[sl], case.tol_handed, case.tol) if handed is not None else np.full(n, case.tol)
        for k in ("total_return",) + (() if case.returns_only else FIELDS):
            for c in range(n):
                d = err(got[k][sl][c], ref[k][c])
                worst[k] = max(worst.get(k, 0.0), d / tol[c])
                assert d <= tol[c], (name, e, c, k, d, float(tol[c]))
    print(f"{name}: worst error / tolerance by buffer {worst}; handed on {None if handed is None else int(handed.sum())} of {E * n}")


def sequential_update(ctx, n_elite, skip):
    """the single planner's path on the context's last PLAIN rollout: topk(n_elite + 1) without the nominal, elite_moments twice"""
    idx, ret = ctx.topk(min(n_elite + 1, ctx.N))
    keep = idx != skip
    idx, ret = idx[keep][:n_elite], ret[keep][:n_elite]
    s, sret = ctx.elite_moments(idx)
    mean = s / n_elite
    sq, _ = ctx.elite_moments(idx, mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        return idx, ret, mean, sq / (n_elite - 1), sret / n_elite


def check_update(got, want, e, what):
    idx, ret, mean, var, avg = (x[e] for x in got)
    widx, wret, wmean, wvar, wavg = want
    assert np.array_equal(idx, widx) and same(ret, wret), (what, e)
    assert np.allclose(mean, wmean, rtol=0, atol=1e-12), (what, e)
    finite = np.isfinite(wvar)
    assert np.array_equal(np.isfinite(var), finite), (what, e)
    assert np.allclose(var[finite], wvar[finite], rtol=1e-9, atol=1e-15), (what, e)
    assert abs(avg - wavg) < 1e-10, (what, e)
    # one reduction routine on both sides: the same bits
    assert same(mean, wmean) and same(var, wvar) and avg == wavg, (what, e, float(np.max(np.abs(mean - wmean))))


@pytest.mark.parametrize("name", ["cartpole64", "quad"])
def test_segmented_ce_update(name):
    cc = CeCase(name)
    case, n = cc.case, cc.n
    ctx = case.make_context()
    skip = n - 1
    for n_elite in (6, 1, n - 1):
        cc.run_batched(ctx, list(range(E)))
        ret, _ = ctx.returns()
        got = ctx.ce_update_batched(E, n_elite, skip)
        again = ctx.ce_update_batched(E, n_elite, skip)
        for a, b in zip(got, again):
            assert same(a, b), (name, n_elite, "a second call gives other bits")
        for e in range(E):
            assert skip not in got[0][e] and same(got[1][e], ret[e * n:(e + 1) * n][got[0][e]])
        if n_elite == 1:
            assert not np.isfinite(got[3]).any()
        if n_elite == n - 1:
            assert all(sorted(got[0][e].tolist()) == list(range(n - 1)) for e in range(E))
        for e in range(E):
            cc.run_single(ctx, e)
            check_update(got, sequential_update(ctx, n_elite, skip), e, (name, n_elite))
    # without a skip the best candidate of all is the first elite
    cc.run_batched(ctx, list(range(E)))
    ret, _ = ctx.returns()
    idx = ctx.ce_update_batched(E, 3, -1)[0]
    assert [int(i) for i in idx[:, 0]] == [int(np.argmin(ret[e * n:(e + 1) * n])) for e in range(E)]
    # ---- a constructed tie (as tests/test_gpu_batch.py::test_segmented_best): every candidate of an environment is the same spline
    # from the same state -> equal returns, the elites are the lowest indices; after rollout_splines_batched
    s = case.states[0]
    nu = case.task.model.nu
    ctx.set_states(np.stack([s.state] * E), [s.time] * E, np.stack([case.mocap(0)] * E) if case.task.model.nmocap else None)
    values = np.broadcast_to(case.nominal[0], (E, n, P, nu)).copy()
    values[1, :5] *= 0.5      # environment 1: candidates 0..4 differ from the rest
    ctx.rollout_splines_batched(H, capi.SPLINE_CUBIC, np.stack([case.times[0]] * E), values, num_envs=E, n_per_env=n)
    ret, _ = ctx.returns()
    got = ctx.ce_update_batched(E, 6, 0)          # candidate 0 is the one to skip here
    for e in (0, 2):
        assert len(set(ret[e * n:(e + 1) * n].tolist())) == 1               # the tie is real
        assert got[0][e].tolist() == [1, 2, 3, 4, 5, 6]
        assert np.all(got[3][e] < 1e-28)                                      # equal parameters: zero up to the rounding of sum / n_elite
    assert 0 not in got[0][1]
    for e in range(E):
        ctx.set_state(s.state, s.time, case.mocap(0) if case.task.model.nmocap else None)
        ctx.rollout_splines(H, capi.SPLINE_CUBIC, case.times[0], values[e])
        check_update(got, sequential_update(ctx, 6, 0), e, (name, "tie"))
    ctx.close()


def test_ce_update_of_16384_candidates():
    """one environment of 16384 candidates (the keys do not fit the LDS: the global scratch path) against topk + elite_moments"""
    task = load_task("Cartpole")
    ctx = capi.Context(task.packed_model(), task.packed(), 0, 64)
    n, h, p = 16384, 8, 6
    state, times, nominal = np.array([0.0, 0.2, 0.0, 0.0]), np.linspace(0, 0.07, p), np.zeros((p, 1))
    var = np.full((1, p, 1), 0.3 ** 2)
    ns = capi.make_noise_spec(seed=2, mode=capi.NOISE_CROSS_ENTROPY, nominal_candidate=n - 1, explore_count=100, std0=0.5, std1=0.05)
    ctx.set_states(state[None], [0.0])
    ctx.rollout_noise_batched_ce(n, h, capi.SPLINE_LINEAR, times[None], nominal[None], var, ns, num_envs=1)
    ret, _ = ctx.returns()
    for n_elite in (1638, n - 1):
        got = ctx.ce_update_batched(1, n_elite, n - 1)
        order = np.lexsort((np.arange(n), ret))
        order = order[order != n - 1][:n_elite]
        assert np.array_equal(got[0][0], order) and same(got[1][0], ret[order])
        ctx.set_state(state, 0.0)
        ns1 = capi.make_noise_spec(seed=2, mode=capi.NOISE_CROSS_ENTROPY, nominal_candidate=n - 1, explore_count=100, std0=0.5, std1=0.05,
                                   param_variance=var[0])
        ctx.rollout_noise(n, h, capi.SPLINE_LINEAR, times, nominal, ns1)
        assert same(ctx.returns()[0], ret)
        check_update(got, sequential_update(ctx, n_elite, n - 1), 0, ("16384", n_elite))
        ctx.set_states(state[None], [0.0])
        ctx.rollout_noise_batched_ce(n, h, capi.SPLINE_LINEAR, times[None], nominal[None], var, ns, num_envs=1)
    ctx.close()


PLANNER_SEED, N_NOISED, N_ELITE = 9, 63, 6


@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_batch_ce_planner_on_the_device_against_the_oracle_backend(name):
    """GpuBatchCrossEntropyPlanner, E = 3, 63 noised candidates + the nominal, n_elite_ = 6, explore_fraction_ = 0.1, three plan steps,
    seed 9 (the bank states are the ones the smallest rank gaps were checked on: 1.0e-4 on the Quadruped with this seed). The device and
    the oracle backend pick the same elites wherever the oracle's own ranking is decided -- which is asserted for every environment and
    step, not assumed -- and end every step with policies within 1e-9 (1 + |x|), variances within rtol 1e-9 / atol 1e-15 and
    `improvement` within the kernel family's return tolerance."""
    if name == "Cartpole":
        task, bank_states, horizon, rtol = load_task("Cartpole"), step_bank.lane_bank("Cartpole").states[:E], 30, 1e-9
    else:
        b = step_bank.a1_bank()
        task, bank_states, horizon, rtol = b.task, b.states[:E], 20, 1e-6
        task.residual_int, task.residual_real = list(bank_states[0].residual_int), list(bank_states[0].residual_real)
    old = os.environ.get("MJPCX_QUAD_MIN_N")
    os.environ["MJPCX_QUAD_MIN_N"] = "0"
    try:
        dev = GpuBatchCrossEntropyPlanner(E, seed=PLANNER_SEED)
        ref = GpuBatchCrossEntropyPlanner(E, seed=PLANNER_SEED, backend_factory=lambda t: BatchCeOracleContext(t, threads=16))
        for p in (dev, ref):
            p.initialize(task.model, task)
            p.num_trajectory_, p.n_elite_, p.explore_fraction_ = N_NOISED, N_ELITE, 0.1
            if name == "QuadrupedFlat":
                p.std_initial_, p.std_min_ = 0.05, 0.01
            p.allocate()
            p.reset(horizon)
    finally:
        if old is None:
            os.environ.pop("MJPCX_QUAD_MIN_N", None)
        else:
            os.environ["MJPCX_QUAD_MIN_N"] = old
    states = _states(task, bank_states)
    nq = task.model.nq
    npar = ref.num_parameters()
    for step in range(3):
        for p in (dev, ref):
            p.set_states(states)
            p.optimize_policy(horizon)
        # the condition: the oracle's ranking is decided at the elite boundary, and no oracle rollout failed
        ret, fail = ref.ctx.returns()
        assert not fail.any(), step
        for e in range(E):
            r = np.sort(ret[e * (N_NOISED + 1):(e + 1) * (N_NOISED + 1) - 1])      # the noised candidates, without the nominal
            gap = (r[N_ELITE] - r[N_ELITE - 1]) / (1 + abs(r[N_ELITE - 1]))
            print(f"{name} step {step} env {e}: gap between ranks {N_ELITE} and {N_ELITE + 1} = {gap:.3e}")
            assert gap > 10 * rtol, (step, e, gap)
        for e in range(E):
            d, o = dev.envs[e], ref.envs[e]
            assert d.trajectory_order == o.trajectory_order, (step, e, d.trajectory_order, o.trajectory_order)
            assert err(d.policy.plan.values(), o.policy.plan.values()) <= 1e-9, (step, e)
            assert err(d.policy.plan.times(), o.policy.plan.times()) <= 1e-9, (step, e)
            assert np.allclose(d.variance[:npar], o.variance[:npar], rtol=1e-9, atol=1e-15), (step, e)
            assert np.all(d.variance[npar:] == 0)
            best = float(np.min(ret[e * (N_NOISED + 1):(e + 1) * (N_NOISED + 1) - 1]))
            assert abs(d.improvement - o.improvement) <= (1e-9 if name == "Cartpole" else 1e-6 * (1 + abs(best))), (step, e)
        for e in range(E):   # every environment moves two steps along the oracle side's nominal trajectory
            tr = ref.best_trajectory(e)
            mp = states[e].mocap.reshape(-1, 7)
            states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None, mocap_quat=mp[:, 3:] if len(mp) else None,
                          time=float(tr.times[2]))
    tb = dev.best_trajectory(1)
    assert err(tb.states, ref.best_trajectory(1).states) <= 1e-6
    dev.ctx.close()


def test_validation():
    cc = CeCase("cartpole64")
    case, n = cc.case, cc.n
    ctx = case.make_context()
    ns = cc.noise()

    def refused(fn, code=-1):
        with pytest.raises(capi.MjpcxError) as ei:
            fn()
        assert ei.value.code == code, ei.value
        return str(ei.value)

    every = list(range(E))
    # no set_states yet
    assert "set_states" in refused(lambda: ctx.rollout_noise_batched_ce(n, H, 2, case.times, case.nominal, cc.var, ns, num_envs=E))
    cc.set_states(ctx, every)
    assert "multiple of 64" in refused(lambda: ctx.rollout_noise_batched_ce(96, H, 2, case.times, case.nominal, cc.var, ns, num_envs=E))
    sampling = capi.make_noise_spec(seed=SEED, iteration=2, mode=capi.NOISE_SAMPLING, std0=0.1)
    assert "CROSS_ENTROPY" in refused(lambda: ctx.rollout_noise_batched_ce(n, H, 2, case.times, case.nominal, cc.var, sampling, num_envs=E))
    # the update after a plain rollout, and with n_elite outside 1 .. n - 1
    cc.run_single(ctx, 0)
    assert "not a batched one" in refused(lambda: ctx.ce_update_batched(E, 6, n - 1))
    cc.run_batched(ctx, every)
    refused(lambda: ctx.ce_update_batched(E, 0, n - 1))
    refused(lambda: ctx.ce_update_batched(E, n, n - 1))
    refused(lambda: ctx.ce_update_batched(2, 6, n - 1))      # another fleet size than the rollout's
    assert ctx.ce_update_batched(E, n, -1)[0].shape == (E, n)  # without a skip all n candidates may be elites
    # the context still serves a plain call, and its result is the one of a fresh context
    cc.run_single(ctx, 0)
    ret, fail = ctx.returns()
    fresh = case.make_context()
    cc.run_single(fresh, 0)
    ret2, fail2 = fresh.returns()
    assert np.array_equal(ret, ret2) and np.array_equal(fail, fail2)
    ctx.close(); fresh.close()
