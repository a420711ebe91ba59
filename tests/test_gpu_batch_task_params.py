"""-m gpu: per-environment task weights and parameters (mjpcx_set_task_params_batched) on every kernel family.

Every fleet here starts its environments from the SAME state, clock and mocap pose with DIFFERENT rows (tests/task_rows.py: weights,
norm parameters, residual parameters, risk 0 / positive / negative), and every case first rolls ONE spline out for all of them and
asserts that the environments' returns differ from one another: a staging that ignored the rows would not get that far. One model cannot
show it: tests/models/capsules_small.xml's only residual is a constant user sensor of value 0, so its cost is 0 under any rows. That case
keeps the bit comparison, and the A1 on the same wavefront-per-candidate kernel (MJPCX_NO_LDS_MODEL=1) is added beside it, where the
returns do differ.

   a batched call with rows <-> E plain calls, each after set_state + set_task_params(row e), on the same context: np.array_equal on
       the returns, the failure flags and every Trajectory buffer of every global candidate
   gradient_step_batched / ilqg_step_batched after a batched rollout with rows <-> the sequential chain per environment after the plain
       set_task_params(row e), as tests/test_gpu_batch_gradient.py and tests/test_gpu_batch_ilqg_step.py build it: every output
       np.array_equal with every step evaluated; derivative_skip 3: 1e-12 (1 + |x|) for the Gradient chain and equality for the iLQG
       chain, the bounds of those files
   a field given as None is the context's; all four None gives the bits of a context that never had rows; a plain call between two
       batched ones is unaffected and does not affect them; permuting the rows permutes the outputs; two calls give the same bits; another E
       is MJPCX_EINVAL naming the call; set_states with another E drops the rows
   one fleet per family against the oracle, at the tolerances of tests/test_gpu_batch.py: lane fp64 1e-9 (1 + |x|), quad kernel 1e-9,
       tree and wave kernels 1e-6, fp32 returns 2e-3
   the four fleet planners with set_tasks on the device <-> E single planners on the device, each created on its own task: equal"""

import numpy as np
import pytest

import step_bank
import task_rows
import test_gpu_batch_gradient as tg
import test_gpu_batch_ilqg as ti
import test_gpu_batch_ilqg_step as ts
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import (GpuBatchCrossEntropyPlanner, GpuBatchGradientPlanner, GpuBatchILQGPlanner, GpuBatchSamplingPlanner,
                                     GpuCrossEntropyPlanner, GpuGradientPlanner, GpuILQGPlanner, GpuSamplingPlanner, State, derivative_steps)
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle
from test_gpu_batch import context, err, everything

pytestmark = pytest.mark.gpu
FIELDS = ("states", "actions", "times", "residual", "costs", "trace")
ALL = ("total_return", "failure") + FIELDS
ROWS = ("weight", "norm_parameter", "parameters", "risk")
P, SEED = 3, 31


class Fleet:
    """E environments of one task from ONE state, each with its own rows"""

    def __init__(self, name, task, state, E, precision, n, H, env=None, kernel="rollout_lane", std=0.1, risks=task_rows.RISKS, differentiable=False):
        self.name, self.task, self.state, self.E, self.precision, self.n, self.H = name, task, state, E, precision, n, H
        self.env, self.kernel, self.std = dict(env or {}), kernel, std
        self.rows = task_rows.unlike_rows(task, E, risks=risks)
        self.base = dict(weight=np.array(task.weight, float), norm_parameter=np.array(task.norm_parameter, float),
                         parameters=np.array(task.parameters, float), risk=float(task.risk))
        self.pm = task.packed_model(differentiable=differentiable)
        m = task.model
        dt = m.get_number("agent_timestep", m.timestep)
        rng = np.random.default_rng(3)
        lo, hi = np.asarray(m.arrays["actuator_ctrlrange"], float).reshape(-1, 2).T
        self.lo, self.hi = lo, hi
        self.times = np.tile(state.time + np.arange(P) * ((H - 1) * dt / (P - 1)), (E, 1))
        self.nominal = np.tile(np.clip(rng.normal(0, 0.05, (P, m.nu)), lo, hi), (E, 1, 1))      # one nominal spline for all
        self.mocap = None if not m.nmocap else np.asarray(state.mocap, float)

    def make_context(self, extra=None):
        ctx = context(self.pm, step_bank.packed_task(self.task, self.state), self.precision, dict(self.env, **(extra or {})))
        assert self.kernel in ctx.kernel_name, ctx.kernel_name
        return ctx

    def noise(self, e=0, mode=capi.NOISE_SAMPLING, var=None):
        return capi.make_noise_spec(seed=SEED + e, iteration=2, mode=mode, std0=self.std, param_variance=var)

    # ---- the fleet's side
    def push(self, ctx, envs=None, fields=ROWS):
        envs = list(range(self.E)) if envs is None else envs
        ctx.set_states(np.stack([self.state.state] * len(envs)), [self.state.time] * len(envs),
                       None if self.mocap is None else np.stack([self.mocap] * len(envs)))
        ctx.set_task_params_batched(**{k: (self.rows[k][envs] if k in fields else None) for k in ROWS})

    # ---- one robot's side
    def plain(self, ctx, e=None, fields=ROWS):
        """set_state + set_task_params(row e) (e None: the task's own values)"""
        v = {k: (self.rows[k][e] if e is not None and k in fields else self.base[k]) for k in ROWS}
        ctx.set_task_params(v["weight"], v["norm_parameter"], v["parameters"] if len(self.base["parameters"]) else None, float(v["risk"]))
        ctx.set_state(self.state.state, self.state.time, self.mocap)

    def packed(self, e):
        return step_bank.packed_task(task_rows.task_of_row(self.task, self.rows, e), self.state)

    def assert_rows_decide_the_cost(self, ctx):
        """the nominal spline from the one state under every environment's rows: E different returns"""
        self.push(ctx)
        values = np.tile(self.nominal[:, None], (1, 64, 1, 1))
        ctx.rollout_splines_batched(self.H, capi.SPLINE_LINEAR, self.times, values, num_envs=self.E, n_per_env=64)
        ret, fail = ctx.returns()
        firsts = [float(ret[64 * e]) for e in range(self.E)]
        if self.name == "wave":    # capsules_small.xml's only residual is a constant user sensor of value 0: its cost is 0 under any rows
            assert not fail.any() and firsts == [0.0] * self.E, firsts     # (the A1 on the same kernel, "wave_a1", is where the rows show)
            return
        assert not fail.any() and len(set(firsts)) == self.E, (self.name, firsts)

    # ---- the three sampling calls, batched and plain
    def run(self, ctx, call, envs=None):
        envs = list(range(self.E)) if envs is None else envs
        n, H, t, nom = self.n, self.H, self.times[:len(envs)], self.nominal[:len(envs)]
        if call == "noise":
            ctx.rollout_noise_batched(n, H, capi.SPLINE_CUBIC, t, nom, self.noise(), num_envs=len(envs))
        elif call == "splines":
            ctx.rollout_splines_batched(H, capi.SPLINE_LINEAR, t, self.nodes()[:len(envs)], num_envs=len(envs), n_per_env=n)
        else:
            ctx.rollout_noise_batched_ce(n, H, capi.SPLINE_CUBIC, t, nom, self.variance()[:len(envs)], self.noise(mode=capi.NOISE_CROSS_ENTROPY),
                                         num_envs=len(envs))

    def run_plain(self, ctx, call, i):
        """what environment number i of a batched call is as a plain one: seed + i, its nodes, its variance row"""
        n, H = self.n, self.H
        if call == "noise":
            ctx.rollout_noise(n, H, capi.SPLINE_CUBIC, self.times[i], self.nominal[i], self.noise(i))
        elif call == "splines":
            ctx.rollout_splines(H, capi.SPLINE_LINEAR, self.times[i], self.nodes()[i])
        else:
            ctx.rollout_noise(n, H, capi.SPLINE_CUBIC, self.times[i], self.nominal[i], self.noise(i, capi.NOISE_CROSS_ENTROPY, self.variance()[i]))

    def nodes(self):
        rng = np.random.default_rng(11)
        return np.clip(rng.normal(0, 2 * self.std, (self.E, self.n, P, self.task.model.nu)), self.lo, self.hi)

    def variance(self):
        return np.random.default_rng(12).uniform(0.5, 1.5, (self.E, P, self.task.model.nu)) * self.std ** 2

    def assert_batched_equals_plain(self, ctx, call, envs=None, fields=ROWS):
        envs = list(range(self.E)) if envs is None else envs
        self.push(ctx, envs, fields)
        self.run(ctx, call, envs)
        got = everything(ctx)
        assert ctx.N == len(envs) * self.n
        for i, e in enumerate(envs):
            self.plain(ctx, e, fields)
            self.run_plain(ctx, call, i)
            one = everything(ctx)
            for k in ALL:
                assert np.array_equal(got[k][i * self.n:(i + 1) * self.n], one[k], equal_nan=True), (self.name, call, e, k)
        self.plain(ctx)      # (the context's own values again)
        return got


def lane_fleet(task_name, precision, n, E=3, H=5, differentiable=False):
    b = step_bank.lane_bank(task_name)
    return Fleet(f"{task_name}{precision}", b.task, b.states[1], E, precision, n, H, differentiable=differentiable)


def contact_fleet(name):
    if name in ("quad", "tree_a1", "wave_a1"):
        b = step_bank.a1_bank()
        env, kernel = {"quad": ({"MJPCX_QUAD_MIN_N": "0"}, "rollout_quad_kernel"), "tree_a1": ({"MJPCX_NO_QUAD": "1"}, "rollout_tree_kernel<A1>"),
                       "wave_a1": ({"MJPCX_NO_LDS_MODEL": "1"}, "rollout_wave_kernel")}[name]     # (the A1 on the generic kernel: its residual is not constant)
        return Fleet(name, b.task, b.states[0], 2, 64, 1024 if name == "quad" else 64, 6, env, kernel, std=0.06)
    if name in ("limb32", "tree_humanoid"):
        b = step_bank.humanoid_bank()
        st = [s for s in b.states if s.label.startswith("clip9/key")][0]
        limb = name == "limb32"
        return Fleet(name, b.task, st, 2, 32 if limb else 64, 1280 if limb else 64, 4, {"MJPCX_LIMB_MIN_N": "0"} if limb else {"MJPCX_NO_LIMB": "1"},
                     "rollout_limb_kernel" if limb else "rollout_tree_kernel<Humanoid>", std=0.05, risks=(0.0, 0.05))
    if name == "wave":
        task, states = ts.scene_task()                          # tests/models/capsules_small.xml
        return Fleet(name, task, states[0], 2, 64, 64, 6, {}, "rollout_wave_kernel", std=0.2)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------- lane family
@pytest.mark.parametrize("n", [64, 128])            # one wavefront per environment; two, so that a wrong environment index from blockIdx shows
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("task_name", ["Cartpole", "Particle"])
def test_lane_rollouts_with_rows_equal_plain_calls(task_name, precision, n):
    f = lane_fleet(task_name, precision, n)
    ctx = f.make_context()
    f.assert_rows_decide_the_cost(ctx)
    for call in ("noise", "splines", "ce"):
        f.assert_batched_equals_plain(ctx, call)
    ctx.close()


class FeedbackCase(ti.Case):
    """tests/test_gpu_batch_ilqg.py's case on a Fleet: every environment the fleet's one state (its own policy), rows pushed with the states"""

    def __init__(self, fleet):
        super().__init__(fleet.name, fleet.task, [fleet.state] * fleet.E, fleet.precision, fleet.env, fleet.kernel)
        self.fleet = fleet

    def push(self, ctx, envs):
        self.fleet.push(ctx, envs)

    def run_plain(self, ctx, e, row, horizon, mode, rep, use):
        self.fleet.plain(ctx, e)
        ctx.rollout_feedback(horizon, mode, rep, use, *row)


def assert_feedback_equals_plain(case, ctx, n, combos=((0, 0, 1), (1, 2, 1))):
    envs = list(range(case.fleet.E))
    pol = case.policy(envs, n, case.fleet.H)
    for mode, rep, use in combos:
        case.run_batched(ctx, envs, pol, case.fleet.H, mode, rep, use)
        got = everything(ctx)
        assert ctx.N == len(envs) * n and not got["failure"].any()
        for e in envs:
            case.run_plain(ctx, e, [p[e] for p in pol], case.fleet.H, mode, rep, use)
            ref = everything(ctx)
            for k in ALL:
                assert np.array_equal(got[k][e * n:(e + 1) * n], ref[k]), (case.name, mode, rep, use, n, e, k)
        assert len({float(got["total_return"][e * n]) for e in envs}) == len(envs)


@pytest.mark.parametrize("n", [3, 70])              # 70: two wavefronts per environment, the second partly filled (the padding lanes)
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("task_name", ["Cartpole", "Particle"])
def test_lane_feedback_rollouts_with_rows_equal_plain_calls(task_name, precision, n):
    f = lane_fleet(task_name, precision, 64, differentiable=True)
    ctx = f.make_context()
    f.assert_rows_decide_the_cost(ctx)
    assert_feedback_equals_plain(FeedbackCase(f), ctx, n)
    ctx.close()


# ------------------------------------------------------------------------------------------------- contact families
@pytest.mark.parametrize("name", ["quad", "tree_a1", "limb32", "tree_humanoid", "wave", "wave_a1"])
def test_contact_rollouts_with_rows_equal_plain_calls(name):
    f = contact_fleet(name)
    assert (f.rows["risk"] == 0).any() and (f.rows["risk"] != 0).any()      # a risk-neutral and a risk-sensitive robot in one launch
    ctx = f.make_context()
    f.assert_rows_decide_the_cost(ctx)
    f.assert_batched_equals_plain(ctx, "noise")
    if name in ("quad", "limb32"):
        f.push(ctx)
        f.run(ctx, "noise")
        assert f.kernel in ctx.kernel_name and ctx.quad_stats()["handed_on"] == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------- against the oracle
ORACLE = {"Cartpole64": (1e-9, False), "quad": (1e-9, False), "tree_a1": (1e-6, False), "limb32": (2e-3, True), "wave": (1e-6, False)}


@pytest.mark.parametrize("name", list(ORACLE))
def test_fleet_with_rows_against_the_oracle(name):
    """a share of every environment's candidates (64 of them, spread over the batch) against the oracle with the task packed from row e"""
    tol, returns_only = ORACLE[name]
    f = lane_fleet("Cartpole", 64, 64) if name == "Cartpole64" else contact_fleet(name)
    ctx = f.make_context()
    f.push(ctx)
    f.run(ctx, "noise")
    ret, fail = ctx.returns()
    cands = np.arange(0, f.n, f.n // 64)
    worst = 0.0
    for e in range(f.E):
        nodes = pyoracle.noise_candidates(f.pm, f.noise(e), P, f.nominal[e], cands)
        ref = pyoracle.rollout_batch(f.pm, f.packed(e), f.state.state, f.state.time, f.mocap if f.mocap is not None else np.zeros(0), len(cands), f.H, P,
                                     capi.SPLINE_CUBIC, f.times[e], nodes, num_threads=16)
        assert not ref["failure"].any() and not fail[e * f.n + cands].any(), (name, e)
        for i, c in enumerate(cands):
            d = err(ret[e * f.n + c], ref["total_return"][i])
            if not returns_only:
                tr = ctx.fetch_trajectory(e * f.n + int(c))
                d = max([d] + [err(getattr(tr, k), ref[k][i]) for k in FIELDS])
            worst = max(worst, d)
            assert d <= tol, (name, e, int(c), d)
    print(f"{name}: worst error against the oracle {worst:.3e} (bound {tol:g})")
    ctx.close()


# ------------------------------------------------------------------------------------------------- derivative chains
def chain_fleet(name):
    if name == "quad":
        b = step_bank.a1_bank()
        return Fleet(name, b.task, b.states[0], tg.E, 64, tg.N, tg.H, {}, "rollout_", differentiable=True)
    f = lane_fleet("Cartpole" if name.startswith("cartpole") else "Particle", 64 if name.endswith("64") else 32, tg.N, tg.E, tg.H, differentiable=True)
    f.name = name
    return f


@pytest.mark.parametrize("skip", [0, 3])
@pytest.mark.parametrize("name", ["cartpole64", "cartpole32", "particle64", "quad"])
def test_gradient_step_with_rows_equals_the_sequential_chain(name, skip):
    """tests/test_gpu_batch_gradient.py's comparison: T = 20 steps, so num_eval x NC (Cartpole 11, Particle 13 columns) is no multiple of
    64 and the environments' finite-difference items are padded to whole wavefronts"""
    f = chain_fleet(name)
    ctx = f.make_context()
    f.assert_rows_decide_the_cost(ctx)
    E, N, T = f.E, f.n, tg.T
    times = np.tile(f.state.time + np.arange(5) * ((f.H - 1) * float(f.pm.struct.timestep) / 4), (E, 1))
    nodes = np.tile(np.clip(np.random.default_rng(7).normal(0, 0.2, (1, N, 5, f.task.model.nu)), f.lo, f.hi), (E, 1, 1, 1))
    f.push(ctx)
    ctx.rollout_splines_batched(f.H, capi.SPLINE_LINEAR, times, nodes, num_envs=E, n_per_env=N)
    ret, fail = ctx.returns()
    cand = 5
    assert not fail.reshape(E, N)[:, cand].any() and len(set(ret.reshape(E, N)[:, cand])) == E
    trs = [ctx.fetch_trajectory(e * N + cand) for e in range(E)]
    ev = derivative_steps(T, skip)
    assert (len(ev) * (1 + 2 * (2 * f.task.model.nv + f.task.model.nu))) % 64 != 0 or name == "quad"
    eps = 1e-5 if f.precision == 64 else 1e-3
    got = ctx.gradient_step_batched(E, cand, T, ev, eps, 1, 2, times, with_matrices=True)
    again = ctx.gradient_step_batched(E, cand, T, ev, eps, 1, 2, times, with_matrices=True)
    worst = 0.0
    for key in tg.RESULTS + tg.MATRICES:
        assert np.array_equal(got[key], again[key]), key
    env = tg.Env(f.state.state, f.state.time, f.mocap, f.state.residual_int, f.state.residual_real)
    for e in range(E):
        f.plain(ctx, e)
        ref = tg.sequential_chain(ctx, f.task, env, trs[e], ev, eps, 1, 2, times[e])
        for key in tg.RESULTS + tg.MATRICES:
            g, r = np.asarray(got[key][e], float), np.asarray(ref[key], float)
            assert np.all(np.isfinite(r)), (e, key)
            if skip == 0:
                assert np.array_equal(g, r), (name, e, key, float(np.abs(g - r).max()))
            else:
                d = float(np.max(np.abs(g - r) / (1 + np.abs(r))))
                worst = max(worst, d)
                assert d <= 1e-12, (name, e, key, d)
    if skip:
        print(f"gradient_step_batched with rows vs sequential chain, {name} skip {skip}: max err {worst:.3e}")
    assert len({tuple(np.round(got["cx"][e].ravel(), 12)) for e in range(E)}) == E          # the cost derivatives are each environment's own
    ctx.close()


class StepCase(ts.Case):
    """tests/test_gpu_batch_ilqg_step.py's case on a Fleet"""

    def __init__(self, fleet):
        super().__init__(fleet.name, fleet.task, [fleet.state] * fleet.E, fleet.precision, fleet.kernel)
        self.fleet = fleet

    def rollout(self, ctx, envs, horizon, n):
        self.fleet.push(ctx, envs)
        ctx.rollout_feedback_batched(horizon, 1, 1, 1, *self.policy(envs, n, horizon))
        _, fail = ctx.returns()
        assert not fail.any(), (self.name, fail)

    def set_plain(self, ctx, e):
        s = self.fleet.state
        if s.residual_int or s.residual_real:
            ctx.set_residual_state(s.residual_int, s.residual_real)
        self.fleet.plain(ctx, e)


@pytest.mark.parametrize("skip,steps", [(0, 8), (3, 12)])
@pytest.mark.parametrize("name", ["cartpole64", "cartpole32", "particle64", "quad"])
def test_ilqg_step_with_rows_equals_the_plain_calls(name, skip, steps):
    f = chain_fleet(name)
    f.E = 3
    for k in ROWS:
        f.rows[k] = f.rows[k][:3]
    case = StepCase(f)
    ctx = f.make_context()
    f.H = steps
    envs, n, cands = [0, 1, 2], 3, [2, 0, 1]
    case.rollout(ctx, envs, steps, n)
    ev, eps = derivative_steps(steps, skip), 1e-6 if f.precision == 64 else 1e-3
    assert (len(ev) * (1 + 2 * (2 * f.task.model.nv + f.task.model.nu))) % 64 != 0 or name == "quad"
    mu, rate = [1.0, 0.5, 2.0], [1.0, 0.5, 2.0]
    refs = [ts.Reference(case, ctx, e, cands[e], steps, skip, eps, 1, n) for e in envs]
    f.plain(ctx)
    for reg_type, use_limits in ((0, 1), (2, 0)):
        got = ctx.ilqg_step_batched(cands, steps, ev, eps, 1, reg_type, use_limits, mu, rate, with_matrices=True, **ts.REG)
        again = ctx.ilqg_step_batched(cands, steps, ev, eps, 1, reg_type, use_limits, mu, rate, with_matrices=True, **ts.REG)
        for e in envs:
            ref = refs[e].backward(reg_type, use_limits, mu[e], rate[e], **ts.REG)
            ts.assert_env_equal(got, e, ref, (name, skip, reg_type, use_limits, e))
            ts.assert_env_equal(again, e, ref, (name, skip, reg_type, use_limits, e, "again"))
            assert ref["status"] == 1
    assert len({tuple(np.round(got["cx"][e].ravel(), 12)) for e in envs}) == 3
    ctx.close()


# ------------------------------------------------------------------------------------------------- semantics
@pytest.mark.parametrize("name", ["Cartpole64", "Particle32", "tree_a1"])
def test_semantics_of_the_rows(name):
    f = contact_fleet(name) if name == "tree_a1" else lane_fleet(name[:-2], int(name[-2:]), 64)
    E, n = f.E, f.n
    fresh = f.make_context()                                           # a context that never has rows
    fresh.set_states(np.stack([f.state.state] * E), [f.state.time] * E, None if f.mocap is None else np.stack([f.mocap] * E))
    f.run(fresh, "noise")
    shared = everything(fresh)
    f.plain(fresh, 1)
    f.run_plain(fresh, "noise", 0)
    plain_ref = everything(fresh)                                      # ... and a plain call with row 1 on it
    fresh.close()
    ctx = f.make_context()
    base = f.assert_batched_equals_plain(ctx, "noise")
    assert not all(np.array_equal(base[k], shared[k], equal_nan=True) for k in ALL)
    # ---- two calls give the same bits; the rows persist without being pushed again
    f.run(ctx, "noise")
    again = everything(ctx)
    # ---- a plain call between two batched ones: unaffected by the rows, and the rows unaffected by its set_task_params
    f.plain(ctx, 1)
    f.run_plain(ctx, "noise", 0)
    between = everything(ctx)
    f.plain(ctx)
    f.run(ctx, "noise")
    after = everything(ctx)
    for k in ALL:
        assert np.array_equal(again[k], base[k], equal_nan=True), (k, "two calls")
        assert np.array_equal(between[k], plain_ref[k], equal_nan=True), (k, "the plain call")
        assert np.array_equal(after[k], base[k], equal_nan=True), (k, "after the plain call")
    # ---- a field given as None is the context's for every environment
    for field in ROWS:
        if f.rows[field].size:
            f.assert_batched_equals_plain(ctx, "noise", fields=(field,))
    # ---- all four None: the bits of a context that never had rows
    ctx.set_task_params_batched()
    f.run(ctx, "noise")
    none = everything(ctx)
    for k in ALL:
        assert np.array_equal(none[k], shared[k], equal_nan=True), (k, "all None")
    # ---- another E than set_states': refused, naming the call; set_states with another E drops the rows
    ctx.E = E - 1
    with pytest.raises(capi.MjpcxError, match="mjpcx_set_task_params_batched") as ei:
        ctx.set_task_params_batched(weight=f.rows["weight"][:E - 1])
    assert ei.value.code == -1
    f.push(ctx)
    f.push(ctx, list(range(E - 1)), fields=())                          # (set_states of E - 1 environments, then no rows)
    ctx.set_states(np.stack([f.state.state] * E), [f.state.time] * E, None if f.mocap is None else np.stack([f.mocap] * E))
    f.run(ctx, "noise")
    dropped = everything(ctx)
    for k in ALL:
        assert np.array_equal(dropped[k], shared[k], equal_nan=True), (k, "rows of another fleet size")
    ctx.close()


def test_permuting_rows_permutes_the_outputs():
    """one state, one spline set for every environment: the outputs follow the rows"""
    f = lane_fleet("Cartpole", 64, 64)
    f.nodes = lambda: np.tile(Fleet.nodes(f)[:1], (f.E, 1, 1, 1))
    ctx = f.make_context()
    n, perm = f.n, [2, 0, 1]
    f.push(ctx)
    f.run(ctx, "splines")
    ref = everything(ctx)
    f.push(ctx, perm)
    f.run(ctx, "splines")
    got = everything(ctx)
    assert len({float(ref["total_return"][e * n]) for e in range(f.E)}) == f.E
    for k in ALL:
        for i, e in enumerate(perm):
            assert np.array_equal(got[k][i * n:(i + 1) * n], ref[k][e * n:(e + 1) * n], equal_nan=True), (k, i, e)
    ctx.close()


# ------------------------------------------------------------------------------------------------- the planners
T_PLAN, E_PLAN = 12, 3


def plan_fleet():
    task = load_task("Cartpole")
    st = State(task.model)
    st.set([0.3, 2.5], [-0.2, 0.4], time=0.1)
    return task, [st] * E_PLAN, task_rows.unlike_tasks(task, E_PLAN)


def configure(p, task, tasks, settings):
    p.initialize(task.model, task)
    for k, v in settings.items():
        setattr(p, k, v)
    p.allocate()
    if tasks is not None:
        p.set_tasks(tasks)
    p.reset(T_PLAN)
    return p


def assert_same_trajectory(tb, tp, where):
    assert tb.total_return == tp.total_return and tb.failure == tp.failure, where
    for k in FIELDS:
        assert np.array_equal(getattr(tb, k), getattr(tp, k)), (where, k)


def advance(task, states, members):
    nq = task.model.nq
    out = []
    for e, st in enumerate(states):
        tr = members[e].best_trajectory()
        new = State(task.model)
        new.set(tr.states[2, :nq], tr.states[2, nq:], time=float(tr.times[2]))
        out.append(new)
    return out


@pytest.mark.parametrize("kind", ["sampling", "cross_entropy", "gradient", "ilqg"])
def test_fleet_planner_with_tasks_equals_single_planners_on_the_device(kind):
    task, states, tasks = plan_fleet()
    fleet_cls, single_cls, settings = {
        "sampling": (GpuBatchSamplingPlanner, GpuSamplingPlanner, dict(num_trajectory_=64)),
        "cross_entropy": (GpuBatchCrossEntropyPlanner, GpuCrossEntropyPlanner, dict(num_trajectory_=63, n_elite_=6)),
        "gradient": (GpuBatchGradientPlanner, GpuGradientPlanner, dict(num_trajectory=64)),
        "ilqg": (GpuBatchILQGPlanner, GpuILQGPlanner, dict(num_rollouts_gui_=10))}[kind]
    seeded = kind in ("sampling", "cross_entropy")
    batch = configure(fleet_cls(E_PLAN, seed=SEED) if seeded else fleet_cls(E_PLAN), task, tasks, settings)
    singles = [configure(single_cls(seed=SEED + e) if seeded else single_cls(), tasks[e], None, settings) for e in range(E_PLAN)]
    for step in range(2):
        batch.set_states(states)
        batch.optimize_policy(T_PLAN)
        for e, p in enumerate(singles):
            b = batch.envs[e]
            p.set_state(states[e])
            p.optimize_policy(T_PLAN)
            where = (kind, step, e)
            if kind in ("sampling", "cross_entropy"):
                assert b.improvement == p.improvement, where
                assert np.array_equal(b.policy.plan.times(), p.policy.plan.times()), where
                assert np.array_equal(b.policy.plan.values(), p.policy.plan.values()), where
                if kind == "cross_entropy":
                    assert b.trajectory_order == p.trajectory_order and np.array_equal(b.variance, p.variance), where
                else:
                    assert batch.winners[e] == p.winner and (b.best_return, b.nominal_return) == (p.best_return, p.nominal_return), where
            elif kind == "gradient":
                Pn = p.policy.num_spline_points
                assert b.winner == p.winner and b.action_step == p.action_step and np.array_equal(b.dV, p.dV), where
                assert np.array_equal(b.policy.parameters[:Pn], p.policy.parameters[:Pn]), where
            else:
                ti.assert_members_equal(b, p, True, where)
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), where)
        if step == 0:     # one state, one initial policy: what tells the members apart is their task (and, where there is noise, the seed)
            assert len({batch.best_trajectory(e).total_return for e in range(E_PLAN)}) == E_PLAN
        states = advance(task, states, singles)
    batch.ctx.close()
    for p in singles:
        p.ctx.close()
