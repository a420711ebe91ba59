"""-m gpu: iLQG's feedback rollouts for a fleet (mjpcx_rollout_feedback_batched) on every feedback kernel family, and GpuBatchILQGPlanner
on the device.

   mjpcx_rollout_feedback_batched <-> E x mjpcx_rollout_feedback on the same context: bit for bit -- returns, failure flags and all six
       Trajectory buffers of EVERY global candidate -- for both modes, the three representations, use_state 0 / 1 and 1, 3, 10 (lane
       family also 70: two wavefronts per environment, the second partly filled) rollouts per environment
   permuting the environments permutes the outputs bit for bit; two calls give the same bits; a plain call after a batched one equals
       one made before it
   GpuBatchILQGPlanner on the device <-> E sequential GpuILQGPlanner on the device: everything exactly equal
   GpuBatchILQGPlanner on the device <-> the same planner on the oracle backend: equal winners; returns, dV, gains to 1e-7 max(1, |x|),
       the figure of tests/test_gpu_quadruped.py::test_one_ilqg_iteration_on_the_a1_against_the_oracle (rollout returns) and of
       tests/test_gpu_batch_gradient.py::test_planner_matches_the_oracle_backend; the fleet's states are chosen so that the oracle's
       best and second-best line-search returns are at least 1000 x that apart, asserted here
Shapes: E = 3, H = Tn = 6 unless stated; every environment has its own state, clock, mocap pose and nominal. The policies are tame
(gains and improvements of 0.02) so that no candidate fails: a failed candidate stops recording, and what its buffers hold past that
step is whatever an earlier launch of another shape left there.
Not exercised: the refusal on a sharded context (needs two ranks) and the one for xfrc noise (the request lives only inside
mjpcx_rollout_splines_noisy; no public call leaves it pending)."""
import os

import numpy as np
import pytest

import step_bank
from batch_ilqg_oracle_backend import BatchILQGOracleContext
from mujoco_mpc_amd import capi, mjcf
from mujoco_mpc_amd.planners import GpuBatchILQGPlanner, GpuILQGPlanner, State
from mujoco_mpc_amd.task import Task, load_task

pytestmark = pytest.mark.gpu
FIELDS = ("states", "actions", "times", "residual", "costs", "trace")
E, H = 3, 6
COMBOS = [(mode, rep, use) for mode in (0, 1) for rep in (0, 1, 2) for use in (0, 1)]


def context(pm, pt, precision, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.Context(pm, pt, 0, precision)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def everything(ctx):
    """returns, failure flags and the six buffers of every candidate of the last rollout"""
    ret, fail = ctx.returns()
    out = {"total_return": ret.copy(), "failure": fail.copy()}
    trs = [ctx.fetch_trajectory(c) for c in range(ctx.N)]
    for k in FIELDS:
        out[k] = np.stack([getattr(tr, k) for tr in trs])
    return out


def scene_task():
    """tests/models/capsules_tendon.xml: a generic contact model (no registered kernel configuration)"""
    fm = mjcf.load_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "capsules_tendon.xml"))
    task = Task(name="scene", residual_id=0, model=fm).reset()
    states = []
    for k in range(4):   # (tests/test_gpu_batch.py's scene states)
        q, v = fm.arrays["qpos0"].copy(), np.zeros(fm.nv)
        q[14 + 2] = 1.0 + 0.0995 - 0.002 * k
        v[12 + 2] = -0.5 + 0.1 * k
        q[fm.nq - 2] = 0.6 - 0.1 * k
        v[0] = 0.3 + 0.2 * k
        states.append(step_bank.BankState(f"scene{k}", np.concatenate([q, v]), 0.05 * k, None))
    return task, states


class Case:
    """one feedback kernel family: the task, its environments, how the context is made and what it must be running"""

    def __init__(self, name, task, states, precision, env, kernel, integrator=None, per_env_residual=False):
        self.name, self.task, self.states, self.precision, self.env, self.kernel = name, task, list(states), precision, env, kernel
        self.per_env_residual = per_env_residual
        self.pm = task.packed_model(differentiable=True)
        if integrator is not None:
            self.pm.struct.integrator = integrator
        self.lane = kernel == "rollout_lane"

    def make_context(self):
        ctx = context(self.pm, step_bank.packed_task(self.task, self.states[0]), self.precision, self.env)
        assert self.kernel in ctx.kernel_name, ctx.kernel_name   # (the context's family decides the feedback kernel: mjpcx.hip, do_feedback)
        return ctx

    def mocap(self, e):
        s = self.states[e]
        return np.zeros(0) if s.mocap is None else np.asarray(s.mocap, float)

    def policy(self, envs, n, Tn=H, seed=5, action_scale=None):
        """per environment: a nominal of Tn steps on its own clock around its own state, small gains and improvements, n steps
        (action_scale: {environment: factor on its nominal actions, clipped to the control range})"""
        m = self.task.model
        nq, nv, nu = m.nq, m.nv, m.nu
        dt = float(self.pm.struct.timestep)
        out = [[] for _ in range(6)]
        for e in envs:
            rng = np.random.default_rng(seed + 13 * e)    # (the environment's own policy, whatever its place in the fleet)
            s = self.states[e]
            times = s.time + dt * (np.arange(Tn) + 0.3)    # knots off the step grid: mode 1 interpolates at every step
            x = np.tile(s.state, (Tn, 1)) + 0.01 * rng.normal(size=(Tn, nq + nv))
            adr = np.asarray(m.arrays["jnt_qposadr"]).astype(int)
            for j, jt in enumerate(np.asarray(m.arrays["jnt_type"]).astype(int)):
                if jt in (0, 1):                           # free / ball: unit quaternions
                    a = adr[j] + (3 if jt == 0 else 0)
                    x[:, a:a + 4] /= np.linalg.norm(x[:, a:a + 4], axis=1, keepdims=True)
            lo, hi = np.asarray(m.arrays["actuator_ctrlrange"], float).reshape(-1, 2).T
            alpha = np.concatenate([np.exp(np.linspace(0, np.log(1e-3), n - 1)), [0.0]]) if n > 1 else np.array([0.7])
            scale = (action_scale or {}).get(e, 1.0)
            for k, v in enumerate((times, x, np.clip(scale * np.clip(0.1 * rng.normal(size=(Tn, nu)), lo, hi), lo, hi), 0.02 * rng.normal(size=(Tn, nu, 2 * nv)),
                                   0.02 * rng.normal(size=(Tn, nu)), alpha)):
                out[k].append(v)
        return [np.stack(v) for v in out]

    def push(self, ctx, envs):
        ctx.set_states(np.stack([self.states[e].state for e in envs]), [self.states[e].time for e in envs],
                       np.stack([self.mocap(e) for e in envs]) if self.task.model.nmocap else None)
        if self.per_env_residual:
            ctx.set_residual_states(np.array([self.states[e].residual_int for e in envs], np.int32),
                                    np.array([self.states[e].residual_real for e in envs], float))

    def run_batched(self, ctx, envs, pol, horizon, mode, rep, use):
        self.push(ctx, envs)
        ctx.rollout_feedback_batched(horizon, mode, rep, use, *pol)

    def run_plain(self, ctx, e, row, horizon, mode, rep, use):
        s = self.states[e if self.per_env_residual else 0]
        if s.residual_int or s.residual_real:
            ctx.set_residual_state(s.residual_int, s.residual_real)
        ctx.set_state(self.states[e].state, self.states[e].time, self.mocap(e) if self.task.model.nmocap else None)
        ctx.rollout_feedback(horizon, mode, rep, use, *row)


def make_case(name):
    if name.startswith("cartpole") or name.startswith("particle"):
        b = step_bank.lane_bank("Cartpole" if name.startswith("cartpole") else "Particle")
        return Case(name, b.task, b.states[:4], 64 if name.endswith("64") else 32, {}, "rollout_lane")
    if name in ("quad", "tree_a1", "quad_residual"):
        b = step_bank.a1_bank()
        st = b.states[:4]                                  # home and three trot states; modes 0..3
        assert [s.label.split("/")[0] for s in st] == ["home", "trot0", "trot1", "trot2"]
        return Case(name, b.task, st, 64, {"MJPCX_NO_QUAD_FEEDBACK": "1"} if name == "tree_a1" else {}, "rollout_quad_kernel",
                    per_env_residual=name == "quad_residual")
    if name in ("wave", "wave_rk4"):
        task, states = scene_task()
        return Case(name, task, states, 64, {}, "rollout_wave_kernel", integrator=1 if name == "wave_rk4" else None)
    raise KeyError(name)


def assert_equals_plain(case, ctx, envs, n, horizon=H, Tn=H, combos=COMBOS, expect_handed_on=None, action_scale=None):
    """one batched call against len(envs) plain calls, for every (mode, representation, use_state) of `combos`"""
    pol = case.policy(envs, n, Tn, action_scale=action_scale)
    for mode, rep, use in combos:
        case.run_batched(ctx, envs, pol, horizon, mode, rep, use)
        assert ctx.N == len(envs) * n
        got = everything(ctx)
        if expect_handed_on is not None:
            handed = ctx.quad_stats()["handed_on"]
            print(f"{case.name} mode {mode}: {handed} of {len(envs) * n} candidates handed on")
            assert expect_handed_on(mode, handed), (mode, handed)
        assert not got["failure"].any(), (case.name, mode, rep, use, got["failure"])
        for i, e in enumerate(envs):
            case.run_plain(ctx, e, [p[i] for p in pol], horizon, mode, rep, use)
            ref = everything(ctx)
            for k in ("total_return", "failure") + FIELDS:
                assert np.array_equal(got[k][i * n:(i + 1) * n], ref[k]), (case.name, mode, rep, use, n, e, k)
        # the environments were different problems
        assert len({tuple(got["states"][i * n, -1]) for i in range(len(envs))}) == len(envs)


LANE_CASES = ["cartpole64", "cartpole32", "particle64", "particle32"]
CASES = LANE_CASES + ["quad", "tree_a1", "wave", "wave_rk4"]
# 70 rollouts per environment is the lane family's case (two wavefronts per environment, the second partly filled); on the other
# kernels a workgroup is one candidate
SHAPES = [(name, n) for name in CASES for n in (1, 3, 10)] + [(name, 70) for name in LANE_CASES]


@pytest.mark.parametrize("name,n", SHAPES)
def test_batched_equals_plain_calls(name, n):
    case = make_case(name)
    ctx = case.make_context()
    # (the quad feedback kernel rolls at least some of these tame candidates out itself: the comparison is not only of its hand-on path)
    assert_equals_plain(case, ctx, [0, 1, 2], n, expect_handed_on=(lambda mode, h: h < 3 * n) if name == "quad" else None)
    ctx.close()


@pytest.mark.parametrize("name", ["particle64", "quad", "wave"])
def test_horizons_beyond_and_within_the_nominal(name):
    """H > Tn: the time policy holds its ends (the index policy is refused, as by the plain call); H < Tn: both modes"""
    case = make_case(name)
    ctx = case.make_context()
    assert_equals_plain(case, ctx, [0, 1, 2], 3, horizon=9, Tn=6, combos=[(1, 1, 1), (1, 2, 1), (1, 0, 0)])
    assert_equals_plain(case, ctx, [0, 1, 2], 3, horizon=4, Tn=6, combos=[(0, 0, 1), (1, 2, 1)])
    pol = case.policy([0, 1, 2], 3, 6)
    case.push(ctx, [0, 1, 2])
    with pytest.raises(capi.MjpcxError, match="at least as long") as e:
        ctx.rollout_feedback_batched(9, 0, 0, 1, *pol)
    assert e.value.code == -1
    ctx.close()


HAND_ON_STATE, HAND_ON_H = "tangled3/step25", 12


def test_hand_on_in_a_fleet():
    """One environment starts from a tangled state of the A1 bank and rollout_feedback_quad_kernel hands its candidates on; home and a
    trot state are not handed on. The second launch (only_flagged) rolls the handed-on candidates out on the tree kernel with their own
    environment's blob and nominal, and the fleet still equals the plain calls bit for bit.
    Which state: probed on an MI355X over the whole bank, plain calls -- with the tame policy of this file NO bank state but random4 /
    random8 / random12 (out of the pair proofs' joint range from their first step) is handed on at H = 6, 12 or 36, the tangled ones
    included: the kernel covers their leg-leg contacts. With nominal actions as wild as the rollouts that made the tangled states
    (x 10, clipped to the control range) none is handed on at H = 6 either; at H = Tn = 12 tangled3/step25 hands all three candidates
    on under the index policy (a joint leaves the range the pair proofs cover), home and trot0 under the tame policy none. So this case
    alone runs 12 steps, and only the tangled environment gets the wild nominal. Under the time policy the count is printed, not fixed."""
    b = step_bank.a1_bank()
    tangled = [s for s in b.states if s.label.startswith(HAND_ON_STATE)]
    assert len(tangled) == 1
    case = Case("quad", b.task, [tangled[0], b.states[0], b.states[1]], 64, {}, "rollout_quad_kernel")
    ctx = case.make_context()
    n = 3
    assert_equals_plain(case, ctx, [0, 1, 2], n, horizon=HAND_ON_H, Tn=HAND_ON_H, combos=[(0, 0, 1), (1, 1, 1)], action_scale={0: 10.0},
                        expect_handed_on=lambda mode, h: 0 < h < 3 * n if mode == 0 else h < 3 * n)
    ctx.close()


def test_four_residual_modes_in_one_fleet():
    case = make_case("quad_residual")
    assert len({s.residual_int[0] for s in case.states}) == 4
    ctx = case.make_context()
    assert_equals_plain(case, ctx, [0, 1, 2, 3], 3, combos=[(0, 0, 1), (1, 2, 1)])
    ctx.close()


@pytest.mark.parametrize("name", ["particle32", "quad_residual", "wave"])
def test_environment_independence_and_determinism(name):
    case = make_case(name)
    ctx = case.make_context()
    n, envs, perm = 3, [0, 1, 2, 3], [2, 0, 3, 1]
    for mode, rep, use in ((0, 0, 1), (1, 2, 1)):
        case.run_batched(ctx, envs, case.policy(envs, n), H, mode, rep, use)
        base = everything(ctx)
        case.run_batched(ctx, envs, case.policy(envs, n), H, mode, rep, use)
        again = everything(ctx)
        case.run_batched(ctx, perm, case.policy(perm, n), H, mode, rep, use)
        got = everything(ctx)
        for k in ("total_return", "failure") + FIELDS:
            assert np.array_equal(base[k], again[k]), (k, "two identical calls")
            for i, e in enumerate(perm):
                assert np.array_equal(got[k][i * n:(i + 1) * n], base[k][e * n:(e + 1) * n]), (k, i, e)
    ctx.close()


@pytest.mark.parametrize("name", ["cartpole64", "quad"])
def test_plain_call_is_untouched_by_a_batched_one(name):
    case = make_case(name)
    ctx = case.make_context()
    pol = case.policy([0, 1, 2], 10)
    row = [r[0] for r in case.policy([3], 10)]
    case.run_plain(ctx, 3, row, H, 0, 0, 1)
    before = everything(ctx)
    case.run_batched(ctx, [0, 1, 2], pol, H, 0, 0, 1)
    ctx.returns()
    ctx.rollout_feedback(H, 0, 0, 1, *row)                  # no set_state in between: the plain call keeps the state of set_state
    after = everything(ctx)
    for k in ("total_return", "failure") + FIELDS:
        assert np.array_equal(before[k], after[k]), k
    ctx.close()


def test_a_plain_feedback_rollout_ends_the_batched_one():
    """mjpcx_rollout_feedback resets the context's candidates-per-environment like every plain rollout. After a batched feedback
    rollout of E x n candidates and then a plain one of N = E * n, mjpcx_ilqg_step_batched and mjpcx_gradient_step_batched refuse -- the
    shape alone (E * n == N, E environments set) would let them gather "environment e's candidate" from a rollout that had no
    environments -- and a batched rollout + iLQG step after that equal the same pair on a fresh context bit for bit.
    Cartpole fp64, E = 2, n = 3, H = Tn = 6."""
    case = make_case("cartpole64")
    envs, n = [0, 1], 3
    pol = case.policy(envs, n)
    ev = np.arange(H, dtype=np.int32)
    step = dict(T=H, evaluate=ev, eps=1e-6, centered=0, reg_type=0, use_limits=1, mu=np.full(2, 1e-3), rate=np.ones(2), factor=2.0,
                min_reg=1e-6, max_reg=1e6, max_iter=5)

    def batched_pair(ctx):
        case.run_batched(ctx, envs, pol, H, 0, 0, 1)
        return ctx.ilqg_step_batched([0, 0], **step)

    ctx = case.make_context()
    case.run_batched(ctx, envs, pol, H, 0, 0, 1)
    flat = [np.concatenate([p[0], p[0]]) if k == 5 else p[0] for k, p in enumerate(pol)]    # one nominal, N = 6 step sizes
    case.run_plain(ctx, 0, flat, H, 0, 0, 1)
    assert ctx.N == len(envs) * n
    with pytest.raises(capi.MjpcxError, match="the last rollout was not a batched one") as e:
        ctx.ilqg_step_batched([0, 0], **step)
    assert e.value.code == -1
    with pytest.raises(capi.MjpcxError, match="the last rollout was not a batched one") as e:
        ctx.gradient_step_batched(2, 0, H, ev, 1e-6, 0, 1, np.tile(np.linspace(0.0, 0.05, 3), (2, 1)))
    assert e.value.code == -1
    got = batched_pair(ctx)
    ctx.close()
    fresh = case.make_context()
    ref = batched_pair(fresh)
    fresh.close()
    for k in ("K", "du", "dV"):
        assert np.array_equal(got[k], ref[k]), k


def test_refusals():
    case = make_case("cartpole64")
    ctx = case.make_context()
    envs, n = [0, 1, 2], 3
    pol = case.policy(envs, n)

    def refused(code, match, horizon=H, mode=0, rep=0, arrays=pol, **kw):
        with pytest.raises(capi.MjpcxError, match=match) as e:
            ctx.rollout_feedback_batched(horizon, mode, rep, 1, *arrays, **kw)
        assert e.value.code == code, (match, e.value.code)

    refused(-1, "before mjpcx_set_states")
    case.push(ctx, [0, 1])
    refused(-1, "3 environments after mjpcx_set_states of 2")
    case.push(ctx, envs)
    ctx.rollout_feedback_batched(H, 0, 0, 1, *pol)
    refused(-1, "number of environments", num_envs=0, n_per_env=n)
    refused(-1, "must be >= 1", num_envs=3, n_per_env=0)
    refused(-1, "must be >= 1", horizon=0)
    refused(-1, "must be >= 1", arrays=[np.zeros((3, 0))] + pol[1:], num_envs=3, n_per_env=n)
    refused(-1, "unknown feedback policy mode", mode=2)
    refused(-1, "representation", mode=1, rep=3)
    refused(-1, "at least as long", horizon=H + 1)
    with pytest.raises(ValueError, match="array sizes"):
        ctx.rollout_feedback_batched(H, 0, 0, 1, *([pol[0][:2]] + pol[1:]))
    ctx.close()
    # fp32 contexts of the wavefront-per-candidate family: refused as by the plain call
    quad = make_case("quad")
    quad.precision = 32
    quad.kernel = "rollout_"
    ctx = quad.make_context()
    qpol = quad.policy(envs, n)
    quad.push(ctx, envs)
    with pytest.raises(capi.MjpcxError, match="fp64 only") as e:
        ctx.rollout_feedback_batched(H, 0, 0, 1, *qpol)
    assert e.value.code == -2
    ctx.set_state(quad.states[0].state, 0.0, quad.mocap(0))
    with pytest.raises(capi.MjpcxError, match="fp64 only") as e:
        ctx.rollout_feedback(H, 0, 0, 1, *[p[0] for p in qpol])
    assert e.value.code == -2
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- the planner
T = 12


def planner_fleet(name):
    """the task and three States, chosen on the CPU: on the oracle backend every environment's best and second-best line-search
    returns of the first plan step are more than 1e-4 max(1, |r|) apart (asserted in the oracle test below)"""
    task = load_task(name)
    m = task.model
    rng = np.random.default_rng(38)
    states = []
    for e in range(E):
        st = State(m)
        if name == "QuadrupedFlat":
            q = np.asarray(m.keyframes["home"]["qpos"], float).copy()
            q[0:2] += 0.05 * e
            q[7:] += rng.normal(0, 0.05, 12)
            st.set(q, rng.normal(0, 0.1, 18), mocap_pos=[[0.3 + 0.2 * e, -0.1 * e, 0.26], [-2.5, 0, 0]], mocap_quat=[[1, 0, 0, 0], [1, 0, 0, 0]],
                   time=0.04 * e)
        else:
            st.set(rng.uniform(-0.5, 0.5, m.nq), rng.normal(0, 0.3, m.nv), time=0.1 * e)
        states.append(st)
    if name == "QuadrupedFlat":
        task.transition(0.0)
    return task, states


def fleet_planner(task, backend_factory=None):
    p = GpuBatchILQGPlanner(E, backend_factory=backend_factory)
    p.initialize(task.model, task)
    p.allocate()
    p.reset(T)
    return p


def assert_members_equal(b, p, exact, where):
    rel = lambda x, y: np.all(np.abs(np.asarray(x, float) - np.asarray(y, float)) <= 1e-7 * np.maximum(1.0, np.abs(np.asarray(y, float))))
    same = (lambda x, y: np.array_equal(np.asarray(x), np.asarray(y))) if exact else rel
    assert b.winner == p.winner and b.action_step == p.action_step and b.feedback_scaling == p.feedback_scaling, where
    assert b.regularization == p.regularization and b.iteration_completed == p.iteration_completed, where
    assert same(b.dV, p.dV) and same(b.improvement, p.improvement) and same(b.expected, p.expected), (where, b.dV, p.dV)
    for pb, pp in ((b.policy, p.policy), (b.candidate0, p.candidate0)):
        assert same(pb.trajectory.total_return, pp.trajectory.total_return), where
        for k in ("states", "actions", "times") + (("residual", "costs", "trace") if exact else ()):
            assert same(getattr(pb.trajectory, k)[:T], getattr(pp.trajectory, k)[:T]), (where, k)
    if exact:
        assert b.surprise == p.surprise, where
        assert np.array_equal(b.policy.feedback_gain[:T], p.policy.feedback_gain[:T]), where
        assert np.array_equal(b.policy.action_improvement[:T], p.policy.action_improvement[:T]), where


@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_planner_equals_sequential_planners_on_the_device(name):
    task, states = planner_fleet(name)
    batch = fleet_planner(task)
    batch.set_states(states)
    batch.optimize_policy(T)
    assert not any(batch.sat_out)
    for e in range(E):
        p = GpuILQGPlanner()
        p.initialize(task.model, task); p.allocate(); p.reset(T)
        p.set_state(states[e])
        p.optimize_policy(T)
        assert p.iteration_completed
        assert_members_equal(batch.envs[e], p, True, (name, e))
        p.ctx.close()
    assert len(set(batch.winner)) > 1 or len({tuple(np.round(p.dV, 9)) for p in batch.envs}) == E
    batch.ctx.close()


@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_planner_matches_the_oracle_backend(name):
    task, states = planner_fleet(name)
    gpu = fleet_planner(task)
    ora = fleet_planner(task, lambda t: BatchILQGOracleContext(t, threads=8, differentiable=True))
    for p in (gpu, ora):
        p.set_states(states)
        p.optimize_policy(T)
    n = ora.envs[0].num_trajectory_
    ret = ora.ctx.out["total_return"].reshape(E, n)
    fail = ora.ctx.out["failure"].reshape(E, n)
    for e in range(E):
        # a near tie on the oracle side could flip the winner: never compare a coin toss
        r = np.sort(ret[e][fail[e] == 0])
        assert len(r) >= 2 and (r[1] - r[0]) >= 1000 * 1e-7 * max(1.0, abs(r[0])), (e, r[:3])
        assert not ora.sat_out[e] and ora.envs[e].iteration_completed
    for e, (g, o) in enumerate(zip(gpu.envs, ora.envs)):
        assert_members_equal(g, o, False, (name, e))
    gpu.ctx.close()
