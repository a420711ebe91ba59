"""-m gpu: iLQG's derivative chain and backward pass for a fleet (mjpcx_ilqg_step_batched) and GpuBatchILQGPlanner's device chain.

   mjpcx_ilqg_step_batched after mjpcx_rollout_feedback_batched <-> mjpcx_fetch_trajectory of the same candidates fed through the plain
       calls on the same context -- set_state -> planners.model_derivatives (transition_fd) -> zeroed last step -> cost_derivatives ->
       the Python retry loop over backward_pass: every output np.array_equal (A, B, cx, cu, cxx, cxu, cuu, Vx, Vxx, K, du, dV, status,
       mu, rate, retries, nominal_return), for both `centered` values, reg_type 0 / 1 / 2, use_limits 0 / 1, mixed candidates [2, 0, 1],
       on the lane family in both precisions, the quad kernel's A1 and a generic contact model; also with derivative_skip 3
   a fleet whose first environment's sweep fails at mu = min_regularization and succeeds after scalings (found on the CPU oracle:
       Cartpole with the control term's weight at -0.01, regularisation type 0 -- cuu is then -0.01 / T and Quu + mu I is indefinite at
       1e-6 .. 1.024e-3 and positive definite at 3.2768e-2, the sixth sweep), whose second starts at mu = 1 and needs none, whose third
       takes no part; and one whose first environment fails all eight retries (weight -0.1, type 1)
   permuting the environments permutes the outputs bit for bit; two calls give the same bits; a plain backward_pass after a batched
       call equals one made before it
   every refusal by code and message; n > 48 on tests/models/capsules_tendon.xml (2 nv = 64). Not exercised: more than 32 cost terms /
       residuals per term and m > 16 -- no model or task in the tree has them -- and a sharded context, which needs two ranks
   GpuBatchILQGPlanner with the device chain <-> the same planner with device_chain = False, on the device: everything exactly equal
       over two plan steps
With status 0 the plain backward_pass leaves K, du, Vx, Vxx beyond the failing step as its output buffer held them, so those four are
compared only where the last sweep succeeded. Shapes: E = 3, three rollouts per environment, T = H = 8 (skip: 12)."""
import copy
import os

import numpy as np
import pytest

import step_bank
from batch_ilqg_step_oracle_backend import retry_loop
from mujoco_mpc_amd import capi, mjcf
from mujoco_mpc_amd.planners import GpuBatchILQGPlanner, State, derivative_steps, model_derivatives
from mujoco_mpc_amd.task import Task, load_task

pytestmark = pytest.mark.gpu
E, N_PER_ENV, T = 3, 3, 8
CANDS = [2, 0, 1]
MATRICES = ("A", "B", "cx", "cu", "cxx", "cxu", "cuu")
SWEEP = ("Vx", "Vxx", "K", "du")
SCALARS = ("dV", "status", "mu", "rate", "retries", "nominal_return")
REG = dict(factor=2.0, min_reg=1e-6, max_reg=1e6, max_iter=5)


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


def scene_task():
    """tests/models/capsules_small.xml: a generic contact model (no registered kernel configuration) -- capsules_tendon.xml, the `wave`
    family of tests/test_gpu_batch_ilqg.py, without its last two rods: that one has 2 nv = 64 and the backward pass covers n <= 48"""
    fm = mjcf.load_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "capsules_small.xml"))
    task = Task(name="scene", residual_id=0, model=fm).reset()
    states = []
    for k in range(4):
        q, v = fm.arrays["qpos0"].copy(), np.zeros(fm.nv)
        q[14 + 2] = 1.0 + 0.0995 - 0.002 * k
        v[12 + 2] = -0.5 + 0.1 * k
        q[fm.nq - 2] = 0.6 - 0.1 * k
        v[0] = 0.3 + 0.2 * k
        states.append(step_bank.BankState(f"scene{k}", np.concatenate([q, v]), 0.05 * k, None))
    return task, states


class Case:
    """one kernel family (tests/test_gpu_batch_ilqg.py's make_case families): the task, its environments, how the context is made"""

    def __init__(self, name, task, states, precision, kernel):
        self.name, self.task, self.states, self.precision, self.kernel = name, task, list(states), precision, kernel
        self.pm = task.packed_model(differentiable=True)
        self.limits = np.asarray(task.model.actuator_ctrlrange, float).reshape(-1, 2)

    def make_context(self):
        ctx = context(self.pm, step_bank.packed_task(self.task, self.states[0]), self.precision, {})
        assert self.kernel in ctx.kernel_name, ctx.kernel_name
        return ctx

    def mocap(self, e):
        s = self.states[e]
        return np.zeros(0) if s.mocap is None else np.asarray(s.mocap, float)

    def policy(self, envs, n, Tn, seed=5):
        """per environment: a nominal of Tn steps on its own clock around its own state, small gains and improvements, n steps"""
        m = self.task.model
        nq, nv, nu = m.nq, m.nv, m.nu
        dt = float(self.pm.struct.timestep)
        out = [[] for _ in range(6)]
        for e in envs:
            rng = np.random.default_rng(seed + 13 * e)    # (the environment's own policy, whatever its place in the fleet)
            s = self.states[e]
            times = s.time + dt * (np.arange(Tn) + 0.3)
            x = np.tile(s.state, (Tn, 1)) + 0.01 * rng.normal(size=(Tn, nq + nv))
            adr = np.asarray(m.arrays["jnt_qposadr"]).astype(int)
            for j, jt in enumerate(np.asarray(m.arrays["jnt_type"]).astype(int)):
                if jt in (0, 1):                           # free / ball: unit quaternions
                    a = adr[j] + (3 if jt == 0 else 0)
                    x[:, a:a + 4] /= np.linalg.norm(x[:, a:a + 4], axis=1, keepdims=True)
            lo, hi = self.limits.T
            alpha = np.concatenate([np.exp(np.linspace(0, np.log(1e-3), n - 1)), [0.0]]) if n > 1 else np.array([0.7])
            for k, v in enumerate((times, x, np.clip(0.1 * rng.normal(size=(Tn, nu)), lo, hi), 0.02 * rng.normal(size=(Tn, nu, 2 * nv)),
                                   0.02 * rng.normal(size=(Tn, nu)), alpha)):
                out[k].append(v)
        return [np.stack(v) for v in out]

    def rollout(self, ctx, envs, horizon=T, n=N_PER_ENV):
        """the nominal phase: the time policy with feedback, n rollouts per environment; nothing may fail"""
        ctx.set_states(np.stack([self.states[e].state for e in envs]), [self.states[e].time for e in envs],
                       np.stack([self.mocap(e) for e in envs]) if self.task.model.nmocap else None)
        ctx.rollout_feedback_batched(horizon, 1, 1, 1, *self.policy(envs, n, horizon))
        _, fail = ctx.returns()
        assert not fail.any(), (self.name, fail)

    def set_plain(self, ctx, e):
        s = self.states[0]
        if s.residual_int or s.residual_real:
            ctx.set_residual_state(s.residual_int, s.residual_real)
        ctx.set_state(self.states[e].state, self.states[e].time, self.mocap(e) if self.task.model.nmocap else None)


def make_case(name, task=None):
    if name.startswith("cartpole") or name.startswith("particle"):
        b = step_bank.lane_bank("Cartpole" if name.startswith("cartpole") else "Particle")
        return Case(name, task or b.task, b.states[:4], 64 if name.endswith("64") else 32, "rollout_lane")
    if name == "quad":
        b = step_bank.a1_bank()
        return Case(name, b.task, b.states[:4], 64, "rollout_quad_kernel")      # home and three trot states
    if name == "wave":
        task, states = scene_task()
        return Case(name, task, states, 64, "rollout_wave_kernel")
    raise KeyError(name)


class Reference:
    """the plain calls on environment e's fetched candidate: derivatives once per `centered`, the retry loop per regularisation"""

    def __init__(self, case, ctx, e, cand, steps, skip, eps, centered, n=N_PER_ENV):
        self.case, self.ctx, self.steps = case, ctx, steps
        self.tr = tr = ctx.fetch_trajectory(e * n + cand)
        case.set_plain(ctx, e)
        A, B, C, D = (np.asarray(x) for x in model_derivatives(ctx, tr, steps, skip, eps, centered))
        A[steps - 1] = 0; B[steps - 1] = 0; D[steps - 1] = 0
        self.A, self.B = A, B
        self.cx, self.cu, self.cxx, self.cxu, self.cuu = ctx.cost_derivatives(tr.residual[:steps], C, D)

    def backward(self, reg_type, use_limits, mu, rate, factor, min_reg, max_reg, max_iter):
        bp, mu, rate, retries = retry_loop(
            lambda r: self.ctx.backward_pass(r, reg_type, use_limits, self.A, self.B, self.cx, self.cu, self.cxx, self.cxu, self.cuu,
                                             self.tr.actions[:self.steps], self.case.limits), mu, rate, factor, min_reg, max_reg, max_iter)
        out = {k: getattr(self, k) for k in MATRICES}
        out.update({k: bp[k] for k in SWEEP + ("dV",)})
        out.update(status=int(bool(bp["ok"])), mu=mu, rate=rate, retries=retries, nominal_return=self.tr.total_return)
        return out


def assert_env_equal(got, e, ref, where):
    keys = MATRICES + SCALARS + (SWEEP if ref["status"] == 1 else ())
    for k in keys:
        g, r = np.asarray(got[k][e]), np.asarray(ref[k])
        assert np.array_equal(g, r), (where, k, float(np.abs(g.astype(float) - r.astype(float)).max()))
    assert all(np.all(np.isfinite(np.asarray(ref[k], float))) for k in MATRICES)


def compare_with_plain_calls(name, steps, skip):
    case = make_case(name)
    ctx = case.make_context()
    envs = [0, 1, 2]
    case.rollout(ctx, envs, horizon=steps)
    # (fp32 finite differences: a step of 1e-6 is a few units in the last place of the state and the derivatives come out as zeros)
    ev, eps = derivative_steps(steps, skip), 1e-6 if case.precision == 64 else 1e-3
    assert (len(ev) == steps) == (skip == 0)
    mu, rate = [1.0, 0.5, 2.0], [1.0, 0.5, 2.0]
    seen = set()
    for centered in (0, 1):
        refs = [Reference(case, ctx, e, CANDS[e], steps, skip, eps, centered) for e in envs]
        for reg_type in (0, 1, 2):
            for use_limits in (0, 1):
                got = ctx.ilqg_step_batched(CANDS, steps, ev, eps, centered, reg_type, use_limits, mu, rate, with_matrices=True, **REG)
                for e in envs:
                    ref = refs[e].backward(reg_type, use_limits, mu[e], rate[e], **REG)
                    assert_env_equal(got, e, ref, (name, centered, reg_type, use_limits, e))
                    assert ref["status"] == 1, (name, e, ref["status"])
                    # (the generic scene's only residual is a constant user sensor: its derivatives are compared, its gains are zero)
                    assert name == "wave" or np.abs(ref["K"]).max() > 0, (name, e)
                seen.add(tuple(np.round(got["K"].ravel(), 10)))
        # the environments are different problems
        assert len({tuple(np.round(got["A"][e].ravel(), 12)) for e in envs}) == E
    assert name == "wave" or len(seen) > 1                            # ... and the settings were not all the same computation
    ctx.close()


@pytest.mark.parametrize("name", ["cartpole64", "cartpole32", "particle64", "quad", "wave"])
def test_batched_step_equals_the_plain_calls(name):
    compare_with_plain_calls(name, T, 0)


@pytest.mark.parametrize("name", ["cartpole64", "particle32", "quad"])
def test_derivative_skip(name):
    compare_with_plain_calls(name, 12, 3)


@pytest.mark.parametrize("weight,reg_type,expect", [(-0.01, 0, (1, 5)), (-0.1, 1, (0, 8))])
def test_the_retry_loop_runs_in_the_kernel(weight, reg_type, expect):
    task = copy.copy(load_task("Cartpole"))
    task.weight = list(task.weight)
    task.weight[-1] = weight                                           # the control term: cuu = weight / T < 0
    case = make_case("cartpole64", task)
    ctx = case.make_context()
    envs, eps = [0, 1, 2], 1e-6
    case.rollout(ctx, envs)
    ev = derivative_steps(T, 0)
    reg = dict(REG, max_iter=8)
    mu, rate = [1e-6, 1.0, 1e-6], [1.0, 1.0, 1.0]
    got = ctx.ilqg_step_batched([2, 0, -1], T, ev, eps, 0, reg_type, 1, mu, rate, with_matrices=True, **reg)
    print(f"weight {weight} reg_type {reg_type}: status {got['status']} retries {got['retries']} mu {got['mu']} rate {got['rate']}")
    assert (int(got["status"][0]), int(got["retries"][0])) == expect
    assert got["status"][1] == 1 and got["retries"][1] == 0 and got["mu"][1] == 1.0 and got["rate"][1] == 1.0
    if expect[0] == 1:
        assert got["retries"][0] >= 1 and got["mu"][0] == 1e-6 * 2.0 ** 15 and got["rate"][0] == 32.0
    # the third environment takes no part: status -1 and nothing but zeros
    assert got["status"][2] == -1
    for k in MATRICES + SWEEP + ("dV", "mu", "rate", "retries", "nominal_return"):
        assert not np.any(got[k][2]), k
    for e in (0, 1):
        ref = Reference(case, ctx, e, [2, 0][e], T, 0, eps, 0).backward(reg_type, 1, mu[e], rate[e], **reg)
        assert_env_equal(got, e, ref, ("retry", weight, e))
    # ... and the other two equal their two-environment call bit for bit
    case.rollout(ctx, [0, 1])
    two = ctx.ilqg_step_batched([2, 0], T, ev, eps, 0, reg_type, 1, mu[:2], rate[:2], with_matrices=True, **reg)
    for k in MATRICES + SWEEP + SCALARS:
        assert np.array_equal(two[k], got[k][:2]), k
    # nobody takes part: nothing is launched, everything is zero
    none = ctx.ilqg_step_batched([-1, -1], T, ev, eps, 0, reg_type, 1, mu[:2], rate[:2], with_matrices=True, **reg)
    assert list(none["status"]) == [-1, -1] and not any(np.any(none[k]) for k in MATRICES + SWEEP + ("dV", "mu", "rate", "retries"))
    ctx.close()


@pytest.mark.parametrize("name", ["particle32", "quad"])
def test_environment_independence_and_determinism(name):
    case = make_case(name)
    ctx = case.make_context()
    envs, perm = [0, 1, 2, 3], [2, 0, 3, 1]
    cands, mu, rate = np.array([2, 0, 1, 1]), np.array([1.0, 0.5, 2.0, 1e-3]), np.array([1.0, 0.5, 2.0, 4.0])
    ev = derivative_steps(T, 0)
    call = lambda order: ctx.ilqg_step_batched(cands[order], T, ev, 1e-6, 0, 0, 1, mu[order], rate[order], with_matrices=True, **REG)
    # a plain backward pass on arbitrary well-posed inputs, before and after the batched calls
    rng = np.random.default_rng(3)
    n, m = 2 * case.task.model.nv, case.task.model.nu
    sym = lambda k: (lambda x: x @ x.transpose(0, 2, 1) / k + np.eye(k))(rng.normal(size=(T, k, k)))
    plain_args = (0.1, 0, 1, 0.1 * rng.normal(size=(T, n, n)), 0.1 * rng.normal(size=(T, n, m)), rng.normal(size=(T, n)), rng.normal(size=(T, m)),
                  sym(n), 0.1 * rng.normal(size=(T, n, m)), sym(m), np.zeros((T, m)), case.limits)
    before = ctx.backward_pass(*plain_args)
    case.rollout(ctx, envs)
    base, again = call(envs), call(envs)
    after = ctx.backward_pass(*plain_args)
    case.rollout(ctx, perm)
    got = call(perm)
    for k in MATRICES + SWEEP + SCALARS:
        assert np.array_equal(base[k], again[k]), (k, "two identical calls")
        assert np.array_equal(got[k], base[k][perm]), (k, "permuted")
    assert before["ok"] and after["ok"]
    for k in SWEEP + ("dV",):
        assert np.array_equal(before[k], after[k]), (k, "plain backward_pass around a batched call")
    ctx.close()


def test_refusals():
    case = make_case("cartpole64")
    ctx = case.make_context()
    envs = [0, 1, 2]
    ev = derivative_steps(T, 0)

    def call(cand=CANDS, steps=T, evaluate=ev, eps=1e-6, reg_type=0, mu=(1.0, 1.0, 1.0), rate=(1.0, 1.0, 1.0), factor=2.0, min_reg=1e-6,
             max_reg=1e6, max_iter=5, **kw):
        return ctx.ilqg_step_batched(cand, steps, evaluate, eps, 0, reg_type, 1, mu, rate, factor, min_reg, max_reg, max_iter, **kw)

    def refused(code, match, **kw):
        with pytest.raises(capi.MjpcxError, match=match) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value.code)

    refused(-5, "no rollout has been run")
    pol = case.policy([0], N_PER_ENV, T)
    case.set_plain(ctx, 0)
    ctx.rollout_feedback(T, 1, 1, 1, *[p[0] for p in pol])
    refused(-1, "not a batched one of 3 environments")                # the last rollout was a plain one
    case.rollout(ctx, envs)
    assert list(call()["status"]) == [1, 1, 1]
    refused(-1, "not a batched one of 2 environments", cand=[0, 0], mu=(1.0, 1.0), rate=(1.0, 1.0))
    refused(-1, r"candidate outside \[-1, n_per_env\) \(environment 1\)", cand=[0, N_PER_ENV, 0])
    refused(-1, r"candidate outside \[-1, n_per_env\) \(environment 2\)", cand=[0, 0, -2])
    refused(-1, "within the rollout's horizon", steps=1, evaluate=[0])
    refused(-1, "within the rollout's horizon", steps=T + 1, evaluate=derivative_steps(T + 1, 0))
    refused(-1, "evaluate list must be strictly increasing", evaluate=[0, 5, 5, T - 1])
    refused(-1, "evaluate list must be strictly increasing", evaluate=[0, 7, 3])
    refused(-1, "evaluate list must be strictly increasing", evaluate=[0, T])
    refused(-1, "evaluate list must be strictly increasing", evaluate=[-1, 3])
    refused(-1, "num_eval outside", evaluate=[])
    refused(-1, "epsilon must be > 0", eps=0.0)
    refused(-1, "unknown regularization type", reg_type=3)
    refused(-1, "unknown regularization type", reg_type=-1)
    refused(-1, r"max_iter outside \[1, 64\]", max_iter=0)
    refused(-1, r"max_iter outside \[1, 64\]", max_iter=65)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(-1, r"mu and rate must be finite and > 0 \(environment 1\)", mu=(1.0, bad, 1.0))
        refused(-1, r"mu and rate must be finite and > 0 \(environment 2\)", rate=(1.0, 1.0, bad))
        refused(-1, "factor must be finite and > 0", factor=bad)
    for kw in (dict(min_reg=np.nan), dict(max_reg=np.inf), dict(min_reg=-np.inf), dict(min_reg=2.0, max_reg=1.0)):
        refused(-1, "min_reg and max_reg must be finite, min_reg <= max_reg", **kw)
    with pytest.raises(ValueError, match="3 candidates, 2 mu"):
        call(mu=(1.0, 1.0))
    # beyond the kernels' limits: T = 513 steps
    ctx.set_states(np.stack([case.states[e].state for e in envs]), [case.states[e].time for e in envs])
    ctx.rollout_feedback_batched(513, 1, 1, 1, *case.policy(envs, 1, 513))
    refused(-2, r"covers n <= 48, m <= 16, T <= 512", cand=[0, 0, 0], steps=513, evaluate=derivative_steps(513, 0))
    ctx.close()
    # beyond the backward pass's n <= 48: tests/models/capsules_tendon.xml has 2 nv = 64 (the refusal comes before any launch of the call)
    fm = mjcf.load_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "capsules_tendon.xml"))
    assert 2 * fm.nv == 64
    big = Case("wave", Task(name="scene", residual_id=0, model=fm).reset(),
               [step_bank.BankState(f"scene{k}", np.concatenate([fm.arrays["qpos0"], np.zeros(fm.nv)]), 0.05 * k, None) for k in range(3)], 64,
               "rollout_wave_kernel")
    ctx = big.make_context()
    ctx.set_states(np.stack([s.state for s in big.states]), [s.time for s in big.states])
    ctx.rollout_feedback_batched(T, 1, 1, 1, *big.policy(envs, N_PER_ENV, T))
    refused(-2, r"covers n <= 48, m <= 16, T <= 512")
    ctx.close()
    # fp32 contexts of the wavefront-per-candidate family: refused as the plain transition_fd refuses them
    quad = make_case("quad")
    quad.precision, quad.kernel = 32, "rollout_"
    ctx = quad.make_context()
    ctx.set_states(np.stack([quad.states[e].state for e in envs]), [quad.states[e].time for e in envs], np.stack([quad.mocap(e) for e in envs]))
    ctx.rollout_splines_batched(T, capi.SPLINE_ZERO, np.tile(np.linspace(0, 0.1, 3), (E, 1)), np.zeros((E, 64, 3, quad.task.model.nu)), num_envs=E,
                                n_per_env=64)
    with pytest.raises(capi.MjpcxError, match="fp64 only") as e:
        call()
    assert e.value.code == -2
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- the planner
PT = 12


def planner_fleet(name):
    """tests/test_gpu_batch_ilqg.py's fleets: the task and three States"""
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


def fleet_planner(task, device_chain):
    p = GpuBatchILQGPlanner(E)
    p.initialize(task.model, task)
    p.allocate()
    p.reset(PT)
    p.device_chain = device_chain
    return p


def assert_members_equal(b, p, where):
    assert b.winner == p.winner and b.action_step == p.action_step and b.feedback_scaling == p.feedback_scaling, where
    assert b.regularization == p.regularization and b.regularization_rate == p.regularization_rate, where
    assert b.iteration_completed == p.iteration_completed, where
    assert np.array_equal(b.dV, p.dV) and b.improvement == p.improvement and b.expected == p.expected and b.surprise == p.surprise, (where, b.dV, p.dV)
    for pb, pp in ((b.policy, p.policy), (b.previous_policy, p.previous_policy), (b.candidate0, p.candidate0)):
        assert pb.trajectory.total_return == pp.trajectory.total_return and pb.trajectory.failure == pp.trajectory.failure, where
        for k in ("states", "actions", "times", "residual", "costs", "trace"):
            assert np.array_equal(getattr(pb.trajectory, k)[:PT], getattr(pp.trajectory, k)[:PT]), (where, k)
        assert np.array_equal(pb.feedback_gain[:PT], pp.feedback_gain[:PT]), where
        assert np.array_equal(pb.action_improvement[:PT], pp.action_improvement[:PT]), where
        assert pb.feedback_scaling == pp.feedback_scaling, where


@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_planner_with_the_device_chain_equals_the_sequential_middle(name):
    task, states = planner_fleet(name)
    chain, plain = fleet_planner(task, None), fleet_planner(task, False)
    nq = task.model.nq
    for step in range(2):
        for p in (chain, plain):
            p.set_states(states)
            p.optimize_policy(PT)
        assert chain.used_device_chain and not plain.used_device_chain
        assert chain.sat_out == plain.sat_out and not any(chain.sat_out), (step, chain.sat_out, plain.sat_out)
        for e in range(E):
            assert_members_equal(chain.envs[e], plain.envs[e], (name, step, e))
            assert chain.envs[e].iteration_completed
        assert chain.timers["cost_derivative"] == 0 and chain.timers["backward_pass"] == 0 and chain.timers["model_derivative"] > 0
        for e in range(E):                                            # every environment advances along its own best trajectory
            tr = plain.best_trajectory(e)
            mp = states[e].mocap.reshape(-1, 7)
            states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None, mocap_quat=mp[:, 3:] if len(mp) else None,
                          time=float(tr.times[2]))
    chain.ctx.close()
    plain.ctx.close()
