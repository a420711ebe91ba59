"""-m gpu: several environments in one launch (mjpcx_set_states, mjpcx_rollout_*_batched, mjpcx_best_batched) on every rollout kernel.

A batched call of E environments is compared (1) bit for bit with E plain calls on the same context -- returns, failure flags and all
six Trajectory buffers of EVERY candidate -- with seeds s + e, and (2) with the oracle, per environment, at the tolerance the kernel
family's own suite asserts:
  lane kernels, fp64              1e-9 (1 + |x|)   tests/test_gpu_parity.py (TOL)
  quad kernel's own candidates    1e-9             tests/test_gpu_quad.py:1-4
  candidates it hands on, the
  tree and the wave kernels       1e-6             tests/test_gpu_quad.py:1-4, tests/test_gpu_humanoid.py (1e-7 on 60 steps of the scene)
  limb kernel fp64, 40 steps      1e-8             tests/test_gpu_limb.py (test_rollout_longer_than_the_spline_on_both_sides, H = 40)
  fp32, returns                   2e-3             README.md (Parity), tests/test_gpu_limb.py::test_walk_fp32_returns
States come from tests/step_bank.py. The A1 bank holds no three states of equal frozen residual state (mode, gait and mode start are
spread over it), so the cases that do not call set_residual_states give all three environments the residual state of the first one
through the plain set_residual_state; the oracle is given the same. The Humanoid's three states are the keys of one clip: equal
residual state, three clocks, three reference frames."""
import os

import numpy as np
import pytest

import step_bank
from batch_oracle_backend import BatchOracleContext
from mujoco_mpc_amd import capi, mjcf
from mujoco_mpc_amd.planners import GpuBatchSamplingPlanner, State
from mujoco_mpc_amd.task import Task, load_task
from oracle import pyoracle

pytestmark = pytest.mark.gpu
FIELDS = ("states", "actions", "times", "residual", "costs", "trace")
E, H, P, SEED = 3, 40, 4, 31
HANDED_ON = 0x40000000   # failure[] marker of a candidate the quad / limb kernel handed on (kept under MJPCX_*_NO_FALLBACK)


def err(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    e = np.abs(a - b) / (1 + np.abs(b))
    return float(np.max(np.where(np.isnan(e), np.inf, e))) if e.size else 0.0


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


class Case:
    """one kernel family: the task, three states, how the context is made and what it must be running"""

    def __init__(self, name, task, states, precision, n, env, kernel, std, tol, tol_handed=None, per_env_residual=False, returns_only=False):
        self.name, self.task, self.states, self.precision, self.n, self.env, self.kernel = name, task, states, precision, n, env, kernel
        self.std, self.tol, self.tol_handed = std, tol, tol_handed if tol_handed is not None else tol
        self.per_env_residual, self.returns_only = per_env_residual, returns_only
        m = task.model
        self.pm = task.packed_model()
        dt = m.get_number("agent_timestep", m.timestep)
        rng = np.random.default_rng(3)
        self.times = np.stack([s.time + np.arange(P) * ((H - 1) * dt / (P - 1)) for s in states])     # every environment's own clock
        lo, hi = np.asarray(m.arrays["actuator_ctrlrange"], float).reshape(-1, 2).T
        self.nominal = np.clip(rng.normal(0, 0.05, (len(states), P, m.nu)), lo, hi)                    # ... and nominal spline
        self.shared = states[0]

    def residual_of(self, e):
        return self.states[e] if self.per_env_residual else self.shared

    def packed(self, e):
        return step_bank.packed_task(self.task, self.residual_of(e))

    def mocap(self, e):
        s = self.states[e]
        return np.zeros(0) if s.mocap is None else np.asarray(s.mocap, float)

    def noise(self, e=0):
        return capi.make_noise_spec(seed=SEED + e, iteration=2, mode=capi.NOISE_SAMPLING, std0=self.std)

    def make_context(self, extra=None):
        ctx = context(self.pm, self.packed(0), self.precision, dict(self.env, **(extra or {})))
        assert self.kernel in ctx.kernel_name, ctx.kernel_name
        return ctx

    def set_shared_residual(self, ctx):
        s = self.shared
        if s.residual_int or s.residual_real:
            ctx.set_residual_state(s.residual_int, s.residual_real)

    def run_batched(self, ctx, envs):
        ctx.set_states(np.stack([self.states[e].state for e in envs]), [self.states[e].time for e in envs],
                       np.stack([self.mocap(e) for e in envs]) if self.task.model.nmocap else None)
        if self.per_env_residual:
            ctx.set_residual_states(np.array([self.states[e].residual_int for e in envs], np.int32),
                                    np.array([self.states[e].residual_real for e in envs], float))
        else:
            self.set_shared_residual(ctx)
        ctx.rollout_noise_batched(self.n, H, capi.SPLINE_CUBIC, self.times[envs], self.nominal[envs], self.noise(envs[0]), num_envs=len(envs))

    def run_single(self, ctx, e):
        s = self.states[e]
        r = self.residual_of(e)
        if r.residual_int or r.residual_real:
            ctx.set_residual_state(r.residual_int, r.residual_real)
        ctx.set_state(s.state, s.time, self.mocap(e) if self.task.model.nmocap else None)
        ctx.rollout_noise(self.n, H, capi.SPLINE_CUBIC, self.times[e], self.nominal[e], self.noise(e))

    def oracle(self, e):
        nodes = pyoracle.noise_candidates(self.pm, self.noise(e), P, self.nominal[e], np.arange(self.n))
        s = self.states[e]
        return pyoracle.rollout_batch(self.pm, self.packed(e), s.state, s.time, self.mocap(e), self.n, H, P, capi.SPLINE_CUBIC, self.times[e],
                                      nodes, num_threads=16)


def scene_task():
    fm = mjcf.load_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "capsules_tendon.xml"))
    task = Task(name="scene", residual_id=0, model=fm).reset()
    states = []
    for k in range(E):   # (tests/test_gpu_humanoid.py::test_contact_feature_scene's state, varied)
        q, v = fm.arrays["qpos0"].copy(), np.zeros(fm.nv)
        q[14 + 2] = 1.0 + 0.0995 - 0.002 * k
        v[12 + 2] = -0.5 + 0.1 * k
        q[fm.nq - 2] = 0.6 - 0.1 * k
        v[0] = 0.3 + 0.2 * k
        states.append(step_bank.BankState(f"scene{k}", np.concatenate([q, v]), 0.05 * k, None))
    return task, states


def make_case(name):
    a1_env = {"MJPCX_QUAD_MIN_N": "0"}
    if name.startswith("cartpole") or name.startswith("particle"):
        task_name = "Cartpole" if name.startswith("cartpole") else "Particle"
        b = step_bank.lane_bank(task_name)
        p = 64 if name.endswith("64") else 32
        return Case(name, b.task, b.states[:E], p, 64 if task_name == "Cartpole" else 128, {}, "rollout_lane", 0.1, 1e-9 if p == 64 else 2e-3,
                    returns_only=p == 32)
    if name == "quad":       # the quad kernel; MJPCX_QUAD_CON_CAP=<n> hands on every candidate one of whose legs collects more than n contacts
        b = step_bank.a1_bank()
        return Case(name, b.task, b.states[:E], 64, 64, dict(a1_env, MJPCX_QUAD_CON_CAP="1"), "rollout_quad_kernel", 0.06, 1e-9, 1e-6)
    if name == "quad_residual":   # three modes (Quadruped, Biped, Walk) and mode start times through set_residual_states
        b = step_bank.a1_bank()
        return Case(name, b.task, b.states[:E], 64, 64, a1_env, "rollout_quad_kernel", 0.06, 1e-9, 1e-6, per_env_residual=True)
    if name == "tree_a1":
        b = step_bank.a1_bank()
        return Case(name, b.task, b.states[:E], 64, 64, {"MJPCX_NO_QUAD": "1"}, "rollout_tree_kernel<A1>", 0.06, 1e-6)
    if name.startswith("limb"):
        b = step_bank.humanoid_bank()
        st = [s for s in b.states if s.label.startswith("clip9/key")]
        assert len(st) == E and all(s.residual_int == st[0].residual_int and s.residual_real == st[0].residual_real for s in st)
        p = 64 if name.endswith("64") else 32
        return Case(name, b.task, st, p, 64, {"MJPCX_LIMB_MIN_N": "0"}, "rollout_limb_kernel", 0.05, 1e-8 if p == 64 else 2e-3, 1e-6 if p == 64 else 2e-3,
                    returns_only=p == 32)
    if name == "wave":
        task, states = scene_task()
        return Case(name, task, states, 64, 64, {}, "rollout_wave_kernel", 0.2, 1e-6)
    raise KeyError(name)


CASES = ["cartpole64", "cartpole32", "particle64", "particle32", "quad", "quad_residual", "tree_a1", "limb32", "limb64", "wave"]


def handed_on_mask(case):
    """which candidates of the batched run the quad / limb kernel handed on: the same launch with the hand-on pass switched off"""
    if not ("quad" in case.name or "limb" in case.name):
        return None
    ctx = case.make_context({"MJPCX_QUAD_NO_FALLBACK": "1", "MJPCX_LIMB_NO_FALLBACK": "1"})
    case.run_batched(ctx, list(range(E)))
    ctx.returns()
    mask = (ctx.failure_raw & HANDED_ON) != 0
    ctx.close()
    return mask


@pytest.mark.parametrize("name", CASES)
def test_batched_equals_sequential_and_the_oracle(name):
    case = make_case(name)
    n = case.n
    handed = handed_on_mask(case)
    if name == "quad":   # the smallest cap that splits the batch (as tests/test_gpu_quad.py::test_handed_on_candidates_come_back_from_the_other_kernel)
        for cap in (2, 3, 4, 5, 6, 8):
            case.env["MJPCX_QUAD_CON_CAP"] = str(cap)
            handed = handed_on_mask(case)
            if 0 < handed.sum() < E * n:
                break
        assert 0 < handed.sum() < E * n, int(handed.sum())   # both the kernel's own candidates and its hand-on are in the comparison
    ctx = case.make_context()
    case.run_batched(ctx, list(range(E)))
    got = everything(ctx)
    assert ctx.N == E * n
    # ---- bit for bit: E plain calls with seeds s + e on the same context (the same kernel: the thresholds are pinned)
    for e in range(E):
        case.run_single(ctx, e)
        one = everything(ctx)
        for k in ("total_return", "failure") + FIELDS:
            assert np.array_equal(got[k][e * n:(e + 1) * n], one[k], equal_nan=True), (name, e, k)
    # ---- E = 1 batched against the plain call (environment 1: its own clock and nominal)
    case.run_batched(ctx, [1])
    alone = everything(ctx)
    for k in ("total_return", "failure") + FIELDS:
        assert np.array_equal(alone[k], got[k][n:2 * n], equal_nan=True), (name, "E = 1", k)
    ctx.close()
    # the environments are different problems
    assert not np.array_equal(got["states"][:n], got["states"][n:2 * n])
    # ---- the oracle, per environment, every candidate
    worst = {}
    for e in range(E):
        ref = case.oracle(e)
        sl = slice(e * n, (e + 1) * n)
        assert np.array_equal(got["failure"][sl] != 0, ref["failure"] != 0), (name, e)
        assert not ref["failure"].any(), (name, e)   # (the oracle completes these rollouts: chosen so on the CPU)
        tol = np.where(handed[sl], case.tol_handed, case.tol) if handed is not None else np.full(n, case.tol)
        for k in ("total_return",) + (() if case.returns_only else FIELDS):
            for c in range(n):
                d = err(got[k][sl][c], ref[k][c])
                worst[k] = max(worst.get(k, 0.0), d / tol[c])
                assert d <= tol[c], (name, e, c, k, d, float(tol[c]))
    print(f"{name}: worst error / tolerance by buffer {worst}; handed on {None if handed is None else int(handed.sum())} of {E * n}")


@pytest.mark.parametrize("name", ["cartpole64", "quad"])
def test_segmented_best(name):
    case = make_case(name)
    n = case.n
    ctx = case.make_context()
    case.run_batched(ctx, list(range(E)))
    ret, _ = ctx.returns()
    idx, best, ref, sp = ctx.best_batched(E, 0)
    for e in range(E):
        r = ret[e * n:(e + 1) * n]
        assert idx[e] == int(np.argmin(r)) and best[e] == r[idx[e]]
        assert ref[e] == ctx.return_of(e * n)
        assert np.array_equal(sp[e], ctx.fetch_spline(e * n + int(idx[e])))
    assert np.all(np.isnan(ctx.best_batched(E, -1)[2]))
    # a constructed tie: every candidate of an environment is the same spline from the same state -> equal returns, the lower index wins
    s = case.states[0]
    ctx.set_states(np.stack([s.state] * E), [s.time] * E, np.stack([case.mocap(0)] * E) if case.task.model.nmocap else None)
    values = np.broadcast_to(case.nominal[0], (E, n, P, case.task.model.nu)).copy()
    values[1, :5] *= 0.5      # environment 1: candidates 0..4 differ from the rest
    ctx.rollout_splines_batched(H, capi.SPLINE_CUBIC, np.stack([case.times[0]] * E), values, num_envs=E, n_per_env=n)
    ret, _ = ctx.returns()
    idx, best, ref, sp = ctx.best_batched(E, 0)
    for e in range(E):
        r = ret[e * n:(e + 1) * n]
        assert len(set(r[5:].tolist())) == 1                       # the tie is real
        assert idx[e] == int(np.argmin(r)) and best[e] == r[idx[e]]  # numpy.argmin takes the first of equal minima
    assert idx[0] == 0 and idx[2] == 0 and idx[1] in (0, 5)
    ctx.close()


def _states(task, bank_states):
    out = []
    for s in bank_states:
        st = State(task.model)
        m = task.model
        mp = None if s.mocap is None else np.asarray(s.mocap, float).reshape(-1, 7)
        st.set(s.state[:m.nq], s.state[m.nq:], mocap_pos=None if mp is None else mp[:, :3], mocap_quat=None if mp is None else mp[:, 3:], time=s.time)
        out.append(st)
    return out


@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_batch_planner_on_the_device_against_the_oracle_backend(name):
    """GpuBatchSamplingPlanner, E = 3, three plan steps: the device and the oracle backend pick the same winners and end with policies within 1e-9"""
    if name == "Cartpole":
        task, bank_states, horizon = load_task("Cartpole"), step_bank.lane_bank("Cartpole").states[:E], 30
    else:
        b = step_bank.a1_bank()
        task, bank_states, horizon = b.task, b.states[:E], 20
        task.residual_int, task.residual_real = list(bank_states[0].residual_int), list(bank_states[0].residual_real)
    old = os.environ.get("MJPCX_QUAD_MIN_N")
    os.environ["MJPCX_QUAD_MIN_N"] = "0"
    try:
        dev = GpuBatchSamplingPlanner(E, seed=9)
        ref = GpuBatchSamplingPlanner(E, seed=9, backend_factory=lambda t: BatchOracleContext(t, threads=16))
        for p in (dev, ref):
            p.initialize(task.model, task)
            p.num_trajectory_ = 64
            if name == "QuadrupedFlat":
                for q in p.envs:
                    q.noise_exploration = [0.05, 0.0]
            p.allocate()
            p.reset(horizon)
    finally:
        if old is None:
            os.environ.pop("MJPCX_QUAD_MIN_N", None)
        else:
            os.environ["MJPCX_QUAD_MIN_N"] = old
    states = _states(task, bank_states)
    nq = task.model.nq
    for step in range(3):
        for p in (dev, ref):
            p.set_states(states)
            p.optimize_policy(horizon)
        assert dev.winners == ref.winners, (step, dev.winners, ref.winners)
        for e in range(E):
            assert err(dev.envs[e].policy.plan.values(), ref.envs[e].policy.plan.values()) <= 1e-9, (step, e)
            assert err(dev.envs[e].policy.plan.times(), ref.envs[e].policy.plan.times()) <= 1e-9
        for e in range(E):   # every environment moves two steps along the oracle's best trajectory
            tr = ref.best_trajectory(e)
            mp = states[e].mocap.reshape(-1, 7)
            states[e].set(tr.states[2, :nq], tr.states[2, nq:], mocap_pos=mp[:, :3] if len(mp) else None, mocap_quat=mp[:, 3:] if len(mp) else None,
                          time=float(tr.times[2]))
    tb = dev.best_trajectory(1)
    assert err(tb.states, ref.best_trajectory(1).states) <= 1e-6
    dev.ctx.close()


def test_validation():
    case = make_case("cartpole64")
    ctx = case.make_context()
    st = np.stack([s.state for s in case.states])
    tm = [s.time for s in case.states]
    ns = case.noise()

    def refused(fn, code=-1):
        with pytest.raises(capi.MjpcxError) as ei:
            fn()
        assert ei.value.code == code, ei.value
        return str(ei.value)

    # no set_states yet
    assert "set_states" in refused(lambda: ctx.rollout_noise_batched(64, H, 2, case.times, case.nominal, ns, num_envs=E))
    ctx.set_states(st, tm)
    assert "multiple of 64" in refused(lambda: ctx.rollout_noise_batched(96, H, 2, case.times, case.nominal, ns, num_envs=E))
    refused(lambda: ctx.rollout_noise_batched(64, H, 2, case.times, case.nominal, ns, num_envs=0))
    refused(lambda: ctx.rollout_noise_batched(64, H, 2, case.times[:2], case.nominal[:2], ns, num_envs=2))   # E other than the last set_states
    refused(lambda: capi.Context.set_states(ctx, np.zeros((0, ctx.dim_state)), []))
    refused(lambda: ctx.rollout_splines_batched(H, 2, case.times, np.zeros((E, 96, P, 1)), num_envs=E, n_per_env=96))
    # the context still serves a plain call, and its result is the one of a fresh context
    case.run_single(ctx, 0)
    ret, fail = ctx.returns()
    refused(lambda: ctx.best_batched(E, 0))   # (the last rollout was not a batched one)
    fresh = case.make_context()
    case.run_single(fresh, 0)
    ret2, fail2 = fresh.returns()
    assert np.array_equal(ret, ret2) and np.array_equal(fail, fail2)
    # ... and a batched one after that
    case.run_batched(ctx, list(range(E)))
    assert ctx.returns()[0].shape == (E * 64,)
    ctx.close(); fresh.close()
