"""-m gpu: mjpcx_ilqg_step_batched_from -- iLQG's derivative chain and backward pass for a fleet whose nominals lie in two contexts -- and
GpuBatchILQSPlanner on the device.

   mjpcx_ilqg_step_batched_from <-> mjpcx_fetch_trajectory from the context each environment names, fed through the plain calls of
       tests/test_gpu_batch_ilqg_step.py (set_state -> transition_fd -> zeroed last step -> cost_derivatives -> the retry loop over
       backward_pass): every output np.array_equal. The source context holds a batched SPLINE rollout of 64 candidates per environment
       (candidates 5, 0, 63: inside, first and last lane of a wavefront), the own context a feedback rollout of 3 per environment -- two
       batch sizes, two kernels and, on the A1, whichever layouts they leave. Patterns: [1, 0, 1]; all 1 on a context that has only had
       set_states; all 0, which is mjpcx_ilqg_step_batched whatever the source; a rider ([-1, 1, 0]) that rides on a source nominal.
       Lane family in both precisions, the quad kernel's A1, a generic contact model; T = 8, and T = 12 with derivative_skip 3.
   permuting the environments permutes the outputs; two calls give the same bits; source == ctx
   every refusal by code and message. Not exercised: a sharded context, which needs two ranks.
   GpuBatchILQSPlanner with the device chain <-> device_chain = False, exactly, on the two fleets of tests/test_batch_ilqs_planner.py
       (no pattern is asserted on the Cartpole fleet: a gap of 4e-6 between two returns may fall the other way on the device), and
       <-> three single GpuILQSPlanners on the Particle fleet, exactly: a batched launch equals E plain ones and the step call equals
       the plain chain, bit for bit, on the lane family."""
import numpy as np
import pytest

import test_batch_ilqs_planner as tb
import test_gpu_batch_ilqg_step as ts
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchILQSPlanner, GpuILQSPlanner, derivative_steps, model_derivatives
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
E, N_SRC, N_OWN = 3, 64, ts.N_PER_ENV
SRC, OWN = [5, 0, 63, 17], [2, 0, 1, 2]
KEYS = ts.MATRICES + ts.SWEEP + ts.SCALARS
REG = ts.REG


def source_rollout(case, src, envs, horizon):
    """the sampling side: 64 small splines per environment, seeded by the environment whatever its place in the fleet; nothing may fail"""
    m = case.task.model
    lo, hi = case.limits.T
    dt = float(case.pm.struct.timestep)
    times = np.stack([case.states[e].time + np.linspace(0.0, dt * horizon, 3) for e in envs])
    values = np.stack([np.clip(0.1 * np.random.default_rng(71 + 13 * e).normal(size=(N_SRC, 3, m.nu)), lo, hi) for e in envs])
    src.set_states(np.stack([case.states[e].state for e in envs]), [case.states[e].time for e in envs],
                   np.stack([case.mocap(e) for e in envs]) if m.nmocap else None)
    src.rollout_splines_batched(horizon, capi.SPLINE_LINEAR, times, values, num_envs=len(envs), n_per_env=N_SRC)
    _, fail = src.returns()
    assert not fail.any(), (case.name, fail)


def only_states(case, ctx, envs):
    ctx.set_states(np.stack([case.states[e].state for e in envs]), [case.states[e].time for e in envs],
                   np.stack([case.mocap(e) for e in envs]) if case.task.model.nmocap else None)


class Ref(ts.Reference):
    """ts.Reference on a trajectory fetched from whichever context; the plain calls run on `ctx`"""

    def __init__(self, case, ctx, tr, e, steps, skip, eps, centered):
        self.case, self.ctx, self.steps, self.tr = case, ctx, steps, tr
        case.set_plain(ctx, e)
        A, B, C, D = (np.asarray(x) for x in model_derivatives(ctx, tr, steps, skip, eps, centered))
        A[steps - 1] = 0; B[steps - 1] = 0; D[steps - 1] = 0
        self.A, self.B = A, B
        self.cx, self.cu, self.cxx, self.cxu, self.cuu = ctx.cost_derivatives(tr.residual[:steps], C, D)


def assert_no_part(got, e, where):
    assert got["status"][e] == -1, where
    for k in ts.MATRICES + ts.SWEEP + ("dV", "mu", "rate", "retries", "nominal_return"):
        assert not np.any(got[k][e]), (where, k)


def compare_with_plain_calls(name, steps, skip):
    case = ts.make_case(name)
    ctx, src, bare = case.make_context(), case.make_context(), case.make_context()
    envs = [0, 1, 2]
    source_rollout(case, src, envs, steps)
    case.rollout(ctx, envs, horizon=steps)
    only_states(case, bare, envs)
    ev, eps = derivative_steps(steps, skip), 1e-6 if case.precision == 64 else 1e-3
    mu, rate = [1.0, 0.5, 2.0], [1.0, 0.5, 2.0]
    from_src = [src.fetch_trajectory(e * N_SRC + SRC[e]) for e in envs]
    from_own = [ctx.fetch_trajectory(e * N_OWN + OWN[e]) for e in envs]
    # six different nominals (by their actions: the generic scene's only residual is a constant user sensor, every return is 0)
    assert len({tr.actions[:steps].tobytes() for tr in from_src + from_own}) == 2 * E
    for centered, reg_type, use_limits in ((1, 0, 1), (0, 2, 0)):
        setting = (steps, ev, eps, centered, reg_type, use_limits, mu, rate)
        refs = {}
        for which, trs in ((1, from_src), (0, from_own)):
            for e in envs:
                refs[which, e] = Ref(case, ctx, trs[e], e, steps, skip, eps, centered).backward(reg_type, use_limits, mu[e], rate[e], **REG)
                assert refs[which, e]["status"] == 1, (name, which, e)
        call = lambda c, source, frm, cand: c.ilqg_step_batched_from(source, frm, cand, *setting, with_matrices=True, **REG)
        # a mixed fleet
        frm = [1, 0, 1]
        got = call(ctx, src, frm, [SRC[0], OWN[1], SRC[2]])
        for e in envs:
            ts.assert_env_equal(got, e, refs[frm[e], e], (name, "mixed", centered, e))
        # everybody on the source; this context has only had set_states
        got = call(bare, src, [1, 1, 1], SRC[:E])
        for e in envs:
            ts.assert_env_equal(got, e, refs[1, e], (name, "all from the source", centered, e))
        # nobody on the source: mjpcx_ilqg_step_batched, whatever the source
        plain = ctx.ilqg_step_batched(OWN[:E], *setting, with_matrices=True, **REG)
        for source in (src, None, bare):
            got = call(ctx, source, [0, 0, 0], OWN[:E])
            for k in KEYS:
                assert np.array_equal(got[k], plain[k]), (name, "all own", k)
        for e in envs:
            ts.assert_env_equal(plain, e, refs[0, e], (name, "all own", centered, e))
        # a rider on a source nominal
        got = call(ctx, src, [0, 1, 0], [-1, SRC[1], OWN[2]])
        assert_no_part(got, 0, (name, "rider"))
        ts.assert_env_equal(got, 1, refs[1, 1], (name, "rider", centered, 1))
        ts.assert_env_equal(got, 2, refs[0, 2], (name, "rider", centered, 2))
        got = call(ctx, src, [1, 1, 0], [-1, SRC[1], OWN[2]])                       # (what from_source says of a rider means nothing)
        assert_no_part(got, 0, (name, "rider"))
        ts.assert_env_equal(got, 1, refs[1, 1], (name, "rider", centered, 1))
    for c in (ctx, src, bare):
        c.close()


@pytest.mark.parametrize("name", ["cartpole64", "particle32", "quad", "wave"])
def test_step_from_two_contexts_equals_the_plain_calls(name):
    compare_with_plain_calls(name, ts.T, 0)


@pytest.mark.parametrize("name", ["cartpole64", "particle32", "quad"])
def test_derivative_skip(name):
    compare_with_plain_calls(name, 12, 3)


@pytest.mark.parametrize("name", ["particle32", "quad"])
def test_environment_independence_and_determinism(name):
    case = ts.make_case(name)
    ctx, src = case.make_context(), case.make_context()
    envs, perm = [0, 1, 2, 3], [2, 0, 3, 1]
    frm = np.array([1, 0, 1, 0])
    cands, mu, rate = np.where(frm == 1, SRC, OWN), np.array([1.0, 0.5, 2.0, 1e-3]), np.array([1.0, 0.5, 2.0, 4.0])
    ev, eps = derivative_steps(ts.T, 0), 1e-6 if case.precision == 64 else 1e-3
    call = lambda order: ctx.ilqg_step_batched_from(src, frm[order], cands[order], ts.T, ev, eps, 0, 0, 1, mu[order], rate[order],
                                                    with_matrices=True, **REG)
    source_rollout(case, src, envs, ts.T)
    case.rollout(ctx, envs)
    base, again = call(envs), call(envs)
    source_rollout(case, src, perm, ts.T)
    case.rollout(ctx, perm)
    got = call(perm)
    for k in KEYS:
        assert np.array_equal(base[k], again[k]), (k, "two identical calls")
        assert np.array_equal(got[k], base[k][perm]), (k, "permuted")
    assert list(base["status"]) == [1] * 4 and len({float(x) for x in base["nominal_return"]}) == 4
    # source == ctx: the selector picks the same buffers
    own = ctx.ilqg_step_batched(np.asarray(OWN)[perm], ts.T, ev, eps, 0, 0, 1, mu[perm], rate[perm], with_matrices=True, **REG)
    same = ctx.ilqg_step_batched_from(ctx, frm[perm], np.asarray(OWN)[perm], ts.T, ev, eps, 0, 0, 1, mu[perm], rate[perm], with_matrices=True, **REG)
    for k in KEYS:
        assert np.array_equal(own[k], same[k]), (k, "source == ctx")
    ctx.close()
    src.close()


def test_refusals():
    case = ts.make_case("cartpole64")
    ctx, src = case.make_context(), case.make_context()
    envs, T = [0, 1, 2], ts.T
    ev = derivative_steps(T, 0)

    def call(c=ctx, source=src, frm=(1, 0, 1), cand=(5, 0, 63), steps=T, evaluate=ev, mu=(1.0, 1.0, 1.0), rate=(1.0, 1.0, 1.0)):
        return c.ilqg_step_batched_from(source, frm, cand, steps, evaluate, 1e-6, 0, 0, 1, mu, rate, **REG)

    def refused(code, match, **kw):
        with pytest.raises(capi.MjpcxError, match=match) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value.code)
        assert "mjpcx_ilqg_step_batched_from: " in str(e.value) or code == -5, str(e.value)   # every refusal of its own names the call

    # the context the call runs on: states first; a rollout of its own only where somebody names it
    refused(-1, "mjpcx_ilqg_step_batched_from: before mjpcx_set_states", frm=(1, 1, 1))
    only_states(case, ctx, [0, 1])
    refused(-1, "3 environments after mjpcx_set_states of 2", frm=(1, 1, 1))
    only_states(case, ctx, envs)
    refused(-1, "the source's last rollout was not a batched one of 3 environments", frm=(1, 1, 1))   # the source has no rollout at all
    source_rollout(case, src, envs, T)
    assert list(call(frm=(1, 1, 1))["status"]) == [1, 1, 1]
    refused(-1, "the last rollout was not a batched one of 3 environments")   # environment 1 names this context, which has none
    refused(-5, "no rollout has been run", frm=(0, 0, 0), cand=(2, 0, 1))    # nobody names the source: mjpcx_ilqg_step_batched's refusal
    case.rollout(ctx, envs)
    assert list(call()["status"]) == [1, 1, 1]
    # the arguments of the selector
    refused(-1, "from_source names a source, but source is NULL", source=None)
    refused(-1, r"from_source must be 0 or 1 \(environment 1\)", frm=(1, 2, 1))
    refused(-1, r"from_source must be 0 or 1 \(environment 2\)", frm=(0, 0, -1))
    with pytest.raises(ValueError, match="2 from_source entries for 3 environments"):
        call(frm=(1, 0))
    # candidates: each within the context its environment names
    refused(-1, r"candidate outside \[-1, n_per_env\) \(environment 0\)", cand=(64, 0, 63))
    refused(-1, r"candidate outside \[-1, n_per_env\) \(environment 1\)", cand=(5, 3, 63))
    refused(-1, r"candidate outside \[-1, n_per_env\) \(environment 2\)", cand=(5, 0, -2))
    assert list(call(frm=(1, 1, 1), cand=(5, 3, 63))["status"]) == [1, 1, 1]    # 3 is beyond this context's three, not the source's 64
    # the rollouts: batched, of as many environments, long enough
    pol = case.policy([0], N_OWN, T)
    case.set_plain(src, 0)
    src.rollout_feedback(T, 1, 1, 1, *[p[0] for p in pol])
    refused(-1, "the source's last rollout was not a batched one of 3 environments")     # a plain one
    source_rollout(case, src, [0, 1], T)
    refused(-1, "the source's last rollout was not a batched one of 3 environments")     # of two environments
    source_rollout(case, src, envs, T)
    case.rollout(ctx, envs, horizon=12)
    refused(-1, "within the horizon of the source's rollout", steps=12, evaluate=derivative_steps(12, 0))
    source_rollout(case, src, envs, 12)
    case.rollout(ctx, envs, horizon=T)
    refused(-1, "within the rollout's horizon", steps=12, evaluate=derivative_steps(12, 0))
    assert list(call(frm=(1, 1, 1), steps=12, evaluate=derivative_steps(12, 0))["status"]) == [1, 1, 1]   # nobody names the short one
    # the other refusals of mjpcx_ilqg_step_batched stay, under this call's name
    refused(-1, "mjpcx_ilqg_step_batched_from: the evaluate list must be strictly increasing", evaluate=[0, 5, 5, T - 1])
    refused(-1, r"mjpcx_ilqg_step_batched_from: mu and rate must be finite and > 0 \(environment 1\)", mu=(1.0, 0.0, 1.0))
    # two contexts that do not go together: another model, another precision
    other = ts.make_case("particle64")
    pctx = other.make_context()
    source_rollout(other, pctx, envs, T)
    refused(-1, "the two contexts differ in device, precision or model dimensions", source=pctx)
    pctx.close()
    single = ts.make_case("cartpole32")
    sctx = single.make_context()
    source_rollout(single, sctx, envs, T)
    refused(-1, "the two contexts differ in device, precision or model dimensions", source=sctx)
    assert list(call(source=sctx, frm=(0, 0, 0), cand=(2, 0, 1))["status"]) == [1, 1, 1]   # nobody names it: mjpcx_ilqg_step_batched
    sctx.close()
    ctx.close()
    src.close()
    # fp32 contexts of the wavefront-per-candidate family, as mjpcx_ilqg_step_batched refuses them
    quad = ts.make_case("quad")
    quad.precision, quad.kernel = 32, "rollout_"
    qctx, qsrc = quad.make_context(), quad.make_context()
    only_states(quad, qctx, envs)
    only_states(quad, qsrc, envs)
    qsrc.rollout_splines_batched(T, capi.SPLINE_ZERO, np.tile(np.linspace(0, 0.1, 3), (E, 1)), np.zeros((E, 64, 3, quad.task.model.nu)), num_envs=E,
                                 n_per_env=64)
    with pytest.raises(capi.MjpcxError, match="mjpcx_ilqg_step_batched_from: the iLQG kernels of the wavefront-per-candidate family are fp64 only") as e:
        call(c=qctx, source=qsrc, frm=(1, 1, 1))
    assert e.value.code == -2
    qctx.close()
    qsrc.close()


# ------------------------------------------------------------------------------------------------------------- the planner
H, N = tb.H, tb.N


def device_fleet(task, exploration, device_chain):
    p = GpuBatchILQSPlanner(E, seed=0)
    p.initialize(task.model, task)
    p.sampling.num_trajectory_ = N
    if exploration is not None:
        for m in p.sampling.envs:
            m.noise_exploration[0] = exploration
    p.allocate()
    p.reset(H)
    p.device_chain = device_chain
    return p


def close(*planners):
    for p in planners:
        p.sampling.ctx.close()
        p.ilqg.ctx.close()


@pytest.mark.parametrize("name,plans", [("Particle", 6), ("Cartpole", 8)])
def test_planner_with_the_device_chain_equals_the_sequential_middle(name, plans):
    states_of, exploration = tb.FLEETS[name]
    task = load_task(name)
    chain, plain = device_fleet(task, exploration, None), device_fleet(task, exploration, False)
    assert "rollout_lane" in chain.sampling.ctx.kernel_name and "rollout_lane" in chain.ilqg.ctx.kernel_name
    steps = []
    for k in range(plans):
        states = states_of(task, k)
        for p in (chain, plain):
            p.set_states(states)
            p.optimize_policy(H)
        for e in range(E):
            tb.assert_member_equal(chain.envs[e], plain.envs[e], task.model.nu, (name, k, e))
        assert plain.last_step is None and not plain.used_device_chain
        if chain.last_step is not None:
            assert chain.used_device_chain
            steps.append(chain.last_step[0])
    print(name, "from_source of the step calls:", steps, "active:", chain.active_policy)
    if name == "Particle":
        assert [1, 0, 0] in steps and steps[0] == [1, 1, 1], steps        # the mixed fleet, after the all-sampling start
    close(chain, plain)


def test_fleet_equals_single_planners_on_the_device():
    states_of, exploration = tb.FLEETS["Particle"]
    task = load_task("Particle")
    fleet = device_fleet(task, exploration, None)
    singles = []
    for e in range(E):
        p = GpuILQSPlanner(seed=e)
        p.initialize(task.model, task)
        p.sampling.num_trajectory_ = N
        p.sampling.noise_exploration[0] = exploration
        p.allocate()
        p.reset(H)
        singles.append(p)
    for k in range(6):
        states = states_of(task, k)
        fleet.set_states(states)
        fleet.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            tb.assert_member_equal(fleet.envs[e], p, task.model.nu, ("fleet = single", k, e))
    assert fleet.active_policy == [fleet.SAMPLING, fleet.ILQG, fleet.ILQG] and fleet.last_step[0] == [1, 0, 0], (fleet.active_policy, fleet.last_step)
    close(fleet, *singles)
