"""-m gpu: the Robust planner for a fleet -- mjpcx_rollout_splines_noisy_batched (Trajectory::NoisyRollout for E environments in one
launch) and mjpcx_robust_step_batched (select, replicate, roll out, score: one call, one sync) -- on the device.

  1. A batched noisy call is compared bit for bit with E plain noisy calls on the same context (seed + e, the same local candidate
     offset): returns, failure flags and all six Trajectory buffers of EVERY candidate, on the lane kernels (NOISY = true, both
     precisions), the wave kernel and the tree kernel of both registered models; and with the oracle's NoisyRollout, per environment,
     at the tolerance tests/test_gpu_batch.py lists for the family.
  2. mjpcx_robust_step_batched is compared, every output bit for bit, with the sequential path on the same two contexts:
     ce_update_batched(skip = -1) for the order, fetch_spline, rollout_splines_noisy_batched of the replicated splines, returns() and
     the planner's Python loop (planners.robust_scores); its perturbed rollouts with the plain noisy calls.
  3. GpuBatchRobustPlanner against E GpuRobustPlanner, and GpuRobustPlanner against the C++ planner (HostPlanner(kind="robust")).
Every context of a comparison is created under the same kernel thresholds (MJPCX_QUAD_MIN_N / MJPCX_NO_QUAD / MJPCX_NO_LIMB)."""
import contextlib
import os

import numpy as np
import pytest

import task_rows
import test_batch_robust_planner as cpu
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuRobustPlanner, GpuSamplingPlanner, State, robust_scores
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle
from test_gpu_batch import E, FIELDS, H, P, SEED, err, everything, make_case

pytestmark = pytest.mark.gpu
CUBIC = capi.SPLINE_CUBIC
XSEED, OFFSET, RATE = 41, 7, 0.1
STD = {"cartpole64": 0.5, "cartpole32": 0.5, "particle64": 0.5, "tree_a1": 0.3, "wave": 0.3, "humanoid_tree": 0.2}
PAIRS = cpu.PAIRS + [(1, 3), (None, 1)]   # (None: every candidate of the environment, once)


def noisy_case(name):
    if name == "humanoid_tree":   # force noise keeps the Humanoid off the limb kernel: its wavefront-per-candidate kernel
        case = make_case("limb64")
        case.name, case.env, case.kernel, case.tol = name, {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>", 1e-6
        return case
    return make_case(name)


def splines(case):
    """E x n x P x nu: every environment's candidates (the clamped noise of tests/test_gpu_batch.py about its nominal)"""
    return np.stack([np.asarray(pyoracle.noise_candidates(case.pm, case.noise(e), P, case.nominal[e], np.arange(case.n)), float).reshape(case.n, P, -1)
                     for e in range(E)])


def push_states(case, ctx, envs):
    ctx.set_states(np.stack([case.states[e].state for e in envs]), [case.states[e].time for e in envs],
                   np.stack([case.mocap(e) for e in envs]) if case.task.model.nmocap else None)
    case.set_shared_residual(ctx)


def set_single(case, ctx, e):
    s = case.states[e]
    case.set_shared_residual(ctx)
    ctx.set_state(s.state, s.time, case.mocap(e) if case.task.model.nmocap else None)


def noisy_batched(case, ctx, envs, values, seed=XSEED, offset=OFFSET):
    push_states(case, ctx, envs)
    ctx.rollout_splines_noisy_batched(H, CUBIC, case.times[envs], values[envs], STD[case.name], RATE, seed=seed, candidate_offset=offset,
                                      num_envs=len(envs), n_per_env=values.shape[1])


def noisy_single(case, ctx, e, values, seed, offset=OFFSET):
    set_single(case, ctx, e)
    ctx.rollout_splines_noisy(H, CUBIC, case.times[e], values, STD[case.name], RATE, seed=seed, candidate_offset=offset)


def same(a, b, where):
    for k in ("total_return", "failure") + FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (where, k)


def sampled(ctx, n):
    """the variants' lighter reading: returns and flags of every candidate, the six buffers of three candidates per environment"""
    ret, fail = ctx.returns()
    picks = np.concatenate([b + np.array([0, 17, n - 1]) for b in range(0, ctx.N, n)])
    trs = [ctx.fetch_trajectory(int(c)) for c in picks]
    return dict(total_return=ret, failure=fail, picks=picks, **{k: np.stack([getattr(tr, k) for tr in trs]) for k in FIELDS})


def same_sampled(s, full, where):
    for k in ("total_return", "failure"):
        assert np.array_equal(s[k], full[k], equal_nan=True), (where, k)
    for k in FIELDS:
        assert np.array_equal(s[k], full[k][s["picks"]], equal_nan=True), (where, k)


@pytest.mark.parametrize("name", ["cartpole64", "cartpole32", "particle64", "tree_a1", "wave", "humanoid_tree"])
def test_noisy_batched_equals_plain_noisy_calls_and_the_oracle(name):
    case = noisy_case(name)
    n, values = case.n, splines(case)
    ctx = case.make_context()
    noisy_batched(case, ctx, [0, 1, 2], values)
    got = everything(ctx)
    assert ctx.N == E * n
    noisy_batched(case, ctx, [0, 1, 2], values)
    same_sampled(sampled(ctx, n), got, "a repeated call")
    # ---- bit for bit: E plain noisy calls with seeds s + e and the same local offset, on the same context
    part = lambda out, e: {k: v[e * n:(e + 1) * n] for k, v in out.items()}
    for e in range(E):
        noisy_single(case, ctx, e, values[e], XSEED + e)
        same(everything(ctx), part(got, e), ("plain", e))
    # ---- E = 1 batched (environment 1 with the stream it had in the fleet) against its share
    noisy_batched(case, ctx, [1], values, seed=XSEED + 1)
    same_sampled(sampled(ctx, n), part(got, 1), "E = 1")
    # ---- permuted environments: the place in the fleet decides the stream (seed + place), nothing else
    perm = [2, 0, 1]
    noisy_batched(case, ctx, perm, values)
    permuted = everything(ctx)
    for place, e in enumerate(perm):
        noisy_single(case, ctx, e, values[e], XSEED + place)
        same_sampled(sampled(ctx, n), part(permuted, place), ("permuted", place))
    noisy_batched(case, ctx, [0, 0, 0], values[[0, 0, 0]])   # one environment three times: three different force-noise streams
    thrice = [ctx.fetch_trajectory(b).states for b in (0, n, 2 * n)]   # (the states: the scene of the wave case has no cost terms)
    assert not np.array_equal(thrice[0], thrice[1]) and not np.array_equal(thrice[0], thrice[2])
    ctx.close()
    # the force noise does something, and the environments are different problems
    plain = case.make_context()
    push_states(case, plain, [0, 1, 2])
    plain.rollout_splines_batched(H, CUBIC, case.times, values, num_envs=E, n_per_env=n)
    assert not np.array_equal(plain.fetch_trajectory(0).states, got["states"][0])
    plain.close()
    assert not np.array_equal(got["states"][:n], got["states"][n:2 * n])
    # ---- the oracle's NoisyRollout, per environment, every candidate
    worst = {}
    for e in range(E):
        s = case.states[e]
        ref = pyoracle.rollout_batch(case.pm, case.packed(e), s.state, s.time, case.mocap(e), n, H, P, CUBIC, case.times[e], values[e], num_threads=16,
                                     xfrc_std=STD[name], xfrc_rate=RATE, seed=XSEED + e, candidate_offset=OFFSET)
        sl = slice(e * n, (e + 1) * n)
        assert np.array_equal(got["failure"][sl] != 0, ref["failure"] != 0), (name, e)
        ok = ref["failure"] == 0
        assert ok.sum() >= n // 2, (name, e, int(ok.sum()))
        for k in ("total_return",) + (() if case.returns_only else FIELDS):
            d = err(got[k][sl][ok], ref[k][ok])
            worst[k] = max(worst.get(k, 0.0), d / case.tol)
            assert d <= case.tol, (name, e, k, d, case.tol)
    print(f"{name}: worst error / tolerance by buffer {worst}")


def refused(fn, code=-1):
    with pytest.raises(capi.MjpcxError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_noisy_batched_validation_and_a_plain_call_afterwards():
    case = noisy_case("cartpole64")
    values = splines(case)
    ctx = case.make_context()
    call = lambda **kw: ctx.rollout_splines_noisy_batched(H, CUBIC, kw.get("times", case.times), kw.get("values", values), kw.get("std", 0.5),
                                                          kw.get("rate", RATE), num_envs=kw.get("E", E), n_per_env=kw.get("n", 64))
    assert "set_states" in refused(call)                                         # no set_states yet
    push_states(case, ctx, [0, 1, 2])
    assert "multiple of 64" in refused(lambda: call(values=np.zeros((E, 96, P, 1)), n=96))
    refused(lambda: call(E=0, times=case.times[:0], values=values[:0]))
    refused(lambda: call(times=case.times[:2], values=values[:2], E=2))          # E other than the last set_states
    assert "xfrc" in refused(lambda: call(std=-0.1))
    assert "xfrc" in refused(lambda: call(rate=0.0))
    bad = case.times.copy()
    bad[1, 2] = bad[1, 1]
    assert "increasing" in refused(lambda: call(times=bad))
    # a refused or a finished noisy call leaves no force noise pending: the plain and the batched calls give what a fresh context gives
    call()
    case.run_single(ctx, 0)
    one = everything(ctx)
    case.run_batched(ctx, [0, 1, 2])
    three = everything(ctx)
    fresh = case.make_context()
    case.run_single(fresh, 0)
    same(everything(fresh), one, "plain after noisy")
    case.run_batched(fresh, [0, 1, 2])
    same(everything(fresh), three, "batched after noisy")
    # xfrc_std = 0 is the plain rollout
    push_states(case, ctx, [0, 1, 2])
    call(std=0.0)
    zero = everything(ctx)
    push_states(case, fresh, [0, 1, 2])
    fresh.rollout_splines_batched(H, CUBIC, case.times, values, num_envs=E, n_per_env=64)
    same(everything(fresh), zero, "xfrc_std = 0")
    ctx.close(); fresh.close()


# ------------------------------------------------------------------------------------------------ mjpcx_robust_step_batched
def n_pad_of(k, R):
    return 64 * ((k * R + 63) // 64)


def sequential_step(case, src, ctx, k, R, times, std, rate, seed, offset, single=None):
    """the plan step through the host: order, k fetches per environment, replication, the batched noisy rollout, returns, the loop.
    single(e): prepares ctx for a plain call of environment e; the first k R perturbed rollouts are then also checked against E plain
    noisy calls."""
    n, n_pad = src.n_per_env, n_pad_of(k, R)
    idx, cret = src.ce_update_batched(E, k, -1)[:2]
    rank = np.minimum(np.arange(n_pad) // R, k - 1)
    chosen = np.stack([[src.fetch_spline(e * n + int(i)) for i in idx[e]] for e in range(E)])   # E x k x P x nu
    values = chosen[:, rank]
    ctx.rollout_splines_noisy_batched(H, CUBIC, times, values, std, rate, seed=seed, candidate_offset=offset, num_envs=E, n_per_env=n_pad)
    ret, fail = ctx.returns()
    out = dict(best=np.zeros(E, np.int32), candidate=idx, candidate_return=cret, perturbed_score=np.zeros((E, k)), valid=np.zeros((E, k), np.int32),
               spline=np.zeros((E, P, chosen.shape[-1])), returns=ret, failure=fail)
    for e in range(E):
        sl = slice(e * n_pad, e * n_pad + k * R)
        out["perturbed_score"][e], out["valid"][e], out["best"][e] = robust_scores(cret[e], ret[sl], fail[sl], R)
        out["spline"][e] = chosen[e, out["best"][e]]
    if single is not None:
        for e in range(E):
            single(e)
            ctx.rollout_splines_noisy(H, CUBIC, times[e], values[e, :k * R], std, rate, seed=seed + e, candidate_offset=offset)
            r1, f1 = ctx.returns()
            sl = slice(e * n_pad, e * n_pad + k * R)
            assert np.array_equal(r1, ret[sl], equal_nan=True) and np.array_equal(f1, fail[sl]), ("plain noisy calls", e)
    return out


def device_step(src, ctx, k, R, times, std, rate, seed, offset):
    out = ctx.robust_step_batched(src, E, k, R, H, CUBIC, times, std, rate, seed=seed, candidate_offset=offset)
    assert ctx.n_per_env == n_pad_of(k, R) and ctx.N == E * ctx.n_per_env
    out["returns"], out["failure"] = ctx.returns()
    return out


def assert_same_step(dev, seq, where):
    for key in ("best", "candidate", "candidate_return", "perturbed_score", "valid", "spline", "returns", "failure"):
        assert dev[key].shape == seq[key].shape and np.array_equal(dev[key], seq[key], equal_nan=True), (where, key)


def source_state(src):
    ret, fail = src.returns()
    return ret, fail, src.fetch_spline(0), src.fetch_spline(src.N - 1), src.fetch_trajectory(src.N // 2).states, src.N


@pytest.mark.parametrize("k,R", PAIRS)
@pytest.mark.parametrize("name", ["cartpole64", "cartpole32", "tree_a1"])
def test_robust_step_equals_the_sequential_path(name, k, R):
    case = noisy_case(name)
    k = case.n if k is None else k
    src, ctx = case.make_context(), case.make_context()
    case.run_batched(src, [0, 1, 2])
    before = source_state(src)
    push_states(case, ctx, [0, 1, 2])
    args = (k, R, case.times, STD[name], RATE, XSEED, OFFSET)
    dev = device_step(src, ctx, *args)
    again = device_step(src, ctx, *args)
    assert_same_step(again, dev, "two calls")
    seq = sequential_step(case, src, ctx, *args, single=lambda e: set_single(case, ctx, e))
    assert_same_step(dev, seq, (name, k, R))
    n = case.n
    ret = before[0].reshape(E, n)
    for e in range(E):   # the order is (return, index) ascending; the winner's rank has the lowest score, the lowest rank of equals
        order = np.lexsort((np.arange(n), ret[e]))[:k]
        assert np.array_equal(dev["candidate"][e], order) and np.array_equal(dev["candidate_return"][e], ret[e][order])
        assert dev["best"][e] == int(np.argmin(dev["perturbed_score"][e])) and np.all(dev["valid"][e] == R)
    for a, b in zip(before, source_state(src)):   # the source is unchanged: returns, flags, splines, a trajectory, its shape
        assert np.array_equal(a, b)
    src.close(); ctx.close()


def test_ties_in_the_returns_and_in_the_scores():
    """two identical splines in the source tie in the return: the lower index ranks first; with R = 1 and no force noise they tie in
    the score as well: the lower rank wins"""
    case = noisy_case("cartpole64")
    n = case.n
    src, ctx = case.make_context(), case.make_context()
    values = splines(case)
    push_states(case, src, [0, 1, 2])
    src.rollout_splines_batched(H, CUBIC, case.times, values, num_envs=E, n_per_env=n)
    ret = src.returns()[0].reshape(E, n)
    for e in range(E):   # the environment's best spline at places 7 and 3 as well
        values[e, 7] = values[e, 3] = values[e, int(np.argmin(ret[e]))]
    src.rollout_splines_batched(H, CUBIC, case.times, values, num_envs=E, n_per_env=n)
    ret = src.returns()[0].reshape(E, n)
    push_states(case, ctx, [0, 1, 2])
    args = (5, 1, case.times, 0.0, RATE, XSEED, OFFSET)
    dev = device_step(src, ctx, *args)
    for e in range(E):
        tied = sorted({3, 7, int(np.argmin(ret[e]))})
        assert ret[e][3] == ret[e][7] == ret[e].min()                                        # the tie is real
        assert dev["candidate"][e][:len(tied)].tolist() == tied
        assert np.array_equal(dev["perturbed_score"][e], dev["candidate_return"][e])       # (0 * r + r) / 1: the unperturbed return
        assert dev["perturbed_score"][e][0] == dev["perturbed_score"][e][1] and dev["best"][e] == 0
        assert np.array_equal(dev["spline"][e], values[e, 3])
    assert_same_step(dev, sequential_step(case, src, ctx, *args), "ties")
    src.close(); ctx.close()


def test_failed_perturbed_rollouts_on_the_particle():
    cases = cpu.failure_mix(lambda task: capi.Context(task.packed_model(), task.packed(), 0, 64))
    print("ranks by valid repetitions:", cases)
    assert set(cases) == {"none", "some", "all"}, cases


def test_robust_step_with_task_rows_on_both_contexts():
    case = noisy_case("cartpole64")
    rows = task_rows.unlike_rows(case.task, E)
    src, ctx = case.make_context(), case.make_context()
    push_states(case, src, [0, 1, 2])
    src.set_task_params_batched(**rows)
    src.rollout_noise_batched(case.n, H, CUBIC, case.times, case.nominal, case.noise(), num_envs=E)
    push_states(case, ctx, [0, 1, 2])
    ctx.set_task_params_batched(**rows)
    args = (13, 5, case.times, STD[case.name], RATE, XSEED, OFFSET)
    dev = device_step(src, ctx, *args)

    def single(e):   # the plain call after set_task_params(row e)
        set_single(case, ctx, e)
        ctx.set_task_params(rows["weight"][e], rows["norm_parameter"][e], rows["parameters"][e], rows["risk"][e])
    assert_same_step(dev, sequential_step(case, src, ctx, *args, single=single), "task rows")
    ctx.set_task_params(case.task.weight, case.task.norm_parameter, case.task.parameters, case.task.risk)
    ctx.set_task_params_batched()                     # shared again: other scores
    shared = device_step(src, ctx, *args)
    assert not np.array_equal(shared["perturbed_score"], dev["perturbed_score"])
    src.close(); ctx.close()


def test_robust_step_refusals():
    case = noisy_case("cartpole64")
    src, ctx = case.make_context(), case.make_context()
    step = lambda c=ctx, s=src, E_=E, k=5, R=4, times=case.times, std=0.5, rate=RATE: c.robust_step_batched(s, E_, k, R, H, CUBIC, times, std, rate)
    push_states(case, ctx, [0, 1, 2])
    case.run_single(src, 0)
    assert "not a batched one" in refused(step)                            # the source's last rollout is a plain one
    case.run_batched(src, [0, 1])
    assert "not a batched one" in refused(step)                            # ... or of another number of environments
    case.run_batched(src, [0, 1, 2])
    step()
    assert "another context" in refused(lambda: step(c=src, s=src))
    refused(lambda: step(k=0))
    refused(lambda: step(k=case.n + 1))
    refused(lambda: step(R=0))
    refused(lambda: step(E_=0, times=case.times[:0]))
    assert "xfrc" in refused(lambda: step(std=-1.0))
    assert "xfrc" in refused(lambda: step(rate=0.0))
    bad = case.times.copy()
    bad[2, 1] = bad[2, 0]
    assert "increasing" in refused(lambda: step(times=bad))
    fresh = case.make_context()
    assert "set_states" in refused(lambda: step(c=fresh))                  # this context without set_states(E)
    push_states(case, fresh, [0, 1])
    refused(lambda: step(c=fresh))                                         # ... or with another E
    single = noisy_case("cartpole32")
    other = single.make_context()
    push_states(single, other, [0, 1, 2])
    assert "precision" in refused(lambda: step(c=other))                   # fp32 against an fp64 source
    part = noisy_case("particle64")
    pctx = part.make_context()
    push_states(part, pctx, [0, 1, 2])
    assert "model dimensions" in refused(lambda: pctx.robust_step_batched(src, E, 5, 4, H, CUBIC, part.times, 0.5, RATE))
    # a refusal leaves both contexts usable
    assert_same_step(device_step(src, ctx, 5, 4, case.times, 0.5, RATE, 0, 0), device_step(src, fresh_like(case), 5, 4, case.times, 0.5, RATE, 0, 0), "after refusals")
    for c in (src, ctx, fresh, other, pctx):
        c.close()


def fresh_like(case):
    ctx = case.make_context()
    push_states(case, ctx, [0, 1, 2])
    return ctx


# ------------------------------------------------------------------------------------------------ the planners
@contextlib.contextmanager
def pinned(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_fleet_planner_equals_one_robust_planner_per_environment_on_the_device(name):
    """three plan steps, E = 3: trajectory order, scores, best candidate, perturbed scores, policy and best trajectory, exactly. The A1's
    delegate rollouts run on the quad kernel on both sides (its threshold pinned to 0: a fleet's 192 and a robot's 64 candidates would
    otherwise still agree on the tree kernel, but 2048 and 683 would not), the perturbed ones on rollout_tree_kernel<A1>."""
    with pinned(MJPCX_QUAD_MIN_N="0"):
        batch, singles, _ = cpu.run_fleet_against_members(load_task(name), 13, 5, factory=None)
    want = "rollout_quad_kernel" if name == "QuadrupedFlat" else "rollout_lane"
    assert want in batch.delegate.ctx.kernel_name and want in singles[0].delegate.ctx.kernel_name
    assert batch.ctx.n_per_env == 128 and singles[0].ctx.N == 65
    for p in singles + [batch]:
        p.ctx.close()
        p.delegate.ctx.close()


def mirror_against_cpp(task, seed, n, k, R, std, rate, state_args, steps=2):
    from mujoco_mpc_amd.hostplanner import HostPlanner
    H_ = task.planning_steps()
    cpp = HostPlanner(task, seed=seed, num_trajectory=n, kind="robust")
    cpp.robust_config(ncandidates=k, nrepetitions=R, xfrc_std=std, xfrc_rate=rate)
    if task.name == "QuadrupedFlat":
        cpp.task_transition(0.0)
        task.transition(0.0)
    cpp.reset(H_)
    py = GpuRobustPlanner(GpuSamplingPlanner(seed=seed), seed=seed)
    py.initialize(task.model, task)
    py.delegate.num_trajectory_, py.ncandidates_, py.nrepetitions_, py.xfrc_std_, py.xfrc_rate_ = n, k, R, std, rate
    py.allocate()
    py.reset(H_)
    st = State(task.model)
    for step in range(steps):
        st.set(**state_args)
        py.set_state(st)
        py.optimize_policy(H_)
        cpp.set_state(state_args["qpos"], state_args["qvel"], state_args.get("time", 0.0), mocap_pos=state_args.get("mocap_pos"),
                      mocap_quat=state_args.get("mocap_quat"))
        cpp.optimize_policy(H_)
        best, scores = cpp.robust_result(k)
        assert best == py.best_candidate, (step, best, py.best_candidate)
        assert np.array_equal(scores[:k], np.array(py.perturbed_score)), step
        ct, cv = cpp.policy()
        assert np.array_equal(ct, py.delegate.policy.plan.times()) and np.array_equal(cv, py.delegate.policy.plan.values()), step
    cpp.close()
    py.ctx.close(); py.delegate.ctx.close()


def test_python_robust_planner_equals_the_cpp_planner_on_the_cartpole():
    mirror_against_cpp(load_task("Cartpole"), 4, 128, 5, 4, 0.5, 0.05, dict(qpos=[0.4, 2.6], qvel=[0.1, -0.3], time=0.0))


def test_python_robust_planner_equals_the_cpp_planner_on_the_quadruped():
    t = load_task("QuadrupedFlat")
    args = dict(qpos=t.model.keyframes["home"]["qpos"], qvel=np.zeros(18), time=0.0, mocap_pos=np.array([[0.3, 0, 0.26], [-2.5, 0, 0]]),
                mocap_quat=np.array([[1.0, 0, 0, 0], [1.0, 0, 0, 0]]))
    with pinned(MJPCX_NO_QUAD="1"):   # both planners' contexts on rollout_tree_kernel<A1>, whatever the batch
        mirror_against_cpp(t, 2, 64, 4, 3, 0.3, 0.1, args)
