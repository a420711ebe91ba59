"""-m gpu: pruning and parking with a bound per environment (mjpcx_set_pruning_batched). Environment e of a pruned
mjpcx_rollout_noise_batched behaves like the plain pruned launch of that environment alone: its own bound, hint and counters, its own
segment of the resume list, ONE resume launch for the fleet. What mjpcx_best_batched reads, and every candidate not marked pruned, equals
the unpruned batched launch bit for bit, whatever the bounds and hints.

A1, fp64, MJPCX_QUAD_MIN_N=1, E = 3 environments x n = 64 candidates, H = 30, P = 3, std0 = 0.04, at 4 and at 16 candidates per wavefront.
The environments are unlike: home, the trot3 state of tests/step_bank.py, home again under another noise stream -- a launch that compared
environment 1 with environment 0's bound would retire all of environment 1. With each environment's initial bound at its own unpruned
minimum the bound never moves, and which candidates are retired, parked and resumed is a function of the unpruned costs that numpy computes
(expected_with_fixed_bound, the rule of tests/test_gpu_quad_park.py per environment)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import model_variants
import step_bank
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchSamplingPlanner, State
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
E, n, H, P = 3, 64, 30, 3
N = E * n
TIMES = np.arange(P) * ((H - 1) * 0.01 / P)
NOMINAL = np.zeros((P, 12))
PARKED, PRUNED, FALLBACK = 0x10000000, 0x20000000, 0x40000000
BUFFERS = ("states", "actions", "times", "residual", "costs", "trace")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -5
INF = np.inf


def noise(seed=0):
    return capi.make_noise_spec(seed=seed, iteration=1, mode=capi.NOISE_SAMPLING, std0=0.04)


@pytest.fixture(scope="module")
def quad():
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    return t


@pytest.fixture(scope="module")
def states(quad):
    home = np.concatenate([quad.model.keyframes["home"]["qpos"], np.zeros(18)])
    trot = [s for s in step_bank.a1_bank().states if s.label.startswith("trot3/")][0].state
    return np.stack([home, np.asarray(trot, float), home])


def context(t, states, env=None, cpw=None, rows=None, num_envs=E):
    env = dict({"MJPCX_QUAD_MIN_N": "1"}, **(env or {}))
    if cpw is not None and cpw != 4:
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
    ctx.set_states(states[:num_envs], np.zeros(num_envs), np.stack([MOCAP] * num_envs))
    if rows is not None:
        ctx.set_task_params_batched(weight=rows)
    return ctx


def launch(ctx, num_envs=E, per_env=n):
    ctx.rollout_noise_batched(per_env, H, capi.SPLINE_ZERO, np.stack([TIMES] * num_envs), np.stack([NOMINAL] * num_envs), noise(), num_envs=num_envs)


def snapshot(ctx, trajectories=True):
    ret, _ = ctx.returns()
    out = dict(total_return=ret.copy(), failure=ctx.failure_raw.copy())
    if trajectories:
        trs = [ctx.fetch_trajectory(c) for c in range(ctx.N)]
        for k in BUFFERS:
            out[k] = np.stack([getattr(tr, k) for tr in trs])
    return out


def task_rows(quad, variant):
    """the fourth variant: environment 1's weights x 4, so that the bounds differ by construction as well"""
    if variant == "plain":
        return None
    w = np.stack([np.asarray(quad.weight, float)] * E)
    w[1] *= 4.0
    return w


_FULL = {}


def full_launch(quad, states, variant):
    """the unpruned batched launch (computed once per variant, never written to): every buffer, what mjpcx_best_batched reads, and the
    non-vacuity conditions every case below rests on"""
    if variant not in _FULL:
        ctx = context(quad, states, rows=task_rows(quad, variant))
        launch(ctx)
        out = snapshot(ctx)
        out["best"] = ctx.best_batched(E, 0)
        out["stats"] = ctx.quad_stats()
        st = ctx.prune_stats_batched(E)
        assert not st["retired"].any() and not st["parked"].any() and not st["final_bound"].any()
        ctx.topk(4)
        ctx.close()
        assert not out["failure"].any() and out["costs"].min() > 0 and out["stats"]["handed_on"] == 0
        out["min"] = out["total_return"].reshape(E, n).min(axis=1)
        assert np.array_equal(out["min"], out["best"][1])
        # the environments are unlike: environment 1's best is above everything environment 0 and 2 would let through
        assert out["min"][1] > 2 * out["min"][0] and out["min"][1] > 2 * out["min"][2]
        for e in range(E):
            _, final, _ = expected_with_fixed_bound(out["costs"][e * n:(e + 1) * n], out["min"][e], INF)
            assert 1 <= (final >= 0).sum() <= n - 2, (variant, e)     # every environment retires at least one candidate and keeps at least two
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FULL[variant] = out
    return _FULL[variant]


def same_best(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def expected_with_fixed_bound(costs, bound, hint, nominal=0):
    """one environment, bound fixed at its minimum: per local candidate the park step (-1: never) and the retire step (-1: completes). Per
    step the proven test comes first, then the hint; neither at the last step; never the nominal. The settling rule retires nothing here
    (the proven test has just failed against the same bound): every parked candidate is resumed"""
    partial = np.cumsum(costs, axis=1) / float(H)
    parked, final = np.full(len(costs), -1), np.full(len(costs), -1)
    for c in range(len(costs)):
        if c == nominal:
            continue
        for t in range(H - 1):
            if partial[c, t] > bound:
                final[c] = t
                break
            if parked[c] < 0 and partial[c, t] > hint:
                parked[c] = t
    return parked, final, partial


def expected_fleet(full, bounds, hints):
    got = [expected_with_fixed_bound(full["costs"][e * n:(e + 1) * n], bounds[e], hints[e]) for e in range(E)]
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]), np.concatenate([g[2] for g in got])


@pytest.mark.parametrize("variant", ["plain", "task rows"])
@pytest.mark.parametrize("cpw", [4, 16])
def test_bounds_at_the_minima_retire_park_and_resume_exactly_the_computed_sets(quad, states, cpw, variant):
    full = full_launch(quad, states, variant)
    best = full["min"]
    ctx = context(quad, states, cpw=cpw, rows=task_rows(quad, variant))
    cases = {"no hints": [INF, INF, INF], "mixed": [INF, 0.5 * best[1], 0.0], "mixed, rotated": [0.0, INF, 0.5 * best[2]],
             "1.05 best": list(1.05 * best), "all zero": [0.0, 0.0, 0.0]}
    for name, hints in cases.items():
        parked, final, partial = expected_fleet(full, best, hints)
        ctx.set_pruning_batched(True, E, best, hints)
        launch(ctx)
        assert same_best(ctx.best_batched(E, 0), full["best"]), name
        st = ctx.prune_stats_batched(E)
        retired = final >= 0
        run = snapshot(ctx)
        assert np.array_equal(run["failure"], np.where(retired, PRUNED | (final << 8), 0)), name
        for e in range(E):
            sl = slice(e * n, (e + 1) * n)
            assert st["retired"][e] == retired[sl].sum() and st["retire_step_sum"][e] == final[sl][retired[sl]].sum() and not st["negative_cost"][e], (name, e)
            assert st["parked"][e] == (parked[sl] >= 0).sum() and st["parked"][e] == st["settled_retired"][e] + st["resumed"][e], (name, e)
            assert st["settled_retired"][e] == 0 and st["final_bound"][e] == best[e], (name, e)
            if hints[e] == INF or hints[e] >= best[e]:
                assert st["parked"][e] == 0, (name, e)     # at or above the minimum the proven test retires first
        idx, step = ctx.park_resumed()
        assert np.array_equal(idx, np.nonzero(parked >= 0)[0]) and np.array_equal(step, parked[parked >= 0]), name   # global indices
        if name.startswith("mixed"):
            # the resume launch holds candidates of at least two environments, with counts that are not multiples of 4
            assert (st["resumed"] > 0).sum() >= 2 and all(r % 4 != 0 for r in st["resumed"] if r > 0), (name, st["resumed"])
        if name == "all zero":
            assert (st["parked"] == n - 1).all()
        # the sums over the environments
        tot, ptot = ctx.prune_stats(), ctx.park_stats()
        assert tot["retired"] == st["retired"].sum() and tot["retire_step_sum"] == st["retire_step_sum"].sum()
        assert (ptot["parked"], ptot["settled_retired"], ptot["resumed"]) == (st["parked"].sum(), 0, st["resumed"].sum())
        last = np.where(retired, final, H - 1)
        assert np.array_equal(run["total_return"], partial[np.arange(N), last]), name
        for c in range(N):   # (kept and resumed candidates to the horizon, retired ones up to their step: rows of one or of two launches)
            for k in BUFFERS:
                assert np.array_equal(run[k][c, :last[c] + 1], full[k][c, :last[c] + 1]), (name, k, c)
        assert ctx.quad_stats() == full["stats"]
    ctx.close()


@pytest.mark.parametrize("cpw", [4, 16])
def test_bounds_from_infinity_keep_what_the_plan_step_reads_under_any_hints(quad, states, cpw):
    """At these sizes every wavefront runs at once, so possibly nothing is retired by the proven bound: only the invariants are asserted"""
    full = full_launch(quad, states, "plain")
    best = full["min"]
    partial = np.cumsum(full["costs"], axis=1) / float(H)
    names = [INF, 1.0, 1.05, 0.5, 0.0]
    ctx = context(quad, states, cpw=cpw)
    for shift in range(5):
        factors = [names[(shift + 2 * e) % 5] for e in range(E)]
        hints = [INF if f == INF else f * best[e] for e, f in enumerate(factors)]
        ctx.set_pruning_batched(True, E, None, hints)
        launch(ctx)
        assert same_best(ctx.best_batched(E, 0), full["best"]), factors
        run, st = snapshot(ctx), ctx.prune_stats_batched(E)
        assert ((run["failure"] & (PARKED | FALLBACK)) == 0).all()
        kept = run["failure"] == 0
        for k in BUFFERS + ("total_return",):
            assert np.array_equal(run[k][kept], full[k][kept]), (factors, k)
        gone = ~kept
        assert ((run["failure"][gone] & PRUNED) != 0).all()
        t = (run["failure"][gone] >> 8) & 0xFFFF
        assert (t < H - 1).all() and np.array_equal(run["total_return"][gone], partial[gone, t])
        for e in range(E):
            sl = slice(e * n, (e + 1) * n)
            assert kept[e * n] and kept[e * n + full["best"][0][e]]                       # the local nominal and the winner
            assert (run["total_return"][sl][gone[sl]] > best[e]).all()                    # strictly above the environment's winner
            assert (run["total_return"][sl][gone[sl]] > st["final_bound"][e]).all() and st["final_bound"][e] == best[e]
            assert st["retired"][e] == gone[sl].sum() and st["parked"][e] == st["settled_retired"][e] + st["resumed"][e]
            if factors[e] == INF:
                assert st["parked"][e] == 0
            if factors[e] == 0.0:
                assert st["parked"][e] == n - 1
    ctx.close()


def test_with_a_model_per_environment_each_equals_the_plain_pruned_launch_on_its_model(quad, states):
    rob = model_variants.robot("a1")
    models = [rob.base, rob.mixed["payload"], rob.mixed["weak"]]
    ctx = context(quad, states)
    ctx.set_models_batched([rob.packed(m) for m in models])
    launch(ctx)
    ret = ctx.returns()[0].reshape(E, n).copy()
    assert not ctx.failure_raw.any()
    bounds = ret.min(axis=1)
    ctx.set_pruning_batched(True, E, bounds, None)
    launch(ctx)
    run, st = snapshot(ctx), ctx.prune_stats_batched(E)
    ctx.close()
    assert (st["retired"] > 0).all()
    for e in range(E):
        os.environ["MJPCX_QUAD_MIN_N"] = "1"
        try:
            one = capi.Context(rob.packed(models[e]), quad.packed(), 0, 64)
        finally:
            os.environ.pop("MJPCX_QUAD_MIN_N", None)
        one.set_state(states[e], 0.0, MOCAP)
        one.set_pruning(True, bounds[e])
        one.rollout_noise(n, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise(seed=e))
        ref = snapshot(one)
        assert one.prune_stats()["retired"] == st["retired"][e]
        one.close()
        sl = slice(e * n, (e + 1) * n)
        assert np.array_equal(run["failure"][sl], ref["failure"]), e
        kept = ref["failure"] == 0
        for k in BUFFERS + ("total_return",):
            assert np.array_equal(run[k][sl][kept], ref[k][kept]), (e, k)


def test_a_bound_below_every_return_of_one_environment_names_it(quad, states):
    full = full_launch(quad, states, "plain")
    ctx = context(quad, states)
    bounds = full["min"].copy()
    bounds[1] *= 0.5
    ctx.set_pruning_batched(True, E, bounds, None)
    launch(ctx)
    with pytest.raises(capi.MjpcxError) as e:
        ctx.best_batched(E, 0)
    assert e.value.code == ESTATE and "environment(s) 1 is above" in str(e.value)
    ctx.set_pruning_batched(True, E, full["min"], None)
    launch(ctx)
    assert same_best(ctx.best_batched(E, 0), full["best"])
    ctx.close()


def test_rankings_are_refused_after_a_pruned_batched_launch(quad, states):
    full = full_launch(quad, states, "plain")
    ctx = context(quad, states)
    ctx.set_pruning_batched(True, E, full["min"], None)
    launch(ctx)
    calls = {"ce_update_batched": lambda: ctx.ce_update_batched(E, 4), "topk": lambda: ctx.topk(4), "topk(1)": lambda: ctx.topk(1), "best": lambda: ctx.best(0),
             "elite_moments": lambda: ctx.elite_moments([0, 1, 2]),
             "sample_gradient_update_batched": lambda: ctx.sample_gradient_update_batched(E, 0, 0, 1.0, 1.0, 1.0, 1.0)}
    for name, call in calls.items():
        with pytest.raises(capi.MjpcxError) as e:
            call()
        assert e.value.code == ESTATE and "lower bounds that depend on timing" in str(e.value), name
    other = context(quad, states)
    with pytest.raises(capi.MjpcxError) as e:
        other.robust_step_batched(ctx, E, 2, 2, H, capi.SPLINE_ZERO, np.stack([TIMES] * E), 0.1, 0.1)
    assert e.value.code == ESTATE and "lower bounds that depend on timing" in str(e.value)
    other.close()
    # what stays usable
    ctx.returns()
    ctx.fetch_trajectory(full["best"][0][1] + n)
    ctx.fetch_spline(0)
    ctx.close()


def test_bad_arguments_and_another_fleet_size(quad, states):
    ctx = context(quad, states)
    for bad in (-1.0, float("nan")):
        for kw in (dict(initial_bound=[1.0, bad, 1.0]), dict(park_hint=[INF, INF, bad])):
            with pytest.raises(capi.MjpcxError) as e:
                ctx.set_pruning_batched(True, E, **kw)
            assert e.value.code == EINVAL
    ctx.set_pruning_batched(True, 2, None, None)
    with pytest.raises(capi.MjpcxError) as e:
        launch(ctx)
    assert e.value.code == EINVAL and "mjpcx_set_pruning_batched" in str(e.value)
    ctx.set_pruning_batched(False)
    launch(ctx)
    ctx.topk(4)
    ctx.close()


def unpruned_like_the_parent(ctx, full):
    launch(ctx)
    run = snapshot(ctx, trajectories=False)
    assert np.array_equal(run["total_return"], full["total_return"]) and not run["failure"].any()
    st = ctx.prune_stats_batched(E)
    assert not any(np.asarray(v).any() for v in st.values())
    assert ctx.prune_stats()["retired"] == 0 and ctx.park_stats()["parked"] == 0
    ctx.topk(4)
    ctx.ce_update_batched(E, 4)


def test_launches_that_ignore_the_switch_behave_as_before(quad, states):
    full = full_launch(quad, states, "plain")
    zeros = [0.0, 0.0, 0.0]
    ctx = context(quad, states)
    unpruned_like_the_parent(ctx, full)                                # switch off
    ctx.set_pruning_batched(True, E, full["min"], zeros)
    ctx.set_pruning_batched(False)
    unpruned_like_the_parent(ctx, full)                                # set and cleared
    # the plain switches do not reach a batched launch, and the batched switch does not reach a plain one
    ctx.set_pruning_batched(True, E, full["min"], zeros)
    ctx.set_state(states[0], 0.0, MOCAP)
    ctx.rollout_noise(n, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    one = snapshot(ctx, trajectories=False)
    assert np.array_equal(one["total_return"], full["total_return"][:n]) and not one["failure"].any()
    assert ctx.prune_stats()["retired"] == 0
    ctx.topk(4)
    # given splines and the cross-entropy launch roll everything out under the switch
    nodes = np.stack([ctx.fetch_spline(c) for c in range(n)])
    ctx.rollout_splines_batched(H, capi.SPLINE_ZERO, np.stack([TIMES] * E), np.stack([nodes] * E), num_envs=E, n_per_env=n)
    got = snapshot(ctx, trajectories=False)
    assert not got["failure"].any() and ctx.prune_stats()["retired"] == 0 and not ctx.prune_stats_batched(E)["retired"].any()
    ctx.topk(4)
    ns = capi.make_noise_spec(seed=0, iteration=1, mode=capi.NOISE_CROSS_ENTROPY, nominal_candidate=n - 1, explore_count=8, std0=0.04, std1=0.01)
    ctx.rollout_noise_batched_ce(n, H, capi.SPLINE_ZERO, np.stack([TIMES] * E), np.stack([NOMINAL] * E), np.full((E, P, 12), 1e-3), ns, num_envs=E)
    got = snapshot(ctx, trajectories=False)
    assert not (got["failure"] & PRUNED).any() and not ctx.prune_stats_batched(E)["retired"].any()
    ctx.ce_update_batched(E, 4, n - 1)
    ctx.close()
    # a launch below MJPCX_QUAD_MIN_N goes to the wavefront-per-candidate kernel: everything is rolled out
    ctx = context(quad, states, env={"MJPCX_QUAD_MIN_N": str(N + 1)})
    ctx.set_pruning_batched(True, E, full["min"], zeros)
    launch(ctx)
    got = snapshot(ctx, trajectories=False)
    assert not got["failure"].any() and not ctx.prune_stats_batched(E)["retired"].any() and ctx.prune_stats()["retired"] == 0
    ctx.topk(4)
    ctx.close()


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_batch_prune as T
from mujoco_mpc_amd.task import load_task
quad = load_task("QuadrupedFlat")
quad.transition(0.0)
states = np.load(sys.argv[2])
ctx = T.context(quad, states)
ctx.set_pruning_batched(True, T.E, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
T.launch(ctx)
ret, _ = ctx.returns()
st = ctx.prune_stats_batched(T.E)
ctx.topk(4)
np.savez(sys.argv[3], ret=ret, failure=ctx.failure_raw, retired=st["retired"], parked=st["parked"])
ctx.close()
"""


def test_prune_switch_off_in_the_environment(quad, states, tmp_path):
    """MJPCX_PRUNE=0 is read when the context is created: a fresh child process. The call then does nothing, whatever its bounds"""
    full = full_launch(quad, states, "plain")
    script, st_file, out = tmp_path / "child.py", tmp_path / "states.npy", tmp_path / "out.npz"
    script.write_text(CHILD)
    np.save(st_file, states)
    env = dict(os.environ, MJPCX_PRUNE="0")
    done = subprocess.run([sys.executable, str(script), ROOT, str(st_file), str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    got = dict(np.load(out))
    assert np.array_equal(got["ret"], full["total_return"]) and not got["failure"].any() and not got["retired"].any() and not got["parked"].any()


def test_park_switch_off_in_the_environment_ignores_the_hints(quad, states):
    full = full_launch(quad, states, "plain")
    ctx = context(quad, states, env={"MJPCX_PARK": "0"})
    ctx.set_pruning_batched(True, E, full["min"], [0.0, 0.0, 0.0])
    launch(ctx)
    st = ctx.prune_stats_batched(E)
    assert not st["parked"].any() and (st["retired"] > 0).all()
    assert same_best(ctx.best_batched(E, 0), full["best"])
    ctx.close()


def test_one_environment_is_the_plain_pruned_launch(quad, states):
    """E = 1 through the batched entry point: the same retirements, returns and counters as mjpcx_set_pruning on the plain one"""
    ctx = context(quad, states, num_envs=1)
    launch(ctx, num_envs=1, per_env=128)
    best = ctx.returns()[0].min()
    ctx.set_pruning_batched(True, 1, [best], [0.5 * best])
    launch(ctx, num_envs=1, per_env=128)
    a, sa = snapshot(ctx), ctx.prune_stats_batched(1)
    ctx.set_pruning_batched(False)
    ctx.set_state(states[0], 0.0, MOCAP)
    ctx.set_pruning(True, best)
    ctx.set_park_hint(0.5 * best)
    ctx.rollout_noise(128, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    b, sb, pb = snapshot(ctx), ctx.prune_stats(), ctx.park_stats()
    ctx.close()
    assert np.array_equal(a["failure"], b["failure"]) and np.array_equal(a["total_return"], b["total_return"])
    assert (sa["retired"][0], sa["retire_step_sum"][0], sa["parked"][0], sa["resumed"][0]) == (sb["retired"], sb["retire_step_sum"], pb["parked"], pb["resumed"])
    assert sb["retired"] > 0 and pb["resumed"] > 0
    kept = b["failure"] == 0
    for k in BUFFERS:
        assert np.array_equal(a[k][kept], b[k][kept]), k


def test_the_planner_computes_the_same_policy_with_and_without_pruning(quad, states):
    """GpuBatchSamplingPlanner on the device, three plan steps with every robot advanced along its best trajectory"""
    runs = {}
    for pruning in (False, True):
        os.environ["MJPCX_QUAD_MIN_N"] = "1"
        try:
            pl = GpuBatchSamplingPlanner(E, seed=3)
            pl.initialize(quad.model, quad)
            pl.num_trajectory_ = n
            pl.allocate()
        finally:
            os.environ.pop("MJPCX_QUAD_MIN_N", None)
        pl.pruning = pruning
        pl.reset(H)
        m = quad.model
        sts = []
        for e in range(E):
            st = State(m)
            st.set(states[e][:m.nq], states[e][m.nq:], mocap_pos=MOCAP.reshape(-1, 7)[:, :3], mocap_quat=MOCAP.reshape(-1, 7)[:, 3:], time=0.0)
            sts.append(st)
        log = []
        for step in range(3):
            pl.set_states(sts)
            pl.optimize_policy(H)
            trs = [pl.best_trajectory(e) for e in range(E)]
            log.append(dict(winners=list(pl.winners), values=[p.policy.plan.values().copy() for p in pl.envs], times=[p.policy.plan.times().copy() for p in pl.envs],
                            best=[p.best_return for p in pl.envs], nominal=[p.nominal_return for p in pl.envs],
                            trs=[{k: getattr(tr, k).copy() for k in BUFFERS} for tr in trs], hints=pl.park_hints_used,
                            retired=None if pl.prune_stats is None else pl.prune_stats["retired"].copy(), repeated=pl.pruned_launch_repeated))
            for e in range(E):
                sts[e].set(trs[e].states[1, :m.nq], trs[e].states[1, m.nq:], mocap_pos=MOCAP.reshape(-1, 7)[:, :3], mocap_quat=MOCAP.reshape(-1, 7)[:, 3:],
                           time=float(trs[e].times[1]))
        runs[pruning] = log
        pl.ctx.close()
    for step, (a, b) in enumerate(zip(runs[False], runs[True])):
        assert a["winners"] == b["winners"] and a["best"] == b["best"] and a["nominal"] == b["nominal"], step
        for e in range(E):
            assert np.array_equal(a["values"][e], b["values"][e]) and np.array_equal(a["times"][e], b["times"][e]), (step, e)
            for k in BUFFERS:
                assert np.array_equal(a["trs"][e][k], b["trs"][e][k]), (step, e, k)
        assert a["hints"] is None and a["retired"] is None and not b["repeated"]
        assert np.isinf(b["hints"]).all() if step == 0 else np.isfinite(b["hints"]).all(), step
        if step > 0:
            assert np.array_equal(b["hints"], np.array(runs[True][step - 1]["best"]) * 1.05)
