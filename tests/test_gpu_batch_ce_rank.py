"""-m gpu: rank mode for a fleet (mjpcx_set_prune_rank with mjpcx_set_pruning_batched) under the Cross-Entropy launch,
mjpcx_rollout_noise_batched_ce. Every environment settles on its own T = the K-th smallest return its candidates completed with
(rank_bound_kernel, one workgroup per environment); what mjpcx_ce_update_batched reads -- the n_elite best without the nominal, their mean,
variance and mean return -- equals the unpruned launch bit for bit, whatever the hints.

A1, fp64, MJPCX_QUAD_MIN_N=1, E = 3 environments x n = 64 candidates (63 + the nominal, local candidate 63), H = 30, P = 3, n_elite = 6,
K = 7, at 4 and at 16 candidates per wavefront; the states of tests/test_gpu_batch_prune.py (home, trot3, home under another stream). The
hints come from the unpruned launch's returns: environment 0's is its K-th return (its K best complete, T is that return and what the hint
parks is retired), environment 1's half its best return (too low: only the nominal completes, T = +inf, everything parked is resumed),
environment 2 has none. The word does not move while candidates run, so the counters and T are the numpy function of the unpruned costs
(tests/quademu/rank.py `expected`)."""
import os

import numpy as np
import pytest

import step_bank
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchCrossEntropyPlanner, State
from mujoco_mpc_amd.task import load_task
from tests.quademu import rank

pytestmark = pytest.mark.gpu
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
E, n, H, P = 3, 64, 30, 3
N_ELITE, K = 6, 7
NOM = n - 1
TIMES = np.arange(P) * ((H - 1) * 0.01 / P)
NOMINAL = np.zeros((P, 12))
PARKED, PRUNED, FALLBACK = 0x10000000, 0x20000000, 0x40000000
BUFFERS = ("states", "actions", "times", "residual", "costs", "trace")
EINVAL, ESTATE = -1, -5
INF = np.inf


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


def context(t, states, env=None, cpw=None, rows=None):
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
    ctx.set_states(states, np.zeros(E), np.stack([MOCAP] * E))
    if rows is not None:
        ctx.set_task_params_batched(weight=rows)
    return ctx


def launch(ctx):
    ns = capi.make_noise_spec(seed=0, iteration=1, mode=capi.NOISE_CROSS_ENTROPY, nominal_candidate=NOM, explore_count=8, std0=0.04, std1=0.01)
    ctx.rollout_noise_batched_ce(n, H, capi.SPLINE_ZERO, np.stack([TIMES] * E), np.stack([NOMINAL] * E), np.full((E, P, 12), 1.6e-3), ns, num_envs=E)


def snapshot(ctx):
    ret, _ = ctx.returns()
    out = dict(total_return=ret.copy(), failure=ctx.failure_raw.copy())
    trs = [ctx.fetch_trajectory(c) for c in range(ctx.N)]
    for k in BUFFERS:
        out[k] = np.stack([getattr(tr, k) for tr in trs])
    return out


def task_rows(quad, variant):
    """the second variant: the robots weigh their costs differently, so that their bounds differ by construction as well"""
    if variant == "plain":
        return None
    w = np.stack([np.asarray(quad.weight, float)] * E)
    w[1] *= 4.0
    w[2] *= 0.5
    return w


_FULL = {}


def full_launch(quad, states, variant):
    """the unpruned launch (once per variant, never written to), what the Cross-Entropy update reads of it, and the hints of the cases"""
    if variant not in _FULL:
        ctx = context(quad, states, rows=task_rows(quad, variant))
        launch(ctx)
        out = snapshot(ctx)
        out["update"] = ctx.ce_update_batched(E, N_ELITE, NOM)
        out["best"] = ctx.best_batched(E, NOM)
        out["stats"] = ctx.quad_stats()
        ctx.close()
        assert not out["failure"].any() and out["costs"].min() > 0 and out["stats"]["handed_on"] == 0
        ret = np.sort(out["total_return"].reshape(E, n), axis=1)
        out["hints"] = np.array([ret[0, K - 1], 0.5 * ret[1, 0], INF])
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FULL[variant] = out
    return _FULL[variant]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def expected_fleet(full, hints):
    return [rank.expected(full["costs"][e * n:(e + 1) * n], H, K, hints[e], nominal=NOM) for e in range(E)]


def check_run(ctx, full, hints, what):
    want = expected_fleet(full, hints)
    got = ctx.ce_update_batched(E, N_ELITE, NOM)
    assert same(got, full["update"]), what   # index, return, mean, variance, avg_return
    assert same(ctx.best_batched(E, NOM), full["best"]), what
    st = ctx.prune_stats_batched(E)
    run = snapshot(ctx)
    assert ((run["failure"] & (PARKED | FALLBACK)) == 0).all(), what
    for e, w in enumerate(want):
        final = np.where(w["retired"], w["park"], w["late"])
        gone = final >= 0
        seg = slice(e * n, (e + 1) * n)
        assert np.array_equal(run["failure"][seg], np.where(gone, PRUNED | (final << 8), 0)), (what, e)
        for k in BUFFERS + ("total_return",):
            assert np.array_equal(run[k][seg][~gone], full[k][seg][~gone]), (what, e, k)
        assert (run["total_return"][seg][gone] > w["T"]).all() and not gone[NOM]
        assert (st["parked"][e], st["settled_retired"][e], st["resumed"][e]) == ((w["park"] >= 0).sum(), w["retired"].sum(), w["resumed"].sum()), (what, e)
        assert (st["retired"][e], st["retire_step_sum"][e], st["negative_cost"][e]) == (gone.sum(), final[gone].sum(), False), (what, e)
        assert st["final_bound"][e] == w["T"], (what, e, st["final_bound"][e], w["T"])
    return want, st


@pytest.mark.parametrize("variant", ["plain", "task rows"])
@pytest.mark.parametrize("cpw", [4, 16])
def test_the_update_does_not_depend_on_the_hints(quad, states, cpw, variant):
    full = full_launch(quad, states, variant)
    ctx = context(quad, states, cpw=cpw, rows=task_rows(quad, variant))
    ctx.set_prune_rank(K)
    cases = {"retire, resume, none": full["hints"], "no hints": [INF] * E, "all zero": [0.0] * E, "rotated": np.roll(full["hints"], 1)}
    for name, hints in cases.items():
        ctx.set_pruning_batched(True, E, None, hints)
        launch(ctx)
        want, st = check_run(ctx, full, hints, name)
        if name == "retire, resume, none":
            # environment 0 retires what it parked, environment 1 resumes everything (its hint was too low), environment 2 parks nothing
            assert st["parked"][0] > 0 and st["settled_retired"][0] == st["parked"][0] and want[0]["T"] == hints[0]
            assert st["parked"][1] == n - 1 and st["resumed"][1] == n - 1 and st["retired"][1] == 0 and want[1]["T"] == INF
            assert st["parked"][2] == 0 and st["retired"][2] == 0 and want[2]["T"] == np.sort(full["total_return"][2 * n:])[K - 1]
        if name == "all zero":
            assert (st["parked"] == n - 1).all() and (st["resumed"] == n - 1).all()
        # beyond the first K the ranking is refused; so are the planners that read every return
        with pytest.raises(capi.MjpcxError) as e:
            ctx.ce_update_batched(E, N_ELITE + 1, NOM)
        assert e.value.code == ESTATE and "rank 7" in str(e.value), name
        ctx.ce_update_batched(E, N_ELITE + 1)   # (no skipped candidate: 7 elites fit in the first 7)
        with pytest.raises(capi.MjpcxError) as e:
            ctx.sample_gradient_update_batched(E, 0, 0, 1.0, 1.0, 1.0, 1.0)
        assert e.value.code == ESTATE, name
    ctx.close()


def test_at_rank_one_the_cross_entropy_launch_keeps_ignoring_the_switch(quad, states):
    full = full_launch(quad, states, "plain")
    ctx = context(quad, states)
    ctx.set_pruning_batched(True, E, None, [0.0] * E)
    for back_from in (None, K):
        if back_from:
            ctx.set_prune_rank(back_from)
            ctx.set_prune_rank(1)
        launch(ctx)
        ret, _ = ctx.returns()
        assert np.array_equal(ret, full["total_return"]) and not ctx.failure_raw.any()
        st = ctx.prune_stats_batched(E)
        assert not any(np.asarray(v).any() for v in st.values())
        assert same(ctx.ce_update_batched(E, N_ELITE, NOM), full["update"])
        ctx.ce_update_batched(E, 2 * N_ELITE, NOM)
    ctx.close()


def test_arguments(quad, states):
    ctx = context(quad, states)
    ctx.set_prune_rank(K)
    with pytest.raises(capi.MjpcxError) as e:   # nobody can vouch for a K-th return
        ctx.set_pruning_batched(True, E, [INF, 2.0, INF], None)
    assert e.value.code == EINVAL
    ctx.set_pruning_batched(True, 2, None, None)
    with pytest.raises(capi.MjpcxError) as e:   # another fleet size under the switch: an error, as for mjpcx_rollout_noise_batched
        launch(ctx)
    assert e.value.code == EINVAL and "mjpcx_set_pruning_batched" in str(e.value)
    ctx.set_prune_rank(1)
    ctx.set_pruning_batched(True, E, [INF, 2.0, INF], None)
    with pytest.raises(capi.MjpcxError) as e:
        ctx.set_prune_rank(K)
    assert e.value.code == EINVAL
    ctx.close()


def test_the_planner_computes_the_same_policy_with_and_without_pruning(quad, states):
    """GpuBatchCrossEntropyPlanner on the device, three plan steps from the same seed with every robot advanced along its nominal rollout:
    policies, variances, trajectory_order, improvement and best_trajectory are identical, and from the second plan on some robot parks"""
    runs = {}
    m = quad.model
    for pruning in (False, True):
        os.environ["MJPCX_QUAD_MIN_N"] = "1"
        try:
            pl = GpuBatchCrossEntropyPlanner(E, seed=3)
            pl.initialize(m, quad)
            pl.num_trajectory_ = n - 1
            pl.n_elite_ = N_ELITE
            pl.std_min_ = pl.std_initial_   # (the noise keeps its first plan's width: returns that a fitted variance has drawn within 5 % of each other park nothing)
            pl.allocate()
        finally:
            os.environ.pop("MJPCX_QUAD_MIN_N", None)
        assert pl.pruning is False and pl.park_slack == 0.05   # off by default
        pl.pruning = pruning
        pl.reset(H)
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
            log.append(dict(values=[p.policy.plan.values().copy() for p in pl.envs], times=[p.policy.plan.times().copy() for p in pl.envs],
                            variance=[p.variance.copy() for p in pl.envs], order=[list(p.trajectory_order) for p in pl.envs],
                            improvement=[p.improvement for p in pl.envs], trs=[{k: getattr(tr, k).copy() for k in BUFFERS} for tr in trs],
                            hints=pl.park_hints_used, repeated=pl.pruned_launch_repeated,
                            prune=None if pl.prune_stats is None else {k: v.copy() for k, v in pl.prune_stats.items()},
                            park=None if pl.park_stats is None else {k: v.copy() for k, v in pl.park_stats.items()},
                            worst=[float(pl.ctx.returns()[0][e * n + p.trajectory_order[-1]]) for e, p in enumerate(pl.envs)]))
            for e in range(E):
                sts[e].set(trs[e].states[1, :m.nq], trs[e].states[1, m.nq:], mocap_pos=MOCAP.reshape(-1, 7)[:, :3], mocap_quat=MOCAP.reshape(-1, 7)[:, 3:],
                           time=float(trs[e].times[1]))
        runs[pruning] = log
        pl.ctx.close()
    for step, (a, b) in enumerate(zip(runs[False], runs[True])):
        assert a["order"] == b["order"] and a["improvement"] == b["improvement"], step
        for e in range(E):
            assert np.array_equal(a["values"][e], b["values"][e]) and np.array_equal(a["times"][e], b["times"][e]), (step, e)
            assert np.array_equal(a["variance"][e], b["variance"][e]), (step, e)
            for k in BUFFERS:
                assert np.array_equal(a["trs"][e][k], b["trs"][e][k]), (step, e, k)
        assert a["hints"] is None and a["prune"] is None and a["park"] is None and not b["repeated"]
        assert not b["prune"]["negative_cost"].any()
        if step == 0:
            assert np.isinf(b["hints"]).all() and not b["park"]["parked"].any()
        else:
            # the hint is the previous plan's worst elite return x 1.05 (none for a robot whose previous plan resumed more than a quarter of
            # its candidates: its hint was stale), and something was parked on it
            before = runs[True][step - 1]
            stale = before["park"]["resumed"] > 0.25 * n
            assert np.array_equal(b["hints"], np.where(stale, INF, np.array(before["worst"]) * 1.05)), step
            assert b["park"]["parked"].sum() >= 1, (step, b["park"])
