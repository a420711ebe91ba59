"""-m gpu: pruning in rollout_quad_kernel (mjpcx_set_pruning): candidates whose partial return strictly exceeds a return that another
candidate of the launch has completed with are retired. WHICH candidates are retired, and when, depends on the order the wavefronts
finish in; what the plan step reads (the argmin, its return, the nominal's return, the winner's spline and trajectory) may not, and every
candidate not marked pruned must equal the unpruned launch bit for bit. With the initial bound at the unpruned minimum the bound can never
move, and the retired set is a function of the unpruned costs that numpy computes.

The bench's initial condition and noise (home keyframe, sigma 0.04, 3 zero-order-hold nodes), N = 128, H = 30, fp64; MJPCX_QUAD_MIN_N is
set before the context is created so that small batches reach the quad kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
N, H, P = 128, 30, 3
TIMES = np.arange(P) * ((H - 1) * 0.01 / P)
NOMINAL = np.zeros((P, 12))
PRUNED = 0x20000000  # MJPCX_FAILURE_PRUNED
FALLBACK = 0x40000000
BUFFERS = ("states", "actions", "times", "residual", "costs", "trace")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noise():
    return capi.make_noise_spec(seed=0, iteration=1, mode=capi.NOISE_SAMPLING, std0=0.04)


@pytest.fixture(scope="module")
def quad():
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    return t


def context(t, env=None):
    env = dict({"MJPCX_QUAD_MIN_N": "1"}, **(env or {}))
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


def snapshot(ctx, trajectories=True):
    ret, _ = ctx.returns()
    out = dict(total_return=ret.copy(), failure=ctx.failure_raw.copy())
    if trajectories:
        trs = [ctx.fetch_trajectory(c) for c in range(ctx.N)]
        for k in BUFFERS:
            out[k] = np.stack([getattr(tr, k) for tr in trs])
    return out


@pytest.fixture(scope="module")
def full(quad):
    """the unpruned launch: every buffer of every candidate, and what mjpcx_best reads"""
    ctx = context(quad)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    out = snapshot(ctx)
    out["best"] = ctx.best(0)
    out["stats"] = ctx.quad_stats()
    assert ctx.prune_stats()["retired"] == 0
    ctx.close()
    assert not out["failure"].any() and out["costs"].min() > 0
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def same_best(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_what_the_plan_step_reads_does_not_depend_on_pruning(quad, full):
    ctx = context(quad)
    ctx.set_pruning(True)
    partial = np.cumsum(full["costs"], axis=1) / float(H)
    w = full["best"][0]
    for _ in range(3):  # the pruned set may differ between launches; these outputs may not
        ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
        assert same_best(ctx.best(0), full["best"])
        run = snapshot(ctx)
        for k in BUFFERS + ("total_return",):
            assert np.array_equal(run[k][w], full[k][w]), k
        kept = run["failure"] == 0
        assert kept[w] and kept[0]
        for k in BUFFERS + ("total_return",):
            assert np.array_equal(run[k][kept], full[k][kept]), k
        gone = ~kept
        assert ((run["failure"][gone] & PRUNED) != 0).all() and ((run["failure"][gone] & FALLBACK) == 0).all()
        t = (run["failure"][gone] >> 8) & 0xFFFF
        assert (t < H - 1).all()
        assert np.array_equal(run["total_return"][gone], partial[gone, t]) and (run["total_return"][gone] > full["best"][1]).all()
        for c, tc in zip(np.nonzero(gone)[0], t):
            for k in BUFFERS:
                assert np.array_equal(run[k][c, :tc + 1], full[k][c, :tc + 1]), (k, c)
        st = ctx.prune_stats()
        assert st["retired"] == gone.sum() and st["retire_step_sum"] == t.sum() and not st["negative_cost"]
        assert ctx.quad_stats() == full["stats"]
    ctx.close()


@pytest.mark.parametrize("cpw", [4, 16])
def test_bound_at_the_minimum_retires_exactly_the_computed_set(quad, full, cpw):
    """cpw: candidates per wavefront. 4 is what the library picks for 128 candidates (left to it here), 16 the full batches' (MJPCX_QUAD_CPW):
    a wavefront of several quads ends early iff ALL of its candidates were retired, and its first quad's leg 0 counts it"""
    assert full["stats"]["handed_on"] == 0  # (a candidate handed on before the last step would end its wavefront's share early too)
    best = full["best"][1]
    partial = np.cumsum(full["costs"], axis=1) / float(H)
    steps = np.full(N, -1)
    for c in range(1, N):  # (candidate 0 is the nominal)
        over = np.nonzero(partial[c, :H - 1] > best)[0]
        if len(over):
            steps[c] = over[0]
    retired = steps >= 0
    assert 0 < retired.sum() < N - 1
    ctx = context(quad, {} if cpw == 4 else {"MJPCX_QUAD_CPW": str(cpw)})
    ctx.set_pruning(True, best)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    assert same_best(ctx.best(0), full["best"])
    idx, ret = ctx.topk(1)
    assert idx[0] == full["best"][0] and ret[0] == best
    run = snapshot(ctx, trajectories=False)
    assert np.array_equal(run["failure"], np.where(retired, PRUNED | (steps << 8), 0))
    assert np.array_equal(run["total_return"], np.where(retired, partial[np.arange(N), np.maximum(steps, 0)], full["total_return"]))
    st = ctx.prune_stats()
    assert st["retired"] == retired.sum() and st["retire_step_sum"] == steps[retired].sum() and not st["negative_cost"]
    ended = retired.reshape(N // cpw, cpw).all(axis=1)
    assert not ended[0] and (cpw == 16 or ended.any())  # (the nominal's wavefront never ends early; at 4 per wavefront some do)
    assert st["wavefronts_ended_early"] == ended.sum()
    ctx.close()


def test_handed_on_candidates_are_still_rolled_out_and_pruned_ones_are_not(quad):
    """MJPCX_QUAD_CON_CAP=1 hands on every candidate a leg of which holds two contacts at some step. They never lower the bound (their
    return is not known inside the launch) and the other kernel rolls them out as before; the hand-on statistics do not change. (That
    last equality holds as long as no candidate is retired before the step it would have been handed on at: nothing can be retired
    before some wavefront has finished all H steps, and the wavefronts of a launch this small run side by side. Per candidate, what
    cannot depend on timing is asserted below it: every candidate not marked pruned has the unpruned run's flag and return.)"""
    runs = {}
    for pruning in (False, True):
        ctx = context(quad, {"MJPCX_QUAD_CON_CAP": "1"})
        ctx.set_pruning(pruning)
        ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
        runs[pruning] = (snapshot(ctx, trajectories=False), ctx.quad_stats(), ctx.best(0), ctx.prune_stats())
        ctx.close()
    (a, sa, ba, _), (b, sb, bb, pb) = runs[False], runs[True]
    assert 0 < sa["handed_on"] and sa == sb
    assert same_best(ba, bb)
    gone = (b["failure"] & PRUNED) != 0
    assert np.array_equal(b["failure"][~gone], a["failure"][~gone]) and np.array_equal(b["total_return"][~gone], a["total_return"][~gone])
    assert pb["retired"] == gone.sum() and (b["total_return"][gone] > ba[1]).all() and (b["total_return"][gone] < 1.0e6).all()


def test_a_bound_below_every_return_is_reported(quad, full):
    ctx = context(quad)
    ctx.set_pruning(True, 0.0)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    with pytest.raises(capi.MjpcxError) as e:
        ctx.best(0)
    assert e.value.code == -5  # MJPCX_ESTATE
    assert ctx.prune_stats()["retired"] == N - 1
    # ... and negative or NaN bounds are refused
    for bad in (-1.0, float("nan")):
        with pytest.raises(capi.MjpcxError) as e:
            ctx.set_pruning(True, bad)
        assert e.value.code == -1  # MJPCX_EINVAL
    ctx.set_pruning(False)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    assert same_best(ctx.best(0), full["best"])
    ctx.close()


def test_a_wrong_bound_shows_on_given_splines_and_when_a_candidate_slips_past_it_at_the_last_step(quad, full):
    """mjpcx_rollout_splines has no nominal: under a bound of 0 all N candidates are retired. And the last step is never checked: with
    the bound at the winner's partial return one step before the end, the winner completes ABOVE the bound -- something completed, yet the
    bound was below every return, every stored return is above it, and mjpcx_best (and the argmin of mjpcx_topk) must say so"""
    ctx = context(quad)
    nodes = np.clip(np.random.default_rng(2).normal(0, 0.04, (N, P, 12)), -1, 1)
    ctx.set_pruning(True, 0.0)
    ctx.rollout_splines(H, capi.SPLINE_ZERO, TIMES, nodes)
    assert ctx.prune_stats()["retired"] == N
    for call in (lambda: ctx.best(-1), lambda: ctx.topk(1)):
        with pytest.raises(capi.MjpcxError) as e:
            call()
        assert e.value.code == -5
    w = full["best"][0]
    partial = np.cumsum(full["costs"], axis=1) / float(H)
    bound = partial[w, H - 2]
    assert bound < full["total_return"].min()
    ctx.set_pruning(True, bound)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    ret, _ = ctx.returns()
    assert ctx.failure_raw[w] == 0 and ret[w] == full["total_return"][w] and 0 < ctx.prune_stats()["retired"] < N - 1
    for call in (lambda: ctx.best(0), lambda: ctx.topk(1)):
        with pytest.raises(capi.MjpcxError) as e:
            call()
        assert e.value.code == -5
    ctx.close()


def test_the_no_fallback_tuning_switch_is_not_pruned(quad, full):
    ctx = context(quad, {"MJPCX_QUAD_NO_FALLBACK": "1"})
    ctx.set_pruning(True)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    run = snapshot(ctx, trajectories=False)
    assert np.array_equal(run["total_return"], full["total_return"]) and not run["failure"].any()
    assert ctx.prune_stats()["retired"] == 0 and same_best(ctx.best(0), full["best"])
    ctx.topk(4)
    ctx.close()


def test_rankings_are_refused_after_a_pruned_launch(quad, full):
    ctx = context(quad)
    ctx.set_pruning(True)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    with pytest.raises(capi.MjpcxError) as e:
        ctx.topk(4)
    assert e.value.code == -5
    with pytest.raises(capi.MjpcxError) as e:
        ctx.elite_moments([0, 1, 2])
    assert e.value.code == -5
    idx, ret = ctx.topk(1)
    assert idx[0] == full["best"][0] and ret[0] == full["best"][1]
    ctx.set_pruning(False)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    idx, ret = ctx.topk(4)
    order = np.argsort(full["total_return"], kind="stable")[:4]
    assert np.array_equal(idx, order) and np.array_equal(ret, full["total_return"][order])
    ctx.close()


@pytest.mark.parametrize("E", [1, 2])
def test_batched_launches_ignore_the_switch(quad, E):
    """also with ONE environment: the calls that follow a batched launch (mjpcx_best_batched, the CE and robust updates) read every return"""
    n = 64
    state = np.concatenate([quad.model.keyframes["home"]["qpos"], np.zeros(18)])
    got = []
    for pruning in (False, True):
        ctx = context(quad)
        ctx.set_pruning(pruning)
        ctx.set_states(np.stack([state] * E), np.zeros(E), np.stack([MOCAP] * E))
        ctx.rollout_noise_batched(n, H, capi.SPLINE_ZERO, np.stack([TIMES] * E), np.stack([NOMINAL] * E), noise(), num_envs=E)
        got.append(snapshot(ctx))
        assert ctx.prune_stats()["retired"] == 0
        got[-1]["best_index"], got[-1]["best_return"], _, got[-1]["best_spline"] = ctx.best_batched(E)
        ctx.topk(4)  # (not refused: the launch was not pruned)
        ctx.close()
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


def test_the_limb_kernel_ignores_the_switch():
    t = load_task("HumanoidTrack")
    e = t.transition(0.0, mode=9)
    state = np.concatenate([e["qpos"], e["qvel"]])
    mocap = np.concatenate([np.concatenate([p, [1, 0, 0, 0]]) for p in np.asarray(e["mocap_pos"]).reshape(-1, 3)])
    n, h, p = 16, 12, 3
    nodes = np.clip(np.random.default_rng(1).normal(0, 0.3, (n, p, t.model.nu)), -1, 1)
    times = np.arange(p) * 0.05
    got = []
    for pruning in (False, True):
        os.environ["MJPCX_LIMB_MIN_N"] = "0"
        try:
            ctx = capi.Context(t.packed_model(), t.packed(), 0, 64)
        finally:
            os.environ.pop("MJPCX_LIMB_MIN_N", None)
        assert ctx.kernel_name.startswith("rollout_limb_kernel")
        ctx.set_pruning(pruning)
        ctx.set_state(state, 0.0, mocap)
        ctx.rollout_splines(h, capi.SPLINE_ZERO, times, nodes)
        got.append(snapshot(ctx))
        assert ctx.prune_stats()["retired"] == 0
        idx, _ = ctx.topk(4)  # (not refused: the launch was not pruned)
        ctx.close()
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mujoco_mpc_amd.hostplanner import HostPlanner
from mujoco_mpc_amd.task import load_task
task = load_task("QuadrupedFlat")
H = 30
pl = HostPlanner(task, device=0, precision=64, seed=0, num_trajectory=2048, kind="sampling")
pl.task_transition(0.0)
home = task.model.keyframes["home"]
pl.reset(H)
pl.set_state(np.array(home["qpos"], float), np.zeros(task.model.nv), 0.0)
out = {}
for step in range(4):
    pl.optimize_policy(H)
    times, values = pl.policy()
    best = pl.best_trajectory(cap=512)
    out.update({f"times{step}": times, f"values{step}": values, f"winner{step}": np.array([pl.winner]), f"score{step}": np.array([pl.best_score]),
                f"improvement{step}": np.array([pl.improvement]), f"retired{step}": np.array([pl.prune_stats()[0]])})
    for k in ("states", "actions", "times", "costs"):
        out[f"best_{k}{step}"] = np.asarray(best[k])
    out[f"best_return{step}"] = np.array([best["total_return"]])
np.savez(sys.argv[2], **out)
pl.close()
"""


def test_the_planner_computes_the_same_policy_with_and_without_pruning(tmp_path):
    """HostPlanner(kind="sampling") on QuadrupedFlat, 2048 x 30, four plan steps, each run in a fresh child process because MJPCX_PRUNE is
    read when the context is created"""
    script = tmp_path / "plan.py"
    script.write_text(CHILD)
    runs = {}
    for name, value in (("pruned", None), ("unpruned", "0")):
        env = dict(os.environ)
        env.pop("MJPCX_PRUNE", None)
        if value is not None:
            env["MJPCX_PRUNE"] = value
        out = tmp_path / (name + ".npz")
        done = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-2000:]
        runs[name] = dict(np.load(out))
    a, b = runs["pruned"], runs["unpruned"]
    assert set(a) == set(b)
    for k in a:
        if not k.startswith("retired"):
            assert np.array_equal(a[k], b[k]), k
    assert all(b[f"retired{s}"][0] == 0 for s in range(4))
    assert sum(a[f"retired{s}"][0] for s in range(4)) > 0  # (the pruned run did prune: the comparison compares something)
