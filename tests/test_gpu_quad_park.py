"""-m gpu: parking in rollout_quad_kernel (mjpcx_set_park_hint). In a pruned launch a candidate whose partial return strictly exceeds the
caller's UNPROVEN estimate of the best return is set aside with its state; the settling pass retires it if its partial return is above the
launch's final bound, rollout_quad_resume_kernel continues it otherwise. The hint may change no result: what the plan step reads, and every
candidate not marked pruned, equals the unpruned launch bit for bit, whatever the hint. With the initial bound at the unpruned minimum the
bound never moves, and which candidates are parked (and when), settled and resumed is a function of the unpruned costs that numpy computes
(tests/test_quad_park_emulator.py checks the same function against the emulator; test_device_equals_the_emulator runs the emulator
beside the device for each hint).

The bench's initial condition and noise, N = 128, H = 30, fp64, at 4 and at 16 candidates per wavefront (a parked quad then shares its
wavefront with live ones); MJPCX_QUAD_MIN_N is set before the context is created so that small batches reach the quad kernel."""
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
PARKED, PRUNED, FALLBACK = 0x10000000, 0x20000000, 0x40000000
BUFFERS = ("states", "actions", "times", "residual", "costs", "trace")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINTS = ("inf", "best", "1.05 best", "0.5 best", "zero")


def hint_value(name, best):
    return {"inf": np.inf, "best": best, "1.05 best": 1.05 * best, "0.5 best": 0.5 * best, "zero": 0.0}[name]


def noise():
    return capi.make_noise_spec(seed=0, iteration=1, mode=capi.NOISE_SAMPLING, std0=0.04)


@pytest.fixture(scope="module")
def quad():
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    return t


def context(t, env=None, cpw=None):
    env = dict({"MJPCX_QUAD_MIN_N": "1"}, **(env or {}))
    if cpw is not None and cpw != 4:   # (4 is what the library picks for 128 candidates)
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
    """the unpruned launch: every buffer of every candidate, the candidates' nodes, and what mjpcx_best reads"""
    ctx = context(quad)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    out = snapshot(ctx)
    out["best"] = ctx.best(0)
    out["stats"] = ctx.quad_stats()
    out["nodes"] = np.stack([ctx.fetch_spline(c) for c in range(N)])
    assert ctx.park_stats() == dict(parked=0, settled_retired=0, resumed=0, resume_ms=0.0)
    ctx.close()
    assert not out["failure"].any() and out["costs"].min() > 0 and out["stats"]["handed_on"] == 0
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def same_best(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def check_kept_and_retired(run, full, st, pk):
    """what holds after any pruned launch, hinted or not: no parked marker is left, the counts add up, every candidate not marked pruned is
    the unpruned launch's, every retired one stopped at a partial return strictly above the best"""
    partial = np.cumsum(full["costs"], axis=1) / float(H)
    assert ((run["failure"] & (PARKED | FALLBACK)) == 0).all()
    assert pk["parked"] == pk["settled_retired"] + pk["resumed"]
    kept = run["failure"] == 0
    assert kept[full["best"][0]] and kept[0]
    for k in BUFFERS + ("total_return",):
        assert np.array_equal(run[k][kept], full[k][kept]), k
    gone = ~kept
    assert ((run["failure"][gone] & PRUNED) != 0).all()
    t = (run["failure"][gone] >> 8) & 0xFFFF
    assert (t < H - 1).all()
    assert np.array_equal(run["total_return"][gone], partial[gone, t]) and (run["total_return"][gone] > full["best"][1]).all()
    for c, tc in zip(np.nonzero(gone)[0], t):
        for k in BUFFERS:
            assert np.array_equal(run[k][c, :tc + 1], full[k][c, :tc + 1]), (k, c)
    assert st["retired"] == gone.sum() and st["retire_step_sum"] == t.sum() and not st["negative_cost"]


@pytest.mark.parametrize("cpw", [4, 16])
def test_what_the_plan_step_reads_does_not_depend_on_the_hint(quad, full, cpw):
    """the planner's launch (bound from +inf) under every hint: argmin, best return, the nominal's return, the winner's spline and its rows in
    all six buffers are the unpruned launch's"""
    ctx = context(quad, cpw=cpw)
    ctx.set_pruning(True)
    w, best = full["best"][0], full["best"][1]
    for name in HINTS:
        ctx.set_park_hint(hint_value(name, best))
        ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
        assert same_best(ctx.best(0), full["best"]), name
        idx, ret = ctx.topk(1)
        assert idx[0] == w and ret[0] == best
        run = snapshot(ctx)
        for k in BUFFERS + ("total_return",):
            assert np.array_equal(run[k][w], full[k][w]), (name, k)
            assert np.array_equal(run[k][0], full[k][0]), (name, k)   # the nominal
        pk = ctx.park_stats()
        check_kept_and_retired(run, full, ctx.prune_stats(), pk)
        assert ctx.quad_stats() == full["stats"]
        if name == "inf":
            assert pk["parked"] == 0
        if name == "zero":   # every candidate but the nominal passes 0 at its first step; the winner is among the resumed
            assert pk["parked"] == N - 1 and pk["resumed"] >= 1 and pk["resume_ms"] > 0
        if name == "0.5 best":
            assert pk["parked"] > 0 and pk["resumed"] >= (1 if w != 0 else 0)
    ctx.close()


def expected_with_fixed_bound(costs, bound, hint, nominal=0):
    """bound fixed at the launch's minimum: per candidate the park step (-1: never) and the final retire step (-1: completes). Per step
    the proven test comes first, then the hint; neither at the last step; never the nominal. The settling rule cannot retire anything here:
    the proven test has just failed against the same bound, so every parked candidate is resumed"""
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


@pytest.mark.parametrize("cpw", [4, 16])
def test_bound_at_the_minimum_parks_settles_and_resumes_exactly_the_computed_sets(quad, full, cpw):
    best = full["best"][1]
    ctx = context(quad, cpw=cpw)
    ctx.set_pruning(True, best)
    for name in HINTS:
        hint = hint_value(name, best)
        parked, final, partial = expected_with_fixed_bound(full["costs"], best, hint)
        ctx.set_park_hint(hint)
        ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
        assert same_best(ctx.best(0), full["best"]), name
        pk = ctx.park_stats()
        assert (pk["parked"], pk["settled_retired"], pk["resumed"]) == ((parked >= 0).sum(), 0, (parked >= 0).sum()), name
        idx, step = ctx.park_resumed()
        assert np.array_equal(idx, np.nonzero(parked >= 0)[0]) and np.array_equal(step, parked[parked >= 0]), name
        if name in ("inf", "best", "1.05 best"):
            assert pk["parked"] == 0   # at or above the minimum the proven test retires first
        else:
            assert pk["parked"] > 0
        retired = final >= 0
        run = snapshot(ctx)
        assert np.array_equal(run["failure"], np.where(retired, PRUNED | (final << 8), 0)), name
        last = np.where(retired, final, H - 1)
        assert np.array_equal(run["total_return"], partial[np.arange(N), last])
        for c in range(N):   # (the resumed candidates among them: rows written by two launches)
            for k in BUFFERS:
                assert np.array_equal(run[k][c, :last[c] + 1], full[k][c, :last[c] + 1]), (name, k, c)
        st = ctx.prune_stats()
        assert st["retired"] == retired.sum() and st["retire_step_sum"] == final[retired].sum() and not st["negative_cost"]
    ctx.close()


@pytest.mark.parametrize("name", HINTS)
def test_device_equals_the_emulator(quad, full, name):
    """the same candidates (the device's nodes) through the emulator's main pass, settling rule and resume pass, bound at the minimum, for
    each hint: the counts, park steps, the resumed set, flags, returns and the resumed candidates' rows. Hint 0 parks the whole batch at step
    0 and resumes it wholesale, the solver starting cold in the resume launch"""
    from tests.quademu import park
    best = full["best"][1]
    hint = hint_value(name, best)
    state = np.concatenate([quad.model.keyframes["home"]["qpos"], np.zeros(18)])
    emu = park.rollout(quad.packed_model(), quad.packed(), state, 0.0, MOCAP, N, H, P, capi.SPLINE_ZERO, TIMES, full["nodes"], nominal_candidate=0,
                       initial_bound=best, hint=hint)
    ctx = context(quad, cpw=16)
    ctx.set_pruning(True, best)
    ctx.set_park_hint(hint)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    pk = ctx.park_stats()
    assert (pk["parked"], pk["settled_retired"], pk["resumed"]) == (emu["parked"], emu["settled_retired"], emu["resumed_count"])
    parked, _, _ = expected_with_fixed_bound(full["costs"], best, hint)
    assert np.array_equal(emu["park_step"], parked)   # (the emulator's park steps are also what numpy computes from the device's costs)
    if name in ("inf", "best", "1.05 best"):
        assert pk["parked"] == 0
    else:
        assert pk["resumed"] > 0
    if name == "zero":
        assert (emu["park_step"][emu["resumed"]] == 0).all() and pk["resumed"] >= N // 2
    idx, step = ctx.park_resumed()
    assert np.array_equal(idx, np.nonzero(emu["resumed"])[0]) and np.array_equal(step, emu["park_step"][emu["resumed"]])
    run = snapshot(ctx)
    assert np.array_equal(run["failure"], emu["failure"])
    # (the device's returns and rows equal the device's unpruned launch bit for bit -- the tests above; against the emulator, whose host
    # compiler rounds differently from the device's fused arithmetic, the flags and steps are exact and the numbers agree closely)
    assert np.allclose(run["total_return"], emu["total_return"], rtol=1e-9, atol=0)
    for c in idx:
        t = H - 1 if run["failure"][c] == 0 else (run["failure"][c] >> 8) & 0xFFFF
        for k in BUFFERS:
            assert np.array_equal(run[k][c, :t + 1], full[k][c, :t + 1]), (k, c)
    ctx.close()


def test_a_handed_on_candidate_among_the_resumed_is_still_rolled_out(quad):
    """MJPCX_QUAD_CON_CAP=1 hands on every candidate a leg of which holds two contacts at some step. Hint 0 parks everything but the nominal
    at step 0, so every hand-on happens in the resume launch; the fallback kernel rolls those candidates out as it does after a plain launch"""
    runs = {}
    for hinted in (False, True):
        ctx = context(quad, {"MJPCX_QUAD_CON_CAP": "1"})
        ctx.set_pruning(hinted)
        ctx.set_park_hint(0.0 if hinted else np.inf)
        ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
        runs[hinted] = (snapshot(ctx, trajectories=False), ctx.quad_stats(), ctx.best(0), ctx.park_stats(), ctx.prune_stats())
        ctx.close()
    (a, sa, ba, pa, _), (b, sb_, bb, pb, st) = runs[False], runs[True]
    assert sa["handed_on"] > 0 and pa["parked"] == 0
    assert pb["parked"] == N - 1 and pb["resumed"] >= 1
    assert same_best(ba, bb)
    assert ((b["failure"] & PARKED) == 0).all()
    gone = (b["failure"] & PRUNED) != 0
    assert np.array_equal(b["failure"][~gone], a["failure"][~gone]) and np.array_equal(b["total_return"][~gone], a["total_return"][~gone])
    assert st["retired"] == gone.sum() and (b["total_return"][gone] > ba[1]).all() and (b["total_return"][gone] < 1.0e6).all()
    # which candidates the quad kernel hands on, and at which step: a plain launch that leaves them flagged. One handed on at a step >= 1
    # and not retired in the hinted run was parked at step 0 there, so its hand-on happened in the resume launch; some such candidate other
    # than the nominal must exist, end unflagged and carry the unhinted run's return (asserted for every kept candidate above)
    ctx = context(quad, {"MJPCX_QUAD_CON_CAP": "1", "MJPCX_QUAD_NO_FALLBACK": "1"})
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    flagged = snapshot(ctx, trajectories=False)["failure"]
    ctx.close()
    after_resume = ((flagged & FALLBACK) != 0) & (((flagged >> 8) & 0xFFFF) >= 1) & ~gone
    after_resume[0] = False
    assert after_resume.any() and sb_["handed_on"] >= after_resume.sum()
    assert ((b["failure"][after_resume] & FALLBACK) == 0).all() and (b["total_return"][after_resume] < 1.0e6).all()
    # the nominal's own hand-on (if any) happened in the main launch; all others' in the resume launch, and they were rolled out
    assert 0 < sb_["handed_on"] <= sa["handed_on"]


def test_without_pruning_the_hint_is_ignored_by_noise_and_given_splines(quad, full):
    ctx = context(quad)
    ctx.set_park_hint(0.0)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    run = snapshot(ctx, trajectories=False)
    assert np.array_equal(run["total_return"], full["total_return"]) and not run["failure"].any()
    assert ctx.park_stats()["parked"] == 0 and ctx.prune_stats()["retired"] == 0
    ctx.rollout_splines(H, capi.SPLINE_ZERO, TIMES, full["nodes"])
    run = snapshot(ctx, trajectories=False)
    assert np.array_equal(run["total_return"], full["total_return"]) and not run["failure"].any()
    assert ctx.park_stats()["parked"] == 0
    ctx.topk(4)  # (not refused: nothing was retired)
    for bad in (-1.0, float("nan")):
        with pytest.raises(capi.MjpcxError) as e:
            ctx.set_park_hint(bad)
        assert e.value.code == -1  # MJPCX_EINVAL
    ctx.close()


def test_park_switch_off_in_the_environment(quad, full):
    """MJPCX_PARK=0 at creation: the hint does nothing, the launch is the pruned launch"""
    ctx = context(quad, {"MJPCX_PARK": "0"})
    ctx.set_pruning(True)
    ctx.set_park_hint(0.0)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    assert ctx.park_stats() == dict(parked=0, settled_retired=0, resumed=0, resume_ms=0.0)
    assert same_best(ctx.best(0), full["best"])
    check_kept_and_retired(snapshot(ctx), full, ctx.prune_stats(), ctx.park_stats())
    ctx.close()


def test_the_no_fallback_tuning_switch_ignores_the_hint(quad, full):
    ctx = context(quad, {"MJPCX_QUAD_NO_FALLBACK": "1"})
    ctx.set_pruning(True)
    ctx.set_park_hint(0.0)
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    run = snapshot(ctx, trajectories=False)
    assert np.array_equal(run["total_return"], full["total_return"]) and not run["failure"].any()
    assert ctx.park_stats()["parked"] == 0
    ctx.close()


@pytest.mark.parametrize("E", [1, 2])
def test_batched_launches_ignore_the_hint(quad, E):
    n = 64
    state = np.concatenate([quad.model.keyframes["home"]["qpos"], np.zeros(18)])
    got = []
    for hinted in (False, True):
        ctx = context(quad)
        ctx.set_pruning(hinted)
        ctx.set_park_hint(0.0 if hinted else np.inf)
        ctx.set_states(np.stack([state] * E), np.zeros(E), np.stack([MOCAP] * E))
        ctx.rollout_noise_batched(n, H, capi.SPLINE_ZERO, np.stack([TIMES] * E), np.stack([NOMINAL] * E), noise(), num_envs=E)
        got.append(snapshot(ctx))
        assert ctx.park_stats()["parked"] == 0 and ctx.prune_stats()["retired"] == 0
        ctx.topk(4)
        ctx.close()
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


def test_the_limb_kernel_ignores_the_hint():
    t = load_task("HumanoidTrack")
    e = t.transition(0.0, mode=9)
    state = np.concatenate([e["qpos"], e["qvel"]])
    mocap = np.concatenate([np.concatenate([p, [1, 0, 0, 0]]) for p in np.asarray(e["mocap_pos"]).reshape(-1, 3)])
    n, h, p = 16, 12, 3
    nodes = np.clip(np.random.default_rng(1).normal(0, 0.3, (n, p, t.model.nu)), -1, 1)
    times = np.arange(p) * 0.05
    got = []
    for hinted in (False, True):
        os.environ["MJPCX_LIMB_MIN_N"] = "0"
        try:
            ctx = capi.Context(t.packed_model(), t.packed(), 0, 64)
        finally:
            os.environ.pop("MJPCX_LIMB_MIN_N", None)
        assert ctx.kernel_name.startswith("rollout_limb_kernel")
        ctx.set_pruning(hinted)
        ctx.set_park_hint(0.0 if hinted else np.inf)
        ctx.set_state(state, 0.0, mocap)
        ctx.rollout_splines(h, capi.SPLINE_ZERO, times, nodes)
        got.append(snapshot(ctx))
        assert ctx.park_stats()["parked"] == 0 and ctx.prune_stats()["retired"] == 0
        ctx.close()
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


def test_rankings_are_refused_after_a_hinted_launch_that_retired_anything(quad, full):
    ctx = context(quad)
    ctx.set_pruning(True)
    ctx.set_park_hint(1.05 * full["best"][1])
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, noise())
    assert ctx.prune_stats()["retired"] > 0
    with pytest.raises(capi.MjpcxError) as e:
        ctx.topk(4)
    assert e.value.code == -5  # MJPCX_ESTATE
    with pytest.raises(capi.MjpcxError) as e:
        ctx.elite_moments([0, 1, 2])
    assert e.value.code == -5
    idx, ret = ctx.topk(1)
    assert idx[0] == full["best"][0] and ret[0] == full["best"][1]
    ctx.close()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mujoco_mpc_amd.hostplanner import HostPlanner
from mujoco_mpc_amd.task import load_task
task = load_task("QuadrupedFlat")
H = 30
pl = HostPlanner(task, device=0, precision=64, seed=0, num_trajectory=2048, kind="sampling")
pl.park_set(float(sys.argv[3]))
pl.task_transition(0.0)
home = task.model.keyframes["home"]
pl.reset(H)
qpos, qvel, time = np.array(home["qpos"], float), np.zeros(task.model.nv), 0.0
out = {}
for step in range(10):
    pl.set_state(qpos, qvel, time)
    pl.optimize_policy(H)
    times, values = pl.policy()
    best = pl.best_trajectory(cap=512)
    info = pl.park_info()
    out.update({f"times{step}": times, f"values{step}": values, f"winner{step}": np.array([pl.winner]), f"score{step}": np.array([pl.best_score]),
                f"improvement{step}": np.array([pl.improvement]), f"parked{step}": np.array([info["parked"]]), f"resumed{step}": np.array([info["resumed"]]),
                f"hinted{step}": np.array([np.isfinite(info["hint"])])})
    for k in ("states", "actions", "times", "costs"):
        out[f"best_{k}{step}"] = np.asarray(best[k])
    out[f"best_return{step}"] = np.array([best["total_return"]])
    # the robot moves: the next plan starts from the second state of this plan's best trajectory
    s = np.asarray(best["states"])[1]
    qpos, qvel, time = s[:task.model.nq].copy(), s[task.model.nq:task.model.nq + task.model.nv].copy(), float(np.asarray(best["times"])[1])
np.savez(sys.argv[2], **out)
pl.close()
"""


def test_the_planner_computes_the_same_policy_with_and_without_parking(tmp_path):
    """HostPlanner(kind="sampling") on QuadrupedFlat, 2048 x 30, ten plans with the state advanced along the best trajectory between them,
    each run in a fresh child process because MJPCX_PARK is read when the context is created. The slack is lowered to -0.3 (hint = 0.7 x the
    previous best: below what the launch will find) so that the resume path is taken for certain; policy and best trajectory are equal"""
    script = tmp_path / "plan.py"
    script.write_text(CHILD)
    runs = {}
    for name, value in (("parked", None), ("off", "0")):
        env = dict(os.environ)
        env.pop("MJPCX_PARK", None)
        if value is not None:
            env["MJPCX_PARK"] = value
        out = tmp_path / (name + ".npz")
        done = subprocess.run([sys.executable, str(script), ROOT, str(out), "-0.3"], env=env, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-2000:]
        runs[name] = dict(np.load(out))
    a, b = runs["parked"], runs["off"]
    assert set(a) == set(b)
    for k in a:
        if not k.startswith(("parked", "resumed", "hinted")):
            assert np.array_equal(a[k], b[k]), k
    assert all(b[f"parked{s}"][0] == 0 for s in range(10))
    assert not a["hinted0"][0] and a["hinted1"][0]   # (the first plan has no previous best)
    assert sum(a[f"resumed{s}"][0] for s in range(10)) > 0 and sum(a[f"parked{s}"][0] for s in range(10)) > 0
