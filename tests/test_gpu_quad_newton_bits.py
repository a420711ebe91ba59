"""-m gpu: rollout_quad_kernel computes, bit for bit, what it computed before the Newton solver's statements were reordered for the
register allocator. N = 2048 (the smallest batch the kernel serves without being asked to: 128 wavefronts of 16
candidates), H = 6, noise std 0.1, from

  home          the keyframe: four feet on the floor from the first steps
  two_lanes_on  the start state of tests/test_gpu_quad_pair_walk.py: a front foot coming onto the calf of the rear leg of its side, the
                trunk 0.45 m up (self-collision rows in about half of the candidates)
  trot          the contact-rich trot state of the step bank (tests/test_quad_park_emulator.py's: feet, calves, a thigh and a hip on the floor)

* every return and every failure word `array_equal` to tests/golden/quad_newton_bits_device.npz, recorded on an MI355X from the build of
  that round's parent commit (tools/record_quad_newton_bits.py --device);
* the rows of 32 candidates spread over the batch against the CPU emulator of the same source (tests/quademu), every Trajectory buffer
  and the return, |d - e| <= 1e-9 (1 + |e|), the bound of the other quad suites."""
import os

import numpy as np
import pytest

import step_bank as sb
import test_quad_pair_walk_emulator as walk
from mujoco_mpc_amd import capi
from oracle import pyoracle
from tests import quademu

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_newton_bits_device.npz")
N, H, P = 2048, 6, 3
TIMES = np.arange(P) * ((H - 1) * 0.01 / (P - 1))
NOMINAL = np.zeros((P, 12))
SAMPLE = np.arange(5, N, 64)      # 32 candidates, one in every fourth wavefront
STARTS = ("home", "two_lanes_on", "trot")


def close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * (1 + np.abs(b)))


def noise():
    return capi.make_noise_spec(seed=23, iteration=1, mode=capi.NOISE_SAMPLING, std0=0.1)


def start(which):
    """(state, time, mocap)"""
    task = walk.cull._task()
    if which == "home":
        return np.concatenate([task.model.keyframes["home"]["qpos"], np.zeros(18)]), 0.0, walk.MOCAP
    if which == "two_lanes_on":
        return walk.sweep_states("foot_on_the_calf_two_lanes_on")[24].state, 0.0, walk.MOCAP
    s = next(s for s in sb.a1_bank().states if s.label.startswith("trot3/"))
    return s.state, s.time, s.mocap


def launch(which):
    """the batch from the start state -> dict(ret, failure, failure_raw, handed_on, rows: {candidate: {field: array}})"""
    task = walk.cull._task()
    state, time, mocap = start(which)
    ctx = capi.Context(task.packed_model(), task.packed(), 0, 64)
    try:
        assert "rollout_quad_kernel" in ctx.kernel_name
        ctx.set_state(state, time, mocap)
        ctx.rollout_noise(N, H, 0, TIMES + time, NOMINAL, noise())
        ret, fail = ctx.returns()
        out = dict(ret=ret.copy(), failure=np.asarray(fail).copy(), failure_raw=ctx.failure_raw.copy(), handed_on=ctx.quad_stats()["handed_on"])
        out["rows"] = {int(c): {k: np.array(getattr(tr, k)) for k in sb.FIELDS} for c, tr in ((c, ctx.fetch_trajectory(int(c))) for c in SAMPLE)}
    finally:
        ctx.close()
    return out


@pytest.fixture(scope="module")
def results():
    return {w: launch(w) for w in STARTS}


@pytest.mark.parametrize("which", STARTS)
def test_returns_and_failure_words_equal_the_parent_builds(results, which):
    g = np.load(GOLDEN)
    r = results[which]
    print(f"{which}: handed on {r['handed_on']} (recorded {int(g[which + '_handed_on'])}), returns {r['ret'].min():.4f}..{r['ret'].max():.4f}, "
          f"{int(np.sum(r['ret'] != g[which + '_ret']))} returns and {int(np.sum(r['failure_raw'] != g[which + '_failure_raw']))} failure words differ")
    assert np.all(np.isfinite(r["ret"]))
    assert np.array_equal(r["ret"], g[which + "_ret"])
    assert np.array_equal(r["failure_raw"], g[which + "_failure_raw"]) and np.array_equal(r["failure"], g[which + "_failure"])
    assert r["handed_on"] == int(g[which + "_handed_on"])


@pytest.mark.parametrize("which", STARTS)
def test_rows_follow_the_emulator_of_the_same_source(results, which):
    task = walk.cull._task()
    pm, pt = task.packed_model(), task.packed()
    state, time, mocap = start(which)
    r = results[which]
    nodes = pyoracle.noise_candidates(pm, noise(), P, NOMINAL, SAMPLE)
    emu = quademu.rollout(pm, pt, state, time, mocap, len(SAMPLE), H, P, 0, TIMES + time, node_values=nodes)
    ok = (emu["flags"] == 0) & (r["failure"][SAMPLE] == 0)
    # what the compared candidates' solver works on, by the oracle's contact lists of the emulator's states
    contacts = walk.leg_contacts()
    leg_leg = sum(1 for i in np.flatnonzero(ok) if any(contacts(emu["states"][i, t], time, mocap) for t in range(H)))
    feats = set().union(*[sb.state_features(task, emu["states"][i, H - 1], time, mocap) for i in np.flatnonzero(ok)[:8]])
    worst = float(np.max(np.abs(r["ret"][SAMPLE][ok] - emu["total_return"][ok]) / (1 + np.abs(emu["total_return"][ok]))))
    print(f"{which}: {int(ok.sum())} of {len(SAMPLE)} candidates compared, {leg_leg} of them with a leg-leg contact, features at the last state {sorted(feats)}, "
          f"worst relative error of the returns {worst:.2e}")
    assert ok.sum() >= len(SAMPLE) - 4
    if which == "two_lanes_on":
        assert leg_leg >= 4
    else:
        assert "floor" in feats
    assert close(r["ret"][SAMPLE][ok], emu["total_return"][ok], 1e-9), worst
    for i, c in enumerate(SAMPLE):
        if ok[i]:
            for k in sb.FIELDS:
                assert close(r["rows"][int(c)][k], emu[k][i], 1e-9), (which, int(c), k)
