"""-m gpu: the contact search of rollout_quad_kernel (quad_step.h: static_pretest and the wavefront ballot in front of collide_geom, one geom
body for leg and trunk geoms) on the device, at the smallest batch the kernel serves without being asked to (N = 2048, 128 wavefronts of 16
candidates), H = 12, from two states of the A1 bank (tests/step_bank.py) in which a wavefront's candidates differ in what they touch:

  trot3     feet, calves, a thigh and a hip on the floor, a calf on the neighbouring calf, a foot on another leg's hip cylinder
  tangled0  (step 49) the trunk, hips and thighs on the floor, feet on feet, calves and feet on other legs' hip cylinders

Parity: 32 candidates spread over the batch against the oracle, every Trajectory buffer and the return, |d - o| <= 1e-9 (1 + |o|) (fp64, as
tests/test_gpu_quad.py). Lock-step independence: the same launches with 16 and with 2 candidates per wavefront are bit-equal -- a ballot
only decides whether the wavefront walks a piece of code, never what a lane computes there, so a candidate's result must not depend on its
neighbours. The CPU twin (emulator, sweeps across contact onset) is tests/test_quad_cull_emulator.py."""
import os

import numpy as np
import pytest

import step_bank as sb
from mujoco_mpc_amd import capi
from oracle import pyoracle

pytestmark = pytest.mark.gpu
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
N, H, P = 2048, 12, 3
TIMES = np.arange(P) * ((H - 1) * 0.01 / (P - 1))
NOMINAL = np.zeros((P, 12))
SAMPLE = np.arange(5, N, 64)      # 32 candidates, one in every fourth wavefront
STARTS = {"trot": "trot3/", "tangled": "tangled0/step49/"}


def close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * (1 + np.abs(b)))


def noise():
    return capi.make_noise_spec(seed=17, iteration=2, mode=capi.NOISE_SAMPLING, std0=0.1)


def start_state(which):
    bank = sb.a1_bank()
    return next(s.state for s in bank.states if s.label.startswith(STARTS[which]))


def launch(task, state, cpw=None):
    """the batch from `state` -> (returns, failure flags, the trajectories of SAMPLE's first and last candidate, candidates handed on)"""
    env = {} if cpw is None else {"MJPCX_QUAD_CPW": str(cpw)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = capi.Context(task.packed_model(), task.packed(), 0, 64)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert "rollout_quad_kernel" in ctx.kernel_name
    ctx.set_state(state, 0.0, MOCAP)
    ctx.rollout_noise(N, H, 0, TIMES, NOMINAL, noise())
    ret, fail = ctx.returns()
    handed = ctx.quad_stats()["handed_on"]
    trs = {int(c): ctx.fetch_trajectory(int(c)) for c in SAMPLE}
    out = (ret.copy(), fail.copy(), {c: {k: np.array(getattr(tr, k)) for k in sb.FIELDS} for c, tr in trs.items()}, handed)
    ctx.close()
    return out


@pytest.fixture(scope="module")
def results():
    """every launch of this module once: per start state the default shape (16 candidates per wavefront) and 2 per wavefront"""
    task = sb.a1_bank().task
    return task, {w: {cpw: launch(task, start_state(w), cpw) for cpw in (16, 2)} for w in STARTS}


@pytest.mark.parametrize("which", sorted(STARTS))
def test_parity_with_the_oracle_at_the_smallest_batch(results, which):
    task, res = results
    ret, fail, trs, handed = res[which][16]
    pm, pt = task.packed_model(), task.packed()
    nodes = pyoracle.noise_candidates(pm, noise(), P, NOMINAL, SAMPLE)
    ref = pyoracle.rollout_batch(pm, pt, start_state(which), 0.0, MOCAP, len(SAMPLE), H, P, 0, TIMES, nodes, num_threads=8)
    assert handed == 0 and not fail.any() and not ref["failure"].any()   # (the quad kernel's own results, none from the kernel it hands on to)
    worst = float(np.max(np.abs(ret[SAMPLE] - ref["total_return"]) / (1 + np.abs(ref["total_return"]))))
    print(f"{which}: worst relative error of the returns {worst:.2e}")
    assert close(ret[SAMPLE], ref["total_return"], 1e-9), worst
    for i, c in enumerate(SAMPLE):
        for k in sb.FIELDS:
            assert close(trs[int(c)][k], ref[k][i], 1e-9), (which, int(c), k)


@pytest.mark.parametrize("which", sorted(STARTS))
def test_results_do_not_depend_on_the_candidates_per_wavefront(results, which):
    _, res = results
    a, b = res[which][16], res[which][2]
    assert np.all(np.isfinite(a[0])) and a[3] == 0 and b[3] == 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for c in a[2]:
        for k in sb.FIELDS:
            assert np.array_equal(a[2][c][k], b[2][c][k]), (which, c, k)
