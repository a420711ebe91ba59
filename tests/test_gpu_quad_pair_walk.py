"""-m gpu: the self-collision walk of rollout_quad_kernel (quad_step.h: pair_contacts, pair_contacts_tests -- the unrolled pretests, the
fetch of only the partner geoms and link velocities that a ballot of the wavefront names) on the device, at the smallest batch the kernel
serves without being asked to (N = 2048, 128 wavefronts of 16 candidates), H = 12, noise std 0.1, from two states of the onset sweeps of
tests/test_quad_pair_walk_emulator.py, each three states short of the first touching one, the trunk 0.45 m up:

  two_lanes_on  a front foot coming onto the calf of the rear leg of its side (legs 0 and 2: lane offset 2 from either lane)
  diagonal      a front foot coming onto the foot of the diagonal leg (legs 0 and 3: lane offsets 3 and 1)

Under the noise about half of a wavefront's candidates close the gap and half do not (the oracle on the CPU when the states were chosen:
16 and 15 of the 32 sampled candidates touch; further legs and geoms join in some of them), so the ballots that decide what the wavefront
fetches are taken over lanes that disagree -- asserted below from the oracle's contact lists.

Parity: 32 candidates spread over the batch against the oracle, every Trajectory buffer and the return, |d - o| <= 1e-9 (1 + |o|) (fp64, as
tests/test_gpu_quad_cull.py). Lock-step independence: the same launches with 16 and with 2 candidates per wavefront are bit-equal -- a
ballot only decides whether the wavefront walks a piece of code, never what a lane computes there."""
import os

import numpy as np
import pytest

import step_bank as sb
import test_quad_pair_walk_emulator as walk
from mujoco_mpc_amd import capi
from oracle import pyoracle

pytestmark = pytest.mark.gpu
MOCAP = walk.MOCAP
N, H, P = 2048, 12, 3
TIMES = np.arange(P) * ((H - 1) * 0.01 / (P - 1))
NOMINAL = np.zeros((P, 12))
SAMPLE = np.arange(5, N, 64)      # 32 candidates, one in every fourth wavefront
STARTS = {"two_lanes_on": ("foot_on_the_calf_two_lanes_on", 24), "diagonal": ("foot_on_the_diagonal_foot", 24)}   # (sweep, state of it)


def close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= tol * (1 + np.abs(b)))


def noise():
    return capi.make_noise_spec(seed=17, iteration=2, mode=capi.NOISE_SAMPLING, std0=0.1)


def start_state(which):
    name, k = STARTS[which]
    return walk.sweep_states(name)[k].state


def launch(task, state, cpw=None):
    """the batch from `state` -> (returns, failure flags, the trajectories of SAMPLE's candidates, candidates handed on)"""
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
    task = walk.cull._task()
    return task, {w: {cpw: launch(task, start_state(w), cpw) for cpw in (16, 2)} for w in STARTS}


@pytest.mark.parametrize("which", sorted(STARTS))
def test_parity_with_the_oracle_where_candidates_differ_in_what_they_touch(results, which):
    task, res = results
    ret, fail, trs, handed = res[which][16]
    pm, pt = task.packed_model(), task.packed()
    nodes = pyoracle.noise_candidates(pm, noise(), P, NOMINAL, SAMPLE)
    ref = pyoracle.rollout_batch(pm, pt, start_state(which), 0.0, MOCAP, len(SAMPLE), H, P, 0, TIMES, nodes, num_threads=8)
    # the sampled candidates differ in which partner geoms are near: by the oracle's contact lists some touch another leg and some do not
    contacts = walk.leg_contacts()
    touch = [set().union(*[contacts(ref["states"][i, t], 0.0, MOCAP) for t in range(H)]) for i in range(len(SAMPLE))]
    pair = walk.SWEEPS[STARTS[which][0]][3]
    print(f"{which}: {sum(1 for t in touch if t)} of {len(SAMPLE)} sampled candidates touch another leg: {sorted(set().union(*touch))}")
    assert any(not t for t in touch) and any(any(p == pair for _, p in t) for t in touch), touch
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
