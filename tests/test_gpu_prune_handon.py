"""-m gpu: a hand-on after a pruned launch leaves the retired candidates as they were. The quad kernel marks a retired candidate
MJPCX_FAILURE_PRUNED | (retire step << 8); the second pass of rollout_tree_kernel, which runs whenever the quad kernel handed a candidate
on, reads bit 13 of failure[] as its own "overflowed in the first pass" marker -- bit 5 of a retire step. A candidate retired at steps
32..63 must not be rolled out again there: its marker, its partial return and the counters of mjpcx_prune_stats stay.

A1, fp64, N = 128, H = 60 (the pruning tests elsewhere use H = 30, where no retire step has bit 5), MJPCX_QUAD_CON_CAP=3 so that some candidates
(those with four contacts on a leg at some step) are handed on and the others can still be retired. The initial bound is the unpruned minimum, so the bound never moves and a candidate that is not
handed on in the unpruned launch is retired exactly where numpy says."""
import os

import numpy as np
import pytest

from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
N, H, P = 128, 60, 3
TIMES = np.arange(P) * ((H - 1) * 0.01 / P)
NOMINAL = np.zeros((P, 12))
PRUNED, FALLBACK = 0x20000000, 0x40000000


def context(t, **env):
    env = dict({"MJPCX_QUAD_MIN_N": "1", "MJPCX_QUAD_CON_CAP": "3"}, **env)
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
    ctx.set_state(np.concatenate([t.model.keyframes["home"]["qpos"], np.zeros(18)]), 0.0, MOCAP)
    return ctx


def rollout(ctx):
    ctx.rollout_noise(N, H, capi.SPLINE_ZERO, TIMES, NOMINAL, capi.make_noise_spec(seed=0, iteration=1, mode=capi.NOISE_SAMPLING, std0=0.04))


def test_a_hand_on_does_not_roll_retired_candidates_out_again():
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    ctx = context(t)
    rollout(ctx)
    ret, _ = ctx.returns()
    assert not ctx.failure_raw.any() and ctx.quad_stats()["handed_on"] > 0
    costs = np.stack([ctx.fetch_trajectory(c).costs for c in range(N)])
    assert costs.min() > 0
    partial = np.cumsum(costs, axis=1) / float(H)
    best = ret.min()
    ctx.set_pruning(True, best)
    rollout(ctx)
    got, fail, st, handed = ctx.returns()[0], ctx.failure_raw.copy(), ctx.prune_stats(), ctx.quad_stats()["handed_on"]
    rows = {c: ctx.fetch_trajectory(c) for c in range(N)}
    ctx.close()
    assert handed > 0 and ((fail & FALLBACK) == 0).all()
    gone = (fail & PRUNED) != 0
    step = (fail >> 8) & 0xFFFF
    # every retirement the kernel counted is still marked, and some of them sit at steps whose bit 5 is set
    assert st["retired"] == gone.sum() and st["retire_step_sum"] == step[gone].sum()
    assert ((step[gone] & 32) != 0).any(), sorted(step[gone])
    # a retired candidate stopped where the fixed bound says, with its partial return and its rows up to that step. The unpruned launch may
    # have handed that candidate on LATER than its retire step, and then its reference rows come from the wavefront-per-candidate kernel, which
    # sums in another order: the two agree to rounding, not bit for bit. RTOL: 60 terms, each within a few units of 2^-53 -- below 1e-13
    RTOL = 1e-12
    for c in np.nonzero(gone)[0]:
        s_c = step[c]
        assert s_c < H - 1 and got[c] > best and np.isclose(got[c], partial[c, s_c], rtol=RTOL, atol=0), c
        assert s_c == 0 or partial[c, s_c - 1] <= best * (1 + RTOL), c          # not retired late
        assert np.allclose(rows[c].costs[:s_c + 1], costs[c, :s_c + 1], rtol=RTOL, atol=0), c
    # everything else, handed on or not, was rolled to the horizon and equals the unpruned launch
    kept = ~gone
    assert kept[0] and kept[int(np.argmin(ret))] and np.array_equal(got[kept], ret[kept]) and not fail[kept].any()
    for c in np.nonzero(kept)[0]:
        assert np.array_equal(rows[c].costs, costs[c]), c
