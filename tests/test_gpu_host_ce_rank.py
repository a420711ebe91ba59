"""-m gpu: the C++ mjpc::GpuCrossEntropyPlanner's pruning switch through HostPlanner(kind="cross_entropy"): the plan launch at rank
n_elite + 1 (mjpcx_set_prune_rank), parked on the previous plan's worst elite return x (1 + slack). QuadrupedFlat, 255 candidates + the
nominal, H = 30, n_elite = 12, five plans with the state advanced along the nominal trajectory between them: policy, variance, elites and
improvement equal the unpruned planner's, the first plan runs without a hint, the later ones with one. The slack is also lowered to -0.3
(hint = 0.7 x the previous worst elite: below what the launch will find) so that the resume path is taken for certain."""
import os

import numpy as np
import pytest

from mujoco_mpc_amd.hostplanner import HostPlanner
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
H, N, N_ELITE, PLANS = 30, 255, 12, 5


def run(task, pruning, slack):
    os.environ["MJPCX_QUAD_MIN_N"] = "1"
    try:
        pl = HostPlanner(task, device=0, precision=64, seed=0, num_trajectory=N, kind="cross_entropy")
    finally:
        os.environ.pop("MJPCX_QUAD_MIN_N", None)
    assert "rollout_quad_kernel" in pl.kernel_name
    pl.ce_set(n_elite=N_ELITE)
    assert pl.prune_info() == dict(parked=0, settled_retired=0, resumed=0, hint=0.0, retired=0, repeated=False)   # off by default
    if pruning:
        pl.prune_set(True, slack)
    pl.task_transition(0.0)
    home = task.model.keyframes["home"]
    pl.reset(H)
    nq, nv = task.model.nq, task.model.nv
    qpos, qvel, time = np.array(home["qpos"], float), np.zeros(nv), 0.0
    log = []
    for step in range(PLANS):
        pl.set_state(qpos, qvel, time)
        pl.optimize_policy(H)
        times, values = pl.policy()
        best = pl.best_trajectory(cap=512)
        log.append(dict(times=times, values=values, variance=pl.ce_variance(len(times) * task.model.nu), elites=np.asarray(pl.ce_elites()),
                        improvement=pl.improvement, info=pl.prune_info(),
                        best={k: np.asarray(best[k]).copy() for k in ("states", "actions", "times", "costs")}))
        s = np.asarray(best["states"])[1]
        qpos, qvel, time = s[:nq].copy(), s[nq:nq + nv].copy(), float(np.asarray(best["times"])[1])
    pl.close()
    return log


@pytest.fixture(scope="module")
def task():
    return load_task("QuadrupedFlat")


@pytest.fixture(scope="module")
def unpruned(task):
    return run(task, False, 0.05)


@pytest.mark.parametrize("slack", [0.05, -0.3])
def test_the_planner_computes_the_same_policy_with_and_without_pruning(task, unpruned, slack):
    pruned = run(task, True, slack)
    for step, (a, b) in enumerate(zip(unpruned, pruned)):
        for k in ("times", "values", "variance", "elites"):
            assert np.array_equal(a[k], b[k]), (step, k)
        assert a["improvement"] == b["improvement"], step
        for k, v in a["best"].items():
            assert np.array_equal(v, b["best"][k]), (step, k)
        assert a["info"]["parked"] == 0 and a["info"]["retired"] == 0 and not np.isfinite(a["info"]["hint"]) and not b["info"]["repeated"]
        if step < 2:   # the first plan has no previous elites, the second has (later ones may follow a stale plan, which leaves no hint)
            assert np.isfinite(b["info"]["hint"]) == (step == 1), step
        assert b["info"]["parked"] == b["info"]["settled_retired"] + b["info"]["resumed"]
    assert len({tuple(a["values"].ravel()) for a in unpruned}) == PLANS   # the plans differ: the comparison is not of one plan with itself
    if slack < 0:   # a hint below the best return parks every candidate and fewer than K complete: everything is resumed
        assert pruned[1]["info"]["parked"] > 0 and pruned[1]["info"]["resumed"] == pruned[1]["info"]["parked"]
