"""-m gpu: the constraint-free step of every rollout kernel against the independent 50-digit reference of tests/smooth_step_cases.py (the
method, the cases, the conditions and the bounds are there; tests/test_smooth_step_cases.py holds the reference to itself and the oracle
and both emulators to it on the CPU). One step is a rollout of horizon 2 with one zero-order node, N = 16: the sixteen controls of
step_bank.step_controls on each state. Kernel names, environment switches, precisions and bounds come from test_gpu_step_parity.ROWS
(smooth_step_cases.DEVICE_ROWS names the row); every row asserts the kernel it ran on, one context per row, closed in `finally`.

Full-step rows: |d - r| <= bound (1 + |r|) on the whole next state. The limb row runs with its fallback off and asserts that no candidate
carries LIMB_HANDED_ON. Friction-loss rows (the quad kernel takes no disable flag and the A1 always has friction loss): the momentum
balance rho = (M + h D)(v' - v) / h - (tau_act + passive - bias) of the device's v', zero on the trunk and within dof_frictionloss on
the joints, and q' against q (+) h v' of the device's own v' (smooth_step_cases.momentum_balance).

Worst share of the bound, measured on the MI355X (states x candidates compared):

    row                                              fp64              fp32
    rollout_limb_kernel, fallback off      6 x 16    4.0e-5            0.080
    rollout_tree_kernel<Humanoid>          6 x 16    3.1e-5            0.0020
    rollout_tree_kernel<A1>, flags         6 x 16    5.3e-6            2.9e-4
    rollout_wave_kernel, probe, Euler      3 x 16    1.6e-6            0.015
    rollout_wave_kernel, tree, Euler       3 x 16    2.7e-6            --
    rollout_wave_kernel, RK4, tree         3 x 16    1.1e-6            --
    rollout_wave_kernel, RK4, probe        2 x 4     4.7e-7            --
    rollout_wave_kernel, RK4, A1 (flags)   2 x 4     1.4e-6            --
    rollout_wave_kernel, RK4, Humanoid     2 x 4     1.7e-5            --
    rollout_lane, Cartpole                 6 x 16    1.0e-7            6.7e-4
    rollout_lane, Particle                 6 x 16    7.3e-8            5.3e-4
    rollout_quad_kernel, momentum balance  6 x 16    7.5e-7            --
    rollout_tree_kernel<A1>, momentum bal. 6 x 16    8.5e-7            --

The RK4 rows of the probe, the A1 and the Humanoid launch all sixteen controls on the fastest state and the next of the ranking and compare
four of them -- zero, both saturated ends, one past an end (smooth_step_cases.rk4_candidates): their 50-digit reference needs new
Jacobians for stages 3 and 4 of every candidate. The module adds 14 s to the -m gpu suite, the mpmath reference most of it (the
Humanoid's RK4 row 4 s)."""
import numpy as np
import pytest

import feedback_policy_cases as fpc
import smooth_step_cases as ss
import step_bank as sb
import test_gpu_step_parity as tpar

pytestmark = pytest.mark.gpu

def device_next(key, prow, integrator=None, states=None):
    """{case: [16, nq + nv]}: the state after one step of every case (of the cases `states`) of the model on the kernel of ROWS[prow]"""
    _, env, kernel, precision, _, _, _ = tpar.ROWS[prow]
    mdl = ss.model(key)
    pm = mdl.pm
    if integrator is not None:
        pm = mdl.task.packed_model()
        pm.struct.integrator, pm.struct.disableflags = integrator, mdl.pm.struct.disableflags
    ctx = tpar.context(pm, mdl.pt, precision, env)
    out = {}
    try:
        assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
        for i, c in enumerate(ss.cases(key)):
            if states is not None and i not in states:
                continue
            ctx.set_state(c.state, mdl.time, mdl.mocap)
            ctx.rollout_splines(2, 0, np.array([mdl.time]), c.controls)
            _, fail = ctx.returns()
            raw = np.asarray(ctx.failure_raw)
            assert not np.any(raw & sb.LIMB_HANDED_ON), (key, c.label, "a candidate was handed on")
            assert not np.any(fail), (key, c.label, fail)
            traj, _, _ = fpc.fetch_all(ctx)
            assert traj.shape[0] == len(c.controls) == sb.STEP_CANDIDATES
            out[i] = traj[:, 1].copy()
        assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("row", [r for r, v in ss.DEVICE_ROWS.items() if v[2] == "state"])
def test_the_step_obeys_mechanics(row):
    key, prow, _ = ss.DEVICE_ROWS[row]
    tol = tpar.ROWS[prow][4]
    got = device_next(key, prow)
    worst, where = 0.0, None
    for i, c in enumerate(ss.cases(key)):
        w, at = ss.share(got[i], ss.expect(key, i).next_state, tol)
        if w > worst:
            worst, where = w, (c.label, tuple(int(x) for x in at))
    print(f"{row}: {len(got)} states x {sb.STEP_CANDIDATES} candidates, worst share of the bound ({tol:.0e}) {worst:.3g} at {where}")
    assert worst <= 1.0, (row, worst, where)


@pytest.mark.parametrize("row", list(ss.RK4_DEVICE_ROWS))
def test_the_rk4_step_obeys_mechanics(row):
    key, prow = ss.RK4_DEVICE_ROWS[row]
    tol = tpar.ROWS[prow][4]
    assert tpar.ROWS[prow][5] == 1 and tpar.ROWS[prow][3] == 64
    got = device_next(key, prow, integrator=tpar.ROWS[prow][5], states=ss.rk4_states(key))
    worst, where, n = 0.0, None, 0
    for i in ss.rk4_states(key):
        cands, want = ss.rk4_expect(key, i)
        w, at = ss.share(got[i][cands], want, tol)
        n += len(cands)
        if w > worst:
            worst, where = w, (ss.cases(key)[i].label, tuple(int(x) for x in at))
    print(f"{row}: {len(got)} states, {n} candidates compared, worst share of the bound ({tol:.0e}) {worst:.3g} at {where}")
    assert worst <= 1.0, (row, worst, where)


@pytest.mark.parametrize("row", [r for r, v in ss.DEVICE_ROWS.items() if v[2] == "momentum"])
def test_the_step_with_friction_loss_keeps_the_momentum_balance(row):
    key, prow, _ = ss.DEVICE_ROWS[row]
    tol = tpar.ROWS[prow][4]
    got = device_next(key, prow)
    worst, n = 0.0, 0
    for i in range(len(ss.cases(key))):
        w, k = ss.momentum_balance(key, i, got[i], tol)
        worst, n = max(worst, w), n + k
    print(f"{row}: {len(got)} states x {sb.STEP_CANDIDATES} candidates, {n} entries, worst share of the allowance {worst:.3g}")
    assert worst <= 1.0, (row, worst)
