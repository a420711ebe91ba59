"""-m gpu: ModelDerivatives on the device against answers that are neither the kernel's nor the oracle's (tests/derivative_cases.py).

   A1  transition_fd_kernel + fd_assemble_kernel, Particle, fp64 and fp32: A, B <-> the difference quotient of the closed-form step in
       rational arithmetic, 4 x gamma_k (|y_c| + |y_0|) / eps; C == I and D == 0 exactly; the column of a control outside its range is
       exactly 0.0; on a limit, and within eps of one, the quotient is one-sided and divided by eps in either mode
   A2  transition_fd_wave_kernel + fd_tangent_kernel + fd_assemble_kernel on tests/models/free_body.xml (the generic kernel): the free
       body's 12 x 12 block of A <-> mj_integratePos, the closed-form step, mj_differentiatePos and mjd_transitionFD's quotient in mpmath,
       at a large rotation, with w < 0, beyond pi and at the identity; 8 x the oracle's measured error (floor 64 u (1 + |y|) / eps); the
       blocks coupling body and arm and the body's rows of B are exactly 0.0; the arm's block, B and D <-> the oracle, 2e-8 (1 + |x|)
   B   the linearisation predicts the kernel's own step: StateDiff(step(x (+) s d), step(x)) / s -> A d, with (+) and StateDiff written in
       the harness, on the A1 at rotated bases (one with its feet on the floor) and on the Cartpole; the error halves with s, stays
       below 4 K s (K the oracle's, a curvature of the physics), and the same quotient with a world-frame (+) misses by > 100 x that;
       A, B, C, D at these states <-> the oracle's, 5e-6 (1 + |x|)
   D   fd_interpolate_kernel through mjpcx_gradient_step_batched: evaluated steps carry the bits of mjpcx_transition_fd, every other step
       is x0 * (1.0 - w) + x1 * w bit for bit (the nearest evaluated step outside the list's range), step T - 1 of A and B is 0.0
The worst error / bound of each family is printed."""
import numpy as np
import pytest

import derivative_cases as dc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import derivative_steps
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ A1
@pytest.mark.parametrize("centered", [0, 1])
@pytest.mark.parametrize("precision,eps", [(64, 2.0 ** -20), (32, 2.0 ** -10)])
def test_particle_quotient_against_the_closed_form(precision, eps, centered):
    task = load_task("Particle")
    pm, pt = task.packed_model(differentiable=True), task.packed()
    ctx = capi.Context(pm, pt, 0, precision)
    assert ctx.kernel_name.startswith("rollout_lane<TopoParticle,TaskParticle")
    states, actions = dc.particle_steps(eps)
    ref, census = dc.particle_reference(dc.ParticleModel.of(pm, precision), states, actions, eps, centered, precision)
    census.require(*(r for r in dc.PARTICLE_REGIMES if centered or r != "lone_side_centred"))
    ctx.set_state(states[0], 0.0, dc.PARTICLE_GOAL)
    A, B, C, D = ctx.transition_fd(np.zeros(len(states)), states, actions, eps, centered)
    worst = 0.0
    for got, key in ((A, "A"), (B, "B")):
        err, tol = np.abs(got - ref[key]), ref["bound_" + key] + dc.U64 * np.abs(ref[key])
        worst = max(worst, float(np.max(err[tol > 0] / tol[tol > 0])))
        assert np.all(err <= tol), (key, float(err.max()), np.argwhere(err > tol)[:4].tolist())
    print(f"Particle fp{precision} eps 2^{int(np.log2(eps))} centered {centered}: worst error / bound {worst:.3e}, "
          f"worst error {max(np.abs(A - ref['A']).max(), np.abs(B - ref['B']).max()):.3e}")
    assert np.array_equal(C, ref["C"]) and np.array_equal(C[0], np.eye(4))
    assert not D.any() and not ref["D"].any()
    assert not B[3, :, 0].any() and not B[4, :, 1].any() and actions[3, 0] == 1.5 and actions[4, 1] == -1.5      # outside the range: exactly 0.0
    h2 = float(ref["B"][0, 0, 0])
    assert abs(B[1, 0, 0] - h2) <= ref["bound_B"][1, 0, 0] and h2 > 0.02                                          # on the limit: still h^2 g / (m + h d)
    ctx.close()


# ------------------------------------------------------------------------------------------------ A2
def close(a, b, tol):
    return np.all(np.abs(np.asarray(a) - b) <= tol * (1 + np.abs(b)))


@pytest.mark.parametrize("centered", [0, 1])
@pytest.mark.parametrize("eps", dc.FREE_BODY_EPS, ids=lambda e: f"eps2^{int(np.log2(e))}")
def test_free_body_quotient_against_mpmath(eps, centered):
    from oracle import pyoracle
    task = dc.free_body_task()
    pm, pt = task.packed_model(differentiable=True), task.packed()
    ctx = capi.Context(pm, pt, 0, 64)
    assert "rollout_wave_kernel" in ctx.kernel_name, ctx.kernel_name            # an unregistered model: the generic kernels
    states = dc.free_body_states()
    X, U = np.array(list(states.values())), np.full((len(states), 1), dc.FREE_BODY_ACTION)
    ctx.set_state(X[0], 0.0)
    A, B, C, D = ctx.transition_fd(np.zeros(len(X)), X, U, eps, centered)
    Ao, Bo, Co, Do = pyoracle.transition_fd(pm, pt, X, np.zeros(len(X)), U, eps, centered)
    ref = dc.free_body_reference(pm, eps, centered)
    blk, arm = dc.FREE_BODY_BLOCK, dc.FREE_BODY_ARM
    for t, name in enumerate(states):
        want, z0 = ref[name]
        err, bound = np.abs(A[t][np.ix_(blk, blk)] - want), dc.free_body_bound(name, eps, centered, z0, 8)
        print(f"free body {name} eps 2^{int(np.log2(eps))} centered {centered}: worst error {err.max():.3e}, error / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound), (name, float(err.max()), np.argwhere(err > bound)[:4].tolist())
        assert not A[t][np.ix_(blk, arm)].any() and not A[t][np.ix_(arm, blk)].any() and not B[t][blk].any()
        assert close(A[t][np.ix_(arm, arm)], Ao[t][np.ix_(arm, arm)], 2e-8) and close(B[t][arm], Bo[t][arm], 2e-8) and np.abs(B[t][arm]).max() > 0
    assert close(D, Do, 2e-8) and close(C, Co, 2e-8)
    ctx.close()


# ------------------------------------------------------------------------------------------------ B
LIN_KERNEL = {"a1_home_yawed": ("rollout_quad_kernel", "rollout_tree_kernel"), "a1_turned_in_the_air": ("rollout_quad_kernel", "rollout_tree_kernel"),
              "a1_trot_turned": ("rollout_quad_kernel", "rollout_tree_kernel"), "cartpole": ("rollout_lane",)}


@pytest.mark.parametrize("key", dc.LIN_KEYS)
def test_linearisation_predicts_the_step(key):
    from oracle import pyoracle
    case = dc.linearisation_case(key)
    pm = case.task.packed_model(differentiable=True)
    ctx = capi.Context(pm, case.packed_task, 0, 64)
    assert any(k in ctx.kernel_name for k in LIN_KERNEL[key]), ctx.kernel_name
    n, nu, S = 64, case.layout.nu, len(dc.LIN_S)
    xs = case.perturbed_states()
    if case.rotated:
        xs = np.concatenate([xs, case.perturbed_states("world")[1:]])
    E = len(xs)
    assert E == 1 + dc.LIN_DIRECTIONS * S * (2 if case.rotated else 1)
    us = case.perturbed_actions()
    nodes = np.tile(case.action, (E, n, 1, 1))
    nodes[0, :len(us), 0] = us                                                  # the unperturbed environment's candidates carry the control perturbations
    ctx.set_states(xs, np.full(E, case.time), None if case.mocap is None else np.tile(case.mocap, (E, 1)))
    ctx.rollout_splines_batched(2, capi.SPLINE_ZERO, np.full((E, 1), case.time), nodes, num_envs=E, n_per_env=n)
    _, fail = ctx.returns()
    assert not fail.any()
    by_env = [ctx.fetch_trajectory(e * n) for e in range(E)]
    by_ctrl = [ctx.fetch_trajectory(c) for c in range(len(us))]
    assert all(np.array_equal(tr.actions[0], u) for tr, u in zip(by_ctrl, us))
    ctx.set_state(case.state, case.time, case.mocap)
    A, B, C, D = (x[0] for x in ctx.transition_fd([case.time], case.state[None], case.action[None], dc.LIN_EPS, 1))
    m = 1 + dc.LIN_DIRECTIONS * S
    errs = dc.linearisation_errors(case, [tr.states[1] for tr in by_env[:m]], [tr.residual[0] for tr in by_env[:m]],
                                   [tr.states[1] for tr in by_ctrl], [tr.residual[0] for tr in by_ctrl], A, B, C, D)
    world = None
    if case.rotated:
        rows = [by_env[0]] + by_env[m:]
        world = dc.linearisation_errors(case, [tr.states[1] for tr in rows], [tr.residual[0] for tr in rows], None, None, A, B, C, D)["A"]
    for name in "ABCD":
        print(f"linearisation {key} {name}: err(s) per direction {[[float(f'{v:.2e}') for v in row] for row in errs[name]]}")
    worst = dc.check_linearisation(case, errs, world, by_env[0].states[1], by_env[0].residual[0])
    print(f"linearisation {key}: worst err / bound {worst:.3f}" + (f", world-frame miss {world[:, -1].min():.3f}" if case.rotated else ""))
    # the device's A, B, C, D at this state against the oracle's: the comparison tests/test_gpu_quadruped.py makes at the identity orientation
    ref = pyoracle.transition_fd(pm, case.packed_task, case.state[None], np.array([case.time]), case.action[None], dc.LIN_EPS, 1, mocap=case.mocap)
    for g, o in zip((A, B, C, D), ref):
        assert close(g, o[0], 5e-6), (key, float(np.abs(g - o[0]).max()))
    ctx.close()


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("centered", [0, 1])
def test_interpolation_edges(centered):
    task = load_task("Particle")
    ctx = capi.Context(task.packed_model(differentiable=True), task.packed(), 0, 64)
    E, N, H, T, eps = 2, 64, 12, 12, 1e-6
    states, times, mocap = dc.particle_fleet(E)
    ctx.set_states(states, times, mocap)
    rng = np.random.default_rng(11)
    roll_times = np.stack([t + np.linspace(0.0, (H - 1) * 0.1, 4) for t in times])
    ctx.rollout_splines_batched(H, capi.SPLINE_CUBIC, roll_times, np.clip(rng.normal(0, 0.4, (E, N, 4, 2)), -1, 1), num_envs=E, n_per_env=N)
    cand = 3
    trs = [ctx.fetch_trajectory(e * N + cand) for e in range(E)]
    assert not any(tr.failure for tr in trs)
    census = dc.Census()
    for ev in dc.INTERPOLATION_LISTS:
        ev = list(derivative_steps(T, 3)) if ev is None else ev
        got = ctx.gradient_step_batched(E, cand, T, ev, eps, centered, 1, roll_times, with_matrices=True)
        for e in range(E):
            ctx.set_state(states[e], times[e], mocap[e])
            A, B, _, _ = ctx.transition_fd(trs[e].times[ev], trs[e].states[ev], trs[e].actions[ev], eps, centered)
            assert np.abs(A).max() > 0 and np.abs(B).max() > 0
            for t in range(T):
                for name, X in (("A", A), ("B", B)):
                    want = dc.interpolate_step(ev, X, t, T, census)
                    assert np.array_equal(got[name][e, t], want), (ev, e, t, name, float(np.abs(got[name][e, t] - want).max()))
        # steps between two evaluated ones differ from both neighbours: the interpolation is observable
        if ev == [0, 11]:
            assert not np.array_equal(got["A"][0, 5], got["A"][0, 0])
    census.require(*dc.INTERPOLATION_REGIMES)
    ctx.close()
