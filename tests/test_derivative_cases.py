"""CPU checks of tests/derivative_cases.py: its references against each other and against the oracle, and the census of its cases.
No GPU: what the -m gpu tests of tests/test_gpu_model_derivatives.py and tests/test_gpu_gradient_exact.py hold the kernels to, the oracle
(and tests/gradient_reference.py) must meet first."""
import numpy as np
import pytest

import derivative_cases as dc
from gradient_reference import gradient_pass, spline_mapping
from mujoco_mpc_amd.planners import derivative_steps
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle


# ------------------------------------------------------------------------------------------------ A1
@pytest.mark.parametrize("centered", [0, 1])
def test_oracle_particle_quotient_against_the_closed_form(centered):
    task = load_task("Particle")
    pm, pt = task.packed_model(differentiable=True), task.packed()
    assert pm.struct.timestep == 0.1                                   # the packed step is the agent's, not the XML's 0.01
    eps = 2.0 ** -20
    states, actions = dc.particle_steps(eps)
    ref, census = dc.particle_reference(dc.ParticleModel.of(pm), states, actions, eps, centered)
    census.require(*(r for r in dc.PARTICLE_REGIMES if centered or r != "lone_side_centred"))
    A, B, C, D = pyoracle.transition_fd(pm, pt, states, np.zeros(len(states)), actions, eps, centered, mocap=dc.PARTICLE_GOAL)
    assert np.all(np.abs(A - ref["A"]) <= ref["bound_A"] + dc.U64 * np.abs(ref["A"]))
    assert np.all(np.abs(B - ref["B"]) <= ref["bound_B"] + dc.U64 * np.abs(ref["B"]))
    assert max(np.abs(A - ref["A"]).max(), np.abs(B - ref["B"]).max()) < 1e-10          # measured: 5.8e-11
    assert np.array_equal(C, ref["C"]) and np.array_equal(C[0], np.eye(4)) and not D.any() and not ref["D"].any()
    assert not B[3, :, 0].any() and not B[4, :, 1].any()
    # the closed form of the issue, not only its quotient: B = (h^2, h) g / (m + h d) on the limit as inside
    m = dc.ParticleModel.of(pm)
    want = float(m.h * m.gear[0] / (m.mass + m.h * m.damping[0]))
    assert abs(ref["B"][1, 2, 0] - want) < 1e-15 and abs(ref["B"][1, 0, 0] - float(m.h) * want) < 1e-15 and ref["B"][0, 2, 0] == ref["B"][1, 2, 0]


# ------------------------------------------------------------------------------------------------ A2
@pytest.mark.parametrize("centered", [0, 1])
@pytest.mark.parametrize("eps", dc.FREE_BODY_EPS)
def test_oracle_free_body_quotient_against_mpmath(eps, centered):
    task = dc.free_body_task()
    pm, pt = task.packed_model(differentiable=True), task.packed()
    states = dc.free_body_states()
    assert tuple(states) == dc.FREE_BODY_REGIMES
    assert states["negative_w"][3] < 0 and np.array_equal(states["negative_w"][3:7], -states["large_rotation"][3:7])
    assert 2 * np.arccos(states["wrap_beyond_pi"][3]) > np.pi
    X = np.array(list(states.values()))
    A, B, _, _ = pyoracle.transition_fd(pm, pt, X, np.zeros(len(X)), np.full((len(X), 1), dc.FREE_BODY_ACTION), eps, centered)
    ref = dc.free_body_reference(pm, eps, centered)
    blk, arm = dc.FREE_BODY_BLOCK, dc.FREE_BODY_ARM
    for t, name in enumerate(states):
        want, z0 = ref[name]
        err = np.abs(A[t][np.ix_(blk, blk)] - want)
        assert np.all(err <= dc.free_body_bound(name, eps, centered, z0, 8)), (name, float(err.max()))
        assert not A[t][np.ix_(blk, arm)].any() and not A[t][np.ix_(arm, blk)].any() and not B[t][blk].any()
    # the quotient is a rotation's: the orientation block is far from the identity at these states and eps
    assert np.abs(ref["large_rotation"][0][3:6, 3:6] - np.eye(3)).max() > 1e-3


def test_free_body_step_is_the_closed_form():
    """the oracle's step of the free body against the mpmath step: the model is what the harness says it is"""
    task = dc.free_body_task()
    pm, pt = task.packed_model(differentiable=True), task.packed()
    fb = dc.FreeBody.of(pm)
    for name, x in dc.free_body_states().items():
        r = pyoracle.rollout_batch(pm, pt, x, 0.0, None, 1, 2, 1, 0, np.zeros(1), np.full((1, 1, 1), dc.FREE_BODY_ACTION))
        y = r["states"][0, 1]
        want = np.array([float(v) for v in fb.step([dc.mpf(float(v)) for v in np.concatenate([x[0:7], x[8:14]])])])
        got = np.concatenate([y[0:7], y[8:14]])
        assert np.abs(got - want).max() <= 16 * dc.U64 * (1 + np.abs(want).max()), (name, np.abs(got - want).max())


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("key", dc.LIN_KEYS)
def test_oracle_linearisation_predicts_its_step(key):
    case = dc.linearisation_case(key)
    errs, _, (y0, r0) = dc.oracle_linearisation(case)
    world = dc.oracle_linearisation(case, "world")[0]["A"] if case.rotated else None
    dc.check_linearisation(case, errs, world, y0, r0)
    assert np.all(np.abs(case.perturbed_actions()) < 1)                     # the perturbed controls stay inside the limits
    assert np.all(case.directions != 0) and np.all(case.control_directions != 0)


def test_linearisation_regimes():
    import step_bank
    census = dc.Census()
    for key in dc.LIN_KEYS:
        case = dc.linearisation_case(key)
        if case.layout.has_quaternion():
            f = step_bank.state_features(case.task, case.state, case.time, case.mocap)
            assert ("floor" in f) == case.contacts, (key, f)
            angle = 2 * np.arccos(abs(case.state[3]))
            assert angle > 0.8
            census["rotated_base"] += 1
            census["rotated_base_with_contacts" if case.contacts else "airborne"] += 1
        else:
            census["lane_family"] += 1
    census.require(*dc.LIN_REGIMES)
    assert census["rotated_base"] == 3 and census["rotated_base_with_contacts"] == 1 and census["airborne"] == 2


# ------------------------------------------------------------------------------------------------ C
def test_gradient_regimes_are_all_visited():
    census = dc.Census()
    for n, m in dc.GRADIENT_SHAPES:
        for T in dc.GRADIENT_T:
            for _, _, nodes, steps in dc.gradient_cases(T):
                census += dc.gradient_census(n, m, T, nodes, steps)
    census.require(*dc.GRADIENT_REGIMES)


def test_spline_mapping_agrees_with_the_exact_weights():
    """tests/gradient_reference.py's transcription of spline_mapping.cc against the exact linear form of TimeSpline::Sample"""
    worst = 0.0
    for T in dc.GRADIENT_T:
        for _, rep, nodes, steps in dc.gradient_cases(T):
            M = spline_mapping(rep, nodes, steps[:T - 1])
            W = dc.step_weights(nodes, steps, rep)
            for t in range(T - 1):
                exact, mag = np.zeros(len(nodes)), np.zeros(len(nodes))
                for p, (w, a) in W[t].items():
                    exact[p], mag[p] = float(w), max(float(a), abs(float(w)))
                err = np.abs(M[t] - exact)
                assert np.all(err <= dc.gamma(dc.WEIGHT_ROUNDINGS[rep] + 2) * mag), (T, rep, t, err.max())
                worst = max(worst, float(err.max()))
    assert worst < 1e-15            # measured: 3.3e-16


@pytest.mark.parametrize("shape", dc.GRADIENT_SHAPES, ids=lambda s: f"n{s[0]}m{s[1]}")
def test_numpy_restatement_meets_the_exact_bound(shape):
    n, m = shape
    for T in (3, 65):
        args, sweep = dc.gradient_sweep_case(n, m, T)
        for _, rep, nodes, steps in dc.gradient_cases(T):
            dc.check_gradient_pass(gradient_pass(*args, rep, nodes, steps), sweep, nodes, steps, rep)


def test_exact_sweep_on_a_case_done_by_hand():
    """n = m = 1, T = 3: Vx = cx2 a1 a0 + cx1 a0 + cx0, k1 = -(b1 cx2 + cu1), k0 = -(b0 (a1 cx2 + cx1) + cu0)"""
    A = np.array([0.5, -0.25, 9.0]).reshape(3, 1, 1)
    B = np.array([2.0, -1.5, 9.0]).reshape(3, 1, 1)
    cx, cu = np.array([[1.0], [-2.0], [0.75]]), np.array([[0.5], [0.25], [9.0]])
    sw = dc.exact_sweep(A, B, cx, cu)
    v1 = -0.25 * 0.75 - 2.0
    assert sw.Vx[:, 0].tolist() == [0.5 * v1 + 1.0, v1, 0.75]
    assert sw.k[:, 0].tolist() == [-(2.0 * v1 + 0.5), -(-1.5 * 0.75 + 0.25), -(-1.5 * 0.75 + 0.25)]
    assert sw.dV0 == -(sw.k[0, 0] ** 2 + sw.k[1, 0] ** 2)


# ------------------------------------------------------------------------------------------------ D
def test_evaluate_list_matches_derivative_steps():
    for T in range(1, 41):
        for skip in range(7):
            assert list(derivative_steps(T, skip)) == dc.evaluate_list(T, skip), (T, skip)


def test_interpolation_regimes():
    census = dc.Census()
    X = np.arange(5.0)[:, None]
    for ev in dc.INTERPOLATION_LISTS:
        ev = dc.evaluate_list(12, 3) if ev is None else ev
        for t in range(12):
            dc.interpolate_step(ev, X[:len(ev)], t, 12, census)
    census.require(*dc.INTERPOLATION_REGIMES)
    assert dc.interpolate_step([3, 7], X[:2], 1, 12)[0] == 0.0 and dc.interpolate_step([3, 7], X[:2], 9, 12)[0] == 1.0
    assert dc.interpolate_step([0, 4], X[:2], 1, 12)[0] == 0.0 * 0.75 + 1.0 * 0.25
