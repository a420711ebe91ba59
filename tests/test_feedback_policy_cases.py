"""CPU tests of the feedback-policy harness (tests/feedback_policy_cases.py): the exact policy between the knots against
   the oracle (oracle/ilqg.c)                      Cartpole, Particle, the A1, tests/models/capsules_tendon.xml; held to a QUARTER of the bound
   the quad kernel's feedback_ctrl                 mujoco_mpc_amd/csrc/quad_step.h through its lock-step emulator (tests/quademu), the A1 cases,
                                                   at the full bound; no candidate handed on
   the Python ILQGPolicy.action                    mujoco_mpc_amd/planners.py, at the oracle's (state, time) pairs
and the conditions on the cases themselves: the caps on the bounds (fp64 1e-10, fp32 2e-3), the census of interior / clamped / ambiguous
entries and of the interpolation regimes, on the oracle's outputs by the reference alone. The worst error / bound of each is printed.
The -m gpu suite (tests/test_gpu_feedback_policy.py) runs the same cases and the same checker on the device kernels."""
import numpy as np
import pytest

import feedback_policy_cases as fpc
from mujoco_mpc_amd.planners import ILQGPolicy

_ORACLE = {}


def oracle(case):
    if case.name not in _ORACLE:
        _ORACLE[case.name] = fpc.run_oracle(case)
    return _ORACLE[case.name]


def test_the_reference_on_textbook_answers():
    """the restated functions on answers known without them"""
    m = fpc.mpf
    xs = [m(0), m(1), m(3)]
    assert [fpc.find_interval(xs, m(v), 3) for v in (-1, 0, 0.5, 1, 2, 3, 4)] == [(0, 0), (0, 1), (0, 1), (1, 2), (1, 2), (2, 2), (2, 2)]
    ys = [[m(1)], [m(3)], [m(-1)]]
    assert fpc.linear_interpolation(m(0.25), xs, ys, 3) == [m(1.5)] and fpc.zero_interpolation(m(2.5), xs, ys, 3) == [m(3)]
    # a cubic Hermite interpolant reproduces a straight line exactly where both slopes are the secants: the first interval of a 3-grid of a line
    line = [[m(2) * x + 1] for x in xs]
    assert abs(fpc.cubic_interpolation(m(0.4), xs, line, 3)[0] - m(1.8)) < m(10) ** -35
    assert fpc.finite_difference_slope(xs[1], xs, ys, 3, 0) == m(0.5) * (m(-4) / 2) + m(0.5) * 2   # the mean of the two secants
    assert fpc.finite_difference_slope(xs[1], xs[:2], ys[:2], 2, 0) == 0 and fpc.finite_difference_slope(xs[0], xs[:2], ys[:2], 2, 0) == 2
    assert fpc.finite_difference_slope(xs[2], xs, ys, 3, 0) == -2                                     # one-sided at the end of a 3-grid
    # a rotation of 3.3 rad about z comes back as 3.3 - 2 pi; the negated quaternion is the same rotation
    q = [fpc.M.cos(m(3.3) / 2), m(0), m(0), fpc.M.sin(m(3.3) / 2)]
    r = fpc.sub_quat(q, [m(1), m(0), m(0), m(0)])
    assert r[0] == 0 and abs(r[2] - (m(3.3) - 2 * fpc.M.pi)) < m(10) ** -35
    r = fpc.sub_quat([-v for v in q], [m(1), m(0), m(0), m(0)])
    assert abs(r[2] - (m(3.3) - 2 * fpc.M.pi)) < m(10) ** -35
    assert fpc.sub_quat([m(1), m(0), m(0), m(0)], [m(1), m(0), m(0), m(0)]) == [0, 0, 0]                # the zero-rotation guard


@pytest.mark.parametrize("model", ["cartpole", "particle", "a1", "scene"])
def test_the_oracle_follows_the_exact_policy(model):
    total = fpc.Census()
    for case in fpc.family(model):
        ref = oracle(case)
        total.add(fpc.check(case, 64, ref["states"], ref["actions"], ref["times"], scale=0.25))
    print(f"oracle {model}: worst error / bound {0.25 * total.worst:.3f} ({total.where}); largest bound {total.worst_bound:.2e}; {total}")
    assert 0.25 * total.worst <= 0.25
    total.assert_shares(model)


@pytest.mark.parametrize("model", ["cartpole", "particle"])
def test_the_fp32_cases_keep_their_caps_and_census(model):
    """the reference alone, on the float roundings of the oracle's (state, time) pairs: every fp32 bound within 2e-3, the census kept"""
    total = fpc.Census()
    for case in fpc.family(model):
        ref = oracle(case)
        total.add(fpc.check(case, 32, fpc.rounded(ref["states"], 32), None, fpc.rounded(ref["times"], 32)))
    print(f"fp32 {model}: largest bound {total.worst_bound:.2e}; {total}")
    total.assert_shares(model)


def test_the_other_gpu_cases_on_the_oracle():
    """the Humanoid's two cases and the batched pairs: the oracle follows them too, the caps hold"""
    total = fpc.Census()
    for case in fpc.humanoid_cases() + [c for m in ("cartpole", "particle", "a1", "scene") for c in fpc.batched_pair(m)]:
        ref = oracle(case)
        total.add(fpc.check(case, 64, ref["states"], ref["actions"], ref["times"], scale=0.25))
    print(f"oracle, humanoid and batched pairs: worst error / bound {0.25 * total.worst:.3f}; largest bound {total.worst_bound:.2e}")


def test_the_quad_form_follows_the_exact_policy():
    """quad_step.h feedback_ctrl on the CPU: the first proof for the quad copy. No candidate of any A1 case is handed on: the numbers are
    the quad form's, and the failure flag carries no fallback bit."""
    from mujoco_mpc_amd import capi  # noqa: F401  (the emulator binds the package's structs)
    from tests import quademu
    pm, pt = fpc.packed("a1")
    total = fpc.Census()
    for case in fpc.family("a1") + fpc.batched_pair("a1"):
        emu = quademu.rollout_feedback(pm, pt, case.start, case.t0, case.mocap, len(case.alpha), case.H, case.mode, case.representation,
                                       case.use_state, *case.policy_args())
        assert not emu["flags"].any() and not (emu["failure"] & 0x40000000).any() and not emu["failure"].any(), (case.name, emu["flags"])
        total.add(fpc.check(case, 64, emu["states"], emu["actions"], emu["times"]))
    print(f"quad emulator: worst error / bound {total.worst:.3f} ({total.where}); {total}")
    assert total.worst <= 1.0
    total.assert_shares("a1 on the quad emulator")


@pytest.mark.parametrize("model", ["cartpole", "particle", "a1"])
def test_the_python_policy_follows_the_exact_policy(model):
    """ILQGPolicy.action at the oracle's (state, time) pairs, every mode-1 case"""
    task, _, _ = fpc.setup(model)
    total = fpc.Census()
    for case in fpc.family(model):
        if case.mode != 1:
            continue
        ref = oracle(case)
        Tn = len(case.times)
        pol = ILQGPolicy(task.model, task, horizon_cap=Tn)
        tr = pol.trajectory
        tr.horizon = Tn
        tr.times[:], tr.states[:], tr.actions[:] = case.times, case.states, case.actions
        pol.feedback_gain[:], pol.representation = case.gains, case.representation
        N, H = ref["times"].shape
        got = np.zeros((N, H, case.joints.nu))
        for c in range(N):
            pol.feedback_scaling = float(case.alpha[c])
            for t in range(H - 1):
                pol.action(got[c, t], ref["states"][c, t] if case.use_state else None, ref["times"][c, t])
            got[c, H - 1] = got[c, H - 2]
        total.add(fpc.check(case, 64, ref["states"], got, ref["times"]))
    print(f"ILQGPolicy.action {model}: worst error / bound {total.worst:.3f} ({total.where})")
    assert total.worst <= 1.0
