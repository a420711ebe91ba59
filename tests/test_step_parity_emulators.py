"""CPU twin of tests/test_gpu_step_parity.py: the step-parity harness (tests/step_bank.py) on the lock-step emulators -- the limb kernel's step
function (tests/limbemu) over the Humanoid bank in float and double, the quad kernel's (tests/quademu) over the A1 bank in double. One
mj_step per bank state and candidate against the fp64 oracle, every Trajectory field element by element, |d - o| <= tol (1 + |o|):

    row                      bound   observed worst
    limb step, fp64          1e-9    5e-12
    limb step, fp32          3e-4    1.7e-4
    quad step, fp64          1e-9    6e-12

The float row's own bound: on the fastest states of the bank (|qacc| up to 2.6e3, cond(M) 4-5e3) the float qacc_smooth alone is off by
1-2e-4 of (1 + |qvel|) after one step, whatever the solver does; the Newton floors do not move it. The bound is 2x above that and 10x below
what float-only changes of the solver's stopping rule give (test_the_step_bound_sees_a_float_only_solver_change): the gradient floor
raised 10x reaches 1.0e-3, the former relative cost floor 4.1e-3 (a Walk keyframe at full control).

Time: about 25 s, of which three g++ builds of the emulator variants take most."""
import numpy as np
import pytest

import step_bank as sb
from tests import limbemu, quademu

TOL = {("limb", 64): 1e-9, ("limb", 32): 3e-4, ("quad", 64): 1e-9}


def emulator_step(mod, bank, **kw):
    t = bank.task
    pm = t.packed_model()

    def step(k, s, nodes):
        o = mod.rollout(pm, sb.packed_task(t, s), s.state, s.time, s.mocap, len(nodes), 2, 1, 0, np.array([s.time]), node_values=nodes, **kw)
        o["kept"] = o["flags"] == 0      # (a candidate the kernel's form does not cover is flagged: the device hands it on)
        return o
    return step


def report(name, bank, rep, tol):
    print(f"{name}: {len(bank.states)} states, {sum(rep.compared)} candidates compared, worst {rep.worst:.2e} (bound {tol:.0e}, "
          f"{rep.ratio:.2f} of it), census of the compared states {sb.covered_counts(bank, rep)}; worst at {rep.where}")


@pytest.mark.parametrize("precision", [64, 32])
def test_limb_step_function_against_the_oracle(precision):
    bank = sb.humanoid_bank()
    tol = TOL[("limb", precision)]
    rep = sb.run_bank(bank, emulator_step(limbemu, bank, precision=precision), tol)
    report(f"limb emulator fp{precision}", bank, rep, tol)
    assert not rep.failures, rep.failures[:4]
    # what the limb form covers of the hard paths: contacts between moving geoms (the Woodbury terms) and tendon-limit rows
    c = sb.covered_counts(bank, rep)
    assert c.get("moving", 0) >= 3 and c.get("tendon", 0) >= 3, c


def test_quad_step_function_against_the_oracle():
    bank = sb.a1_bank()
    tol = TOL[("quad", 64)]
    rep = sb.run_bank(bank, emulator_step(quademu, bank), tol)
    report("quad emulator fp64", bank, rep, tol)
    assert not rep.failures, rep.failures[:4]
    c = sb.covered_counts(bank, rep)
    assert c.get("leg_leg", 0) >= 3 and c.get("hip_cyl", 0) >= 3, c
    assert len({s.residual_int[0] for s in bank.states}) == 5     # every residual mode of the QuadrupedFlat task


@pytest.mark.parametrize("name,flags", [("gfloor", ["-DLEXP_GFLOOR=160"]),                       # the gradient floor raised 10x: 1.0e-3
                                        ("cfloor", ["-DLEXP_GFLOOR=16", "-DLEXP_CFLOOR=8"]),    # the former relative cost floor: 4.1e-3
                                        ("floors", ["-DLEXP_GFLOOR=160", "-DLEXP_CFLOOR=80"])])  # both, 10x: 4.1e-3
def test_the_step_bound_sees_a_float_only_solver_change(name, flags):
    """the limb step function built with other Newton floors -- a change that only acts in float: in double both floors lie far below the
    tolerance -- must miss the fp32 step bound, and still pass the fp64 one"""
    limbemu.register_variant(name, flags)
    bank = sb.humanoid_bank()
    rep32 = sb.run_bank(bank, emulator_step(limbemu, bank, precision=32, variant=name), TOL[("limb", 32)])
    report(f"limb emulator fp32, {' '.join(flags)}", bank, rep32, TOL[("limb", 32)])
    assert rep32.failures
    rep64 = sb.run_bank(bank, emulator_step(limbemu, bank, precision=64, variant=name), TOL[("limb", 64)])
    assert not rep64.failures, rep64.failures[:4]
