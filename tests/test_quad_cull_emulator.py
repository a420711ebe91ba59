"""CPU tests of the quad kernel's contact SEARCH (mujoco_mpc_amd/csrc/quad_step.h: static_pretest and the wavefront ballot in front of
collide_geom, the one geom body for leg and trunk geoms, the leg-level cull in front of pair_contacts_tests) through the lock-step emulator
(tests/quademu) against the oracle. A cull may only skip work that creates no contact; a pair culled wrongly is a missing contact force, an
O(1) error in the step from the first touching state on. So: one mj_step against the oracle, every Trajectory field, |d - o| <= 1e-9 (1 + |o|)
as the neighbouring emulator tests (tests/test_step_parity_emulators.py),

  * from every state of the A1 bank (tests/step_bank.py: trots, falls, tumbles, tangled legs, random states), and
  * along six sweeps of 41 states each across the ONSET of one contact: one leg's joints, or the trunk's height, move linearly from a state
    in which the pair is clear to one in which it touches (trunk 0.45 m up for the leg-leg sweeps, so nothing else interferes).

Non-vacuity comes from the oracle's own contact lists (the census below, and step_bank.contact_census for the leg-leg and hip-cylinder kinds):
every sweep has states without its contact and states with it, and the states checked hold a leg-leg, a trunk-leg, an own-hip and a
trunk-on-floor contact at least once.

The trunk-leg kind needs a note. On the A1 of the task no leg geom can reach the trunk's two pair geoms (the capsules at its front): over
300 000 joint samples of a front leg, up to 0.19 rad past the joint ranges, the oracle lists no such contact, and the nearest approach is
2 cm (a foot, at two joint limits). The step bank therefore has no trunk-leg state, and the sweep "calf on a trunk pair geom" runs on the A1
with the thinner of the two capsules lengthened from 6 to 11 cm half length -- quad_build accepts the model, the oracle steps the same
model -- where a front calf reaches it inside the joint ranges. Its touching states are the trunk-leg states of the census. Likewise a
foot reaches its own hip cylinder only with the knee past its (soft) limit: the bank's two such states lie outside the joint box the kernel
serves and are handed on, so a sixth sweep takes a knee up to 0.19 rad past the limit, inside that box."""
import functools

import numpy as np
import pytest

import step_bank as sb
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle
from tests import quademu

TOL = 1e-9
POINTS = 41
MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
HOME_LEGS = [-0.0003, 0.0182, -0.0268, 0.0016, 0.0248, -0.027, 0.0019, -0.033, -0.0675, -0.002, -0.0375, -0.0682]
TRUNK_CAPSULE, LONG_HALF = 9, 0.11      # the trunk's thin pair capsule (model geom id) and its half length in the variant model


def _q(z, quat, legs):
    return np.array([0.0, 0.0, z] + list(quat) + list(legs))


def _legs(**over):
    """the home joint values with legs replaced: _legs(l0=[...], l3=[...])"""
    v = list(HOME_LEGS)
    for k, val in over.items():
        v[3 * int(k[1]):3 * int(k[1]) + 3] = val
    return v


UP, FLIPPED = (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0)
# name: (first state, last state, the contact kind whose onset lies between them, model variant). Found on the CPU with the oracle alone
# (random joint samples until the kind shows up, then the 30 % of the way around its first touching state).
SWEEPS = {
    "calf_on_the_neighbouring_calf": (_q(0.45, UP, _legs(l0=[0.389, 0.835, 0.563], l3=[0.0672, -0.8639, 0.1368])),
                                      _q(0.45, UP, _legs(l0=[0.389, 0.835, 0.563], l3=[0.099, -1.2438, 0.2311])), "calf-calf:other", False),
    "foot_on_another_legs_hip_cylinder": (_q(0.45, UP, _legs(l1=[-0.0805, 0.8856, 0.5818], l2=[0.721, 0.462, 0.452])),
                                          _q(0.45, UP, _legs(l1=[-0.117, 1.2681, 0.8524], l2=[0.721, 0.462, 0.452])), "foot-hip:other", False),
    "calf_on_a_trunk_pair_geom": (_q(0.45, UP, _legs(l1=[-0.3466, -1.0825, -0.7241])),
                                  _q(0.45, UP, _legs(l1=[-0.427, -1.338, -0.885])), "calf-trunk", True),
    "foot_on_its_own_hip_cylinder": (_q(0.45, UP, _legs(l1=[0.7302, 2.5695, -0.9756])),      # (the knee up to 0.19 rad past its soft limit: inside the
                                     _q(0.45, UP, _legs(l1=[0.8124, 2.8568, -1.0827])), "foot-hip:own", False),  # joint box the kernel serves)
    "trunk_box_on_the_floor": (_q(0.056, FLIPPED, _legs()), _q(0.04, FLIPPED, _legs()), "floor-trunk:box", False),
    "a_thigh_reaching_the_floor": (_q(0.2144, UP, [-0.6653, -0.7073, 0.5299, 0.1319, -1.4543, -0.1255, -0.0336, -1.1108, 0.4112, -0.6203, 0.1013, 0.0234]),
                                   _q(0.1824, UP, [-0.6653, -0.7073, 0.5299, 0.1319, -1.4543, -0.1255, -0.0336, -1.1108, 0.4112, -0.6203, 0.1013, 0.0234]),
                                   "floor-thigh", False),
}


@functools.lru_cache(maxsize=None)
def _task():
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    return t


@functools.lru_cache(maxsize=None)
def _model(variant):
    """the task's planning model, or the variant with the long trunk capsule (module docstring); kept alive for the session"""
    t = _task()
    pm = t.packed_model()
    if variant:
        size = np.ctypeslib.as_array(pm.struct.geom_size, (t.model.ngeom * 3,)).reshape(-1, 3)
        size[TRUNK_CAPSULE, 1] = LONG_HALF
        assert quademu.check(pm, t.packed()) == ""
    return pm


@functools.lru_cache(maxsize=None)
def _census(variant):
    """state -> the kinds of contact in the oracle's contact list: '<part>-<part>' of floor | trunk | hip | thigh | calf | foot (sorted), ':own' /
    ':other' if both geoms are on legs (the same one / two), ':box' if one of them is a box"""
    t = _task()
    m = t.model
    a = m.arrays
    parent, gb, gt = a["body_parentid"], a["geom_bodyid"], a["geom_type"]
    trunk = next(b for b in range(m.nbody) if a["body_dofnum"][b] == 6)
    legs = sb._legs(t)
    static = [int(b) == 0 or a["body_mocapid"][int(b)] >= 0 for b in gb]
    ph = pyoracle.Physics(_model(variant))

    def part(g):
        if static[g]:
            return "floor"
        b = int(gb[g])
        if b == trunk:
            return "trunk"
        if gt[g] == 2:      # MJPCX_GEOM_SPHERE: the feet
            return "foot"
        depth = 0
        while parent[b] != trunk:
            b, depth = int(parent[b]), depth + 1
        return ("hip", "thigh", "calf")[depth]

    def kinds(state, time, mocap):
        ph.set_state(state[:m.nq], state[m.nq:], float(time), mocap)
        ph.forward()
        out = set()
        for r in ph.get("contact").reshape(-1, 11)[:int(ph.get("ncon")[0])]:
            g1, g2 = int(r[7]), int(r[8])
            k = "-".join(sorted([part(g1), part(g2)]))
            if legs[g1] >= 0 and legs[g2] >= 0:
                k += ":own" if legs[g1] == legs[g2] else ":other"
            if 6 in (gt[g1], gt[g2]):   # MJPCX_GEOM_BOX
                k += ":box"
            out.add(k)
        return out
    return kinds


def _sweep_states(name):
    q0, q1, kind, variant = SWEEPS[name]
    v = 0.2 * np.random.default_rng(sorted(SWEEPS).index(name)).normal(size=18)   # (moving: the contact rows' velocity terms take part)
    return [sb.BankState(f"{name}/{i}", np.concatenate([q0 + s * (q1 - q0), v]), 0.0, MOCAP, *sb._a1_residual(_task(), 0, 2, 0.0))
            for i, s in enumerate(np.linspace(0.0, 1.0, POINTS))]


def _step_all(states, variant, ncand=4):
    """one step of every state, ncand candidates each (zero control, both saturated ends, one random), emulator against oracle -> StepReport"""
    t = _task()
    pm = _model(variant)
    bank = sb.Bank("cull", t, states)

    def step(k, s, nodes):
        o = quademu.rollout(pm, sb.packed_task(t, s), s.state, s.time, s.mocap, len(nodes), 2, 1, 0, np.array([s.time]), node_values=nodes)
        o["kept"] = o["flags"] == 0
        return o
    rep = sb.StepReport()
    for k, s in enumerate(states):
        nodes = sb.controls_for(t, k)[:ncand]
        ref = sb.oracle_step(pm, t, s, nodes)
        got = step(k, s, nodes)
        cands = np.flatnonzero(got["kept"])
        rep.compared.append(len(cands))
        if not len(cands) or ref["failure"].any():
            rep.per_state.append(np.nan)
            continue
        worst, where, ok = sb.compare_step(s.label, got, ref, TOL, cands)
        rep.per_state.append(worst)
        if worst > rep.worst:
            rep.worst, rep.where = worst, where
        if not ok:
            rep.failures.append((worst / TOL, where))
    return bank, rep


@functools.lru_cache(maxsize=None)
def _sweep_result(name):
    """(per state: whether the oracle lists the sweep's contact, per state: the kinds, the step report): computed once, shared by the tests"""
    kind, variant = SWEEPS[name][2], SWEEPS[name][3]
    states = _sweep_states(name)
    kinds = [_census(variant)(s.state, s.time, s.mocap) for s in states]
    _, rep = _step_all(states, variant)
    return [kind in k for k in kinds], kinds, rep


@functools.lru_cache(maxsize=None)
def _bank_result():
    bank = sb.a1_bank()
    kinds = [_census(False)(s.state, s.time, s.mocap) for s in bank.states]
    _, rep = _step_all(bank.states, False, ncand=sb.STEP_CANDIDATES)
    return bank, kinds, rep


def test_one_step_from_every_state_of_the_a1_bank():
    bank, kinds, rep = _bank_result()
    print(f"A1 bank: {len(bank.states)} states, {sum(rep.compared)} candidates compared, worst {rep.worst:.2e} at {rep.where}")
    assert not rep.failures, rep.failures[:4]
    # the entries that matter to the culls were compared, not handed on
    for label in ("tangled", "falling", "tumbling"):
        assert sum(n for s, n in zip(bank.states, rep.compared) if s.label.startswith(label)) > 0, label


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_sweep_across_contact_onset(name):
    touching, kinds, rep = _sweep_result(name)
    first = touching.index(True) if True in touching else -1
    print(f"{name}: first touching state {first} of {POINTS}, kinds along the sweep {sorted(set().union(*kinds))}, {sum(rep.compared)} candidates "
          f"compared, worst {rep.worst:.2e} at {rep.where}")
    # non-vacuous by the oracle alone: clear at the start, touching further on, and both sides of the onset are compared
    assert not touching[0] and 0 < sum(touching) < POINTS, touching
    assert all(n > 0 for n in rep.compared[max(first - 2, 0):first + 3]), rep.compared
    assert sum(n > 0 for n in rep.compared) >= POINTS - 4, rep.compared
    assert not rep.failures, rep.failures[:4]


def test_the_states_checked_hold_every_kind_of_contact_the_culls_decide_on():
    """leg-leg, trunk-leg, own-hip and trunk-on-floor, each in at least one state that was compared (not handed on); the bank's own leg-leg and
    hip-cylinder states as step_bank.contact_census sees them"""
    bank, kinds, rep = _bank_result()
    t = _task()
    in_bank = set().union(*kinds)
    assert any(k.endswith(":other") for k in in_bank) and {"calf-hip:own", "foot-hip:own"} & in_bank and {"floor-trunk", "floor-trunk:box"} & in_bank, in_bank
    # ... and in states that were compared. (The bank's two own-hip states have joints outside the box the kernel serves and are handed on:
    # that kind is compared on its sweep, whose knee stays inside the box.)
    have = set().union(*[k for k, n in zip(kinds, rep.compared) if n > 0])
    assert any(k.endswith(":other") for k in have), have                               # leg - leg
    assert "floor-trunk" in have or "floor-trunk:box" in have, have                     # the trunk on the floor
    states = np.array([[s.state] for s, n in zip(bank.states, rep.compared) if n > 0])  # [n, H = 1, nq + nv]
    leg_leg, hip_cyl = sb.contact_census(t, MOCAP, states)
    assert len(leg_leg) >= 3 and len(hip_cyl) >= 3, (leg_leg, hip_cyl)
    for name in ("foot_on_its_own_hip_cylinder", "calf_on_a_trunk_pair_geom"):          # (trunk - leg: unreachable on the task's A1, module docstring)
        touching, _, srep = _sweep_result(name)
        assert any(tch and n > 0 for tch, n in zip(touching, srep.compared)), name
