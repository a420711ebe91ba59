"""CPU tests of the quad kernel's self-collision WALK (mujoco_mpc_amd/csrc/quad_step.h: pair_contacts and pair_contacts_tests -- the
leg-level cull, the unrolled pretests with the partner's geom j taken from the partner lane's registers, the fetch of only the partner
geoms and link velocities that the surviving pairs name, the pose slots the collision loop no longer zeroes) through the lock-step
emulator (tests/quademu). A cull may only remove pairs the exact test would reject, and a fetch may only leave out what no exact test reads, so

  * the emulator built as it is and built with -DQEXP_PAIRS_WALK_ALL (nothing culled: every pair of pg_active reaches the exact test, in
    the same order) must agree in every output BIT, two steps from every state of the A1 bank and of the sweeps below, and
  * along three sweeps of 41 states each across the ONSET of one leg-leg contact the emulator must follow the oracle, one step, every
    Trajectory field, |d - o| <= 1e-9 (1 + |o|) as tests/test_quad_cull_emulator.py, whose helpers run them.

The sweeps are of the kinds and lane offsets that file's do not have (it has calf-calf, foot-other hip, calf-trunk, foot-own hip). One
leg moves linearly from a pose in which the pair is clear to one in which it touches, the trunk 0.45 m up so that nothing else interferes
(the oracle lists no other contact along any of them). Found on the CPU with the oracle alone: 240 000 uniform samples of two legs' joints
inside the joint ranges, keeping states with exactly one contact, of the wanted kind and leg pair, nearest to its onset; then the line
from the moving leg's home pose to that sample, 12 % of it before the first touching point to 6 % after.

  sweep                                   kind         legs     lane offset d (from either lane of the pair)
  foot_on_the_diagonal_foot               foot-foot    (0, 3)   3 and 1
  foot_on_the_calf_two_lanes_on           calf-foot    (0, 2)   2 and 2
  calf_on_the_neighbouring_thigh          calf-thigh   (0, 1)   1 and 3

All three kinds were reachable at all three offsets inside the joint ranges (the search listed foot-foot at (0,1), (0,2), (0,3), calf-foot
at every pair, calf-thigh at (0,1), (0,2), (1,3), (2,3)), so no substitute was needed. In each sweep the fetch's ballot names the touching
partner geom and its link and leaves the partner's other geoms and links unfetched, at each of the three lane offsets; the build that culls nothing and fetches everything is the witness that nothing left out mattered."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import step_bank as sb
import test_quad_cull_emulator as cull
from mujoco_mpc_amd.cstructs import MjpcxModel, MjpcxNoiseSpec, MjpcxTask, as_f64p, as_i32p, c_f64p, c_i32p
from oracle import pyoracle
from tests import quademu

POINTS = cull.POINTS
MOCAP = cull.MOCAP
STEPS = 2            # of the equivalence runs (H = STEPS + 1 states)
_q, _legs, UP = cull._q, cull._legs, cull.UP
# name: (first state, last state, kind, the two legs)
SWEEPS = {
    "foot_on_the_diagonal_foot": (_q(0.45, UP, _legs(l0=[0.7877, 0.3615, 0.3521], l3=[-0.2334, -0.6986, 0.2688])),
                                  _q(0.45, UP, _legs(l0=[0.7877, 0.3615, 0.3521], l3=[-0.2808, -0.8338, 0.3377])), "foot-foot", (0, 3)),
    "foot_on_the_calf_two_lanes_on": (_q(0.45, UP, _legs(l0=[0.7466, 0.1558, -0.3709], l2=[0.4697, -1.0967, 0.3343])),
                                      _q(0.45, UP, _legs(l0=[0.7466, 0.1558, -0.3709], l2=[0.5697, -1.3239, 0.4201])), "calf-foot", (0, 2)),
    "calf_on_the_neighbouring_thigh": (_q(0.45, UP, _legs(l0=[0.4506, -1.2525, -0.3612], l1=[-0.6986, -0.7604, 0.707])),
                                       _q(0.45, UP, _legs(l0=[0.4506, -1.2525, -0.3612], l1=[-0.8418, -0.921, 0.8571])), "calf-thigh", (0, 1)),
}


def sweep_states(name):
    q0, q1 = SWEEPS[name][0], SWEEPS[name][1]
    v = 0.2 * np.random.default_rng(100 + sorted(SWEEPS).index(name)).normal(size=18)   # (moving: the contact rows' velocity terms take part)
    return [sb.BankState(f"{name}/{i}", np.concatenate([q0 + s * (q1 - q0), v]), 0.0, MOCAP, *sb._a1_residual(cull._task(), 0, 2, 0.0))
            for i, s in enumerate(np.linspace(0.0, 1.0, POINTS))]


@functools.lru_cache(maxsize=None)
def leg_contacts():
    """state -> the oracle's contacts between two legs: a set of ('<part>-<part>' sorted, (leg, leg) sorted, legs numbered in joint order)"""
    t = cull._task()
    m = t.model
    a = m.arrays
    parent, gb, gt = a["body_parentid"], a["geom_bodyid"], a["geom_type"]
    trunk = next(b for b in range(m.nbody) if a["body_dofnum"][b] == 6)
    legs = sb._legs(t)
    order = sorted(set(x for x in legs if x >= 0))
    ph = pyoracle.Physics(cull._model(False))

    def part(g):
        if gt[g] == 2:      # MJPCX_GEOM_SPHERE: the feet
            return "foot"
        b, depth = int(gb[g]), 0
        while parent[b] != trunk:
            b, depth = int(parent[b]), depth + 1
        return ("hip", "thigh", "calf")[depth]

    def contacts(state, time, mocap):
        ph.set_state(state[:m.nq], state[m.nq:], float(time), mocap)
        ph.forward()
        out = set()
        for r in ph.get("contact").reshape(-1, 11)[:int(ph.get("ncon")[0])]:
            g1, g2 = int(r[7]), int(r[8])
            if legs[g1] >= 0 and legs[g2] >= 0 and legs[g1] != legs[g2]:
                out.add(("-".join(sorted([part(g1), part(g2)])), tuple(sorted([order.index(legs[g1]), order.index(legs[g2])]))))
        return out
    return contacts


# ------------------------------------------------------------------------------------------ the two builds of the emulator
@functools.lru_cache(maxsize=None)
def _builds():
    """(as it is, with -DQEXP_PAIRS_WALK_ALL): tests/quademu/quademu.cc compiled into a temporary directory, the g++ line of
    tests/quademu/__init__.py; the directory lives as long as the session"""
    tmp = tempfile.TemporaryDirectory(prefix="quademu_walk_")
    src = os.path.join(os.path.dirname(os.path.abspath(quademu.__file__)), "quademu.cc")
    libs = []
    for name, flags in (("product", []), ("walk_all", ["-DQEXP_PAIRS_WALK_ALL"])):
        so = os.path.join(tmp.name, f"libquademu_{name}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off"] + flags + ["-o", so, src])
        L = C.CDLL(so)
        L.quademu_rollout.argtypes = [C.POINTER(MjpcxModel), C.POINTER(MjpcxTask), c_f64p, C.c_double, c_f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      c_f64p, c_f64p, C.POINTER(MjpcxNoiseSpec), c_f64p] + [c_f64p] * 7 + [c_i32p, c_f64p, c_i32p]
        libs.append(L)
    return tmp, libs[0], libs[1]


def _rollout(L, pm, pt, s, nodes, H):
    """tests/quademu rollout() on the library L: N = len(nodes) candidates, H states, one zero-order node"""
    m = pm.struct
    N, ds, nu, nr, ntr = len(nodes), m.nq + m.nv, m.nu, pt.struct.num_residual, pt.struct.num_trace
    f = lambda x: np.ascontiguousarray(x, dtype=np.float64)   # noqa: E731
    out = dict(states=np.zeros((N, H, ds)), actions=np.zeros((N, H, nu)), times=np.zeros((N, H)), residual=np.zeros((N, H, nr)),
               costs=np.zeros((N, H)), trace=np.zeros((N, H, 3 * ntr)), total_return=np.zeros(N), failure=np.zeros(N, np.int32),
               nodes=np.zeros((N, 1, nu)), flags=np.zeros(N, np.int32))
    keep = [f(s.state), f(s.mocap), f([s.time]), f(nodes), f(np.zeros((1, nu)))]
    rc = L.quademu_rollout(pm.ptr, pt.ptr, as_f64p(keep[0]), float(s.time), as_f64p(keep[1]), N, H, 1, 0, as_f64p(keep[2]), as_f64p(keep[3]), None,
                           as_f64p(keep[4]), as_f64p(out["states"]), as_f64p(out["actions"]), as_f64p(out["times"]), as_f64p(out["residual"]),
                           as_f64p(out["costs"]), as_f64p(out["trace"]), as_f64p(out["total_return"]), as_i32p(out["failure"]), as_f64p(out["nodes"]),
                           as_i32p(out["flags"]))
    assert rc == 0, s.label
    return out


@functools.lru_cache(maxsize=None)
def _equivalence():
    """every state of the bank and of the sweeps through both builds -> (states, per state: candidates neither build handed on, the
    differences found: (label, field))"""
    _, product, walk_all = _builds()
    t, pm = cull._task(), cull._model(False)
    states = list(sb.a1_bank().states) + [s for name in sorted(SWEEPS) for s in sweep_states(name)]
    kept, diffs = [], []
    for k, s in enumerate(states):
        nodes = sb.controls_for(t, k)
        pt = sb.packed_task(t, s)
        a, b = _rollout(product, pm, pt, s, nodes, STEPS + 1), _rollout(walk_all, pm, pt, s, nodes, STEPS + 1)
        for name in ("flags",) + sb.FIELDS:
            if not np.array_equal(a[name], b[name]):
                diffs.append((s.label, name))
        kept.append(int(np.sum((a["flags"] == 0) & (b["flags"] == 0))))
    return states, kept, diffs


def test_the_culled_walk_and_the_unculled_walk_agree_bit_for_bit():
    states, kept, diffs = _equivalence()
    print(f"{len(states)} states x {sb.STEP_CANDIDATES} candidates x {STEPS} steps, {sum(kept)} candidates kept by both builds")
    assert not diffs, diffs[:6]
    assert sum(k > 0 for k in kept) >= len(states) - 12, kept


def test_the_states_compared_hold_leg_leg_and_hip_cylinder_contacts():
    """non-vacuity by the oracle alone (step_bank.contact_census, as tests/test_quad_cull_emulator.py asserts for its own), over the states
    of which some candidate was rolled by both builds, not handed on"""
    states, kept, _ = _equivalence()
    arr = np.array([[s.state] for s, n in zip(states, kept) if n > 0])   # [n, H = 1, nq + nv]
    leg_leg, hip_cyl = sb.contact_census(cull._task(), MOCAP, arr)
    assert len(leg_leg) >= 3 and len(hip_cyl) >= 3, (leg_leg, hip_cyl)


@functools.lru_cache(maxsize=None)
def _sweep_result(name):
    """(per state: whether the oracle lists the sweep's contact, every leg-leg contact along the sweep, the step report against the oracle)"""
    kind, pair = SWEEPS[name][2], SWEEPS[name][3]
    states = sweep_states(name)
    seen = [leg_contacts()(s.state, s.time, s.mocap) for s in states]
    _, rep = cull._step_all(states, False)
    return [(kind, pair) in c for c in seen], set().union(*seen), rep


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_sweep_across_the_onset_of_a_leg_leg_contact(name):
    touching, seen, rep = _sweep_result(name)
    first = touching.index(True) if True in touching else -1
    print(f"{name}: first touching state {first} of {POINTS}, leg-leg contacts along the sweep {sorted(seen)}, {sum(rep.compared)} candidates compared, "
          f"worst {rep.worst:.2e} at {rep.where}")
    assert not touching[0] and 0 < sum(touching) < POINTS, touching
    assert all(n > 0 for n in rep.compared[max(first - 2, 0):first + 3]), rep.compared
    assert sum(n > 0 for n in rep.compared) >= POINTS - 4, rep.compared
    assert not rep.failures, rep.failures[:4]


def test_the_sweeps_cover_the_three_lane_offsets_and_the_three_kinds():
    """by the oracle's contact lists of states that were compared: foot-foot, foot-calf and calf-thigh, and pairs at lane offsets 1, 2 and 3"""
    kinds, offsets = set(), set()
    for name in SWEEPS:
        touching, _, rep = _sweep_result(name)
        if any(tch and n > 0 for tch, n in zip(touching, rep.compared)):
            a, b = SWEEPS[name][3]
            kinds.add(SWEEPS[name][2])
            offsets |= {(b - a) & 3, (a - b) & 3}
    assert kinds == {"foot-foot", "calf-foot", "calf-thigh"} and offsets == {1, 2, 3}, (kinds, offsets)
