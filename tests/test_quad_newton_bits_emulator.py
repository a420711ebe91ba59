"""The quad kernel's Newton solver (mujoco_mpc_amd/csrc/quad_step.h constraint_newton) rounds every operation as it did before its
statements were reordered for the register allocator: single forward steps through the lock-step emulator
(tests/quademu, the same source, g++ -ffp-contract=off) give qacc, qfrc_smooth, qfrc_constraint, the cost and the solver's iteration
count BIT FOR BIT as tests/golden/quad_newton_bits.npz holds them, recorded by tools/record_quad_newton_bits.py from the emulator built
at the parent commit of that round.

The states: every state of the A1 bank (tests/step_bank.py), and four that the recording script found with the oracle's contact lists and
stored -- the first touching state of a foot-foot and of a calf-thigh sweep (tests/test_quad_pair_walk_emulator.py), a leg with five
contacts (more than the line search's four register slots: the memory-resident coefficients of line_search<.., BEYOND>), a leg touching
two others (the leaf elimination of constraint_newton<true>). Each is solved cold and from a warm start (0.9 x the cold answer), so the
warm-start comparison and the way back from a rejected one (rows_step_only) run as well."""
import functools
import os

import numpy as np
import pytest

import step_bank as sb
from mujoco_mpc_amd.task import load_task
from tests import quademu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_newton_bits.npz")
FIELDS = ("qacc", "qfrc_smooth", "qfrc_constraint")
EXTRA = ("foot_foot", "calf_thigh", "five_in_a_lane", "two_partners")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def results():
    """per recorded case: (row, label, [(run, what the emulator gives now)]); the bank's states are the bank's own (checked against the stored ones)"""
    g = golden()
    bank = sb.a1_bank()
    t = bank.task
    pm = t.packed_model()
    n = len(g["label"])
    assert n == len(bank.states) + len(EXTRA)
    out = []
    for i in range(n):
        label = str(g["label"][i])
        state, time, mocap, ctrl = g["state"][i], float(g["time"][i]), g["mocap"][i], g["ctrl"][i]
        if i < len(bank.states):
            s = bank.states[i]
            assert label == s.label and np.array_equal(state, s.state) and time == s.time and np.array_equal(mocap, s.mocap), label
            pt = sb.packed_task(t, s)
        else:
            assert label == EXTRA[i - len(bank.states)]
            pt = t.packed()
        runs = [("cold", quademu.forward(pm, pt, state, time, mocap, ctrl))]
        if g["warm_flags"][i] >= 0:
            runs.append(("warm", quademu.forward(pm, pt, state, time, mocap, ctrl, warm=0.9 * g["cold_qacc"][i])))
        out.append((i, label, runs))
    return out


def test_every_recorded_step_is_reproduced_bit_for_bit():
    g = golden()
    bad, solved, iters = [], 0, []
    for i, label, runs in results():
        for name, o in runs:
            if o["flags"] != int(g[f"{name}_flags"][i]):
                bad.append((label, name, "flags", o["flags"]))
                continue
            if o["flags"] != 0:
                continue   # (a state the quad form hands on: nothing is computed)
            solved += 1
            iters.append(o["iters"])
            for f in FIELDS:
                if not np.array_equal(o[f], g[f"{name}_{f}"][i]):
                    bad.append((label, name, f, float(np.max(np.abs(o[f] - g[f"{name}_{f}"][i])))))
            if o["cost"] != float(g[f"{name}_cost"][i]):
                bad.append((label, name, "cost", o["cost"] - float(g[f"{name}_cost"][i])))
            if o["iters"] != int(g[f"{name}_iters"][i]):
                bad.append((label, name, "iters", o["iters"], int(g[f"{name}_iters"][i])))
    print(f"{solved} solves compared, Newton iterations {min(iters)}..{max(iters)}, {sum(k > 1 for k in iters)} of them more than one")
    assert not bad, bad[:8]


def test_the_recording_is_not_vacuous():
    """most states are solved by the quad form, the solver iterates in most of them, the four searched states are solved in at least two
    iterations, and a warm start is recorded wherever a cold one is"""
    g = golden()
    flags, it = g["cold_flags"], g["cold_iters"]
    n, ok = len(flags), g["cold_flags"] == 0
    assert ok.sum() >= n - 12 and (it[ok] >= 2).sum() >= ok.sum() // 2, (flags, it)
    assert ok[-len(EXTRA):].all() and (it[-len(EXTRA):] >= 2).all()
    assert np.array_equal(g["warm_flags"] >= 0, ok)


@pytest.mark.parametrize("label", EXTRA)
def test_the_searched_states_are_what_their_names_say(label):
    """by the oracle's contact list of the stored state: the leg-leg pair of the sweep, five contacts in one leg's lane, a leg with two partners"""
    import test_quad_pair_walk_emulator as walk
    from oracle import pyoracle
    g = golden()
    i = len(g["label"]) - len(EXTRA) + EXTRA.index(label)
    state, time, mocap = g["state"][i], float(g["time"][i]), g["mocap"][i]
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    if label in ("foot_foot", "calf_thigh"):
        name = {"foot_foot": "foot_on_the_diagonal_foot", "calf_thigh": "calf_on_the_neighbouring_thigh"}[label]
        assert (walk.SWEEPS[name][2], walk.SWEEPS[name][3]) in walk.leg_contacts()(state, time, mocap)
        return
    m = t.model
    legs = sb._legs(t)
    order = sorted(set(x for x in legs if x >= 0))
    ph = pyoracle.Physics(t.packed_model())
    ph.set_state(state[:m.nq], state[m.nq:], time, mocap)
    ph.forward()
    n, partners = [0] * 4, [set() for _ in range(4)]
    for r in ph.get("contact").reshape(-1, 11)[:int(ph.get("ncon")[0])]:
        a, b = legs[int(r[7])], legs[int(r[8])]
        for x, y in ((a, b),) if a == b else ((a, b), (b, a)):
            if x >= 0:
                n[order.index(x)] += 1
                if y >= 0 and y != x:
                    partners[order.index(x)].add(order.index(y))
    if label == "five_in_a_lane":
        assert max(n) >= 5, n
    else:
        assert max(len(p) for p in partners) >= 2, partners
