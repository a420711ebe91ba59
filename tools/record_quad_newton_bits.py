#!/usr/bin/env python3
"""Writes tests/golden/quad_newton_bits.npz, the fixture of tests/test_quad_newton_bits_emulator.py: single forward steps of the quad kernel's
step function through the CPU emulator (tests/quademu, g++ -ffp-contract=off), recorded bit for bit.
    python tools/record_quad_newton_bits.py [out.npz]
    python tools/record_quad_newton_bits.py --device [out.npz]     on an MI355X: tests/golden/quad_newton_bits_device.npz, the returns, failure
                                                                   words and hand-on counts of tests/test_gpu_quad_newton_bits.py's launches
RUN IT FROM A CHECKOUT OF THE COMMIT WHOSE BITS ARE THE REFERENCE (the fixture in the tree is the parent of round 12's: the solver before
its statements were reordered): the test then says that a later quad_step.h still rounds every operation of the solver alike.

The states: every state of the A1 bank (tests/step_bank.py), cold and warm-started, and four states found here with the oracle's contact
lists (deterministic searches; the states themselves are stored, so the test needs no search):
  foot_foot / calf_thigh   the first touching state of two of tests/test_quad_pair_walk_emulator.py's sweeps across a contact's onset
  five_in_a_lane           a leg with at least five contacts (more than the line search's four register slots: the BEYOND search)
  two_partners             a leg in contact with two other legs (the leaf elimination: constraint_newton<true>)
the last two from the large-noise rollouts of tests/test_quad_emulator.py::test_a_leg_touching_two_others_and_cylinders."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import step_bank as sb                                  # noqa: E402
import test_quad_pair_walk_emulator as walk             # noqa: E402
from oracle import pyoracle                             # noqa: E402
from tests import quademu                               # noqa: E402

FIELDS = ("qacc", "qfrc_smooth", "qfrc_constraint")


def per_leg_contacts(task, ph, legs, state, time, mocap):
    """(contacts per leg, the set of other legs each leg touches) by the oracle's contact list"""
    m = task.model
    ph.set_state(state[:m.nq], state[m.nq:], float(time), mocap)
    ph.forward()
    order = sorted(set(x for x in legs if x >= 0))
    n, partners = [0] * 4, [set() for _ in range(4)]
    for r in ph.get("contact").reshape(-1, 11)[:int(ph.get("ncon")[0])]:
        a, b = legs[int(r[7])], legs[int(r[8])]
        for x, y in ((a, b),) if a == b else ((a, b), (b, a)):   # (a leg-leg contact is a row of both lanes)
            if x >= 0:
                n[order.index(x)] += 1
                if y >= 0 and y != x:
                    partners[order.index(x)].add(order.index(y))
    return n, partners


def searched_states(task):
    """[(label, state, time, mocap)]"""
    out = []
    for name, label in (("foot_on_the_diagonal_foot", "foot_foot"), ("calf_on_the_neighbouring_thigh", "calf_thigh")):
        states = walk.sweep_states(name)
        kind, pair = walk.SWEEPS[name][2], walk.SWEEPS[name][3]
        first = next(s for s in states if (kind, pair) in walk.leg_contacts()(s.state, s.time, s.mocap))
        out.append((label, first.state, first.time, first.mocap))
    pm, pt = task.packed_model(), task.packed()
    ph = pyoracle.Physics(pm)
    legs = sb._legs(task)
    home = np.concatenate([task.model.keyframes["home"]["qpos"], np.zeros(18)])
    mocap = walk.MOCAP
    N, H, P = 12, 100, 3
    times = np.arange(P) * ((H - 1) * 0.01 / (P - 1))
    want = {"five_in_a_lane": lambda n, p: max(n) >= 5 and max(len(x) for x in p) <= 1, "two_partners": lambda n, p: max(len(x) for x in p) >= 2}
    for seed in (0, 1):
        nodes = np.clip(np.random.default_rng(seed).normal(0, 0.5, (N, P, 12)), -1, 1)
        ref = pyoracle.rollout_batch(pm, pt, home, 0.0, mocap, N, H, P, 0, times, nodes, num_threads=4)
        for c in range(N):
            for k in range(H):
                if not want:
                    return out
                st, tm = ref["states"][c, k], float(ref["times"][c, k])
                n, p = per_leg_contacts(task, ph, legs, st, tm, mocap)
                for label in [w for w in want if want[w](n, p)]:
                    if quademu.forward(pm, pt, st, tm, mocap, np.zeros(12))["flags"] == 0:   # (a state the quad form covers)
                        out.append((label, st.copy(), tm, mocap))
                        print(f"{label}: seed {seed} candidate {c} step {k}, contacts per leg {n}, partners {[sorted(x) for x in p]}")
                        del want[label]
    raise SystemExit(f"not found: {sorted(want)}")


def cases():
    """[(label, packed model, packed task, state, time, mocap, ctrl)]: the test walks the same list"""
    bank = sb.a1_bank()
    t = bank.task
    pm = t.packed_model()
    out = []
    for k, s in enumerate(bank.states):
        out.append((s.label, pm, sb.packed_task(t, s), s.state, s.time, s.mocap, sb.controls_for(t, k)[3 + k % 13, 0]))
    pt = t.packed()
    for k, (label, state, time, mocap) in enumerate(searched_states(t)):
        out.append((label, pm, pt, state, time, mocap, sb.controls_for(t, 500 + k)[3, 0]))
    return out


def record(case_list):
    """one row per case in every array; <run>_flags -1: not run (no warm start where the cold solve was handed on), rows of a run whose
    flags are not 0 stay zero"""
    n = len(case_list)
    rec = {"label": np.array([c[0] for c in case_list]), "state": np.array([c[3] for c in case_list]), "time": np.array([c[4] for c in case_list]),
           "mocap": np.array([c[5] for c in case_list]), "ctrl": np.array([c[6] for c in case_list])}
    for name in ("cold", "warm"):
        rec[f"{name}_flags"] = np.full(n, -1, np.int32)
        rec[f"{name}_iters"] = np.zeros(n, np.int32)
        rec[f"{name}_cost"] = np.zeros(n)
        for f in FIELDS:
            rec[f"{name}_{f}"] = np.zeros((n, 18))
    for i, (label, pm, pt, state, time, mocap, ctrl) in enumerate(case_list):
        cold = quademu.forward(pm, pt, state, time, mocap, ctrl)
        runs = [("cold", cold)]
        if cold["flags"] == 0:   # the warm start: the cold answer pulled a tenth towards zero (the solver compares it with qacc_smooth, then iterates)
            runs.append(("warm", quademu.forward(pm, pt, state, time, mocap, ctrl, warm=0.9 * cold["qacc"])))
        for name, o in runs:
            rec[f"{name}_flags"][i] = o["flags"]
            if o["flags"] == 0:
                for f in FIELDS:
                    rec[f"{name}_{f}"][i] = o[f]
                rec[f"{name}_cost"][i], rec[f"{name}_iters"][i] = o["cost"], o["iters"]
    return rec


def record_device(path):
    """--device (on an MI355X, the library built at the reference commit): the launches of tests/test_gpu_quad_newton_bits.py, their
    returns, failure words and hand-on counts -> tests/golden/quad_newton_bits_device.npz"""
    import test_gpu_quad_newton_bits as dev
    rec = {}
    for which in dev.STARTS:
        r = dev.launch(which)
        for k in ("ret", "failure", "failure_raw"):
            rec[f"{which}_{k}"] = r[k]
        rec[f"{which}_handed_on"] = np.array(r["handed_on"])
        print(f"{which}: handed on {r['handed_on']}, failure words set {int(np.count_nonzero(r['failure_raw']))}, returns {r['ret'].min():.4f}..{r['ret'].max():.4f}")
    np.savez_compressed(path, **rec)
    print(f"{path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    if "--device" in sys.argv:
        sys.argv.remove("--device")
        record_device(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "quad_newton_bits_device.npz"))
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "quad_newton_bits.npz")
    r = record(cases())
    np.savez_compressed(path, **r)
    ok = r["cold_flags"] == 0
    print(f"{len(ok)} states, {int(ok.sum())} solved by the quad form, iterations cold {sorted(r['cold_iters'][ok].tolist())} warm "
          f"{sorted(r['warm_iters'][ok].tolist())}: {path} ({os.path.getsize(path)} bytes)")
