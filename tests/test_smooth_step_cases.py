"""CPU: the constraint-free step of tests/smooth_step_cases.py (an independent 50-digit reference written from d'Alembert's principle on
differentiated positions) against the three CPU copies of the physics -- the oracle (oracle/physics.c), the quad kernel's step function
(tests/quademu) and the limb kernel's (tests/limbemu) --, and the reference held to itself first.

The reference against itself: the cart-pole's textbook Lagrangian; Euler's equations for the torque-free tumbling brick of
tests/models/free_body.xml (inertia by hand from the box's sides); on the hinge-and-slide trees (the probe's chain, the cart-pole) a second
derivation of the bias, (dM/dt) v - dT/dq + dV/dq with M(q) and V(q) differentiated by five-point stencils, which agrees with the
d'Alembert bias to 1e-25; the mutation conditions in both directions (SHOWN / not_shown) and the readings each float row still sees.

Bounds: |d - r| <= 1e-9 (1 + |r|) on every fp64 copy (test_gpu_step_parity.ROWS, asserted equal here), M within 1e-12 max|M|; the float
build of the limb step function at test_step_parity_emulators.TOL (3e-4). Worst share of the bound, measured on the CPU (no GPU):

    copy                                                  states x candidates   worst share
    oracle M (of 1e-12 max|M|)                            27 x 16               6.6e-4 (tree)
    oracle qfrc_bias / qfrc_passive / qfrc_actuator       27 x 16               1.6e-4 / 1.9e-7 / 1.4e-6
    oracle qacc_smooth                                    27 x 16               5.1e-3 (humanoid)
    oracle Euler step, six models                         27 x 16               4.0e-5 (humanoid)
    oracle RK4 step (tree, brick, cartpole, particle)     16 x 16               1.4e-6
    oracle RK4 step, probe / A1 / Humanoid                2 x 4 each            7.9e-7 / 1.4e-6 / 3.2e-5
    oracle with friction loss, momentum balance           6 x 16                1.1e-6
    limb step function fp64: state / M / qacc_smooth      6 x 16                5.3e-5 / 5.2e-4 / 5.2e-3
    limb step function fp32: state (bound 3e-4)           6 x 16                0.067
    quad step function fp64: momentum balance / M         6 x 16                9.3e-7 / 6.0e-5
The two derivations of the bias differ by 7.7e-31 (the probe's chain) and 1.5e-30 (the cart-pole). The module takes about 65 s."""
import numpy as np
import pytest

import force_noise_cases as fn
import residual_reference as rr
import smooth_step_cases as ss
import test_gpu_step_parity as tpar
import test_step_parity_emulators as temu
from tests import limbemu, quademu

mpf, MPC = ss.mpf, ss.MPC
TOL = ss.STEP_TOL64
RK4_KEYS = ss.RK4_SMALL + ss.RK4_LARGE


def test_the_bounds_are_the_projects():
    assert all(r[4] == TOL for r in tpar.ROWS.values() if r[3] == 64)
    assert {k for _, k, _ in ss.DEVICE_ROWS.values()} <= set(tpar.ROWS)


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_cartpole_matches_the_textbook_lagrangian():
    mdl = ss.model("cartpole")
    a = mdl.fm.arrays
    mc, mp, l, g = mpf(1.0), mpf(0.1), mpf(0.5), mpf(9.81)
    assert float(a["body_mass"][1]) == 1.0 and float(a["body_mass"][2]) == 0.1 and abs(float(a["body_ipos"][2][2])) == 0.5
    Ic = mpf(float(a["body_inertia"][2][1]))
    for c in ss.cases("cartpole"):
        s = ss.smooth(mdl, c.state)
        th, w = mpf(float(c.state[1])), mpf(float(c.state[3]))
        M = [[mc + mp, mp * l * MPC.cos(th)], [mp * l * MPC.cos(th), Ic + mp * l * l]]
        bias = [-mp * l * MPC.sin(th) * w * w, -mp * g * l * MPC.sin(th)]
        assert max(abs(s.mass_full()[i][j] - M[i][j]) for i in range(2) for j in range(2)) < 1e-25
        assert max(abs(x - y) for x, y in zip(s.bias(), bias)) < 1e-25


def test_the_tumbling_brick_obeys_eulers_equations():
    """torque-free: I w' = -w x I w in the body's frame, I by hand from the box's half sides (m / 3 (b^2 + c^2), ...); its centre falls
    with g; the reference's M^-1 (-bias) must say the same"""
    mdl = ss.model("brick")
    a = mdl.fm.arrays
    b = mdl.fm.names["body"].index("brick")
    hx, hy, hz = (mpf(float(v)) for v in a["geom_size"][mdl.fm.names["geom"].index("brick")])
    m = mpf(float(a["body_mass"][b]))
    I = [m / 3 * (hy * hy + hz * hz), m / 3 * (hx * hx + hz * hz), m / 3 * (hx * hx + hy * hy)]
    assert len({float(v) for v in I}) == 3 and not np.any(a["body_ipos"][b])
    state = ss.brick_state()
    s = ss.smooth(mdl, state)
    acc = s.acceleration([0.0])
    w = [mpf(float(v)) for v in state[mdl.nq + 3:mdl.nq + 6]]
    Iw = [I[k] * w[k] for k in range(3)]
    want = [-(w[1] * Iw[2] - w[2] * Iw[1]) / I[0], -(w[2] * Iw[0] - w[0] * Iw[2]) / I[1], -(w[0] * Iw[1] - w[1] * Iw[0]) / I[2]]
    assert max(abs(x) for x in want) > 1.0
    # (the model's body_inertia is the compiler's double of the same formula: good to a few ulp, not to 25 digits)
    assert max(abs(x - y) for x, y in zip(acc[3:6], want)) < 1e-13
    assert max(abs(x - y) for x, y in zip(acc[0:3], [0, 0, mpf(-9.81)])) < 1e-25
    # and with the model's own doubles for the inertia, in the order the inertial frame puts them, to the reference's own precision
    Ri = rr.q_matrix(mdl.kin.iquat[b])
    Ib = [[sum(Ri[i][k] * mpf(float(a["body_inertia"][b][k])) * Ri[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
    Iw = [sum(Ib[i][k] * w[k] for k in range(3)) for i in range(3)]
    rhs = MPC.matrix([-(w[1] * Iw[2] - w[2] * Iw[1]), -(w[2] * Iw[0] - w[0] * Iw[2]), -(w[0] * Iw[1] - w[1] * Iw[0])])
    want = MPC.lu_solve(MPC.matrix(Ib), rhs)
    assert max(abs(acc[3 + k] - want[k]) for k in range(3)) < 1e-25


def lagrange_bias(mdl, q, v, dofs, upto):
    """(dM/dt) v - dT/dq + dV/dq on the leading dofs of a hinge-and-slide tree: M(q) = sum m Jc^T Jc + Jw^T I Jw and V(q) = -sum m g . c of
    bodies 1 .. upto - 1, differentiated along each dof by a five-point stencil (step 1e-7 on entries that are smooth to 1e-35)"""
    kin = mdl.kin
    g = ss.vec(mdl.fm.scalars["gravity"])
    h = mpf(10) ** -7

    def at(qq):
        J, base = fn.jacobians(mdl, qq, upto=upto)
        n = len(dofs)
        Mm, V = [[mpf(0)] * n for _ in range(n)], mpf(0)
        for b in sorted({b for b, _ in J}):
            Ri, inertia = base.ximat(b), ss.vec(mdl.fm.arrays["body_inertia"][b])
            Iw = [[sum(Ri[i][k] * inertia[k] * Ri[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
            V -= kin.mass[b] * sum(x * y for x, y in zip(g, base.xipos(b)))
            for k in dofs:
                for l in dofs:
                    if (b, k) in J and (b, l) in J:
                        ck, _, wk = J[(b, k)]
                        cl, _, wl = J[(b, l)]
                        Mm[k][l] += kin.mass[b] * sum(x * y for x, y in zip(ck, cl)) + sum(wk[i] * Iw[i][j] * wl[j] for i in range(3) for j in range(3))
        return Mm, V
    q, v = ss.vec(q), ss.vec(v)
    n = len(dofs)
    dM, dV = [], []
    for k in dofs:
        unit = [mpf(int(i == k)) for i in range(mdl.nv)]
        f = {s: at(kin.displaced(q, unit, s * h)) for s in (-2, -1, 1, 2)}
        dM.append([[(-f[2][0][i][j] + 8 * f[1][0][i][j] - 8 * f[-1][0][i][j] + f[-2][0][i][j]) / (12 * h) for j in range(n)] for i in range(n)])
        dV.append((-f[2][1] + 8 * f[1][1] - 8 * f[-1][1] + f[-2][1]) / (12 * h))
    out = []
    for i in range(n):
        mdot_v = sum(dM[k][i][j] * v[k] * v[j] for k in range(n) for j in range(n))
        dT = sum(dM[i][j][l] * v[j] * v[l] for j in range(n) for l in range(n)) / 2
        out.append(mdot_v - dT + dV[i])
    return out


@pytest.mark.parametrize("key,upto", [("probe", 3), ("cartpole", None)])
def test_a_second_derivation_of_the_bias_agrees(key, upto):
    mdl = ss.model(key)
    assert all(t in (ss.HINGE, ss.SLIDE) for t in mdl.kin.jnt_type[:2]) and list(mdl.kin.dadr[:2]) == [0, 1]
    worst = mpf(0)
    for c in ss.cases(key):
        s = ss.smooth(mdl, c.state)
        second = lagrange_bias(mdl, c.state[:mdl.nq], c.state[mdl.nq:], [0, 1], upto)
        assert max(abs(x) for x in second) > 1e-5
        worst = max(worst, max(abs(x - y) for x, y in zip(s.bias()[:2], second)))
    print(f"{key}: the two derivations of the bias differ by {float(worst):.1e}")
    assert worst < 1e-25


@pytest.mark.parametrize("key", ss.KEYS)
def test_every_shown_reading_misses_and_no_other_moves_anything(key):
    """from the reference alone: a reading the model's arrays can show misses the fp64 bound by more than a factor of two on an entry of
    the next state of a case; a reading listed as not shown stays inside the bound on every case"""
    assert set(ss.SHOWN[key]) | set(ss.not_shown(key)) == set(ss.MUTATIONS)
    for mu in ss.SHOWN[key]:
        w = ss.visibility(key, mu, limit=2.0)
        assert w > 2.0, (key, mu, w)
    for mu in ss.not_shown(key):
        w = ss.visibility(key, mu)
        assert w <= 1.0, (key, mu, w)


def test_no_state_was_passed_over():
    """the states are the first of the ranking: none failed a condition (limits, clearance, the oracle's constraint rows)"""
    for key in ss.KEYS + ("brick",):
        ss.cases(key)
        assert ss.SKIPPED[key] == [], (key, ss.SKIPPED[key])


def test_the_arrays_say_what_cannot_be_shown():
    """the entries of not_shown() that follow from a model's arrays alone, checked against them (as model_variants.ALL_ZERO is)"""
    for key in ss.KEYS:
        a = ss.model(key).fm.arrays
        pred = {
            "armature_outside_damped_solve": bool(np.any(a["dof_armature"])),
            "explicit_damping": bool(np.any(a["dof_damping"])),
            "gear_not_squared_in_bias": bool(np.any(np.asarray(a["actuator_biastype"]) == 1) and np.any(np.asarray(a["actuator_biasprm"])[:, 1:3])),
            "spring_about_qpos0": any(a["jnt_stiffness"][j] and a["qpos_spring"][int(a["jnt_qposadr"][j])] != a["qpos0"][int(a["jnt_qposadr"][j])]
                                      for j in range(len(a["jnt_type"])) if int(a["jnt_type"][j]) in (ss.HINGE, ss.SLIDE)),
            "free_omega_in_world_frame": any(int(t) in (ss.FREE, ss.BALL) for t in a["jnt_type"]),
            "ctrl_unclamped": bool(np.any(a["actuator_ctrllimited"])),
            "gravity_at_body_origin": bool(np.any(ss.model(key).fm.scalars["gravity"])) and bool(np.any(a["body_ipos"][1:ss.model(key).nbody_live])),
        }
        for mu, can in pred.items():
            assert (mu in ss.SHOWN[key]) == can, (key, mu, can)


# A float row still sees a reading that misses its own bound by more than a factor of two on an entry of a case (from the reference alone).
# Every float row sees every reading its model shows, but for these: the A1's gyroscopic torque is 0.83 of the tree kernel's 6e-3, the
# cart-pole's damping of 1e-4 N s / m over one step 0.026 of the lane kernel's 1e-4.
FLOAT_BLIND = {"tree-a1-fp32": ("no_gyroscopic",), "lane-cartpole-fp32": ("explicit_damping",)}


@pytest.mark.parametrize("row", [r for r, (_, k, _) in ss.DEVICE_ROWS.items() if tpar.ROWS[k][3] == 32])
def test_what_a_float_row_still_sees(row):
    key, prow, _ = ss.DEVICE_ROWS[row]
    tol = tpar.ROWS[prow][4]
    seen = tuple(mu for mu in ss.SHOWN[key] if ss.visibility(key, mu, tol, limit=2.0) > 2.0)
    print(f"{row} (bound {tol:.0e}): sees {seen}")
    assert seen == tuple(mu for mu in ss.SHOWN[key] if mu not in FLOAT_BLIND.get(row, ())), (row, seen)


# ------------------------------------------------------------------------------------------------ the oracle
_PHYSICS, _ORACLE = {}, {}


def physics(key, integrator=0):
    from oracle import pyoracle
    if (key, integrator) not in _PHYSICS:
        mdl = ss.model(key)
        pm = mdl.pm
        if integrator:
            pm = mdl.task.packed_model()
            pm.struct.integrator, pm.struct.disableflags = integrator, mdl.pm.struct.disableflags
        _PHYSICS[(key, integrator)] = (pyoracle.Physics(pm), pm)
    return _PHYSICS[(key, integrator)][0]


def oracle_case(key, i, integrator=0):
    """the oracle's fields and next states for the sixteen candidates of a case"""
    if (key, i, integrator) in _ORACLE:
        return _ORACLE[(key, i, integrator)]
    mdl, c = ss.model(key), ss.cases(key)[i]
    ph, nv = physics(key, integrator), mdl.nv
    out = dict(next=[], qacc_smooth=[], actuator=[], rows=set())
    for u in c.controls[:, 0]:
        ph.set_state(c.state[:mdl.nq], c.state[mdl.nq:], mdl.time, mdl.mocap)
        ph.set_ctrl(u)
        ph.forward()
        Mo = ph.get("M").reshape(nv, nv)
        out["M"], out["bias"], out["passive"] = np.tril(Mo) + np.tril(Mo, -1).T, ph.get("qfrc_bias"), ph.get("qfrc_passive")
        out["qacc_smooth"].append(ph.get("qacc_smooth"))
        out["actuator"].append(ph.get("qfrc_actuator"))
        if int(ph.get("nefc")[0]):
            out["rows"] |= set(ph.get("efc_type").astype(int).tolist())
        ph.step()
        out["next"].append(np.concatenate([ph.get("qpos"), ph.get("qvel")]))
    for k in ("next", "qacc_smooth", "actuator"):
        out[k] = np.array(out[k])
    _ORACLE[(key, i, integrator)] = out
    return out


@pytest.mark.parametrize("key", ss.KEYS)
def test_oracle_fields(key):
    """M, qfrc_bias, qfrc_passive, qfrc_actuator and qacc_smooth, each on its own"""
    worst = {k: 0.0 for k in ("M", "bias", "passive", "actuator", "qacc_smooth")}
    for i in range(len(ss.cases(key))):
        e, o = ss.expect(key, i), oracle_case(key, i)
        assert not o["rows"]
        worst["M"] = max(worst["M"], float(np.max(np.abs(o["M"] - e.M)) / (ss.M_ATOL * np.max(np.abs(e.M)))))
        for name, got, want in (("bias", o["bias"], e.bias), ("passive", o["passive"], e.passive), ("actuator", o["actuator"], e.actuator),
                                ("qacc_smooth", o["qacc_smooth"], e.qacc_smooth)):
            worst[name] = max(worst[name], ss.share(got, want, TOL)[0])
    print(f"oracle fields on {key}: {len(ss.cases(key))} states x 16 candidates, worst share of the bound {worst}")
    assert all(w <= 1.0 for w in worst.values()), worst


@pytest.mark.parametrize("key", ss.KEYS)
def test_oracle_euler_step(key):
    worst, where = 0.0, None
    for i, c in enumerate(ss.cases(key)):
        w, at = ss.share(oracle_case(key, i)["next"], ss.expect(key, i).next_state, TOL)
        if w > worst:
            worst, where = w, (c.label, at)
    print(f"oracle Euler step on {key}: {len(ss.cases(key))} states x 16 candidates, worst share of the bound {worst:.2e} at {where}")
    assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize("key", ss.KEYS)
def test_the_oracle_fails_every_shown_reading(key):
    """the reference replaced by one of its wrong readings: the oracle's step (an fp64 row of the model) must then miss on a case"""
    for mu in ss.SHOWN[key]:
        worst = 0.0
        for i in range(len(ss.cases(key))):
            worst = max(worst, ss.share(oracle_case(key, i)["next"], ss.expect(key, i, mu).next_state, TOL)[0])
            if worst > 1.0:
                break
        assert worst > 1.0, (key, mu, worst)


@pytest.mark.parametrize("key", RK4_KEYS)
def test_oracle_rk4_step(key):
    worst, where, n = 0.0, None, 0
    for i in ss.rk4_states(key):
        c = ss.cases(key)[i]
        cands, want = ss.rk4_expect(key, i)
        w, at = ss.share(oracle_case(key, i, 1)["next"][cands], want, TOL)
        n += len(cands)
        if w > worst:
            worst, where = w, (c.label, at)
        # (RK4 is not Euler: the two references differ by far more than the bound, so the integrator switch reached the oracle)
        assert ss.share(ss.expect(key, i).next_state[cands], want, TOL)[0] > 2.0
    print(f"oracle RK4 step on {key}: {len(ss.rk4_states(key))} states, {n} candidates, worst share of the bound {worst:.2e} at {where}")
    assert worst <= 1.0, (worst, where)


def test_oracle_momentum_balance_with_friction_loss():
    worst, n = 0.0, 0
    for i in range(len(ss.cases("a1"))):
        o = oracle_case("a1-floss", i)
        assert o["rows"] == {ss.EFC_FRICTION}
        w, k = ss.momentum_balance("a1-floss", i, o["next"], TOL)
        worst, n = max(worst, w), n + k
    print(f"oracle with friction loss: {n} entries, worst share of the allowance {worst:.2e}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the emulators
def emulator_next(mod, key, i, **kw):
    mdl, c = ss.model(key), ss.cases(key)[i]
    o = mod.rollout(mdl.pm, mdl.pt, c.state, mdl.time, mdl.mocap, len(c.controls), 2, 1, 0, np.array([mdl.time]), node_values=c.controls, **kw)
    assert not o["flags"].any() and not o["failure"].any(), (key, c.label, o["flags"], o["failure"])
    return o["states"][:, 1]


@pytest.mark.parametrize("precision", [64, 32])
def test_limb_step_function(precision):
    tol = temu.TOL[("limb", precision)]
    mdl = ss.model("humanoid")
    worst = dict(state=0.0, M=0.0, qacc_smooth=0.0)
    for i, c in enumerate(ss.cases("humanoid")):
        e = ss.expect("humanoid", i)
        worst["state"] = max(worst["state"], ss.share(emulator_next(limbemu, "humanoid", i, precision=precision), e.next_state, tol)[0])
        if precision == 64:
            for k, u in enumerate(c.controls[:, 0]):
                f = limbemu.forward(mdl.pm, mdl.pt, c.state, mdl.time, mdl.mocap, np.clip(u, -1, 1))
                M = np.tril(f["M"]) + np.tril(f["M"], -1).T
                worst["M"] = max(worst["M"], float(np.max(np.abs(M - e.M)) / (ss.M_ATOL * np.max(np.abs(e.M)))))
                worst["qacc_smooth"] = max(worst["qacc_smooth"], ss.share(f["qacc_smooth"], e.qacc_smooth[k], tol)[0])
    print(f"limb step function fp{precision}: {len(ss.cases('humanoid'))} states x 16 candidates, worst share of the bound {worst}")
    assert all(w <= 1.0 for w in worst.values()), worst


def test_quad_step_function():
    """the quad kernel's form takes no disable flag and the A1 always has friction loss: its step is held to the momentum balance, its M to
    the reference's"""
    mdl = ss.model("a1-floss")
    worst, n, worst_m = 0.0, 0, 0.0
    for i, c in enumerate(ss.cases("a1")):
        e = ss.expect("a1", i)
        w, k = ss.momentum_balance("a1-floss", i, emulator_next(quademu, "a1-floss", i), TOL)
        worst, n = max(worst, w), n + k
        f = quademu.forward(mdl.pm, mdl.pt, c.state, mdl.time, mdl.mocap, np.zeros(mdl.fm.nu))
        M = np.tril(f["M"]) + np.tril(f["M"], -1).T
        worst_m = max(worst_m, float(np.max(np.abs(M - e.M)) / (ss.M_ATOL * np.max(np.abs(e.M)))))
    print(f"quad step function fp64: {n} entries, worst share of the allowance {worst:.2e}; M {worst_m:.2e} of its bound")
    assert worst <= 1.0 and worst_m <= 1.0
