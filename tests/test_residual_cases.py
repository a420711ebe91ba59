"""CPU: the residual cases of tests/residual_cases.py (answers from the independent mpmath reference, tests/residual_reference.py) against
the three CPU copies of the task residuals: the oracle, the quad kernel's step function (quademu) and the limb kernel's (limbemu, fp64 and
fp32); and the reference held to itself: its self-checks, the hand-derived literals, the branch census, the mutations.

Bounds: fp64 copies |d - e| <= 1e-9 (1 + |e|) (residual_cases.FP64_BOUND, the project's one-step bound); the float build of the limb step
function STEP_GOAL = 1e-4 against the reference at the float32-rounded inputs."""
import numpy as np
import pytest

import residual_cases as rc
import residual_reference as rr
from oracle import pyoracle

M = rr._M
mpf = M.mpf


def packed(c):
    """the case's task packed with its frozen residual state and parameters"""
    t = rc.task_of(c.task)
    keep = t.residual_int, t.residual_real, t.parameters
    t.residual_int, t.residual_real = list(c.residual_int), list(c.residual_real)
    t.parameters = list(c.parameters) if c.parameters else keep[2]
    try:
        return t.packed()
    finally:
        t.residual_int, t.residual_real, t.parameters = keep


def clamped(c):
    a = rc.task_of(c.task).model.arrays
    return np.clip(c.ctrl, a["actuator_ctrlrange"][:, 0], a["actuator_ctrlrange"][:, 1])


def rel(d, e):
    return np.abs(np.asarray(d) - e) / (1 + np.abs(e))


def report(title, rows, bound):
    worst = max(rows, key=lambda r: r[0])
    print(f"{title}: {len(rows)} cases, worst {worst[0]:.2e} (bound {bound:.0e}) at {worst[1]}")
    missed = [r for r in rows if not r[0] <= bound]
    assert not missed, sorted(missed, reverse=True)[:5]


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_reference_kinematics_self_checks():
    kin = rc.kinematics("QuadrupedFlat")
    a = kin.m.arrays
    assert all(np.array_equal(q, [1, 0, 0, 0]) for q in a["body_quat"])
    P = kin.forward(a["qpos0"], None)
    for b in range(1, kin.nbody):                        # at qpos0 every body sits at the sum of body_pos up its chain
        s, p = np.zeros(3), b
        while p > 0:
            s, p = s + a["body_pos"][p], kin.parent[p]
        assert max(abs(x - mpf(float(v))) for x, v in zip(P.xpos(b), s)) < 1e-15, b
    rng = np.random.default_rng(1)                       # the head site is p + R(q) (0.3, 0, 0)
    q = np.array(a["qpos0"], float)
    q[:3], q[3:7], q[7:] = rng.normal(0, 1, 3), rng.normal(0, 1, 4), rng.normal(0, 0.5, 12)
    u = rr.q_unit(rr.MP, rr.MP.vec(q[3:7]))
    w, x, y, z = u
    first_column = [1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)]
    head = kin.forward(q, None).site_xpos(kin.name("site", "head"))
    assert max(abs(h - (mpf(float(p)) + mpf(0.3) * c)) for h, p, c in zip(head, q[:3], first_column)) < 1e-17    # (0.3 as the double the model holds)
    cart = rc.task_of("Cartpole").model                      # a slide joint: the cart sits at body_pos + q axis, its frame unturned
    ck, ca = rr.Kinematics(cart), cart.arrays
    j = int(np.flatnonzero(np.asarray(ca["jnt_type"]) == rr.JOINT_TYPES["slide"])[0])
    b, q = int(ca["jnt_bodyid"][j]), np.array([0.37, -0.8])
    assert ck.parent[b] == 0 and np.array_equal(ca["body_quat"][b], [1, 0, 0, 0])
    Pc = ck.forward(q, None)
    want = [mpf(float(p)) + mpf(float(q[ck.qadr[j]])) * mpf(float(x)) for p, x in zip(ca["body_pos"][b], ca["jnt_axis"][j])]
    assert max(abs(x - w) for x, w in zip(Pc.xpos(b), want)) < 1e-17
    assert Pc.xmat(b) == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    # a ball joint: the trunk's free joint read as a ball about an anchor off the body's origin. The body turns about the anchor by
    # Rodrigues' formula for the angle t about the unit axis n, composed by hand: R = cos t I + (1 - cos t) n n^T + sin t [n]x, and
    # its origin sits at body_pos + anchor - R anchor; body_iquat turns the inertial frame on top of that
    trunk, jt = kin.name("body", "trunk"), int(np.flatnonzero(np.asarray(a["jnt_type"]) == rr.JOINT_TYPES["free"])[0])
    saved = {k: a[k] for k in ("jnt_type", "jnt_pos", "body_iquat")}
    anchor, iq = np.array([0.05, -0.02, 0.03]), np.array([0.8, 0.2, 0.4, -0.4])
    a["jnt_type"] = np.where(np.arange(len(saved["jnt_type"])) == jt, rr.JOINT_TYPES["ball"], saved["jnt_type"])
    a["jnt_pos"], a["body_iquat"] = np.array(saved["jnt_pos"], float), np.array(saved["body_iquat"], float)
    a["jnt_pos"][jt], a["body_iquat"][trunk] = anchor, iq
    try:
        bk = rr.Kinematics(kin.m)
        t, n = mpf(0.9), [mpf(2) / 7, mpf(-3) / 7, mpf(6) / 7]
        qb = np.array(a["qpos0"], float).tolist()
        adr = bk.qadr[jt]
        qb = rr.MP.vec(qb)
        qb[adr:adr + 4] = [M.cos(t / 2)] + [M.sin(t / 2) * v for v in n]
        cross = [[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]]
        R = [[M.cos(t) * (i == j_) + (1 - M.cos(t)) * n[i] * n[j_] + M.sin(t) * cross[i][j_] for j_ in range(3)] for i in range(3)]
        Pb = bk.forward(qb, None)
        am = rr.MP.vec(anchor)
        want = [mpf(float(a["body_pos"][trunk][i])) + am[i] - sum(R[i][k] * am[k] for k in range(3)) for i in range(3)]
        assert max(abs(x - w) for x, w in zip(Pb.xpos(trunk), want)) < 1e-40
        assert max(abs(Pb.xmat(trunk)[i][k] - R[i][k]) for i in range(3) for k in range(3)) < 1e-40
        Ri = rr.q_matrix(rr.q_unit(rr.MP, rr.MP.vec(iq)))
        RRi = [[sum(R[i][k] * Ri[k][j_] for k in range(3)) for j_ in range(3)] for i in range(3)]
        assert max(abs(Pb.ximat(trunk)[i][k] - RRi[i][k]) for i in range(3) for k in range(3)) < 1e-40
        # and q (+) eps v turns a ball in its own frame: after a turn by s about the same axis the angle is t + s
        vel = [0.0] * kin.m.nv
        vel[bk.dadr[jt]:bk.dadr[jt] + 3] = [float(x) for x in n]
        qs = bk.displaced(qb, vel, mpf(0.25))
        assert max(abs(x - w) for x, w in zip(qs[adr:adr + 4], [M.cos((t + 0.25) / 2)] + [M.sin((t + 0.25) / 2) * mpf(float(v)) for v in n])) < 1e-15
    finally:
        for k, v in saved.items():
            a[k] = v


def test_reference_com_velocity_is_the_mass_weighted_body_velocity():
    kin = rc.kinematics("HumanoidTrack")
    c = rc.cases("HumanoidTrack")[1]
    nq = kin.m.nq
    root = kin.name("body", "pelvis") if "pelvis" in kin.m.names["body"] else 1
    while kin.parent[root] != 0:
        root = kin.parent[root]
    bodies = kin.forward(c.state[:nq], None).subtree(root)
    com_v = kin.velocity(c.state[:nq], c.state[nq:], None, lambda p: p.subtree_com(root))
    each = kin.velocity(c.state[:nq], c.state[nq:], None, lambda p: [x for b in bodies for x in p.xipos(b)])
    total = sum(kin.mass[b] for b in bodies)
    mean = [sum(kin.mass[b] * each[3 * i + k] for i, b in enumerate(bodies)) / total for k in range(3)]
    assert len(bodies) > 10 and max(abs(a - b) for a, b in zip(com_v, mean)) < 1e-25
    assert max(abs(v) for v in com_v) > 0.1


def test_flip_constants_meet_their_anchors():
    """the fourteen constants QuadrupedFlat.reset hands the kernels, against the design: heights 0.25 -> 0.15 -> 0.5 -> 0.8 -> 0.5 -> 0.25 and
    angles 0, 0, pi/2, 1.125 pi, 1.75 pi, 2 pi at 0, crouch_time, jump_time, + flight_time / 2, + flight_time, + land_time; rest at the
    bottom of the crouch and at the end of the landing; continuous speed and turning rate at take-off"""
    g, jump_vel, flight, jump_acc, crouch, leap, jump, crouch_vel, land, land_acc, w_flight, w_jump, rot_acc, land_rot_acc = rc.task_of("QuadrupedFlat").flip
    pi = np.pi
    h = lambda t: 0.25 + t * crouch_vel + 0.5 * t * t * jump_acc
    near = lambda a, b: abs(a - b) < 1e-13
    assert g == 9.81 and near(jump, crouch + leap)
    assert near(h(crouch), 0.15) and near(crouch_vel + jump_acc * crouch, 0.0)
    assert near(h(jump), 0.5) and near(crouch_vel + jump_acc * jump, jump_vel)
    assert near(0.5 + jump_vel * flight / 2 - 0.5 * g * (flight / 2) ** 2, 0.8) and near(jump_vel - g * flight / 2, 0.0)
    assert near(0.5 + jump_vel * flight - 0.5 * g * flight ** 2, 0.5)
    assert near(0.5 - jump_vel * land + 0.5 * land_acc * land ** 2, 0.25) and near(-jump_vel + land_acc * land, 0.0)
    assert near(0.5 * rot_acc * leap ** 2 + w_jump * leap, pi / 2) and near(w_jump + rot_acc * leap, w_flight)
    assert near(pi / 2 + w_flight * flight / 2, 1.125 * pi) and near(pi / 2 + w_flight * flight, 1.75 * pi)
    assert near(1.75 * pi + w_flight * land - 0.5 * land_rot_acc * land ** 2, 2 * pi)
    P = rr.flip_profile(rr.MP)                            # and the reference's own design values
    for got, key in ((jump_vel, "v_jump"), (flight, "flight"), (jump_acc, "acc"), (crouch, "crouch"), (leap, "leap"), (jump, "jump"), (land, "land"),
                     (w_flight, "w_flight"), (w_jump, "w_jump")):
        assert abs(mpf(got) - P[key]) < 1e-13, key
    th = [crouch, jump, jump + flight, jump + flight + land]
    for t, height, angle in ((0, 0.25, 0), (P["crouch"], 0.15, 0), (P["jump"], 0.5, M.pi / 2), (P["jump"] + P["flight"] / 2, 0.8, 1.125 * M.pi),
                             (P["jump"] + P["flight"], 0.5, 1.75 * M.pi), (P["jump"] + P["flight"] + P["land"], 0.25, 2 * M.pi)):
        _, hh, aa = rr.flip_target(rr.MP, mpf(t), th)
        assert abs(hh - mpf(height)) < 1e-15 and abs(aa - angle) < 1e-14, (t, hh, aa)


def test_step_height_known_values():
    pi = rr.MP.pi
    for phi in (0, 0.25, 0.33, 0.75):                    # duty 0: a half cosine over the whole cycle
        assert abs(rr.step_height(rr.MP, 2 * pi * mpf(phi) + pi / 3, 2 * pi * mpf(phi), mpf(0), set()) - M.cos(pi / 6)) < 1e-45
    assert abs(rr.step_height(rr.MP, pi / 3, mpf(0), mpf(0.5), set()) - mpf(0.5)) < 1e-45          # duty 0.5: cos(pi / 3)
    assert rr.step_height(rr.MP, pi / 3, mpf(0), mpf(0.75), set()) == 0                            # duty 0.75: 2 pi / 3 clipped to pi / 2
    assert abs(rr.step_height(rr.MP, pi / 8, mpf(0), mpf(0.75), set()) - M.cos(pi / 4)) < 1e-45
    assert rr.step_height(rr.MP, mpf(1), mpf(0), mpf(1), set()) == 0
    lab = set()
    assert rr.step_height(rr.MP, mpf(-4), mpf(0), mpf(0), lab) == 0 and "gait:negative-fmod" in lab  # C's fmod keeps the sign: clipped to -pi / 2


def test_ground_closed_forms():
    kin = rc.kinematics("QuadrupedFlat")
    mocap = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.0, 0.5, 0.1, *rc.quat([0, 0, 1], 0.5)])
    P = kin.forward(kin.m.arrays["qpos0"], mocap)
    z, name, inside = rr.ground_height(P, mpf(0), mpf(0), mpf(1))
    assert (z, name, inside) == (mpf(-0.01), "floor", False)
    z, name, inside = rr.ground_height(P, mpf(-2.7), mpf(1.1), mpf(1))          # the yawed box's flat top at 0.1 + 0.3
    assert abs(z - mpf("0.4")) < 1e-16 and name == "box" and not inside
    z, name, inside = rr.ground_height(P, mpf(-2.0), mpf(0.5), mpf("0.3"))      # from inside it: the floor is nearer than its bottom face
    assert name == "floor"
    z, name, inside = rr.ground_height(P, mpf(6), mpf(6), mpf(1))
    assert abs(z - mpf("0.5")) < 1e-40 and name == "hill"
    z, name, inside = rr.ground_height(P, mpf("3.13"), mpf("2.5"), mpf(1))      # the ramp's top face over its centre: c_z + 0.5 / cos(0.2)
    assert abs(z - (mpf("-0.18") + mpf("0.5") / M.cos(mpf("0.2")))) < 1e-15 and name == "ramp"
    zl = rr.ground_height(P, mpf("2.63"), mpf("2.5"), mpf(1))[0]                # ... rising with x: euler 0 -0.2 0 tips the +x end up
    assert abs((z - zl) - mpf("0.5") * M.tan(mpf("0.2"))) < 1e-15


def test_literals_derived_by_hand():
    n = 0
    for c in rc.cases():
        for k, v in c.literal.items():
            assert abs(c.expected[k] - v) <= rc.LITERAL_TOL, (c.name, k, c.expected[k], v)
            n += 1
    assert n > 80


def test_branch_census_is_complete():
    assert rc.census() == rc.BRANCHES, (sorted(rc.BRANCHES - rc.census()), sorted(rc.census() - rc.BRANCHES))


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_a_wrong_reading_misses_the_cases(mutation):
    """every named wrong reading of the reference moves some expected entry by more than 1e3 x the fp64 bound: the cases can fail"""
    worst, where = 0.0, ""
    for c in rc.cases():
        if c.task != ("HumanoidTrack" if mutation in ("k1_unclamped", "velocity_without_omega_cross_r") else "QuadrupedFlat"):
            continue
        e, _, _ = rc.evaluate(c, mutation=mutation)
        d = float(np.max(rel(e, c.expected)))
        if d > worst:
            worst, where = d, c.name
    print(f"{mutation}: moves {where} by {worst:.2e}")
    assert worst > 1e3 * rc.FP64_BOUND


def test_float32_sensitivity_of_the_cases():
    s = rc.sensitivities()
    worst = max(s, key=s.get)
    print(f"largest change of an expected entry under a one-ulp float32 move of one input: {s[worst]:.2e} ({worst}); excluded from fp32 rows: "
          f"{sorted(rc.fp32_excluded())}")
    assert rc.fp32_excluded() == rc.FP32_EXCLUDED
    for task in ("QuadrupedFlat", "HumanoidTrack", "Cartpole", "Particle", "ParticleCopy"):
        names = [c.name for c in rc.cases(task) if not c.fp64_only]
        assert 10 * len(rc.fp32_excluded() & set(names)) <= len(names), task
    assert 10 * sum(c.fp64_only for c in rc.cases("QuadrupedFlat")) <= 2 * len(rc.cases("QuadrupedFlat"))   # (the boundary instants: fp64 rows only)


# ------------------------------------------------------------------------------------------------ the CPU copies
def test_the_oracle():
    rows, ph = [], {}
    for c in rc.cases():
        t = rc.task_of(c.task)
        if c.task not in ph:
            ph[c.task] = pyoracle.Physics(t.packed_model())
        nq = t.model.nq
        ph[c.task].set_state(c.state[:nq], c.state[nq:], c.time, c.mocap)
        ph[c.task].set_ctrl(clamped(c))
        rows.append((float(np.max(rel(ph[c.task].forward_task(packed(c)), c.expected))), c.name))
    report("oracle", rows, rc.FP64_BOUND)


def test_the_quad_step_function():
    import quademu
    rows = []
    pm = rc.task_of("QuadrupedFlat").packed_model()
    for c in rc.cases("QuadrupedFlat"):
        out = quademu.forward(pm, packed(c), c.state, c.time, c.mocap, clamped(c))
        rows.append((float(np.max(rel(out["residual"], c.expected))), c.name))
    report("quademu", rows, rc.FP64_BOUND)


@pytest.mark.parametrize("precision", [64, 32])
def test_the_limb_step_function(precision):
    import limbemu
    rows = []
    pm = rc.task_of("HumanoidTrack").packed_model()
    for c in rc.cases("HumanoidTrack"):
        out = limbemu.forward(pm, packed(c), c.state, c.time, c.mocap, clamped(c), precision=precision)
        e = c.expected if precision == 64 else c.expected32
        rows.append((float(np.max(rel(out["residual"], e))), c.name))
    report(f"limbemu fp{precision}", rows, rc.FP64_BOUND if precision == 64 else rc.STEP_GOAL)


@pytest.mark.parametrize("integrator", [0, 1])
def test_the_oracle_trace_is_the_framepos_sensor_of_the_step(integrator):
    """Trajectory::Rollout records the trace from the framepos sensors (GetTraces), which mj_step evaluates once, at the state the step starts
    from; the three further stages of mj_RungeKutta run no sensor stage. So trace[t] is the head site at states[t] under Euler and RK4 alike
    (the RK4 rollouts recorded the last stage's site position before)"""
    t = rc.task_of("QuadrupedFlat")
    pm = t.packed_model()
    pm.struct.integrator = integrator
    rows = []
    for c in rc.cases("QuadrupedFlat"):
        if not c.name.startswith(("quadruped/", "walk/", "flip/delta")):
            continue
        out = pyoracle.rollout_batch(pm, packed(c), c.state, c.time, c.mocap, 1, 2, 1, 0, np.array([c.time]), clamped(c)[None, None, :])
        rows.append((float(np.max(rel(out["trace"][0, 0], c.head))), c.name))
        rows.append((float(np.max(rel(out["residual"][0, 0], c.expected))), c.name))
    report(f"oracle rollout, integrator {integrator}", rows, rc.FP64_BOUND)
