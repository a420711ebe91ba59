"""An independent reference for the task residuals (test infrastructure, CPU only; not a conftest).

Nothing here shares arithmetic with the kernels, the oracle or the emulators:
- forward kinematics composes homogeneous transforms [R p; 0 1] down the body tree from the model's arrays (free, ball, hinge and slide
  joints; the inertial frame is the body's times body_iquat);
- velocities are central differences of POSITIONS along q(eps) = q (+) eps v, eps = 1e-15 in 50-digit arithmetic (no spatial algebra, no cvel);
- the ground under a point is the closed-form height of each group-0 geom on the vertical line through it: the plane's equation, the
  sphere's z_c +- sqrt(r^2 - dx^2 - dy^2), and for a box the six face planes cut by the line, kept where the cut lies on the face;
- the residual entries are written from the meaning of each entry and the design constants of the tasks (heights 0.25 / 0.6 / 0.15 / 0.5 /
  0.8, foot radius 0.02, the gait phase table, posture gains 2 1 1; 30 fps, 16 bodies, interpolation clamped to the clip), feet, joints,
  sites and parameters resolved BY NAME, not through the frozen index tables the kernels read.

The functions are generic over a number backend: MP (mpmath, 50 digits; every expected value) and FL (Python floats; only the one-ulp
sensitivity scan of residual_cases.py, where eight digits are plenty). `mutation=` runs a named wrong reading (MUTATIONS), so that the
suite can prove its cases tell the readings apart."""
from __future__ import annotations

import math

import mpmath

_M = mpmath.mp.clone()
_M.dps = 50


class _Backend:
    def __init__(self, num, sqrt, cos, sin, atan2, floor, pi, eps):
        self.num, self.sqrt, self.cos, self.sin, self.atan2, self.floor, self.pi, self.eps = num, sqrt, cos, sin, atan2, floor, pi, eps

    def vec(self, x):
        return [self.num(v) for v in x]


MP = _Backend(lambda x: x if isinstance(x, _M.mpf) else _M.mpf(float(x)), _M.sqrt, _M.cos, _M.sin, _M.atan2, _M.floor, +_M.pi, _M.mpf(10) ** -15)
FL = _Backend(float, math.sqrt, math.cos, math.sin, math.atan2, math.floor, math.pi, 1e-6)

MUTATIONS = ("foot_permutation", "walk_phase_shift", "flip_direction", "handstand_sign", "height_swap", "box_world_frame", "k1_unclamped",
             "velocity_without_omega_cross_r")
MINVAL = 1e-15                                             # below this length a vector is left unnormalised (or replaced by the x axis)
JOINT_TYPES = {"free": 0, "ball": 1, "slide": 2, "hinge": 3}
GEOM_PLANE, GEOM_SPHERE, GEOM_BOX = 0, 2, 6


# ------------------------------------------------------------------------------------------------ quaternions and transforms
def q_mul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def q_conj(a):
    return [a[0], -a[1], -a[2], -a[3]]


def q_unit(B, q):
    n = B.sqrt(sum(v * v for v in q))
    return [v / n for v in q]


def q_rotvec(B, r):
    """exp(r / 2): the rotation by |r| about r / |r|"""
    t = B.sqrt(sum(v * v for v in r))
    if t == 0:
        return [B.num(1), B.num(0), B.num(0), B.num(0)]
    s = B.sin(t / 2) / t
    return [B.cos(t / 2), r[0] * s, r[1] * s, r[2] * s]


def q_matrix(q):
    w, x, y, z = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def transform(R, p):
    return [R[0] + [p[0]], R[1] + [p[1]], R[2] + [p[2]], [0, 0, 0, 1]]


def t_mul(A, Bm):
    """the product of two transforms [R p; 0 1]: the last rows are 0 0 0 1, so their terms are left out (the same numbers, bit for bit)"""
    out = [[A[i][0] * Bm[0][j] + A[i][1] * Bm[1][j] + A[i][2] * Bm[2][j] for j in range(4)] for i in range(3)]
    for i in range(3):
        out[i][3] = out[i][3] + A[i][3]
    return out + [[0, 0, 0, 1]]


def t_point(T, p):
    return [T[i][0] * p[0] + T[i][1] * p[1] + T[i][2] * p[2] + T[i][3] for i in range(3)]


def t_rot(T):
    return [T[i][:3] for i in range(3)]


def t_pos(T):
    return [T[i][3] for i in range(3)]


def pose(B, pos, quat):
    return transform(q_matrix(q_unit(B, quat)), list(pos))


# ------------------------------------------------------------------------------------------------ kinematics
class Kinematics:
    """forward kinematics of a model (mjcf.FlatModel) by homogeneous transforms; geoms and sites on demand"""

    def __init__(self, model, B=MP):
        self.m, self.B, a = model, B, model.arrays
        self.nbody = int(model.nbody)
        self.parent = [int(v) for v in a["body_parentid"]]
        self.mocapid = [int(v) for v in a["body_mocapid"]]
        self.jntadr, self.jntnum = [int(v) for v in a["body_jntadr"]], [int(v) for v in a["body_jntnum"]]
        self.jnt_type = [int(v) for v in a["jnt_type"]]
        self.qadr, self.dadr = [int(v) for v in a["jnt_qposadr"]], [int(v) for v in a["jnt_dofadr"]]
        for t in self.jnt_type:
            if t not in JOINT_TYPES.values():
                raise NotImplementedError(f"joint type {t}: the reference kinematics knows free, ball, hinge and slide joints")
        self.body_T = [pose(B, B.vec(a["body_pos"][b]), B.vec(a["body_quat"][b])) for b in range(self.nbody)]
        self.body_q = [q_unit(B, B.vec(a["body_quat"][b])) for b in range(self.nbody)]
        self.ipos = [B.vec(v) for v in a["body_ipos"]]
        self.iquat = [q_unit(B, B.vec(v)) for v in a["body_iquat"]]
        self.mass = B.vec(a["body_mass"])
        self.jnt_pos, self.jnt_axis = [B.vec(v) for v in a["jnt_pos"]], [B.vec(v) for v in a["jnt_axis"]]
        self.qpos0 = B.vec(a["qpos0"])
        # per joint, what no qpos changes: the unit axis and the transforms to the anchor and back
        one = q_matrix(B.vec([1, 0, 0, 0]))
        self.axis_unit = [[v / B.sqrt(sum(w * w for w in ax)) for v in ax] if any(ax) else ax for ax in self.jnt_axis]
        self.to_anchor = [transform(one, p) for p in self.jnt_pos]
        self.from_anchor = [transform(one, [-v for v in p]) for p in self.jnt_pos]
        self.one = one

    def name(self, kind, name):
        return self.m.names[kind].index(name)

    def forward(self, qpos, mocap=None, upto=None):
        """the pose of every body (of bodies 0 .. upto - 1: enough where only a leading part of the tree is asked for)"""
        B = self.B
        q = B.vec(qpos)
        ident = transform(q_matrix(B.vec([1, 0, 0, 0])), B.vec([0, 0, 0]))
        T, Q = [ident], [B.vec([1, 0, 0, 0])]
        for b in range(1, self.nbody if upto is None else upto):
            Tb, Qb = self.body_pose(b, T[self.parent[b]], Q[self.parent[b]], q, mocap)
            T.append(Tb)
            Q.append(Qb)
        return Pose(self, T, Q)

    def body_pose(self, b, T_parent, Q_parent, q, mocap=None):
        """(transform, quaternion) of body b given its parent's, q a backend vector"""
        B = self.B
        if self.mocapid[b] >= 0 and mocap is not None:
            mc = B.vec(mocap[7 * self.mocapid[b]:7 * self.mocapid[b] + 7])
            Tb, Qb = pose(B, mc[:3], mc[3:]), q_unit(B, mc[3:])
        else:
            Tb, Qb = t_mul(T_parent, self.body_T[b]), q_mul(Q_parent, self.body_q[b])
        for j in range(self.jntadr[b], self.jntadr[b] + self.jntnum[b]):
            adr = self.qadr[j]
            if self.jnt_type[j] == JOINT_TYPES["free"]:
                Qb = q_unit(B, q[adr + 3:adr + 7])
                Tb = transform(q_matrix(Qb), q[adr:adr + 3])
            elif self.jnt_type[j] == JOINT_TYPES["ball"]:
                qj = q_unit(B, q[adr:adr + 4])               # the turn about the anchor, in the body's frame (qpos0's turn is in body_quat)
                Tb = t_mul(t_mul(t_mul(Tb, self.to_anchor[j]), transform(q_matrix(qj), B.vec([0, 0, 0]))), self.from_anchor[j])
                Qb = q_mul(Qb, qj)
            elif self.jnt_type[j] == JOINT_TYPES["slide"]:
                Tb = t_mul(Tb, transform(self.one, [v * (q[adr] - self.qpos0[adr]) for v in self.axis_unit[j]]))
            else:
                qj = q_rotvec(B, [v * (q[adr] - self.qpos0[adr]) for v in self.axis_unit[j]])
                Tb = t_mul(t_mul(t_mul(Tb, self.to_anchor[j]), transform(q_matrix(qj), B.vec([0, 0, 0]))), self.from_anchor[j])
                Qb = q_mul(Qb, qj)
        return Tb, Qb

    def displaced(self, qpos, qvel, eps):
        """q (+) eps v: a free joint moves by eps v_lin in the world and turns by eps omega in its own frame, a ball joint turns by eps omega
        in its own frame, a hinge or a slide moves by eps v"""
        B = self.B
        q, v = B.vec(qpos), B.vec(qvel)
        for j, t in enumerate(self.jnt_type):
            qa, da = self.qadr[j], self.dadr[j]
            if t == JOINT_TYPES["free"]:
                for k in range(3):
                    q[qa + k] = q[qa + k] + eps * v[da + k]
                q[qa + 3:qa + 7] = q_mul(q_unit(B, q[qa + 3:qa + 7]), q_rotvec(B, [eps * v[da + 3 + k] for k in range(3)]))
            elif t == JOINT_TYPES["ball"]:
                q[qa:qa + 4] = q_mul(q_unit(B, q[qa:qa + 4]), q_rotvec(B, [eps * v[da + k] for k in range(3)]))
            else:
                q[qa] = q[qa] + eps * v[da]
        return q

    def velocity(self, qpos, qvel, mocap, fn):
        """d/dt of fn(pose) (a list of numbers) by a central difference of positions"""
        e = self.B.eps
        hi, lo = fn(self.forward(self.displaced(qpos, qvel, e), mocap)), fn(self.forward(self.displaced(qpos, qvel, -e), mocap))
        return [(a - b) / (2 * e) for a, b in zip(hi, lo)]


class Pose:
    def __init__(self, kin, T, Q):
        self.kin, self.T, self.xquat = kin, T, Q

    def xpos(self, b):
        return t_pos(self.T[b])

    def xmat(self, b):
        return t_rot(self.T[b])

    def xipos(self, b):
        return t_point(self.T[b], self.kin.ipos[b])

    def ximat(self, b):
        """the inertial frame's rotation: the body's frame times body_iquat"""
        R, Ri = t_rot(self.T[b]), q_matrix(self.kin.iquat[b])
        return [[sum(R[i][k] * Ri[k][j] for k in range(3)) for j in range(3)] for i in range(3)]

    def site_xpos(self, s):
        a = self.kin.m.arrays
        return t_point(self.T[int(a["site_bodyid"][s])], self.kin.B.vec(a["site_pos"][s]))

    def geom_T(self, g):
        a, B = self.kin.m.arrays, self.kin.B
        return t_mul(self.T[int(a["geom_bodyid"][g])], pose(B, B.vec(a["geom_pos"][g]), B.vec(a["geom_quat"][g])))

    def geom_xpos(self, g):
        return t_pos(self.geom_T(g))

    def subtree(self, root):
        out = []
        for b in range(self.kin.nbody):
            p = b
            while p != root and p > 0:
                p = self.kin.parent[p]
            if p == root:
                out.append(b)
        return out

    def subtree_com(self, root):
        bodies = self.subtree(root)
        total = sum(self.kin.mass[b] for b in bodies)
        return [sum(self.kin.mass[b] * self.xipos(b)[k] for b in bodies) / total for k in range(3)]


# ------------------------------------------------------------------------------------------------ ground
def ground_height(pose_, x, y, zq, mutation=None):
    """the first surface a ray from (x, y, zq) straight down meets among the group-0 planes, spheres and boxes, the far side of a solid the
    point is inside included: (z, geom name, inside a solid)"""
    kin = pose_.kin
    a, B = kin.m.arrays, kin.B
    best = None
    for g in range(len(a["geom_type"])):
        if int(a["geom_group"][g]) != 0:
            continue
        gt, size = int(a["geom_type"][g]), B.vec(a["geom_size"][g])
        T = pose_.geom_T(g)
        c, R = t_pos(T), t_rot(T)
        inside = False
        if gt == GEOM_PLANE:
            n = [R[0][2], R[1][2], R[2][2]]
            z = c[2] - (n[0] * (x - c[0]) + n[1] * (y - c[1])) / n[2]
            if zq < z:
                continue
        elif gt == GEOM_SPHERE:
            h2 = size[0] * size[0] - (x - c[0]) ** 2 - (y - c[1]) ** 2
            if h2 < 0:
                continue
            top, bottom = c[2] + B.sqrt(h2), c[2] - B.sqrt(h2)
            if zq >= top:
                z = top
            elif zq > bottom:
                z, inside = bottom, True
            else:
                continue
        elif gt == GEOM_BOX:
            if mutation == "box_world_frame":
                R = [[B.num(int(i == j)) for j in range(3)] for i in range(3)]
            cuts = []
            for k in range(3):
                for sign in (-1, 1):
                    n = [sign * R[i][k] for i in range(3)]
                    if n[2] == 0:
                        continue
                    f = [c[i] + sign * size[k] * R[i][k] for i in range(3)]
                    z = f[2] - (n[0] * (x - f[0]) + n[1] * (y - f[1])) / n[2]
                    rel = [x - c[0], y - c[1], z - c[2]]
                    local = [sum(R[i][j] * rel[i] for i in range(3)) for j in range(3)]
                    if all(abs(local[j]) <= size[j] for j in range(3) if j != k):
                        cuts.append(z)
            if not cuts:
                continue
            top, bottom = max(cuts), min(cuts)
            if zq >= top:
                z = top
            elif zq > bottom:
                z, inside = bottom, True
            else:
                continue
        else:
            continue
        if best is None or z > best[0]:
            best = (z, kin.m.names["geom"][g], inside)
    if best is None:
        raise ValueError("no ground under the query point")
    return best


# ------------------------------------------------------------------------------------------------ QuadrupedFlat
MODES = ("Quadruped", "Biped", "Walk", "Scramble", "Flip")
GAITS = ("Stand", "Walk", "Trot", "Canter", "Gallop")
GAIT_PHASE = {"Stand": {"FL": 0, "HL": 0, "FR": 0, "HR": 0}, "Walk": {"FL": 0, "HL": 0.75, "FR": 0.5, "HR": 0.25},
              "Trot": {"FL": 0, "HL": 0.5, "FR": 0.5, "HR": 0}, "Canter": {"FL": 0, "HL": 0.33, "FR": 0.33, "HR": 0.66},
              "Gallop": {"FL": 0, "HL": 0.4, "FR": 0.05, "HR": 0.35}}
FEET = ("FL", "HL", "FR", "HR")                      # the order of the four Gait entries
H_QUADRUPED, H_BIPED, H_CROUCH, H_LEAP, H_MAX, FOOT_RADIUS, G = 0.25, 0.6, 0.15, 0.5, 0.8, 0.02, 9.81
POSTURE_GAIN = {"hip": 2, "thigh": 1, "calf": 1}
MIN_ANGVEL, LOOK_AHEAD = 0.01, 0.15


def flip_profile(B):
    """the flip's design: constant acceleration from rest at 0.25 down to 0.15 and up to 0.5 (leaving the ground at the speed that peaks at
    0.8), a ballistic flight, a constant deceleration back to 0.25; the turn is 0 through the crouch, pi/2 at take-off, 1.25 pi more at a
    constant rate in flight, 2 pi at the end of the landing. Returns the instants and (height(t), angle(t)) given the phase of t."""
    n = B.num
    g = n(G)
    v_jump = B.sqrt(2 * g * (n(H_MAX) - n(H_LEAP)))
    flight = 2 * v_jump / g
    acc = v_jump ** 2 / (2 * (n(H_LEAP) - n(H_CROUCH)))
    crouch = B.sqrt(2 * (n(H_QUADRUPED) - n(H_CROUCH)) / acc)
    leap = v_jump / acc
    land = 2 * (n(H_LEAP) - n(H_QUADRUPED)) / v_jump
    w_flight = n(1.25) * B.pi / flight
    w_jump = B.pi / leap - w_flight                      # mean rate pi/2 / leap, ending at the flight's rate
    return dict(crouch=crouch, jump=crouch + leap, flight=flight, land=land, v_jump=v_jump, acc=acc, leap=leap, w_flight=w_flight, w_jump=w_jump)


def flip_target(B, t, thresholds):
    """(phase, target height above `ground`, target angle) at flip time t. The phase is decided against the kernel's own double thresholds
    (crouch_time, jump_time, jump_time + flight_time, ... + land_time) so that a boundary instant falls on the same side; the values inside a
    phase come from the design alone."""
    n, P = B.num, flip_profile(B)
    t_crouch, t_jump, t_land, t_end = (n(v) for v in thresholds)
    if t >= t_end:
        return "after", n(H_QUADRUPED), 2 * B.pi
    if t < t_jump:
        h = n(H_QUADRUPED) - P["acc"] * P["crouch"] * t + P["acc"] * t * t / 2
        if t < t_crouch:
            return "crouch", h, n(0)
        s = t - P["crouch"]
        return "leap", h, P["w_jump"] * s + (P["w_flight"] - P["w_jump"]) / P["leap"] * s * s / 2
    if t < t_land:
        s = t - P["jump"]
        return "flight", n(H_LEAP) + P["v_jump"] * s - n(G) * s * s / 2, B.pi / 2 + P["w_flight"] * s
    s = t - P["jump"] - P["flight"]
    dec = P["v_jump"] / P["land"]
    rot_dec = 2 * (P["w_flight"] * P["land"] - B.pi / 4) / P["land"] ** 2
    return "land", n(H_LEAP) - P["v_jump"] * s + dec * s * s / 2, n(1.75) * B.pi + P["w_flight"] * s - rot_dec * s * s / 2


def c_fmod(B, x, y):
    """C's fmod: the remainder with the sign of x"""
    r = abs(x) - B.floor(abs(x) / y) * y
    return r if x >= 0 else -r


def step_height(B, phase, foot_phase, duty, labels):
    angle = c_fmod(B, phase + B.pi - foot_phase, 2 * B.pi) - B.pi
    if phase + B.pi - foot_phase < 0:
        labels.add("gait:negative-fmod")
    if duty >= 1:
        labels.add("step-zero:duty")
        return B.num(0)
    angle = angle * B.num(0.5) / (1 - duty)
    angle = max(min(angle, B.pi / 2), -B.pi / 2)
    value = B.cos(angle)
    if abs(value) < 1e-6:
        labels.add("step-zero:cos")
        return B.num(0)
    return value


def rotation_between(B, qa, qb, labels):
    """the rotation vector r, in qb's frame, with qb (x) exp(r / 2) = qa, its angle wrapped into (-pi, pi]"""
    d = q_mul(q_conj(qb), qa)
    s = B.sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3])
    axis = d[1:]
    if s > MINVAL:
        axis = [v / s for v in axis]
    angle = 2 * B.atan2(s, d[0])
    if angle > B.pi:
        angle = angle - 2 * B.pi
        labels.add("sub-quat:wrap")
    elif s > MINVAL:
        labels.add("sub-quat:normal")
    else:
        labels.add("sub-quat:small")
    return [v * angle for v in axis]


def unit2(B, v, fallback=(1, 0)):
    n = B.sqrt(v[0] * v[0] + v[1] * v[1])
    if n < MINVAL:
        return [B.num(fallback[0]), B.num(fallback[1])], True
    return [v[0] / n, v[1] / n], False


def quadruped_residual(kin, qpos, qvel, time, mocap, ctrl, frozen, params, mutation=None):
    """the 42 entries of the QuadrupedFlat residual and the set of branch labels taken.
    frozen: mode, gait, flip_dir (0 back, 1 front), handstand, mode_start_time, position[2], heading[2], speed, angvel, ground,
    orientation[4], phase_start, phase_start_time, phase_velocity, flip_thresholds[4]; params: {numeric name: value}"""
    B, n, m, a = kin.B, kin.B.num, kin.m, kin.m.arrays
    labels = set()
    mode, gait = MODES[frozen["mode"]], GAITS[frozen["gait"]]
    handstand = bool(frozen["handstand"])
    P = kin.forward(qpos, mocap)
    trunk, head = kin.name("body", "trunk"), kin.name("site", "head")
    goal = B.vec(mocap[7 * int(a["body_mocapid"][kin.name("body", "goal")]):][:3])
    names = {"FL": "FL", "HL": "HL", "FR": "FR", "HR": "HR"}
    if mutation == "foot_permutation":
        names.update(FL="FR", FR="FL")
    foot = {f: P.geom_xpos(kin.name("geom", names[f])) for f in FEET}
    if mode == "Biped":
        labels.add("biped:hand-stand" if handstand else "biped:foot-stand")
        support = ("FL", "FR") if handstand else ("HL", "HR")
    else:
        support = FEET
    mean_foot = [sum(foot[f][k] for f in support) / len(support) for k in range(3)]
    R, com_z = P.xmat(trunk), P.xipos(trunk)[2]
    t_mode = n(time) - n(frozen["mode_start_time"])
    r = []
    # Upright(3)
    if mode == "Flip":
        flip_phase, h_target, angle = flip_target(B, t_mode, frozen["flip_thresholds"])
        labels.add("flip:" + flip_phase)
        sign = 1 if frozen["flip_dir"] else -1
        if mutation == "flip_direction":
            sign = -sign
        target = q_mul(B.vec(frozen["orientation"]), q_rotvec(B, [n(0), sign * angle, n(0)]))
        r += rotation_between(B, P.xquat[trunk], target, labels)
    elif mode == "Biped":
        up = -1 if handstand else 1                      # the trunk's x axis points down in a hand stand, up in a foot stand
        if mutation == "handstand_sign":
            up = -up
        r += [R[2][0] - up, n(0), n(0)]
    else:
        r += [R[2][2] - 1, n(0), n(0)]
    # Height
    h_goal = n(H_BIPED if mode == "Biped" else H_QUADRUPED)
    if mutation == "height_swap":
        h_goal = n(H_QUADRUPED if mode == "Biped" else H_BIPED)
    if mode == "Scramble":
        r.append(n(0))
    elif mode == "Flip":
        r.append(com_z - (h_target + n(frozen["ground"])))
    else:
        r.append(com_z - mean_foot[2] - h_goal)
    # Position(3)
    hd = P.site_xpos(head)
    if mode == "Walk":
        pos, heading, speed, angvel = B.vec(frozen["position"]), B.vec(frozen["heading"]), n(frozen["speed"]), n(frozen["angvel"])
        if abs(angvel) < MIN_ANGVEL:
            fwd, fell_back = unit2(B, heading)
            labels.add("walk:zero-heading" if fell_back else "walk:straight")
            target = [pos[k] + heading[k] + t_mode * speed * fwd[k] for k in range(2)]
        else:
            labels.add("walk:threshold" if abs(angvel) == MIN_ANGVEL else "walk:circle")
            c, s = B.cos(t_mode * angvel), B.sin(t_mode * angvel)
            target = [pos[0] + c * heading[0] - s * heading[1], pos[1] + s * heading[0] + c * heading[1]]
        r += [hd[0] - target[0], hd[1] - target[1], n(0)]
    else:
        r += [hd[0] - goal[0], hd[1] - goal[1], 2 * (hd[2] - goal[2]) if mode == "Scramble" else n(0)]
    # Gait(4)
    table = dict(GAIT_PHASE["Trot" if mode == "Biped" else gait])
    if mutation == "walk_phase_shift" and gait == "Walk" and mode != "Biped":
        row = [table[f] for f in FEET]
        table = dict(zip(FEET, row[1:] + row[:1]))
    phase = n(frozen["phase_start"]) + (n(time) - n(frozen["phase_start_time"])) * n(frozen["phase_velocity"])
    amplitude, duty = n(params["residual_Amplitude"]), n(params["residual_Duty ratio"])
    for f in FEET:
        step = amplitude * step_height(B, phase, 2 * B.pi * n(table[f]), duty, labels)
        if mode == "Biped" and f not in support:
            r.append(n(0))
            continue
        q = list(foot[f])
        if mode == "Scramble":
            d, _ = unit2(B, [goal[0] - q[0], goal[1] - q[1]])
            q[0], q[1] = q[0] + n(LOOK_AHEAD) * d[0], q[1] + n(LOOK_AHEAD) * d[1]
        z, hit, inside = ground_height(P, q[0], q[1], q[2] + n(0.5), mutation)
        labels.add("terrain:inside-" + hit if inside else "terrain:" + hit)
        if mode == "Scramble" and ground_height(P, foot[f][0], foot[f][1], foot[f][2] + n(0.5), mutation)[1] != hit:
            labels.add("terrain:look-ahead")
        diff = foot[f][2] - (z + n(FOOT_RADIUS) + step)
        if mode == "Scramble":
            diff = min(diff, n(0))
        if step == 0:
            if amplitude == 0:
                labels.add("step-zero:amplitude")
            diff = n(0)
        r.append(diff)
    # Balance(2): the capture point over the mean supporting foot; Angmom(3) is declared as the same subtree velocity
    com = P.subtree_com(trunk)
    comvel = kin.velocity(qpos, qvel, mocap, lambda p: p.subtree_com(trunk))
    fall = B.sqrt(2 * h_goal / n(G))
    r += [com[k] + comvel[k] * fall - mean_foot[k] for k in range(2)]
    # Effort(12): 0.02 x the actuator force, a gain of 40 on the clamped control
    lo, hi = a["actuator_ctrlrange"][:, 0], a["actuator_ctrlrange"][:, 1]
    r += [n(0.02) * n(a["actuator_gainprm"][i][0]) * max(min(n(ctrl[i]), n(hi[i])), n(lo[i])) for i in range(m.nu)]
    # Posture(12): joint angles against a keyframe, in actuator order, weighted by the joint's kind
    key = "home"
    if mode == "Flip":
        key = {"crouch": "crouch", "leap": None, "flight": None, "land": "home", "after": "home"}[flip_phase]
    arm = ("FR", "FL") if not handstand else ("RR", "RL")
    for i in range(m.nu):
        j = int(a["actuator_trnid"][i]) if a["actuator_trnid"].ndim == 1 else int(a["actuator_trnid"][i][0])
        jname = m.names["joint"][j]
        leg, kind = jname.split("_")[0], jname.split("_")[1]
        adr = kin.qadr[j]
        v = n(0) if key is None else (n(qpos[adr]) - n(a["key_qpos"][kin.name("key", key)][adr])) * POSTURE_GAIN[kind]
        if mode == "Biped" and leg in arm:
            v = v * n(params["residual_Arm posture"])
        r.append(v)
    # Yaw(2)
    if mode == "Biped":
        s = 1 if handstand else -1                       # the belly side faces forward in a foot stand, the back in a hand stand
        if mutation == "handstand_sign":
            s = -s
        th, _ = unit2(B, [s * R[0][2], s * R[1][2]])
    else:
        th, _ = unit2(B, [R[0][0], R[1][0]])
    hg = n(params["residual_Heading"])
    r += [th[0] - B.cos(hg), th[1] - B.sin(hg)]
    r += comvel
    return r, labels, dict(head=hd)


# ------------------------------------------------------------------------------------------------ HumanoidTrack
FPS = 30
TRACKED = ("pelvis", "head", "ltoe", "rtoe", "lheel", "rheel", "lknee", "rknee", "lhand", "rhand", "lelbow", "relbow", "lshoulder",
           "rshoulder", "lhip", "rhip")


def humanoid_residual(kin, qpos, qvel, time, ctrl, first_key, last_key, reference_time, mutation=None):
    """joint velocities, clamped controls, mean marker minus mean site, the 16 centred differences, the 16 marker-minus-site velocities"""
    B, n, m, a = kin.B, kin.B.num, kin.m, kin.m.arrays
    labels = set()
    index = (n(time) - n(reference_time)) * FPS + first_key
    if index < first_key:
        labels.add("humanoid:before")      # (before the clip the index runs into the previous clip's keys, or clamps at 0)
    if index > last_key:
        labels.add("humanoid:beyond")
    c = max(min(index, n(last_key)), n(0))
    k0 = int(B.floor(c))
    k1 = min(k0 + 1, len(a["key_mpos"]) - 1) if mutation == "k1_unclamped" else min(k0 + 1, last_key)
    if k0 == last_key:
        labels.add("humanoid:last-key")
    elif first_key <= index <= last_key:
        labels.add("humanoid:interior")
    w1 = c - k0
    mp_ = a["key_mpos"]
    mid = [int(a["body_mocapid"][kin.name("body", f"mocap[{b}]")]) for b in TRACKED]
    sid = [kin.name("site", f"tracking[{b}]") for b in TRACKED]
    key = lambda k, i: B.vec(mp_[k][3 * i:3 * i + 3])
    marker = [[key(k0, i)[d] * (1 - w1) + key(k1, i)[d] * w1 for d in range(3)] for i in mid]
    P = kin.forward(qpos, None)
    site = [P.site_xpos(s) for s in sid]
    mean_m = [sum(p[d] for p in marker) / 16 for d in range(3)]
    mean_s = [sum(p[d] for p in site) / 16 for d in range(3)]
    r = [n(v) for v in qvel[6:]]
    lo, hi, lim = a["actuator_ctrlrange"][:, 0], a["actuator_ctrlrange"][:, 1], a["actuator_ctrllimited"]
    r += [max(min(n(ctrl[i]), n(hi[i])), n(lo[i])) if lim[i] else n(ctrl[i]) for i in range(m.nu)]
    r += [mean_m[d] - mean_s[d] for d in range(3)]
    for pm_, ps in zip(marker, site):
        r += [(pm_[d] - mean_m[d]) - (ps[d] - mean_s[d]) for d in range(3)]
    if mutation == "velocity_without_omega_cross_r":
        bodies = [int(a["site_bodyid"][s]) for s in sid]
        vel = kin.velocity(qpos, qvel, None, lambda p: [x for b in bodies for x in p.xpos(b)])
    else:
        vel = kin.velocity(qpos, qvel, None, lambda p: [x for s in sid for x in p.site_xpos(s)])
    for j, i in enumerate(mid):
        r += [(key(k1, i)[d] - key(k0, i)[d]) * FPS - vel[3 * j + d] for d in range(3)]
    return r, labels, {}


# ------------------------------------------------------------------------------------------------ the lane tasks
def cartpole_residual(B, qpos, qvel, ctrl, goal, ctrl_range):
    """cos(theta) - 1 (as -2 sin^2(theta / 2), which keeps its digits near theta = 0), cart position minus the goal, pole velocity, control"""
    n = B.num
    u = max(min(n(ctrl[0]), n(ctrl_range[1])), n(ctrl_range[0]))
    return [-2 * B.sin(n(qpos[1]) / 2) ** 2, n(qpos[0]) - n(goal), n(qvel[1]), u]


def particle_residual(B, qpos, qvel, goal_xy=None):
    """position (minus the goal's, for Particle) and velocity"""
    n = B.num
    g = [0, 0] if goal_xy is None else goal_xy
    return [n(qpos[0]) - n(g[0]), n(qpos[1]) - n(g[1]), n(qvel[0]), n(qvel[1])]
