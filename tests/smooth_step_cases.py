"""Smooth-step harness (test infrastructure, like force_noise_cases.py; not a conftest, no GPU code of its own): an independent 50-digit
reference of the CONSTRAINT-FREE step of every covered model, the cases the oracle, both emulators and every rollout kernel are held to it
at, the wrong readings the cases must tell apart, and the bounds.

THE REFERENCE imports nothing from oracle/, csrc/, the emulators or mjcf.mass_matrix: it reads the model's arrays and differentiates the
POSITIONS of residual_reference.Kinematics (homogeneous transforms, mpmath, 50 digits). It is written from d'Alembert's principle. Along
the path q(s) = q (+) s v (Kinematics.displaced) the generalized acceleration is zero in the velocity coordinates of the model, so the
force the path itself asks for is the bias. Per body b: the centre of mass c_b, the inertial frame R_b (body frame times body_iquat), the
world inertia I_b = R_b diag(body_inertia) R_b^T.
  Jc_b, Jw_b  d c_b / d q_k and vee(dR_b/dq_k R_b^T): force_noise_cases.jacobians (central differences, step 1e-15)
  M           sum_b m_b Jc_b^T Jc_b + Jw_b^T I_b Jw_b + diag(dof_armature)
  bias        sum_b Jc_b^T m_b (c''_b - g) + Jw_b^T (I_b W'_b + W_b x I_b W_b); c'', W = vee(R' R^T), W' = vee of the skew part of
              R'' R^T are derivatives of the poses along the path by five-point stencils (step 1e-9: truncation 1e-36 |v|^6, rounding
              1e-32)
  passive     -D v - K (q - qpos_spring) on hinge and slide joints; no covered model has a tendon with stiffness or damping (asserted)
  actuators   joint transmission; ctrl clamped to ctrlrange where limited; force = gain ctrl + b0 + b1 gear q + b2 gear v (the bias terms
              under biastype affine only), clamped to forcerange where limited, times gear
  Euler       (M + h D) (v' - v) / h = tau_act + passive - bias, then q' = q (+) h v'
  RK4         the classical tableau on (q, v), (+) for the positions, no implicit damping
`mutation=` runs a named wrong reading (MUTATIONS). SHOWN lists per model the readings its arrays can show; every other is listed by name
in not_shown(), and tests/test_smooth_step_cases.py asserts both directions from the reference alone: a shown reading misses the fp64
bound by more than a factor of two on a compared entry of a case, a reading not shown moves nothing beyond it.

THE CASES. Models: force_noise_cases.model keys (probe, cartpole, particle, a1 -- friction loss and contacts disabled --, humanoid);
a1-floss (the A1 as registered: friction loss on, for the momentum-balance rows); tree (tests/models/smooth_tree.xml: a ball joint, springs
off qpos0, an affine actuator bias under a gear, a force range -- what no registered model's arrays can show); brick (tests/models/
free_body.xml, the self-checks and the oracle's RK4 only). Per robot and lane model N_STATES = 6 states of the step bank: the fastest by
|qvel|_inf, then every (n / 6)-th of the bank's ranking by speed; a robot's lifted by 1 m, limited joints clipped to the middle half of
their range, the recorded velocities kept. The probe and the tree: probe_state() / tree_state() and two more each. Per state the sixteen
controls of step_bank.step_controls (zero, both saturated ends, thirteen that reach past the ends): 6 x 16 = 96 candidates a robot and
lane model, 3 x 16 = 48 on the probe and on the tree.
CONDITIONS, asserted on every state that is used, where the cases are built (not measurements): every limited joint strictly inside its
range before and after the reference's step (Euler and RK4); every body's centre more than 0.5 m + a bounding radius above the floor;
the oracle reports nefc = 0 with the flags the row passes (a1-floss: friction-loss rows only). The states are taken in the order of the
ranking; one that fails a condition would be passed over and recorded in SKIPPED with the reason (the fastest must pass). NONE is: every
model's SKIPPED is empty, which tests/test_smooth_step_cases.py asserts. No state is dropped for missing a bound. Two readings of the
clearance, written down because the letter of it cannot hold: the radius is the largest among the geoms of moving bodies (0.23 m on the
Humanoid; the A1's scene has a static 6 m box, which nothing lifts a robot over and which comes down on nothing), and the clearance is
asked where a floor collides and contacts are enabled (the A1 under both sets of flags, the Humanoid): Cartpole and Particle run with
contacts disabled and the particle slides 1 cm above its plane by design; the probe, the tree and the brick have no floor.

BOUNDS. fp64: |d - r| <= 1e-9 (1 + |r|), the project's step tolerance, imported from test_gpu_step_parity.ROWS by the test modules; M:
1e-12 max|M| (tests/test_oracle_physics.py). fp32: the row's own bound in ROWS. Momentum balance (a1-floss): rho = (M + h D)(v' - v) / h
- (tau_act + passive - bias) from the device's v' and the reference's everything else; rho_k = 0 on the trunk, |rho_k| <=
dof_frictionloss_k on the joints, each within sum_j |M + h D|_kj tol (1 + |v'_j|) / h; q' against q (+) h v' of the device's own v'.

RK4 at 50 digits costs two further sets of Jacobians per CANDIDATE (stages 3 and 4 start from candidate-dependent positions; stages 1 and
2 share theirs among the candidates of a state). The tree, the brick, the cart-pole and the particle are held on every state and all
sixteen controls (3 + 1 + 6 + 6 states). The probe, the A1 and the Humanoid (0.5 / 0.9 / 1.8 s a candidate) on the fastest state and the
next of the ranking, under four controls each -- zero, both saturated ends, the first random one with an entry past an end (the probe's first state
has none: its first random one): 2 x 4 = 8
candidates a model (rk4_candidates). The device launches all sixteen controls and the four are compared. The whole Euler expectation of
all models builds in about 10 s, the RK4 one in about 35 s.

No product code imports this module."""
from __future__ import annotations

import dataclasses
import os

import numpy as np

import force_noise_cases as fn
import residual_reference as rr
import step_bank as sb

MPC = rr._M                    # the kinematics' own mpmath context: every number of the reference lives in it
mpf = MPC.mpf
STENCIL = mpf(10) ** -9
STEP_TOL64, M_ATOL = 1e-9, 1e-12          # (the test modules assert STEP_TOL64 against test_gpu_step_parity.ROWS)
N_STATES, N_PROBE_STATES, LIFT, CLEARANCE = 6, 3, 1.0, 0.5
FREE, BALL, SLIDE, HINGE = (rr.JOINT_TYPES[k] for k in ("free", "ball", "slide", "hinge"))
GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_ELLIPSOID, GEOM_CYLINDER, GEOM_BOX = 0, 2, 3, 4, 5, 6
EFC_FRICTION = sb.EFC_FRICTION

MUTATIONS = ("no_gyroscopic", "no_velocity_products", "ipos_ignored", "iquat_ignored", "gravity_at_body_origin", "armature_outside_damped_solve",
             "explicit_damping", "gear_not_squared_in_bias", "free_omega_in_world_frame", "spring_about_qpos0", "ctrl_unclamped",
             "position_from_old_velocity")
KEYS = ("probe", "tree", "cartpole", "particle", "a1", "humanoid")
# what each model's arrays can show. Everything else is in not_shown(), by name:
#   tree      everything (tests/models/smooth_tree.xml is there for what the others cannot: a ball joint, springs off qpos0, an affine
#             actuator bias under a gear, a force range)
#   probe     no gravity, no armature, no spring, biastype none
#   cartpole  the pole turns about a principal axis through a fixed direction (no gyroscopic torque, body_iquat is the identity); no
#             armature, no spring, no free joint, biastype none
#   particle  two slides of a point mass: the mass matrix is constant and nothing turns; only damping, the clamp and the update order
#   a1        jnt_stiffness is zero on every joint (qpos_spring differs from qpos0, with nothing to act on it), biastype none
#   humanoid  qpos_spring equals qpos0 on every sprung joint, biastype none
SHOWN = {
    "tree": MUTATIONS,
    "probe": ("no_gyroscopic", "no_velocity_products", "ipos_ignored", "iquat_ignored", "explicit_damping", "free_omega_in_world_frame",
              "ctrl_unclamped", "position_from_old_velocity"),
    "cartpole": ("no_velocity_products", "ipos_ignored", "gravity_at_body_origin", "explicit_damping", "ctrl_unclamped", "position_from_old_velocity"),
    "particle": ("explicit_damping", "ctrl_unclamped", "position_from_old_velocity"),
    "a1": ("no_gyroscopic", "no_velocity_products", "ipos_ignored", "iquat_ignored", "gravity_at_body_origin", "armature_outside_damped_solve",
           "explicit_damping", "free_omega_in_world_frame", "ctrl_unclamped", "position_from_old_velocity"),
    "humanoid": ("no_gyroscopic", "no_velocity_products", "ipos_ignored", "iquat_ignored", "gravity_at_body_origin", "armature_outside_damped_solve",
                 "explicit_damping", "free_omega_in_world_frame", "ctrl_unclamped", "position_from_old_velocity"),
}


def not_shown(key):
    return tuple(m for m in MUTATIONS if m not in SHOWN[key])


def num(x):
    return x if isinstance(x, mpf) else mpf(float(x))


def vec(x):
    return [num(v) for v in x]


def floats(x):
    return np.array([float(v) for v in x])


# ------------------------------------------------------------------------------------------------ kinematics of the wrong readings
class WorldOmegaKinematics(rr.Kinematics):
    """free_omega_in_world_frame: a free or ball joint's angular velocity read in the parent's frame (q <- exp(eps w / 2) q)"""

    def displaced(self, qpos, qvel, eps):
        B = self.B
        q, v = B.vec(qpos), B.vec(qvel)
        out = super().displaced(qpos, qvel, eps)
        for j, t in enumerate(self.jnt_type):
            qa, da = self.qadr[j], self.dadr[j]
            if t == FREE:
                out[qa + 3:qa + 7] = rr.q_mul(rr.q_rotvec(B, [eps * v[da + 3 + k] for k in range(3)]), rr.q_unit(B, q[qa + 3:qa + 7]))
            if t == BALL:
                out[qa:qa + 4] = rr.q_mul(rr.q_rotvec(B, [eps * v[da + k] for k in range(3)]), rr.q_unit(B, q[qa:qa + 4]))
        return out


def _world_kin(mdl):
    if "world_kin" not in mdl._cache:
        mdl._cache["world_kin"] = WorldOmegaKinematics(mdl.fm)
    return mdl._cache["world_kin"]


def _with_kin(mdl, kin):
    return dataclasses.replace(mdl, kin=kin, _cache={})


# ------------------------------------------------------------------------------------------------ the smooth dynamics at (q, v)
def _mat_vec(A, x):
    return [sum(a * b for a, b in zip(row, x)) for row in A]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _skew_vee(W):
    return [(W[2][1] - W[1][2]) / 2, (W[0][2] - W[2][0]) / 2, (W[1][0] - W[0][1]) / 2]


def _d1(f, e):
    """first derivative at 0 from f[-2], f[-1], f[1], f[2] (lists of numbers)"""
    return [(-a2 + 8 * a1 - 8 * b1 + b2) / (12 * e) for a2, a1, b1, b2 in zip(f[2], f[1], f[-1], f[-2])]


def _d2(f, e):
    return [(-a2 + 16 * a1 - 30 * z + 16 * b1 - b2) / (12 * e * e) for a2, a1, z, b1, b2 in zip(f[2], f[1], f[0], f[-1], f[-2])]


def _flat(R):
    return [v for row in R for v in row]


def _mat(f):
    return [f[0:3], f[3:6], f[6:9]]


class AtPose:
    """what depends on q alone, shared by every Smooth at the same q (the candidates of a case; stages 1 and 2 of RK4): the Jacobians,
    the world inertias, M and the inverses of M + h D"""

    def __init__(self, mdl, q, kin, world_omega):
        self.a = mdl.fm.arrays
        live = mdl.nbody_live
        jkey = ("J", floats(q).tobytes())          # force_noise_cases.force_map's own cache entry, where q is a vector of doubles
        exact = not world_omega and all(num(float(x)) == x for x in q)
        if exact and jkey in mdl._cache:
            self.J, self.base = mdl._cache[jkey]
        else:
            self.J, self.base = fn.jacobians(_with_kin(mdl, kin) if world_omega else mdl, q, upto=live)
            if exact:
                mdl._cache[jkey] = (self.J, self.base)
        self.bodies = sorted({b for b, _ in self.J})
        self.dofs = {b: sorted(k for bb, k in self.J if bb == b) for b in self.bodies}
        self.body = {}
        for b in self.bodies:
            inertia = vec(self.a["body_inertia"][b])
            R0, Ri = self.base.xmat(b), self.base.ximat(b)
            Iw = [[sum(Ri[i][k] * inertia[k] * Ri[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
            Ib = [[sum(R0[i][k] * inertia[k] * R0[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
            self.body[b] = dict(m=num(self.a["body_mass"][b]), Iw=Iw, Ib=Ib)
        self.memo = {}


def at_pose(mdl, q, kin, world_omega=False):
    key = ("pose", tuple(q), world_omega)
    if key not in mdl._cache:
        mdl._cache[key] = AtPose(mdl, q, kin, world_omega)
    return mdl._cache[key]


class Smooth:
    """everything of the smooth dynamics at one (q, v) that no control changes: the Jacobians, the poses' derivatives along the path, M, the
    bias and the passive force; `world_omega` builds them for the free_omega_in_world_frame reading"""

    def __init__(self, mdl, q, v, world_omega=False):
        self.mdl, self.a = mdl, mdl.fm.arrays
        self.q, self.v = vec(q), vec(v)
        self.nv, self.nq = mdl.nv, mdl.nq
        kin = _world_kin(mdl) if world_omega else mdl.kin
        self.kin = kin
        self.pose = at_pose(mdl, self.q, kin, world_omega)
        self.J, self.bodies, self.dofs = self.pose.J, self.pose.bodies, self.pose.dofs
        e, live = STENCIL, mdl.nbody_live
        P = {s: (self.pose.base if s == 0 else kin.forward(kin.displaced(self.q, self.v, s * e), mdl.mocap, live)) for s in (-2, -1, 0, 1, 2)}
        self.gravity = vec(mdl.fm.scalars["gravity"])
        self.body = {}
        for b in self.bodies:
            c = {s: P[s].xipos(b) for s in P}
            x = {s: P[s].xpos(b) for s in P}
            R = {s: _flat(P[s].xmat(b)) for s in P}
            R0 = P[0].xmat(b)
            Rd, Rdd = _mat(_d1(R, e)), _mat(_d2(R, e))
            W = _skew_vee(fn._mat_mul_t(Rd, R0))
            Wd = _skew_vee(fn._mat_mul_t(Rdd, R0))
            self.body[b] = dict(self.pose.body[b], cdd=_d2(c, e), xdd=_d2(x, e), W=W, Wd=Wd)
        self._memo = {}

    # ---- M
    def mass(self, mutation=None):
        key = ("M", mutation if mutation in ("ipos_ignored", "iquat_ignored") else None)
        memo = self.pose.memo
        if key not in memo:
            nv = self.nv
            Mm = [[mpf(0)] * nv for _ in range(nv)]
            for b in self.bodies:
                d = self.body[b]
                I = d["Ib"] if key[1] == "iquat_ignored" else d["Iw"]
                lin = {k: self.J[(b, k)][1 if key[1] == "ipos_ignored" else 0] for k in self.dofs[b]}
                Iw = {k: _mat_vec(I, self.J[(b, k)][2]) for k in self.dofs[b]}
                for k in self.dofs[b]:
                    for l in self.dofs[b]:
                        if l > k:
                            continue
                        val = d["m"] * _dot(lin[k], lin[l]) + _dot(self.J[(b, k)][2], Iw[l])
                        Mm[k][l] += val
                        if l != k:
                            Mm[l][k] += val
            memo[key] = Mm
        return memo[key]

    def armature(self):
        return vec(self.a["dof_armature"])

    def mass_full(self, mutation=None):
        Mm = [list(r) for r in self.mass(mutation)]
        for k, arm in enumerate(self.armature()):
            Mm[k][k] += arm
        return Mm

    # ---- the bias
    def bias(self, mutation=None):
        muts = ("no_gyroscopic", "no_velocity_products", "ipos_ignored", "iquat_ignored", "gravity_at_body_origin")
        key = ("bias", mutation if mutation in muts else None)
        if key not in self._memo:
            mut = key[1]
            out = [mpf(0)] * self.nv
            for b in self.bodies:
                d = self.body[b]
                I = d["Ib"] if mut == "iquat_ignored" else d["Iw"]
                acc = d["xdd"] if mut == "ipos_ignored" else d["cdd"]
                if mut == "no_velocity_products":
                    inertial, torque = [mpf(0)] * 3, [mpf(0)] * 3
                else:
                    inertial = [d["m"] * v for v in acc]
                    torque = _mat_vec(I, d["Wd"])
                    if mut != "no_gyroscopic":
                        torque = [t + w for t, w in zip(torque, _cross(d["W"], _mat_vec(I, d["W"])))]
                weight = [-d["m"] * v for v in self.gravity]
                for k in self.dofs[b]:
                    dc, dx, dth = self.J[(b, k)]
                    lin = dx if mut == "ipos_ignored" else dc
                    out[k] += _dot(lin, inertial) + _dot(dx if mut in ("gravity_at_body_origin", "ipos_ignored") else dc, weight) + _dot(dth, torque)
            self._memo[key] = out
        return self._memo[key]

    # ---- passive forces
    def passive(self, mutation=None):
        a, kin = self.a, self.kin
        out = [mpf(0)] * self.nv
        damp = vec(a["dof_damping"])
        for j, t in enumerate(kin.jnt_type):
            qa, da = kin.qadr[j], kin.dadr[j]
            stiff = num(a["jnt_stiffness"][j])
            if t in (FREE, BALL):
                assert stiff == 0 and not any(damp[da:da + (6 if t == FREE else 3)]), "a sprung or damped free or ball joint is not covered"
                continue
            ref = num(a["qpos0" if mutation == "spring_about_qpos0" else "qpos_spring"][qa])
            out[da] = -damp[da] * self.v[da] - stiff * (self.q[qa] - ref)
        for name in ("tendon_stiffness", "tendon_damping"):
            assert name not in a or not np.any(a[name]), name
        return out

    # ---- actuators
    def actuation(self, ctrl, mutation=None):
        a, kin = self.a, self.kin
        out = [mpf(0)] * self.nv
        trn = np.asarray(a["actuator_trnid"]).reshape(len(ctrl), -1)[:, 0]
        for i, u in enumerate(ctrl):
            j = int(trn[i])
            assert kin.jnt_type[j] in (HINGE, SLIDE) and int(a["actuator_gaintype"][i]) == 0 and int(a["actuator_biastype"][i]) in (0, 1)
            u = num(u)
            if a["actuator_ctrllimited"][i] and mutation != "ctrl_unclamped":
                u = max(min(u, num(a["actuator_ctrlrange"][i][1])), num(a["actuator_ctrlrange"][i][0]))
            gear = num(np.asarray(a["actuator_gear"]).reshape(len(ctrl), -1)[i, 0])
            force = num(a["actuator_gainprm"][i][0]) * u
            if int(a["actuator_biastype"][i]) == 1:
                b0, b1, b2 = vec(a["actuator_biasprm"][i][:3])
                scale = mpf(1) if mutation == "gear_not_squared_in_bias" else gear
                force += b0 + b1 * scale * self.q[kin.qadr[j]] + b2 * scale * self.v[kin.dadr[j]]
            if a["actuator_forcelimited"][i]:
                force = max(min(force, num(a["actuator_forcerange"][i][1])), num(a["actuator_forcerange"][i][0]))
            out[kin.dadr[j]] += gear * force
        return out

    def damping(self):
        return vec(self.a["dof_damping"])

    def smooth_force(self, ctrl, mutation=None):
        return [t + p - b for t, p, b in zip(self.actuation(ctrl, mutation), self.passive(mutation), self.bias(mutation))]

    def inverse(self, h, mutation=None):
        """(M + h D)^-1 -- of M alone for the explicit readings (h = 0: the plain acceleration)"""
        kind = mutation if mutation in ("ipos_ignored", "iquat_ignored", "armature_outside_damped_solve", "explicit_damping") else None
        key, memo = ("inv", kind, float(h)), self.pose.memo
        if key not in memo:
            A = self.mass(kind) if kind == "armature_outside_damped_solve" else self.mass_full(kind)
            A = [list(r) for r in A]
            if kind != "explicit_damping":
                for k, dmp in enumerate(self.damping()):
                    A[k][k] += num(h) * dmp
            memo[key] = (A, MPC.matrix(A) ** -1)
        return memo[key]

    def acceleration(self, ctrl, mutation=None):
        """qacc_smooth = M^-1 (tau_act + passive - bias)"""
        _, Ai = self.inverse(0.0, mutation if mutation in ("ipos_ignored", "iquat_ignored") else None)
        f = self.smooth_force(ctrl, mutation)
        return [sum(Ai[k, l] * f[l] for l in range(self.nv)) for k in range(self.nv)]

    def euler(self, ctrl, h, mutation=None):
        """(q', v') of one Euler step with implicit joint damping"""
        h = num(h)
        _, Ai = self.inverse(h, mutation)
        f = self.smooth_force(ctrl, mutation)
        v1 = [self.v[k] + h * sum(Ai[k, l] * f[l] for l in range(self.nv)) for k in range(self.nv)]
        q1 = self.kin.displaced(self.q, self.v if mutation == "position_from_old_velocity" else v1, h)
        return q1, v1


def smooth(mdl, state, mutation=None):
    """the cached Smooth of a model at a recorded state"""
    world = mutation == "free_omega_in_world_frame"
    key = ("smooth", np.asarray(state, float).tobytes(), world)
    if key not in mdl._cache:
        mdl._cache[key] = Smooth(mdl, state[:mdl.nq], state[mdl.nq:], world)
    return mdl._cache[key]


def rk4(mdl, q, v, ctrl, h, first=None):
    """the classical tableau on (q, v): k_i = (v_i, a(q_i, v_i)), q_i = q (+) c_i h (the stage's velocity), no implicit damping. Stages 1
    and 2 start from positions no control changes (q and q (+) h / 2 v): their Jacobians and M are shared by the candidates of a state
    (at_pose); `first` is the state's cached Smooth"""
    h = num(h)
    kin = mdl.kin
    q, v = vec(q), vec(v)
    A = ((), (mpf(1) / 2,), (0, mpf(1) / 2), (0, 0, mpf(1)))
    Bw = (mpf(1) / 6, mpf(1) / 3, mpf(1) / 3, mpf(1) / 6)
    dq, dv = [], []
    for i in range(4):
        dqi = [sum(A[i][j] * dq[j][k] for j in range(i)) for k in range(len(v))] if i else [mpf(0)] * len(v)
        vi = [v[k] + h * sum(A[i][j] * dv[j][k] for j in range(i)) for k in range(len(v))] if i else v
        qi = kin.displaced(q, dqi, h) if i else q
        s = first if i == 0 and first is not None else Smooth(mdl, qi, vi)
        dq.append(vi)
        dv.append(s.acceleration(ctrl))
    vq = [sum(Bw[i] * dq[i][k] for i in range(4)) for k in range(len(v))]
    v1 = [v[k] + h * sum(Bw[i] * dv[i][k] for i in range(4)) for k in range(len(v))]
    return kin.displaced(q, vq, h), v1


# RK4 rows. The small models: every state and all sixteen controls. The probe, the A1 and the Humanoid: two further sets of Jacobians per
# candidate (stages 3 and 4), 0.5 / 0.9 / 1.8 s a candidate, so RK4_STATES = the fastest state and the next of the ranking, each under four
# controls: zero, both saturated ends, and the first of the random ones with an entry past an end -- 2 x 4 = 8 candidates a model.
RK4_SMALL, RK4_LARGE, RK4_STATES = ("tree", "brick", "cartpole", "particle"), ("probe", "a1", "humanoid"), (0, 1)
RK4_DEVICE_ROWS = {"wave-tree-rk4-fp64": ("tree", "wave-rk4-a1-fp64"), "wave-probe-rk4-fp64": ("probe", "wave-rk4-a1-fp64"),
                   "wave-a1-rk4-fp64": ("a1", "wave-rk4-a1-fp64"), "wave-humanoid-rk4-fp64": ("humanoid", "wave-rk4-humanoid-fp64")}
_RK4 = {}


def rk4_states(key):
    return tuple(range(len(cases(key)))) if key in RK4_SMALL else RK4_STATES


def rk4_candidates(key, i):
    """the candidates of case i an RK4 row compares"""
    c = cases(key)[i]
    if key in RK4_SMALL:
        return list(range(len(c.controls)))
    r = np.asarray(model(key).fm.arrays["actuator_ctrlrange"], float).reshape(-1, 2)
    beyond = [k for k in range(3, len(c.controls)) if np.any((c.controls[k, 0] < r[:, 0]) | (c.controls[k, 0] > r[:, 1]))]
    past = beyond[0] if beyond else 3       # (the probe's one motor: none of the first state's thirteen random controls passes an end)
    assert beyond or (key, i) == ("probe", 0), (key, i)
    assert np.all(c.controls[0] == 0) and np.all(c.controls[1, 0] == r[:, 0]) and np.all(c.controls[2, 0] == r[:, 1])
    return [0, 1, 2, past]


def rk4_expect(key, i):
    """(candidates, [len(candidates), nq + nv]): the reference's RK4 step of case i of a model; asserts the case's condition on the limits"""
    if (key, i) not in _RK4:
        mdl, c = model(key), cases(key)[i]
        cands, out = rk4_candidates(key, i), []
        for k in cands:
            q1, v1 = rk4(mdl, c.state[:mdl.nq], c.state[mdl.nq:], c.controls[k, 0], mdl.dt, first=smooth(mdl, c.state))
            assert inside_limits(mdl.fm.arrays, q1), (key, c.label, "a limited joint leaves its range in the RK4 step")
            out.append(np.concatenate([floats(q1), floats(v1)]))
        _RK4[(key, i)] = (cands, np.array(out))
    return _RK4[(key, i)]


# ------------------------------------------------------------------------------------------------ models and cases
_MODELS = {}


def tree_state():
    """qpos 6 (the ball's quaternion, the hinge, the slide), qvel 5: bent, turning about every axis, both springs off their rest"""
    quat = np.array([0.6, -0.5, 0.3, 0.55])
    return np.concatenate([quat / np.linalg.norm(quat), [-0.6, 0.12], [1.4, -2.1, 0.9], [2.5, -0.7]])


def brick_state():
    """tests/models/free_body.xml: the brick in a skew orientation, tumbling about no principal axis; the arm swinging"""
    quat = np.array([0.5, -0.3, 0.7, 0.4])
    return np.concatenate([[0.1, -0.2, 2.0], quat / np.linalg.norm(quat), [0.7], [0.3, -0.2, 0.5], [2.0, -3.0, 1.2], [-1.5]])


XML_MODELS = {"tree": ("smooth_tree.xml", tree_state), "brick": ("free_body.xml", brick_state)}


def model(key):
    """force_noise_cases.model(key); 'a1-floss': the A1 as registered (friction loss and contacts on); 'tree', 'brick': tests/models/smooth_tree.xml, free_body.xml"""
    if key in XML_MODELS:
        if key not in _MODELS:
            from mujoco_mpc_amd import mjcf
            from mujoco_mpc_amd.task import Task
            fm = mjcf.load_xml(os.path.join(fn.HERE, "models", XML_MODELS[key][0]))
            task = Task(name="scene", residual_id=0, model=fm).reset()
            _MODELS[key] = fn.Model(key, task, task.packed_model(), task.packed(), XML_MODELS[key][1](), None, 0.25, rr.Kinematics(fm))
        return _MODELS[key]
    if key != "a1-floss":
        return fn.model(key)
    if key not in _MODELS:
        base = fn.model("a1")
        _MODELS[key] = dataclasses.replace(base, key=key, pm=base.task.packed_model(), _cache=base._cache)
    return _MODELS[key]


@dataclasses.dataclass
class Case:
    key: str
    label: str
    state: np.ndarray
    controls: np.ndarray          # [16, 1, nu]


def _bank(key):
    return {"a1": sb.a1_bank, "humanoid": sb.humanoid_bank}[key]() if key in ("a1", "humanoid") else sb.lane_bank(key.capitalize())


def _mid_range(a, state):
    state = np.array(state, float)
    for j in np.flatnonzero(a["jnt_limited"]):
        lo, hi = a["jnt_range"][j]
        qa = int(a["jnt_qposadr"][j])
        state[qa] = np.clip(state[qa], lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo))
    return state


def rbound_max(a):
    """the largest bounding radius of a geom that moves (the static scenery's boxes do not come down on anything)"""
    out = 0.0
    for t, s, b in zip(a["geom_type"], np.asarray(a["geom_size"], float), a["geom_bodyid"]):
        t = int(t)
        if t == GEOM_PLANE or int(b) == 0 or a["body_mocapid"][int(b)] >= 0:
            continue
        r = s[0] if t == GEOM_SPHERE else s[0] + s[1] if t == GEOM_CAPSULE else float(np.hypot(s[0], s[1])) if t == GEOM_CYLINDER else float(np.linalg.norm(s))
        out = max(out, float(r))
    return out


def contacts_enabled(mdl):
    """contacts are on and the model has a floor that collides"""
    a = mdl.fm.arrays
    floor = any(int(t) == GEOM_PLANE and (int(ct) or int(ca)) for t, ct, ca in zip(a["geom_type"], a["geom_contype"], a["geom_conaffinity"]))
    return floor and not (int(mdl.pm.struct.disableflags) & fn.DSBL_CONTACT)


def inside_limits(a, q):
    """every limited joint strictly inside its range"""
    return all(a["jnt_range"][j][0] < float(q[int(a["jnt_qposadr"][j])]) < a["jnt_range"][j][1] for j in np.flatnonzero(a["jnt_limited"]))


def clear_of_the_floor(mdl, state):
    if not contacts_enabled(mdl):
        return True
    P = mdl.kin.forward(state[:mdl.nq], mdl.mocap)
    a = mdl.fm.arrays
    need = CLEARANCE + rbound_max(a)
    moving = [b for b in range(1, mdl.nbody) if a["body_mocapid"][b] < 0]
    return all(float(P.xipos(b)[2]) > need for b in moving)


def oracle_rows(mdl, state, ctrl):
    """the oracle's constraint row types at the state, with the model's flags (selection only)"""
    orc = fn.oracle_of(mdl)
    _, nefc = orc.at(state, mdl.time, ctrl)
    return set(orc.ph.get("efc_type").astype(int).tolist()) if nefc else set()


def _refusal(mdl, state, nodes):
    """why a state is not taken (None: it meets every condition): the limits, the clearance and, with the flags of every row that uses it,
    the oracle's constraint rows (none; the friction-loss rows: friction loss only)"""
    a = mdl.fm.arrays
    if not inside_limits(a, state):
        return "a limited joint on or outside its range"
    if not clear_of_the_floor(mdl, state) or (mdl.key == "a1" and not clear_of_the_floor(model("a1-floss"), state)):
        return "a body's centre within 0.5 m + the bounding radius of the floor"
    for u in nodes[:3, 0]:
        rows = oracle_rows(mdl, state, u)
        if rows:
            return f"the oracle reports constraint rows of types {sorted(rows)}"
        if mdl.key == "a1" and not oracle_rows(model("a1-floss"), state, u) <= {EFC_FRICTION}:
            return "with friction loss on, the oracle reports rows other than friction loss"
    return None


SKIPPED = {}       # model: [(label, why)] -- the states of the ranking that were passed over before the cases were complete
# device row: (model, the row of test_gpu_step_parity.ROWS its kernel, switches, precision and bound come from, what is held). The probe
# and the tree run the generic wavefront kernel under their own integrator (Euler). ROWS has no row for either: kernel name, switches and
# bound are BORROWED from the generic kernel's A1 rows (wave-rk4-a1-fp64: 1e-9, the bound of every fp64 row; wave-rk4-a1-fp32: 1e-4, which
# is also test_gpu_step_parity.STEP_GOAL, the per-step bound every float row should meet). A change of that A1 row's bound moves these too.
DEVICE_ROWS = {
    "limb-fp64": ("humanoid", "limb-no-fallback-fp64", "state"), "limb-fp32": ("humanoid", "limb-no-fallback-fp32", "state"),
    "tree-humanoid-fp64": ("humanoid", "tree-humanoid-fp64", "state"), "tree-humanoid-fp32": ("humanoid", "tree-humanoid-fp32", "state"),
    "tree-a1-fp64": ("a1", "tree-a1-fp64", "state"), "tree-a1-fp32": ("a1", "tree-a1-fp32", "state"),
    "wave-probe-fp64": ("probe", "wave-rk4-a1-fp64", "state"), "wave-probe-fp32": ("probe", "wave-rk4-a1-fp32", "state"),
    "wave-tree-fp64": ("tree", "wave-rk4-a1-fp64", "state"),
    "lane-cartpole-fp64": ("cartpole", "lane-cartpole-fp64", "state"), "lane-cartpole-fp32": ("cartpole", "lane-cartpole-fp32", "state"),
    "lane-particle-fp64": ("particle", "lane-particle-fp64", "state"), "lane-particle-fp32": ("particle", "lane-particle-fp32", "state"),
    "quad-floss-fp64": ("a1-floss", "quad-fp64", "momentum"), "tree-a1-floss-fp64": ("a1-floss", "tree-a1-fp64", "momentum"),
}
_CASES = {}


def cases(key):
    """the cases of a model (the a1-floss rows use those of a1)"""
    key = "a1" if key == "a1-floss" else key
    if key in _CASES:
        return _CASES[key]
    mdl = model(key)
    a = mdl.fm.arrays
    r = np.asarray(a["actuator_ctrlrange"], float).reshape(-1, 2)
    out = []
    if key == "probe":
        s0 = fn.probe_state()
        rng = np.random.default_rng(77)
        s1 = s0.copy()
        s1[mdl.nq:] *= 2.5                                   # the same pose, everything faster
        s2 = s0.copy()                                        # another pose of the chain, the ball and the hinges, other rates
        s2[0:2] = [-1.1, 0.9]
        quat = np.array([-0.2, 0.6, 0.3, -0.7])
        s2[5:9] = quat / np.linalg.norm(quat)
        s2[9:mdl.nq] = rng.uniform(-2.5, 2.5, mdl.nq - 9)
        s2[mdl.nq:] = rng.uniform(-3, 3, mdl.nv)
        pool = [("probe_state", s0), ("probe_state x 2.5", s1), ("second pose", s2)]
        want = N_PROBE_STATES
    elif key == "brick":
        pool, want = [("brick_state", brick_state())], 1
    elif key == "tree":
        s0 = tree_state()
        s1, s2 = s0.copy(), s0.copy()
        s1[mdl.nq:] *= -2.0                                  # the same pose, turning the other way, faster
        quat = np.array([-0.3, 0.2, 0.8, 0.4])
        s2[0:4], s2[4:6], s2[mdl.nq:] = quat / np.linalg.norm(quat), [0.9, -0.08], [-0.8, 0.6, 2.2, -1.9, 1.1]
        pool = [("tree_state", s0), ("tree_state x -2", s1), ("second pose", s2)]
        want = N_PROBE_STATES
    else:
        bank = _bank(key)
        # by speed: the fastest, then every (n / 6)-th of the ranking -- fast and slow ones alike --, then whatever is left, in that order
        rank = sorted(range(len(bank.states)), key=lambda i: -float(np.max(np.abs(bank.states[i].state[mdl.nq:]))))
        order = rank[::max(len(rank) // N_STATES, 1)]
        order += [i for i in rank if i not in order]
        pool = []
        for i in order:
            s = np.array(bank.states[i].state, float)
            if key in ("a1", "humanoid"):
                s[2] += LIFT
            pool.append((bank.states[i].label, _mid_range(a, s)))
        want = N_STATES
    for label, state in pool:
        nodes = sb.step_controls(mdl.fm.nu, r[:, 0], r[:, 1], seed=1000 + len(out))
        why = _refusal(mdl, state, nodes)
        assert why is None or out, (key, label, "the fastest state of the bank does not meet the conditions", why)
        if why is None:
            out.append(Case(key, label, state, nodes))
        else:
            SKIPPED.setdefault(key, []).append((label, why))
        if len(out) == want:
            break
    assert len(out) == want, (key, len(out))
    for c in out:          # the conditions, on the states that are used
        assert inside_limits(a, c.state) and clear_of_the_floor(mdl, c.state), (key, c.label)
        assert not oracle_rows(mdl, c.state, c.controls[0, 0]), (key, c.label)
        if key == "a1":
            assert clear_of_the_floor(model("a1-floss"), c.state) and oracle_rows(model("a1-floss"), c.state, c.controls[0, 0]) <= {EFC_FRICTION}
    SKIPPED.setdefault(key, [])
    _CASES[key] = out
    return out


# ------------------------------------------------------------------------------------------------ expectations
@dataclasses.dataclass
class Expect:
    """one case under a reading: per candidate the next state, and what the oracle's fields are held to"""
    next_state: np.ndarray        # [16, nq + nv]
    qacc_smooth: np.ndarray       # [16, nv]
    actuator: np.ndarray          # [16, nv]
    M: np.ndarray
    bias: np.ndarray
    passive: np.ndarray


_EXPECT = {}


def expect(key, i, mutation=None):
    """the reference's answers for case i of a model under a reading (None: the right one); asserts the case's conditions"""
    key = "a1" if key == "a1-floss" else key
    if (key, i, mutation) in _EXPECT:
        return _EXPECT[(key, i, mutation)]
    mdl, c = model(key), cases(key)[i]
    s = smooth(mdl, c.state, mutation)
    nxt, acc, act = [], [], []
    for u in c.controls[:, 0]:
        q1, v1 = s.euler(u, mdl.dt, mutation)
        nxt.append(np.concatenate([floats(q1), floats(v1)]))
        acc.append(floats(s.acceleration(u, mutation)))
        act.append(floats(s.actuation(u, mutation)))
        if mutation is None:
            assert inside_limits(mdl.fm.arrays, q1), (key, c.label, "a limited joint leaves its range in the step")
    out = Expect(np.array(nxt), np.array(acc), np.array(act), np.array([[float(v) for v in r_] for r_ in s.mass_full(mutation)]),
                 floats(s.bias(mutation)), floats(s.passive(mutation)))
    _EXPECT[(key, i, mutation)] = out
    return out


def share(got, want, tol):
    """max |d - r| / (tol (1 + |r|)) and where"""
    e = np.abs(np.asarray(got, float) - want) / (tol * (1 + np.abs(want)))
    e = np.where(np.isnan(e), np.inf, e)
    i = int(np.argmax(e))
    return float(e.flat[i]), np.unravel_index(i, e.shape)


def visibility(key, mutation, tol=STEP_TOL64, limit=None):
    """the largest miss, in bounds, of the reading's next states against the right ones over the model's cases -- from the reference alone;
    stops at the first case that shows it by more than `limit` bounds"""
    worst = 0.0
    for i in range(len(cases(key))):
        worst = max(worst, share(expect(key, i, mutation).next_state, expect(key, i).next_state, tol)[0])
        if limit is not None and worst > limit:
            break
    return worst


# ------------------------------------------------------------------------------------------------ the momentum balance
def momentum_balance(key, i, got_next, tol):
    """the friction-loss rows: got_next [16, nq + nv] of a kernel that steps the A1 WITH friction loss. Returns (worst share of the
    allowance, entries compared): rho_k = 0 on the trunk and |rho_k| <= dof_frictionloss_k on the joints, each within
    sum_j |M + h D|_kj tol (1 + |v'_j|) / h; q' within tol (1 + |q'|) of q (+) h v' of the kernel's own v'"""
    mdl, c = model("a1"), cases("a1")[i]
    s = smooth(mdl, c.state)
    h = num(mdl.dt)
    A, _ = s.inverse(mdl.dt)
    Aabs = np.abs(np.array([[float(v) for v in r_] for r_ in A]))
    floss = np.asarray(mdl.fm.arrays["dof_frictionloss"], float)
    assert not floss[:6].any() and floss[6:].all()
    worst, n = 0.0, 0
    for cand, u in enumerate(c.controls[:, 0]):
        v1 = vec(got_next[cand, mdl.nq:])
        f = s.smooth_force(u)
        rho = floats([sum(A[k][l] * (v1[l] - s.v[l]) for l in range(mdl.nv)) / h - f[k] for k in range(mdl.nv)])
        allow = Aabs @ (tol * (1 + np.abs(got_next[cand, mdl.nq:]))) / mdl.dt
        over = np.maximum(np.abs(rho) - floss, 0.0) / allow
        worst, n = max(worst, float(over.max())), n + mdl.nv
        q1 = floats(s.kin.displaced(s.q, v1, h))
        worst, n = max(worst, share(got_next[cand, :mdl.nq], q1, tol)[0]), n + mdl.nq
    return worst, n
