"""Residual cases whose answers are known before any kernel runs (test infrastructure, CPU only; not a conftest).

A case is (task, state, time, mocap, frozen residual state, task parameters, control) with the expected residual row from
tests/residual_reference.py (mpmath, 50 digits), the branch labels the reference took on it, and, for the anchor cases, literals derived by
hand from the tasks' design constants (`literal`: entry -> value, held to 1e-12 against the reference by tests/test_residual_cases.py).

`fp64_only` cases sit exactly on a comparison the kernels make in their own precision (the flip's phase instants, |angvel| = 0.01): a float
kernel holds another threshold, so they run on fp64 rows only. `expected32` is the reference at the float32-rounded state, time, mocap,
frozen reals and parameters; sensitivities() gives, per case, the largest relative change of an expected entry when one input moves by one
float32 ulp, and the cases where that exceeds a tenth of STEP_GOAL stay off the fp32 rows (FP32_EXCLUDED)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import residual_reference as rr
from mujoco_mpc_amd.task import load_task

FP64_BOUND = 1e-9          # |d - e| <= 1e-9 (1 + |e|): the project's one-step fp64 bound (tests/test_gpu_step_parity.py)
STEP_GOAL = 1e-4           # the standing fp32 per-step goal (tests/test_gpu_step_parity.py STEP_GOAL)
LITERAL_TOL = 1e-12
CONTROL_ENTRIES = {"QuadrupedFlat": slice(13, 25), "HumanoidTrack": slice(21, 42), "Cartpole": slice(3, 4)}

BRANCHES = frozenset(
    ["flip:" + p for p in ("crouch", "leap", "flight", "land", "after")]
    + ["terrain:" + g for g in ("floor", "box", "ramp", "hill", "inside-box", "look-ahead")]
    + ["walk:" + w for w in ("straight", "circle", "threshold", "zero-heading")]
    + ["biped:foot-stand", "biped:hand-stand"]
    + ["step-zero:" + s for s in ("duty", "amplitude", "cos")]
    + ["sub-quat:" + s for s in ("small", "normal", "wrap")]
    + ["humanoid:" + h for h in ("before", "interior", "last-key", "beyond")]
    + ["gait:negative-fmod"])


@dataclass
class Case:
    name: str
    task: str
    state: np.ndarray
    time: float
    mocap: np.ndarray | None
    ctrl: np.ndarray
    frozen: dict = field(default_factory=dict)
    residual_int: list = field(default_factory=list)
    residual_real: list = field(default_factory=list)
    parameters: list = field(default_factory=list)
    literal: dict = field(default_factory=dict)
    fp64_only: bool = False
    expected: np.ndarray = None
    expected32: np.ndarray = None
    head: np.ndarray = None
    labels: frozenset = frozenset()


@functools.lru_cache(maxsize=None)
def task_of(name):
    t = load_task(name)
    if name == "QuadrupedFlat":
        t.transition(0.0)
    return t


@functools.lru_cache(maxsize=None)
def kinematics(name, backend="MP"):
    return rr.Kinematics(task_of(name).model, getattr(rr, backend))


def parameter_names(t):
    return [k for k in t.model.numeric if k.startswith("residual_")]


# ------------------------------------------------------------------------------------------------ small float helpers (placing the robot)
def quat(axis, angle):
    a = np.asarray(axis, float)
    n = np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a / n]) if n > 0 else np.array([1.0, 0, 0, 0])


def qmul(a, b):
    return np.array(rr.q_mul(list(a), list(b)), float)


def rotvec_quat(r):
    return np.array(rr.q_rotvec(rr.FL, [float(v) for v in r]), float)


def qmat(q):
    return np.array(rr.q_matrix([float(v) for v in q]), float)


# ------------------------------------------------------------------------------------------------ evaluation
def _round32(x):
    return None if x is None else np.asarray(x, np.float32).astype(np.float64)


def a1_frozen_from_reals(c, reals):
    f = dict(c.frozen)
    f.update(mode_start_time=reals[0], position=reals[1:3], heading=reals[4:6], speed=reals[6], angvel=reals[7], ground=reals[8],
             orientation=reals[9:13], phase_start=reals[13], phase_start_time=reals[14], phase_velocity=reals[15],
             flip_thresholds=[reals[20], reals[22], reals[22] + reals[18], reals[22] + reals[18] + reals[24]])
    return f


def evaluate(c, backend="MP", inputs=None, mutation=None, ctrl=None):
    """the reference on a case -> (residual as float64, labels, extras). inputs: (state, time, mocap, reals, parameters) to replace the
    case's (the float32-rounded ones, or a one-ulp move)"""
    B = getattr(rr, backend)
    t = task_of(c.task)
    state, time, mocap, reals, pars = inputs if inputs is not None else (c.state, c.time, c.mocap, c.residual_real, c.parameters)
    ctrl = c.ctrl if ctrl is None else ctrl
    nq = t.model.nq
    if c.task == "QuadrupedFlat":
        params = dict(zip(parameter_names(t), pars))
        r, labels, extra = rr.quadruped_residual(kinematics(c.task, backend), state[:nq], state[nq:], time, mocap, ctrl,
                                                 a1_frozen_from_reals(c, list(reals)), params, mutation)
    elif c.task == "HumanoidTrack":
        r, labels, extra = rr.humanoid_residual(kinematics(c.task, backend), state[:nq], state[nq:], time, ctrl, c.residual_int[0],
                                                c.residual_int[1], reals[0], mutation)
    elif c.task == "Cartpole":
        r, labels, extra = rr.cartpole_residual(B, state[:nq], state[nq:], ctrl, pars[0], t.model.arrays["actuator_ctrlrange"][0]), set(), {}
    else:
        goal = mocap[:2] if c.task == "Particle" else None
        r, labels, extra = rr.particle_residual(B, state[:nq], state[nq:], goal), set(), {}
    return np.array([float(v) for v in r]), labels, extra


def expected_for(c, ctrl, single=False):
    """the expected row under another control: only the control entries (Effort / action) change"""
    e = np.array(c.expected32 if single else c.expected)
    sl = CONTROL_ENTRIES.get(c.task)
    if sl is not None:
        a = task_of(c.task).model.arrays
        lo, hi = a["actuator_ctrlrange"][:, 0], a["actuator_ctrlrange"][:, 1]
        u = np.where(np.asarray(a["actuator_ctrllimited"]) != 0, np.clip(ctrl, lo, hi), ctrl)
        e[sl] = 0.02 * np.asarray(a["actuator_gainprm"])[:, 0] * u if c.task == "QuadrupedFlat" else u
    return e


def inputs32(c):
    return (_round32(c.state), float(np.float32(c.time)), _round32(c.mocap), list(_round32(c.residual_real)) if c.residual_real else [],
            list(_round32(c.parameters)) if c.parameters else [])


def sensitivity(c):
    """the largest |change| / (1 + |e|) of an expected entry when one input moves by one float32 ulp (Python floats: eight digits do)"""
    base_in = inputs32(c)
    base, _, _ = evaluate(c, "FL", base_in)
    worst = 0.0
    for which, arr in enumerate(base_in):
        if arr is None or which == 1:
            continue
        for i in range(len(arr)):
            if c.task == "QuadrupedFlat" and which == 3 and i >= 16:
                continue       # (the flip's constants: the kernels read them, the reference derives its own)
            moved = [np.array(a, float) if isinstance(a, (np.ndarray, list)) else a for a in base_in]
            moved[which][i] = float(np.nextafter(np.float32(arr[i]), np.float32(np.inf)))
            e, _, _ = evaluate(c, "FL", tuple(moved))
            worst = max(worst, float(np.max(np.abs(e - base) / (1 + np.abs(base)))))
    moved = list(base_in)
    moved[1] = float(np.nextafter(np.float32(base_in[1]), np.float32(np.inf)))
    e, _, _ = evaluate(c, "FL", tuple(moved))
    return max(worst, float(np.max(np.abs(e - base) / (1 + np.abs(base)))))


def finish(c):
    c.expected, labels, extra = evaluate(c)
    c.labels = frozenset(labels)
    c.head = None if "head" not in extra else np.array([float(v) for v in extra["head"]])
    if not c.fp64_only:
        c.expected32, _, _ = evaluate(c, inputs=inputs32(c))
    return c


# ------------------------------------------------------------------------------------------------ QuadrupedFlat
A1_MODES = {m: i for i, m in enumerate(rr.MODES)}
A1_GAITS = {g: i for i, g in enumerate(rr.GAITS)}
BOX_HOME = [-2.5, 0, 0, 1, 0, 0, 0]


def a1_case(name, qpos, qvel=None, time=0.0, goal=(0.3, 0.0, 0.26), box=BOX_HOME, ctrl=None, params=None, mode="Quadruped", gait="Trot",
            flip_dir=0, handstand=0, mode_start_time=0.0, position=(0.0, 0.0, 0.0), heading=(0.0, 0.0), speed=0.0, angvel=0.0, ground=0.0,
            orientation=(1.0, 0.0, 0.0, 0.0), phase=None, phase_start=0.0, phase_start_time=0.0, phase_velocity=4 * np.pi, **kw):
    t = task_of("QuadrupedFlat")
    ri = list(t.residual_int)
    ri[0], ri[8], ri[9], ri[10] = A1_MODES[mode], A1_GAITS[gait], int(flip_dir), int(handstand)
    if phase is not None:                  # the phase itself: the clock started at `time` with this value
        phase_start, phase_start_time = phase, time
    reals = [mode_start_time, *position, *heading, speed, angvel, ground, *orientation, phase_start, phase_start_time, phase_velocity, *t.flip]
    names = parameter_names(t)
    pars = list(t.parameters)
    pars[names.index("residual_select_Gait")] = float(A1_GAITS[gait])
    pars[names.index("residual_select_Flip dir")] = float(flip_dir)
    pars[names.index("residual_select_Biped type")] = float(handstand)
    for k, v in (params or {}).items():
        pars[names.index("residual_" + k)] = float(v)
    state = np.concatenate([np.asarray(qpos, float), np.zeros(18) if qvel is None else np.asarray(qvel, float)])
    mocap = np.concatenate([[*goal, 1, 0, 0, 0], np.asarray(box, float)])
    frozen = dict(mode=ri[0], gait=ri[8], flip_dir=ri[9], handstand=ri[10])
    return Case(name, "QuadrupedFlat", state, float(time), mocap, np.zeros(12) if ctrl is None else np.asarray(ctrl, float), frozen, ri,
                [float(v) for v in reals], pars, **kw)


def a1_qpos(pos, q=(1, 0, 0, 0), legs=None, key="home"):
    t = task_of("QuadrupedFlat")
    out = np.array(t.model.keyframes[key]["qpos"], float)
    out[0:3], out[3:7] = pos, q
    if legs is not None:
        out[7:] = legs
    return out


def trunk_at(q, com_height, xy=(0.0, 0.0)):
    """the trunk position that puts its inertial frame at com_height over xy, for the trunk orientation q"""
    t = task_of("QuadrupedFlat")
    ipos = np.asarray(t.model.arrays["body_ipos"], float)[t.ids["torso"]]
    off = qmat(q) @ ipos
    return np.array([xy[0] - off[0], xy[1] - off[1], com_height - off[2]])


def flip_cases():
    t = task_of("QuadrupedFlat")
    f = t.flip
    crouch, jump, flight, land = f[4], f[6], f[2], f[8]
    orientation = quat([0.1, -0.05, 1.0], 0.7)
    ground = 0.07
    rng = np.random.default_rng(21)
    out = []
    # (label, time, target height, target angle or None: ask the design, at the very threshold?)
    anchors = [("t0", 0.0, 0.25, 0.0, False), ("crouch-end", crouch, 0.15, 0.0, True), ("take-off", jump, 0.5, np.pi / 2, True),
               ("apex", jump + flight / 2, 0.8, 1.125 * np.pi, False), ("touch-down", jump + flight, 0.5, 1.75 * np.pi, True),
               ("landed", jump + flight + land, 0.25, 2 * np.pi, True)]
    interior = [("crouch", 0.08), ("leap", 0.3), ("flight", 0.6), ("land", 1.0), ("after", 1.5)]
    thresholds = [f[4], f[6], f[6] + f[2], f[6] + f[2] + f[8]]
    for k, (label, time, h, angle, edge) in enumerate(anchors + [(n, tm, None, None, False) for n, tm in interior]):
        if h is None:
            _, h, angle = rr.flip_target(rr.FL, time, thresholds)
        flip_dir = k % 2
        q = qmul(orientation, quat([0, 1, 0], (1 if flip_dir else -1) * angle))
        legs = a1_qpos([0, 0, 0], key="crouch" if k % 3 == 0 else "home")[7:] + rng.normal(0, 0.2, 12)
        start = 0.0 if edge else 0.4
        out.append(a1_case(f"flip/{label}", a1_qpos(trunk_at(q, h + ground, (0.2, -0.1)), q, legs), rng.normal(0, 0.5, 18), time + start,
                           mode="Flip", flip_dir=flip_dir, mode_start_time=start, ground=ground, orientation=orientation,
                           ctrl=rng.uniform(-1.3, 1.3, 12), fp64_only=edge, literal={0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0}))
    # the trunk composed with a known rotation vector in its own frame: Upright is that vector
    skew = np.array([0.48, -0.6, 0.64])
    for label, delta, time, ori in (("tiny", 1e-17 * skew, 0.0, np.array([1.0, 0, 0, 0])), ("skew", 0.3 * skew, 0.6, orientation),
                                    ("wrap", (np.pi + 0.2) * skew, 0.3, orientation)):
        _, h, angle = rr.flip_target(rr.FL, time, thresholds)
        q = qmul(qmul(ori, quat([0, 1, 0], -angle)), rotvec_quat(delta))
        expect = delta if label != "wrap" else delta * (np.linalg.norm(delta) - 2 * np.pi) / np.linalg.norm(delta)
        out.append(a1_case(f"flip/delta-{label}", a1_qpos(trunk_at(q, h + ground), q), None, time, mode="Flip", ground=ground, orientation=ori,
                           literal={0: expect[0], 1: expect[1], 2: expect[2], 3: 0.0}))
    return out


def terrain_cases():
    rng = np.random.default_rng(22)
    yawed = [-2.0, 0.5, 0.1, *quat([0, 0, 1], 0.5)]
    lifted = [-2.5, 0.0, 0.5, 1, 0, 0, 0]
    tilt = quat([0.3, 1.0, 0.1], 0.15)
    place = [("floor", (0.2, -0.3, 0.3), BOX_HOME, "Quadruped"), ("box-moved", (-2.0, 0.5, 0.72), yawed, "Quadruped"),
             ("ramp", (3.13, 2.5, 0.62), BOX_HOME, "Quadruped"), ("hill", (5.5, 6.3, 0.8), BOX_HOME, "Quadruped"),
             ("straddle", (-1.5, 0.1, 0.6), BOX_HOME, "Quadruped"), ("inside-box", (-2.5, 0.0, 0.5), lifted, "Quadruped")]
    out = []
    for k, (label, pos, box, mode) in enumerate(place):
        legs = a1_qpos([0, 0, 0])[7:] + rng.normal(0, 0.15, 12)
        out.append(a1_case(f"terrain/{label}", a1_qpos(pos, tilt, legs), rng.normal(0, 0.3, 18), 0.1 * k, box=box, gait="Canter", phase=1.0 + 0.3 * k,
                           ctrl=rng.uniform(-1.3, 1.3, 12)))
    # Scramble: the hind feet 0.08 short of the box edge at x = -1.5, the goal beyond it: the look-ahead lands on the box
    qp = a1_qpos((0.0, 0.0, 0.45))
    P = kinematics("QuadrupedFlat", "FL").forward(qp, None)
    hl = P.geom_xpos(kinematics("QuadrupedFlat", "FL").name("geom", "HL"))
    qp[0] = -1.42 - hl[0]
    out.append(a1_case("scramble/look-ahead", qp, rng.normal(0, 0.3, 18), 0.3, goal=(-3.0, 0.05, 0.4), mode="Scramble", gait="Walk", phase=2.0,
                       literal={3: 0.0}))
    # the goal exactly over a foot: no direction to look ahead in
    qp = a1_qpos((0.3, 0.2, 0.31))
    fl = kinematics("QuadrupedFlat").forward(qp, None).geom_xpos(kinematics("QuadrupedFlat").name("geom", "FL"))
    out.append(a1_case("scramble/goal-over-foot", qp, None, 0.0, goal=(float(fl[0]), float(fl[1]), 0.3), mode="Scramble", gait="Trot", phase=0.4,
                       literal={3: 0.0}))
    return out


def gait_cases():
    rng = np.random.default_rng(23)
    out = []

    def case(label, gait, phase=None, **kw):
        legs = a1_qpos([0, 0, 0])[7:] + rng.normal(0, 0.1, 12)
        return a1_case("gait/" + label, a1_qpos((0.1, 0.2, 0.33), quat([1, 0.5, 0.2], 0.1), legs), None, kw.pop("time", 0.25), gait=gait, phase=phase, **kw)
    for k, g in enumerate(rr.GAITS):
        out.append(case(f"{g}/duty0", g, np.pi / 3 + 0.1 * k))
    out.append(case("Walk/clock", "Walk", None, time=0.37, phase_start=0.4, phase_start_time=0.11, phase_velocity=2 * np.pi * 1.5))
    out.append(case("Gallop/duty0.5", "Gallop", 1.0, params={"Duty ratio": 0.5}))
    out.append(case("Canter/duty0.75", "Canter", 2.5, params={"Duty ratio": 0.75, "Amplitude": 0.1}))
    out.append(case("Walk/duty1", "Walk", 1.0, params={"Duty ratio": 1.0}))
    out.append(case("Walk/amplitude0", "Walk", 1.0, params={"Amplitude": 0.0}))
    out.append(case("Trot/phase0", "Trot", 0.0))                       # the hind-left and front-right feet at cos(-pi/2)
    out.append(case("Walk/before-clock", "Walk", None, time=0.2, phase_start=0.0, phase_start_time=1.0, phase_velocity=4 * np.pi))
    return out


def walk_cases():
    rng = np.random.default_rng(24)
    out = []
    for label, heading, speed, angvel, edge in (("straight", (0.6, -0.8), 0.7, 0.0, False), ("circle", (0.6, -0.8), 0.7, 0.5, False),
                                                ("threshold", (0.6, -0.8), 0.7, 0.01, True), ("below-threshold", (0.3, 0.5), 0.7, 0.0099, False),
                                                ("above-threshold", (0.3, 0.5), 0.7, -0.0101, False), ("zero-heading", (0.0, 0.0), 0.4, 0.0, False)):
        legs = a1_qpos([0, 0, 0])[7:] + rng.normal(0, 0.1, 12)
        out.append(a1_case("walk/" + label, a1_qpos((0.5, -0.4, 0.3), quat([0, 0, 1], 0.3), legs), rng.normal(0, 0.3, 18), 1.3 + 0.25, mode="Walk",
                           gait="Walk", mode_start_time=0.25, position=(0.4, -0.2, 0.0), heading=heading, speed=speed, angvel=angvel,
                           phase=1.7, fp64_only=edge))
    return out


def biped_cases():
    rng = np.random.default_rng(25)
    out = []
    for handstand in (0, 1):
        for k, extra in enumerate((0.0, 0.4)):
            psi = 0.8 - 1.5 * handstand
            q = qmul(quat([0, 0, 1], psi), quat([0, 1, 0], np.pi / 2 if handstand else -np.pi / 2))
            legs = a1_qpos([0, 0, 0])[7:] + rng.normal(0, 0.3, 12)
            lit = {0: 0.0}
            if extra == 0.0:
                lit.update({37: 0.0, 38: 0.0})
            else:
                lit.update({37: np.cos(psi) - np.cos(psi + extra), 38: np.sin(psi) - np.sin(psi + extra)})
            out.append(a1_case(f"biped/{'hand' if handstand else 'foot'}-stand/{k}", a1_qpos((0.1, -0.2, 0.65), q, legs), rng.normal(0, 0.4, 18),
                               0.2, mode="Biped", gait="Trot", handstand=handstand, phase=0.9, params={"Heading": psi + extra}, literal=lit))
    return out


def quadruped_cases():
    rng = np.random.default_rng(26)
    out = []
    for k in range(2):
        q = rng.normal(0, 1, 4)
        v = rng.normal(0, 2.0, 18)
        v[3:6] = rng.normal(0, 6.0, 3)
        legs = a1_qpos([0, 0, 0])[7:] + rng.normal(0, 0.3, 12)
        ctrl = np.array([1.7, -1.4, 1.0, -1.0, 0.999, -2.5, 0.0, 3.0, 0.3, -0.2, 1.0000001, -1.01]) * (1 if k == 0 else -1)
        out.append(a1_case(f"quadruped/tumbling{k}", a1_qpos((0.3, 0.1, 0.7), q / np.linalg.norm(q), legs), v, 0.05, gait="Trot", phase=0.6, ctrl=ctrl,
                           goal=(0.7, -0.4, 0.26), literal={13 + i: 0.8 * float(np.clip(ctrl[i], -1, 1)) for i in range(12)}))
    return out


# ------------------------------------------------------------------------------------------------ HumanoidTrack
def humanoid_cases():
    t = task_of("HumanoidTrack")
    m = t.model
    rng = np.random.default_rng(27)
    kq = np.asarray(m.arrays["key_qpos"], float)
    lo, hi = m.arrays["actuator_ctrlrange"][:, 0], m.arrays["actuator_ctrlrange"][:, 1]
    out = []
    # (clip, reference time, time, keyframe of the pose)
    plan = [(0, 0.5, 0.25, 0), (0, 0.0, 0.5, 15), (0, 0.0, 0.52, 16), (0, 0.0, 4.0 - 0.4 / 30, 119), (0, 0.0, 4.0, 120), (0, 0.0, 5.0, 120),
            (3, 0.75, 0.5, 2), (3, 0.75, 1.25, 15), (3, 0.75, 0.75 + 76.5 / 30, 76), (3, 0.75, 0.75 + 77.25 / 30, 77), (3, 0.75, 4.5, 40),
            (9, 0.0, 0.52, 16), (9, 0.0, 509 / 30 - 0.01, 508), (9, 0.0, 18.0, 509)]
    for clip, ref, time, j in plan:
        start = t.motion_start(clip)
        ri = [start, start + t.MOTION_LENGTHS[clip] - 1, *t.site_ids, *t.mocap_ids]
        v = rng.normal(0, 1.0, m.nv)
        ctrl = rng.uniform(lo - 0.2, hi + 0.2)
        mocap = np.concatenate([np.concatenate([p, [1, 0, 0, 0]]) for p in np.asarray(m.arrays["key_mpos"], float)[start + j].reshape(-1, 3)])
        out.append(Case(f"humanoid/clip{clip}/t{time:.3f}", "HumanoidTrack", np.concatenate([kq[start + j], v]), float(time), mocap, ctrl,
                        residual_int=ri, residual_real=[float(ref)]))
    return out


# ------------------------------------------------------------------------------------------------ the lane tasks
def lane_cases():
    rng = np.random.default_rng(28)
    out = []
    t = task_of("Cartpole")
    for k, theta in enumerate((np.pi - 1e-8, np.pi + 1e-8, 1e-8, 0.3, -2.0, 7.0)):
        pars = list(t.parameters)
        pars[0] = 0.3 * k - 0.5
        out.append(Case(f"cartpole/{k}", "Cartpole", np.array([rng.normal(), theta, rng.normal(), rng.normal()]), 0.1 * k, None,
                        np.array([(-1.4, 0.3, 1.2)[k % 3]]), parameters=pars))
    for name in ("Particle", "ParticleCopy"):
        t = task_of(name)
        for k in range(3):
            mocap = np.array([*rng.uniform(-0.2, 0.2, 2), 0.01, 1, 0, 0, 0])
            out.append(Case(f"{name.lower()}/{k}", name, np.concatenate([rng.uniform(-0.3, 0.3, 2), rng.normal(0, 0.5, 2)]), 0.2 * k, mocap,
                            rng.uniform(-1.2, 1.2, 2), parameters=list(t.parameters)))
    return out


@functools.lru_cache(maxsize=None)
def cases(task=None):
    """every case, evaluated once per session"""
    if task is not None:
        return tuple(c for c in cases() if c.task == task)
    built = flip_cases() + terrain_cases() + gait_cases() + walk_cases() + biped_cases() + quadruped_cases() + humanoid_cases() + lane_cases()
    assert len({c.name for c in built}) == len(built)
    return tuple(finish(c) for c in built)


def census():
    return frozenset(l for c in cases() for l in c.labels)


@functools.lru_cache(maxsize=None)
def sensitivities():
    """{case name: one-ulp sensitivity} of the cases that may run on fp32 rows"""
    return {c.name: sensitivity(c) for c in cases() if not c.fp64_only}


def fp32_excluded():
    """the cases an fp32 row leaves out: a one-ulp move of one input changes an expected entry by more than a tenth of the goal"""
    return frozenset(n for n, s in sensitivities().items() if s > 0.1 * STEP_GOAL)


# the result of fp32_excluded(), held equal to it by tests/test_residual_cases.py so that the GPU module need not repeat the scan:
# an amplitude of exactly 0 (one ulp up the step is no longer zero) and a time exactly on a key (one ulp down the interval is the one before)
FP32_EXCLUDED = frozenset(["gait/Walk/amplitude0", "humanoid/clip3/t1.250"])
