"""Step-parity harness (test infrastructure, like oracle_backend.py; not a conftest): deterministic banks of pre-step states, one mj_step of
every bank state compared element by element with the oracle, and the oracle's constraint census of each pre-step state.

A bank state is (state, time, mocap, frozen residual state). Banks are built on the CPU from the repository's models and the oracle, cached
for the session, and keep only states whose fp64 oracle step does not fail. One step = a rollout of horizon 2 with one zero-order node,
STEP_CANDIDATES candidates per state: zero control, both saturated ends, and random controls that reach past the ends (clamped). What is
compared: states, actions, times, residual, costs, trace, total return and the failure flags, |d - o| <= tol (1 + |o|).

The census of a pre-step state is exact for the step: one mj_step's constraint set is fixed by the state it starts from."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from mujoco_mpc_amd.task import load_task
from oracle import pyoracle

FIELDS = ("states", "actions", "times", "residual", "costs", "trace")
STEP_CANDIDATES = 16
K_TREE_MAX_CONE = 16            # csrc/wave_tree.h kTreeMaxCone: cones the tree kernel's first pass keeps in LDS
LIMB_HANDED_ON = 0x40000000     # failure bit of a candidate the limb kernel did not cover (under MJPCX_LIMB_NO_FALLBACK it stays set)
EFC_FRICTION, EFC_LIMIT, EFC_TENDON = 0, 1, 5   # oracle/contact.inc


def mocap7(mpos):
    return np.concatenate([np.concatenate([p, [1, 0, 0, 0]]) for p in np.asarray(mpos).reshape(-1, 3)])


@dataclass
class BankState:
    label: str
    state: np.ndarray
    time: float
    mocap: np.ndarray | None
    residual_int: list = field(default_factory=list)
    residual_real: list = field(default_factory=list)


@dataclass
class Bank:
    name: str
    task: object
    states: list
    census: list = None          # per state: the set of constraint features of its step (see census())


def packed_task(task, s):
    """the task packed with the bank state's frozen residual state (what mjpcx_set_residual_state gives a context)"""
    ri, rr = task.residual_int, task.residual_real
    task.residual_int, task.residual_real = list(s.residual_int), list(s.residual_real)
    try:
        return task.packed()
    finally:
        task.residual_int, task.residual_real = ri, rr


def step_controls(nu, lo, hi, seed, n=STEP_CANDIDATES):
    """zero, the lower and the upper end, then random controls spread 10 % past both ends (the rollout clamps them)"""
    rng = np.random.default_rng(seed)
    span = hi - lo
    u = [np.zeros(nu), lo.copy(), hi.copy()]
    u += [rng.uniform(lo - 0.1 * span, hi + 0.1 * span) for _ in range(n - 3)]
    return np.array(u)[:, None, :]          # [n, P = 1, nu]


def controls_for(task, k):
    r = np.asarray(task.model.arrays["actuator_ctrlrange"], float).reshape(-1, 2)
    return step_controls(task.model.nu, r[:, 0], r[:, 1], seed=1000 + k)


def oracle_step(pm, task, s, nodes):
    return pyoracle.rollout_batch(pm, packed_task(task, s), s.state, s.time, s.mocap, len(nodes), 2, 1, 0, np.array([s.time]), nodes,
                                  num_threads=4)


def _oracle_ok(pm, task, s):
    ref = oracle_step(pm, task, s, controls_for(task, 0)[:3])
    return not ref["failure"].any() and all(np.all(np.isfinite(ref[f])) for f in FIELDS)


def _bank(name, task, states):
    pm = task.packed_model()
    kept = [s for s in states if _oracle_ok(pm, task, s)]
    b = Bank(name, task, kept)
    b.census = [census(task, s) for s in kept]
    return b


# ----------------------------------------------------------------------------------------------------------------------- census
def _legs(task):
    """per geom, the child of the A1's trunk the geom hangs under (-1: the trunk itself or a body outside the robot)"""
    m = task.model
    parent = m.arrays["body_parentid"]
    trunk = next(b for b in range(m.nbody) if m.arrays["body_dofnum"][b] == 6)

    def leg_of(b):
        while b > 0 and parent[b] != trunk:
            b = parent[b]
        return int(b) if b > 0 else -1
    return [leg_of(int(b)) for b in m.arrays["geom_bodyid"]]


def state_features(task, state, time, mocap, legs=None, ph=None):
    """the constraint features of one step from (state, time, mocap), by the oracle's own contact and row lists:
    floor (a contact with a static geom), moving (a contact between two moving geoms), tendon (an active fixed-tendon limit row),
    joint_limit, cones>16 (more pyramidal / elliptic cones than kTreeMaxCone), friction_loss; for the A1 (legs given) also
    leg_leg (geoms of two different legs) and hip_cyl (a hip cylinder against a geom of a leg)."""
    m = task.model
    if ph is None:
        ph = pyoracle.Physics(task.packed_model())
    ph.set_state(state[:m.nq], state[m.nq:], float(time), mocap)
    ph.forward()
    static = [int(b) == 0 or m.arrays["body_mocapid"][int(b)] >= 0 for b in m.arrays["geom_bodyid"]]
    gt = m.arrays["geom_type"]
    f = set()
    nc = int(ph.get("ncon")[0])
    cones = 0
    for r in ph.get("contact").reshape(-1, 11)[:nc]:
        g1, g2 = int(r[7]), int(r[8])
        f.add("moving" if not static[g1] and not static[g2] else "floor")
        if int(r[9]) > 1:
            cones += 1
        if legs is not None and legs[g1] >= 0 and legs[g2] >= 0:
            if legs[g1] != legs[g2]:
                f.add("leg_leg")
            if 5 in (gt[g1], gt[g2]):          # MJPCX_GEOM_CYLINDER: the A1's hips
                f.add("hip_cyl")
    if cones > K_TREE_MAX_CONE:
        f.add("cones>16")
    if int(ph.get("nefc")[0]):
        types = set(ph.get("efc_type").astype(int).tolist())
        for t, name in ((EFC_TENDON, "tendon"), (EFC_LIMIT, "joint_limit"), (EFC_FRICTION, "friction_loss")):
            if t in types:
                f.add(name)
    return f


def census(task, s):
    legs = _legs(task) if task.name == "QuadrupedFlat" else None
    return state_features(task, s.state, s.time, s.mocap, legs)


def counts(features):
    """{feature: number of states that have it} over an iterable of feature sets"""
    out = {}
    for f in features:
        for k in f:
            out[k] = out.get(k, 0) + 1
    return dict(sorted(out.items()))


def contact_census(task, mocap, states):
    """Which kinds of contact the oracle sees along recorded A1 rollouts (states [n, H, nq + nv]): per candidate, whether some step carries a
    contact between geoms of two different LEGS, and whether one involves a hip CYLINDER and a geom of another moving body -- the cases
    the quad kernel's solver pays most for (super-leg elimination, the thin-solid narrow phase). Legs: the chains below the free-joint body."""
    legs = _legs(task)
    ph = pyoracle.Physics(task.packed_model())
    leg_leg, hip_cyl = set(), set()
    for k in range(states.shape[0]):
        for t in range(states.shape[1]):
            f = state_features(task, states[k, t], 0.0, mocap, legs, ph)
            if "leg_leg" in f:
                leg_leg.add(k)
            if "hip_cyl" in f:
                hip_cyl.add(k)
    return leg_leg, hip_cyl


def humanoid_census(task, mocap, states, times, lds_cones=K_TREE_MAX_CONE):
    """What the oracle sees along recorded Humanoid rollouts (states [n, H, nq + nv]): candidates with a contact between two MOVING bodies
    (self-collision: frictionless rows that couple two limbs), with an active fixed-tendon limit row (the hamstrings), and with more
    pyramidal cones at one step than the tree kernel's LDS list holds (csrc/wave_tree.h kTreeMaxCone: the rest go through its HBM slab)."""
    assert lds_cones == K_TREE_MAX_CONE
    ph = pyoracle.Physics(task.packed_model())
    selfc, tendon, beyond = set(), set(), set()
    for k in range(states.shape[0]):
        for t in range(states.shape[1]):
            f = state_features(task, states[k, t], times[k, t], mocap, None, ph)
            if "moving" in f:
                selfc.add(k)
            if "tendon" in f:
                tendon.add(k)
            if "cones>16" in f:
                beyond.add(k)
    return selfc, tendon, beyond


# ----------------------------------------------------------------------------------------------------------------------- banks
_FOLDED = [-0.04934, -0.00198, 0.032594, 0.351929, -0.166098, 0.001753, 0.92117, -0.571485, 0.278631, -0.418609, 0.178522, 0.04022,
           0.050714, 0.63989, -0.043285, 0.662039, 0.162139, 0.387659, -0.046413, 0.214907, 0.638488, 0.143949, 0.316314, -0.489671,
           -0.674248, 0.724606, -0.506946, -0.298564]   # a folded body pressed into the floor: 36 contacts (tests/test_gpu_humanoid.py)


def _clip(t, mode, ref_time, time):
    """the tracking task on clip `mode` whose reference started at ref_time, at `time`: (mocap, residual_int, residual_real)"""
    t.current_mode, t.reference_time = mode, ref_time
    e = t.transition(time, mode=mode)
    return mocap7(e["mocap_pos"]), list(t.residual_int), list(t.residual_real)


@functools.lru_cache(maxsize=None)
def humanoid_bank():
    t = load_task("HumanoidTrack")
    m = t.model
    pm = t.packed_model()
    nq, nu = m.nq, m.nu
    kq, kv = np.asarray(m.arrays["key_qpos"], float), np.asarray(m.arrays["key_qvel"], float)
    rng = np.random.default_rng(7)
    out = []
    # keyframes of all ten clips, three per clip, each clip's reference started at its own time
    for mode in range(10):
        start, n = t.motion_start(mode), t.MOTION_LENGTHS[mode]
        ref = 0.25 * mode
        for j in (0, n // 2, n - 2):
            time = ref + j / t.K_FPS
            mocap, ri, rr = _clip(t, mode, ref, time)
            out.append(BankState(f"clip{mode}/key{j}", np.concatenate([kq[start + j], kv[start + j]]), time, mocap, ri, rr))
    # mid-flight: 12 steps of an oracle rollout under random controls from the first keyframe of every clip
    for mode in range(10):
        s0 = out[3 * mode]
        H = 12
        nodes = np.clip(rng.normal(0, 0.5, (1, 1, nu)), -1, 1)
        r = pyoracle.rollout_batch(pm, packed_task(t, s0), s0.state, s0.time, s0.mocap, 1, H, 1, 0, np.array([s0.time]), nodes)
        time = float(r["times"][0, -1])
        mocap, ri, rr = _clip(t, mode, 0.25 * mode, time)
        out.append(BankState(f"clip{mode}/flight", r["states"][0, -1].copy(), time, mocap, ri, rr))
    # folding and spinning: a spinning crouch under near-random controls (the body folds, limbs touch, the hamstrings reach their limits)
    mocap, ri, rr = _clip(t, 4, 0.0, 0.0)
    e_q = kq[t.motion_start(4)]
    v = np.zeros(27)
    v[3:6] = [1.5, -1.0, 0.5]
    s0 = BankState("spin", np.concatenate([e_q, v]), 0.0, mocap, ri, rr)
    N, H = 6, 60
    nodes = np.clip(np.random.default_rng(9).normal(0, 0.8, (N, 1, nu)), -1, 1)
    r = pyoracle.rollout_batch(pm, packed_task(t, s0), s0.state, 0.0, mocap, N, H, 1, 0, np.array([0.0]), nodes)
    for c in range(N):
        for k in (20, 35, 50, 59):
            if not r["failure"][c]:
                out.append(BankState(f"spin{c}/step{k}", r["states"][c, k].copy(), float(r["times"][c, k]), mocap, ri, rr))
    # a folded body pressed into the floor (more than 16 cones: the tree kernel's second pass), as it is and perturbed
    mocap, ri, rr = _clip(t, 0, 0.0, 0.0)
    q = np.array(_FOLDED)
    q[3:7] /= np.linalg.norm(q[3:7])
    out.append(BankState("folded", np.concatenate([q, np.zeros(27)]), 0.0, mocap, ri, rr))
    for k in range(3):
        q2 = q.copy()
        q2[7:] += rng.normal(0, 0.05, nq - 7)
        q2[2] -= 0.01 * k
        out.append(BankState(f"folded/{k}", np.concatenate([q2, rng.normal(0, 0.3, 27)]), 0.0, mocap, ri, rr))
    # the "far" cases of tools/fuzz_humanoid.py: folded limbs, a tilted trunk, fast joints
    for k in range(8):
        mode = int(rng.integers(0, 10))
        time = float(rng.uniform(0, 1.5))
        q = kq[t.motion_start(mode)].copy()
        q[7:] += rng.normal(0, 0.6, nq - 7)
        quat = q[3:7] + rng.normal(0, 0.4, 4)
        q[3:7] = quat / np.linalg.norm(quat)
        q[2] += rng.uniform(-0.3, 0.3)
        v = kv[t.motion_start(mode)] + rng.normal(0, 2.0, 27)
        mocap, ri, rr = _clip(t, mode, 0.0, time)
        out.append(BankState(f"far{k}/clip{mode}", np.concatenate([q, v]), time, mocap, ri, rr))
    return _bank("HumanoidTrack", t, out)


def _a1_residual(t, mode, gait, mode_start):
    ri, rr = list(t.residual_int), list(t.residual_real)
    ri[0], ri[8] = mode, gait
    rr[0] = mode_start
    return ri, rr


@functools.lru_cache(maxsize=None)
def a1_bank():
    """home, a trot, falling, tumbling, tangled legs and random states in the style of tools/fuzz_quad.py; the five residual modes and the
    gaits spread over the states (frozen residual state: mode residual_int[0], gait residual_int[8], mode start time residual_real[0])"""
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    pm = t.packed_model()
    home = np.asarray(t.model.keyframes["home"]["qpos"], float)
    rng = np.random.default_rng(11)
    base = []   # (label, state, time, goal x, goal y)
    base.append(("home", np.concatenate([home, np.zeros(18)]), 0.0, 0.3, 0.0))
    # a trot: oracle rollouts under smooth random controls from home; falling: dropped from a height; tumbling: spun in the air
    s_home = BankState("home", np.concatenate([home, np.zeros(18)]), 0.0, None, *_a1_residual(t, 0, 2, 0.0))
    mocap0 = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
    N, H = 4, 40
    nodes = np.clip(rng.normal(0, 0.3, (N, 1, 12)), -1, 1)
    r = pyoracle.rollout_batch(pm, packed_task(t, s_home), s_home.state, 0.0, mocap0, N, H, 1, 0, np.array([0.0]), nodes)
    for c in range(N):
        base.append((f"trot{c}", r["states"][c, 10 + 9 * c].copy(), float(r["times"][c, 10 + 9 * c]), 0.3, 0.0))
    for k in range(3):
        q = home.copy()
        q[2] += 0.15 + 0.1 * k
        quat = np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.3, 4)
        q[3:7] = quat / np.linalg.norm(quat)
        v = np.zeros(18)
        v[2] = -1.5 - k
        base.append((f"falling{k}", np.concatenate([q, v]), 0.1 * k, 0.0, 0.5))
    for k in range(3):
        q = home.copy()
        q[2] += 0.1
        v = rng.normal(0, 1.0, 18)
        v[3:6] = rng.normal(0, 6.0, 3)
        base.append((f"tumbling{k}", np.concatenate([q, v]), 0.2, -0.5, 0.0))
    # tangled legs: large-noise rollouts (std 1 on the controls) fold the legs into each other
    N, H = 6, 50
    nodes = np.clip(rng.normal(0, 1.0, (N, 1, 12)), -1, 1)
    r = pyoracle.rollout_batch(pm, packed_task(t, s_home), s_home.state, 0.0, mocap0, N, H, 1, 0, np.array([0.0]), nodes)
    for c in range(N):
        for k in (25, 49):
            if not r["failure"][c]:
                base.append((f"tangled{c}/step{k}", r["states"][c, k].copy(), float(r["times"][c, k]), 0.3, 0.0))
    # random states (tools/fuzz_quad.py): trunk poses and heights, legs far from home, fast joints
    for case in range(14):
        q = home.copy()
        q[0:2] += rng.normal(0, 0.3, 2)
        q[2] += rng.uniform(-0.12, 0.25)
        quat = np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.25 if case % 3 else 0.6, 4)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.normal(0, 0.35 if case % 4 else 0.9, 12)
        v = rng.normal(0, 0.5 if case % 5 else 2.5, 18)
        base.append((f"random{case}", np.concatenate([q, v]), 0.01 * case, rng.normal(0, 1.0), rng.normal(0, 1.0)))
    out = []
    for i, (label, state, time, gx, gy) in enumerate(base):
        mode, gait = i % 5, (i // 5) % 5
        mocap = np.array([gx, gy, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
        ri, rr = _a1_residual(t, mode, gait, max(time - 0.05 * (i % 4), 0.0))
        out.append(BankState(f"{label}/mode{mode}", state, time, mocap, ri, rr))
    return _bank("QuadrupedFlat", t, out)


@functools.lru_cache(maxsize=None)
def lane_bank(name, n=12):
    """random states of a small model of the lane kernels (Cartpole, Particle: no frozen residual state)"""
    t = load_task(name)
    m = t.model
    rng = np.random.default_rng(3 if name == "Cartpole" else 5)
    out = []
    for k in range(n):
        q = rng.uniform(-1.5, 1.5, m.nq) * (np.pi if name == "Cartpole" else 0.2)
        v = rng.normal(0, 2.0 if name == "Cartpole" else 0.5, m.nv)
        mocap = np.concatenate([np.concatenate([rng.uniform(-0.2, 0.2, 2), [0.01], [1, 0, 0, 0]]) for _ in range(m.nmocap)]) if m.nmocap else None
        out.append(BankState(f"{name.lower()}{k}", np.concatenate([q, v]), float(rng.uniform(0, 2)), mocap))
    return _bank(name, t, out)


# ----------------------------------------------------------------------------------------------------------------------- comparison
@dataclass
class StepReport:
    worst: float = 0.0              # max |d - o| / (1 + |o|) over everything compared
    where: str = ""                 # the state, candidate, field and element of the worst
    failures: list = field(default_factory=list)   # (ratio to tol, message) of every state that missed tol
    per_state: list = field(default_factory=list)  # worst per state (nan: nothing compared)
    compared: list = field(default_factory=list)   # per state: candidates compared
    ratio: float = 0.0              # worst / tol


def compare_step(label, got, ref, tol, cands):
    """worst relative error over the candidates `cands` and a message naming state, candidate, field and element of the worst"""
    worst, where = 0.0, ""
    gf, of = np.asarray(got["failure"]) != 0, np.asarray(ref["failure"]) != 0
    if not np.array_equal(gf[cands], of[cands]):
        c = int(cands[np.flatnonzero(gf[cands] != of[cands])[0]])
        return np.inf, f"{label}: candidate {c}: failure flag {int(gf[c])}, oracle {int(of[c])}", False
    for name in FIELDS + ("total_return",):
        g, o = np.asarray(got[name], float)[cands], np.asarray(ref[name], float)[cands]
        e = np.abs(g - o) / (1 + np.abs(o))
        e = np.where(np.isnan(e), np.inf, e)
        i = int(np.argmax(e))
        if e.size and e.flat[i] > worst:
            idx = np.unravel_index(i, e.shape)
            worst = float(e.flat[i])
            where = (f"{label}: candidate {int(cands[idx[0]])}, {name}{list(int(x) for x in idx[1:])}: device {g[idx]!r}, oracle {o[idx]!r}, "
                     f"error {worst:.3e}")
    ok = worst <= tol
    return worst, where, ok


def run_bank(bank, step, tol, pm=None):
    """every bank state through `step(k, s, nodes) -> dict of FIELDS, total_return, failure[, kept]` against the fp64 oracle on `pm` (default:
    the bank task's planning model). A step may return a 'kept' mask: the candidates to compare (the limb kernel's covered ones)."""
    t = bank.task
    pm = t.packed_model() if pm is None else pm
    rep = StepReport()
    for k, s in enumerate(bank.states):
        nodes = controls_for(t, k)
        ref = oracle_step(pm, t, s, nodes)
        got = step(k, s, nodes)
        mask = np.asarray(got.get("kept", np.ones(len(nodes), bool)), bool)
        cands = np.flatnonzero(mask)
        rep.compared.append(len(cands))
        if not len(cands):
            rep.per_state.append(np.nan)
            continue
        worst, where, ok = compare_step(s.label, got, ref, tol, cands)
        rep.per_state.append(worst)
        if worst > rep.worst:
            rep.worst, rep.where = worst, where
        if not ok:
            rep.failures.append((worst / tol, where))
    rep.ratio = rep.worst / tol
    return rep


def covered_counts(bank, rep, only=None):
    """census counts over the states at least one of whose candidates was compared (only: restrict to these features)"""
    c = counts(f for f, n in zip(bank.census, rep.compared) if n > 0)
    return {k: v for k, v in c.items() if only is None or k in only}
