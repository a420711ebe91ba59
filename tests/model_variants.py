"""The physically unlike robots of the fleet-model tests (tests/test_batch_models.py on the CPU, tests/test_gpu_batch_models.py on the device),
defined once: per robot one variant per field the models of a fleet may differ in (mjcf.VARIANT_FIELDS) -- it differs from the base
model in that field only, by one factor between 0.5 and 2 on the entries named below -- and three mixed ones: a payload, ice, weak motors.

A model may change a permitted field's values, not which of its entries are zero (mjpcx_set_models_batched): a field that is zero
everywhere in a robot's model cannot differ in a fleet of that robot, so it has no variant here. ALL_ZERO lists those fields per robot,
and single_field() asserts that exactly they are without one -- nothing else may be left out.

The derived quantities (body_subtreemass, body_invweight0, dof_invweight0, tendon_invweight0, meaninertia) follow through mjcf.variant."""
import numpy as np

import step_bank
from mujoco_mpc_amd import mjcf

ALL_ZERO = {"a1": ("jnt_stiffness", "actuator_biasprm"), "humanoid": ("dof_frictionloss", "actuator_biasprm")}

# field -> (factor, columns it applies to; None: every entry). Where a column is named the others have a meaning a factor would break:
# solref = (timeconst, dampratio), solimp = (dmin, dmax, width, midpoint, power), gainprm = (kp, -, -) of which only kp is non-zero.
FACTORS = {
    "body_mass": (1.3, None), "body_inertia": (1.5, None), "body_ipos": (1.25, None),
    "dof_armature": (2.0, None), "dof_damping": (0.5, None), "dof_frictionloss": (2.0, None), "jnt_stiffness": (2.0, None),
    "actuator_gear": (0.8, None), "actuator_gainprm": (0.7, (0,)), "actuator_biasprm": (0.5, None),
    "geom_friction": (0.5, (0,)), "geom_solref": (1.5, (0,)), "geom_solimp": (0.8, (0, 1)),
}


def scaled(fm, field, factor, cols=None, rows=None):
    a = np.array(fm.arrays[field], dtype=float, copy=True)
    v = a.reshape(a.shape[0], -1)
    r = slice(None) if rows is None else rows
    if cols is None:
        v[r] *= factor
    else:
        for c in cols:
            v[r, c] *= factor
    return v.reshape(a.shape)


def single_field(robot, fm):
    """{field: the model that differs from fm in that field only}"""
    out = {}
    for field in mjcf.VARIANT_FIELDS:
        if not np.any(np.asarray(fm.arrays[field], float)):
            assert field in ALL_ZERO[robot], (robot, field)
            continue
        assert field not in ALL_ZERO[robot], (robot, field)
        factor, cols = FACTORS[field]
        assert 0.5 <= factor <= 2.0
        out[field] = mjcf.variant(fm, **{field: scaled(fm, field, factor, cols)})
    return out


def mixed(robot, fm):
    """payload: the trunk a half heavier, with its inertia; ice: a fifth of the sliding friction everywhere; weak motors: 60 % of the
    actuators' strength (the A1's position gain, the Humanoid's gear)"""
    trunk = [int(np.flatnonzero(np.asarray(fm.arrays["body_dofnum"]) > 0)[0])]
    weak = dict(actuator_gainprm=scaled(fm, "actuator_gainprm", 0.6, (0,))) if robot == "a1" else dict(actuator_gear=scaled(fm, "actuator_gear", 0.6))
    return {
        "payload": mjcf.variant(fm, body_mass=scaled(fm, "body_mass", 1.5, rows=trunk), body_inertia=scaled(fm, "body_inertia", 1.5, rows=trunk)),
        "ice": mjcf.variant(fm, geom_friction=scaled(fm, "geom_friction", 0.2, (0,))),
        "weak": mjcf.variant(fm, **weak),
    }


class Robot:
    """a robot of the step bank with its variants, the state the fleets start from and the spline and horizon the variants are told apart by"""

    def __init__(self, name):
        self.name = name
        if name == "a1":
            self.bank = step_bank.a1_bank()
            self.state = self.bank.states[STATE["a1"]]
            self.H = 6
        else:
            self.bank = step_bank.humanoid_bank()
            self.state = [s for s in self.bank.states if s.label.startswith("clip9/key")][STATE["humanoid"]]
            self.H = 5
        self.task = self.bank.task
        self.base = self.task.model
        self.single = single_field(name, self.base)
        self.mixed = mixed(name, self.base)

    def packed(self, fm, differentiable=False):
        """fm packed as Task.packed_model packs the task's model: the planning timestep and integrator"""
        from mujoco_mpc_amd.cstructs import PackedModel
        ref = self.base
        return PackedModel(fm, timestep=ref.get_number("agent_timestep", ref.timestep),
                           integrator=int(ref.get_number("agent_integrator", ref.integrator)), differentiable=differentiable)

    def all(self):
        """name -> model: the base, every single-field variant, the mixed ones"""
        return {"base": self.base, **self.single, **self.mixed}

    def spline(self, P=3, seed=3, std=0.3):
        """one spline, node times over the horizon from the state's clock (P x nu values inside the control range)"""
        m = self.base
        dt = m.get_number("agent_timestep", m.timestep)
        lo, hi = np.asarray(m.arrays["actuator_ctrlrange"], float).reshape(-1, 2).T
        times = self.state.time + np.arange(P) * ((self.H - 1) * dt / (P - 1))
        return times, np.clip(np.random.default_rng(seed).normal(0, std, (P, m.nu)), lo, hi)


# which state of the bank a robot's fleets start from: one in which every field shows in the return within the horizon (a foot that slides
# for the friction, joints that move for damping and friction loss) -- settled with the oracle, tests/test_batch_models.py asserts it
STATE = {"a1": 0, "humanoid": 0}

_ROBOTS = {}


def robot(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = BiasScene() if name == "bias_scene" else Robot(name)
    return _ROBOTS[name]


# ---- actuator_biasprm: zero everywhere in both robots, so it is shown on a small generic contact model with an affine bias instead
def bias_scene():
    """tests/models/capsules_bias.xml (capsules_small.xml with an affine bias of three non-zero parameters on its actuator): the task, a
    state, and the models base / actuator_biasprm (that field only, x 1.5)"""
    import os
    from mujoco_mpc_amd.task import Task
    fm = mjcf.load_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "capsules_bias.xml"))
    task = Task(name="scene", residual_id=0, model=fm).reset()
    q, v = fm.arrays["qpos0"].copy(), np.zeros(fm.nv)
    q[14 + 2], v[12 + 2], q[fm.nq - 2], v[0], v[fm.nv - 1] = 1.0 + 0.0995, -0.5, 0.6, 0.3, 0.8      # (tests/test_gpu_batch_ilqg_step.py's scene; the actuated joint moving)
    state = step_bank.BankState("bias_scene", np.concatenate([q, v]), 0.05, None)
    assert np.all(np.asarray(fm.arrays["actuator_biasprm"], float) != 0)
    return task, state, {"base": fm, "actuator_biasprm": mjcf.variant(fm, actuator_biasprm=scaled(fm, "actuator_biasprm", 1.5))}


class BiasScene(Robot):
    """bias_scene() with a Robot's interface (robot("bias_scene")): one single-field variant, no mixed ones"""

    def __init__(self):
        self.name, self.H = "bias_scene", 6
        self.task, self.state, models = bias_scene()
        self.base = self.task.model
        self.single, self.mixed = {"actuator_biasprm": models["actuator_biasprm"]}, {}
