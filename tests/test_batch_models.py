"""A model per environment (mjpcx_set_models_batched, mjcf.variant, set_models of the fleet planners) without a device.

   mjcf.variant against the same change made in the XML: every array and scalar of the two compiled models equal
   the variants of tests/model_variants.py, with the oracle alone: every variant's return differs from the base model's and from every
       other variant's, and no rollout fails -- what the device tests' "a staging that ignored the models" check stands on
   the four fleet planners with set_models on the oracle backend (batch_model_oracle_backend.py) equal E single planners, each created
       on model e, over two plan steps; set_models(None) restores the shared model; a wrong count, a model of another source and the
       three planners with a derivative chain raise"""
import os
import re
import shutil

import numpy as np
import pytest

import model_variants as mv
import step_bank
import task_rows
import test_batch_robust_planner as tr
import test_batch_sample_gradient_planner as tsg
from batch_model_oracle_backend import (ModelBatchCeOracleContext, ModelBatchOracleContext, ModelBatchRobustOracleContext,
                                        ModelBatchSampleGradientOracleContext)
from mujoco_mpc_amd import capi, mjcf
from mujoco_mpc_amd.planners import (GpuBatchCrossEntropyPlanner, GpuBatchGradientPlanner, GpuBatchILQGPlanner, GpuBatchILQSPlanner,
                                     GpuBatchSamplingPlanner, GpuCrossEntropyPlanner, GpuSamplingPlanner)
from mujoco_mpc_amd.task import MODELS_DIR, load_task
from oracle import pyoracle
from oracle_backend import OracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, SEED, T, STEPS = 3, 9, 6, 2


def test_the_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mjpcx.h")).read(), flags=re.S)
    assert re.search(r"\bint mjpcx_set_models_batched\s*\(", src)
    assert "mjpcx_set_models_batched" in capi.EXPORTS
    assert getattr(capi.lib(), "mjpcx_set_models_batched").argtypes is not None
    assert callable(capi.Context.set_models_batched)


# ------------------------------------------------------------------------------------------------- mjcf.variant
def assert_same_model(a, b):
    assert set(a.arrays) == set(b.arrays) and set(a.scalars) == set(b.scalars)
    for k in a.arrays:
        assert np.array_equal(np.asarray(a.arrays[k]), np.asarray(b.arrays[k])), k
    for k in a.scalars:
        assert np.array_equal(np.asarray(a.scalars[k]), np.asarray(b.scalars[k])), k
    assert a.names == b.names and list(a.keyframes) == list(b.keyframes) and set(a.numeric) == set(b.numeric)


@pytest.mark.parametrize("robot", ["a1", "humanoid"])
def test_variant_equals_the_same_change_in_the_xml(robot, tmp_path):
    """one body twice as heavy, with twice the inertia (a power of two: the XML's numbers are then the variant's, bit for bit)"""
    sub, main, edited, body = (("quadruped", "task_flat.xml", "a1_modified.xml", "trunk") if robot == "a1" else
                               ("humanoid", os.path.join("tracking", "task.xml"), "humanoid_modified.xml", "head"))
    shutil.copytree(os.path.join(MODELS_DIR, sub), tmp_path / sub)
    base = mjcf.load_xml(str(tmp_path / sub / main))
    i = base.name2id("body", body)
    mass, inertia = np.array(base.arrays["body_mass"], float), np.array(base.arrays["body_inertia"], float)
    mass[i] *= 2.0
    inertia[i] *= 2.0
    want = mjcf.variant(base, body_mass=mass, body_inertia=inertia)
    assert want.source == base.source and want.meaninertia != base.meaninertia
    # the same in the XML
    path = tmp_path / sub / edited
    text = open(path).read()
    at = text.index(f'<body name="{body}"')
    if robot == "a1":    # an explicit <inertial mass fullinertia>: both doubled
        m = re.compile(r'<inertial mass="([^"]+)"([^>]*?)fullinertia="([^"]+)"', re.S).search(text, at)
        new = '<inertial mass="%r"%sfullinertia="%s"' % (2.0 * float(m.group(1)), m.group(2), " ".join(repr(2.0 * float(x)) for x in m.group(3).split()))
        text = text[:m.start()] + new + text[m.end():]
    else:                # inertia from the geoms: an explicit <inertial> with the compiled frame and the doubled values
        end = text.index(">", at) + 1
        f = lambda v: " ".join(repr(float(x)) for x in v)
        text = (text[:end] + '<inertial pos="%s" quat="%s" mass="%r" diaginertia="%s"/>' % (
            f(base.arrays["body_ipos"][i]), f(base.arrays["body_iquat"][i]), float(mass[i]), f(inertia[i])) + text[end:])
    open(path, "w").write(text)
    got = mjcf.load_xml(str(tmp_path / sub / main))
    assert_same_model(got, want)
    with pytest.raises(ValueError, match="geom_size"):
        mjcf.variant(base, geom_size=base.arrays["geom_size"])
    with pytest.raises(ValueError, match="body_pos"):
        mjcf.variant(base, body_pos=base.arrays["body_pos"])


# ------------------------------------------------------------------------------------------------- the variants of the device tests
@pytest.mark.parametrize("robot", ["a1", "humanoid"])
def test_every_variant_shows_in_the_return(robot):
    """tests/model_variants.py's state, spline and horizon: the oracle's return on every model -- the base, one variant per permitted field
    that is not zero everywhere in the robot's model, the three mixed ones -- differs from every other, and no rollout fails"""
    r = mv.robot(robot)
    models = r.all()
    assert set(r.single) == set(mjcf.VARIANT_FIELDS) - set(mv.ALL_ZERO[robot]) and set(r.mixed) == {"payload", "ice", "weak"}
    for field, fm in r.single.items():      # that field only (and what follows from it), by one factor between 0.5 and 2
        for k in mjcf.VARIANT_FIELDS:
            same = np.array_equal(np.asarray(fm.arrays[k], float), np.asarray(r.base.arrays[k], float))
            assert same == (k != field), (field, k)
        a, b = np.asarray(fm.arrays[field], float).ravel(), np.asarray(r.base.arrays[field], float).ravel()
        ratio = a[a != b] / b[a != b]
        assert np.allclose(ratio, ratio[0], rtol=1e-12) and 0.5 <= ratio[0] <= 2.0 and np.array_equal(a == 0, b == 0), field
    times, nodes = r.spline()
    rets = {}
    for name, fm in models.items():
        ref = pyoracle.rollout_batch(r.packed(fm), step_bank.packed_task(r.task, r.state), r.state.state, r.state.time, r.state.mocap, 1, r.H, len(times),
                                     capi.SPLINE_LINEAR, times, nodes[None], num_threads=1)
        assert not ref["failure"].any(), name
        rets[name] = float(ref["total_return"][0])
    assert len(set(rets.values())) == len(models), rets


def test_an_affine_actuator_bias_shows_in_the_states():
    """actuator_biasprm, zero everywhere in both robots: on tests/models/capsules_bias.xml the variant moves the actuated joint elsewhere
    (the scene's only residual is a constant: the return is 0 on every model, so the states are compared)"""
    task, s, models = mv.bias_scene()
    r = mv.robot("bias_scene")
    assert np.array_equal(np.asarray(models["actuator_biasprm"].arrays["actuator_biasprm"]), 1.5 * np.asarray(models["base"].arrays["actuator_biasprm"]))
    times, nodes = r.spline()
    out = {}
    for name, fm in models.items():
        ref = pyoracle.rollout_batch(r.packed(fm), step_bank.packed_task(task, s), s.state, s.time, None, 1, r.H, len(times), capi.SPLINE_LINEAR, times,
                                     nodes[None], num_threads=1)
        assert not ref["failure"].any(), name
        out[name] = ref["states"][0]
    assert np.max(np.abs(out["base"][-1] - out["actuator_biasprm"][-1])) > 1e-4


# ------------------------------------------------------------------------------------------------- the fleet planners
def fleet_models():
    """the A1 task, three robots: the base model, a payload, ice -- and the Tasks the single planners are created on"""
    task = load_task("QuadrupedFlat")
    task.transition(0.0)
    r = mv.robot("a1")
    models = [task.model, r.mixed["payload"], r.mixed["ice"]]
    tasks = []
    for fm in models:
        t = task_rows.copy_task(task)
        t.model = fm
        tasks.append(t)
    return task, models, tasks


def sampling(task, fleet, seed, factory):
    p = (GpuBatchSamplingPlanner(E, seed=seed, backend_factory=factory) if fleet else GpuSamplingPlanner(seed=seed, backend_factory=factory))
    p.initialize(task.model, task)
    p.num_trajectory_ = 64
    for q in (p.envs if fleet else [p]):
        q.noise_exploration = [0.05, 0.0]
    p.allocate()
    return p


def cross_entropy(task, fleet, seed, factory):
    p = (GpuBatchCrossEntropyPlanner(E, seed=seed, backend_factory=factory) if fleet else GpuCrossEntropyPlanner(seed=seed, backend_factory=factory))
    p.initialize(task.model, task)
    p.num_trajectory_, p.n_elite_, p.explore_fraction_, p.std_initial_ = 63, 6, 0.1, 0.05
    p.allocate()
    return p


def same_sampling(batch, e, p, where):
    b = batch.envs[e]
    assert batch.winners[e] == p.winner, where
    assert (b.best_return, b.nominal_return, b.improvement) == (p.best_return, p.nominal_return, p.improvement), where
    assert np.array_equal(b.policy.plan.times(), p.policy.plan.times()) and np.array_equal(b.policy.plan.values(), p.policy.plan.values()), where


def same_cross_entropy(batch, e, p, where):
    b = batch.envs[e]
    assert b.trajectory_order == p.trajectory_order and b.improvement == p.improvement, where
    assert np.array_equal(b.policy.plan.times(), p.policy.plan.times()) and np.array_equal(b.policy.plan.values(), p.policy.plan.values()), where
    assert np.array_equal(b.variance, p.variance), where


# kind -> (the fleet, a single planner, the comparison of member e with the single planner); factories: (fleet's, single's) backend, None = the device's
KINDS = {
    "sampling": (lambda task, f: sampling(task, True, SEED, f), lambda task, e, f: sampling(task, False, SEED + e, f), same_sampling),
    "cross_entropy": (lambda task, f: cross_entropy(task, True, SEED, f), lambda task, e, f: cross_entropy(task, False, SEED + e, f), same_cross_entropy),
    "robust": (lambda task, f: tr.fleet_planner(task, 5, 4, factory=f), lambda task, e, f: tr.single_planner(task, tr.SEED + e, 5, 4, factory=f),
               lambda batch, e, p, where: tr.assert_member_equals_planner(batch.envs[e], p, where)),
    "sample_gradient": (lambda task, f: tsg.configure(tsg.GpuBatchSampleGradientPlanner(E, seed=tsg.SEED, backend_factory=f), task, 5),
                        lambda task, e, f: tsg.configure(tsg.GpuSampleGradientPlanner(seed=tsg.SEED + e, backend_factory=f), task, 5),
                        tsg.assert_member_equals_planner),
}
ORACLE = {
    "sampling": (lambda t: ModelBatchOracleContext(t, threads=8), lambda t: OracleContext(t, threads=8)),
    "cross_entropy": (lambda t: ModelBatchCeOracleContext(t, threads=8), lambda t: OracleContext(t, threads=8)),
    "robust": (lambda t: ModelBatchRobustOracleContext(t, threads=8), tr.backend),
    "sample_gradient": (lambda t: ModelBatchSampleGradientOracleContext(t, threads=8), tsg.backend),
}


def run_fleet_with_models(kind, factories=(None, None), horizon=T, steps=STEPS):
    """the fleet planner with set_models against one single planner per environment created on that environment's model"""
    make_fleet, make_single, same = KINDS[kind]
    task, models, tasks = fleet_models()
    batch = make_fleet(task, factories[0])
    batch.set_models(models)
    singles = [make_single(tasks[e], e, factories[1]) for e in range(E)]
    for p in [batch] + singles:
        p.reset(horizon)
    states = [tr.initial_states(task)[0] for _ in range(E)]        # ONE state for every robot: the models tell them apart (and the seeds)
    for step in range(steps):
        batch.set_states(states)
        batch.optimize_policy(horizon)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(horizon)
            same(batch, e, p, (kind, step, e))
            tr.assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (kind, step, e))
        tr.step_along(task, states, singles)
    return batch, singles, task, models


@pytest.mark.parametrize("kind", list(KINDS))
def test_fleet_with_models_is_one_planner_per_model(kind):
    batch, singles, task, models = run_fleet_with_models(kind, ORACLE[kind])
    ctxs = [batch.ctx] + ([batch.delegate.ctx] if kind == "robust" else [])
    for ctx in ctxs:                                                   # (Robust: both contexts were given the models)
        assert len(ctx.model_pushes) == 1 and len(ctx.model_pushes[0]) == E
        for pm, fm in zip(ctx.model_pushes[0], models):              # packed as Task.packed_model packs: the planning timestep and integrator
            assert pm.struct.timestep == batch.ctx.pm.struct.timestep and pm.struct.integrator == batch.ctx.pm.struct.integrator
            assert np.array_equal(pm.keep["body_mass"], np.asarray(fm.arrays["body_mass"], float).ravel())
    # the models decide the plan: three robots from one state are three problems
    assert len({batch.best_trajectory(e).total_return for e in range(E)}) == E


def test_set_models_checks_and_reverts():
    task, models, tasks = fleet_models()
    factory = ORACLE["sampling"]
    batch = sampling(task, True, SEED, factory[0])
    with pytest.raises(ValueError, match="2 models for 3 environments"):
        batch.set_models(models[:2])
    other = load_task("Cartpole").model
    with pytest.raises(ValueError, match="environment 1"):
        batch.set_models([models[0], other, models[2]])
    assert batch.ctx.env_models is None
    state = tr.initial_states(task)[0]

    def nominal_returns():
        batch.reset(T)
        batch.set_states([state] * E)
        return [tj.total_return for tj in batch.nominal_trajectory(T)]
    shared = nominal_returns()
    assert len(set(shared)) == 1
    batch.set_models(models)
    unlike = nominal_returns()
    assert unlike[0] == shared[0] and len(set(unlike)) == E
    batch.allocate()                                   # a new context: the models are pushed again
    assert batch.ctx.env_models is not None and nominal_returns() == unlike
    batch.set_models(None)
    assert batch.ctx.env_models is None and nominal_returns() == shared
    # allocate on a factory that hands out the SAME context: the models it holds are not built again
    batch.set_models(models)
    keep = batch.ctx
    batch._backend_factory = lambda t: keep
    pushes = len(keep.model_pushes)
    batch.allocate()
    assert batch.ctx is keep and len(keep.model_pushes) == pushes
    # the planners with a derivative chain say that theirs is a follow-up
    for cls in (GpuBatchGradientPlanner, GpuBatchILQGPlanner, GpuBatchILQSPlanner):
        with pytest.raises(NotImplementedError, match="derivative chain"):
            cls(E).set_models(models)


def test_robust_set_models_is_all_or_nothing_over_both_contexts():
    task, models, tasks = fleet_models()
    batch = tr.fleet_planner(task, 5, 4, factory=ORACLE["robust"][0])
    batch.set_models(models)
    first = (batch.ctx.env_models, batch.delegate.ctx.env_models)
    assert first[0] is not None and first[1] is not None
    accept = batch.delegate.ctx.set_models_batched

    def refuse(packed):
        raise capi.MjpcxError.__new__(capi.MjpcxError)
    batch.delegate.ctx.set_models_batched = refuse             # the second context refuses: the first goes back to what it held
    with pytest.raises(capi.MjpcxError):
        batch.set_models([models[0], models[2], models[1]])
    batch.delegate.ctx.set_models_batched = accept
    for held in (batch._models, batch.delegate._models):
        assert len(held) == E and all(a is b for a, b in zip(held, models))
    for ctx, was in zip((batch.ctx, batch.delegate.ctx), first):
        assert [pm.keep["body_mass"].tolist() for pm in ctx.env_models] == [pm.keep["body_mass"].tolist() for pm in was]
