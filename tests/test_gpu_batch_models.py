"""-m gpu: a model per environment (mjpcx_set_models_batched) on every kernel a contact-family context rolls out on.

Every fleet starts its environments from ONE state with ONE nominal spline and DIFFERENT models (tests/model_variants.py), and every
case first rolls one shared spline out for all of them and asserts that the environments' returns differ pairwise: a staging that
ignored the models would not get that far.

   a batched call after set_models_batched <-> E contexts, each CREATED on model e (the code path there was before), given the plain
       call with seed + e: np.array_equal on the returns, the failure flags and all six Trajectory buffers of every candidate
   every field a fleet's models may differ in, one environment per single-field variant, against the oracle on that environment's
       model at the bounds of tests/test_gpu_batch.py: quad kernel 1e-9 (1 + |x|), tree and wave kernels 1e-6, fp32 returns 2e-3
   the hand-on: candidates the quad / limb kernel hands to rollout_tree_kernel are rolled out on their environment's model too
   semantics on the registered-model kernel of the A1; models together with task rows; the four fleet planners with set_models"""
import numpy as np
import pytest

import model_variants as mv
import step_bank
import task_rows
import test_batch_models as cpu
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle
from test_gpu_batch import context, err, everything

pytestmark = pytest.mark.gpu
FIELDS = ("states", "actions", "times", "residual", "costs", "trace")
ALL = ("total_return", "failure") + FIELDS
P, SEED = 3, 31
MIXED = ("base", "payload", "ice", "weak")


class ModelFleet:
    """E environments of one robot from ONE state, each with its own model"""

    def __init__(self, name, robot, labels, precision, n, H, env, kernel, std, state=None):
        self.name, self.labels, self.precision, self.n, self.H = name, list(labels), precision, n, H
        self.env, self.kernel, self.std = dict(env), kernel, std
        self.r = r = mv.robot(robot)
        self.state = r.state if state is None else state
        self.E = len(self.labels)
        models = r.all()
        self.pms = [r.packed(models[k]) for k in self.labels]
        self.base_pm = r.packed(r.base)
        self.pt = step_bank.packed_task(r.task, self.state)
        m = r.base
        dt = m.get_number("agent_timestep", m.timestep)
        lo, hi = np.asarray(m.arrays["actuator_ctrlrange"], float).reshape(-1, 2).T
        self.lo, self.hi, self.nu = lo, hi, m.nu
        self.times = np.tile(self.state.time + np.arange(P) * ((H - 1) * dt / (P - 1)), (self.E, 1))
        self.nominal = np.tile(np.clip(np.random.default_rng(3).normal(0, 0.05, (P, m.nu)), lo, hi), (self.E, 1, 1))    # one nominal spline for all
        self.mocap = None if not m.nmocap else np.asarray(self.state.mocap, float)

    def make_context(self, e=None, extra=None):
        """e None: a context on the base model (the fleet's); else one CREATED on the model of environment e"""
        ctx = context(self.base_pm if e is None else self.pms[e], self.pt, self.precision, dict(self.env, **(extra or {})))
        assert self.kernel in ctx.kernel_name, ctx.kernel_name
        return ctx

    def noise(self, e=0, mode=capi.NOISE_SAMPLING, var=None):
        return capi.make_noise_spec(seed=SEED + e, iteration=2, mode=mode, std0=self.std, param_variance=var)

    def push(self, ctx, envs=None, models=True):
        envs = list(range(self.E)) if envs is None else envs
        ctx.set_states(np.stack([self.state.state] * len(envs)), [self.state.time] * len(envs),
                       None if self.mocap is None else np.stack([self.mocap] * len(envs)))
        if models:
            ctx.set_models_batched([self.pms[e] for e in envs])

    def plain(self, ctx):
        ctx.set_state(self.state.state, self.state.time, self.mocap)

    def nodes(self):
        return np.clip(np.random.default_rng(11).normal(0, 2 * self.std, (self.E, self.n, P, self.nu)), self.lo, self.hi)

    def variance(self):
        return np.random.default_rng(12).uniform(0.5, 1.5, (self.E, P, self.nu)) * self.std ** 2

    def run(self, ctx, call, k=None):
        k = self.E if k is None else k
        n, H, t, nom = self.n, self.H, self.times[:k], self.nominal[:k]
        if call == "noise":
            ctx.rollout_noise_batched(n, H, capi.SPLINE_CUBIC, t, nom, self.noise(), num_envs=k)
        elif call == "splines":
            ctx.rollout_splines_batched(H, capi.SPLINE_LINEAR, t, self.nodes()[:k], num_envs=k, n_per_env=n)
        else:
            ctx.rollout_noise_batched_ce(n, H, capi.SPLINE_CUBIC, t, nom, self.variance()[:k], self.noise(mode=capi.NOISE_CROSS_ENTROPY), num_envs=k)

    def run_plain(self, ctx, call, i):
        """what environment number i of a batched call is as a plain one: seed + i, its nodes, its variance row"""
        n, H = self.n, self.H
        if call == "noise":
            ctx.rollout_noise(n, H, capi.SPLINE_CUBIC, self.times[i], self.nominal[i], self.noise(i))
        elif call == "splines":
            ctx.rollout_splines(H, capi.SPLINE_LINEAR, self.times[i], self.nodes()[i])
        else:
            ctx.rollout_noise(n, H, capi.SPLINE_CUBIC, self.times[i], self.nominal[i], self.noise(i, capi.NOISE_CROSS_ENTROPY, self.variance()[i]))

    def assert_models_decide_the_cost(self, ctx):
        """one spline from the one state on every environment's model: E different returns, none failed"""
        values = np.tile(self.nominal[:, None], (1, 64, 1, 1))
        ctx.rollout_splines_batched(self.H, capi.SPLINE_LINEAR, self.times, values, num_envs=self.E, n_per_env=64)
        ret, fail = ctx.returns()
        firsts = [float(ret[64 * e]) for e in range(self.E)]
        assert not fail.any() and len(set(firsts)) == self.E, (self.name, firsts)

    def created(self, call, e, i=None):
        """everything of the plain call on a context created on the model of environment e (as environment number i of the batched call)"""
        ctx = self.make_context(e)
        self.plain(ctx)
        self.run_plain(ctx, call, e if i is None else i)
        out = everything(ctx)
        ctx.close()
        return out

    def assert_batched_equals_created(self, ctx, call):
        self.run(ctx, call)
        got = everything(ctx)
        assert ctx.N == self.E * self.n
        for e in range(self.E):
            one = self.created(call, e)
            for k in ALL:
                assert np.array_equal(got[k][e * self.n:(e + 1) * self.n], one[k], equal_nan=True), (self.name, call, self.labels[e], k)
        return got

    def oracle(self, e, n):
        nodes = pyoracle.noise_candidates(self.pms[e], self.noise(e), P, self.nominal[e], np.arange(n))
        return pyoracle.rollout_batch(self.pms[e], self.pt, self.state.state, self.state.time, self.mocap, n, self.H, P, capi.SPLINE_CUBIC, self.times[e],
                                      nodes, num_threads=16)


FAMILIES = {   # name -> (robot, precision, n, H, environment, kernel, exploration std)
    "quad": ("a1", 64, 1024, 6, {"MJPCX_QUAD_MIN_N": "0"}, "rollout_quad_kernel", 0.06),
    "tree_a1": ("a1", 64, 64, 6, {"MJPCX_NO_QUAD": "1"}, "rollout_tree_kernel<A1>", 0.06),
    "wave_a1": ("a1", 64, 64, 6, {"MJPCX_NO_LDS_MODEL": "1"}, "rollout_wave_kernel", 0.06),
    "limb32": ("humanoid", 32, 1280, 4, {"MJPCX_LIMB_MIN_N": "0"}, "rollout_limb_kernel", 0.05),
    "limb64": ("humanoid", 64, 1280, 4, {"MJPCX_LIMB_MIN_N": "0"}, "rollout_limb_kernel", 0.05),
    "tree_humanoid64": ("humanoid", 64, 64, 4, {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>", 0.05),
    "tree_humanoid32": ("humanoid", 32, 64, 4, {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>", 0.05),
}


def fleet(name, labels=MIXED, n=None, state=None, H=None, extra=None):
    robot, precision, n0, H0, env, kernel, std = FAMILIES[name]
    return ModelFleet(name, robot, labels, precision, n0 if n is None else n, H0 if H is None else H, dict(env, **(extra or {})), kernel, std, state)


# ------------------------------------------------------------------------------------------------- 4: batched = created on the model
@pytest.mark.parametrize("name", list(FAMILIES))
def test_batched_with_models_equals_contexts_created_on_the_models(name):
    f = fleet(name)
    ctx = f.make_context()
    f.push(ctx)
    f.assert_models_decide_the_cost(ctx)
    f.assert_batched_equals_created(ctx, "noise")
    if name in ("quad", "limb32"):
        for call in ("splines", "ce"):
            f.assert_batched_equals_created(ctx, call)
    if "quad" in name or "limb" in name:
        assert ctx.quad_stats()["handed_on"] == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------- 5: every permitted field, the oracle
BOUND = {"quad": 1e-9, "tree_a1": 1e-6, "limb64": 1e-8, "tree_humanoid64": 1e-6}   # (limb64: tests/test_gpu_batch.py's bound of that kernel)


@pytest.mark.parametrize("name", list(BOUND))
def test_every_permitted_field_against_the_oracle(name):
    """One environment per single-field variant, and the base model's. A variant environment that misses its family's bound while the
    base environment of the same launch is inside it is measured on a context CREATED on that variant: the same error there is the
    kernel's precision at those parameters (the bound then is twice the created context's error, and the bits must be equal); an error
    only the fleet shows is a defect of the new path. Measured on MI355X: no variant needed that -- see the printed worst errors."""
    labels = ["base"] + list(mv.robot(FAMILIES[name][0]).single)
    f = fleet(name, labels, n=64)
    ctx = f.make_context()
    f.push(ctx)
    f.assert_models_decide_the_cost(ctx)
    f.run(ctx, "noise")
    got = everything(ctx)
    ctx.close()
    tol, n, worst = BOUND[name], f.n, {}
    for e, label in enumerate(labels):
        ref = f.oracle(e, n)
        sl = slice(e * n, (e + 1) * n)
        assert not ref["failure"].any() and not got["failure"][sl].any(), (name, label)
        worst[label] = max(err(got[k][sl], ref[k]) for k in ("total_return",) + FIELDS)
    print(f"{name}: worst error against the oracle by environment {worst} (bound {tol})")
    assert worst["base"] <= tol, worst
    for e, label in enumerate(labels):
        if worst[label] <= tol:
            continue
        one = f.created("noise", e)
        ref = f.oracle(e, n)
        single = max(err(one[k], ref[k]) for k in ("total_return",) + FIELDS)
        print(f"{name}: {label}: the fleet's error {worst[label]}, a context created on the variant {single}")
        assert single > tol, (name, label, "only the fleet misses the bound", worst[label], single)
        assert worst[label] <= 2 * single, (name, label, worst[label], single)
        for k in ALL:
            assert np.array_equal(got[k][e * n:(e + 1) * n], one[k], equal_nan=True), (name, label, k)


def test_an_affine_actuator_bias_per_environment():
    """actuator_biasprm is zero everywhere in the A1 and in the Humanoid, so no fleet of theirs can show it: tests/models/capsules_bias.xml
    has an affine bias with three non-zero parameters, on the generic kernel (one launch per environment). Its only residual is a constant,
    so the returns are 0 on every model: the STATES tell the environments apart, are the bits of a context created on the variant, and
    the oracle's on that model at the wave kernel's bound."""
    f = ModelFleet("bias_scene", "bias_scene", ("base", "actuator_biasprm", "base"), 64, 64, 6, {}, "rollout_wave_kernel", 0.2)
    ctx = f.make_context()
    f.push(ctx)
    got = f.assert_batched_equals_created(ctx, "noise")
    ctx.close()
    n = f.n
    assert not got["failure"].any()
    assert not np.array_equal(got["states"][0], got["states"][n]) and np.array_equal(got["states"][0], got["states"][2 * n])   # (candidate 0: the nominal)
    for e in range(f.E):
        ref = f.oracle(e, n)
        assert not ref["failure"].any()
        for k in FIELDS:
            assert err(got[k][e * n:(e + 1) * n], ref[k]) <= 1e-6, (f.labels[e], k)


# ------------------------------------------------------------------------------------------------- 6: the hand-on
# bank state, horizon, exploration. Found on the device: from tangled3/step25 the quad kernel hands on 26 of the 192 candidates (the
# others are its own: both kernels in one launch), from the folded Humanoid the limb kernel hands on every one
HAND_ON = {"quad": ("tangled3/step25", 12, 0.6), "limb64": ("folded/0", 4, 0.2)}


@pytest.mark.parametrize("name", ["quad", "limb64"])
def test_handed_on_candidates_roll_out_on_their_environments_model(name):
    """candidates the quad / limb kernel hands to rollout_tree_kernel: that pass stages the environment's image too"""
    label, H, std = HAND_ON[name]
    state = hand_on_state(name)
    f = fleet(name, ("base", "payload", "weak"), n=64, state=state, H=H)
    f.std = std
    ctx = f.make_context()
    f.push(ctx)
    f.run(ctx, "noise")
    got = everything(ctx)
    handed = ctx.quad_stats()["handed_on"]
    ctx.close()
    print(f"{name}: {state.label}: {handed} of {f.E * f.n} candidates handed on")
    assert handed > 0
    for e in range(f.E):
        one = f.created("noise", e)
        ref = f.oracle(e, f.n)
        sl = slice(e * f.n, (e + 1) * f.n)
        for k in ALL:
            assert np.array_equal(got[k][sl], one[k], equal_nan=True), (name, f.labels[e], k)
        ok = ref["failure"] == 0
        assert np.array_equal(got["failure"][sl] != 0, ~ok), (name, f.labels[e])
        for k in ("total_return", "states"):
            assert err(got[k][sl][ok], ref[k][ok]) <= 1e-6, (name, f.labels[e], k)
    assert len({float(got["total_return"][e * f.n]) for e in range(f.E)}) == f.E


def hand_on_state(name):
    r = mv.robot(FAMILIES[name][0])
    found = [s for s in r.bank.states if s.label.startswith(HAND_ON[name][0])]
    assert len(found) == 1, [s.label for s in found]
    return found[0]


# ------------------------------------------------------------------------------------------------- 7: semantics
def refused(fn, code, *words):
    with pytest.raises(capi.MjpcxError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_semantics_on_the_registered_kernel():
    f = fleet("tree_a1")
    E, n = f.E, f.n
    never = f.make_context()
    f.push(never, models=False)
    f.run(never, "noise")
    shared = everything(never)
    f.plain(never)
    f.run_plain(never, "noise", 0)
    plain_ref = everything(never)
    never.close()
    ctx = f.make_context()
    f.push(ctx)
    f.run(ctx, "noise")
    first = everything(ctx)
    f.run(ctx, "noise")
    second = everything(ctx)
    # ---- a plain call between two batched ones sees the context's own model and leaves the next batched call alone
    f.plain(ctx)
    f.run_plain(ctx, "noise", 0)
    between = everything(ctx)
    f.run(ctx, "noise")
    after = everything(ctx)
    for k in ALL:
        assert np.array_equal(first[k], second[k], equal_nan=True), (k, "two calls")
        assert np.array_equal(between[k], plain_ref[k], equal_nan=True), (k, "the plain call")
        assert np.array_equal(after[k], first[k], equal_nan=True), (k, "after the plain call")
    assert len({float(first["total_return"][e * n]) for e in range(E)}) == E      # (candidate 0 is the nominal: the models alone differ)
    # ---- permuting the models permutes the outputs (one seed per POSITION: compare the nominal candidate and, with given splines, everything)
    perm = [2, 0, 3, 1]
    same_nodes = np.tile(f.nodes()[:1], (E, 1, 1, 1))
    ctx.rollout_splines_batched(f.H, capi.SPLINE_LINEAR, f.times, same_nodes, num_envs=E, n_per_env=n)
    ref = everything(ctx)
    f.push(ctx, perm)
    ctx.rollout_splines_batched(f.H, capi.SPLINE_LINEAR, f.times, same_nodes, num_envs=E, n_per_env=n)
    got = everything(ctx)
    for k in ALL:
        for i, e in enumerate(perm):
            assert np.array_equal(got[k][i * n:(i + 1) * n], ref[k][e * n:(e + 1) * n], equal_nan=True), (k, i, e)
    f.push(ctx)
    # ---- another E in a batched call: refused, naming both numbers; nothing is dropped
    f.push(ctx, [0, 1, 2], models=False)
    refused(lambda: f.run(ctx, "noise", 3), -1, "3 environments", "4 models")
    f.push(ctx, models=False)
    # ---- a model that differs where it may not, or changes a zero pattern: refused, naming environment and field; the old models still serve
    r, base = f.r, f.r.base
    for field, index in (("geom_size", 4), ("jnt_range", 5), ("body_parentid", 3)):
        fm = mjcf_copy(base)
        a = np.array(fm.arrays[field], copy=True)
        a.reshape(-1)[index] = a.reshape(-1)[index] * 1.5 if a.dtype.kind == "f" else a.reshape(-1)[index] - 1
        fm.arrays[field] = a
        refused(lambda: ctx.set_models_batched([f.pms[0], f.pms[1], r.packed(fm), f.pms[3]]), -1, "environment 2", field)
    fm = mjcf_copy(base)
    fl = np.array(fm.arrays["dof_frictionloss"], float, copy=True)
    dof = int(np.flatnonzero(fl == 0.2)[0])
    fl[dof] = 0.0
    fm.arrays["dof_frictionloss"] = fl
    refused(lambda: ctx.set_models_batched([f.pms[0], r.packed(fm), f.pms[2], f.pms[3]]), -1, "environment 1", "dof_frictionloss")
    f.run(ctx, "noise")
    kept = everything(ctx)
    for k in ALL:
        assert np.array_equal(kept[k], first[k], equal_nan=True), (k, "after refused calls")
    # ---- the derivative chain is a follow-up
    H, nv, nu, dim = f.H, base.nv, base.nu, base.nq + base.nv
    zeros = lambda *s: np.zeros(s)
    refused(lambda: ctx.rollout_feedback_batched(H, 0, 0, 1, np.tile(f.times[:, :1] + 0.01 * np.arange(H), (1, 1)), zeros(E, H, dim), zeros(E, H, nu),
                                                 zeros(E, H, nu, 2 * nv), zeros(E, H, nu), zeros(E, 1)), -2, "derivative chain")
    refused(lambda: ctx.gradient_step_batched(E, 0, H, list(range(H)), 1e-6, 0, 0, f.times), -2, "derivative chain")
    # ---- cleared: the bits of a context that never had models
    ctx.set_models_batched(None)
    f.run(ctx, "noise")
    none = everything(ctx)
    for k in ALL:
        assert np.array_equal(none[k], shared[k], equal_nan=True), (k, "cleared")
    ctx.close()
    # ---- a lane-family context has no model to exchange
    cart = step_bank.lane_bank("Cartpole")
    c2 = capi.Context(cart.task.packed_model(), cart.task.packed(), 0, 64)
    refused(lambda: c2.set_models_batched([cart.task.packed_model()]), -2, "lane-per-candidate")
    c2.close()


def mjcf_copy(fm):
    from mujoco_mpc_amd import mjcf
    return mjcf.variant(fm)          # (no field named: a deep copy with the same derived quantities)


# ------------------------------------------------------------------------------------------------- 8: models with task rows
def test_models_with_task_rows_on_the_quad_kernel():
    f = fleet("quad", ("base", "payload", "ice"))
    task = f.r.task
    rows = task_rows.unlike_rows(task, f.E)
    ctx = f.make_context()
    f.push(ctx)
    ctx.set_task_params_batched(**{k: rows[k] for k in ("weight", "norm_parameter", "parameters", "risk")})
    f.run(ctx, "noise")
    got = everything(ctx)
    ctx.close()
    for e in range(f.E):
        c1 = f.make_context(e)
        c1.set_task_params(rows["weight"][e], rows["norm_parameter"][e], rows["parameters"][e] if len(task.parameters) else None, float(rows["risk"][e]))
        f.plain(c1)
        f.run_plain(c1, "noise", e)
        one = everything(c1)
        c1.close()
        for k in ALL:
            assert np.array_equal(got[k][e * f.n:(e + 1) * f.n], one[k], equal_nan=True), (f.labels[e], k)


# ------------------------------------------------------------------------------------------------- 9: the planners on the device
@pytest.mark.parametrize("kind", list(cpu.KINDS))
def test_fleet_planner_with_models_equals_single_planners_on_the_device(kind):
    batch, singles, task, models = cpu.run_fleet_with_models(kind, (None, None), horizon=12, steps=2)
    assert len({batch.best_trajectory(e).total_return for e in range(cpu.E)}) == cpu.E
    for p in [batch] + singles:
        for c in ([p.ctx] + ([p.delegate.ctx] if kind == "robust" else [])):
            c.close()
