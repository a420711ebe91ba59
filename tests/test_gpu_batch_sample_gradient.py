"""-m gpu: the Sample-Gradient planner for a fleet -- mjpcx_rollout_sample_gradient_batched (the candidates generated on the device, then
the batched rollout) and mjpcx_sample_gradient_update_batched (sort, winner, fitness-shaped gradient, gradient-step candidates: one
launch, one sync) -- on the device.

  1. The candidates of every kernel family of tests/test_gpu_batch.py against batch_sample_gradient_oracle_backend.candidates: the
     nominal exactly, the noisy ones at the tolerance the repository holds a device normal to (sample_gradient_cases.NORMAL_TOL) times
     noise_exploration, uploaded gradient candidates over the node times exactly after the clamp. On a 32-bit context "exactly" is the
     value rounded to float32, and a noisy node may land on the neighbouring float: 2^-24 relative is added.
  2. The re-sampling of gradient splines over shifted times against exact rational arithmetic.
  3. A batched call against E one-environment calls on the same context, bit for bit in every buffer and every update output, and
     against the oracle at the family's tolerance.
  4. The update on INJECTED returns (selection_cases) against planners.sample_gradient_update fed the oracle's normals.
  5. GpuBatchSampleGradientPlanner against its members, and GpuSampleGradientPlanner against the C++ planner."""
import math
from fractions import Fraction

import numpy as np
import pytest

import sample_gradient_cases as sgc
import selection_cases as sc
import test_batch_sample_gradient_planner as cpu
import test_gpu_selection as sel
from batch_sample_gradient_oracle_backend import candidates, oracle_normals
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuSampleGradientPlanner, State, clamp, sample_gradient_update
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle
from test_gpu_batch import E, FIELDS, H, P, SEED, err, everything, make_case
from test_gpu_batch_robust import pinned, push_states

pytestmark = pytest.mark.gpu
CUBIC = capi.SPLINE_CUBIC
BOTH = capi.SG_COMPUTE_WEIGHTS | capi.SG_ZERO_GRADIENT
EXPLORATION, ITERATION, G = 0.07, 3, 5
MAX_STEP, MIN_STEP = 2.0, 1.0e-3
EINVAL = -1
FAMILIES = ["cartpole64", "particle32", "quad", "tree_a1", "limb32", "wave"]


def ctrlrange_of(task):
    return np.asarray(task.model.actuator_ctrlrange, float).reshape(-1, 2)


def uploaded(case, envs, num_gradient):
    """gradient candidates to upload: beyond the control range here and there, so the clamp acts"""
    b = ctrlrange_of(case.task)
    rng = np.random.default_rng(11)
    return rng.uniform(1.3 * b[:, 0], 1.3 * b[:, 1], (len(envs), num_gradient, P, b.shape[0]))


def sg_rollout(case, ctx, envs, gv, gt, seed=SEED, horizon=H):
    push_states(case, ctx, envs)
    ctx.rollout_sample_gradient_batched(case.n, G, horizon, CUBIC, case.times[envs], case.nominal[envs], EXPLORATION, seed=seed + envs[0],
                                        iteration=ITERATION, gradient_values=gv, gradient_times=gt, num_envs=len(envs))


def update(ctx, num_envs, flags=BOTH, gradient_filter=0.7, num_gradient=G):
    return ctx.sample_gradient_update_batched(num_envs, num_gradient, flags, gradient_filter, MAX_STEP, MIN_STEP, EXPLORATION)


@pytest.mark.parametrize("name", FAMILIES)
def test_candidates_batched_sequential_and_the_oracle(name):
    """1. and 3. of the module's docstring on one context per family"""
    case = make_case(name)
    n, envs, b = case.n, list(range(E)), ctrlrange_of(case.task)
    gv = uploaded(case, envs, G)
    ctx = case.make_context()
    sg_rollout(case, ctx, envs, gv, case.times[envs])
    got = everything(ctx)
    out = update(ctx, E)
    single = np.float32 if case.precision == 32 else np.float64
    made = [candidates(b, n, G, CUBIC, case.times[e], case.nominal[e], EXPLORATION, SEED + e, ITERATION, gv[e], case.times[e]) for e in range(E)]
    nodes = np.stack([np.stack([ctx.fetch_spline(e * n + c) for c in range(n)]) for e in range(E)])
    for e in range(E):
        want = made[e][0]
        stored = want.astype(single).astype(np.float64)
        assert np.array_equal(nodes[e, 0], stored[0]), (name, e)                                                   # the nominal
        assert np.array_equal(nodes[e, n - G:], clamp(gv[e].copy(), b).astype(single).astype(np.float64)), (name, e)   # uploaded, over the node times
        tol = sgc.NORMAL_TOL * EXPLORATION + (2.0 ** -24 * np.abs(want[1:n - G]) if case.precision == 32 else 0.0)
        assert np.all(np.abs(nodes[e, 1:n - G] - want[1:n - G]) <= tol), (name, e, float(np.max(np.abs(nodes[e, 1:n - G] - want[1:n - G]))))
        assert np.all(nodes[e] >= b[:, 0]) and np.all(nodes[e] <= b[:, 1])
    assert len({nodes[e, 1].tobytes() for e in range(E)}) == E                                                     # seed + e: other normals
    # ---- one environment at a time, on the same context: every buffer and every output of the update, bit for bit
    for e in range(E):
        sg_rollout(case, ctx, [e], gv[e:e + 1], case.times[e:e + 1])
        one = everything(ctx)
        sl = slice(e * n, (e + 1) * n)
        assert np.array_equal(one["total_return"], got["total_return"][sl]) and np.array_equal(one["failure"], got["failure"][sl]), (name, e)
        for k in FIELDS:
            assert np.array_equal(one[k], got[k][sl]), (name, e, k)
        alone = update(ctx, 1)
        for k, v in out.items():
            assert sc.same_bits(alone[k][0], v[e]) if v.dtype == np.float64 else np.array_equal(alone[k][0], v[e]), (name, e, k)
    # ---- the oracle, per environment, on the candidates the device made (what the rollout kernels' own suites compare)
    for e in range(E):
        s = case.states[e]
        ref = pyoracle.rollout_batch(case.pm, case.packed(e), s.state, s.time, case.mocap(e), n, H, P, CUBIC, case.times[e], nodes[e], num_threads=16)
        sl = slice(e * n, (e + 1) * n)
        assert np.array_equal(got["failure"][sl] != 0, ref["failure"] != 0), (name, e)
        ok = ref["failure"] == 0
        assert ok.any(), (name, e)
        worst = err(got["total_return"][sl][ok], ref["total_return"][ok])
        print(f"{name} env {e}: returns off the oracle by {worst:.3g} (tolerance {max(case.tol, case.tol_handed):.3g})")
        assert worst <= max(case.tol, case.tol_handed), (name, e, worst)
        ret = got["total_return"][sl]
        w = int(out["index"][e])
        assert w == (sc.order(ret)[0] if ret[sc.order(ret)[0]] < ret[0] else 0) and out["winner_type"][e] == (0 if w == 0 else 1 if w < n - G else 2)
        assert sc.same_bits(out["best_return"][e], ret[w]) and sc.same_bits(out["nominal_return"][e], ret[0])
        assert np.array_equal(out["spline"][e], nodes[e, w])
    ctx.close()


@pytest.mark.parametrize("nodes", [1, 2, 3, 4])
@pytest.mark.parametrize("interp", [0, 1, 2])
def test_resampling_against_exact_arithmetic(interp, nodes):
    """Gradient splines over one grid, re-sampled at node times shifted against it -- before its first node, inside every interval, on a
    node, beyond the last -- against sample_gradient_cases.resample_exact: |device - exact| <= k u M with k = 0 / 8 / 26 roundings for
    zero / linear / cubic and M the magnitude of the terms (the derivation is sample_gradient_cases' docstring); the clamp is
    1-Lipschitz, so the bound holds after it."""
    ctx = sel.make_context("Cartpole", 64)
    (lo, hi), = ctrlrange_of(sel._task("Cartpole"))
    num_envs, n, grad = 2, 64, 7
    rng = np.random.default_rng(40 + 10 * interp + nodes)
    old = np.stack([0.1 * e + np.cumsum(rng.uniform(0.01, 0.03, nodes)) for e in range(num_envs)])
    shift = [-0.05, 0.013]
    new = np.stack([old[e] + shift[e] for e in range(num_envs)])
    if nodes > 1:
        new[1, 0] = old[1, 1]                                         # exactly on a node
    new = np.sort(new, axis=1)
    assert np.all(np.diff(new, axis=1) > 0) if nodes > 1 else True
    gv = rng.uniform(-1.4, 1.4, (num_envs, grad, nodes, 1))
    sel.set_fleet(ctx, "Cartpole", num_envs)
    ctx.rollout_sample_gradient_batched(n, grad, 2, interp, new, np.zeros((num_envs, nodes, 1)), 0.1, seed=1, iteration=0, gradient_values=gv,
                                        gradient_times=old, num_envs=num_envs)
    worst = 0.0
    for e in range(num_envs):
        for g in range(grad):
            got = ctx.fetch_spline(e * n + n - grad + g).reshape(-1)
            for p in range(nodes):
                exact, magnitude = sgc.resample_exact(old[e], gv[e, g, :, 0], interp, new[e, p])
                exact = min(max(exact, Fraction(float(lo))), Fraction(float(hi)))
                bound = sgc.RESAMPLE_ROUNDINGS[interp] * Fraction(sgc.U) * magnitude
                d = abs(Fraction(float(got[p])) - exact)
                assert d <= bound, (interp, nodes, e, g, p, float(d), float(bound))
                worst = max(worst, float(d / bound) if bound else 0.0)
    print(f"interpolation {interp}, {nodes} nodes: worst error / bound {worst:.3g}")
    ctx.close()


# ------------------------------------------------------------------------------------------------ the update on injected returns
class Fleet:
    """a context with a Sample-Gradient rollout of E environments to inject returns into; Cartpole (P = 3: an odd number of parameters,
    the last pair half empty; or `nodes` of them) or the A1 (P = 4, 48 parameters: six chunks of four pairs)"""

    def __init__(self, model, precision, n, num_envs=E, nodes=sel.P):
        self.model, self.precision, self.n, self.num_envs = model, precision, n, num_envs
        if model == "A1":
            self.case = make_case("tree_a1")
            self.ctx = self.case.make_context()
            self.times, self.task = self.case.times, self.case.task
        else:
            self.case = None
            self.ctx = sel.make_context(model, precision)
            self.times = np.tile(np.linspace(sel.TIMES[0], sel.TIMES[-1], nodes), (num_envs, 1)) + 0.01 * np.arange(num_envs)[:, None]
            self.task = sel._task(model)
        self.range = ctrlrange_of(self.task)
        self.nodes_per_spline = self.times.shape[1]
        self.num_parameters = self.nodes_per_spline * self.ctx.nu
        self.nominal = np.random.default_rng(n).uniform(-0.2, 0.2, (num_envs, self.nodes_per_spline, self.ctx.nu))
        self.seed, self.iteration = 77, 4
        self._normals = {}

    def normals(self, iteration):
        if iteration not in self._normals:
            self._normals[iteration] = [oracle_normals(self.seed + e, self.n, self.num_parameters, iteration, first=1) for e in range(self.num_envs)]
        return self._normals[iteration]

    def rollout(self, num_gradient, upload):
        num_envs = self.num_envs
        if self.case is not None:
            push_states(self.case, self.ctx, list(range(num_envs)))
        else:
            sel.set_fleet(self.ctx, self.model, num_envs)
        gv = np.zeros((num_envs, num_gradient, self.nodes_per_spline, self.ctx.nu)) if upload else None
        self.ctx.rollout_sample_gradient_batched(self.n, num_gradient, 2, CUBIC, self.times, self.nominal, EXPLORATION, seed=self.seed,
                                                 iteration=self.iteration, gradient_values=gv, gradient_times=self.times if upload else None, num_envs=num_envs)

    def spline(self, e, c):
        return self.ctx.fetch_spline(e * self.n + c).reshape(-1)


def check_update(fleet, cases, num_noisy, out, flags, gradient_filter, state, where):
    """every output of one update against the contract and sample_gradient_update; `state` carries the reference's weights, gradient and
    bound per environment from step to step -> the reference's results"""
    n, num_gradient = fleet.n, fleet.n - num_noisy
    refs = []
    for e, c in enumerate(cases):
        at = where + (c.name, e)
        order = sc.order(c.ret)
        w = int(order[0]) if c.ret[order[0]] < c.ret[0] else 0
        assert out["index"][e] == w and out["winner_type"][e] == (0 if w == 0 else 1 if w < num_noisy else 2), at + (int(out["index"][e]), w)
        assert sc.same_bits(out["best_return"][e], c.ret[w]) and sc.same_bits(out["nominal_return"][e], c.ret[0]), at
        with np.errstate(invalid="ignore"):
            d = c.ret[0] - c.ret[w]       # (inf - inf and NaN: no improvement)
        assert sc.same_bits(out["improvement"][e], d if d > 0 else 0.0), at
        assert np.array_equal(out["spline"][e].reshape(-1), fleet.spline(e, w)), at
        if num_gradient < 1:
            assert not np.any(out["gradient"][e]), at
            refs.append(None)
            continue
        z = fleet.normals(fleet.iteration)[e]
        compute = bool(flags & capi.SG_COMPUTE_WEIGHTS)
        previous = None if flags & capi.SG_ZERO_GRADIENT else state[e]["gradient"]
        with np.errstate(invalid="ignore"):
            ref = sample_gradient_update(c.ret, fleet.nominal[e], z, num_gradient, fleet.range, None if compute else state[e]["weights"], previous, compute,
                                         gradient_filter, MAX_STEP, MIN_STEP, EXPLORATION)
        assert np.array_equal(ref["order"], order) and ref["winner"] == w
        used = sc.order(c.ret[:num_noisy]) if compute else order[:num_noisy]
        bound = sgc.gradient_bound(used, ref["weights"], z, num_noisy)
        off = np.abs(out["gradient"][e] - ref["gradient"])
        assert np.all(off <= bound), at + (float(np.max(off)), float(np.max(bound)))
        ref["bound"], ref["bound_previous"] = bound, (np.zeros_like(bound) if previous is None else state[e]["bound"])
        refs.append(ref)
    return refs


def check_next_candidates(fleet, num_noisy, refs, gradient_filter, where):
    """the gradient candidates the update left on the device, read back through the next rollout over the same node times (TimeSpline::Sample
    on a node returns the node)"""
    num_gradient = fleet.n - num_noisy
    picks = range(num_gradient) if num_gradient <= 16 else sorted({0, 1, num_gradient // 2, num_gradient - 2, num_gradient - 1})
    for e, ref in enumerate(refs):
        for g in picks:
            got = fleet.spline(e, num_noisy + g)
            tol = sgc.candidate_bound(g, fleet.nominal[e].reshape(-1), ref["gradient"], ref["gradient_previous"], ref["bound"], ref["bound_previous"],
                                      num_gradient, gradient_filter, MAX_STEP, MIN_STEP, EXPLORATION, fleet.precision)
            off = np.abs(got - ref["candidates"][g])
            assert np.all(off <= tol), where + (e, g, float(np.max(off)), float(np.max(tol)))


NOISY = (1, 63, 64, 65, 255, 256, 257)


SLAB_NODES = 9   # Cartpole: 9 parameters = 5 pairs = 2 chunks of four pairs (sel.P = 3 is one chunk: one slab per environment, no chunk factor)
UPDATE_MODELS = {"Cartpole64": ("Cartpole", 64), "Cartpole32": ("Cartpole", 32), "A1": ("A1", 64)}
UPDATE_CASES = [(name, n) for n in (64, 256, 320, 1088) for name in UPDATE_MODELS] + [("Cartpole64", sc.SCRATCH_FIRST), ("Cartpole32", sc.SCRATCH_FIRST)]


@pytest.mark.parametrize("name,n", UPDATE_CASES, ids=[f"{name}-{n}" for name, n in UPDATE_CASES])
def test_update_on_injected_returns(name, n):
    """mjpcx_sample_gradient_update_batched on returns the test chose (selection_cases: the minimum at every place and across every
    boundary of the reductions, ties, NaN, signed zeros, infinities, failed rollouts, the nominal as the minimum), a different case in each of
    the three environments, for every num_noisy that changes a path: index, winner_type and the winner's spline bit for bit,
    improvement and the returns exactly, the gradient within sample_gradient_cases.gradient_bound of planners.sample_gradient_update
    fed the oracle's normals, the next candidates within candidate_bound. Per num_noisy a two-step chain: the first step computes the
    weights from a zero gradient, the second (filter 0.3) uses them cached on the order over all candidates, with the gradient of the
    first as gradient_previous.

    n = 8256 is the first size sorted in the global slab (n2 = 16384), sg_update_kernel<T, false>: there the Cartpole alone, two
    environments and SLAB_NODES nodes, so that with gradient candidates the grid is 2 environments x 2 chunks and slab (e, chunk)
    must lie at (e * chunks + chunk) * 1.5 n2 doubles. What changes a path at that size is the number of chunks (num_gradient = 0: one;
    > 0: two) and what is sorted (the noisy candidates when the weights are computed, every candidate otherwise): num_noisy = n, n - 1
    and 257 cover them, each on every fifth round of cases; the boundaries of the reductions inside num_noisy are the smaller sizes'."""
    model, precision = UPDATE_MODELS[name]
    slab = n > sc.LDS_LAST
    fleet = Fleet(model, precision, n, 2, SLAB_NODES) if slab else Fleet(model, precision, n)
    ctx, E = fleet.ctx, fleet.num_envs
    rounds = sc.segmented_rounds(n, E)
    nominal_best = [sc.Case("nominal-min", sc.with_min(n, 300 + n + e, 0)) for e in range(E)]
    rounds.append(nominal_best)
    for num_noisy in (257, n - 1, n) if slab else sorted({m for m in NOISY + (n - 1, n) if 1 <= m <= n}):
        num_gradient = n - num_noisy
        fleet.iteration = 4
        fleet.rollout(num_gradient, upload=num_gradient > 0)
        for ri, cases in enumerate(rounds if num_noisy in (1, 64, n - 1, n) and not slab else rounds[::5] + [nominal_best]):
            where = (model, precision, n, num_noisy, ri)
            sc.inject(ctx, np.concatenate([c.ret for c in cases]), np.concatenate([c.fail for c in cases]))
            out = update(ctx, E, BOTH, 1.0, num_gradient)
            check_update(fleet, cases, num_noisy, out, BOTH, 1.0, None, where)
            if ri < 2:    # deterministic: the same rollout, the gradient zeroed again
                again = update(ctx, E, BOTH, 1.0, num_gradient)
                for k, v in out.items():
                    assert sc.same_bits(again[k], v) if v.dtype == np.float64 else np.array_equal(again[k], v), where + (k,)
        if cases is nominal_best:
            assert not np.any(out["index"]) and not np.any(out["winner_type"]) and not np.any(out["improvement"])   # no strict improvement: the nominal stays
        if num_gradient < 1:
            continue
        # ---- the chain. Step 1 on the first round's returns ...
        cases = rounds[0]
        sc.inject(ctx, np.concatenate([c.ret for c in cases]), np.concatenate([c.fail for c in cases]))
        first = check_update(fleet, cases, num_noisy, update(ctx, E, BOTH, 1.0, num_gradient), BOTH, 1.0, None, (model, n, num_noisy, "step 1"))
        fleet.iteration = 5
        fleet.rollout(num_gradient, upload=False)            # ... its candidates come back as the last splines of the next rollout
        check_next_candidates(fleet, num_noisy, first, 1.0, (model, n, num_noisy, "step 1"))
        # ... step 2 on returns that put the last gradient candidate first: a zero-noise row inside the cached weights' reach
        cases = [sc.Case(c.name + ",gradient-first", np.where(np.arange(n) == n - 1, sc.LOW / 2, c.ret)) for c in rounds[1]]
        sc.inject(ctx, np.concatenate([c.ret for c in cases]), np.concatenate([c.fail for c in cases]))
        second = check_update(fleet, cases, num_noisy, update(ctx, E, 0, 0.3, num_gradient), 0, 0.3, first, (model, n, num_noisy, "step 2"))
        assert all(int(o) == n - 1 for o in [sc.order(c.ret)[0] for c in cases])
        assert all(np.array_equal(s["weights"], f["weights"]) and np.array_equal(s["gradient_previous"], f["gradient"]) for s, f in zip(second, first))
        fleet.iteration = 6
        fleet.rollout(num_gradient, upload=False)
        check_next_candidates(fleet, num_noisy, second, 0.3, (model, n, num_noisy, "step 2"))
    ctx.close()


def test_refusals():
    ctx = sel.make_context("Cartpole", 64)
    nominal = np.zeros((E, sel.P, 1))
    times = np.tile(sel.TIMES, (E, 1))
    sel.set_fleet(ctx, "Cartpole", E)
    call = lambda G_, s=EXPLORATION, gv=None, gt=None: ctx.rollout_sample_gradient_batched(64, G_, 2, CUBIC, times, nominal, s, gradient_values=gv,
                                                                                        gradient_times=gt, num_envs=E)
    for bad in (lambda: call(-1), lambda: call(64, gv=np.zeros((E, 64, sel.P, 1)), gt=times), lambda: call(0, s=0.0), lambda: call(0, s=-1.0),
                lambda: call(4)):                                      # (no update of this shape has run: nothing to take from the device)
        with pytest.raises(capi.MjpcxError) as info:
            bad()
        assert info.value.code == EINVAL
    with pytest.raises(capi.MjpcxError):
        update(ctx, E)                                                 # no Sample-Gradient rollout yet
    call(4, gv=np.zeros((E, 4, sel.P, 1)), gt=times)
    for bad in (lambda: update(ctx, E, num_gradient=3), lambda: update(ctx, 1, num_gradient=4), lambda: update(ctx, E, 0, num_gradient=4),   # (no cached weights)
                lambda: update(ctx, E, 4, num_gradient=4)):
        with pytest.raises(capi.MjpcxError) as info:
            bad()
        assert info.value.code == EINVAL
    update(ctx, E, BOTH, num_gradient=4)
    call(4)                                                            # now the device has candidates of this shape
    update(ctx, E, 0, num_gradient=4)
    ctx.rollout_noise_batched(64, 2, CUBIC, times, nominal, capi.make_noise_spec(seed=1, std0=0.1), num_envs=E)
    with pytest.raises(capi.MjpcxError):
        update(ctx, E, 0, num_gradient=4)                              # the last rollout is another kind now
    ctx.close()


# ------------------------------------------------------------------------------------------------ the planners
@pytest.mark.parametrize("name", ["Cartpole", "QuadrupedFlat"])
def test_planner_fleet_is_one_planner_per_environment(name):
    with pinned(MJPCX_QUAD_MIN_N="0"):
        batch, singles, seen = cpu.run_fleet_against_members(load_task(name), 5, factory=None)
    want = "rollout_quad_kernel" if name == "QuadrupedFlat" else "rollout_lane"
    assert want in batch.ctx.kernel_name and want in singles[0].ctx.kernel_name
    assert all(np.any(g != 0.0) for _, _, g in seen)
    for p in singles + [batch]:
        p.ctx.close()


CPP_SEED = 5


def test_python_planner_against_the_cpp_planner(cartpole):
    """GpuSampleGradientPlanner against HostPlanner(kind="sample_gradient"), Cartpole, 64 candidates of which 8 gradient candidates, the
    same seed. The two planners sum the gradient in different orders (and the C++ one draws its normals on the host), so their returns
    agree to rounding, not to the bit: the orders are compared only where the C++ planner's own sorted returns are nowhere closer than
    1e-9 relatively (asserted; CPP_SEED was chosen on the oracle so that it holds: 7e-7 and 1e-7 there). The FIRST plan step after a
    reset can never meet that: the reference starts its gradient candidates from the empty spline, so they and the nominal are nine
    times the same spline, nine equal returns (asserted, bit for bit). That step is compared on the 56 candidates that differ; the two
    plan steps after it are compared in full: orders, winners and types equal, the gradients within
    sample_gradient_cases.gradient_bound widened by what the C++ planner does differently -- it adds the m = num_noisy terms one after
    the other, m - 1 more roundings, and its host normals are a second draw held to NORMAL_TOL. The C++ planner does not hand out its
    candidates' splines: the gradient candidates of steps 2 and 3 are rebuilt from ITS gradients by the reference's formula about the
    nominal of the step before and held to the device's (the last 8 splines of the Python planner's rollout) within candidate_bound."""
    from mujoco_mpc_amd.hostplanner import HostPlanner
    n, num_gradient, Hc, gradient_filter = 64, 8, 40, 0.8
    num_noisy = n - num_gradient
    cpp = HostPlanner(cartpole, seed=CPP_SEED, num_trajectory=n, kind="sample_gradient")
    cpp.sample_gradient_config(num_gradient=num_gradient, gradient_filter=gradient_filter)
    cpp.reset(Hc)
    py = GpuSampleGradientPlanner(seed=CPP_SEED)
    py.initialize(cartpole.model, cartpole)
    py.num_trajectory_, py.num_gradient_, py.gradient_filter_ = n, num_gradient, gradient_filter
    py.allocate()
    py.reset(Hc)
    num_parameters = cpp.num_spline_points * cartpole.model.nu
    assert num_parameters == py.num_parameters()
    q, v = [0.2, 0.6], [0.0, 0.1]
    st = State(cartpole.model)
    st.set(q, v, time=0.0)
    zero = np.zeros(num_parameters)
    bounds, gradients, nominals, weights = [zero, zero], [zero, zero], [], None
    b = ctrlrange_of(cartpole)
    steps = sgc.log_scale(MAX_STEP, MIN_STEP, num_gradient) / py.noise_exploration
    for step in range(3):
        cpp.set_state(q, v, 0.0)
        cpp.optimize_policy(Hc)
        py.set_state(st)
        py.optimize_policy(Hc)
        wt, g, ret = cpp.sample_gradient_result(num_parameters, n)
        ret, g = np.asarray(ret[:n], float), np.asarray(g, float)[:num_parameters]
        mine = py.ctx.returns()[0]
        same = [0] + list(range(num_noisy, n))
        if step == 0:
            assert len(set(ret[same])) == 1 and len(set(mine[same])) == 1
        compared = np.arange(num_noisy) if step == 0 else np.arange(n)
        srt = np.sort(ret[compared])
        assert np.all(np.diff(srt) > 1e-9 * np.abs(srt[1:])), (step, float(np.min(np.diff(srt) / np.abs(srt[1:]))))    # the precondition
        assert np.array_equal(sc.order(mine[compared]), sc.order(ret[compared])), step
        assert (py.winner, py.winner_type_) == (cpp.winner, wt), step
        z = oracle_normals(CPP_SEED, n, num_parameters, step, first=1)
        ref = sample_gradient_update(mine, zero, z, num_gradient, b, weights, None, step == 0)
        weights = ref["weights"]                # (computed at the first step, cached afterwards: both planners)
        used = sc.order(mine[:num_noisy]) if step == 0 else sc.order(mine)[:num_noisy]
        abs_terms, abs_q = sgc.gradient_terms(used, weights, z, num_noisy)
        bound = (2 * math.ceil(num_noisy / 256) + 20 + num_noisy) * sgc.U * abs_terms + 2 * sgc.NORMAL_TOL * abs_q
        off = np.abs(py.gradient - g)
        assert np.any(py.gradient != 0.0) and np.all(off <= bound), (step, float(np.max(off)), float(np.max(bound)))
        if step > 0:
            # what the update of the step before left: nominal + (-s filter) g + (-s (1 - filter)) g', then ResamplePolicy at this step's
            # node times -- the same clock here, so the nodes themselves
            for k in range(num_gradient):
                v_ = nominals[-1].copy()
                v_ += -steps[k] * gradient_filter * gradients[-1]
                v_ += -steps[k] * (1.0 - gradient_filter) * gradients[-2]
                got = py.ctx.fetch_spline(num_noisy + k).reshape(-1)
                tol = sgc.candidate_bound(k, nominals[-1], gradients[-1], gradients[-2], bounds[-1], bounds[-2], num_gradient, gradient_filter, MAX_STEP,
                                          MIN_STEP, py.noise_exploration)
                assert np.all(np.abs(got - clamp(v_, b)) <= tol), (step, k, float(np.max(np.abs(got - clamp(v_, b)))))
        bounds.append(bound)
        gradients.append(g.copy())
        nominals.append(py.ctx.fetch_spline(0).reshape(-1))
    py.ctx.close()
