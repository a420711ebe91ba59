"""GpuSampleGradientPlanner and GpuBatchSampleGradientPlanner (mujoco_mpc_amd/planners.py) on the oracle-backed test backend
(batch_sample_gradient_oracle_backend.py), and planners.sample_gradient_update against a plain-loop restatement of the reference's update.
Fleet and members both run the oracle and the same arithmetic, so their equality is exact."""
import math
import os
import re

import numpy as np
import pytest
from fractions import Fraction

import sample_gradient_cases as sgc
import task_rows
from batch_sample_gradient_oracle_backend import BatchSampleGradientOracleContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchSampleGradientPlanner, GpuSampleGradientPlanner, sample_gradient_update, strided_tree_sum
from mujoco_mpc_amd.task import load_task
from test_batch_robust_planner import HORIZON, assert_same_trajectory, initial_states, step_along

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, STEPS, SEED, N = 3, 3, 9, 64
U = 2.0 ** -53


def test_the_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mjpcx.h")).read(), flags=re.S)
    for name, method in (("mjpcx_rollout_sample_gradient_batched", "rollout_sample_gradient_batched"),
                         ("mjpcx_sample_gradient_update_batched", "sample_gradient_update_batched")):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and getattr(capi.lib(), name).argtypes is not None
        assert callable(getattr(capi.Context, method))
    assert re.search(r"#define MJPCX_SG_COMPUTE_WEIGHTS %d\b" % capi.SG_COMPUTE_WEIGHTS, src)
    assert re.search(r"#define MJPCX_SG_ZERO_GRADIENT %d\b" % capi.SG_ZERO_GRADIENT, src)


# ---------------------------------------------------------------- the update against the reference's loops
def before(ret, a, b):
    """the device's order of two candidates: ascending returns, ties (and -0 / +0) to the lower index, NaN last"""
    ra, rb = ret[a], ret[b]
    if math.isnan(ra) != math.isnan(rb):
        return math.isnan(rb)
    if not math.isnan(ra) and ra != rb:
        return ra < rb
    return a < b


def sort_head(ret, count):
    """trajectory_order[0..count) after `for i: order[i] = i; partial_sort(..., returns[a] < returns[b])`, the comparison made total"""
    order = []
    for c in range(count):
        at = len(order)
        while at > 0 and before(ret, c, order[at - 1]):
            at -= 1
        order.insert(at, c)
    return order


class ReferenceLoops:
    """sample_gradient/planner.cc:168-212 and 401-493 in plain loops and Python floats, one robot: the state the reference keeps
    (return_weight_, gradient, gradient_previous, trajectory_order) and its statements in their order; the noise rows of the nominal
    and of the gradient candidates are zero."""

    def __init__(self, num_parameters, ctrlrange, nu):
        self.weight, self.np, self.nu, self.range = [], num_parameters, nu, [float(x) for x in np.asarray(ctrlrange).reshape(-1)]
        self.gradient, self.gradient_previous = [0.0] * num_parameters, [0.0] * num_parameters

    def update(self, returns, nominal, noise, G, gradient_filter, max_step, min_step, noise_exploration):
        n = len(returns)
        num_noisy = n - G
        order = sort_head(returns, n)
        winner = order[0] if returns[order[0]] < returns[0] else 0
        winner_type = (1 if winner < n - G else 2) if winner > 0 else 0
        improvement = max(returns[0] - returns[winner], 0.0) if not math.isnan(returns[0] - returns[winner]) else 0.0
        out = dict(order=list(order), winner=winner, winner_type=winner_type, improvement=improvement)
        if G < 1:
            return out
        self.gradient_previous = list(self.gradient)
        if len(self.weight) != num_noisy:
            order[:num_noisy] = sort_head(returns, num_noisy)
            f0 = math.log(0.5 * num_noisy + 1.0)
            den = 0.0
            for i in range(num_noisy):
                den += max(0.0, f0 - math.log(order[i] + 1))
            self.weight = [max(0.0, f0 - math.log(order[i] + 1)) / den - 1.0 / num_noisy for i in range(num_noisy)]
        self.gradient = [0.0] * self.np
        magnitude = [0.0] * self.np   # (for the bound: sum_i |w_i| / num_noisy |z|, with |w_i| <= f_i / den + 1 / num_noisy)
        for i in range(num_noisy):
            c = order[i]
            for k in range(self.np):
                z = float(noise[c][k]) if 0 < c < num_noisy else 0.0
                self.gradient[k] += z * (self.weight[i] / num_noisy)
                magnitude[k] += abs(z) * ((abs(self.weight[i]) + 2.0 / num_noisy) / num_noisy)
        step = (math.log(max_step) - math.log(min_step)) / (G - 1 if G > 1 else 1)
        step_size = [math.exp(math.log(min_step) + i * step) for i in range(G)]
        candidates = []
        for g in range(G):
            scaling = step_size[g] / noise_exploration
            v = [float(x) for x in nominal]
            for k in range(self.np):
                v[k] += -scaling * gradient_filter * self.gradient[k]
                v[k] += -scaling * (1.0 - gradient_filter) * self.gradient_previous[k]
                lo, hi = self.range[2 * (k % self.nu)], self.range[2 * (k % self.nu) + 1]
                v[k] = max(lo, min(hi, v[k]))
            candidates.append(v)
        out.update(gradient=list(self.gradient), gradient_previous=list(self.gradient_previous), candidates=candidates, magnitude=magnitude,
                   step_size=step_size)
        return out


def returns_of(kind, n, rng):
    r = rng.uniform(1.0, 50.0, n)
    if kind == "ties":
        r = np.round(r / 10.0) * 10.0 + 10.0    # a handful of values: ties everywhere, the nominal's among them
    elif kind == "nan":
        r[rng.integers(0, n, max(1, n // 5))] = np.nan
        r[-1] = np.nan
    elif kind == "failed":
        r[rng.integers(0, n, max(1, n // 3))] = 1.0e6
    elif kind == "nominal_best":
        r[0] = 0.125
    return r


KINDS = ["random", "ties", "nan", "failed", "nominal_best"]


@pytest.mark.parametrize("G", [0, 1, 63])
@pytest.mark.parametrize("num_noisy", [1, 2, 63, 64, 65])
def test_the_update_is_the_references(num_noisy, G):
    """sample_gradient_update against ReferenceLoops: order, winner, winner type and improvement exactly; the gradient and the next
    candidates within a bound from the operation count. Both sides compute t_i = z w_i / num_noisy with the same few roundings
    (w_i = f_i / den - 1 / num_noisy) but sum differently: the reference one after the other, (m - 1) rounded additions,
    sample_gradient_update by the device's strided tree, at most ceil(m / 256) - 1 + 8 <= m + 7 -- and den likewise, which moves
    f_i / den by 2 (m - 1) u relatively. With the 4 roundings of a term on either side, the two gradients differ by at most
        B_j = (4 m + 16) u * sum_i (f_i / den + 1 / m) / m |z_ij|,   m = num_noisy, u = 2^-53,
    the sum taken with |w_i| + 2 / m >= f_i / den + 1 / m. A candidate is nominal + a g + b g' clamped (1-Lipschitz), a = -s filter,
    b = -s (1 - filter): the difference is at most |a| B + |b| B' + 4 u (|nominal| + |a g| + |b g'|), B' the bound of the step before.
    Two steps: the first computes the weights, the second uses them cached, with returns that put a gradient candidate first."""
    n, P, nu = num_noisy + G, 3, 2
    num_parameters = P * nu
    ctrlrange = np.array([[-1.0, 1.0], [-0.4, 0.7]])
    noise_exploration, max_step, min_step = 0.1, 2.0, 1.0e-3
    for case, kind in enumerate(KINDS):
        rng = np.random.default_rng(100 * num_noisy + G + 1000 * case)
        ref = ReferenceLoops(num_parameters, ctrlrange, nu)
        weights, gradient = None, None
        bound_previous = np.zeros(num_parameters)
        for step, gradient_filter in enumerate((1.0, 0.3)):
            ret = returns_of(kind, n, rng)
            if step == 1 and G > 0:
                ret[n - 1] = 0.25                                   # a gradient candidate is the best of all: it sits in the cached order's head
            nominal = rng.uniform(-0.3, 0.3, num_parameters)
            noise = rng.normal(0, 1, (n, num_parameters))
            want = ref.update([float(x) for x in ret], nominal, noise, G, gradient_filter, max_step, min_step, noise_exploration)
            got = sample_gradient_update(ret, nominal, noise, G, ctrlrange, weights, gradient, compute_weights=step == 0,
                                         gradient_filter=gradient_filter, max_step=max_step, min_step=min_step, noise_exploration=noise_exploration)
            where = (kind, step)
            assert [int(i) for i in got["order"]] == want["order"], where
            assert got["winner"] == want["winner"] and got["winner_type"] == want["winner_type"], where
            assert got["improvement"] == want["improvement"], where
            if kind == "nominal_best":
                assert got["winner"] == 0 and got["winner_type"] == 0 and got["improvement"] == 0.0
            if G < 1:
                assert got["candidates"] is None and got["gradient"] is gradient
                continue
            if step == 1:
                assert (got["winner"], got["winner_type"]) == ((0, 0) if kind == "nominal_best" or math.isnan(ret[0]) else (n - 1, 2)), where   # (nothing is < a NaN nominal)
                assert np.array_equal(got["weights"], weights)                      # cached, not recomputed
                assert (got["order"][:min(num_noisy, 2)] >= num_noisy).any() or (kind == "nominal_best" and num_noisy == 1)   # a zero-noise row pairs with a weight
            bound = (4 * num_noisy + 16) * U * np.array(want["magnitude"])
            assert np.all(np.abs(got["gradient"] - np.array(want["gradient"])) <= bound), where
            assert np.array_equal(got["gradient_previous"], np.zeros(num_parameters) if gradient is None else gradient)
            for g in range(G):
                s = want["step_size"][g] / noise_exploration
                a, b = abs(s * gradient_filter), abs(s * (1.0 - gradient_filter))
                tol = a * bound + b * bound_previous + 4 * U * (np.abs(nominal) + a * np.abs(want["gradient"]) + b * np.abs(want["gradient_previous"]))
                assert np.all(np.abs(got["candidates"][g] - np.array(want["candidates"][g])) <= tol), (where, g)
            lo, hi = np.tile(ctrlrange[:, 0], P), np.tile(ctrlrange[:, 1], P)
            assert np.all(got["candidates"] >= lo) and np.all(got["candidates"] <= hi)
            weights, gradient, bound_previous = got["weights"], got["gradient"], bound
        if G > 0 and num_noisy > 2:
            assert np.any(gradient != 0.0)


def test_the_weights_take_the_candidate_index_not_the_rank():
    """the reference's quirk, kept: w[i] = max(0, f0 - log(order[i] + 1)) / den - 1 / m with the CANDIDATE at sorted position i"""
    ret = np.array([5.0, 1.0, 4.0, 2.0, 9.0])       # four noisy candidates and one gradient candidate: their order is 1, 3, 2, 0
    got = sample_gradient_update(ret, np.zeros(2), np.zeros((5, 2)), 1, [[-1, 1]])
    f0 = math.log(3.0)
    f = [max(0.0, f0 - math.log(c + 1)) for c in (1, 3, 2, 0)]
    assert np.allclose(got["weights"], np.array(f) / sum(f) - 0.25, rtol=0, atol=4 * U)
    by_rank = np.array([max(0.0, f0 - math.log(i + 1)) for i in range(4)]) / sum(f) - 0.25
    assert not np.allclose(got["weights"], by_rank, rtol=0, atol=1e-3)


def test_the_summation_order_is_the_strided_tree():
    x = np.random.default_rng(5).normal(0, 1, (700, 3))
    acc = [[0.0] * 3 for _ in range(256)]
    for i, row in enumerate(x):
        for k in range(3):
            acc[i % 256][k] += float(row[k])
    s = 128
    while s:
        for t in range(s):
            for k in range(3):
                acc[t][k] += acc[t + s][k]
        s //= 2
    assert np.array_equal(strided_tree_sum(x), np.array(acc[0]))


def test_the_emulated_sum_is_inside_the_additions_share_of_the_gradient_bound():
    """the numpy emulation of the device's summation order against the exact sum of the same terms: inside the additions' share of
    sample_gradient_cases.gradient_bound, (ceil(m / 256) + 8) u sum |t| -- the bound the device test uses was not fitted to the kernel"""
    rng = np.random.default_rng(2)
    for m in (1, 63, 257, 1087):
        terms = rng.normal(0, 1, (m, 4)) * rng.uniform(0, 1e-3, (m, 1))
        got = strided_tree_sum(terms)
        for j in range(4):
            exact = sum(Fraction(float(x)) for x in terms[:, j])
            bound = (math.ceil(m / 256) + 8) * Fraction(sgc.U) * sum(abs(Fraction(float(x))) for x in terms[:, j])
            assert abs(Fraction(float(got[j])) - exact) <= bound


# ---------------------------------------------------------------- fleet against members
def backend(task):
    return BatchSampleGradientOracleContext(task, threads=8)


def configure(p, task, G, n=N, gradient_filter=0.6):
    p.initialize(task.model, task)
    p.num_trajectory_, p.num_gradient_, p.gradient_filter_ = n, G, gradient_filter
    if task.name == "QuadrupedFlat":
        p.noise_exploration = 0.05
    p.allocate()
    return p


def order_of(ctx, e, n):
    ret = ctx.returns()[0][e * n:(e + 1) * n]
    return [int(i) for i in np.lexsort((np.arange(n), ret))]


def assert_member_equals_planner(batch, e, p, where):
    b = batch.envs[e]
    assert order_of(batch.ctx, e, N) == order_of(p.ctx, 0, N), where
    assert (b.winner, b.winner_type_, b.improvement) == (p.winner, p.winner_type_, p.improvement), where
    assert (b.best_return, b.nominal_return) == (p.best_return, p.nominal_return), where
    assert np.array_equal(b.gradient, p.gradient), where
    for mine, theirs in ((b.policy, p.policy), (b.previous_policy, p.previous_policy)):
        assert np.array_equal(mine.plan.times(), theirs.plan.times()), where
        assert np.array_equal(mine.plan.values(), theirs.plan.values()), where


def run_fleet_against_members(task, G, tasks=None, steps=STEPS, factory=backend):
    """factory: the contexts' backend (the oracle's here; None: the device's, tests/test_gpu_batch_sample_gradient.py)"""
    H = HORIZON[task.name]
    if task.name == "QuadrupedFlat":
        task.transition(0.0)
    batch = configure(GpuBatchSampleGradientPlanner(E, seed=SEED, backend_factory=factory), task, G)
    if tasks is not None:
        batch.set_tasks(tasks)
    singles = [configure(GpuSampleGradientPlanner(seed=SEED + e, backend_factory=factory), tasks[e] if tasks is not None else task, G) for e in range(E)]
    batch.reset(H)
    for p in singles:
        p.reset(H)
    states = initial_states(task)
    seen = []
    for step in range(steps):
        batch.set_states(states)
        batch.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            assert p.iteration == step + 1 == batch.envs[e].iteration
            assert_member_equals_planner(batch, e, p, (step, e))
            assert_same_trajectory(batch.best_trajectory(e), p.best_trajectory(), (step, e))
            x, y = np.zeros(task.model.nu), np.zeros(task.model.nu)
            batch.action_from_policy(e, x, None, states[e].time + 0.005)
            p.action_from_policy(y, None, states[e].time + 0.005)
            assert np.array_equal(x, y)
            seen.append((p.winner, p.winner_type_, p.gradient.copy()))
        step_along(task, states, singles)
    return batch, singles, seen


@pytest.mark.parametrize("G", [0, 5, 63])
@pytest.mark.parametrize("name", ["Cartpole", "Particle", "QuadrupedFlat"])
def test_fleet_is_one_sample_gradient_planner_per_environment(name, G):
    task = load_task(name)
    batch, singles, seen = run_fleet_against_members(task, G)
    assert batch.ctx.n_per_env == N and batch.ctx.N == E * N
    assert all(0 <= w < N and t == (0 if w == 0 else 1 if w < N - G else 2) for w, t, _ in seen)
    if G > 0:
        assert all(np.any(g != 0.0) for _, _, g in seen) if G < 63 else True      # (one noisy candidate, the nominal: a zero estimate)
        assert len({tuple(g) for _, _, g in seen}) == (len(seen) if G < 63 else 1)  # every robot, every step its own estimate
    else:
        assert all(not np.any(g) for _, _, g in seen)
    assert len({tuple(np.round(p.policy.plan.times(), 12)) for p in batch.envs}) == E   # three clocks


@pytest.mark.parametrize("name", ["Particle", "QuadrupedFlat"])
def test_fleet_with_tasks_is_one_sample_gradient_planner_per_task(name):
    """set_tasks: every robot its own weights, norm parameters, parameters and risk (the A1s their own gait and mode as well)"""
    task = load_task(name)
    if name == "QuadrupedFlat":
        task.transition(0.0)
    tasks = task_rows.unlike_tasks(task, E)
    batch, singles, _ = run_fleet_against_members(task, 5, tasks=tasks, steps=2)
    want = task_rows.rows_of(tasks)
    push = batch.ctx.pushes[-1]
    for key in ("weight", "norm_parameter", "parameters"):
        assert np.array_equal(push[key].reshape(want[key].shape), want[key]), key


def test_reset_zeroes_the_gradient_and_keeps_the_weights(cartpole):
    """Planner::Reset as the reference has it: gradient and gradient_previous zero, return_weight_ untouched"""
    H, G = HORIZON["Cartpole"], 5
    p = configure(GpuBatchSampleGradientPlanner(E, seed=SEED, backend_factory=backend), cartpole, G)
    flags = []
    update = p.ctx.sample_gradient_update_batched
    p.ctx.sample_gradient_update_batched = lambda E_, G_, f, *a: (flags.append(f), update(E_, G_, f, *a))[1]
    p.reset(H)
    states = initial_states(cartpole)
    for _ in range(2):
        p.set_states(states)
        p.optimize_policy(H)
    weights = p.ctx.sg["weights"].copy()
    assert all(np.any(q.gradient != 0.0) for q in p.envs) and np.any(p.ctx.sg_last[0]["gradient_previous"] != 0.0)
    p.reset(H)
    assert all(not np.any(q.gradient) and q.winner == 0 and q.improvement == 0.0 for q in p.envs)
    p.set_states(states)
    p.optimize_policy(H)
    assert flags == [capi.SG_COMPUTE_WEIGHTS | capi.SG_ZERO_GRADIENT, 0, capi.SG_ZERO_GRADIENT]
    assert all(not np.any(u["gradient_previous"]) for u in p.ctx.sg_last)           # the step after the reset starts from zero
    assert np.array_equal(p.ctx.sg["weights"], weights)                              # ... with the weights of before
    # and the gradient candidates of that step were the zero spline again, not what the update before the reset left
    n = p.ctx.n_per_env
    assert all(not np.any(p.ctx.nodes[e * n + n - G:(e + 1) * n]) for e in range(E))


def test_settings_as_initialize_reads_them(cartpole):
    p = GpuBatchSampleGradientPlanner(2, backend_factory=backend)
    p.initialize(cartpole.model, cartpole)
    m = cartpole.model
    assert p.noise_exploration == m.get_number("sampling_exploration", 0.1)
    assert p.num_trajectory_ == int(m.get_number("sampling_trajectories", 10))
    assert p.num_gradient_ == int(m.get_number("sample_gradient_trajectories", 0)) and p.gradient_filter_ == m.get_number("sample_gradient_filter", 1.0)
    p.allocate()
    assert p.envs[0].policy.num_spline_points == int(m.get_number("sampling_spline_points", 512))
    p.num_trajectory_ = 10
    with pytest.raises(ValueError, match="multiple of 64"):
        p.optimize_policy(10)
