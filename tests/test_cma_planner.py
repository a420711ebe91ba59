"""GpuBatchCMAESPlanner / GpuCMAESPlanner (mujoco_mpc_amd/planners.py) on the oracle-backed test backend (batch_cmaes_oracle_backend.py:
the candidates and the update in numpy, in the device's order of operations). Both sides of every comparison run the oracle, so equality
is exact. Particle and Cartpole, E = 3, 64 candidates, H <= 16."""
import numpy as np
import pytest

from batch_cmaes_oracle_backend import STATE_KEYS, BatchCmaOracleContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchCMAESPlanner, GpuCMAESPlanner, cma_parameters
from mujoco_mpc_amd.task import load_task
from selection_cases import same_bits
from test_batch_planner import initial_states
from test_mppi_planner import HORIZON, advance, same_policy

E, N, SEED = 3, 64, 5
MEMBER_KEYS = ("winner", "best_return", "nominal_return", "improvement", "sigma", "restarted", "valid")


def ready(p, task, n=N):
    p.initialize(task.model, task)
    p.num_trajectory_ = n
    p.allocate()
    p.reset(HORIZON[task.name])
    return p


def fleet(task, num_envs=E, seed=SEED, **kw):
    return ready(GpuBatchCMAESPlanner(num_envs, seed=seed, backend_factory=lambda t: BatchCmaOracleContext(t), **kw), task)


def single(task, seed, **kw):
    return ready(GpuCMAESPlanner(seed=seed, backend_factory=lambda t: BatchCmaOracleContext(t), **kw), task)


def state_of(p, d):
    return p.ctx.cma_get_state_batched(len(p.ctx.cma), d)


def same_state(a, b):
    return all(same_bits(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)) for k in STATE_KEYS)


@pytest.mark.parametrize("name", ["Cartpole", "Particle"])
def test_a_fleets_member_is_the_single_planner(name, cartpole, particle):
    task = cartpole if name == "Cartpole" else particle
    H = HORIZON[name]
    batch = fleet(task)
    singles = [single(task, SEED + e) for e in range(E)]
    assert not hasattr(batch, "pruning")
    states = initial_states(task, name)
    d = batch.num_parameters()
    dt = task.model.get_number("agent_timestep", task.model.timestep)
    for step in range(2):
        batch.set_states(states)
        batch.optimize_policy(H)
        whole = state_of(batch, d)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
            b = batch.envs[e]
            assert same_policy(b, p), (step, e)
            for k in MEMBER_KEYS:
                assert getattr(b, k) == getattr(p, k), (step, e, k)
            assert same_state({k: whole[k][e:e + 1] for k in STATE_KEYS}, state_of(p.fleet, d)), (step, e)
            x, y = np.zeros(task.model.nu), np.zeros(task.model.nu)
            batch.action_from_policy(e, x, None, states[e].time + 0.5 * dt)
            p.action_from_policy(y, None, states[e].time + 0.5 * dt)
            assert np.array_equal(x, y)
            tb, ts = batch.best_trajectory(e), p.best_trajectory()
            assert np.array_equal(tb.states, ts.states) and tb.total_return == ts.total_return == p.best_return
        assert np.array_equal(whole["generation"], [step + 1] * E)
        advance(task, states, [p.best_trajectory() for p in singles])
    # the distribution moved: a step size that is no longer sigma0, a covariance that is no longer the identity, paths that are not zero
    assert all(p.sigma != singles[0].noise_exploration[0] for p in singles) and not np.array_equal(whole["C"][0], np.eye(d))
    assert np.abs(whole["p_sigma"]).max() > 0 and np.allclose(whole["A"] @ np.swapaxes(whole["A"], 1, 2), whole["C"], rtol=1e-12, atol=1e-14)
    assert len({p.winner for p in singles} | {0}) > 1                     # somebody left the mean


@pytest.mark.parametrize("name", ["Cartpole", "Particle"])
def test_two_generations_are_two_plan_steps_from_a_frozen_state(name, cartpole, particle):
    task = cartpole if name == "Cartpole" else particle
    H = HORIZON[name]
    twice, once = fleet(task, generations=2), fleet(task)
    states = initial_states(task, name)
    twice.set_states(states)
    twice.optimize_policy(H)
    once.set_states(states)
    once.optimize_policy(H)
    first = [p.policy.plan.values().copy() for p in once.envs]
    once.optimize_policy(H)                                               # the same states: the mean is resampled at the same times
    d = once.num_parameters()
    assert same_state(state_of(twice, d), state_of(once, d)) and twice.iteration == once.iteration == 2
    for e in range(E):
        assert same_policy(twice.envs[e], once.envs[e]), e
        assert all(getattr(twice.envs[e], k) == getattr(once.envs[e], k) for k in MEMBER_KEYS), e
        assert not np.array_equal(once.envs[e].policy.plan.values(), first[e])   # the second generation moved the mean again
    with pytest.raises(ValueError, match="generations"):
        fleet(task, generations=0).optimize_policy(H)


def test_reset_and_a_change_of_spline_points_restore_the_state(particle):
    H = HORIZON["Particle"]
    p = fleet(particle, sigma0=[0.05, 0.1, 0.2], sigma_min=0.01, sigma_max=0.5)
    states = initial_states(particle, "Particle")
    d = p.num_parameters()
    p.set_states(states)
    p.optimize_policy(H)
    moved = state_of(p, d)
    assert not np.array_equal(moved["sigma"], [0.05, 0.1, 0.2]) and np.all(moved["generation"] == 1)
    assert np.all(moved["sigma"] >= 0.01) and np.all(moved["sigma"] <= 0.5)
    first = [(q.winner, q.best_return, q.sigma) for q in p.envs]
    p.reset(H)
    p.set_states(states)
    p.iteration = 0                                                       # (the noise counter: the same candidates again)
    p.optimize_policy(H)
    assert same_state(state_of(p, d), moved) and [(q.winner, q.best_return, q.sigma) for q in p.envs] == first
    points = p.envs[0].policy.num_spline_points
    for q in p.envs:                                                      # another number of spline points: another d, a fresh state
        q.policy.num_spline_points = q.winner_policy.num_spline_points = points + 1
    p.optimize_policy(H)
    d2 = (points + 1) * particle.model.nu
    fresh = state_of(p, d2)
    assert fresh["C"].shape == (E, d2, d2) and np.all(fresh["generation"] == 1)


def test_a_member_whose_returns_are_nan_keeps_its_policy_and_its_distribution(particle):
    H = HORIZON["Particle"]
    p = fleet(particle)
    states = initial_states(particle, "Particle")
    d = p.num_parameters()
    p.set_states(states)
    p.optimize_policy(H)
    before = [(q.policy.plan.times().copy(), q.policy.plan.values().copy()) for q in p.envs]
    kept = state_of(p, d)
    p.ctx.nan_envs = (1,)
    p.optimize_policy(H)
    after, q = state_of(p, d), p.envs[1]
    assert q.valid == 0 and q.restarted == 0 and np.isnan(q.best_return) and q.sigma == kept["sigma"][1]
    assert same_state({k: after[k][1:2] for k in STATE_KEYS}, {k: kept[k][1:2] for k in STATE_KEYS})
    assert np.array_equal(q.policy.plan.times(), before[1][0]) and same_bits(q.policy.plan.values(), before[1][1])
    for e in (0, 2):
        assert p.envs[e].valid == 1 and after["generation"][e] == 2 and not np.array_equal(p.envs[e].policy.plan.values(), before[e][1])


def test_refusals_raise(particle):
    H = HORIZON["Particle"]
    p = fleet(particle)
    p.set_states(initial_states(particle, "Particle"))
    p.num_trajectory_ = 100                                               # not a multiple of 64
    with pytest.raises(ValueError, match="multiple of 64"):
        p.optimize_policy(H)
    p.num_trajectory_ = N
    for q in p.envs:                                                      # 65 spline points x 2 actuators = 130 parameters
        q.policy.num_spline_points = q.winner_policy.num_spline_points = capi.CMA_MAX_PARAMS // particle.model.nu + 1
    with pytest.raises(ValueError, match="130 parameters"):
        p.optimize_policy(H)
    with pytest.raises(ValueError):
        GpuBatchCMAESPlanner(0)
    ctx = BatchCmaOracleContext(particle)
    ctx.set_states(np.zeros((1, 4)), np.zeros(1))
    with pytest.raises(ValueError, match="no state"):
        ctx.rollout_cma_batched(N, H, capi.SPLINE_CUBIC, np.linspace(0, 0.1, 3)[None], np.zeros((1, 3, 2)))
    bad = np.eye(6)
    bad[0, 0] = -1.0
    with pytest.raises(ValueError, match="environment 0"):
        ctx.cma_set_state_batched(1, 6, 0.1, bad[None])
    prm = dict(cma_parameters(6, N - 1), sigma_min=1e-6, sigma_max=1.0, pivot_floor=0.0)
    ctx.cma_set_state_batched(1, 6, 0.1)
    with pytest.raises(ValueError, match="not a rollout_cma_batched"):
        ctx.cma_update_batched(1, prm)


def test_the_hansen_defaults():
    prm = cma_parameters(10, 63)
    assert prm["mu"] == 31 and abs(prm["weights"].sum() - 1) < 1e-15 and np.all(np.diff(prm["weights"]) < 0)
    assert prm["c_one"] + prm["c_mu"] <= 1 and 0 < prm["c_sigma"] < 1 and 0 < prm["c_c"] < 1 and prm["d_sigma"] > 1
