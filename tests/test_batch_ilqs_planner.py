"""GpuBatchILQSPlanner and mjpcx_ilqg_step_batched_from without a device: the symbol is declared, exported and bound, and the fleet
planner is, member by member and exactly, E single GpuILQSPlanners -- with the device chain (one ilqg_step_batched_from per plan step,
tests/batch_ilqs_oracle_backend.py: each nominal fetched from the backend its member names) and with device_chain = False. Every side
runs the CPU oracle, so equality is exact.
Two fleets of E = 3, H = 12, 64 candidates, 8 plans:
 (a) Particle with exploration 0, states held: member 0 sits on the goal at rest -- its cost is exactly 0, iLQG never beats it, it hands
     off from sampling at every plan --, members 1 and 2 switch to iLQG at plan 0 and stay: the step call's from_source is [1, 1, 1] at
     plan 0 and [1, 0, 0] afterwards, the mixed fleet;
 (b) Cartpole, default exploration, seed 0, a new state per member and plan: nobody leaves sampling in plans 0-5, member 2 alone runs iLQG
     at plan 6 and activates it (two members sit out), and at plan 7 it alone is in the nominal phase, with two riders."""
import os
import re

import numpy as np
import pytest

from batch_ilqs_oracle_backend import BatchILQSOracleContext
from batch_oracle_backend import BatchOracleContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import GpuBatchILQSPlanner, GpuILQSPlanner, State
from mujoco_mpc_amd.task import load_task
from oracle_backend import OracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, H, N, PLANS = 3, 12, 64, 8


def test_the_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpcx.h")).read()
    assert re.search(r"\bint mjpcx_ilqg_step_batched_from\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "mjpcx_ilqg_step_batched_from" in capi.EXPORTS
    assert hasattr(capi.lib(), "mjpcx_ilqg_step_batched_from") and callable(getattr(capi.Context, "ilqg_step_batched_from"))
    doc = text[:text.index("int mjpcx_ilqg_step_batched_from")]
    doc = doc[doc.rindex("/*"):]
    for cite in ("ilqs/planner.cc:87-214", "ilqg.candidate_policy[0].trajectory = sampling.trajectory[0]", "ilqg/planner.cc:377-520",
                 "model_derivatives.cc:45-165", "cost_derivatives.cc:112-230", "backward_pass.cc:65-356"):
        assert cite in doc, cite


# ------------------------------------------------------------------------------------------------ the two fleets
def particle_states(task, k):
    goal = State(task.model).mocap[:2].copy()
    out = []
    for q in (goal, np.zeros(2), goal + np.array([0.15, -0.1])):
        st = State(task.model)
        st.set(q, [0.0, 0.0])
        out.append(st)
    return out


def cartpole_states(task, k):
    out = []
    for e in range(E):
        rng = np.random.default_rng(1000 + 10 * e + k)
        push = 1.0 if (k + e) % 3 == 2 else 0.0
        st = State(task.model)
        st.set(np.array([0.3 + 0.1 * e, 2.5 - 0.2 * e]) + rng.normal(0, 0.3, 2) * push, [-0.2, 0.4], time=0.01 * k + 0.1 * e)
        out.append(st)
    return out


FLEETS = {"Particle": (particle_states, 0.0), "Cartpole": (cartpole_states, None)}


def make_fleet(task, exploration, device_chain=None):
    def backend(t, half):
        return (BatchOracleContext if half == "sampling" else BatchILQSOracleContext)(t, threads=8, differentiable=True)
    p = GpuBatchILQSPlanner(E, seed=0, backend_factory=backend)
    p.initialize(task.model, task)
    p.sampling.num_trajectory_ = N
    if exploration is not None:
        for m in p.sampling.envs:
            m.noise_exploration[0] = exploration
    p.allocate()
    p.reset(H)
    p.device_chain = device_chain
    return p


def make_singles(task, exploration):
    out = []
    for e in range(E):
        p = GpuILQSPlanner(seed=e, backend_factory=lambda t: OracleContext(t, threads=8, differentiable=True))
        p.initialize(task.model, task)
        p.sampling.num_trajectory_ = N
        if exploration is not None:
            p.sampling.noise_exploration[0] = exploration
        p.allocate()
        p.reset(H)
        out.append(p)
    return out


def same_plan(a, b):
    return a.interpolation() == b.interpolation() and np.array_equal(a.times(), b.times()) and np.array_equal(a.values(), b.values())


def assert_member_equal(a, b, nu, where):
    """a, b: two iLQS planners (a fleet's member or a single one)"""
    assert (a.active_policy, a.previous_active_policy, a.ilqg_ran) == (b.active_policy, b.previous_active_policy, b.ilqg_ran), where
    assert (a.fit_status, a.fit_unreached) == (b.fit_status, b.fit_unreached), where
    assert (a.last_fit is None) == (b.last_fit is None), where
    if a.last_fit is not None:
        for k in a.last_fit:
            assert np.array_equal(a.last_fit[k], b.last_fit[k]), (where, k)
    sa, sb = a.sampling, b.sampling
    assert (sa.winner, sa.best_return, sa.nominal_return, sa.improvement) == (sb.winner, sb.best_return, sb.nominal_return, sb.improvement), where
    for name in ("policy", "previous_policy", "winner_policy"):
        assert same_plan(getattr(sa, name).plan, getattr(sb, name).plan), (where, name)
    ga, gb = a.ilqg, b.ilqg
    assert np.array_equal(ga.dV, gb.dV) and ga.regularization == gb.regularization and ga.regularization_rate == gb.regularization_rate, where
    assert (ga.winner, ga.action_step, ga.feedback_scaling, ga.iteration_completed) == (gb.winner, gb.action_step, gb.feedback_scaling,
                                                                                       gb.iteration_completed), where
    assert (ga.improvement, ga.expected, ga.surprise) == (gb.improvement, gb.expected, gb.surprise), where
    for name in ("policy", "previous_policy", "candidate0"):
        pa, pb = getattr(ga, name), getattr(gb, name)
        assert pa.trajectory.total_return == pb.trajectory.total_return and pa.trajectory.failure == pb.trajectory.failure, (where, name)
        for k in ("states", "actions", "times", "residual", "costs", "trace"):
            assert np.array_equal(getattr(pa.trajectory, k)[:H], getattr(pb.trajectory, k)[:H]), (where, name, k)
        assert np.array_equal(pa.feedback_gain[:H], pb.feedback_gain[:H]), (where, name)
        assert np.array_equal(pa.action_improvement[:H], pb.action_improvement[:H]), (where, name)
        assert pa.feedback_scaling == pb.feedback_scaling, (where, name)
    x = np.asarray(a.sampling.state, float) + 0.01
    for use_previous in (False, True):
        for t in a.sampling.time + np.array([0.0, 0.013, 0.05, 0.11, 0.4]):
            ua, ub = np.zeros(nu), np.zeros(nu)
            a.action_from_policy(ua, x, t, use_previous)
            b.action_from_policy(ub, x, t, use_previous)
            assert np.array_equal(ua, ub), (where, use_previous, t)


@pytest.fixture(scope="module", params=sorted(FLEETS))
def run(request):
    """the fleet with the chain, the fleet without, E single planners: 8 plans side by side, compared after each; the history"""
    name = request.param
    states_of, exploration = FLEETS[name]
    task = load_task(name)
    chain, plain, singles = make_fleet(task, exploration), make_fleet(task, exploration, device_chain=False), make_singles(task, exploration)
    history = []
    for k in range(PLANS):
        states = states_of(task, k)
        for p in (chain, plain):
            p.set_states(states)
            p.optimize_policy(H)
        for e, p in enumerate(singles):
            p.set_state(states[e])
            p.optimize_policy(H)
        for e in range(E):
            assert_member_equal(chain.envs[e], singles[e], task.model.nu, ("fleet = single", name, k, e))
            assert_member_equal(plain.envs[e], chain.envs[e], task.model.nu, ("no chain = chain", name, k, e))
        assert plain.last_step is None and plain.ilqg.ctx.from_calls == []
        history.append(dict(previous=list(chain.previous_active_policy), active=list(chain.active_policy), ran=list(chain.ilqg_ran),
                            fit=list(chain.fit_status), last_step=chain.last_step, calls=len(chain.ilqg.ctx.from_calls),
                            timers=dict(chain.timers)))
    return name, chain, history


def test_fleet_equals_single_planners_and_the_sequential_middle(run):
    name, chain, history = run
    S, G = chain.SAMPLING, chain.ILQG
    if name == "Particle":
        # member 0: cost 0 on the goal, never beaten; members 1 and 2 switch at plan 0 and stay
        for k, h in enumerate(history):
            assert h["active"] == [S, G, G] and h["ran"] == [True] * E, (k, h)
            assert h["previous"] == ([S, S, S] if k == 0 else [S, G, G]), (k, h)
            assert h["calls"] == k + 1                                # ONE step call per plan
            assert h["last_step"][0] == ([1, 1, 1] if k == 0 else [1, 0, 0]), (k, h)
            assert h["last_step"][1][0] == 0 and min(h["last_step"][1]) >= 0 and h["last_step"][2] == [1] * E, (k, h)
            assert set(h["timers"]) == {"nominal", "fit", "sampling", "handoff", "derivatives_backward", "rollouts"}
            assert (h["timers"]["nominal"] > 0) == (k > 0) and h["timers"]["derivatives_backward"] > 0 and h["timers"]["rollouts"] > 0
        assert chain.ilqg.ctx.from_calls[3][0] == [1, 0, 0] and chain.ilqg.ctx.step_calls == []
    else:
        for k in range(6):
            assert history[k]["active"] == [S] * E and history[k]["ran"] == [False] * E and history[k]["last_step"] is None, (k, history[k])
        h = history[6]                                                # member 2 alone runs iLQG and activates it: two sit out
        assert h["previous"] == [S] * E and h["ran"] == [False, False, True] and h["active"] == [S, S, G], h
        assert h["last_step"] == ([0, 0, 1], [-1, -1, 0], [-1, -1, 1]), h
        h = history[7]                                                # member 2 alone in the nominal phase, two riders; sampling wins it back
        assert h["previous"] == [S, S, G] and h["fit"] == [-1, -1, 0] and h["timers"]["nominal"] > 0, h
        assert h["ran"] == [False] * E and h["active"] == [S] * E and h["last_step"] is None, h
        assert history[7]["calls"] == 1


def test_refusals():
    task = load_task("Particle")
    p = make_fleet(task, 0.0)
    p.sampling.num_trajectory_ = 10
    p.set_states(particle_states(task, 0))
    with pytest.raises(ValueError, match="multiple of 64"):
        p.optimize_policy(H)
    from batch_ilqg_step_oracle_backend import BatchILQGStepOracleContext
    q = GpuBatchILQSPlanner(E, backend_factory=lambda t, half: (BatchOracleContext if half == "sampling" else BatchILQGStepOracleContext)(
        t, differentiable=True))
    q.initialize(task.model, task)
    q.sampling.num_trajectory_ = N
    for m in q.sampling.envs:
        m.noise_exploration[0] = 0.0                                  # sampling never wins: everybody goes on to iLQG
    q.allocate()
    q.reset(H)
    q.device_chain = True                                             # asked for on a backend without the call
    q.set_states(particle_states(task, 0))
    with pytest.raises(ValueError, match="without ilqg_step_batched_from"):
        q.optimize_policy(H)
    with pytest.raises(ValueError, match="at least one environment"):
        GpuBatchILQSPlanner(0)
