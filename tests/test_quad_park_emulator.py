"""CPU tests of the quad kernel's parking (QArgs::park_hint, quad_abi.h) through the lock-step emulator: the SAME step source the device
build compiles, run as main pass, settling rule and resume pass (tests/quademu/quademu_park.cc). A1, N = 32, H = 30, from the bench's home
state and from the contact-rich trot state of the step bank (tests/step_bank.py: feet, calves, a thigh and a hip on the floor).

Everything compared is exact. A step's cost is > 0 here, so a candidate's partial returns grow strictly: with the hint at its partial
return of step k - 1 (0 for k = 0) a candidate is parked at step k and at no earlier one -- the emulator gives each candidate a hint of its
own. With the initial bound at the launch's minimum the bound never moves, and what is parked, settled and resumed is a function of the
plain launch's costs that numpy computes."""
import numpy as np
import pytest

import step_bank as sb
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task
from tests.quademu import park

MOCAP = np.array([0.3, 0, 0.26, 1, 0, 0, 0, -2.5, 0, 0, 1, 0, 0, 0.0])
N, H, P = 32, 30, 3
BUFFERS = ("states", "actions", "times", "residual", "costs", "trace")
ALL = BUFFERS + ("total_return", "failure")


@pytest.fixture(scope="module")
def quad():
    t = load_task("QuadrupedFlat")
    t.transition(0.0)
    return t


@pytest.fixture(scope="module", params=["home", "trot"])
def case(quad, request):
    """the candidates (0 is the nominal: zero noise; the others with growing noise, so that the returns spread) and their plain rollout"""
    pm, pt = quad.packed_model(), quad.packed()
    if request.param == "home":
        state, time = np.concatenate([quad.model.keyframes["home"]["qpos"], np.zeros(18)]), 0.0
    else:
        s = next(s for s in sb.a1_bank().states if s.label.startswith("trot3/"))
        state, time = np.array(s.state), float(s.time)
    times = time + np.arange(P) * ((H - 1) * 0.01 / P)
    rng = np.random.default_rng(5)
    sigma = np.linspace(0.0, 0.25, N)[:, None, None]
    nodes = np.clip(rng.normal(0, 1, (N, P, 12)) * sigma, -1, 1)
    args = (pm, pt, state, time, MOCAP, N, H, P, capi.SPLINE_ZERO, times, nodes)
    full = park.rollout(*args, initial_bound=None)
    assert not full["failure"].any() and full["costs"].min() > 0
    assert np.array_equal(full["total_return"], np.cumsum(full["costs"], axis=1)[:, -1] / float(H))
    for a in full.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return args, full


def hints_for_step(costs, k):
    """per candidate: the hint that parks it at step k exactly (its partial return one step earlier; strictly-greater does not park on a tie)"""
    partial = np.cumsum(costs, axis=1) / float(H)
    return np.zeros(len(costs)) if k == 0 else partial[:, k - 1].copy()


@pytest.mark.parametrize("k", [0, 1, 7, H - 2])
def test_round_trip_of_every_candidate_at_step_k(case, k):
    """every candidate parked at step k (no nominal: none is exempt), none retired (nothing completes in the main pass: the bound stays at
    +inf), all resumed and rolled to the horizon: every buffer, return and failure word is the uninterrupted rollout's"""
    args, full = case
    run = park.rollout(*args, nominal_candidate=-1, initial_bound=np.inf, hint=hints_for_step(full["costs"], k), resume_unpruned=True)
    assert (run["park_step"] == k).all() and run["resumed"].all()
    assert (run["parked"], run["settled_retired"], run["resumed_count"]) == (N, 0, N) and run["bound_settle"] == np.inf
    for key in ALL:
        assert np.array_equal(run[key], full[key]), key


def test_a_candidate_that_hands_on_after_its_resume_is_flagged_with_the_right_step(case):
    """QArgs::con_cap = c hands on a candidate when a leg holds more than c contacts (the smallest c at which some candidate of the case
    is handed on at a step s >= 2: from the trot state every candidate holds two at step 0). Those candidates are parked at s - 1 and
    resumed: their failure word (marker, reason, step s) and their rows up to s are those of the launch that never parked"""
    args, _ = case
    for cap in range(1, 12):
        ref = park.rollout(*args, initial_bound=None, con_cap=cap)
        step = (ref["failure"] >> 8) & 0xFFFF
        late = ((ref["failure"] & park.FALLBACK) != 0) & (step >= 2) & (step < H - 1)
        if late.any():
            break
    assert late.any(), ref["failure"]
    partial = np.cumsum(ref["costs"], axis=1) / float(H)
    hints = np.full(N, np.inf)
    hints[late] = partial[late, step[late] - 2]   # parked at s - 1
    run = park.rollout(*args, nominal_candidate=-1, initial_bound=np.inf, hint=hints, resume_unpruned=True, con_cap=cap)
    assert np.array_equal(run["park_step"][late], step[late] - 1) and run["resumed"][late].all() and (run["park_step"][~late] == -1).all()
    for key in ALL:
        assert np.array_equal(run[key][late], ref[key][late]), key
    # (the others ran with pruning against what completed: those not retired are the reference's too)
    kept = (run["failure"] & park.PRUNED) == 0
    for key in ALL:
        assert np.array_equal(run[key][kept], ref[key][kept]), key


def expected_with_fixed_bound(costs, bound, hint, nominal=0):
    """bound fixed at the launch's minimum: per candidate the park step (-1: never), whether the settling rule retires it, and the final
    retire step (-1: completes). Per step the proven test comes first, then the hint; neither at the last step; never the nominal"""
    partial = np.cumsum(costs, axis=1) / float(H)
    parked, settled, final = np.full(len(costs), -1), np.zeros(len(costs), bool), np.full(len(costs), -1)
    for c in range(len(costs)):
        if c == nominal:
            continue
        for t in range(H - 1):
            if partial[c, t] > bound:
                final[c] = t
                break
            if parked[c] < 0 and partial[c, t] > hint:
                parked[c] = t   # (the proven test has just failed against the same bound: the settling rule cannot retire it; it goes on)
    return parked, settled, final, partial


@pytest.mark.parametrize("which", ["minimum", "half", "zero", "inf"])
def test_the_settling_rule_with_the_bound_at_the_minimum(case, which):
    args, full = case
    best = full["total_return"].min()
    hint = {"minimum": best, "half": 0.5 * best, "zero": 0.0, "inf": np.inf}[which]
    parked, settled, final, partial = expected_with_fixed_bound(full["costs"], best, hint)
    run = park.rollout(*args, nominal_candidate=0, initial_bound=best, hint=hint)
    assert run["bound"] == best and run["bound_settle"] == best
    assert np.array_equal(run["park_step"], parked)
    assert run["parked"] == (parked >= 0).sum() and run["settled_retired"] == settled.sum() and run["resumed_count"] == ((parked >= 0) & ~settled).sum()
    assert np.array_equal(run["resumed"], (parked >= 0) & ~settled)
    if which in ("minimum", "inf"):
        assert run["parked"] == 0   # above the minimum the proven test retires first; +inf is off
    if which == "zero":
        assert run["parked"] == N - 1 and (parked[1:] == 0).all()
    # a hint below the minimum parks before anything can be retired: nothing is settled-retired, everything parked is resumed
    if which in ("half", "zero"):
        assert run["parked"] > 0 and run["settled_retired"] == 0
    retired = final >= 0
    assert 0 < retired.sum() < N - 1
    assert np.array_equal(run["failure"], np.where(retired, park.PRUNED | (final << 8), 0))
    assert run["prune_stats"][0] == retired.sum() and run["prune_stats"][1] == final[retired].sum() and run["prune_stats"][2] == 0
    for c in range(N):
        t = final[c] if retired[c] else H - 1
        assert run["total_return"][c] == partial[c, t], c
        for key in BUFFERS:
            assert np.array_equal(run[key][c, :t + 1], full[key][c, :t + 1]), (key, c)
            assert not run[key][c, t + 1:].any(), (key, c)   # rows beyond the retire step are not written, by either pass
    assert (full["total_return"][retired] > run["bound"]).all()


@pytest.mark.parametrize("which", ["minimum", "half", "zero", "inf"])
def test_the_settling_rule_with_no_initial_bound(case, which):
    """as the planner launches: the bound starts at +inf and falls as candidates complete, so which candidates are retired depends on the
    finish order. What may not: parked = settled-retired + resumed, no parked marker survives, every retired candidate's plain return
    is strictly above the final bound, every other candidate equals the plain launch, and the argmin is the plain launch's"""
    args, full = case
    best = full["total_return"].min()
    hint = {"minimum": best, "half": 0.5 * best, "zero": 0.0, "inf": np.inf}[which]
    run = park.rollout(*args, nominal_candidate=0, initial_bound=np.inf, hint=hint)
    assert run["parked"] == run["settled_retired"] + run["resumed_count"] == (run["park_step"] >= 0).sum()
    if which == "inf":
        assert run["parked"] == 0
    if which in ("half", "zero"):   # (at the minimum itself a candidate is parked only if it passes the hint before anything has completed)
        assert run["parked"] > 0
    assert ((run["failure"] & park.PARKED) == 0).all() and ((run["failure"] & park.FALLBACK) == 0).all()
    retired = (run["failure"] & park.PRUNED) != 0
    assert not retired[0] and run["park_step"][0] == -1   # the nominal
    assert run["bound"] == best and run["bound_settle"] >= best
    assert (full["total_return"][retired] > run["bound"]).all() and (run["total_return"][retired] > run["bound"]).all()
    assert run["prune_stats"][0] == retired.sum()
    for key in ALL:
        assert np.array_equal(run[key][~retired], full[key][~retired]), key
    assert run["total_return"].argmin() == full["total_return"].argmin()
