"""-m gpu: every device copy of the sampling policy -- the candidate nodes clamp(nominal + sigma z) and the action
clamp(TimeSpline::Sample(nodes, time)) of every step -- held to exact answers (tests/sampling_policy_cases.py: Philox in integers and the
normals in mpmath from the text of include/mjpcx.h, the spline in rational arithmetic, the derived bounds, the comparison rule).

   lane family          Cartpole (nu = 1) and Particle (nu = 2), fp64 and fp32; 70 candidates (a full wavefront and a ragged one)
   generic wave kernel  tests/models/capsules_tendon.xml in fp64 and fp32; the A1 under MJPCX_NO_LDS_MODEL=1 (P nu > 128)
   registered tree      the A1 under MJPCX_NO_QUAD=1; the Humanoid under MJPCX_NO_LIMB=1, fp64 and fp32
   quad form            the A1 under MJPCX_QUAD_MIN_N=64, 64 candidates, quad_stats()["handed_on"] == 0
   limb form            the Humanoid under MJPCX_LIMB_MIN_N=64, fp64 and fp32, 64 candidates, none handed on
   batched              one rollout_noise_batched and one rollout_noise_batched_ce launch per family: E = 3 environments of 64 candidates
                        (n_per_env is a multiple of 64), seed + e, each its own node times, clock and (CE) variance row; H = 12 cubic, so
                        the same launch is held to the exact spline as well; seven candidates of every environment are compared
The kernel that ran is asserted each time. The quad and limb forms launch 64 candidates and compare ten of them (the exact references are
Python): the first quad, lanes across the wavefront and the last. Every test prints its census and the worst error / bound."""
import numpy as np
import pytest

import feedback_policy_cases as fpc
import sampling_policy_cases as spc
from mujoco_mpc_amd import capi

pytestmark = pytest.mark.gpu

# family: (model, precision, environment, what the kernel name must hold, candidates per launch, the rows compared)
ROWS64 = (0, 1, 2, 3, 17, 31, 32, 33, 62, 63)
FAMILIES = {
    "cartpole64": ("cartpole", 64, {}, "rollout_lane", 70, None),
    "cartpole32": ("cartpole", 32, {}, "rollout_lane", 70, None),
    "particle64": ("particle", 64, {}, "rollout_lane", 70, None),
    "particle32": ("particle", 32, {}, "rollout_lane", 70, None),
    "scene64": ("scene", 64, {}, "rollout_wave_kernel", 5, None),
    "scene32": ("scene", 32, {}, "rollout_wave_kernel", 5, None),
    "a1_generic": ("a1", 64, {"MJPCX_NO_LDS_MODEL": "1"}, "rollout_wave_kernel", 5, None),
    "a1_tree": ("a1", 64, {"MJPCX_NO_QUAD": "1"}, "rollout_tree_kernel<A1>", 5, None),
    "humanoid_tree64": ("humanoid", 64, {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>", 5, None),
    "humanoid_tree32": ("humanoid", 32, {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>", 5, None),
    "a1_quad": ("a1", 64, {"MJPCX_QUAD_MIN_N": "64"}, "rollout_quad_kernel", 64, ROWS64),
    "limb64": ("humanoid", 64, {"MJPCX_LIMB_MIN_N": "64"}, "rollout_limb_kernel", 64, ROWS64),
    "limb32": ("humanoid", 32, {"MJPCX_LIMB_MIN_N": "64"}, "rollout_limb_kernel", 64, ROWS64),
}
FOUR_LANES = ("a1_quad", "limb64", "limb32")
BATCH_ROWS = (0, 1, 2, 31, 32, 33, 63)
EUNSUPPORTED = -2      # MJPCX_EUNSUPPORTED (include/mjpcx.h)


def make_context(name, monkeypatch):
    model, precision, env, kernel, _, _ = FAMILIES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = capi.Context(*fpc.packed(model), 0, precision)
    assert kernel in ctx.kernel_name, ctx.kernel_name
    return ctx


def own_numbers(name, ctx):
    """the four-lane forms handed no candidate on: the numbers are theirs"""
    if name in FOUR_LANES:
        assert ctx.quad_stats()["handed_on"] == 0 and not (ctx.failure_raw & 0x40000000).any()


def s8_nodes(name):
    return 63 if name == "particle64" else 70      # (P nu 64 + P) * 8 bytes of LDS: the Particle in fp64 stages at most 63 nodes


@pytest.mark.parametrize("group", list(spc.GROUPS))
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_kernel_follows_the_exact_spline(name, group, monkeypatch):
    model, precision, _, _, N, rows = FAMILIES[name]
    ctx = make_context(name, monkeypatch)

    def run(interp, knots, nodes):
        out = spc.run_spline_device(ctx, model, interp, knots, nodes)
        own_numbers(name, ctx)
        return out
    total = spc.spline_group(model, group, run, precision, n_lane=N, n_other=N, P8=s8_nodes(name), rows=rows)
    ctx.close()
    print(f"{name} {group}: worst error / bound {total.worst:.3f} ({total.where}); largest bound / range {total.worst_bound:.2e}; {total}")
    total.assert_shares((name, group), spc.GROUPS[group][1])


def test_one_node_more_than_the_lds_stage_holds_is_refused(monkeypatch):
    ctx = make_context("particle64", monkeypatch)
    with pytest.raises(capi.MjpcxError) as e:
        spc.run_spline_device(ctx, "particle", 2, spc.knots_of("particle", "S8", 64), spc.node_values("particle", "S8", 64, 4))
    ctx.close()
    assert e.value.code == EUNSUPPORTED, e.value


def noise_launches(name):
    model, _, _, _, N, rows = FAMILIES[name]
    if model == "scene":
        N = 40       # (one actuator: forty candidates for a census worth the name)
    return spc.noise_cases(model, N, rows=rows) + spc.searched_cases(model, N=max(N, 3) if rows else 3) + [spc.bernoulli_case(model, N=max(N, 3) if rows else 3)]


@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_kernel_draws_the_exact_nodes(name, monkeypatch):
    """sampling and cross-entropy modes, the searched counters (tails, log near 0, the roots and extrema of both functions) and the
    Bernoulli window, in which every copy takes std0"""
    model, precision = FAMILIES[name][:2]
    ctx = make_context(name, monkeypatch)
    total, normal = spc.Census(), spc.Census()
    for case in noise_launches(name):
        got = spc.run_noise_device(ctx, case)
        c = spc.check_nodes(case, precision, got)
        total.add(c)
        if case.seed == spc.SEARCHED_SEED:
            normal.add(c)
    ctx.close()
    print(f"{name} nodes: worst error / bound {total.worst:.3f} ({total.where}); searched counters and window {normal.worst:.3f}; "
          f"largest bound / range {total.worst_bound:.2e}; {total}")
    total.assert_shares(name, clamped=None)
    assert total.clamped >= 5 and total.interior >= 100, total


@pytest.mark.parametrize("ce", [False, True])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_batched_launch_draws_the_exact_nodes_and_follows_the_exact_spline(name, ce, monkeypatch):
    model, precision = FAMILIES[name][:2]
    n, rows = 64, BATCH_ROWS                       # (n_per_env is a multiple of 64: every wavefront serves one environment)
    envs = spc.batched_noise_cases(model, n, ce=ce, rows=rows)
    ctx = make_context(name, monkeypatch)
    _, start, mocap = fpc.setup(model)
    E = len(envs)
    ctx.set_states(np.tile(start, (E, 1)), [c.t0 for c in envs], None if mocap is None else np.tile(mocap, (E, 1)))
    knots, nominal = np.stack([c.node_times() for c in envs]), np.stack([c.nominal for c in envs])
    spec = envs[0].spec()
    if ce:
        ctx.rollout_noise_batched_ce(n, spc.H, 2, knots, nominal, np.stack([c.variance for c in envs]), spec)
    else:
        ctx.rollout_noise_batched(n, spc.H, 2, knots, nominal, spec)
    _, fail = ctx.returns()
    assert ctx.N == E * n and not fail.any(), ctx.failure_raw
    own_numbers(name, ctx)
    nodes_, acts = spc.Census(), spc.Census()
    first = []
    for e, case in enumerate(envs):
        got = np.zeros((n, case.P, ctx.nu))
        trs = []
        for c in rows:
            got[c] = ctx.fetch_spline(e * n + c)
            trs.append(ctx.fetch_trajectory(e * n + c))
        nodes_.add(spc.check_nodes(case, precision, got))
        actions, times = np.stack([t.actions for t in trs]), np.stack([t.times for t in trs])
        first.append(times[0])
        acts.add(spc.check_actions(case.name, model, precision, spc.Grid(knots[e], precision), 2, got[list(rows)], actions, times))
    assert not np.array_equal(first[0], first[1])       # (the environments ran on their own clocks)
    ctx.close()
    print(f"{name} batched{' ce' if ce else ''}: nodes worst error / bound {nodes_.worst:.3f} ({nodes_.where}), {nodes_}; "
          f"actions {acts.worst:.3f} ({acts.where}), {acts}")
    nodes_.assert_shares((name, "batched nodes"), clamped=None)
    acts.assert_shares((name, "batched actions"), {"before_first", "mean_slopes", "past_end"}, clamped=None)
