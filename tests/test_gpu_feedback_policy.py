"""-m gpu: every device copy of the iLQG feedback policy held to the exact policy BETWEEN the knots of the nominal
(tests/feedback_policy_cases.py: the mpmath reference, the cases, the derived bounds, the comparison rule).

Every case runs through Context.rollout_feedback; fetch_trajectory of every candidate gives the states and times the policy was asked at
and the actions it gave, and the checker recomputes the policy from those. The kernel that ran is asserted each time.
   lane family          Cartpole (nu = 1) and Particle (nu = 2, mocap), fp64 and fp32; 70 candidates (a full wavefront and a ragged one)
   generic wave kernel  tests/models/capsules_tendon.xml (five free joints, two hinges, nu = 1); the A1 under MJPCX_NO_LDS_MODEL=1
   registered tree      the A1 under MJPCX_NO_QUAD_FEEDBACK=1; the Humanoid (Walk's first keyframe): one cubic G2 case, one mode-0 case
   quad form            the A1 by default, with quad_stats()["handed_on"] == 0: the numbers are the quad form's
   batched              one rollout_feedback_batched call per family, E = 2 environments x 3 candidates, each environment its own knots
                        (G2, and G2 moved by 0.37 steps), clock and start state; the same checker on the environment-major candidates
A family's cases are split into four groups (the grids G1, G2, G3 + G4, and the rest: use_state 0, the two mode-0 cases, the zero-quaternion case G5) so that a test stays
at a few seconds; each group asserts its census and the interpolation regimes its grids must meet. The worst error / bound is printed."""
import numpy as np
import pytest

import feedback_policy_cases as fpc
from mujoco_mpc_amd import capi

pytestmark = pytest.mark.gpu

GROUPS = {
    "G1": (lambda c: c.mode == 1 and c.use_state and c.grid == "G1",
           {"before_first", "left_slope", "mean_slopes", "action_grid_last", "state_grid_last", "past_end"}),
    "G2": (lambda c: c.mode == 1 and c.grid == "G2", {"on_knot", "mean_slopes", "action_grid_last", "state_grid_last"}),
    "G3+G4": (lambda c: c.mode == 1 and c.grid in ("G3", "G4"), {"action_grid_last", "state_grid_last", "past_end"}),
    "rest": (lambda c: c.mode == 0 or not c.use_state or c.grid == "G5", set()),
}
# family: (model, precision, environment, what the context's kernel name must hold)
FAMILIES = {
    "cartpole64": ("cartpole", 64, {}, "rollout_lane"),
    "cartpole32": ("cartpole", 32, {}, "rollout_lane"),
    "particle64": ("particle", 64, {}, "rollout_lane"),
    "particle32": ("particle", 32, {}, "rollout_lane"),
    "scene": ("scene", 64, {}, "rollout_wave_kernel"),
    "a1_generic": ("a1", 64, {"MJPCX_NO_LDS_MODEL": "1"}, "rollout_wave_kernel"),
    "a1_tree": ("a1", 64, {"MJPCX_NO_QUAD_FEEDBACK": "1"}, "rollout_quad_kernel"),   # (the context of a registered A1; its feedback rollouts stay on the tree kernel)
    "a1_quad": ("a1", 64, {}, "rollout_quad_kernel"),
}


def make_context(name, monkeypatch, model=None, precision=64, env=None, kernel=None):
    if name is not None:
        model, precision, env, kernel = FAMILIES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pm, pt = fpc.packed(model)
    ctx = capi.Context(pm, pt, 0, precision)
    assert kernel in ctx.kernel_name, ctx.kernel_name
    return ctx


def quad_form_only(name, ctx):
    if name == "a1_quad":
        assert ctx.quad_stats()["handed_on"] == 0


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_kernel_follows_the_exact_policy(name, group, monkeypatch):
    model, precision = FAMILIES[name][:2]
    ctx = make_context(name, monkeypatch)
    pick, regimes = GROUPS[group]
    total = fpc.Census()
    for case in filter(pick, fpc.family(model)):
        got = fpc.run_device(ctx, case)
        quad_form_only(name, ctx)
        total.add(fpc.check(case, precision, *got))
    ctx.close()
    print(f"{name} {group}: worst error / bound {total.worst:.3f} ({total.where}); largest bound {total.worst_bound:.2e}; {total}")
    total.assert_shares((name, group), regimes)


def test_the_humanoid_tree_kernel_follows_the_exact_policy(monkeypatch):
    ctx = make_context(None, monkeypatch, "humanoid", 64, {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>")
    total = fpc.Census()
    for case in fpc.humanoid_cases():
        total.add(fpc.check(case, 64, *fpc.run_device(ctx, case)))
    ctx.close()
    print(f"humanoid: worst error / bound {total.worst:.3f} ({total.where}); largest bound {total.worst_bound:.2e}; {total}")
    assert total.ambiguous <= 0.05 * total.total and total.interior >= 0.3 * total.total and total.clamped >= 0.1 * total.total, total


@pytest.mark.parametrize("name", ["cartpole64", "particle32", "scene", "a1_generic", "a1_tree", "a1_quad"])
def test_the_batched_launch_follows_the_exact_policy(name, monkeypatch):
    model, precision = FAMILIES[name][:2]
    ctx = make_context(name, monkeypatch)
    envs = fpc.batched_pair(model)
    n = len(envs[0].alpha)
    ctx.set_states(np.stack([c.start for c in envs]), [c.t0 for c in envs], None if envs[0].mocap is None else np.stack([c.mocap for c in envs]))
    a = envs[0]
    ctx.rollout_feedback_batched(a.H, a.mode, a.representation, a.use_state, *[np.stack(x) for x in zip(*[c.policy_args() for c in envs])])
    quad_form_only(name, ctx)
    states, actions, times = fpc.fetch_all(ctx)
    assert len(times) == 2 * n
    total = fpc.Census()
    for e, case in enumerate(envs):
        rows = slice(e * n, (e + 1) * n)
        total.add(fpc.check(case, precision, states[rows], actions[rows], times[rows]))
    ctx.close()
    assert not np.array_equal(times[0], times[n])      # (the environments ran on their own clocks)
    print(f"{name} batched: worst error / bound {total.worst:.3f} ({total.where}); largest bound {total.worst_bound:.2e}; {total}")
    assert {"on_knot", "mean_slopes", "action_grid_last", "state_grid_last"} <= total.regimes
