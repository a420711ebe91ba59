"""-m gpu: gradient_pass_kernel and gradient_pass_batched_kernel against rational arithmetic (tests/derivative_cases.py, section C).

   mjpcx_gradient_pass          Vx, k, dV[0], gradient <-> the sweep in Python integers and sum_t W_p(t) k[t], W the exact linear form of
                                TimeSpline::Sample; 4 x a running forward bound, itself capped at 1e-9; dV[1] == 0.0 and
                                k[T-1] == k[T-2] bit for bit
   mjpcx_gradient_step_batched  k, dV[0], gradient of every environment <-> the same reference fed with the call's own A, B, cx, cu
Neither tests/gradient_reference.py nor the oracle takes part. The worst error / bound of each family is printed."""
import numpy as np
import pytest

import derivative_cases as dc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    task = load_task("Particle")
    c = capi.Context(task.packed_model(differentiable=True), task.packed(), 0, 64)
    yield c
    c.close()


@pytest.mark.parametrize("T", dc.GRADIENT_T)
@pytest.mark.parametrize("shape", dc.GRADIENT_SHAPES, ids=lambda s: f"n{s[0]}m{s[1]}")
def test_gradient_pass_against_rational_arithmetic(ctx, shape, T):
    n, m = shape
    args, sweep = dc.gradient_sweep_case(n, m, T)
    cases = dc.gradient_cases(T)
    assert len(cases) == 3 * len(dc.GRADIENT_GRIDS)
    census, worst = dc.Census(), 0.0
    for name, rep, nodes, steps in cases:
        got = ctx.gradient_pass(*args, rep, nodes, steps)
        worst = max(worst, dc.check_gradient_pass(got, sweep, nodes, steps, rep))
        census += dc.gradient_census(n, m, T, nodes, steps)
    print(f"gradient pass n {n} m {m} T {T}: worst error / bound {worst:.3f} over {len(cases)} cases")
    # what this shape and horizon are here for
    census.require("on_knot", "grid_before_steps", "grid_after_steps", "past_last_node", "before_first_node", "single_node")
    if T >= 3:
        census.require("on_interior_knot", "unequal_spans")
    if T >= 65:
        census.require("full_stride")
    if T >= 130:
        census.require("second_stride")
    if shape == (10, 12):
        census.require("qu_in_row1", "qu_straddles_rows_0_1")
    if shape == (20, 16):
        census.require("qu_in_row1", "qu_straddles_rows_1_2")


def test_batched_gradient_pass_against_rational_arithmetic():
    """gradient_pass_batched_kernel through mjpcx_gradient_step_batched on the Particle: three environments, a grid each"""
    task = load_task("Particle")
    c = capi.Context(task.packed_model(differentiable=True), task.packed(), 0, 64)
    E, N, H, T = 3, 64, 12, 12
    states, times, mocap = dc.particle_fleet(E)
    c.set_states(states, times, mocap)
    rng = np.random.default_rng(5)
    roll_times = np.stack([t + np.linspace(0.0, (H - 1) * 0.1, 4) for t in times])
    c.rollout_splines_batched(H, capi.SPLINE_LINEAR, roll_times, np.clip(rng.normal(0, 0.3, (E, N, 4, 2)), -1, 1), num_envs=E, n_per_env=N)
    _, fail = c.returns()
    assert not fail.any()
    cand = 5
    step_times = np.stack([c.fetch_trajectory(e * N + cand).times[:T] for e in range(E)])
    nodes = dc.batched_grids(step_times)
    assert nodes.shape == (E, dc.BATCHED_NODES)
    census, worst = dc.Census(), 0.0
    for rep in (0, 1, 2):
        got = c.gradient_step_batched(E, cand, T, list(range(T)), 2.0 ** -20, 1, rep, nodes, with_matrices=True)
        for e in range(E):
            sweep = dc.exact_sweep(got["A"][e], got["B"][e], got["cx"][e], got["cu"][e])
            one = dict(k=got["k"][e], dV=got["dV"][e], gradient=got["gradient"][e])
            worst = max(worst, dc.check_gradient_pass(one, sweep, nodes[e], step_times[e], rep))
            census += dc.gradient_census(4, 2, T, nodes[e], step_times[e])
            assert np.abs(got["gradient"][e]).max() > 0
    print(f"batched gradient pass, Particle E {E} T {T}: worst error / bound {worst:.3f}")
    census.require("on_interior_knot", "unequal_spans", "grid_before_steps", "before_first_node", "past_last_node")
    c.close()
