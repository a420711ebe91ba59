"""-m gpu: the Ornstein-Uhlenbeck force noise of mjpcx_rollout_splines_noisy (and its batched form) against exact answers on every kernel
that draws it -- tests/force_noise_cases.py has the method, the bounds and the conditions; nothing here goes through the oracle's
NoisyRollout. One context per row, closed in `finally`; every row asserts the kernel it ran on.

  Method A  tests/models/xfrc_probe.xml on rollout_wave_kernel (Euler and RK4, fp64 and fp32), N = 5, H = 6, the three decays (e^-1,
            0.980, 0.9999): for every candidate and every t < H - 1 the recorded qvel[t + 1] is the closed-form image of the RECORDED
            state t under the exact force series. 3 nbody = 81 pairs a step wrap the 64 lanes; agent_timestep differs from the XML's.
  Method B  rollout_lane (Cartpole, Particle; N = 70 crosses a 64-lane block; candidates 0, 1, 31, 63, 64, 69 are compared),
            rollout_tree_kernel<A1> (MJPCX_NO_QUAD, friction loss and contacts disabled) and rollout_tree_kernel<Humanoid>
            (MJPCX_NO_LIMB), N = 5, on airborne mid-range states where the oracle reports nefc = 0:
              t = 0   both precisions: a plain and a noisy launch (H = 2) of the same state and splines on one context;
                      qvel_noisy[1] - qvel_plain[1] = dt (M + dt D)^-1 Q within kappa gamma_n |Delta|_inf + 2 u |qvel|
              t >= 1  fp64 rows, and the lane rows in fp32: qvel[t + 1] minus the oracle's PLAIN step from the recorded state t equals
                      the same expression within the step-parity tolerance of the row (1e-9, lanes in fp32 1e-4, times 1 + |x|).
                      The float tree rows stop at t = 0: their recursion is the source line of wave_rollout_body Method A covers in float.
  Batched   rollout_splines_noisy_batched, E = 3, n_per_env = 64, on the probe (Method A, candidates 0 and 63 of every environment) and
            on Cartpole (Method B at t = 0): environment e follows the exact series of seed + e with the local offset.
candidate_offset = 7 and the seed has a non-zero high word throughout. RESOLUTION (A: bound <= 1e-3 of dt scale |dv/df|) and VISIBLE (B:
bound <= 5 % of |Delta|_inf) are asserted on every compared entry, nefc = 0 on every state used.

NEGATIVE CONTROL (test_a_shifted_offset_fails): the device is given candidate_offset + 1, the reference keeps candidate_offset; every
row must then miss.

Worst error / bound (B at t >= 1: / tolerance), measured on the MI355X:

    row                                     fp64        fp32
    A  rollout_wave_kernel, Euler, e^-1     0.057       0.034
    A  rollout_wave_kernel, Euler, 0.980    0.027       0.057
    A  rollout_wave_kernel, Euler, 0.9999   0.0015      0.046
    A  rollout_wave_kernel, RK4, e^-1       0.044       0.034
    A  rollout_wave_kernel, RK4, 0.980      0.027       0.054
    A  rollout_wave_kernel, RK4, 0.9999     0.0015      0.046
    B  rollout_lane Cartpole, t = 0         0.0058      0.0058
    B  rollout_lane Cartpole, t >= 1        2.4e-7      0.0014
    B  rollout_lane Particle, t = 0         0.037       0.013
    B  rollout_lane Particle, t >= 1        1.4e-7      1.8e-4
    B  rollout_tree_kernel<A1>, t = 0       6.7e-4      0.0017
    B  rollout_tree_kernel<A1>, t >= 1      5.3e-7      --
    B  rollout_tree_kernel<Humanoid>, t = 0 1.0e-4      5.9e-5
    B  rollout_tree_kernel<Humanoid>, t >= 1 6.9e-6     --
    batched probe (worst environment)       0.038       0.079
    batched Cartpole (worst environment)    0.0080      0.0068

With the offset shifted by one the same rows are off by 6e13 / 2e5 (A), 1e13 / 8e4 (Cartpole), 1e14 / 6e5 (Particle), 3e12 / 7e3 (A1) and
3e10 / 59 (Humanoid) bounds. The largest bound against its condition: RESOLUTION 0.68 (fp32, decay 0.9999), VISIBLE 0.71 (Humanoid fp32:
kappa = 1.0e3, n = 146). The module takes 22 s of the -m gpu suite, the mpmath reference most of it.
"""
import os

import numpy as np
import pytest

import feedback_policy_cases as fpc
import force_noise_cases as fn
from mujoco_mpc_amd import capi

pytestmark = pytest.mark.gpu

A_ROWS = {"wave-euler-fp64": (64, False), "wave-euler-fp32": (32, False), "wave-rk4-fp64": (64, True), "wave-rk4-fp32": (32, True)}
B_ROWS = {
    "lane-cartpole-fp64": ("cartpole", {}, "rollout_lane", 64),
    "lane-cartpole-fp32": ("cartpole", {}, "rollout_lane", 32),
    "lane-particle-fp64": ("particle", {}, "rollout_lane", 64),
    "lane-particle-fp32": ("particle", {}, "rollout_lane", 32),
    "tree-a1-fp64": ("a1", {"MJPCX_NO_QUAD": "1"}, "rollout_tree_kernel<A1>", 64),
    "tree-a1-fp32": ("a1", {"MJPCX_NO_QUAD": "1"}, "rollout_tree_kernel<A1>", 32),
    "tree-humanoid-fp64": ("humanoid", {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>", 64),
    "tree-humanoid-fp32": ("humanoid", {"MJPCX_NO_LIMB": "1"}, "rollout_tree_kernel<Humanoid>", 32),
}
LANE_COMPARED = (0, 1, 31, 63, 64, 69)
BATCH_COMPARED = (0, 63)


def context(pm, pt, precision, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.Context(pm, pt, 0, precision)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def noisy(ctx, mdl, nz, H, nodes, skew):
    ctx.set_state(mdl.state, mdl.time, mdl.mocap)
    ctx.rollout_splines_noisy(H, 0, np.array([mdl.time]), nodes, nz.std, nz.rate, seed=nz.seed, candidate_offset=nz.offset + skew)
    return fpc.fetch_all(ctx)


def run_a(row, pairs=tuple(fn.PAIRS), skew=0):
    precision, rk4 = A_ROWS[row]
    mdl = fn.model("probe")
    pm = mdl.task.packed_model()
    pm.struct.integrator = 1 if rk4 else 0
    ctx = context(pm, mdl.pt, precision, {})
    rep = fn.Report()
    try:
        assert ctx.kernel_name.startswith("rollout_wave_kernel"), ctx.kernel_name
        for pair in pairs:
            nz = fn.pair_noise(mdl, pair)
            states, actions, _ = noisy(ctx, mdl, nz, fn.H_A, fn.controls(mdl, fn.N_WAVE), skew)
            one = fn.check_probe(mdl, nz, precision, rk4, states, actions, range(fn.N_WAVE))
            print(f"{row} {pair}: {one.compared} entries, worst error / bound {one.worst:.3g}, bound / resolution {one.tightest:.3g}")
            rep.add(one)
        assert ctx.kernel_name.startswith("rollout_wave_kernel"), ctx.kernel_name
    finally:
        ctx.close()
    return rep


def run_b(row, later=True, skew=0):
    key, env, kernel, precision = B_ROWS[row]
    mdl = fn.model(key)
    lane = kernel == "rollout_lane"
    N = fn.N_LANE if lane else fn.N_WAVE
    cands = LANE_COMPARED if lane else range(N)
    nodes = fn.controls(mdl, N)
    ctx = context(mdl.pm, mdl.pt, precision, env)
    first, rest = fn.Report(), fn.Report()
    try:
        assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
        ctx.set_state(mdl.state, mdl.time, mdl.mocap)
        ctx.rollout_splines(2, 0, np.array([mdl.time]), nodes)
        plain, actions, times = fpc.fetch_all(ctx)
        assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
        nz = fn.b_noise(mdl, later=False)
        states, _, _ = noisy(ctx, mdl, nz, 2, nodes, skew)
        assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
        assert np.array_equal(states[:, 0], plain[:, 0])
        first = fn.check_b_first(mdl, nz, precision, plain[0, 0], times[0, 0], actions[:, 0], plain[:, 1, mdl.nq:], states[:, 1, mdl.nq:], cands)
        print(f"{row} t = 0: {first.compared} entries, worst error / bound {first.worst:.3g}, bound / (5 % of Delta) {first.tightest:.3g}")
        if later and (precision == 64 or lane):
            nz = fn.b_noise(mdl, later=True)
            states, actions, times = noisy(ctx, mdl, nz, fn.H_B, nodes, skew)
            assert ctx.kernel_name.startswith(kernel), ctx.kernel_name
            rest = fn.check_b_later(mdl, nz, precision, states, times, actions, cands)
            print(f"{row} t >= 1: {rest.compared} entries, worst error / tolerance {rest.worst:.3g}, tolerance / (5 % of Delta) {rest.tightest:.3g}")
    finally:
        ctx.close()
    return first, rest


@pytest.mark.parametrize("row", list(A_ROWS))
def test_the_probe_obeys_the_closed_forms(row):
    rep = run_a(row)
    assert not rep.misses, sorted(rep.misses, reverse=True)[:4]
    assert rep.compared == 3 * fn.N_WAVE * (fn.H_A - 1) * (22 if A_ROWS[row][1] else 30)
    assert {"stride_wrapped", "decay>0.999", "decay<0.5", "offset_ne_0", "seed_high_word"} <= rep.regimes
    if not A_ROWS[row][1]:         # (RK4 compares neither the chain nor the damped hinges)
        assert {"damped_hinge", "child_to_ancestor"} <= rep.regimes


@pytest.mark.parametrize("row", list(B_ROWS))
def test_the_registered_kernels_apply_the_exact_force(row):
    first, rest = run_b(row)
    assert not first.misses, sorted(first.misses, reverse=True)[:4]
    assert not rest.misses, sorted(rest.misses, reverse=True)[:4]
    assert first.compared > 0 and (rest.compared > 0) == (B_ROWS[row][3] == 64 or B_ROWS[row][2] == "rollout_lane")


@pytest.mark.parametrize("row", list(A_ROWS) + list(B_ROWS))
def test_a_shifted_offset_fails(row):
    """the device draws the stream of candidate_offset + 1, the reference keeps candidate_offset: the row must miss"""
    rep = run_a(row, pairs=("fast",), skew=1) if row in A_ROWS else run_b(row, later=False, skew=1)[0]
    assert rep.misses and rep.worst > 2.0, (row, rep.worst)


@pytest.mark.parametrize("precision", [64, 32])
def test_batched_probe(precision):
    """environment e of rollout_splines_noisy_batched follows the exact series of seed + e with the local offset (Method A)"""
    mdl = fn.model("probe")
    nz0 = fn.pair_noise(mdl, "mid")
    E, n = fn.E_BATCH, fn.N_BATCH
    starts = np.stack([np.concatenate([mdl.state[:mdl.nq], (1 - 0.25 * e) * mdl.state[mdl.nq:]]) for e in range(E)])
    times = mdl.time + 0.5 * np.arange(E)
    nodes = np.full((E, n, 1, 1), fn.ACTION)
    ctx = context(mdl.pm, mdl.pt, precision, {})
    try:
        assert ctx.kernel_name.startswith("rollout_wave_kernel"), ctx.kernel_name
        ctx.set_states(starts, times, np.tile(mdl.mocap, (E, 1)))
        ctx.rollout_splines_noisy_batched(fn.H_B, 0, times[:, None], nodes, nz0.std, nz0.rate, seed=nz0.seed, candidate_offset=nz0.offset,
                                          num_envs=E, n_per_env=n)
        states, actions, _ = fpc.fetch_all(ctx)
        assert ctx.kernel_name.startswith("rollout_wave_kernel"), ctx.kernel_name
    finally:
        ctx.close()
    for e in range(E):
        assert np.array_equal(states[e * n, 0], fpc.rounded(starts[e], precision))
        rep = fn.check_probe(mdl, fn.pair_noise(mdl, "mid", env=e), precision, False, states[e * n:(e + 1) * n], actions[e * n:(e + 1) * n], BATCH_COMPARED)
        print(f"batched probe fp{precision} environment {e}: {rep.compared} entries, worst error / bound {rep.worst:.3g}")
        assert not rep.misses, sorted(rep.misses, reverse=True)[:4]
        assert rep.compared == len(BATCH_COMPARED) * (fn.H_B - 1) * 30


@pytest.mark.parametrize("precision", [64, 32])
def test_batched_cartpole(precision):
    """the same on the lane kernel's batched NOISY form (Method B at t = 0: a plain and a noisy batched launch of the same splines)"""
    mdl = fn.model("cartpole")
    nz0 = fn.b_noise(mdl, later=False)
    E, n = fn.E_BATCH, fn.N_BATCH
    starts = np.stack([mdl.state * (1 - 0.25 * e) for e in range(E)])
    times = mdl.time + 0.5 * np.arange(E)
    nodes = np.stack([fn.controls(mdl, n, seed=5 + e) for e in range(E)])
    ctx = context(mdl.pm, mdl.pt, precision, {})
    try:
        assert ctx.kernel_name.startswith("rollout_lane"), ctx.kernel_name
        ctx.set_states(starts, times)
        ctx.rollout_splines_batched(2, 0, times[:, None], nodes, num_envs=E, n_per_env=n)
        plain, actions, tms = fpc.fetch_all(ctx)
        ctx.rollout_splines_noisy_batched(2, 0, times[:, None], nodes, nz0.std, nz0.rate, seed=nz0.seed, candidate_offset=nz0.offset, num_envs=E, n_per_env=n)
        states, _, _ = fpc.fetch_all(ctx)
        assert ctx.kernel_name.startswith("rollout_lane"), ctx.kernel_name
    finally:
        ctx.close()
    nq = mdl.nq
    for e in range(E):
        sl = slice(e * n, (e + 1) * n)
        rep = fn.check_b_first(mdl, fn.b_noise(mdl, False, env=e), precision, plain[e * n, 0], tms[e * n, 0], actions[sl, 0], plain[sl, 1, nq:],
                               states[sl, 1, nq:], BATCH_COMPARED)
        print(f"batched cartpole fp{precision} environment {e}: worst error / bound {rep.worst:.3g}")
        assert not rep.misses, sorted(rep.misses, reverse=True)[:4]
