"""The force-noise harness against itself and the oracle (CPU): tests/force_noise_cases.py.

- the oracle's NoisyRollout hands back the xfrc_applied it applied (orollout_noisy_xfrc): every entry of every row equals the exact series
  at the draw bound, on the probe, Cartpole, Particle, the A1 and the Humanoid; the last row repeats the one before;
- on the probe every step of the oracle obeys the closed forms (Euler and RK4, the three decays);
- on the registered models M (qacc_noisy - qacc_plain) of the oracle equals the exact generalized force on constraint-free states, and the
  oracle's own rollouts pass the checks the device is held to (which also asserts, from the reference alone, the conditions VISIBLE and
  RESOLUTION in both precisions);
- every named wrong reading misses at least one case by more than twice the bound the device is held to; the census of regimes is met.

draw_on_last_row is the one reading no recorded state can show: the last row takes no step, and no shipped residual reads a force. It is
held on the oracle's recorded series alone (row H - 1 must repeat row H - 2)."""
import numpy as np
import pytest

import force_noise_cases as fn

KEYS = ("probe", "cartpole", "particle", "a1", "humanoid")
CANDS = (0, 3)


def _noise_of(key, later=True):
    mdl = fn.model(key)
    return fn.pair_noise(mdl, "mid") if key == "probe" else fn.b_noise(mdl, later)


@pytest.mark.parametrize("key", KEYS)
def test_the_oracle_draws_the_exact_series(key):
    mdl = fn.model(key)
    noises = [fn.pair_noise(mdl, p) for p in fn.PAIRS] if key == "probe" else [_noise_of(key)]
    for nz in noises:
        _, _, _, xfrc = fn.oracle_rollouts(mdl, nz, fn.H_B + 1, 4, CANDS)
        for c in CANDS:
            got = xfrc[c].reshape(fn.H_B + 1, -1)
            worst = fn.check_series(nz, c, got, mdl.nbody, mdl.dt)
            assert np.array_equal(got[-1], got[-2]) and np.any(got[0] != 0), "nothing is drawn for the last row; the first step draws"
            print(f"{key} {nz}: candidate {c}, worst error / bound {worst:.3f}")


def test_the_header_and_the_kernels_count_the_models_bodies():
    """the census' body counts: 3 nbody of the probe exceeds a wavefront, the Humanoid's live bodies are fewer than its model's"""
    probe, hum = fn.model("probe"), fn.model("humanoid")
    assert probe.nbody == 27 and 3 * probe.nbody_live > 64 and probe.nv <= 32 and probe.nbody <= 64
    assert hum.nbody_live < hum.nbody
    assert probe.dt != probe.dt_xml and fn.model("cartpole").dt != fn.model("cartpole").dt_xml


@pytest.mark.parametrize("rk4", [False, True], ids=["euler", "rk4"])
@pytest.mark.parametrize("pair", list(fn.PAIRS))
def test_the_oracle_obeys_the_closed_forms_on_the_probe(pair, rk4):
    mdl = fn.model("probe")
    nz = fn.pair_noise(mdl, pair)
    saved = mdl.pm.struct.integrator
    mdl.pm.struct.integrator = 1 if rk4 else 0
    try:
        states, _, actions, _ = fn.oracle_rollouts(mdl, nz, fn.H_A, fn.N_WAVE, range(fn.N_WAVE))
    finally:
        mdl.pm.struct.integrator = saved
    for precision in (64, 32):     # (32: the oracle's doubles under the float bounds -- what is asserted is RESOLUTION, from the reference alone)
        rep = fn.check_probe(mdl, nz, precision, rk4, states, actions, range(fn.N_WAVE))
        print(f"probe {pair} rk4={rk4} fp{precision}: {rep.compared} entries, worst error / bound {rep.worst:.3g}, bound / resolution {rep.tightest:.3g}")
        assert not rep.misses, sorted(rep.misses, reverse=True)[:4]
    assert rep.compared == fn.N_WAVE * (fn.H_A - 1) * (22 if rk4 else 30)


@pytest.mark.parametrize("key", KEYS)
def test_the_oracle_applies_the_exact_generalized_force(key):
    """M (qacc_noisy - qacc_plain) = Q. Bound: Q's own gamma_n on its absolute terms, n = 11 + nbody (one body's term and one sum per
    further body) + 30 for the frames it reads, and the two solves: each computed qacc solves (M + dM) qacc = F with |dM| <=
    gamma_(3 nv + 1) |L| |L^T| (Higham Th. 10.4), so M qacc is off by that times |qacc|; HEADROOM times the sum."""
    mdl = fn.model(key)
    nz = _noise_of(key, later=False)
    orc = fn.oracle_of(mdl)
    ctrl = fn.controls(mdl, 1)[0, 0]
    Mo, nefc = orc.at(mdl.state, mdl.time, ctrl)
    assert nefc == 0
    Ms = fn.effective_mass(mdl, Mo) - mdl.dt * np.diag(mdl.damping())
    L = np.linalg.cholesky(Ms)
    LL = np.abs(L) @ np.abs(L.T)
    a0 = orc.acceleration(mdl.state, mdl.time, ctrl, np.zeros((mdl.nbody, 6)))
    A = fn.force_map(mdl, mdl.state[:mdl.nq])
    worst = 0.0
    for c in CANDS:
        xs, _ = fn.series(nz, c, 2, mdl.nbody, mdl.dt, 64)
        a1 = orc.acceleration(mdl.state, mdl.time, ctrl, np.array([float(v) for v in xs[0]]).reshape(-1, 6))
        Q, Qabs = fn.generalized_force(A, xs[0])
        got = Ms @ (a1 - a0)
        bound = fn.SLACK * (float(fn.gamma(41 + mdl.nbody, fn.U64)) * np.array([float(v) for v in Qabs])
                            + float(fn.gamma(3 * mdl.nv + 1, fn.U64)) * (LL @ (np.abs(a0) + np.abs(a1))) + fn.U64 * np.abs(Ms) @ (np.abs(a0) + np.abs(a1)))
        err = np.abs(got - np.array([float(v) for v in Q]))
        assert np.all(err <= bound), (key, c, float((err / bound).max()))
        assert np.abs(got).max() > 1e6 * bound.max(), "the force is visible far above the bound"
        worst = max(worst, float((err / bound).max()))
    print(f"{key}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("key", KEYS[1:])
def test_the_oracle_passes_method_b(key):
    """the checks of tests/test_gpu_force_noise.py on the oracle's own rollouts; VISIBLE is asserted here from the reference alone, in both
    precisions (the lane rows also for t >= 1 at the float step tolerance)"""
    mdl = fn.model(key)
    orc = fn.oracle_of(mdl)
    nodes = fn.controls(mdl, fn.N_WAVE)
    first = fn.b_noise(mdl, later=False)
    s1, _, _, _ = fn.oracle_rollouts(mdl, first, 2, fn.N_WAVE, CANDS)
    v_plain = np.stack([orc.plain_step(mdl.state, mdl.time, nodes[c, 0]) for c in range(fn.N_WAVE)])
    for precision in (64, 32):
        rep = fn.check_b_first(mdl, first, precision, mdl.state, mdl.time, nodes[:, 0], v_plain, s1[:, 1, mdl.nq:], CANDS)
        print(f"{key} t = 0 fp{precision}: worst error / bound {rep.worst:.3g}, bound / (5 % of Delta) {rep.tightest:.3g}")
        assert not rep.misses, sorted(rep.misses, reverse=True)[:4]
    later = fn.b_noise(mdl, later=True)
    st, tm, ac, _ = fn.oracle_rollouts(mdl, later, fn.H_B, fn.N_WAVE, CANDS)
    for precision in ((64, 32) if key in ("cartpole", "particle") else (64,)):
        rep = fn.check_b_later(mdl, later, precision, st, tm, ac, CANDS)
        print(f"{key} t >= 1 fp{precision}: worst error / tolerance {rep.worst:.3g}, tolerance / (5 % of Delta) {rep.tightest:.3g}")
        assert not rep.misses, sorted(rep.misses, reverse=True)[:4]


# ------------------------------------------------------------------------------------------------ the wrong readings
def _gap_probe(mutation, pair="fast", rk4=False, precision=32, env=0):
    """max |mutated - exact| / bound over the compared entries of the probe's steps, on the oracle's states of the true reading"""
    mdl = fn.model("probe")
    nz = fn.pair_noise(mdl, pair, env)
    states, _, actions, _ = fn.oracle_rollouts(mdl, nz, 4, fn.N_WAVE, (1,))
    true = fn.probe_expect(mdl, nz, precision, rk4, states, actions, (1,))
    wrong = fn.probe_expect(mdl, nz, precision, rk4, states, actions, (1,), mutation)
    return max(float(np.max(np.abs(wrong[k].want - true[k].want)[true[k].mask] / true[k].bound[true[k].mask])) for k in true)


def _gap_b(mutation, key, later, precision, env=0):
    mdl = fn.model(key)
    nz = fn.b_noise(mdl, later, env)
    H = fn.H_B if later else 2
    st, tm, ac, _ = fn.oracle_rollouts(mdl, nz, H, fn.N_WAVE, (1,))
    worst = 0.0
    for t in range(1 if later else 0, H - 1):
        d0, b0, _ = fn.b_expect(mdl, nz, precision, 1, t, H, st[1, t], tm[1, t], ac[1, t])
        d1, _, _ = fn.b_expect(mdl, nz, precision, 1, t, H, st[1, t], tm[1, t], ac[1, t], mutation)
        v = np.abs(st[1, t + 1, mdl.nq:])
        bound = fn.STEP_TOL[precision] * (1 + v) if later else b0 + fn.SLACK * 4 * fn.U(precision) * v
        worst = max(worst, float(np.max(np.abs(d1 - d0) / bound)))
    return worst


def _gap_last_row(mutation):
    mdl = fn.model("probe")
    nz = fn.pair_noise(mdl, "fast")
    x0, e0 = fn.series(nz, 1, 4, mdl.nbody, mdl.dt, 64)
    x1, _ = fn.series(nz, 1, 4, mdl.nbody, mdl.dt, 64, mutation, mdl.nbody_live, mdl.dt_xml)
    return max(float(abs(a - b) / (fn.SLACK * e)) for a, b, e in zip(x0[-1], x1[-1], e0[-1]) if e > 0)


CASES = {    # name: the gap of a wrong reading on it (the float bound wherever the row has one)
    "probe-fast-euler-fp32": lambda m: _gap_probe(m),
    "probe-slow-rk4-fp32": lambda m: _gap_probe(m, "slow", True),
    "probe-batched-env2-fp32": lambda m: _gap_probe(m, "mid", False, 32, 2),
    "cartpole-t0-fp32": lambda m: _gap_b(m, "cartpole", False, 32),
    "cartpole-batched-env1-t0-fp32": lambda m: _gap_b(m, "cartpole", False, 32, 1),
    "particle-later-fp32": lambda m: _gap_b(m, "particle", True, 32),
    "a1-t0-fp32": lambda m: _gap_b(m, "a1", False, 32),
    "humanoid-later-fp64": lambda m: _gap_b(m, "humanoid", True, 64),
    "oracle-series-last-row": _gap_last_row,
}
# reading: the cases that must each miss it by more than twice their bound
MUST_MISS = {
    "stride_live_bodies": ("probe-fast-euler-fp32", "humanoid-later-fp64"),
    "z_swapped": ("probe-fast-euler-fp32", "cartpole-t0-fp32", "a1-t0-fp32"),
    "torque_before_force": ("probe-fast-euler-fp32", "a1-t0-fp32"),
    "stream_word_zero": ("probe-fast-euler-fp32", "cartpole-t0-fp32"),
    "decay_outside": ("probe-fast-euler-fp32", "cartpole-t0-fp32"),      # (at decay 0.9999 it is 1e-4 of the draw: two bounds in float)
    "scale_without_root": ("probe-fast-euler-fp32", "probe-slow-rk4-fp32", "a1-t0-fp32"),
    "scale_root_of_one_minus_decay": ("probe-fast-euler-fp32", "probe-slow-rk4-fp32", "a1-t0-fp32"),
    "draw_on_last_row": ("oracle-series-last-row",),
    "no_draw_at_first_step": ("probe-fast-euler-fp32", "cartpole-t0-fp32"),
    "offset_ignored": ("probe-fast-euler-fp32", "cartpole-t0-fp32", "humanoid-later-fp64"),
    "env_seed_ignored": ("probe-batched-env2-fp32", "cartpole-batched-env1-t0-fp32"),
    "xml_timestep": ("probe-fast-euler-fp32", "cartpole-t0-fp32", "particle-later-fp32"),
    "at_body_origin": ("probe-fast-euler-fp32", "a1-t0-fp32"),
    "torque_in_body_frame": ("probe-fast-euler-fp32", "a1-t0-fp32"),
    "no_ancestors": ("probe-fast-euler-fp32", "a1-t0-fp32", "humanoid-later-fp64"),
}


def test_every_reading_is_listed():
    assert set(MUST_MISS) == set(fn.MUTATIONS) and len(fn.MUTATIONS) == 15


@pytest.mark.parametrize("mutation", fn.MUTATIONS)
def test_every_wrong_reading_misses_a_case(mutation):
    for case in MUST_MISS[mutation]:
        gap = CASES[case](mutation)
        print(f"{mutation} on {case}: off by {gap:.3g} bounds")
        assert gap > 2.0, (mutation, case, gap)


def test_the_true_reading_misses_none():
    for case, gap in CASES.items():
        assert gap(None) == 0.0, case


def test_the_census_of_regimes():
    met = set()
    probe = fn.model("probe")
    for pair in fn.PAIRS:
        nz = fn.pair_noise(probe, pair, env=1)
        states, _, actions, _ = fn.oracle_rollouts(probe, nz, 3, fn.N_WAVE, (0,))
        met |= fn.check_probe(probe, nz, 64, False, states, actions, (0,)).regimes
    for key in KEYS[1:]:
        met |= fn.noise_regimes(fn.model(key), fn.b_noise(fn.model(key), True))
    assert set(fn.REGIMES) <= met, sorted(set(fn.REGIMES) - met)
    assert "live_ne_model" in fn.noise_regimes(fn.model("humanoid"), fn.b_noise(fn.model("humanoid"), True))
    assert "stride_wrapped" in fn.noise_regimes(probe, fn.pair_noise(probe, "fast"))
