"""CPU tests of the sampling-policy harness (tests/sampling_policy_cases.py): the exact candidate nodes and the exact spline policy against
   the oracle (oracle/rng.c, oracle/spline.c through its rollouts)   held to a QUARTER of the bound
   the quad and limb kernels' step functions                         quad_step.h / limb_step.h through their lock-step emulators, no
                                                                     candidate handed on; the limb copy in float as well
   the Python TimeSpline                                             mujoco_mpc_amd/spline.py, at the oracle's step times
and the conditions on the cases themselves: Philox against the Random123 vectors, the property of every searched counter recomputed in
integers, the caps on the bounds, and the reference-only census (ambiguous share, clamped share, regimes) of every group at both
precisions. The worst error / bound of each is printed. The -m gpu suite (tests/test_gpu_sampling_policy.py) runs the same cases and the
same checkers on the device kernels."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import feedback_policy_cases as fpc
import sampling_policy_cases as spc
from test_rng import KAT

MODELS = ["cartpole", "particle", "a1", "scene", "humanoid"]
N_OF = {"cartpole": 70, "particle": 70}


def uniforms(seed, candidate, c, iteration, stream):
    k1, k2 = spc.uniform_k(seed, candidate, c, iteration, stream)
    return Fraction(2 * k1 + 1, 2 * spc.TWO53), Fraction(2 * k2 + 1, 2 * spc.TWO53)


def test_philox_in_integers_gives_the_known_answers():
    for ctr, key, out in KAT:
        assert spc.philox(ctr, key) == out


def test_every_searched_counter_has_its_property():
    for name, gi in spc.SEARCHED.items():
        assert gi > 1 << 20
        u1, u2 = uniforms(spc.SEARCHED_SEED, gi, 0, spc.SEARCHED_ITERATION, 0)
        assert spc.PROPERTY[name](u1, u2), (name, float(u1), float(u2))
    z, _ = spc.normal_pair(*spc.uniform_k(spc.SEARCHED_SEED, spc.SEARCHED["u1_small"], 0, spc.SEARCHED_ITERATION, 0))
    assert max(abs(z[0]), abs(z[1])) > 5 * 2 ** -0.5 and z[0] ** 2 + z[1] ** 2 > 25      # r > 5
    w = spc.BERNOULLI_WINDOW
    u, _ = uniforms(w["seed"], w["candidate"], 0, w["iteration"], 1)
    assert Fraction(0.2) <= u < Fraction(float(np.float32(0.2)))
    assert not spc.takes_std1(w["seed"], w["candidate"], w["iteration"])
    assert spc.SEARCHED_SEED >> 32 and w["seed"] >> 32


def test_the_oracle_normal_is_the_exact_one():
    """ogaussian_pair against mpmath, at a quarter of the bound (the worst case with 4-ulp functions; glibc's are within 1)"""
    from oracle import pyoracle
    z = np.zeros(2)
    counters = [(spc.SEARCHED_SEED, gi, 0, spc.SEARCHED_ITERATION) for gi in spc.SEARCHED.values()]
    counters += [(12345 + (s << 32), c, p, 7) for s in (0, 9) for c in range(40) for p in range(5)]
    worst = 0.0
    for seed, cand, pair, it in counters:
        pyoracle.lib().ogaussian_pair(C.c_uint64(seed), cand, pair, it, z.ctypes.data_as(C.POINTER(C.c_double)))
        want, e = spc.normal_pair(*spc.uniform_k(seed, cand, pair, it, 0))
        for i in range(2):
            worst = max(worst, float(abs(z[i] - want[i]) / e[i]))
    print(f"oracle normal: worst error / worst-case bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("model", MODELS)
def test_the_oracle_draws_the_exact_nodes(model):
    from oracle import pyoracle
    pm, _ = fpc.packed(model)
    total = spc.Census()
    N = N_OF.get(model, 8)
    cases = spc.noise_cases(model, N) + spc.searched_cases(model) + [spc.bernoulli_case(model)]
    cases += spc.batched_noise_cases(model, 4) + spc.batched_noise_cases(model, 4, ce=True)
    for case in cases:
        got = pyoracle.noise_candidates(pm, case.spec(), case.P, case.nominal, range(case.candidate_offset, case.candidate_offset + case.N))
        total.add(spc.check_nodes(case, 64, got, scale=0.25))
        spc.check_nodes(case, 32, None)                       # the caps of the fp32 bounds
    print(f"oracle nodes {model}: worst error / bound {0.25 * total.worst:.3f} ({total.where}); largest bound / range {total.worst_bound:.2e}; {total}")
    total.assert_shares(model, clamped=None)
    assert total.clamped >= 5 and total.interior >= 100, total


def test_the_noise_cases_meet_what_they_are_for():
    """the reference alone: both std of the mixture are drawn, the nominal candidate is met in the middle, the variance sits above, below and
    on zero, the Bernoulli-window candidate takes std0 and nothing of the searched cases clamps"""
    cases = spc.noise_cases("cartpole", 70)
    assert cases[0].P * 1 % 2 == 1                             # odd P nu: the last pair is half used
    _, _, took = cases[1].reference(64)
    assert 0 < took.sum() < 70
    want, bound, _ = cases[2].reference(64)
    assert np.array_equal(want[35], fpc.rounded(cases[2].nominal, 64)) and not bound[35].any() and cases[2].candidate_offset > 1 << 20
    v = cases[3].variance
    assert (v == 0).any() and (np.sqrt(v) > cases[3].std0).sum() == 0 and (np.sqrt(v) > cases[3].std1).any() and (np.sqrt(v[v > 0]) < cases[3].std1).any()
    for case in spc.searched_cases("cartpole"):
        c = spc.check_nodes(case, 64, None)
        assert c.clamped == 0 and c.ambiguous == 0
    w, _, took = spc.bernoulli_case("cartpole").reference(64)
    assert not took.any()


@pytest.mark.parametrize("group", list(spc.GROUPS))
@pytest.mark.parametrize("model", MODELS)
def test_the_oracle_follows_the_exact_spline(model, group):
    run = lambda interp, knots, nodes: spc.run_spline_oracle(model, interp, knots, nodes)
    total = spc.spline_group(model, group, run, 64, scale=0.25)
    print(f"oracle spline {model} {group}: worst error / bound {0.25 * total.worst:.3f} ({total.where}); largest bound / range "
          f"{total.worst_bound:.2e}; {total}")
    total.assert_shares((model, group), spc.GROUPS[group][1])


@pytest.mark.parametrize("group", list(spc.GROUPS))
@pytest.mark.parametrize("model", ["cartpole", "particle", "humanoid"])
def test_the_fp32_cases_keep_their_caps_and_census(model, group):
    """the reference alone on the float roundings of the oracle's step times"""
    def run(interp, knots, nodes):
        _, _, times = spc.run_spline_oracle(model, interp, knots, nodes)
        return fpc.rounded(nodes, 32), None, fpc.rounded(times, 32)
    total = spc.spline_group(model, group, run, 32)
    print(f"fp32 reference {model} {group}: largest bound / range {total.worst_bound:.2e}; {total}")
    total.assert_shares((model, group), spc.GROUPS[group][1])


def _emu_run(emu, model, precision=None):
    pm, pt = fpc.packed(model)
    _, start, mocap = fpc.setup(model)
    kw = {} if precision is None else {"precision": precision}

    def run(interp, knots, nodes):
        nodes = np.asarray(nodes, float)
        r = emu.rollout(pm, pt, start, spc.T0, mocap, nodes.shape[0], spc.H, nodes.shape[1], interp, knots, node_values=nodes, **kw)
        assert not r["flags"].any() and not r["failure"].any(), r["flags"]
        return fpc.rounded(nodes, precision or 64), r["actions"], r["times"]
    return run


@pytest.mark.parametrize("group", list(spc.GROUPS))
def test_the_quad_form_follows_the_exact_spline(group):
    from mujoco_mpc_amd import capi  # noqa: F401
    from tests import quademu
    total = spc.spline_group("a1", group, _emu_run(quademu, "a1"), 64)
    print(f"quad emulator {group}: worst error / bound {total.worst:.3f} ({total.where}); {total}")
    total.assert_shares(("quad emulator", group), spc.GROUPS[group][1])


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("group", list(spc.GROUPS))
def test_the_limb_form_follows_the_exact_spline(group, precision):
    from mujoco_mpc_amd import capi  # noqa: F401
    from tests import limbemu
    total = spc.spline_group("humanoid", group, _emu_run(limbemu, "humanoid", precision), precision)
    print(f"limb emulator fp{precision} {group}: worst error / bound {total.worst:.3f} ({total.where}); {total}")
    total.assert_shares(("limb emulator", group), spc.GROUPS[group][1])


@pytest.mark.parametrize("which", ["quad", "limb64", "limb32"])
def test_the_emulated_kernels_draw_the_exact_nodes(which):
    from mujoco_mpc_amd import capi  # noqa: F401
    from tests import limbemu, quademu
    model, emu, precision = {"quad": ("a1", quademu, 64), "limb64": ("humanoid", limbemu, 64), "limb32": ("humanoid", limbemu, 32)}[which]
    pm, pt = fpc.packed(model)
    _, start, mocap = fpc.setup(model)
    kw = {} if which == "quad" else {"precision": precision}
    total = spc.Census()
    for case in spc.noise_cases(model, 8) + spc.searched_cases(model) + [spc.bernoulli_case(model)]:
        r = emu.rollout(pm, pt, start, case.t0, mocap, case.N, 2, case.P, 0, case.node_times(), noise=case.spec(), nominal=case.nominal, **kw)
        total.add(spc.check_nodes(case, precision, r["nodes"]))
    acts = spc.Census()
    for ce in (False, True):      # the environments of the batched GPU launches, one by one: H = 12, cubic; nothing handed on
        for case in spc.batched_noise_cases(model, 8, ce=ce):
            r = emu.rollout(pm, pt, start, case.t0, mocap, case.N, spc.H, case.P, 2, case.node_times(), noise=case.spec(), nominal=case.nominal, **kw)
            assert not r["flags"].any() and not r["failure"].any(), (case.name, r["flags"])
            total.add(spc.check_nodes(case, precision, r["nodes"]))
            acts.add(spc.check_actions(case.name, model, precision, spc.Grid(case.node_times(), precision), 2, r["nodes"], r["actions"], r["times"]))
    print(f"{which} emulator nodes: worst error / bound {total.worst:.3f} ({total.where}); {total}; actions of the noised nodes {acts.worst:.3f}, {acts}")
    total.assert_shares(which, clamped=None)
    assert total.clamped >= 5 and total.interior >= 100, total


@pytest.mark.parametrize("model", ["cartpole", "particle"])
def test_the_python_spline_follows_the_exact_spline(model):
    from mujoco_mpc_amd.spline import TimeSpline
    r = spc.ctrlrange(model, 64)

    def run(interp, knots, nodes):
        nodes = np.asarray(nodes, float)[:6]
        _, _, times = spc.run_spline_oracle(model, interp, knots, nodes)
        actions = np.zeros((nodes.shape[0], spc.H, r.shape[0]))
        for c in range(nodes.shape[0]):
            s = TimeSpline(r.shape[0], interp)
            for t, v in zip(knots, nodes[c]):
                s.add_node(t, v)
            for t in range(spc.H - 1):
                actions[c, t] = np.clip(s.sample(times[c, t]), r[:, 0], r[:, 1])
            actions[c, spc.H - 1] = actions[c, spc.H - 2]
        return nodes, actions, times
    total = spc.Census()
    for group in spc.GROUPS:
        total.add(spc.spline_group(model, group, run, 64))
    print(f"TimeSpline.sample {model}: worst error / bound {total.worst:.3f} ({total.where})")
