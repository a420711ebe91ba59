"""-m gpu: backward_pass_kernel's box-QP, gains and shape edges against answers that need no solver to state (riccati_cases.py; the
harness is proven on the CPU by test_riccati_cases.py).
   (a) chains, boxed      <-> the KKT-verified long-double answer         1e-9 (1 + |x|); clamped gains 0.0, clamped du the bound, bit for bit
   (b) chains, unboxed    <-> -H^-1 g, -H^-1 Qxu' in long double          1e-9 (1 + |x|)
   (c) coupled shapes     <-> oracle oriccati                             1e-9 (1 + |x|)
   (d) cond(Quu) to 1e11  <-> long double; the oracle's own error (floor 2^-53 kappa) is the yardstick, factor 8
   (e) pivot threshold    <-> exact pivots either side of 1e-15
   (f) a call's bits do not depend on the calls before it
n and m are the call's, not the model's: the Cartpole context only provides a device and a stream."""
import functools

import numpy as np
import pytest

import riccati_cases as rc
from mujoco_mpc_amd import capi
from oracle import pyoracle

pytestmark = pytest.mark.gpu

TOL = 1e-9              # the tolerance this kernel carries in test_gpu_ilqg.py
OUTPUTS = ("du", "K", "Vx", "Vxx", "dV")


@pytest.fixture(scope="module")
def ctx(cartpole):
    c = capi.Context(cartpole.packed_model(), cartpole.packed(), 0, 64)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def chain_of(m, n):
    return rc.chain(m, n, rc.CHAIN_T, rc.chain_seed(m, n), **rc.chain_options(m, n))


def check_last_index_repeats(out, T):
    assert np.array_equal(out["K"][T - 1], out["K"][T - 2]) and np.array_equal(out["du"][T - 1], out["du"][T - 2])


def worst_errors(out, ex):
    return {k: rc.rel_err(out[k], ex[k]) for k in OUTPUTS}


@pytest.mark.parametrize("mu", rc.CHAIN_MU)
@pytest.mark.parametrize("m", rc.CHAIN_M)
def test_boxed_chains_against_the_exact_answer(ctx, m, mu):
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for n in rc.CHAIN_N:
        ch = chain_of(m, n)
        ref = pyoracle.riccati(n, m, ch.T, mu, 0, 1, *ch.args)        # proposes the active sets; what is compared against is exact
        ex = rc.exact_chain(ch, mu, 1, ref["du"])
        assert ref["ok"] and ex["rejected"] == 0
        out = ctx.backward_pass(mu, 0, 1, *ch.args)
        assert out["ok"]
        err = worst_errors(out, ex)
        worst = {k: max(worst[k], err[k]) for k in OUTPUTS}
        assert all(v <= TOL for v in err.values()), (n, err)
        clamped = ~ex["free"]
        assert np.all(out["K"][:-1][clamped] == 0.0), n                                        # (steps, m, n)[mask] -> rows of clamped controls
        bound = np.where(ex["du"][:-1] == ch.lo, ch.lo, ch.hi)
        assert np.array_equal(out["du"][:-1][clamped], bound[clamped]), n                      # limits - action, bit for bit
        check_last_index_repeats(out, ch.T)
    print(f"boxed chains m={m} mu={mu} worst error vs exact: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("mu", rc.CHAIN_MU)
@pytest.mark.parametrize("m", rc.CHAIN_M)
def test_unboxed_chains_against_the_exact_answer(ctx, m, mu):
    """use_limits = 0: the boxed == false path through the shared solver body"""
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for n in rc.CHAIN_N:
        ch = chain_of(m, n)
        ex = rc.exact_chain(ch, mu, 0)
        out = ctx.backward_pass(mu, 0, 0, *ch.args)
        assert out["ok"]
        err = worst_errors(out, ex)
        worst = {k: max(worst[k], err[k]) for k in OUTPUTS}
        assert all(v <= TOL for v in err.values()), (n, err)
        check_last_index_repeats(out, ch.T)
    print(f"unboxed chains m={m} mu={mu} worst error vs exact: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("m", rc.COUPLED_M)
@pytest.mark.parametrize("n", rc.COUPLED_N)
def test_coupled_shape_sweep_against_the_oracle(ctx, n, m):
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for T in rc.COUPLED_T:
        prob = rc.coupled(n, m, T, rc.coupled_seed(n, m), rc.coupled_limit_scale(n, m))
        for reg_type, limits in rc.COUPLED_REG:
            for mu in rc.COUPLED_MU:
                out = ctx.backward_pass(mu, reg_type, limits, *prob)
                ref = pyoracle.riccati(n, m, T, mu, reg_type, limits, *prob)
                assert out["ok"] and ref["ok"], (T, reg_type, limits, mu)
                err = worst_errors(out, ref)
                worst = {k: max(worst[k], err[k]) for k in OUTPUTS}
                assert all(v <= TOL for v in err.values()), (T, reg_type, limits, mu, err)
                check_last_index_repeats(out, T)
    print(f"coupled n={n} m={m} worst error vs oracle: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))


def du_errors(du, exact):
    """per step: |du - exact|max / |exact|max"""
    exact = np.asarray(exact, rc.LD)
    return np.asarray(np.max(np.abs(np.asarray(du, rc.LD) - exact), axis=1) / np.max(np.abs(exact), axis=1), float)


@pytest.mark.parametrize("limits", [0, 1])
@pytest.mark.parametrize("m", rc.KAPPA_M)
@pytest.mark.parametrize("kappa", rc.KAPPAS)
def test_ill_conditioned_quu(ctx, kappa, m, limits):
    """cuu = Q diag(lambda) Q', cond = kappa; unboxed, and boxed with a range nothing reaches. The kernel's pivots are a 2-ulp root and a
    multiplication by a reciprocal where the oracle has a correctly rounded root and a division: its error on du may be 8 times the
    oracle's own on the same problem (with the textbook floor 2^-53 kappa, so that a lucky oracle does not fail the kernel), no more."""
    ch = rc.kappa_chain(kappa, m)
    n, T = ch.n, ch.T
    ref = pyoracle.riccati(n, m, T, 0.0, 0, limits, *ch.args)
    out = ctx.backward_pass(0.0, 0, limits, *ch.args)
    assert out["ok"] and ref["ok"]
    ex = rc.exact_chain(ch, 0.0, limits, ref["du"])
    assert ex["rejected"] == 0 and ex["free"].all()
    ek, eo = du_errors(out["du"][:-1], ex["du"][:-1]), du_errors(ref["du"][:-1], ex["du"][:-1])
    ratio = ek / np.maximum(eo, 2.0 ** -53 * kappa)
    print(f"kappa={kappa:.0e} m={m} limits={limits}: kernel err {ek.max():.2e} oracle err {eo.max():.2e} worst ratio {ratio.max():.3f}")
    assert np.all(ratio <= 8.0), ratio.max()


@pytest.mark.parametrize("limits", [0, 1])
@pytest.mark.parametrize("m", rc.PIVOT_M)
@pytest.mark.parametrize("where", ["last_processed", "middle"])
def test_pivot_threshold(ctx, where, m, limits):
    """the 1e-15 threshold sits a factor 1e3 from either case"""
    t_bad = 0 if where == "last_processed" else rc.PIVOT_T // 2
    ch = rc.pivot_chain(m, t_bad, 1e-12)
    ref = pyoracle.riccati(ch.n, m, ch.T, 0.0, 0, limits, *ch.args)
    out = ctx.backward_pass(0.0, 0, limits, *ch.args)
    assert out["ok"] and ref["ok"]
    ex = rc.exact_chain(ch, 0.0, limits, ref["du"])
    assert ex["rejected"] == 0 and ex["free"][t_bad, m // 2]
    assert all(v <= 1e-12 for v in worst_errors(ref, ex).values())       # the algorithm reaches the exact answer here
    err = worst_errors(out, ex)
    assert all(v <= TOL for v in err.values()), err
    assert abs(out["du"][t_bad, m // 2] + 0.1) < 1e-12
    for smallest in (1e-18, -1e-12):
        ch = rc.pivot_chain(m, t_bad, smallest)
        assert not pyoracle.riccati(ch.n, m, ch.T, 0.0, 0, limits, *ch.args)["ok"]
        assert not ctx.backward_pass(0.0, 0, limits, *ch.args)["ok"], smallest


@pytest.mark.parametrize("m", [12, 13])
def test_a_call_does_not_see_the_calls_before_it(ctx, m):
    """dV, ok, the warm start and the W / Qxx roles are set up by the sweep itself (the batched kernel's retry loop relies on it): a failing
    call that stops midway between two identical calls changes none of the second one's bits"""
    ch = chain_of(m, 17)
    first = ctx.backward_pass(0.3, 0, 1, *ch.args)
    bad = list(chain_of(m, 3).args)
    bad[6] = bad[6].copy()
    bad[6][20] = -bad[6][20]                  # cuu indefinite at a middle step: an odd number of W / Qxx swaps, a warm start left behind
    assert first["ok"] and not ctx.backward_pass(0.0, 0, 1, *bad)["ok"]
    again = ctx.backward_pass(0.3, 0, 1, *ch.args)
    assert again["ok"]
    for k in OUTPUTS:
        assert np.array_equal(first[k], again[k]), k
