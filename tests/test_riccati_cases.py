"""The backward-pass harness of riccati_cases.py, proven on the CPU before a GPU sees it: every chain problem that
tests/test_gpu_backward_pass.py runs (same seeds and parameters, imported from the harness) has a KKT-verified exact answer, the oracle's
Riccati step and box-QP match it at 1e-12 (1 + |x|) -- up to m = 16, where test_oracle_riccati.py::test_boxqp_against_bruteforce stops
at 4 --, and the problems reach the solver paths they are there for (asserted, not hoped)."""
import functools

import numpy as np
import pytest

import riccati_cases as rc
from oracle import pyoracle

TOL = 1e-12
OUTPUTS = ("du", "K", "Vx", "Vxx", "dV")


@functools.lru_cache(maxsize=None)
def solved(m, n, mu):
    ch = rc.chain(m, n, rc.CHAIN_T, rc.chain_seed(m, n), **rc.chain_options(m, n))
    ref = pyoracle.riccati(n, m, ch.T, mu, 0, 1, *ch.args)
    return ch, ref, rc.exact_chain(ch, mu, 1, ref["du"])


def test_long_double_is_wider_than_double():
    assert np.finfo(rc.LD).eps < 1e-18


@pytest.mark.parametrize("mu", rc.CHAIN_MU)
@pytest.mark.parametrize("m", rc.CHAIN_M)
def test_every_chain_problem_has_a_verified_exact_answer_and_the_oracle_matches_it(m, mu):
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for n in rc.CHAIN_N:
        ch, ref, ex = solved(m, n, mu)
        assert ref["ok"]
        assert ex["rejected"] == 0, (n, ex["rejected"])                  # none may be left out: a seed that breaks this is changed, not the slack
        assert np.array_equal(rc.free_rows(ref["K"]), ex["free"]), n     # the oracle's gains are zero on exactly the clamped rows
        for k in OUTPUTS:
            worst[k] = max(worst[k], rc.rel_err(ref[k], ex[k]))
    print(f"m={m} mu={mu} oracle vs exact: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


@pytest.mark.parametrize("mu", rc.CHAIN_MU)
@pytest.mark.parametrize("m", [m for m in rc.CHAIN_M if m <= 5])
def test_exact_answer_equals_bruteforce_over_active_sets(m, mu):
    for n in rc.CHAIN_N:
        ch, _, ex = solved(m, n, mu)
        for t in range(ch.T - 1):
            x = rc.bruteforce_boxqp(rc.regularised(ch.H[t], mu), ch.g[t], ch.lo[t], ch.hi[t])
            assert rc.rel_err(x, ex["du"][t]) <= 1e-10, (n, t)


@pytest.mark.parametrize("mu", rc.CHAIN_MU)
@pytest.mark.parametrize("m", rc.CHAIN_M)
def test_chains_reach_every_solver_path(m, mu):
    """per m (and regularisation), over its three chains, in the oracle's result"""
    allfree = allclamped = mixed = changes = zero_width = 0
    for n in rc.CHAIN_N:
        ch, ref, ex = solved(m, n, mu)
        a, c, x, d = rc.census(rc.free_rows(ref["K"]))
        allfree, allclamped, mixed, changes = allfree + a, allclamped + c, mixed + x, changes + d
        zero_width += int(np.sum(ch.lo == ch.hi))
        # the coordinate sitting on its bound with zero gradient: there, exactly on the bound, and counted free
        t, i = ch.zero_grad_step, min(1, m - 1)
        assert ch.lo[t, i] == 0.0 and ref["du"][t, i] == 0.0 and np.all(ch.g[t] == 0.0)
        assert np.all(rc.regularised(ch.H[t], mu) @ ref["du"][t] + ch.g[t] == 0.0) and ex["free"][t].all()
    assert allfree >= 5 and allclamped >= 5 and changes >= 1 and zero_width >= 1, (allfree, allclamped, mixed, changes, zero_width)
    assert mixed >= 20 or m == 1, mixed


def coupled_census(n, m, reg_type):
    """steps of the cell's limited problems over both horizons and regularisations: (all free, all clamped, mixed)"""
    tot = np.zeros(3, int)
    for T in rc.COUPLED_T:
        for mu in rc.COUPLED_MU:
            prob = rc.coupled(n, m, T, rc.coupled_seed(n, m), rc.coupled_limit_scale(n, m))
            ref = pyoracle.riccati(n, m, T, mu, reg_type, 1, *prob)
            assert ref["ok"]
            tot += rc.census(rc.free_rows(ref["K"]))[:3]
    return tot


@pytest.mark.parametrize("m", rc.COUPLED_M)
def test_coupled_sweep_binds_in_every_cell(m):
    for n in rc.COUPLED_N:
        for reg_type in sorted({r for r, lim in rc.COUPLED_REG if lim}):
            allfree, allclamped, mixed = coupled_census(n, m, reg_type)
            if m >= 2:
                assert mixed >= 1, (n, reg_type, allfree, allclamped, mixed)
            else:                           # one control: a step is free or clamped; the range binds somewhere in the cell
                assert allclamped >= 1, (n, reg_type, allfree, allclamped)


@pytest.mark.parametrize("limits", [0, 1])
def test_the_conditioning_and_pivot_chains_have_verified_exact_answers(limits):
    """the remaining chains of the GPU file: none rejected; where the pivot chain's smallest entry is 1e-12 the algorithm reaches the exact
    answer, and the oracle refuses 1e-18 and -1e-12"""
    for kappa in rc.KAPPAS:
        for m in rc.KAPPA_M:
            ch = rc.kappa_chain(kappa, m)
            ref = pyoracle.riccati(ch.n, m, ch.T, 0.0, 0, limits, *ch.args)
            ex = rc.exact_chain(ch, 0.0, limits, ref["du"])
            assert ref["ok"] and ex["rejected"] == 0 and ex["free"].all(), (kappa, m)
            assert np.linalg.cond(ch.H[0]) == pytest.approx(kappa, rel=1e-3)
    for m in rc.PIVOT_M:
        for t_bad in (0, rc.PIVOT_T // 2):
            ch = rc.pivot_chain(m, t_bad, 1e-12)
            ref = pyoracle.riccati(ch.n, m, ch.T, 0.0, 0, limits, *ch.args)
            ex = rc.exact_chain(ch, 0.0, limits, ref["du"])
            assert ref["ok"] and ex["rejected"] == 0 and ex["free"][t_bad, m // 2], (m, t_bad)
            assert all(rc.rel_err(ref[k], ex[k]) <= TOL for k in OUTPUTS), (m, t_bad)
            if limits and m > 1:
                assert rc.census(ex["free"])[2] >= 1, (m, t_bad)                 # masks with exact pivots: some steps are mixed
            for smallest in (1e-18, -1e-12):
                bad = rc.pivot_chain(m, t_bad, smallest)
                assert not pyoracle.riccati(bad.n, m, bad.T, 0.0, 0, limits, *bad.args)["ok"], (m, t_bad, smallest)
