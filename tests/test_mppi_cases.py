"""The MPPI harness (tests/mppi_cases.py) against itself, no GPU: the numpy emulation of mppi_weights_kernel / mppi_mean_kernel stays
inside every derived bound on every data set tests/test_gpu_mppi_update.py uses, a kernel that does not subtract the best return falls
far outside them, and the winner follows order() on ties, NaN and signed zeros.

Worst share of each bound over all those data sets, emulation (numpy's exp), fp64 and fp32 nodes: weights 0.50 of (2|x| + 2 ULP_FN + 1) u w +
2^-1074 (a subnormal result's rounding, half a spacing, against the floor of one), weight_sum 0.21 of (m + 8) u, effective_samples 0.17 of
(3 m + 27) u, mean 0.17 of (m + 9) u (A + |S|) / eta (printed by the tests)."""
import numpy as np
import pytest

import mppi_cases as mc

NP = 6   # Particle's P * nu at P = 3


def _check_env(name, ret, lam, nodes, ref, worst, **kw):
    out = mc.emulate_mppi(ret, lam, nodes, ref, **kw)
    want = mc.contract(ret, ref)
    assert out["index"] == want[0] and out["valid"] == want[3], name
    worst["weights"] = max(worst.get("weights", 0.0), mc.check_weights(out["weights"], ret, lam))
    assert worst["weights"] <= 1.0, (name, worst)
    mc.check_outputs(out, ret, nodes, ref, worst)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", mc.SEG_N)
def test_the_emulation_is_inside_every_bound(n, precision):
    nodes = mc.as_device(mc.scaled_nodes(n, NP, seed=n), precision)
    worst = {}
    for k, (name, ret, lam) in enumerate(mc.mppi_cases(n)):
        _check_env(name, ret, lam, nodes, (n - 1, 0, -1)[k % 3], worst)
    print(f"n={n} fp{precision}: worst error / bound {worst}")
    assert worst["weights"] > 0 and worst["mean"] > 0     # (the bounds were exercised: not everything was exact)


def test_the_emulation_is_inside_every_bound_at_the_largest_size():
    name, ret, lam = mc.large_case()
    nodes = mc.scaled_nodes(mc.N_LARGE, NP, seed=1)
    worst = {}
    _check_env(name, ret, lam, nodes, 0, worst)
    w = mc.contract_weights(ret, lam)
    assert (w == 0).sum() > 1000 and ((w > 0) & (w < 2.0 ** -1022)).any() and (w == 1).sum() == 2   # exact zeros, subnormals, the tie
    print(f"n={mc.N_LARGE}: worst error / bound {worst}")


def test_a_kernel_that_does_not_subtract_the_best_return_is_far_outside():
    n = 320
    name, ret, lam = [c for c in mc.mppi_cases(n) if c[0] == "offset-1e3"][0]
    nodes = mc.scaled_nodes(n, NP, seed=3)
    _check_env(name, ret, lam, nodes, 0, {})                  # the right kernel: inside
    wrong = mc.emulate_mppi(ret, lam, nodes, 0, shift=False)
    assert wrong["weight_sum"] == 0.0 and not np.any(wrong["weights"])     # exp(-1e4): every weight underflows
    assert mc.check_weights(wrong["weights"], ret, lam) > 1e12            # the winner's weight is 1: off by the whole of it
    with pytest.raises(AssertionError):
        mc.check_outputs(wrong, ret, nodes, 0, {})


def test_the_winner_follows_order_on_ties_nan_and_signed_zeros():
    n = 320
    seen = set()
    for name, ret, lam in mc.mppi_cases(n):
        w, beta, ref_return, valid = mc.contract(ret, 5)
        assert w == mc.order(ret)[0] and mc.same_bits(beta, ret[w]) and mc.same_bits(ref_return, ret[5]), name
        numbers = ret[~np.isnan(ret)]
        if numbers.size:
            assert beta == numbers.min() and w == int(np.flatnonzero(ret == beta)[0]), name     # the lowest index among the minima
        else:
            assert w == 0 and not valid, name
        assert valid == int(numbers.size > 0 and numbers.min() < np.inf), name
        wts = mc.contract_weights(ret, lam)
        assert np.array_equal(wts == 1.0, (ret == beta) & bool(valid)) or lam >= 1e4, name      # ties weigh 1 each; -0.0 == +0.0
        if name.startswith("zeros"):
            assert beta == 0 and (wts == 1.0).sum() == 2
            seen.add(bool(np.signbit(beta)))
    assert seen == {True, False}                              # the winner carried either sign of zero
    assert np.isnan(mc.contract(mc.base(n, 1), -1)[2])
