"""-m gpu: mjpcx_mppi_update_batched (mppi_weights_kernel, mppi_mean_kernel: csrc/mppi_update.h) held to its contract on returns the
test INJECTS (tests/mppi_cases.py, on selection_cases.py's return vectors and inject()).

A tiny rollout (Particle with P = 1 and P = 3 nodes, nu = 2; Cartpole with P = 3, nu = 1; H = 2; 64- and 32-bit contexts) only sizes the
buffers and puts nodes the test chose on the device; its returns are then overwritten with vectors whose answer is known: the unique
minimum and tied minima at and across lanes 15/16, 63/64, 255/256, NaN of both payloads, +inf, -inf as the minimum, signed zeros, the 1e6
of failed rollouts, all NaN, all +inf, all equal, a spread whose weights run through the subnormals to exact 0, a neighbour one ulp above
the minimum, returns near 1e3 -- each with its own temperature (0.5 .. 1e4, 1e-300, 1e300), a different case and temperature in each of the
E = 3 environments. index, best_return and ref_return are compared bit for bit with the contract AND with mjpcx_best_batched on the same
injection; the weights with mpmath at (2|x| + 2 ULP_FN + 1) u; weight_sum, effective_samples and mean with exact rational arithmetic
about the device's own weights at the bounds derived in mppi_cases' docstring; mean inside the nodes' hull; a second call and the same
data as a fleet of one give the same bits. Every test prints its worst error / bound. Worst on the MI355X over all of them: weights
0.50 (a subnormal result's rounding, half a spacing against the floor of one), weight_sum 0.21, effective_samples 0.17, mean 0.17 -- the
numpy emulation's figures (tests/test_mppi_cases.py).

Not exercised: MJPCX_EUNSUPPORTED on a sharded context, which needs two ranks (as the other batched entry points' tests)."""
import numpy as np
import pytest

import mppi_cases as mc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.task import load_task
from test_gpu_batch_models import fleet, refused

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
H, E = 2, mc.SEG_E
STATE = {"Cartpole": ([0.0, 0.1, 0.0, 0.0], None), "Particle": ([0.05, -0.1, 0.2, 0.0], [0.15, -0.1, 0.01, 1, 0, 0, 0.0])}
CONFIGS = [(m, P, prec) for m, P in (("Particle", 1), ("Particle", 3), ("Cartpole", 3)) for prec in (64, 32)]
IDS = [f"{m}-P{P}-fp{prec}" for m, P, prec in CONFIGS]
KEYS = ("index", "best_return", "ref_return", "weight_sum", "effective_samples", "valid", "mean", "weights")
_TASKS = {}


def make_context(model, precision):
    t = _TASKS.setdefault(model, load_task(model))
    return capi.Context(t.packed_model(), t.packed(), 0, precision)


def rollout_fleet(ctx, model, P, num_envs, nodes):
    """nodes [num_envs * n][P * nu], environment-major: after this the device holds them and num_envs x n returns to overwrite"""
    state, mocap = STATE[model]
    ctx.set_states(np.tile(state, (num_envs, 1)) + 0.01 * np.arange(num_envs)[:, None], np.zeros(num_envs),
                   None if mocap is None else np.tile(mocap, (num_envs, 1)))
    times = np.linspace(0.0, 0.02, P) if P > 1 else np.zeros(1)
    ctx.rollout_splines_batched(H, capi.SPLINE_CUBIC if P > 1 else capi.SPLINE_ZERO, np.tile(times, (num_envs, 1)),
                                nodes.reshape(num_envs, -1, P, ctx.nu), num_envs=num_envs)


def env_of(out, e):
    return {k: out[k][e] for k in KEYS if out[k] is not None}


def same_outputs(a, b):
    return all(mc.same_bits(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)) for k in a)


def check_env(got, ret, lam, dev, ref, worst, where):
    """one environment's outputs (env_of) against the contract and the bounds"""
    w, beta, ref_return, valid = mc.contract(ret, ref)
    assert got["index"] == w and got["valid"] == valid, where + (got["index"], w)
    assert mc.same_bits(got["best_return"], beta), where
    assert mc.same_bits(got["ref_return"], ref_return) if ref >= 0 else np.isnan(got["ref_return"]), where
    worst["weights"] = max(worst.get("weights", 0.0), mc.check_weights(got["weights"], ret, lam))
    assert worst["weights"] <= 1.0, where + (worst["weights"],)
    assert np.array_equal(got["weights"] == 1.0, (ret == beta) & bool(valid)) or lam >= 1e4, where
    mc.check_outputs(dict(got, mean=got["mean"].reshape(-1)), ret, dev, ref, worst)


@pytest.mark.parametrize("n", mc.SEG_N)
@pytest.mark.parametrize("model,P,precision", CONFIGS, ids=IDS)
def test_update_on_injected_returns(model, P, precision, n):
    ctx = make_context(model, precision)
    npar = P * ctx.nu
    nodes = mc.scaled_nodes(E * n, npar, seed=n + P)
    dev = mc.as_device(nodes, precision)
    rollout_fleet(ctx, model, P, E, nodes)
    for c in (0, n, E * n - 1):
        assert np.array_equal(ctx.fetch_spline(c).reshape(-1), dev[c]), c
    rounds = mc.mppi_rounds(n)
    worst, kept = {}, {}
    alone = sorted({0, 2, len(rounds) // 2, len(rounds) - 2, len(rounds) - 1})    # rounds repeated below as fleets of one
    for ri, cases in enumerate(rounds):
        ret = np.concatenate([c[1] for c in cases])
        lam = np.array([c[2] for c in cases])
        fail = ((np.arange(E * n) + ri) % 2).astype(np.int32)           # arbitrary failure words: they are not consulted
        mc.inject(ctx, ret, fail)
        ref = (n - 1, 0, -1)[ri % 3]
        out = ctx.mppi_update_batched(E, lam, ref, want_weights=True)
        idx, br, rr, _ = ctx.best_batched(E, ref)
        assert np.array_equal(out["index"], idx) and mc.same_bits(out["best_return"], br), [c[0] for c in cases]
        assert mc.same_bits(out["ref_return"], rr) if ref >= 0 else np.isnan(out["ref_return"]).all()
        for e, (name, r, lam_e) in enumerate(cases):
            check_env(env_of(out, e), r, lam_e, dev[e * n:(e + 1) * n], ref, worst, (name, e, n))
        if ri < 2:                                                      # a second call on the same buffers; one without the weights
            again = ctx.mppi_update_batched(E, lam, ref, want_weights=True)
            bare = ctx.mppi_update_batched(E, lam, ref)
            assert same_outputs(out, again) and bare["weights"] is None
            assert same_outputs({k: v for k, v in bare.items() if v is not None}, {k: out[k] for k in KEYS if k != "weights"})
        if ri in alone:
            kept[ri] = (ri % E, ref, out)
    for ri, (e, ref, out) in kept.items():                              # environment e of the fleet == the same data as a fleet of one
        name, r, lam_e = rounds[ri][e]
        rollout_fleet(ctx, model, P, 1, nodes[e * n:(e + 1) * n])
        mc.inject(ctx, r)
        one = ctx.mppi_update_batched(1, [lam_e], ref, want_weights=True)
        assert same_outputs(env_of(one, 0), env_of(out, e)), (name, e, n)
    print(f"{model} P={P} fp{precision} n={n}: {len(rounds)} rounds x {E} environments, worst error / bound {worst}")
    ctx.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_one_environment_of_the_largest_size(precision):
    model, P, n = "Particle", 3, mc.N_LARGE
    ctx = make_context(model, precision)
    nodes = mc.scaled_nodes(n, P * ctx.nu, seed=1)
    dev = mc.as_device(nodes, precision)
    rollout_fleet(ctx, model, P, 1, nodes)
    name, ret, lam = mc.large_case()
    mc.inject(ctx, ret)
    out = ctx.mppi_update_batched(1, lam, 0, want_weights=True)
    again = ctx.mppi_update_batched(1, [lam], 0, want_weights=True)
    assert same_outputs(out, again)
    idx, br, rr, _ = ctx.best_batched(1, 0)
    assert out["index"][0] == idx[0] == 255 and mc.same_bits(out["best_return"], br) and mc.same_bits(out["ref_return"], rr)
    worst = {}
    check_env(env_of(out, 0), ret, lam, dev, 0, worst, (name, 0, n))
    w = out["weights"][0]
    assert (w == 0).sum() > 1000 and ((w > 0) & (w < 2.0 ** -1022)).any() and (w == 1).sum() == 2
    print(f"{model} fp{precision} n={n}: worst error / bound {worst}")
    ctx.close()


def test_update_refused():
    model, P, n = "Particle", 3, 64
    ctx = make_context(model, 64)
    rollout_fleet(ctx, model, P, E, mc.scaled_nodes(E * n, P * ctx.nu, seed=2))
    ok = ctx.mppi_update_batched(E, 1.0)
    refused(lambda: ctx.mppi_update_batched(2, 1.0), EINVAL, "not a batched one of 2")
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        refused(lambda: ctx.mppi_update_batched(E, [1.0, bad, 1.0]), EINVAL, "temperature of environment 1")
    refused(lambda: ctx.mppi_update_batched(E, [1.0, 1.0, 0.0]), EINVAL, "temperature of environment 2")
    for ref in (-2, n, n + 5):
        refused(lambda: ctx.mppi_update_batched(E, 1.0, ref), EINVAL, "ref_candidate")
    assert same_outputs({k: v for k, v in ok.items() if v is not None},
                        {k: v for k, v in ctx.mppi_update_batched(E, 1.0).items() if v is not None})     # a refusal changes nothing
    state, mocap = STATE[model]
    ctx.set_state(state, 0.0, mocap)
    ctx.rollout_splines(H, capi.SPLINE_CUBIC, np.linspace(0.0, 0.02, P), mc.scaled_nodes(192, P * ctx.nu, seed=3).reshape(-1, P, ctx.nu))
    refused(lambda: ctx.mppi_update_batched(3, 1.0), EINVAL, "not a batched one")
    ctx.close()


def test_update_refused_after_a_pruned_rollout_and_works_after_an_ensemble():
    f = fleet("quad", ("base", "base"), n=64, H=4)
    ctx = f.make_context()
    f.push(ctx, models=False)
    ctx.set_pruning_batched(True, f.E)
    f.run(ctx, "noise")                                                  # a pruned batched launch: its stored returns are no returns
    refused(lambda: ctx.mppi_update_batched(f.E, 1.0), ESTATE, "pruned")
    ctx.set_pruning_batched(False)
    f.run(ctx, "noise")
    out = ctx.mppi_update_batched(f.E, 1.0, 0)
    idx, br, rr, _ = ctx.best_batched(f.E, 0)
    assert np.array_equal(out["index"], idx) and mc.same_bits(out["best_return"], br) and mc.same_bits(out["ref_return"], rr)
    assert out["valid"].all() and (out["weight_sum"] >= 1.0).all()
    ctx.rollout_noise_ensemble(f.n, f.H, capi.SPLINE_CUBIC, f.times[0], f.nominal[0], f.noise(), num_hypotheses=f.E)
    ens = ctx.mppi_update_batched(f.E, 1.0, 0)                           # the M x n of an ensemble launch is a batched rollout too
    assert np.array_equal(ens["index"], ctx.best_batched(f.E, 0)[0]) and ens["valid"].all()
    ctx.close()
