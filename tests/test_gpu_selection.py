"""-m gpu: the kernels that choose candidates -- argmin_kernel, sort_kernel, best_kernel, best_segmented_kernel, elite_moments_kernel,
ce_update_kernel, robust_select_kernel (mjpcx.hip) -- held to exact answers on returns the test INJECTS (tests/selection_cases.py).

A rollout (Cartpole, nu = 1, and Particle, nu = 2; H = 2, P = 3; 64- and 32-bit contexts) only sizes the buffers and puts nodes the
test chose on the device; its returns and failure flags are then overwritten through mjpcx_device_buffer with vectors whose order
is known: the unique minimum and tied minima at and across lanes 15/16, 63/64, 255/256, 1023/1024, NaN (both signs), infinities,
signed zeros, the 1e6 of failed rollouts, all NaN, all equal. Indices and returns are compared with selection_cases.order() bit for
bit; the elites' mean, variance and mean return with exact rational arithmetic at the bounds derived in selection_cases' docstring
((m + 8) u, (m + 10) u absolute on sum |x|, (m + 16) u relative for the squares, m = ceil(n_elite / 256)). Every test prints its worst
error / bound.

mjpcx_best writes the reference candidate's failure flag into its record but the C ABI does not hand it out, so the flag is read
back with mjpcx_get_return_at instead. The score half of mjpcx_robust_step_batched is tests/test_gpu_batch_robust.py's."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import selection_cases as sc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.cstructs import as_i32p
from mujoco_mpc_amd.task import load_task

pytestmark = pytest.mark.gpu
H, P = 2, 3
TIMES = np.linspace(0.0, 0.02, P)
STATE = {"Cartpole": ([0.0, 0.1, 0.0, 0.0], None), "Particle": ([0.05, -0.1, 0.2, 0.0], [0.15, -0.1, 0.01, 1, 0, 0, 0.0])}
CONFIGS = [("Cartpole", 64), ("Cartpole", 32), ("Particle", 64), ("Particle", 32)]
IDS = [f"{m}{p}" for m, p in CONFIGS]


@lru_cache(maxsize=None)
def _task(model):
    return load_task(model)


def make_context(model, precision):
    t = _task(model)
    return capi.Context(t.packed_model(), t.packed(), 0, precision)


def nodes_for(kind, n, nu, seed):
    """[n][P * nu], candidate c's spline flattened as the device stores it (parameter j = node * nu + actuator)"""
    return sc.NODE_SETS[kind](n, P * nu, seed)


def rollout_plain(ctx, model, nodes):
    state, mocap = STATE[model]
    ctx.set_state(state, 0.0, mocap)
    ctx.rollout_splines(H, capi.SPLINE_CUBIC, TIMES, nodes.reshape(-1, P, ctx.nu))


def set_fleet(ctx, model, E):
    state, mocap = STATE[model]
    ctx.set_states(np.tile(state, (E, 1)) + 0.01 * np.arange(E)[:, None], np.zeros(E), None if mocap is None else np.tile(mocap, (E, 1)))


def rollout_fleet(ctx, model, E, nodes):
    """nodes [E * n][P * nu], environment-major"""
    set_fleet(ctx, model, E)
    ctx.rollout_splines_batched(H, capi.SPLINE_CUBIC, np.tile(TIMES, (E, 1)), nodes.reshape(E, -1, P, ctx.nu), num_envs=E)


def failure_of(ctx, cand):
    r, f = C.c_double(), np.zeros(1, np.int32)
    ctx._chk(capi.lib().mjpcx_get_return_at(ctx.handle, int(cand), C.byref(r), as_i32p(f)))
    return r.value, int(f[0])


def assert_nodes_on_device(ctx, dev, candidates):
    for c in candidates:
        assert np.array_equal(ctx.fetch_spline(c).reshape(-1), dev[c]), c


def nan_last(r):
    nan = np.isnan(r)
    return not nan.any() or bool(nan[int(np.argmax(nan)):].all())


def check_avg_return(avg, ret, elites, worst):
    """the elites' mean return: at mean_bound when they are all finite, else what IEEE addition makes of them"""
    r = ret[elites]
    n = len(elites)
    if np.all(np.isfinite(r)):
        ex = sc.exact_moments(np.zeros((ret.size, 0)), ret, elites)
        q = sc.ratio(avg, ex["ret_sum"] / n, sc.mean_bound(n, ex["ret_abs_sum"]))
        worst["avg_return"] = max(worst.get("avg_return", 0.0), q)
        assert q <= 1.0, (float(avg), n, q)
    elif np.isnan(r).any() or (np.isposinf(r).any() and np.isneginf(r).any()):
        assert np.isnan(avg), (avg, n)
    else:
        assert avg == (np.inf if np.isposinf(r).any() else -np.inf), (avg, n)


def check_moments(mean, var, dev, ret, elites, precision, worst):
    """mean and variance of ce_update_kernel (one environment: dev [n_env][np], local elites) against the exact moments"""
    n = len(elites)
    ex = sc.exact_moments(dev, ret, elites, mean=mean, precision=precision)
    for j in range(dev.shape[1]):
        q = sc.ratio(mean[j], ex["mean"][j], sc.mean_bound(n, ex["abs_sum"][j]))
        worst["mean"] = max(worst.get("mean", 0.0), q)
        assert q <= 1.0, ("mean", j, n, q)
        if n == 1:
            assert np.isnan(var[j])                 # 0 / 0, as the header says
            continue
        exact = ex["sq"][j] / (n - 1)               # about the mean the device reported
        q = sc.ratio(var[j], exact, sc.square_bound(n) * exact)
        worst["variance"] = max(worst.get("variance", 0.0), q)
        assert q <= 1.0, ("variance", j, n, float(var[j]), float(exact), q)


# ------------------------------------------------------------------------------------------------ plain selection
@pytest.mark.parametrize("N", sc.PLAIN_N)
@pytest.mark.parametrize("model,precision", CONFIGS, ids=IDS)
def test_topk_and_best_on_injected_returns(model, precision, N):
    ctx = make_context(model, precision)
    nodes = nodes_for("scaled", N, ctx.nu, seed=N)
    dev = sc.as_device(nodes, precision)
    rollout_plain(ctx, model, nodes)
    own, _ = ctx.returns()
    own_raw = ctx.failure_raw.copy()
    assert_nodes_on_device(ctx, dev, sorted({0, N // 2, N - 1}))
    cases = sc.plain_cases(N)
    for ci, case in enumerate(cases):
        ret, fail = case.ret, case.fail
        sc.inject(ctx, ret, fail)
        want = sc.order(ret)
        for rep in range(2 if ci < 3 else 1):       # a second call on the same buffers: the same bits
            for k in sorted({1, min(2, N), N}):
                idx, r = ctx.topk(k)
                assert np.array_equal(idx, want[:k]), (case.name, k, idx[:8], want[:8])
                assert sc.same_bits(r, ret[want[:k]]), (case.name, k)
                assert nan_last(r), (case.name, k)
            ref = (N - 1, 0, -1)[ci % 3]
            w, br, rr, sp = ctx.best(ref)
            assert w == want[0] == case.winner, (case.name, w, want[0])
            assert sc.same_bits(br, ret[w]), (case.name, br)
            assert np.array_equal(sp.reshape(-1), dev[w]), case.name
            if ref >= 0:
                assert sc.same_bits(rr, ret[ref]), (case.name, rr)
                assert failure_of(ctx, ref)[1] == fail[ref]
            else:
                assert np.isnan(rr)
        if case.nans == N:
            assert w == 0 and ctx.topk(1)[0][0] == 0
    # a real rollout overwrites the injection: the kernel's own returns again
    rollout_plain(ctx, model, nodes)
    again, _ = ctx.returns()
    assert sc.same_bits(again, own) and np.array_equal(ctx.failure_raw, own_raw)
    assert ctx.topk(1)[0][0] == sc.order(own)[0]
    ctx.close()


# ------------------------------------------------------------------------------------------------ segmented selection
def _skips(round_cases, n_env):
    """-1, the would-be winner (of environment 0), a NaN candidate (of the first environment that has one but is not all NaN)"""
    out = [-1, round_cases[0].winner]
    for c in round_cases:
        if 0 < c.nans < n_env:
            out.append(int(np.flatnonzero(np.isnan(c.ret))[0]))
            break
    return out


@pytest.mark.parametrize("n_env", sc.SEG_N)
@pytest.mark.parametrize("model,precision", CONFIGS, ids=IDS)
def test_best_batched_and_ce_update_on_injected_returns(model, precision, n_env):
    E = sc.SEG_E
    ctx = make_context(model, precision)
    nodes = nodes_for("scaled", E * n_env, ctx.nu, seed=n_env)
    dev = sc.as_device(nodes, precision)
    rollout_fleet(ctx, model, E, nodes)
    own, _ = ctx.returns()
    assert_nodes_on_device(ctx, dev, [0, n_env, E * n_env - 1])
    worst = {}
    for ri, cases in enumerate(sc.segmented_rounds(n_env)):
        assert len({c.name for c in cases}) == E
        ret = np.concatenate([c.ret for c in cases])
        fail = np.concatenate([c.fail for c in cases])
        sc.inject(ctx, ret, fail)
        ref = (n_env - 1, 0, -1)[ri % 3]
        for rep in range(2 if ri < 2 else 1):
            idx, br, rr, sp = ctx.best_batched(E, ref)
            for e, c in enumerate(cases):
                where = (c.name, e)
                assert idx[e] == c.winner, where + (idx[e], c.winner)
                assert sc.same_bits(br[e], c.ret[c.winner]), where
                assert np.array_equal(sp[e].reshape(-1), dev[e * n_env + c.winner]), where
                assert sc.same_bits(rr[e], c.ret[ref]) if ref >= 0 else np.isnan(rr[e]), where
                if ref >= 0:
                    assert failure_of(ctx, e * n_env + ref)[1] == c.fail[ref]
        for skip in _skips(cases, n_env):
            want = [sc.order(c.ret, skip) for c in cases]
            for n_elite in sc.elite_counts(n_env, skip):
                idx, r, mean, var, avg = ctx.ce_update_batched(E, n_elite, skip)
                for e, c in enumerate(cases):
                    where = (c.name, e, skip, n_elite)
                    assert np.array_equal(idx[e], want[e][:n_elite]), where + (idx[e][:6], want[e][:6])
                    assert sc.same_bits(r[e], c.ret[want[e][:n_elite]]), where
                    assert nan_last(r[e]) and skip not in idx[e], where
                    if skip == -1 or n_elite <= 2:
                        check_avg_return(avg[e], c.ret, want[e][:n_elite], worst)
                if ri == 0 and skip == -1:          # (the moments have a test of their own: here one round, every elite count)
                    again = ctx.ce_update_batched(E, n_elite, skip)
                    for a, b in zip((idx, r, mean, var, avg), again):
                        assert np.array_equal(a, b, equal_nan=True) and (a.dtype != np.float64 or sc.same_bits(a, b))
                    for e, c in enumerate(cases):
                        check_moments(mean[e].reshape(-1), var[e].reshape(-1), dev[e * n_env:(e + 1) * n_env], c.ret, idx[e], precision, worst)
    print(f"{model} fp{precision} n_env={n_env}: worst error / bound {worst}")
    rollout_fleet(ctx, model, E, nodes)
    again, _ = ctx.returns()
    assert sc.same_bits(again, own)
    assert np.array_equal(ctx.best_batched(E, 0)[0], [sc.order(own[e * n_env:(e + 1) * n_env])[0] for e in range(E)])
    ctx.close()


# ------------------------------------------------------------------------------------------------ moments against the exact reference
MOMENT_N = 1088
MOMENT_ELITES = (1, 2, 255, 256, 257, 513, MOMENT_N - 1)


def _moment_returns(n):
    """three environments: a plain permutation (rank order is not index order), one whose elites reach into a NaN block (only 300
    numbers), one with failed rollouts and a tie"""
    a = sc.base(n, 31)
    b = sc.base(n, 32)
    b[np.random.default_rng(33).permutation(n)[:n - 300]] = np.nan
    c = sc.with_failed(n, 34, every=2)
    c[5] = c[700] = sc.LOW
    return [a, b, c]


@pytest.mark.parametrize("kind", sorted(sc.NODE_SETS))
@pytest.mark.parametrize("model,precision", CONFIGS, ids=IDS)
def test_elite_moments_and_ce_update_against_exact_moments(model, precision, kind):
    E, n = sc.SEG_E, MOMENT_N
    ctx = make_context(model, precision)
    nodes = nodes_for(kind, E * n, ctx.nu, seed=5)
    dev = sc.as_device(nodes, precision)
    if kind != "ill" or precision == 64:
        assert np.unique(dev[:, 0]).size > 50    # (the ill-conditioned set collapses to one value in float32: variance exactly 0)
    rollout_fleet(ctx, model, E, nodes)
    assert_nodes_on_device(ctx, dev, [1, n + 1, E * n - 2])
    rets = _moment_returns(n)
    ret = np.concatenate(rets)
    sc.inject(ctx, ret)
    worst = {}
    # ---- ce_update_kernel
    for n_elite in MOMENT_ELITES:
        idx, r, mean, var, avg = ctx.ce_update_batched(E, n_elite, -1)
        for e in range(E):
            want = sc.order(rets[e])[:n_elite]
            assert np.array_equal(idx[e], want) and sc.same_bits(r[e], rets[e][want]), (e, n_elite)
            check_avg_return(avg[e], rets[e], want, worst)
            check_moments(mean[e].reshape(-1), var[e].reshape(-1), dev[e * n:(e + 1) * n], rets[e], want, precision, worst)
            if n_elite > 300 and e == 1:
                assert np.isnan(avg[e]) and np.isfinite(mean[e]).all() and np.isfinite(var[e]).all()
    # ---- elite_moments_kernel, on its own: global candidates in an order of the test's choosing, the environment with numbers only
    mine = {}
    finite = np.concatenate([np.arange(n), 2 * n + np.arange(n)])
    for count in MOMENT_ELITES + (2 * n,):
        cand = np.random.default_rng(count).permutation(finite)[:count]
        s, sr = ctx.elite_moments(cand)
        s2, sr2 = ctx.elite_moments(cand)
        assert sc.same_bits(s, s2) and sc.same_bits(sr, sr2)
        ex = sc.exact_moments(dev, ret, cand, precision=precision)
        for j in range(dev.shape[1]):
            q = sc.ratio(s.reshape(-1)[j], ex["sum"][j], sc.sum_bound(count, ex["abs_sum"][j]))
            mine["sum"] = max(mine.get("sum", 0.0), q)
            assert q <= 1.0, ("sum", j, count, q)
        q = sc.ratio(sr, ex["ret_sum"], sc.sum_bound(count, ex["ret_abs_sum"]))
        mine["sum_return"] = max(mine.get("sum_return", 0.0), q)
        assert q <= 1.0, ("sum_return", count, q)
        m = s.reshape(-1) / count                    # the host's division (cross_entropy planner)
        sq, _ = ctx.elite_moments(cand, m)
        ex = sc.exact_moments(dev, ret, cand, mean=m, precision=precision)
        for j in range(dev.shape[1]):
            q = sc.ratio(sq.reshape(-1)[j], ex["sq"][j], sc.square_bound(count) * ex["sq"][j])
            mine["squares"] = max(mine.get("squares", 0.0), q)
            assert q <= 1.0, ("squares", j, count, float(sq.reshape(-1)[j]), float(ex["sq"][j]), q)
    # a NaN return among the candidates reaches the return sum and nothing else
    s, sr = ctx.elite_moments([n, n + 1, 3])
    assert np.isnan(sr) == bool(np.isnan(ret[[n, n + 1, 3]]).any()) and np.isfinite(s).all()
    print(f"{model} fp{precision} {kind}: ce_update worst error / bound {worst}; elite_moments {mine}")
    ctx.close()


# ------------------------------------------------------------------------------------------------ the 8192 / 8256 edge
def _edge_returns(n):
    """two environments, different: ties and NaN across the 1023/1024 stride and at both ends"""
    a = sc.with_tie(n, 41, 1023, 1024)
    a[[0, 64, n - 1]] = np.nan
    a[[15, 16]] = sc.LOW
    b = sc.with_nan(n, 42, [1, 63, 1023, 4096, n - 2])
    b[n - 1] = b[255] = -np.inf
    b[::5] = sc.FAILED
    return [a, b]


@pytest.mark.parametrize("n_env", [sc.LDS_LAST, sc.SCRATCH_FIRST])
@pytest.mark.parametrize("model,precision", [("Cartpole", 64), ("Particle", 32)], ids=["Cartpole64", "Particle32"])
def test_ce_update_on_both_sides_of_the_lds_limit(model, precision, n_env):
    """n_env = 8192 is the last size sorted in LDS, 8256 the first sorted in the global slab (n2 = 16384): environment 1's slab
    starts at 1.5 n2 doubles, and what it gives in a fleet of two is what it gives alone"""
    E = 2
    ctx = make_context(model, precision)
    nodes = nodes_for("scaled", E * n_env, ctx.nu, seed=n_env)
    dev = sc.as_device(nodes, precision)
    rollout_fleet(ctx, model, E, nodes)
    rets = _edge_returns(n_env)
    sc.inject(ctx, np.concatenate(rets))
    worst, fleet = {}, {}
    for n_elite, skip in ((2, -1), (513, 1023), (n_env - 1, -1), (n_env - 1, 15)):
        out = ctx.ce_update_batched(E, n_elite, skip)
        twice = ctx.ce_update_batched(E, n_elite, skip)
        for a, b in zip(out, twice):
            assert np.array_equal(a, b, equal_nan=True) and (a.dtype != np.float64 or sc.same_bits(a, b))
        fleet[(n_elite, skip)] = out
        idx, r, mean, var, avg = out
        for e in range(E):
            want = sc.order(rets[e], skip)[:n_elite]
            assert np.array_equal(idx[e], want), (e, n_elite, skip, idx[e][:6], want[:6])
            assert sc.same_bits(r[e], rets[e][want]) and nan_last(r[e]), (e, n_elite, skip)
            check_avg_return(avg[e], rets[e], want, worst)
            if skip == -1:
                check_moments(mean[e].reshape(-1), var[e].reshape(-1), dev[e * n_env:(e + 1) * n_env], rets[e], want, precision, worst)
    # environment 1 alone, E = 1
    rollout_fleet(ctx, model, 1, nodes[n_env:])
    sc.inject(ctx, rets[1])
    for (n_elite, skip), out in fleet.items():
        alone = ctx.ce_update_batched(1, n_elite, skip)
        for a, b in zip(out, alone):
            assert np.array_equal(a[1], b[0], equal_nan=True) and (a.dtype != np.float64 or sc.same_bits(a[1], b[0])), (n_elite, skip)
    print(f"{model} fp{precision} n_env={n_env}: worst error / bound {worst}")
    ctx.close()


@pytest.mark.parametrize("n_src", [64, sc.SCRATCH_FIRST])
@pytest.mark.parametrize("model,precision", [("Cartpole", 64), ("Particle", 32)], ids=["Cartpole64", "Particle32"])
def test_robust_step_selects_by_the_contract(model, precision, n_src):
    """the select side of mjpcx_robust_step_batched (robust_select_kernel, in LDS at 64 candidates, in the global slab at 8256) on
    injected source returns with ties and NaN: k = 5, R = 1, no force noise"""
    E, k = 2, 5
    src, ctx = make_context(model, precision), make_context(model, precision)
    nodes = nodes_for("scaled", E * n_src, src.nu, seed=n_src + 1)
    dev = sc.as_device(nodes, precision)
    rollout_fleet(src, model, E, nodes)
    a = sc.with_tie(n_src, 51, 15, 16)              # a tie for rank 0 across a DPP row
    a[[0, 63]] = np.nan
    a[40] = a[7] = 1.5                              # and one for rank 2
    b = sc.all_nan(n_src)                           # three numbers: ranks 3 and 4 are NaN, lowest index first
    b[[n_src - 1, 33, 20]] = [2.0, 2.0, -np.inf]
    rets = [a, b]
    sc.inject(src, np.concatenate(rets))
    set_fleet(ctx, model, E)
    outs = [ctx.robust_step_batched(src, E, k, 1, H, capi.SPLINE_CUBIC, np.tile(TIMES, (E, 1)), 0.0, 1.0) for _ in range(2)]
    for key in outs[0]:
        assert np.array_equal(outs[0][key], outs[1][key], equal_nan=True), key
    out = outs[0]
    for e in range(E):
        want = sc.order(rets[e])[:k]
        assert np.array_equal(out["candidate"][e], want), (e, out["candidate"][e], want)
        assert sc.same_bits(out["candidate_return"][e], rets[e][want]), e
        assert 0 <= out["best"][e] < k
        assert np.array_equal(out["spline"][e].reshape(-1), dev[e * n_src + want[out["best"][e]]]), e
    assert list(out["candidate"][0][:4]) == [15, 16, 7, 40] and list(out["candidate"][1]) == [20, 33, n_src - 1, 0, 1]
    # the source is left as injected; this context holds the noisy rollout of the chosen splines (R = 1: rollout j is rank j)
    back, _ = src.returns()
    assert sc.same_bits(back, np.concatenate(rets))
    for e in range(E):
        for rank in range(k):
            assert np.array_equal(ctx.fetch_spline(e * 64 + rank).reshape(-1), dev[e * n_src + out["candidate"][e][rank]]), (e, rank)
    src.close()
    ctx.close()
