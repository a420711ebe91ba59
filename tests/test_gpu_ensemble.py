"""-m gpu: an ensemble -- ONE set of candidates under M hypotheses (mjpcx_rollout_noise_ensemble), scored across them (mjpcx_ensemble_best,
ensemble_best_kernel) -- and GpuEnsembleSamplingPlanner on the device.

   1 the score on INJECTED returns (tests/test_gpu_selection.py's contexts: Cartpole and Particle, fp64 and fp32, H = 2, P = 3), M in
     {1, 2, 3, 8, 32} x n in {64, 192, 1088} x tail in {1, 2, M}: index, best_score, ref_score, member_returns, every score and the spline
     against the definition as a Python loop (ensemble_oracle_backend.ensemble_scores), bit for bit -- a NaN is a NaN whatever its payload
     (the device's inf - inf and numpy's differ in the sign bit); M = 1 is mjpcx_best; the refusals
   2 the launch on every kernel family of tests/test_gpu_batch_models.py and on a Cartpole lane context: hypothesis h has the bits of the
     plain mjpcx_rollout_noise with the SAME seed on a context created on model h; mjpcx_rollout_noise_batched beside it still draws seed + 1
   3 the planner against the oracle backend on the cases chosen in tests/test_ensemble_planner.py: the same winner, scores and member returns
     at the quad kernel's 1e-9 (1 + |x|) and at the fp32 limb kernel's 2e-3 (1 + |x|); cross-entropy noise with the one shared variance
   4 the order of calls"""
import numpy as np
import pytest

import selection_cases as sc
import test_ensemble_planner as cpu
import test_gpu_selection as sel
from ensemble_oracle_backend import ensemble_argmin, ensemble_scores
from mujoco_mpc_amd import capi
from test_gpu_batch import context, err, everything
from test_gpu_batch_models import ALL, FAMILIES, fleet, refused

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED, ESTATE = -1, -2, -5


def same(a, b):
    """the same bits, or NaN on both sides"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------- 1: the score
def score_cases(M, n, seed):
    """(name, R of M x n): returns between 1 and 10 with the structure the name says laid over them"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(1.0, 10.0, (M, n))
    spots = sorted({0, 63, n - 1} | ({64} if n > 64 else set()) | ({1023, 1024} if n > 1024 else set()))
    out = [("random", base.copy())]
    for i in spots:                                         # the minimum score at and across the lanes' and the workgroup's edges
        R = base.copy()
        R[:, i] = rng.uniform(0.1, 0.5, M)
        out.append((f"minimum at {i}", R))
    pairs = [(0, n - 1)] + ([(63, 64)] if n > 64 else []) + ([(1023, 1024)] if n > 1024 else [])
    for a, b in pairs:                                      # tied scores: the same M returns in another order of h; the lower index wins
        R = base.copy()
        R[:, a] = rng.uniform(0.1, 0.5, M)
        R[:, b] = R[::-1, a]
        out.append((f"tie {a}/{b}", R))
    R = base.copy()                                         # a NaN in one hypothesis only: the would-be winner's score is NaN and it loses
    R[:, 5] = 0.01
    R[M - 1, 5] = np.nan
    R[0, n - 1] = -np.nan
    out.append(("NaN in one hypothesis", R))
    R = base.copy()                                         # infinities: -inf wins the mean, not the worst case; +inf with -inf is NaN
    R[M // 2, 7] = -np.inf
    R[0, 9] = np.inf
    R[0, 11], R[M - 1, 11] = np.inf, -np.inf
    out.append(("infinities", R))
    R = base.copy()                                         # signed zeros among a candidate's returns: -0.0 only where all M are -0.0
    R[:, 3] = 0.0
    R[::2, 3] = -0.0
    R[:, 2] = -0.0
    R[:, 40] = 0.0
    out.append(("signed zeros", R))
    R = base.copy()                                         # the 1e6 of failed rollouts, in some hypotheses and in all of one candidate's
    R[rng.integers(0, M, n // 4), rng.integers(0, n, n // 4)] = 1e6
    R[:, 1] = 1e6
    out.append(("failed rollouts", R))
    out.append(("all NaN", np.full((M, n), np.nan)))
    return out


@pytest.mark.parametrize("M", [1, 2, 3, 8, 32])
@pytest.mark.parametrize("model,precision", sel.CONFIGS, ids=sel.IDS)
def test_score_and_argmin_on_injected_returns(model, precision, M):
    ctx = sel.make_context(model, precision)
    checked = 0
    for n in (64, 192, 1088):
        nodes = sel.nodes_for("scaled", M * n, ctx.nu, seed=M + n)
        dev = sc.as_device(nodes, precision)
        sel.rollout_fleet(ctx, model, M, nodes)
        for ci, (name, R) in enumerate(score_cases(M, n, seed=7 * M + n)):
            sc.inject(ctx, R.reshape(-1))
            for tail in sorted({1, min(2, M), M}):
                want = ensemble_scores(R, tail)
                w = ensemble_argmin(want)
                ref = (n - 1, 0, -1)[(ci + tail) % 3]
                where = (name, M, n, tail)
                for rep in range(2 if ci == 0 else 1):      # a second call on the same buffers: the same bits
                    idx, best, ref_score, members, spline, scores = ctx.ensemble_best(M, tail, ref, with_scores=True)
                    assert same(scores, want), (where, np.flatnonzero(scores != want)[:8])
                    assert idx == w, (where, idx, w)
                    assert same(best, want[w]) and same(members, R[:, w]), where
                    assert same(ref_score, want[ref] if ref >= 0 else np.nan), where
                    assert np.array_equal(spline.reshape(-1), dev[w]), where          # hypothesis 0's copy
                if ci == 0:                                  # without the scores: the same answers
                    i2, b2, r2, m2, s2, none = ctx.ensemble_best(M, tail, ref)
                    assert none is None and i2 == idx and same(b2, best) and same(r2, ref_score) and same(m2, members) and np.array_equal(s2, spline), where
                if M == 1:                                   # one hypothesis: mjpcx_best
                    bi, br, _, bsp = ctx.best(-1)
                    assert bi == idx and same(br, best) and np.array_equal(bsp, spline), where
                checked += 1
            if name == "NaN in one hypothesis" and M > 1:
                assert np.isnan(want[5]) and w != 5
    print(f"{model} fp{precision}, M = {M}: {checked} (case, n, tail) combinations, all equal to the Python loop")
    ctx.close()


@pytest.mark.parametrize("model,precision", sel.CONFIGS[:2], ids=sel.IDS[:2])
def test_selection_refused(model, precision):
    ctx = sel.make_context(model, precision)
    M, n = 3, 64
    sel.rollout_fleet(ctx, model, M, sel.nodes_for("scaled", M * n, ctx.nu, seed=1))
    for tail in (0, M + 1):
        refused(lambda: ctx.ensemble_best(M, tail), EINVAL, "tail")
    for ref in (-2, n):
        refused(lambda: ctx.ensemble_best(M, 1, ref), EINVAL, "ref_candidate")
    refused(lambda: ctx.ensemble_best(2, 1), EINVAL, "not a batched one of 2")
    sel.rollout_fleet(ctx, model, 33, sel.nodes_for("scaled", 33 * 64, ctx.nu, seed=2))
    refused(lambda: ctx.ensemble_best(33, 1), EUNSUPPORTED, "33 hypotheses")
    sel.rollout_plain(ctx, model, sel.nodes_for("scaled", 192, ctx.nu, seed=3))
    refused(lambda: ctx.ensemble_best(3, 1), EINVAL, "not a batched one")
    ctx.close()


# ------------------------------------------------------------------------------------------------- 2: the launch
@pytest.mark.parametrize("name", list(FAMILIES))
def test_hypothesis_h_is_the_plain_call_with_the_same_seed_on_model_h(name):
    f = fleet(name)
    M, n = f.E, f.n
    ctx = f.make_context()
    f.push(ctx)
    f.assert_models_decide_the_cost(ctx)                     # one shared spline: the hypotheses' returns differ pairwise
    ctx.rollout_noise_ensemble(n, f.H, capi.SPLINE_CUBIC, f.times[0], f.nominal[0], f.noise(), num_hypotheses=M)
    assert ctx.N == M * n
    got = everything(ctx)
    raw = ctx.failure_raw.copy()
    for i in (0, 1, n - 1):
        for h in range(1, M):
            assert np.array_equal(ctx.fetch_spline(h * n + i), ctx.fetch_spline(i)), (name, h, i)
    shared = ctx.fetch_spline(n + 1)
    for h in range(M):
        one_ctx = f.make_context(h)
        f.plain(one_ctx)
        f.run_plain(one_ctx, "noise", 0)                     # (environment number 0: the seed itself, the one row of times and nominal)
        one = everything(one_ctx)
        assert np.array_equal(raw[h * n:(h + 1) * n], one_ctx.failure_raw), (name, f.labels[h], "failure words")
        one_ctx.close()
        for k in ALL:
            assert np.array_equal(got[k][h * n:(h + 1) * n], one[k], equal_nan=True), (name, f.labels[h], k)
    if "quad" in name or "limb" in name:
        assert ctx.quad_stats()["handed_on"] == 0
    # ---- the per-hypothesis argmin and the score work on it
    idx, best, _, _ = ctx.best_batched(M, 0)
    R = got["total_return"].reshape(M, n)
    assert np.array_equal(idx, [ensemble_argmin(R[h]) for h in range(M)])
    w, score, _, members, _, scores = ctx.ensemble_best(M, M, 0, with_scores=True)
    assert same(scores, ensemble_scores(R, M)) and w == ensemble_argmin(scores) and same(members, R[:, w])
    # ---- the old behaviour beside the new: environment 1 of mjpcx_rollout_noise_batched draws seed + 1
    if name == "quad":                                       # the switch is ignored: everything was rolled out (and it is not left behind)
        ctx.set_pruning_batched(True, M)
        ctx.rollout_noise_ensemble(n, f.H, capi.SPLINE_CUBIC, f.times[0], f.nominal[0], f.noise(), num_hypotheses=M)
        assert np.array_equal(ctx.returns()[0], got["total_return"]) and not ctx.prune_stats_batched(M)["retired"].any()
        ctx.ensemble_best(M, 1)
        f.run(ctx, "noise")                                  # a pruned batched launch: its stored returns are no returns
        refused(lambda: ctx.ensemble_best(M, 1), ESTATE, "pruned")
        ctx.set_pruning_batched(False)
    f.run(ctx, "noise")
    ret, _ = ctx.returns()
    assert np.array_equal(ret[:n], got["total_return"][:n])                  # (environment 0: seed + 0)
    assert not np.array_equal(ctx.fetch_spline(n + 1), shared) and not np.array_equal(ret[n:2 * n], got["total_return"][n:2 * n])
    ctx.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_hypotheses_about_the_state_on_a_lane_context(precision):
    model, M, n = "Cartpole", 3, 192
    ctx = sel.make_context(model, precision)
    sel.set_fleet(ctx, model, M)
    nominal = np.array([[0.1], [-0.2], [0.05]])
    ns = capi.make_noise_spec(seed=5, iteration=1, mode=capi.NOISE_SAMPLING, std0=0.3)
    ctx.rollout_noise_ensemble(n, sel.H, capi.SPLINE_CUBIC, sel.TIMES, nominal, ns, num_hypotheses=M)
    got = everything(ctx)
    state, _ = sel.STATE[model]
    one = sel.make_context(model, precision)
    for h in range(M):
        one.set_state(np.asarray(state) + 0.01 * h, 0.0)
        one.rollout_noise(n, sel.H, capi.SPLINE_CUBIC, sel.TIMES, nominal, ns)
        ref = everything(one)
        for k in ref:
            assert np.array_equal(got[k][h * n:(h + 1) * n], ref[k], equal_nan=True), (h, k)
    assert len({float(got["total_return"][h * n]) for h in range(M)}) == M
    one.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------- 3: the planner
def test_planner_on_the_quad_kernel_equals_the_oracle_backend():
    want = cpu.case_on_the_oracle()
    made = []

    def factory(t):
        made.append(context(t.packed_model(), t.packed(), 64, {"MJPCX_QUAD_MIN_N": "0"}))
        return made[-1]
    ens, got = cpu.run_case(factory)
    assert "rollout_quad_kernel" in ens.ctx.kernel_name
    for step, (g, w) in enumerate(zip(got, want)):
        worst = max(err(g[k], w[k]) for k in ("best_score", "nominal_score", "member_returns", "scores"))
        print(f"step {step}: winner {g['winner']} (oracle {w['winner']}), worst error of the scores and member returns {worst:.3e}")
        assert g["winner"] == w["winner"], step
        assert worst <= cpu.QUAD_BOUND, (step, worst)
    for c in made:
        c.close()


def test_planner_on_the_limb_kernel_fp32_equals_the_oracle_backend():
    """tests/test_ensemble_planner.py's LIMB_CASE, whose best score is clear of the second best by more than twice the fp32 bound in both plan
    steps (asserted there on the oracle): the same winner, and scores and member returns at 2e-3 (1 + |x|)"""
    want = cpu.case_on_the_oracle(cpu.LIMB_CASE)
    made = []

    def factory(t):
        made.append(context(t.packed_model(), t.packed(), 32, {"MJPCX_LIMB_MIN_N": "0"}))
        return made[-1]
    ens, got = cpu.run_case(factory, precision=32, case=cpu.LIMB_CASE)
    assert "rollout_limb_kernel" in ens.ctx.kernel_name and ens.ctx.quad_stats()["handed_on"] == 0
    for step, (g, w) in enumerate(zip(got, want)):
        worst = max(err(g[k], w[k]) for k in ("best_score", "nominal_score", "member_returns", "scores"))
        print(f"step {step}: winner {g['winner']} (oracle {w['winner']}), worst error of the scores and member returns {worst:.3e}")
        assert g["winner"] == w["winner"], step
        assert worst <= cpu.LIMB32_BOUND, (step, worst)
    for c in made:
        c.close()


# ------------------------------------------------------------------------------------------------- 2b: cross-entropy noise, one variance for all
@pytest.mark.parametrize("name", ["quad", "tree_a1", "limb32"])
def test_cross_entropy_noise_with_the_shared_variance(name):
    """MJPCX_NOISE_CROSS_ENTROPY: noise->param_variance is every hypothesis's -- hypothesis h is the plain cross-entropy call with the same seed
    and that variance on a context created on model h"""
    f = fleet(name, ("base", "payload", "ice"), n=min(FAMILIES[name][2], 256))
    M, n = f.E, f.n
    var = f.variance()[1]
    spec = lambda: f.noise(0, capi.NOISE_CROSS_ENTROPY, var)
    ctx = f.make_context()
    f.push(ctx)
    ctx.rollout_noise_ensemble(n, f.H, capi.SPLINE_CUBIC, f.times[0], f.nominal[0], spec(), num_hypotheses=M)
    got = everything(ctx)
    ctx.close()
    assert not np.array_equal(got["actions"][1], got["actions"][2])           # (noise was drawn)
    for h in range(M):
        one = f.make_context(h)
        f.plain(one)
        one.rollout_noise(n, f.H, capi.SPLINE_CUBIC, f.times[0], f.nominal[0], spec())
        ref = everything(one)
        one.close()
        for k in ALL:
            assert np.array_equal(got[k][h * n:(h + 1) * n], ref[k], equal_nan=True), (name, f.labels[h], k)
    assert len({float(got["total_return"][h * n + 1]) for h in range(M)}) == M   # (one spline, three models)


# ------------------------------------------------------------------------------------------------- 4: the order of calls
def test_order_of_calls():
    f = fleet("tree_a1")
    M, n = f.E, f.n
    ctx = f.make_context()
    f.plain(ctx)
    f.run_plain(ctx, "noise", 0)
    before = ctx.returns()[0].copy()
    launch = lambda m: ctx.rollout_noise_ensemble(n, f.H, capi.SPLINE_CUBIC, f.times[0], f.nominal[0], f.noise(), num_hypotheses=m)
    refused(lambda: launch(M), EINVAL, "before mjpcx_set_states")
    f.push(ctx)                                              # four states, four models
    refused(lambda: launch(3), EINVAL, "3 environments", "set_states of 4")
    f.push(ctx, [0, 1, 2], models=False)                     # three states, still four models
    refused(lambda: launch(3), EINVAL, "3 environments", "4 models")
    refused(lambda: ctx.rollout_noise_ensemble(100, f.H, capi.SPLINE_CUBIC, f.times[0], f.nominal[0], f.noise(), num_hypotheses=3), EINVAL, "multiple of 64")
    ctx.N, ctx.n_per_env = before.size, 0                    # (the wrapper's own bookkeeping, which a refused call does not touch either)
    assert np.array_equal(ctx.returns()[0], before)          # the context keeps its last rollout
    refused(lambda: ctx.ensemble_best(3, 1), EINVAL, "not a batched one")
    ctx.close()
