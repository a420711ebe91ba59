"""-m gpu: cost_derivatives_kernel (csrc/ilqg_dense.h) against the exact answers of tests/cost_cases.py, on residuals, C and D the
test chooses (mjpcx_cost_derivatives takes them from the host: no rollout is launched).

   every finite step: every entry of cx, cu, cxx, cxu, cuu within the derived bound of the mpmath answer (the bound: cost_cases.py,
       four times the worst case of a forward-error analysis in u = 2^-53), cxx and cuu symmetric to the same bound
   every other step (a norm, or exp(risk c), leaves the finite numbers in the reference's own double arithmetic): the set of
       non-finite entries equals the oracle's
   |risk| < 1e-6: the bits of the risk = 0 call
   Particle (ndx 4, nu 2, terms [2, 2]): every norm type but the null norm on either term (the null norm is for terms of ONE residual,
       task.cc:214; it runs on the A1's 1-wide terms and on the Cartpole's), every point of cost_cases.points(), T in {1, 2, 5}, every
       risk of cost_cases.RISKS on term 0 and {0, 0.7} on term 1, risk * c = 11 on the heavy case, an identity block for C
   QuadrupedFlat's 42 residuals (ndx 36, nu 12) under other term boundaries: a 32-wide term under L22 and under L2, 32 terms with the
       null norm on seven of them, [31, 11], [16, 16, 10], the task's own nine terms; 33 terms and a 33-wide term are refused with
       MJPCX_EUNSUPPORTED and make_cost_spec's message
   Cartpole (nu 1): its own norms, and the null norm on two of its terms, under every risk
   a second call with a smaller T and other data is right and leaves the tail of the caller's larger arrays untouched

Worst error / bound over the file, measured on an MI355X: DESIGN.md 4.3."""
import numpy as np
import pytest

import cost_cases as cc
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.cstructs import as_f64p
from mujoco_mpc_amd.task import load_task
from oracle import pyoracle

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -2


@pytest.fixture(scope="module")
def particle():
    return load_task("Particle")


@pytest.fixture(scope="module")
def a1():
    task = load_task("QuadrupedFlat")
    task.transition(0.0)
    return task


def context(task, spec):
    t2 = cc.task_with(task, spec)
    return capi.Context(t2.packed_model(), t2.packed(), 0, 64), t2


def launch(ctx, run, risk):
    ctx.set_task_params(run.spec.weight, run.spec.norm_parameter() or None, None, float(risk))
    return ctx.cost_derivatives(run.r, run.C, run.D)


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a, b))


def check(task, ctx, run, risks, report):
    """every assertion of the module docstring for one Run under each risk -> worst error / bound"""
    worst, neutral = 0.0, None
    for risk in risks:
        got = launch(ctx, run, risk)
        worst = max(worst, cc.check_run(run, risk, got))
        rest = [t for t in range(run.T) if not run.finite(t, risk)]
        if rest:
            ref = pyoracle.cost_derivatives(cc.task_with(task, run.with_risk(risk)).packed(), run.r, run.C, run.D)
            for t in rest:
                for name, g, o in zip(cc.NAMES, got, ref):
                    assert np.array_equal(np.isfinite(g[t]), np.isfinite(o[t])), (run.name, risk, t, name, g[t], o[t])
        if risk == 0.0:
            neutral = got
        elif abs(risk) < cc.RISK_TOL:
            assert neutral is not None and same_bits(got, neutral), (run.name, risk)
    report.append((worst, run.name))
    return worst


def conclude(report, what):
    worst = max(report)
    print(f"\ncost_derivatives_kernel, {what}: worst error / bound {worst[0]:.4f} at {worst[1]} ({len(report)} runs)")
    assert worst[0] < 1.0, worst


@pytest.mark.parametrize("placement", [0, 1])
@pytest.mark.parametrize("t", cc.VALUE_NORMS)
def test_particle_every_point_of_a_norm(particle, t, placement):
    runs = [run for run in cc.particle_runs(placement) if run.spec.norm[placement] == t]
    assert runs
    ctx, _ = context(particle, runs[0].spec)
    assert (ctx.nv, ctx.nu, ctx.num_residual) == (2, 2, 4)
    report = []
    for run in runs:
        check(particle, ctx, run, cc.RISKS if placement == 0 else (0.0, 0.7), report)
    ctx.close()
    conclude(report, f"Particle, norm {t} on term {placement}")


def test_particle_large_risk_and_identity_block(particle):
    heavy, ident = cc.heavy_run(), cc.identity_run()
    ctx, _ = context(particle, heavy.spec)
    report = []
    check(particle, ctx, heavy, (0.0, cc.RISK_LARGE, -cc.RISK_LARGE), report)
    check(particle, ctx, ident, (0.0, 9e-7, -0.7), report)
    got = launch(ctx, ident, 0.0)                       # by hand: C = I and quadratic norms give cx = w r / T, cxx = diag(w / T)
    w = np.repeat(np.array(cc.WEIGHTS) / ident.T, 2)
    assert np.allclose(got[0], w * ident.r, rtol=4e-16, atol=0) and np.allclose(got[2], np.stack([np.diag(w)] * 2), rtol=4e-16, atol=0)
    ctx.close()
    conclude(report, "Particle, risk * c = 11 and C = I")


def test_second_call_with_a_smaller_T_leaves_the_tail(particle):
    """the larger call's results stay in the caller's arrays beyond the T steps of the smaller call, which is right on its own data"""
    runs = [run for run in cc.particle_runs(0) if run.spec.norm[0] == 6]
    big = next(run for run in runs if run.T == 5)
    small = next(run for run in runs if run.T == 2 and all(run.finite(t) for t in range(2)))
    ctx, _ = context(particle, big.spec)
    out = [np.array(a) for a in launch(ctx, big, 0.7)]
    before = [a.copy() for a in out]
    ctx.set_task_params(small.spec.weight, small.spec.norm_parameter(), None, -0.7)
    ctx._chk(capi.lib().mjpcx_cost_derivatives(ctx.handle, small.T, as_f64p(np.ascontiguousarray(small.r).reshape(-1)),
                                               as_f64p(np.ascontiguousarray(small.C).reshape(-1)), as_f64p(np.ascontiguousarray(small.D).reshape(-1)),
                                               *[as_f64p(a) for a in out]))
    for a, b in zip(out, before):
        assert same_bits([a[small.T:]], [b[small.T:]]) and not np.array_equal(a[:small.T], b[:small.T])
    assert cc.check_run(small, -0.7, [a[:small.T] for a in out]) < 1.0
    ctx.close()


@pytest.mark.parametrize("name", list(cc.LAYOUTS) + ["own"])
def test_a1_residuals_under_other_term_boundaries(a1, name):
    spec = cc.spec_of_task(a1) if name == "own" else cc.LAYOUTS[name]
    ctx, task = context(a1, spec)
    assert (2 * ctx.nv, ctx.nu, ctx.num_residual) == (36, 12, 42)
    run = cc.layout_run(spec, 3 if name == "own" else 2, 36, 12, seed=len(name))
    report = []
    check(a1, ctx, run, (0.0, 0.7), report)
    ctx.close()
    conclude(report, f"A1 residuals as {name}")


@pytest.mark.parametrize("name", list(cc.REFUSED))
def test_a1_layouts_the_kernel_has_no_room_for_are_refused(a1, name):
    spec, message = cc.REFUSED[name]
    ctx, _ = context(a1, spec)
    run = cc.layout_run(spec, 2, 36, 12, seed=1)
    with pytest.raises(capi.MjpcxError) as err:
        ctx.cost_derivatives(run.r, run.C, run.D)
    assert err.value.code == EUNSUPPORTED and message in str(err.value)
    ctx.close()


@pytest.mark.parametrize("null_terms", [(), (0, 3)])
def test_cartpole_one_control(null_terms):
    """nu = 1: the strides of cu, cxu, cuu; the Cartpole's own norms (smooth-abs, smooth-abs, quadratic, quadratic), then the null norm on
    two of its 1-wide terms"""
    task = load_task("Cartpole")
    spec = cc.spec_of_task(task)
    for k in null_terms:
        spec.norm[k], spec.par[k] = -1, (0.0, 0.0)
    ctx, _ = context(task, spec)
    assert (2 * ctx.nv, ctx.nu, ctx.num_residual) == (4, 1, 4)
    rng = np.random.default_rng(9)
    run = cc.Run("cartpole", spec, 0.4 * cc.dense(rng, (3, 4)), cc.dense(rng, (3, 4, 4)), cc.dense(rng, (3, 4, 1)), [])
    report = []
    check(task, ctx, run, cc.RISKS + (0.05, -0.05), report)
    ctx.close()
    conclude(report, f"Cartpole, null norm on {null_terms}")
