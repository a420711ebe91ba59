"""Test-only stand-in for capi.Context.ilqg_step_batched on the CPU oracle, over batch_ilqg_oracle_backend.py's BatchILQGOracleContext:
environment e's middle of an iLQG iteration is the oracle's plain transition_fd at the evaluated steps with that environment's mocap
pose, the skip interpolation of planners.model_derivatives, the zeroed last step, the oracle's cost derivatives and the Python retry
loop of GpuILQGPlanner._iteration_before_rollouts over the oracle's backward pass -- the calls a fleet planner's sequential middle makes,
one environment after the other. `fail_nominal` marks environments whose nominal rollouts are all reported as failed (a test's way to
a member without a device nominal, nothing is provoked). Never used by the product."""
import numpy as np

from batch_gradient_oracle_backend import interpolate
from batch_ilqg_oracle_backend import BatchILQGOracleContext


def retry_loop(backward_pass, mu, rate, factor, min_reg, max_reg, max_iter):
    """ilqg/planner.cc:429-520 with ScaleRegularization (backward_pass.cc:327-340) over `backward_pass(mu) -> dict with "ok"`:
    the last sweep's dict, mu, rate and the number of scalings"""
    ok, retries, out = False, 0, None
    while retries < max_iter and not ok:
        out = backward_pass(mu)
        ok = bool(out["ok"])
        if not ok and mu <= max_reg:
            rate = max(rate * factor, factor) if factor > 1 else min(rate * factor, factor)
            mu = min(max(mu * rate, min_reg), max_reg)
            retries += 1
        elif not ok:
            break
    return out, mu, rate, retries


class BatchILQGStepOracleContext(BatchILQGOracleContext):
    def __init__(self, task, threads=2, differentiable=False, fail_nominal=()):
        super().__init__(task, threads=threads, differentiable=differentiable)
        self.fail_nominal = set(fail_nominal)
        self.step_calls = []                                   # (candidates, status) of every ilqg_step_batched

    def rollout_feedback_batched(self, horizon, mode, *args, **kw):
        super().rollout_feedback_batched(horizon, mode, *args, **kw)
        if mode == 1:                                          # the nominal phase
            n = self.n_per_env
            for e in self.fail_nominal:
                self.out["failure"][e * n:(e + 1) * n] = 1

    def ilqg_step_batched(self, candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor, min_reg, max_reg, max_iter,
                          with_matrices=False, num_envs=None):
        cand = [int(c) for c in candidate]
        E, n, m, ndx = len(cand), self.n_per_env, self.nu, 2 * self.pm.struct.nv
        assert E == self.E and E * n == self.N and 2 <= T <= self.H and 1 <= max_iter <= 64
        ev = [int(i) for i in evaluate]
        limits = np.asarray(self.task.model.actuator_ctrlrange, float).reshape(-1, 2)
        out = dict(K=np.zeros((E, T, m, ndx)), du=np.zeros((E, T, m)), dV=np.zeros((E, 2)), status=np.full(E, -1, np.int32), mu=np.zeros(E),
                   rate=np.zeros(E), retries=np.zeros(E, np.int32), nominal_return=np.zeros(E))
        if with_matrices:
            shapes = dict(A=(ndx, ndx), B=(ndx, m), cx=(ndx,), cu=(m,), cxx=(ndx, ndx), cxu=(ndx, m), cuu=(m, m), Vx=(ndx,), Vxx=(ndx, ndx))
            out.update({k: np.zeros((E, T) + sh) for k, sh in shapes.items()})
        for e in range(E):
            if cand[e] < 0:
                continue
            assert cand[e] < n
            tr = self.fetch_trajectory(e * n + cand[e])
            self.set_state(self.env_states[e], self.env_times[e], None if self.env_mocap is None else self.env_mocap[e])
            A, B, C, D = interpolate(ev, T, self.transition_fd(tr.times[ev], tr.states[ev], tr.actions[ev], eps, centered))
            A, B, C, D = (np.asarray(x) for x in (A, B, C, D))
            A[T - 1] = 0; B[T - 1] = 0; D[T - 1] = 0
            cx, cu, cxx, cxu, cuu = self.cost_derivatives(tr.residual[:T], C, D)
            bp, mu_e, rate_e, retries = retry_loop(
                lambda r: self.backward_pass(r, reg_type, use_limits, A, B, cx, cu, cxx, cxu, cuu, tr.actions[:T], limits),
                float(mu[e]), float(rate[e]), factor, min_reg, max_reg, max_iter)
            out["status"][e], out["mu"][e], out["rate"][e], out["retries"][e] = int(bool(bp["ok"])), mu_e, rate_e, retries
            out["nominal_return"][e] = tr.total_return
            if bp["ok"]:
                out["K"][e], out["du"][e], out["dV"][e] = bp["K"], bp["du"], bp["dV"]
            if with_matrices:
                for k, v in dict(A=A, B=B, cx=cx, cu=cu, cxx=cxx, cxu=cxu, cuu=cuu).items():
                    out[k][e] = v
                if bp["ok"]:
                    out["Vx"][e], out["Vxx"][e] = bp["Vx"], bp["Vxx"]
        self.step_calls.append((cand, out["status"].copy()))
        return out
