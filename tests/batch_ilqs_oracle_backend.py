"""Test-only stand-in for capi.Context.ilqg_step_batched_from on the CPU oracle, over batch_ilqg_step_oracle_backend.py's
BatchILQGStepOracleContext: environment e's nominal is fetched from the backend it names -- this one (from_source[e] == 0) or `source`
(== 1, tests/batch_oracle_backend.py's BatchOracleContext after a batched spline rollout) -- and goes through the plain calls of that
file's ilqg_step_batched, with this backend's states from set_states: the calls a fleet planner's sequential middle makes, one
environment after the other. `from_calls` keeps (from_source, candidates, status) of every call. Never used by the product."""
import numpy as np

from batch_gradient_oracle_backend import interpolate
from batch_ilqg_step_oracle_backend import BatchILQGStepOracleContext, retry_loop


class BatchILQSOracleContext(BatchILQGStepOracleContext):
    def __init__(self, task, threads=2, differentiable=False, fail_nominal=()):
        super().__init__(task, threads=threads, differentiable=differentiable, fail_nominal=fail_nominal)
        self.from_calls = []

    def ilqg_step_batched_from(self, source, from_source, candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor,
                               min_reg, max_reg, max_iter, with_matrices=False, num_envs=None):
        cand, frm = [int(c) for c in candidate], [int(f) for f in from_source]
        E, m, ndx = len(cand), self.nu, 2 * self.pm.struct.nv
        assert E == self.E == len(frm) and set(frm) <= {0, 1} and T >= 2 and 1 <= max_iter <= 64
        ev = [int(i) for i in evaluate]
        limits = np.asarray(self.task.model.actuator_ctrlrange, float).reshape(-1, 2)
        out = dict(K=np.zeros((E, T, m, ndx)), du=np.zeros((E, T, m)), dV=np.zeros((E, 2)), status=np.full(E, -1, np.int32), mu=np.zeros(E),
                   rate=np.zeros(E), retries=np.zeros(E, np.int32), nominal_return=np.zeros(E))
        assert not with_matrices
        for e in range(E):
            if cand[e] < 0:
                continue
            ctx = source if frm[e] else self
            n = ctx.n_per_env
            assert cand[e] < n and ctx.N == E * n and T <= ctx.H
            tr = ctx.fetch_trajectory(e * n + cand[e])
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
        self.from_calls.append((frm, cand, out["status"].copy()))
        return out
