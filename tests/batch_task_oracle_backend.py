"""Test-only stand-ins for capi.Context.set_task_params_batched / set_residual_states on the CPU oracle: the batched oracle backends
(batch_oracle_backend.py and its siblings) with one packed task per environment. The oracle takes its task parameters from the packed
task, so environment e of a batched call is the parent class's call on a fleet of ONE -- environment e's state, clock, mocap pose and
slice of every argument -- with a task packed from row e, and the outputs concatenated environment-major. The plain values
(set_task_params, set_residual_state) live beside the rows, as in the library: the plain calls of a fleet planner's sequential chain use
them, the batched calls never do where a row is given; a plain set_residual_state drops the per-environment residual state, as
mjpcx_set_residual_state does. Never used by the product."""
import numpy as np

from batch_ce_oracle_backend import BatchCeOracleContext
from batch_gradient_oracle_backend import BatchGradientOracleContext
from batch_ilqg_oracle_backend import BatchILQGOracleContext
from batch_ilqg_step_oracle_backend import BatchILQGStepOracleContext
from batch_oracle_backend import BatchOracleContext
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.cstructs import PackedTask

FIELDS = ("weight", "norm_parameter", "parameters", "risk", "residual_int", "residual_real")


class TaskRows:
    """mixin in front of a BatchOracleContext"""

    def _init_rows(self):
        if not hasattr(self, "plain"):
            spec = self.task.spec()
            self.plain = {k: (float(spec[k]) if k == "risk" else list(spec[k])) for k in FIELDS}    # what set_task_params / set_residual_state gave
            self.rows = {k: None for k in FIELDS}                                                    # E x ..., None: the plain value
            self.pushes = []                                                                         # every set_task_params_batched, for the tests

    def _pack(self, values):
        spec = self.task.spec()
        spec.update(values)
        return PackedTask(spec)

    # ---- plain
    def set_task_params(self, weight=None, norm_parameter=None, parameters=None, risk=0.0):
        self._init_rows()
        for k, v in (("weight", weight), ("norm_parameter", norm_parameter), ("parameters", parameters)):
            if v is not None:
                self.plain[k] = [float(x) for x in v]
        self.plain["risk"] = float(risk)
        self.pt = self._pack(self.plain)

    def set_residual_state(self, residual_int=None, residual_real=None):
        self._init_rows()
        if residual_int is not None:
            self.plain["residual_int"] = [int(x) for x in residual_int]
            self.rows["residual_int"] = None
        if residual_real is not None:
            self.plain["residual_real"] = [float(x) for x in residual_real]
            self.rows["residual_real"] = None
        self.pt = self._pack(self.plain)

    # ---- per environment
    def set_states(self, states, times, mocap=None, userdata=None):
        self._init_rows()
        if getattr(self, "E", 0) != len(times):
            self.rows = {k: None for k in FIELDS}
        super().set_states(states, times, mocap, userdata)

    def set_task_params_batched(self, weight=None, norm_parameter=None, parameters=None, risk=None):
        self._init_rows()
        for k, v in (("weight", weight), ("norm_parameter", norm_parameter), ("parameters", parameters), ("risk", risk)):
            self.rows[k] = None if v is None else np.array(v, float).reshape(self.E, -1)
        self.pushes.append({k: None if self.rows[k] is None else self.rows[k].copy() for k in FIELDS})

    def set_residual_states(self, residual_int=None, residual_real=None):
        self._init_rows()
        if residual_int is not None:
            self.rows["residual_int"] = np.array(residual_int, np.int32).reshape(self.E, -1)
        if residual_real is not None:
            self.rows["residual_real"] = np.array(residual_real, float).reshape(self.E, -1)

    def env_values(self, e):
        out = {}
        for k in FIELDS:
            r = self.rows[k]
            if r is None or r.shape[1] == 0:
                out[k] = self.plain[k]
            elif k == "risk":
                out[k] = float(r[e, 0])
            else:
                out[k] = [int(x) if k == "residual_int" else float(x) for x in r[e]]
        return out

    def _each(self, call, view=False):
        """call(e) -- a parent's batched method on the fleet of environment e alone -- for every environment; the environment-major
        concatenation of what each left in self.out / self.nodes. view: the call reads the last rollout (self.out) instead of making one."""
        self._init_rows()
        saved = {k: getattr(self, k) for k in ("E", "env_states", "env_times", "env_mocap", "pt")}
        fail = getattr(self, "fail_nominal", None)
        full, n = (self.out, self.n_per_env) if view else (None, 0)
        outs, nodes, results = [], [], []
        try:
            for e in range(saved["E"]):
                self.E, self.env_states, self.env_times = 1, saved["env_states"][e:e + 1], saved["env_times"][e:e + 1]
                self.env_mocap = None if saved["env_mocap"] is None else saved["env_mocap"][e:e + 1]
                self.pt = self._pack(self.env_values(e))
                if fail is not None:
                    self.fail_nominal = {0} if e in fail else set()
                if view:
                    self.out, self.N = {k: v[e * n:(e + 1) * n] for k, v in full.items()}, n
                results.append(call(e))
                if not view:
                    outs.append(self.out)
                    nodes.append(getattr(self, "nodes", None))
        finally:
            for k, v in saved.items():
                setattr(self, k, v)
            if fail is not None:
                self.fail_nominal = fail
        if view:
            self.out, self.N = full, saved["E"] * n
        else:
            self.out = {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in outs[0]}
            if nodes[0] is not None:
                self.nodes = np.concatenate(nodes)
            self.N = saved["E"] * self.n_per_env
        return results

    def _spec(self, ns, e, **kw):
        return capi.make_noise_spec(seed=ns.seed + e, iteration=ns.iteration, mode=ns.mode, candidate_offset=ns.candidate_offset,
                                    nominal_candidate=ns.nominal_candidate, explore_count=ns.explore_count, std0=ns.std0, std1=ns.std1, **kw)

    def rollout_splines_batched(self, horizon, interp, node_times, node_values, num_envs=None, n_per_env=None):
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        nv = np.asarray(node_values, float).reshape(self.E, -1, nt.shape[1], self.nu)
        sup = super()
        self._each(lambda e: sup.rollout_splines_batched(horizon, interp, nt[e:e + 1], nv[e:e + 1]))

    def rollout_noise_batched(self, n_per_env, horizon, interp, node_times, nominal, ns, num_envs=None):
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        nom = np.asarray(nominal, float).reshape(self.E, nt.shape[1], self.nu)
        sup = super()
        self._each(lambda e: sup.rollout_noise_batched(n_per_env, horizon, interp, nt[e:e + 1], nom[e:e + 1], self._spec(ns, e)))

    def rollout_noise_batched_ce(self, n_per_env, horizon, interp, node_times, nominal, param_variance, ns, num_envs=None):
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        nom = np.asarray(nominal, float).reshape(self.E, nt.shape[1], self.nu)
        var = np.asarray(param_variance, float).reshape(self.E, -1)
        sup = super()
        self._each(lambda e: sup.rollout_noise_batched_ce(n_per_env, horizon, interp, nt[e:e + 1], nom[e:e + 1], var[e:e + 1], self._spec(ns, e)))

    def rollout_feedback_batched(self, horizon, mode, representation, use_state, times, states, actions, gains, improvement, alpha,
                                 num_envs=None, n_per_env=None):
        arrs = [np.asarray(x, float) for x in (times, states, actions, gains, improvement, alpha)]
        sup = super()
        self._each(lambda e: sup.rollout_feedback_batched(horizon, mode, representation, use_state, *[a[e:e + 1] for a in arrs]))


class TaskBatchOracleContext(TaskRows, BatchOracleContext):
    pass


class TaskBatchCeOracleContext(TaskRows, BatchCeOracleContext):
    pass


class TaskBatchGradientOracleContext(TaskRows, BatchGradientOracleContext):
    def gradient_step_batched(self, num_envs, candidate, T, evaluate, eps, centered, representation, node_times, with_matrices=False):
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        sup = super()
        res = self._each(lambda e: sup.gradient_step_batched(1, candidate, T, evaluate, eps, centered, representation, nt[e:e + 1], with_matrices),
                         view=True)
        return {k: np.concatenate([r[k] for r in res]) for k in res[0]}


class TaskBatchILQGOracleContext(TaskRows, BatchILQGOracleContext):
    pass


class TaskBatchILQGStepOracleContext(TaskRows, BatchILQGStepOracleContext):
    def ilqg_step_batched(self, candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor, min_reg, max_reg, max_iter,
                          with_matrices=False, num_envs=None):
        first = len(self.step_calls)
        sup = super()
        res = self._each(lambda e: sup.ilqg_step_batched([candidate[e]], T, evaluate, eps, centered, reg_type, use_limits, [mu[e]], [rate[e]], factor,
                                                         min_reg, max_reg, max_iter, with_matrices), view=True)
        del self.step_calls[first:]                          # (one entry per environment) -> one for the call
        out = {k: np.concatenate([r[k] for r in res]) for k in res[0]}
        self.step_calls.append(([int(c) for c in candidate], out["status"].copy()))
        return out
