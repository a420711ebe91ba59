"""Test-only stand-ins for capi.Context.cma_set_state_batched, cma_get_state_batched, rollout_cma_batched and cma_update_batched on the
CPU oracle, in the manner of batch_sample_gradient_oracle_backend.py: the candidates are built here -- the mean, clamp(mean + sigma s A z)
with the oracle's normals (pyoracle's ogaussian_pair of (seed + e, candidate, pair, iteration)) in planners.cma_candidates' order of
operations -- and rolled out by the oracle, environment by environment; the update is planners.cma_update. What the library keeps in
the context (sigma, C, A, the paths, the generation) is kept here. `nan_envs`: environments whose returns the update sees as NaN.
Never used by the product."""
import numpy as np

from batch_oracle_backend import BatchOracleContext
from batch_sample_gradient_oracle_backend import oracle_normals
from batch_task_oracle_backend import TaskRows
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import cma_candidates, cma_factor, cma_update

STATE_KEYS = ("sigma", "generation", "C", "A", "p_sigma", "p_c")


class _CmaOracleContext(BatchOracleContext):
    cma = None          # per environment: dict of sigma, C, A, p_sigma, p_c, generation
    cma_live = None     # what the last rollout_cma_batched left for the update
    nan_envs = ()

    def cma_set_state_batched(self, num_envs, num_params, sigma, C_=None, p_sigma=None, p_c=None):
        E, d = int(num_envs), int(num_params)
        if d > capi.CMA_MAX_PARAMS:
            raise ValueError(f"cma_set_state_batched: {d} parameters; at most {capi.CMA_MAX_PARAMS}")
        sig = np.broadcast_to(np.asarray(sigma, float).reshape(-1), (E,))
        if E < 1 or d < 1 or d % self.nu or not (np.all(np.isfinite(sig)) and np.all(sig > 0)):
            raise ValueError("cma_set_state_batched: bad shape or a sigma that is not finite and > 0")
        Cs = np.stack([np.eye(d)] * E) if C_ is None else np.asarray(C_, float).reshape(E, d, d)
        ps = np.zeros((E, d)) if p_sigma is None else np.asarray(p_sigma, float).reshape(E, d)
        pc = np.zeros((E, d)) if p_c is None else np.asarray(p_c, float).reshape(E, d)
        states = []
        for e in range(E):
            A = cma_factor(Cs[e]) if np.array_equal(Cs[e], Cs[e].T) else None
            if A is None:
                self.cma = None
                raise ValueError(f"cma_set_state_batched: C of environment {e} is not symmetric positive definite")
            states.append(dict(sigma=float(sig[e]), C=Cs[e].copy(), A=A, p_sigma=ps[e].copy(), p_c=pc[e].copy(), generation=0))
        self.cma = states

    def _cma_for(self, E, d, who):
        if self.cma is None or len(self.cma) != E or self.cma[0]["C"].shape[0] != d:
            raise ValueError(f"{who}: no state of {E} environments x {d} parameters is set")

    def cma_get_state_batched(self, num_envs, num_params):
        self._cma_for(int(num_envs), int(num_params), "cma_get_state_batched")
        return {k: np.stack([np.asarray(s[k]) for s in self.cma]) for k in STATE_KEYS}

    def rollout_cma_batched(self, n_per_env, horizon, interp, node_times, nominal, seed=0, iteration=0, num_envs=None):
        E, n = self.E, int(n_per_env)
        nt = np.asarray(node_times, float).reshape(E, -1)
        P = nt.shape[1]
        d = P * self.nu
        nom = np.asarray(nominal, float).reshape(E, d)
        self._check(n)
        self._cma_for(E, d, "rollout_cma_batched")
        ctrlrange = np.asarray(self.task.model.actuator_ctrlrange, float)
        z = np.stack([oracle_normals(seed + e, n, d, iteration, first=1) for e in range(E)])
        nodes = np.stack([cma_candidates(nom[e], z[e], self.cma[e]["sigma"], self.cma[e]["A"], ctrlrange) for e in range(E)])
        self.cma_live = dict(E=E, n=n, z=z, nominal=nom)
        self.rollout_splines_batched(horizon, interp, nt, nodes.reshape(E, n, P, self.nu))
        self.cma_live["N"] = self.N

    def cma_update_batched(self, num_envs, params, want_order=False):
        s, E = self.cma_live, int(num_envs)
        if s is None or s["E"] != E or self.N != E * s["n"] or self.cma is None or len(self.cma) != E:
            raise ValueError("cma_update_batched: the last rollout was not a rollout_cma_batched of this shape")
        if not 1 <= int(params["mu"]) <= s["n"] - 1 or params["c_one"] + params["c_mu"] > 1 or not all(np.isfinite(params[k]) for k in capi.CMA_CONSTANTS):
            raise ValueError("cma_update_batched: mu outside 1..n-1, c_one + c_mu > 1 or a constant that is not finite")
        ret = self.out["total_return"].reshape(E, s["n"]).copy()
        for e in self.nan_envs:
            ret[e] = np.nan
        ctrlrange = np.asarray(self.task.model.actuator_ctrlrange, float)
        ups = [cma_update(ret[e], s["nominal"][e], s["z"][e], self.cma[e], params, ctrlrange) for e in range(E)]
        self.cma = [u["state"] for u in ups]
        self.cma_last = ups     # (for the tests)
        out = {k: np.array([u[k] for u in ups]) for k in ("best_return", "nominal_return", "improvement", "sigma")}
        out.update({k: np.array([u[k] for u in ups], np.int32) for k in ("index", "valid", "restarted")})
        out["mean"] = np.stack([u["mean"].reshape(-1, self.nu) for u in ups])
        out["order"] = np.stack([u["order"] for u in ups]).astype(np.int32) if want_order else None
        return out


class BatchCmaOracleContext(TaskRows, _CmaOracleContext):
    """... and one packed task per environment where set_task_params_batched / set_residual_states gave rows"""
