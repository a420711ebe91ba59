"""Test-only stand-in for the batched cross-entropy entry points of capi.Context (rollout_noise_batched_ce, ce_update_batched) backed by
the CPU oracle, on top of batch_oracle_backend.py: environment e draws the noise of seed + e with its own variance row, and the update
is OracleContext.topk / elite_moments per environment, in the arithmetic of GpuCrossEntropyPlanner. Never used by the product."""
import numpy as np

from batch_oracle_backend import BatchOracleContext
from mujoco_mpc_amd import capi
from oracle import pyoracle


class BatchCeOracleContext(BatchOracleContext):
    def rollout_noise_batched_ce(self, n_per_env, horizon, interp, node_times, nominal, param_variance, ns, num_envs=None):
        self._check(n_per_env)
        if ns.mode != capi.NOISE_CROSS_ENTROPY:
            raise ValueError("rollout_noise_batched_ce needs the cross-entropy noise mode")
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        P = nt.shape[1]
        nom = np.asarray(nominal, float).reshape(self.E, P, self.nu)
        var = np.asarray(param_variance, float).reshape(self.E, P * self.nu)
        cands = range(ns.candidate_offset, ns.candidate_offset + n_per_env)
        nodes = []
        for e in range(self.E):
            nse = capi.make_noise_spec(seed=ns.seed + e, iteration=ns.iteration, mode=ns.mode, candidate_offset=ns.candidate_offset,
                                       nominal_candidate=ns.nominal_candidate, explore_count=ns.explore_count, std0=ns.std0, std1=ns.std1,
                                       param_variance=var[e])
            nodes.append(np.asarray(pyoracle.noise_candidates(self.pm, nse, P, nom[e], cands), float).reshape(n_per_env, P, self.nu))
        self._run_batched(n_per_env, horizon, interp, nt, np.stack(nodes))

    def ce_update_batched(self, num_envs, n_elite, skip_candidate=-1):
        n = self.n_per_env
        left = n - (1 if 0 <= skip_candidate < n else 0)
        if num_envs != self.E or n_elite < 1 or n_elite > left:
            raise ValueError("ce_update_batched: n_elite outside 1..the candidates left after the skip, or another fleet size")
        r = self.out["total_return"].reshape(num_envs, n)
        nodes = self.nodes.reshape(num_envs, n, self.P, self.nu)
        idx, ret, mean, var, avg = [], [], [], [], []
        for e in range(num_envs):
            order = np.lexsort((np.arange(n), r[e]))       # OracleContext.topk
            order = order[order != skip_candidate][:n_elite]
            p = nodes[e][order]                            # OracleContext.elite_moments, then the planner's divisions
            m = p.sum(axis=0) / n_elite
            sq = ((p - m.reshape(1, self.P, self.nu)) ** 2).sum(axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                var.append(sq / (n_elite - 1))
            idx.append(order.astype(np.int32))
            ret.append(r[e][order])
            mean.append(m)
            avg.append(float(r[e][order].sum()) / n_elite)
        return np.stack(idx), np.stack(ret), np.stack(mean), np.stack(var), np.array(avg)
