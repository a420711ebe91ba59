"""Test-only stand-ins for capi.Context.rollout_splines_noisy, rollout_splines_noisy_batched and robust_step_batched on the CPU oracle,
in the manner of batch_oracle_backend.py: environment e of a batched noisy call is the oracle's NoisyRollout of that environment alone
with the force-noise stream of seed + e (pyoracle.rollout_batch(..., xfrc_std, xfrc_rate, seed, candidate_offset)), laid out
environment-major; robust_step_batched is the selection by (return, index), the replication, that call and the planner's own Python
loop (planners.robust_scores). With the rows of batch_task_oracle_backend.TaskRows, so every environment may have its own task
parameters. Never used by the product."""
import numpy as np

from batch_oracle_backend import BatchOracleContext
from batch_task_oracle_backend import TaskRows
from mujoco_mpc_amd.planners import robust_scores
from oracle import pyoracle


class _NoisyOracleContext(BatchOracleContext):
    def rollout_splines_noisy(self, horizon, interp, node_times, node_values, xfrc_std, xfrc_rate, seed=0, candidate_offset=0):
        nt = np.asarray(node_times, float).reshape(-1)
        nv = np.asarray(node_values, float)
        P = nt.size
        N = nv.size // (P * self.nu)
        self.N, self.H, self.P = N, horizon, P
        self.nodes = nv.reshape(N, P, self.nu).copy()
        self.out = pyoracle.rollout_batch(self.pm, self.pt, self.state, self.time, self.mocap, N, horizon, P, interp, nt, self.nodes,
                                          num_threads=self.threads, xfrc_std=xfrc_std, xfrc_rate=xfrc_rate, seed=seed,
                                          candidate_offset=candidate_offset)

    def rollout_splines_noisy_batched(self, horizon, interp, node_times, node_values, xfrc_std, xfrc_rate, seed=0, candidate_offset=0,
                                      num_envs=None, n_per_env=None):
        E = self.E
        nt = np.asarray(node_times, float).reshape(E, -1)
        P = nt.shape[1]
        nv = np.asarray(node_values, float)
        n = nv.size // (E * P * self.nu)
        self._check(n)
        nv = nv.reshape(E, n, P, self.nu)
        outs = []
        for e in range(E):
            mocap = None if self.env_mocap is None else self.env_mocap[e]
            outs.append(pyoracle.rollout_batch(self.pm, self.pt, self.env_states[e], float(self.env_times[e]), mocap, n, horizon, P, interp,
                                               nt[e], nv[e], num_threads=self.threads, xfrc_std=xfrc_std, xfrc_rate=xfrc_rate,
                                               seed=seed + e, candidate_offset=candidate_offset))
        self.out = {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in outs[0]}
        self.nodes = nv.reshape(E * n, P, self.nu).copy()
        self.state = self.env_states[0]
        self.N, self.H, self.P, self.n_per_env = E * n, horizon, P, n

    def ce_update_batched(self, num_envs, n_elite, skip_candidate=-1):
        """the order and the returns only (what the sequential path of a robust step reads): ascending, ties to the lower index, NaN last"""
        n = self.n_per_env
        ret = self.out["total_return"].reshape(num_envs, n)
        keep = [np.array([i for i in np.lexsort((np.arange(n), ret[e])) if i != skip_candidate][:n_elite], np.int32) for e in range(num_envs)]
        idx = np.stack(keep)
        return idx, np.take_along_axis(ret, idx, 1), None, None, None

    def robust_step_batched(self, source, num_envs, num_candidates, repetitions, horizon, interp, node_times, xfrc_std, xfrc_rate, seed=0,
                            candidate_offset=0):
        E, k, R, n = num_envs, num_candidates, repetitions, source.n_per_env
        if source is self or E != self.E or source.N != E * n or not 1 <= k <= n or R < 1:
            raise ValueError("robust_step_batched: bad arguments")
        ret = source.out["total_return"].reshape(E, n)
        order = np.stack([np.lexsort((np.arange(n), ret[e]))[:k] for e in range(E)]).astype(np.int32)   # ascending, ties to the lower index, NaN last
        n_pad = 64 * ((k * R + 63) // 64)
        rank = np.minimum(np.arange(n_pad) // R, k - 1)                                                 # rollout j = rank * R + repetition; the padding repeats the last rank
        values = np.stack([source.nodes[e * n + order[e][rank]] for e in range(E)])
        self.rollout_splines_noisy_batched(horizon, interp, node_times, values, xfrc_std, xfrc_rate, seed, candidate_offset)
        out = dict(best=np.zeros(E, np.int32), candidate=order, candidate_return=np.take_along_axis(ret, order, 1), perturbed_score=np.zeros((E, k)),
                   valid=np.zeros((E, k), np.int32), spline=np.zeros((E, self.P, self.nu)))
        for e in range(E):
            sl = slice(e * n_pad, e * n_pad + k * R)
            out["perturbed_score"][e], out["valid"][e], out["best"][e] = robust_scores(out["candidate_return"][e], self.out["total_return"][sl],
                                                                                        self.out["failure"][sl], R)
            out["spline"][e] = source.nodes[e * n + order[e][out["best"][e]]]
        return out


class BatchRobustOracleContext(TaskRows, _NoisyOracleContext):
    """... and one packed task per environment where set_task_params_batched / set_residual_states gave rows"""

    def rollout_splines_noisy_batched(self, horizon, interp, node_times, node_values, xfrc_std, xfrc_rate, seed=0, candidate_offset=0,
                                      num_envs=None, n_per_env=None):
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        nv = np.asarray(node_values, float).reshape(self.E, -1, nt.shape[1], self.nu)
        sup = super()
        self._each(lambda e: sup.rollout_splines_noisy_batched(horizon, interp, nt[e:e + 1], nv[e:e + 1], xfrc_std, xfrc_rate, seed + e, candidate_offset))
