"""Test-only stand-ins for a context with mjpcx_set_prune_rank, for the Cross-Entropy planners off the device.

BatchCeRankOracleContext, on top of TaskBatchCeOracleContext (the batched cross-entropy entry points on the CPU oracle, with the task rows of
set_task_params_batched applied per environment): a rollout_noise_batched_ce under set_pruning_batched at a rank K > 1 rolls everything out,
then retires, per environment, every candidate other than the local nominal whose return is strictly above T = the K-th smallest return of the
environment and whose partial return passes T before the last step -- overwriting its return with that partial return and marking it
MJPCX_FAILURE_PRUNED | (step << 8), as the device does. At rank 1 the launch ignores the switch, as the device does. ce_update_batched
after such a launch answers only for n_elite + (skip_candidate >= 0) <= K and raises MJPCX_ESTATE otherwise, so a planner that asks for too
low a rank shows. RankOracleContext does the same for the plain launch of GpuCrossEntropyPlanner (set_pruning, set_park_hint, topk,
elite_moments). What a planner may read of such a launch is untouched; anything else it read would show. The calls are logged. Never used by
the product."""
import numpy as np

from batch_prune_oracle_backend import ESTATE, PRUNED, estate
from batch_task_oracle_backend import TaskBatchCeOracleContext
from oracle_backend import OracleContext

__all__ = ["BatchCeRankOracleContext", "RankOracleContext", "PRUNED", "ESTATE"]


def retire_above_kth(ret, fail, costs, H, rank, nominal):
    """one environment, in place: -> (T, candidates retired)"""
    full = ret.copy()
    T = np.sort(full)[rank - 1] if len(full) >= rank else np.inf
    partial = np.cumsum(costs, axis=1) / float(max(H, 1))
    retired = 0
    for c in range(len(full)):
        if c == nominal or fail[c] or not full[c] > T:
            continue
        over = np.nonzero(partial[c, :H - 1] > T)[0]
        if len(over):
            t = int(over[0])
            ret[c], fail[c] = partial[c, t], PRUNED | (t << 8)
            retired += 1
    return float(T), retired


class BatchCeRankOracleContext(TaskBatchCeOracleContext):
    def __init__(self, task, threads=2, **kw):
        super().__init__(task, threads=threads, **kw)
        self.rank = 1
        self.switch = None             # (num_envs, hints) while set_pruning_batched is on
        self.launches = []             # per launch: dict(kind, pruned, rank, hints, retired, seed, iteration)
        self.resume_next = None        # per environment: the resumed count the next pruned launch reports (a test's way to a stale hint)
        self.refuse_next_update = False  # the next ce_update_batched after a pruned launch raises MJPCX_ESTATE
        self.last_pruned = False
        self.last_rank = 1

    def set_prune_rank(self, rank=1):
        if rank < 1:
            raise ValueError("rank < 1")
        self.rank = int(rank)

    def set_pruning_batched(self, enabled, num_envs=0, initial_bound=None, park_hint=None):
        if not enabled:
            self.switch = None
            return
        if initial_bound is not None and self.rank > 1 and np.isfinite(np.asarray(initial_bound, float)).any():
            raise ValueError("a finite initial bound in rank mode")
        h = np.full(num_envs, np.inf) if park_hint is None else np.array(park_hint, float).reshape(num_envs)
        if not (h >= 0).all():
            raise ValueError("negative or NaN hint")
        self.switch = (int(num_envs), h)

    def rollout_splines_batched(self, *a, **kw):
        super().rollout_splines_batched(*a, **kw)
        self.last_pruned = False
        self.launches.append(dict(kind="splines", switch_on=self.switch is not None, pruned=False, rank=self.rank, hints=None, retired=None))

    def rollout_noise_batched_ce(self, n_per_env, horizon, interp, node_times, nominal, param_variance, ns, num_envs=None):
        super().rollout_noise_batched_ce(n_per_env, horizon, interp, node_times, nominal, param_variance, ns, num_envs=num_envs)
        self.last_pruned = self.switch is not None and self.rank > 1
        self.last_rank = self.rank if self.last_pruned else 1
        log = dict(kind="ce", switch_on=self.switch is not None, pruned=self.last_pruned, rank=self.rank, hints=None, retired=None,
                   iteration=int(ns.iteration), seed=int(ns.seed))
        self.launches.append(log)
        if not self.last_pruned:
            return
        E, n, H = self.E, n_per_env, horizon
        if self.switch[0] != E:
            raise ValueError("the switch was set for another number of environments")
        self.out = {k: np.array(v) for k, v in self.out.items()}
        ret, fail = self.out["total_return"].reshape(E, n), self.out["failure"].reshape(E, n)
        costs = self.out["costs"].reshape(E, n, H)
        self.final_bound, self.retired = np.zeros(E), np.zeros(E, int)
        for e in range(E):
            self.final_bound[e], self.retired[e] = retire_above_kth(ret[e], fail[e], costs[e], H, self.rank, ns.nominal_candidate)
        resumed = np.zeros(E, int) if self.resume_next is None else np.array(self.resume_next, int)
        self.resume_next = None
        self.park = np.stack([resumed, np.zeros(E, int), resumed], axis=1)
        log.update(hints=self.switch[1].copy(), retired=self.retired.copy())

    def prune_stats_batched(self, num_envs):
        E = int(num_envs)
        z = np.zeros(E, np.int64)
        if not self.last_pruned:
            return dict(retired=z, retire_step_sum=z, negative_cost=z != 0, wavefronts_ended_early=z, parked=z, settled_retired=z, resumed=z, final_bound=np.zeros(E))
        return dict(retired=self.retired.astype(np.int64), retire_step_sum=z, negative_cost=z != 0, wavefronts_ended_early=z, parked=self.park[:, 0].astype(np.int64),
                    settled_retired=self.park[:, 1].astype(np.int64), resumed=self.park[:, 2].astype(np.int64), final_bound=self.final_bound.copy())

    def ce_update_batched(self, num_envs, n_elite, skip_candidate=-1):
        if self.last_pruned and self.refuse_next_update:
            self.refuse_next_update = False
            raise estate("pruned batched rollout: a step's cost was negative in environment(s) 1")
        if self.last_pruned and n_elite + (1 if skip_candidate >= 0 else 0) > self.last_rank:
            raise estate("the last rollout was pruned at rank %d" % self.last_rank)
        return super().ce_update_batched(num_envs, n_elite, skip_candidate)


class RankOracleContext(OracleContext):
    """the plain launch of GpuCrossEntropyPlanner under set_pruning + set_prune_rank + set_park_hint"""

    def __init__(self, task, threads=2, **kw):
        super().__init__(task, threads=threads, **kw)
        self.rank, self.prune_on, self.hint = 1, False, np.inf
        self.launches = []
        self.resume_next = 0
        self.refuse_next_topk = False
        self.last_pruned, self.last_rank = False, 1

    def set_prune_rank(self, rank=1):
        if rank < 1:
            raise ValueError("rank < 1")
        self.rank = int(rank)

    def set_pruning(self, enabled, initial_bound=float("inf")):
        if enabled and self.rank > 1 and np.isfinite(initial_bound):
            raise ValueError("a finite initial bound in rank mode")
        self.prune_on = bool(enabled)

    def set_park_hint(self, hint=float("inf")):
        if not hint >= 0:
            raise ValueError("negative or NaN hint")
        self.hint = float(hint)

    def rollout_splines(self, *a, **kw):
        super().rollout_splines(*a, **kw)
        self.last_pruned = False
        self.launches.append(dict(kind="splines", pruned=False, rank=self.rank, hint=None, retired=0))

    def rollout_noise(self, n, horizon, interp, node_times, nominal, ns):
        super().rollout_noise(n, horizon, interp, node_times, nominal, ns)
        self.last_pruned = self.prune_on
        self.last_rank = self.rank if self.last_pruned else 1
        log = dict(kind="noise", pruned=self.last_pruned, rank=self.rank, hint=self.hint if self.last_pruned else None, retired=0,
                   iteration=int(ns.iteration), seed=int(ns.seed))
        self.launches.append(log)
        self.resumed, self.resume_next = (self.resume_next, 0) if self.last_pruned else (0, self.resume_next)
        if not self.last_pruned or self.rank <= 1:
            return
        self.out = {k: np.array(v) for k, v in self.out.items()}
        H = horizon
        _, log["retired"] = retire_above_kth(self.out["total_return"], self.out["failure"], self.out["costs"].reshape(n, H), H, self.rank,
                                             ns.nominal_candidate - ns.candidate_offset)

    def prune_stats(self):
        r = self.launches[-1]["retired"] if self.last_pruned else 0
        return dict(retired=r, retire_step_sum=0, negative_cost=False, wavefronts_ended_early=0)

    def park_stats(self):
        r = self.resumed if self.last_pruned else 0
        return dict(parked=r, settled_retired=0, resumed=r, resume_ms=0.0)

    def topk(self, k):
        if self.last_pruned and self.refuse_next_topk:
            self.refuse_next_topk = False
            raise estate("pruned rollout: a step's cost was negative")
        if self.last_pruned and k > self.last_rank:
            raise estate("the last rollout was pruned at rank %d" % self.last_rank)
        return super().topk(k)

    def elite_moments(self, candidates, mean=None):
        cand = np.asarray(candidates, int).reshape(-1)
        if self.last_pruned and (len(cand) > self.last_rank or (np.asarray(self.out["failure"])[cand] & PRUNED).any()):
            raise estate("the last rollout was pruned at rank %d" % self.last_rank)
        return super().elite_moments(candidates, mean)
