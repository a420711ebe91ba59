"""Test-only stand-in for a context with mjpcx_set_pruning_batched, on top of TaskBatchOracleContext (BatchOracleContext with the task rows
of set_task_params_batched applied per environment, so a robot whose row was edited really rolls out on it): a launch under the switch rolls
everything out, then retires, per environment, every candidate other than the local nominal whose partial return strictly exceeds that
environment's bound -- the return at a chosen quantile of the environment's own returns, never below its minimum -- overwriting its
return with the partial return and marking it MJPCX_FAILURE_PRUNED | (step << 8), as the device does. What the planner may read of such a
launch (argmin, best and nominal return, the winner's spline and trajectory) is untouched; anything else it read would show. The calls are
logged so that a test can see which launches ran under the switch and on which hints. Never used by the product."""
import numpy as np

from batch_task_oracle_backend import TaskBatchOracleContext
from mujoco_mpc_amd import capi

PRUNED = 0x20000000
ESTATE = -5


def estate(text):
    """an MJPCX_ESTATE as capi.Context raises it (built without the library's error-string lookup)"""
    err = capi.MjpcxError.__new__(capi.MjpcxError)
    RuntimeError.__init__(err, text)
    err.code = ESTATE
    return err


class BatchPruneOracleContext(TaskBatchOracleContext):
    def __init__(self, task, threads=2, quantile=0.25, **kw):
        super().__init__(task, threads=threads, **kw)
        self.quantile = quantile
        self.switch = None            # (num_envs, bounds, hints) while the switch is on
        self.launches = []            # per launch: dict(kind, pruned, hints, retired)
        self.resume_next = None       # per environment: the resumed count the next pruned launch reports (a test's way to a stale hint)
        self.refuse_next_best = False  # the next best_batched after a pruned launch raises MJPCX_ESTATE
        self.last_pruned = False

    def set_pruning_batched(self, enabled, num_envs=0, initial_bound=None, park_hint=None):
        if not enabled:
            self.switch = None
            return
        row = lambda v: np.full(num_envs, np.inf) if v is None else np.array(v, float).reshape(num_envs)
        b, h = row(initial_bound), row(park_hint)
        if not (b >= 0).all() or not (h >= 0).all():
            raise ValueError("negative or NaN bound or hint")
        self.switch = (int(num_envs), b, h)

    def rollout_splines_batched(self, *a, **kw):
        super().rollout_splines_batched(*a, **kw)
        self.last_pruned = False
        self.launches.append(dict(kind="splines", switch_on=self.switch is not None, pruned=False, hints=None, retired=None))

    def rollout_noise_batched(self, n_per_env, horizon, interp, node_times, nominal, ns, num_envs=None):
        super().rollout_noise_batched(n_per_env, horizon, interp, node_times, nominal, ns, num_envs=num_envs)
        self.last_pruned = self.switch is not None
        log = dict(kind="noise", switch_on=self.last_pruned, pruned=self.last_pruned, hints=None, retired=None, iteration=int(ns.iteration), seed=int(ns.seed))
        self.launches.append(log)
        if not self.last_pruned:
            return
        E, n, H = self.E, n_per_env, horizon
        if self.switch[0] != E:
            raise ValueError("the switch was set for another number of environments")
        self.out = {k: np.array(v) for k, v in self.out.items()}
        ret, fail = self.out["total_return"].reshape(E, n), self.out["failure"].reshape(E, n)
        partial = np.cumsum(self.out["costs"].reshape(E, n, H), axis=2) / float(max(H, 1))
        retired = np.zeros(E, int)
        self.final_bound = np.zeros(E)
        for e in range(E):
            full = ret[e].copy()
            bound = min(self.switch[1][e], max(np.quantile(full, self.quantile), full.min()))
            self.final_bound[e] = bound
            for c in range(n):
                if c == ns.nominal_candidate or fail[e, c]:
                    continue
                over = np.nonzero(partial[e, c, :H - 1] > bound)[0]
                if len(over) and full[c] > bound:     # (a device candidate whose return is at or under the bound is never retired)
                    t = int(over[0])
                    ret[e, c], fail[e, c] = partial[e, c, t], PRUNED | (t << 8)
                    retired[e] += 1
        resumed = np.zeros(E, int) if self.resume_next is None else np.array(self.resume_next, int)
        self.resume_next = None
        self.park = np.stack([resumed, np.zeros(E, int), resumed], axis=1)
        self.retired = retired
        log.update(hints=self.switch[2].copy(), retired=retired.copy())

    def prune_stats_batched(self, num_envs):
        E = int(num_envs)
        z = np.zeros(E, np.int64)
        if not self.last_pruned:
            return dict(retired=z, retire_step_sum=z, negative_cost=z != 0, wavefronts_ended_early=z, parked=z, settled_retired=z, resumed=z, final_bound=np.zeros(E))
        return dict(retired=self.retired.astype(np.int64), retire_step_sum=z, negative_cost=z != 0, wavefronts_ended_early=z, parked=self.park[:, 0].astype(np.int64),
                    settled_retired=self.park[:, 1].astype(np.int64), resumed=self.park[:, 2].astype(np.int64), final_bound=self.final_bound.copy())

    def best_batched(self, num_envs, ref_candidate=0, with_spline=True):
        if self.last_pruned and self.refuse_next_best:
            self.refuse_next_best = False
            raise estate("pruned batched rollout: a step's cost was negative in environment(s) 1")
        return super().best_batched(num_envs, ref_candidate, with_spline)
