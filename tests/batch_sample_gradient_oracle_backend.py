"""Test-only stand-ins for capi.Context.rollout_sample_gradient_batched and sample_gradient_update_batched on the CPU oracle, in the
manner of batch_robust_oracle_backend.py: the candidates are built here -- the nominal, clamp(nominal + noise_exploration z) with the
oracle's normals (pyoracle's ogaussian_pair of (seed + e, candidate, pair, iteration)), the gradient candidates as TimeSpline.sample of
their own splines at the new node times -- and rolled out by the oracle, environment by environment; the update is
planners.sample_gradient_update. What the library keeps in the context between plan steps (the shaping weights, the gradient, the next
gradient candidates and their node times) is kept here. With the rows of batch_task_oracle_backend.TaskRows, so every environment may
have its own task parameters. Never used by the product."""
import ctypes as C

import numpy as np

from batch_oracle_backend import BatchOracleContext
from batch_task_oracle_backend import TaskRows
from mujoco_mpc_amd import capi
from mujoco_mpc_amd.planners import clamp, sample_gradient_update
from mujoco_mpc_amd.spline import TimeSpline
from oracle import pyoracle


def oracle_normals(seed, n, num_parameters, iteration, first=0):
    """z[c][j] = ogaussian_pair(seed, c, j >> 1, iteration)[j & 1] for the candidates first..n-1 (rows below `first` stay zero)"""
    z = np.zeros((n, num_parameters + (num_parameters & 1)))
    pair = np.zeros(2)
    ptr = pair.ctypes.data_as(C.POINTER(C.c_double))
    draw = pyoracle.lib().ogaussian_pair
    for c in range(first, n):
        for q in range((num_parameters + 1) // 2):
            draw(int(seed), c, q, int(iteration), ptr)
            z[c, 2 * q:2 * q + 2] = pair
    return z[:, :num_parameters]


def resample(times, values, interp, new_times, ctrlrange):
    """ResamplePolicy (sample_gradient/planner.cc:290-318) of one spline: TimeSpline::Sample at the new node times, clamped"""
    spline = TimeSpline(values.shape[1], interp)
    for t, v in zip(times, values):
        spline.add_node(t, v)
    return np.stack([clamp(spline.sample(t), ctrlrange) for t in new_times])


def candidates(ctrlrange, n, num_gradient, interp, node_times, nominal, noise_exploration, seed, iteration, gradient_values, gradient_times):
    """one environment's n candidate splines (n x P x nu) and the normals they were made from (n x P*nu)"""
    P, nu = nominal.shape
    nn = n - num_gradient
    z = oracle_normals(seed, nn, P * nu, iteration, first=1)
    nodes = np.zeros((n, P, nu))
    nodes[0] = nominal
    for c in range(1, nn):
        nodes[c] = clamp(nominal + noise_exploration * z[c].reshape(P, nu), ctrlrange)
    for g in range(num_gradient):
        nodes[nn + g] = resample(gradient_times, gradient_values[g], interp, node_times, ctrlrange)
    return nodes, np.concatenate([z, np.zeros((num_gradient, P * nu))])


class _SampleGradientOracleContext(BatchOracleContext):
    sg = None   # what the library's context keeps between the two calls and between plan steps

    def rollout_sample_gradient_batched(self, n_per_env, num_gradient, horizon, interp, node_times, nominal, noise_exploration, seed=0, iteration=0,
                                        gradient_values=None, gradient_times=None, num_envs=None):
        E, n, G = self.E, int(n_per_env), int(num_gradient)
        nt = np.asarray(node_times, float).reshape(E, -1)
        P = nt.shape[1]
        nom = np.asarray(nominal, float).reshape(E, P, self.nu)
        self._check(n)
        if not 0 <= G <= n - 1 or not noise_exploration > 0 or (gradient_values is None) != (gradient_times is None):
            raise ValueError("rollout_sample_gradient_batched: bad arguments")
        s = self.sg
        same = s is not None and (s["E"], s["G"], s["P"]) == (E, G, P)
        if not same:
            s = self.sg = dict(E=E, G=G, P=P, gradient=np.zeros((E, P * self.nu)), weights=None, candidates=None, times=None)
        if G > 0 and gradient_values is not None:
            gv, gt = np.asarray(gradient_values, float).reshape(E, G, P, self.nu), np.asarray(gradient_times, float).reshape(E, P)
        elif G > 0:
            if s["candidates"] is None:
                raise ValueError("rollout_sample_gradient_batched: no gradient candidates: no update with this E, G, P has run")
            gv, gt = s["candidates"].reshape(E, G, P, self.nu), s["times"]
        else:
            gv, gt = np.zeros((E, 0, P, self.nu)), nt
        ctrlrange = np.asarray(self.task.model.actuator_ctrlrange, float)
        made = [candidates(ctrlrange, n, G, interp, nt[e], nom[e], noise_exploration, seed + e, iteration, gv[e], gt[e]) for e in range(E)]
        s.update(n=n, z=np.stack([m[1] for m in made]), nominal=nom.reshape(E, -1), node_times=nt, live=True)
        self.rollout_splines_batched(horizon, interp, nt, np.stack([m[0] for m in made]))

    def sample_gradient_update_batched(self, num_envs, num_gradient, flags, gradient_filter, max_step, min_step, noise_exploration):
        s, E, G = self.sg, int(num_envs), int(num_gradient)
        if s is None or not s.get("live") or (s["E"], s["G"]) != (E, G) or self.N != E * s["n"]:
            raise ValueError("sample_gradient_update_batched: the last rollout was not a rollout_sample_gradient_batched of this shape")
        n, nn = s["n"], s["n"] - G
        compute = bool(flags & capi.SG_COMPUTE_WEIGHTS)
        if G > 0 and not compute and (s["weights"] is None or s["weights"].shape != (E, nn)):
            raise ValueError("sample_gradient_update_batched: no shaping weights for this shape")
        if flags & capi.SG_ZERO_GRADIENT:
            s["gradient"] = np.zeros_like(s["gradient"])
        ret = self.out["total_return"].reshape(E, n)
        ctrlrange = np.asarray(self.task.model.actuator_ctrlrange, float)
        ups = [sample_gradient_update(ret[e], s["nominal"][e], s["z"][e], G, ctrlrange, None if compute or G < 1 else s["weights"][e], s["gradient"][e],
                                      compute, gradient_filter, max_step, min_step, noise_exploration) for e in range(E)]
        win = np.array([u["winner"] for u in ups], np.int32)
        if G > 0:
            s["weights"] = np.stack([u["weights"] for u in ups])
            s["gradient"] = np.stack([u["gradient"] for u in ups])
            s["candidates"] = np.stack([u["candidates"] for u in ups])
            s["times"] = s["node_times"].copy()
        self.sg_last = ups   # (for the tests: order, gradient_previous)
        return dict(index=win, winner_type=np.array([u["winner_type"] for u in ups], np.int32), best_return=ret[np.arange(E), win].copy(),
                    nominal_return=ret[:, 0].copy(), improvement=np.array([u["improvement"] for u in ups]),
                    spline=np.stack([self.nodes[e * n + win[e]] for e in range(E)]), gradient=s["gradient"].copy())


class BatchSampleGradientOracleContext(TaskRows, _SampleGradientOracleContext):
    """... and one packed task per environment where set_task_params_batched / set_residual_states gave rows (TaskRows runs
    rollout_splines_batched, which the candidates above go through, environment by environment)"""
