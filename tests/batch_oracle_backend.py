"""Test-only stand-in for the batched entry points of capi.Context (set_states, rollout_noise_batched, rollout_splines_batched,
best_batched) backed by the CPU oracle, in the manner of oracle_backend.py: environment e of a batched call is E single-environment
oracle rollouts, with the noise of seed + e, laid out environment-major. Never used by the product."""
import numpy as np

from mujoco_mpc_amd import capi
from oracle import pyoracle
from oracle_backend import OracleContext


class BatchOracleContext(OracleContext):
    def set_states(self, states, times, mocap=None, userdata=None):
        self.env_states = np.array(states, float).reshape(len(times), -1)
        self.env_times = np.array(times, float).reshape(-1)
        self.E = len(self.env_times)
        self.env_mocap = None if mocap is None else np.array(mocap, float).reshape(self.E, -1)

    @staticmethod
    def _check(n):
        if n < 64 or n % 64:
            raise ValueError(f"n_per_env = {n} must be a positive multiple of 64")

    def _run_batched(self, n, H, interp, times, nodes):
        """times E x P, nodes E x n x P x nu"""
        E, P = self.E, times.shape[1]
        outs = []
        for e in range(E):
            mocap = None if self.env_mocap is None else self.env_mocap[e]
            outs.append(pyoracle.rollout_batch(self.pm, self.pt, self.env_states[e], float(self.env_times[e]), mocap, n, H, P, interp,
                                               times[e], nodes[e], num_threads=self.threads))
        self.out = {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in outs[0]}
        self.nodes = nodes.reshape(E * n, P, self.nu)
        self.state = self.env_states[0]
        self.N, self.H, self.P, self.n_per_env = E * n, H, P, n

    def rollout_splines_batched(self, horizon, interp, node_times, node_values, num_envs=None, n_per_env=None):
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        nv = np.asarray(node_values, float)
        n = nv.size // (self.E * nt.shape[1] * self.nu)
        self._check(n)
        self._run_batched(n, horizon, interp, nt, nv.reshape(self.E, n, nt.shape[1], self.nu))

    def rollout_noise_batched(self, n_per_env, horizon, interp, node_times, nominal, ns, num_envs=None):
        self._check(n_per_env)
        nt = np.asarray(node_times, float).reshape(self.E, -1)
        P = nt.shape[1]
        nom = np.asarray(nominal, float).reshape(self.E, P, self.nu)
        cands = range(ns.candidate_offset, ns.candidate_offset + n_per_env)
        nodes = []
        for e in range(self.E):
            nse = capi.make_noise_spec(seed=ns.seed + e, iteration=ns.iteration, mode=ns.mode, candidate_offset=ns.candidate_offset,
                                       nominal_candidate=ns.nominal_candidate, explore_count=ns.explore_count, std0=ns.std0, std1=ns.std1)
            nodes.append(np.asarray(pyoracle.noise_candidates(self.pm, nse, P, nom[e], cands), float).reshape(n_per_env, P, self.nu))
        self._run_batched(n_per_env, horizon, interp, nt, np.stack(nodes))

    def best_batched(self, num_envs, ref_candidate=0, with_spline=True):
        n = self.n_per_env
        r = self.out["total_return"].reshape(num_envs, n)
        idx = np.array([np.lexsort((np.arange(n), r[e]))[0] for e in range(num_envs)], np.int32)
        best = r[np.arange(num_envs), idx]
        ref = r[:, ref_candidate].copy() if ref_candidate >= 0 else np.full(num_envs, np.nan)
        sp = np.stack([self.nodes[e * n + idx[e]] for e in range(num_envs)])
        return idx, best, ref, sp
