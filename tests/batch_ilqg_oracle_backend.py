"""Test-only stand-in for capi.Context.rollout_feedback_batched on the CPU oracle, over batch_oracle_backend.py's BatchOracleContext:
a batched call is E x pyoracle.rollout_feedback with environment e's state, clock, mocap pose and row of every array, concatenated
environment-major. The plain set_state, transition_fd, cost_derivatives and backward_pass of a fleet planner's sequential middle are
OracleContext's. Never used by the product."""
import numpy as np

from batch_oracle_backend import BatchOracleContext
from mujoco_mpc_amd import capi
from oracle import pyoracle


class BatchILQGOracleContext(BatchOracleContext):
    def rollout_feedback_batched(self, horizon, mode, representation, use_state, times, states, actions, gains, improvement, alpha,
                                 num_envs=None, n_per_env=None):
        al = np.asarray(alpha, float)
        E, n = al.shape
        assert E == self.E and n >= 1
        rows = [np.asarray(x, float).reshape(E, -1, *np.asarray(x).shape[2:]) for x in (times, states, actions, gains, improvement)]
        outs = []
        for e in range(E):
            mocap = None if self.env_mocap is None or self.env_mocap.shape[1] == 0 else self.env_mocap[e]
            outs.append(pyoracle.rollout_feedback(self.pm, self.pt, self.env_states[e], float(self.env_times[e]), mocap, horizon, mode,
                                                  representation, use_state, *[r[e] for r in rows], al[e], num_threads=self.threads))
        self.out = {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in outs[0]}
        self.N, self.H, self.P, self.n_per_env = E * n, horizon, 0, n

    def fetch_trajectory(self, i):
        """OracleContext's, without reading the plain state's size: a batched call leaves the state of set_state alone"""
        m = self.pm.struct
        tr = capi.Trajectory(m.nq + m.nv + m.na, self.nu, self.pt.struct.num_residual, self.pt.struct.num_trace, self.H)
        for name in ("states", "actions", "times", "residual", "costs", "trace"):
            getattr(tr, name)[...] = self.out[name][i]
        tr.total_return, tr.failure = float(self.out["total_return"][i]), bool(self.out["failure"][i])
        return tr
