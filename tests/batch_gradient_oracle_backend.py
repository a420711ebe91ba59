"""Test-only stand-in for capi.Context.gradient_step_batched on the CPU oracle, over batch_oracle_backend.py's BatchOracleContext:
environment e's derivative chain is pyoracle.transition_fd at the evaluated steps with that environment's mocap pose, the skip
interpolation of planners.model_derivatives, the zeroed last step, the oracle's cost derivatives and gradient_reference.gradient_pass
-- the calls a GpuGradientPlanner on OracleGradientContext makes, one environment after the other. Never used by the product."""
import numpy as np

from batch_oracle_backend import BatchOracleContext
from gradient_reference import gradient_pass
from oracle import pyoracle


def interpolate(evaluate, T, arrays):
    """planners.model_derivatives' interpolation of arrays given at the evaluated steps to all T steps (the same operations)"""
    if len(evaluate) == T:
        return list(arrays)
    full = [np.zeros((T,) + x.shape[1:]) for x in arrays]
    ev = np.array(evaluate)
    for t in range(T):
        k = int(np.searchsorted(ev, t, side="right")) - 1
        e0 = k
        e1 = min(k + 1, len(ev) - 1)
        tt = 0.0 if (ev[e0] == t or e0 == e1) else (t - ev[e0]) / (ev[e1] - ev[e0])
        for f, x in zip(full, arrays):
            f[t] = x[e0] * (1.0 - tt) + x[e1] * tt
    return full


class BatchGradientOracleContext(BatchOracleContext):
    def gradient_step_batched(self, num_envs, candidate, T, evaluate, eps, centered, representation, node_times, with_matrices=False):
        E, n = int(num_envs), self.n_per_env
        assert E == self.E and E * n == self.N and 0 <= candidate < n and 2 <= T <= self.H
        ev = [int(i) for i in evaluate]
        nt = np.asarray(node_times, float).reshape(E, -1)
        keys = ("nominal_return", "k", "gradient", "dV", "A", "B", "cx", "cu")
        out = {key: [] for key in keys}
        for e in range(E):
            c = e * n + candidate
            states, actions, times = self.out["states"][c], self.out["actions"][c], self.out["times"][c]
            mocap = None if self.env_mocap is None or self.env_mocap.shape[1] == 0 else self.env_mocap[e]
            A, B, C, D = interpolate(ev, T, pyoracle.transition_fd(self.pm, self.pt, states[ev], times[ev], actions[ev], eps, centered,
                                                                   mocap=mocap, num_threads=self.threads))
            A[T - 1] = 0; B[T - 1] = 0; D[T - 1] = 0
            cx, cu, _, _, _ = pyoracle.cost_derivatives(self.pt, np.asarray(self.out["residual"][c][:T]), np.asarray(C), np.asarray(D))
            g = gradient_pass(A, B, cx, cu, representation, nt[e], times[:T])
            for key, v in zip(keys, (float(self.out["total_return"][c]), g["k"], g["gradient"], g["dV"], A, B, cx, cu)):
                out[key].append(v)
        return {key: np.array(v) for key, v in out.items() if with_matrices or key in keys[:4]}
