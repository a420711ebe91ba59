"""Test-only stand-in for capi.Context.mppi_update_batched backed by the CPU oracle, on top of batch_oracle_backend.py: the MPPI update
of every environment in numpy, in the arithmetic and the summation order of mjpcx_mppi_update_batched (mppi_cases.emulate_mppi: numpy's
exp in the place of the device's). `nan_envs`: environments whose returns the update sees as NaN (an injected all-NaN member). Never
used by the product."""
import numpy as np

import mppi_cases as mc
from batch_oracle_backend import BatchOracleContext


class BatchMppiOracleContext(BatchOracleContext):
    nan_envs = ()

    def mppi_update_batched(self, num_envs, temperature, ref_candidate=-1, want_weights=False):
        n = self.n_per_env
        lam = np.broadcast_to(np.asarray(temperature, float).reshape(-1), (num_envs,))
        if num_envs != self.E or not (np.all(np.isfinite(lam)) and np.all(lam > 0)) or not -1 <= ref_candidate < n:
            raise ValueError("mppi_update_batched: another fleet size, a temperature that is not finite and > 0, or ref_candidate outside -1..n-1")
        r = self.out["total_return"].reshape(num_envs, n).copy()
        for e in self.nan_envs:
            r[e] = np.nan
        nodes = self.nodes.reshape(num_envs, n, self.P * self.nu)
        envs = [mc.emulate_mppi(r[e], lam[e], nodes[e], ref_candidate) for e in range(num_envs)]
        out = {k: np.array([o[k] for o in envs]) for k in ("best_return", "ref_return", "weight_sum", "effective_samples")}
        out["index"] = np.array([o["index"] for o in envs], np.int32)
        out["valid"] = np.array([o["valid"] for o in envs], np.int32)
        out["mean"] = np.stack([o["mean"].reshape(self.P, self.nu) for o in envs])
        out["weights"] = np.stack([o["weights"] for o in envs]) if want_weights else None
        return out
