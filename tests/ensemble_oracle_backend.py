"""Test-only stand-in for capi.Context.rollout_noise_ensemble / ensemble_best on the CPU oracle, and the score's definition as a plain
Python loop (what the device tests compare mjpcx_ensemble_best with, bit for bit). Hypothesis h of the launch is the parent class's
batched call on a fleet of ONE (batch_task_oracle_backend.TaskRows._each: state h, task row h, and with ModelRows model h) with the SAME
noise seed for every h -- not seed + h. Never used by the product."""
import numpy as np

from batch_model_oracle_backend import ModelBatchOracleContext
from batch_oracle_backend import BatchOracleContext

MAX_HYPOTHESES = 32


def ensemble_scores(returns, tail):
    """returns M x n -> the n scores: the mean of the `tail` largest of a candidate's M returns -- descending, equal values with the lower
    h first, summed in that order with plain fp64 adds starting at the first, divided by tail; NaN if any of the M is NaN"""
    R = np.asarray(returns, float)
    M, n = R.shape
    assert 1 <= tail <= M
    out = np.empty(n)
    for i in range(n):
        vals = [float(R[h, i]) for h in range(M)]
        if any(v != v for v in vals):
            out[i] = np.nan
            continue
        order = sorted(range(M), key=lambda h: -vals[h])      # (a stable sort: equal values, -0.0 and 0.0 among them, keep the lower h first)
        s = vals[order[0]]
        for k in range(1, tail):
            with np.errstate(invalid="ignore"):
                s = float(np.float64(s) + np.float64(vals[order[k]]))
        out[i] = np.float64(s) / np.float64(tail)
    return out


def ensemble_argmin(scores):
    """mjpcx_topk's order: ascending, ties to the lower index, NaN last"""
    best = 0
    for i in range(1, len(scores)):
        a, b = scores[i], scores[best]
        if (a == a and b != b) or a < b:
            best = i
    return best


class EnsembleOracleContext(ModelBatchOracleContext):
    def rollout_noise_ensemble(self, n, horizon, interp, node_times, nominal, ns, num_hypotheses):
        M = int(num_hypotheses)
        if getattr(self, "E", 0) != M:
            raise ValueError(f"rollout_noise_ensemble of {M} hypotheses after set_states of {getattr(self, 'E', 0)}")
        nt = np.tile(np.asarray(node_times, float).reshape(1, -1), (M, 1))
        nom = np.tile(np.asarray(nominal, float).reshape(1, nt.shape[1], self.nu), (M, 1, 1))
        self._each(lambda h: BatchOracleContext.rollout_noise_batched(self, n, horizon, interp, nt[h:h + 1], nom[h:h + 1], ns))

    def ensemble_best(self, num_hypotheses, tail, ref_candidate=0, with_scores=False):
        M, n = int(num_hypotheses), self.n_per_env
        if M > MAX_HYPOTHESES or M * n != self.N or not 1 <= tail <= M or not -1 <= ref_candidate < n:
            raise ValueError("ensemble_best: bad arguments")
        R = self.out["total_return"].reshape(M, n)
        scores = ensemble_scores(R, tail)
        w = ensemble_argmin(scores)
        ref = float(scores[ref_candidate]) if ref_candidate >= 0 else float("nan")
        return w, float(scores[w]), ref, R[:, w].copy(), self.nodes[w].copy(), scores if with_scores else None
