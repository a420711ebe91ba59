#include "gpu_model_derivatives.h"

#include <algorithm>

namespace mjpc {

void GpuModelDerivatives::Compute(gpu::Context* ctx, const Trajectory& tr, int T, int skip, double fd_tolerance, bool centered,
                                  int n, int m, int nr, int ds) {
  const int s = skip + 1;
  std::vector<int> evaluate;
  evaluate.push_back(0);
  for (int t = s; t < T - s; t += s) evaluate.push_back(t);
  evaluate.push_back(T - 2);
  evaluate.push_back(T - 1);
  std::sort(evaluate.begin(), evaluate.end());
  evaluate.erase(std::unique(evaluate.begin(), evaluate.end()), evaluate.end());
  evaluate.erase(std::remove_if(evaluate.begin(), evaluate.end(), [T](int e) { return e < 0 || e >= T; }), evaluate.end());
  const int E = (int)evaluate.size();
  etimes_.resize(E); estates_.resize((size_t)E * ds); eactions_.resize((size_t)E * m);
  for (int k = 0; k < E; k++) {
    const int t = evaluate[k];
    etimes_[k] = tr.times[t];
    std::copy_n(tr.states.begin() + (size_t)t * ds, ds, estates_.begin() + (size_t)k * ds);
    std::copy_n(tr.actions.begin() + (size_t)t * m, m, eactions_.begin() + (size_t)k * m);
  }
  const size_t sA = (size_t)n * n, sB = (size_t)n * m, sC = (size_t)nr * n, sD = (size_t)nr * m;
  eA_.resize(E * sA); eB_.resize(E * sB); eC_.resize(E * sC); eD_.resize(E * sD);
  ctx->Check(mjpcx_transition_fd(ctx->handle(), E, etimes_.data(), estates_.data(), eactions_.data(), fd_tolerance, centered,
                                 eA_.data(), eB_.data(), eC_.data(), eD_.data()));
  A.assign(T * sA, 0.0); B.assign(T * sB, 0.0); C.assign(T * sC, 0.0); D.assign(T * sD, 0.0);
  int k = 0;
  for (int t = 0; t < T; t++) {
    while (k + 1 < E && evaluate[k + 1] <= t) k++;
    const int e0 = k, e1 = std::min(k + 1, E - 1);
    const double tt = (evaluate[e0] == t || e0 == e1) ? 0.0 : double(t - evaluate[e0]) / double(evaluate[e1] - evaluate[e0]);
    auto mix = [&](std::vector<double>& full, const std::vector<double>& ev, size_t sz) {
      for (size_t i = 0; i < sz; i++) full[t * sz + i] = ev[e0 * sz + i] * (1.0 - tt) + ev[e1 * sz + i] * tt;
    };
    mix(A, eA_, sA); mix(B, eB_, sB); mix(C, eC_, sC); mix(D, eD_, sD);
  }
  std::fill(A.begin() + (T - 1) * sA, A.end(), 0.0);
  std::fill(B.begin() + (T - 1) * sB, B.end(), 0.0);
  std::fill(D.begin() + (T - 1) * sD, D.end(), 0.0);
}

}  // namespace mjpc
