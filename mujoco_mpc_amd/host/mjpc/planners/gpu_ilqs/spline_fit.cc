#include "spline_fit.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "../../utilities.h"

namespace mjpc {

int SplineFit::Fit(spline::SplineInterpolation interpolation, int num_nodes, const double* node_times, int num_steps,
                   const double* step_times, const double* actions, int nu, const double* ctrlrange, double* values) {
  const int P = num_nodes, T = num_steps;
  if (P < 1 || T < 1 || nu < 1) throw std::invalid_argument("spline fit: needs at least one node, one step and one control");
  for (int k = 1; k < P; k++)
    if (!(node_times[k] > node_times[k - 1])) throw std::invalid_argument("spline fit: node times must be strictly increasing");

  // M (T x P): the spline whose node k holds the k-th unit vector, sampled at every step time
  spline::TimeSpline basis(P, interpolation);
  unit_.assign(P, 0.0);
  for (int k = 0; k < P; k++) {
    unit_[k] = 1.0;
    basis.AddNode(node_times[k], spline::Span<const double>(unit_.data(), P));
    unit_[k] = 0.0;
  }
  mapping_.resize((size_t)T * P);
  for (int t = 0; t < T; t++) basis.Sample(step_times[t], spline::Span<double>(mapping_.data() + (size_t)t * P, P));

  // reached nodes
  std::vector<double> norm(P, 0.0);
  for (int t = 0; t < T; t++)
    for (int k = 0; k < P; k++) norm[k] += mapping_[(size_t)t * P + k] * mapping_[(size_t)t * P + k];
  const double max_norm = std::sqrt(*std::max_element(norm.begin(), norm.end()));
  reached.assign(P, 1);
  index_.clear();
  for (int k = 0; k < P; k++) {
    if (std::sqrt(norm[k]) <= kUnreachedTolerance * max_norm) reached[k] = 0;
    else index_.push_back(k);
  }
  const int R = (int)index_.size();
  num_unreached = P - R;

  // unreached nodes: the action at the nearest step time
  solution_.assign((size_t)P * nu, 0.0);
  for (int k = 0; k < P; k++) {
    if (reached[k]) continue;
    int nearest = 0;
    for (int t = 1; t < T; t++)
      if (std::fabs(step_times[t] - node_times[k]) < std::fabs(step_times[nearest] - node_times[k])) nearest = t;
    std::copy_n(actions + (size_t)nearest * nu, nu, solution_.data() + (size_t)k * nu);
  }

  // normal equations of the reached nodes: (M_R^T M_R) x_R = M_R^T (a - M_U x_U), one right-hand side per control
  normal_.assign((size_t)R * R, 0.0);
  rhs_.assign((size_t)R * nu, 0.0);
  std::vector<double> residual(nu);
  for (int t = 0; t < T; t++) {
    const double* row = mapping_.data() + (size_t)t * P;
    std::copy_n(actions + (size_t)t * nu, nu, residual.data());
    if (num_unreached)
      for (int k = 0; k < P; k++)
        if (!reached[k])
          for (int j = 0; j < nu; j++) residual[j] -= row[k] * solution_[(size_t)k * nu + j];
    for (int r = 0; r < R; r++) {
      const double w = row[index_[r]];
      for (int c = 0; c <= r; c++) normal_[(size_t)r * R + c] += w * row[index_[c]];
      for (int j = 0; j < nu; j++) rhs_[(size_t)r * nu + j] += w * residual[j];
    }
  }

  // Cholesky, lower triangle in place
  for (int r = 0; r < R; r++) {
    for (int c = 0; c <= r; c++) {
      double s = normal_[(size_t)r * R + c];
      for (int k = 0; k < c; k++) s -= normal_[(size_t)r * R + k] * normal_[(size_t)c * R + k];
      if (r == c) {
        if (!(s > 0.0) || !std::isfinite(s)) return kSplineFitNotPositiveDefinite;
        normal_[(size_t)r * R + r] = std::sqrt(s);
      } else {
        normal_[(size_t)r * R + c] = s / normal_[(size_t)c * R + c];
      }
    }
  }
  // L y = b, then L^T x = y, every control at once
  for (int r = 0; r < R; r++)
    for (int j = 0; j < nu; j++) {
      double s = rhs_[(size_t)r * nu + j];
      for (int k = 0; k < r; k++) s -= normal_[(size_t)r * R + k] * rhs_[(size_t)k * nu + j];
      rhs_[(size_t)r * nu + j] = s / normal_[(size_t)r * R + r];
    }
  for (int r = R - 1; r >= 0; r--)
    for (int j = 0; j < nu; j++) {
      double s = rhs_[(size_t)r * nu + j];
      for (int k = r + 1; k < R; k++) s -= normal_[(size_t)k * R + r] * rhs_[(size_t)k * nu + j];
      rhs_[(size_t)r * nu + j] = s / normal_[(size_t)r * R + r];
    }
  for (int r = 0; r < R; r++) std::copy_n(rhs_.data() + (size_t)r * nu, nu, solution_.data() + (size_t)index_[r] * nu);

  if (ctrlrange)
    for (int k = 0; k < P; k++) Clamp(solution_.data() + (size_t)k * nu, ctrlrange, nu);
  std::copy(solution_.begin(), solution_.end(), values);
  return num_unreached ? kSplineFitUnreached : kSplineFitOk;
}

}  // namespace mjpc
