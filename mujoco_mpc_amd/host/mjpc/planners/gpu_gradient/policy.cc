#include "policy.h"

#include <algorithm>

#include "../../trajectory.h"
#include "../../utilities.h"

namespace mjpc {

// gradient/policy.cc:29-56. gradient_spline_points defaults to kMaxTrajectoryHorizon in the reference, whose spline mappings
// are sized for kMaxGradientSplinePoints: the port clamps it to [1, kMaxGradientSplinePoints]
void GpuGradientPolicy::Allocate(const mjModel* m, const Task& task, int horizon) {
  model = m;
  k.resize((size_t)m->nu * kMaxTrajectoryHorizon);
  parameters.resize((size_t)m->nu * kMaxTrajectoryHorizon);
  parameter_update.resize((size_t)m->nu * kMaxTrajectoryHorizon);
  times.resize(kMaxTrajectoryHorizon);
  num_parameters = m->nu * kMaxTrajectoryHorizon;
  num_spline_points = std::clamp(GetNumberOrDefault(kMaxTrajectoryHorizon, m, "gradient_spline_points"), 1, kMaxGradientSplinePoints);
  representation = (spline::SplineInterpolation)GetNumberOrDefault((int)spline::kLinearSpline, m, "gradient_representation");
}

// gradient/policy.cc:59-78
void GpuGradientPolicy::Reset(int horizon, const double* initial_repeated_action) {
  const int nu = model->nu;
  std::fill(k.begin(), k.begin() + (size_t)horizon * nu, 0.0);
  if (initial_repeated_action)
    for (int i = 0; i < horizon; i++) std::copy_n(initial_repeated_action, nu, parameters.begin() + (size_t)i * nu);
  else
    std::fill(parameters.begin(), parameters.begin() + (size_t)horizon * nu, 0.0);
  std::fill(parameter_update.begin(), parameter_update.begin() + (size_t)horizon * nu, 0.0);
  std::fill(times.begin(), times.begin() + horizon, 0.0);
}

// gradient/policy.cc:81-103 with the node slopes of TimeSpline (spline.cc:269-287)
void GpuGradientPolicy::Action(double* action, const double* state, double time) const {
  const int nu = model->nu, P = num_spline_points;
  const double* xs = times.data();
  const double* ys = parameters.data();
  int b[2];
  FindInterval(b, xs, time, P);
  if (b[0] == b[1] || representation == spline::kZeroSpline) {
    std::copy_n(ys + (size_t)nu * b[0], nu, action);
  } else if (representation == spline::kLinearSpline) {
    LinearInterpolation(action, time, xs, ys, nu, P);
  } else {
    const double tl = xs[b[0]], tu = xs[b[1]], s = (time - tl) / (tu - tl);
    const double c0 = 2.0 * s * s * s - 3.0 * s * s + 1.0, c1 = (s * s * s - 2.0 * s * s + s) * (tu - tl);
    const double c2 = -2.0 * s * s * s + 3 * s * s, c3 = (s * s * s - s * s) * (tu - tl);
    auto slope = [&](int node, int i) {
      const auto secant = [&](int hi, int lo) { return (ys[(size_t)nu * hi + i] - ys[(size_t)nu * lo + i]) / (xs[hi] - xs[lo]); };
      if (node == 0) return secant(1, 0);
      if (node == P - 1) return secant(P - 1, P - 2);
      return 0.5 * secant(node + 1, node) + 0.5 * secant(node, node - 1);
    };
    for (int i = 0; i < nu; i++)
      action[i] = c0 * ys[(size_t)nu * b[0] + i] + c1 * slope(b[0], i) + c2 * ys[(size_t)nu * b[1] + i] + c3 * slope(b[1], i);
  }
  Clamp(action, model->actuator_ctrlrange, nu);
}

// gradient/policy.cc:106-126
void GpuGradientPolicy::CopyFrom(const GpuGradientPolicy& policy, int horizon) {
  std::copy_n(policy.k.begin(), (size_t)horizon * model->nu, k.begin());
  std::copy_n(policy.parameters.begin(), policy.num_parameters, parameters.begin());
  std::copy_n(policy.parameter_update.begin(), policy.num_parameters, parameter_update.begin());
  std::copy_n(policy.times.begin(), policy.num_spline_points, times.begin());
  num_spline_points = policy.num_spline_points;
  num_parameters = policy.num_parameters;
  representation = policy.representation;
}

// gradient/policy.cc:129-135
void GpuGradientPolicy::CopyParametersFrom(const std::vector<double>& src_parameters, const std::vector<double>& src_times) {
  std::copy_n(src_parameters.begin(), (size_t)num_spline_points * model->nu, parameters.begin());
  std::copy_n(src_times.begin(), num_spline_points, times.begin());
}

}  // namespace mjpc
