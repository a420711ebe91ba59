// mjpc::GpuGradientPolicy (mjpc/planners/gradient/policy.{h,cc}): P spline points of nu parameters each, zero-order, linear or
// cubic, clamped to ctrlrange.
#pragma once
#include <vector>

#include "../../spline/spline.h"
#include "../policy.h"

namespace mjpc {

inline constexpr int kMaxGradientSplinePoints = 25;  // gradient/spline_mapping.h:27

class GpuGradientPolicy : public Policy {
 public:
  void Allocate(const mjModel* model, const Task& task, int horizon) override;
  void Reset(int horizon, const double* initial_repeated_action = nullptr) override;
  // the spline the rollout kernels sample (TimeSpline::Sample, spline.cc:103-156), then Clamp. Equal to the reference's
  // Zero / Linear / CubicInterpolation except for a cubic on two points, where the reference's FiniteDifferenceSlope takes the
  // slope at the second point as 0 and TimeSpline (and the reference's own CubicSplineMapping) the secant
  void Action(double* action, const double* state, double time) const override;
  void CopyFrom(const GpuGradientPolicy& policy, int horizon);
  void CopyParametersFrom(const std::vector<double>& src_parameters, const std::vector<double>& src_times);

  const mjModel* model = nullptr;
  std::vector<double> k;                 // action improvement, T x nu
  std::vector<double> parameters;        // P x nu
  std::vector<double> parameter_update;  // P x nu
  std::vector<double> times;             // P
  int num_parameters = 0;
  int num_spline_points = 0;
  spline::SplineInterpolation representation = spline::kLinearSpline;
};

}  // namespace mjpc
