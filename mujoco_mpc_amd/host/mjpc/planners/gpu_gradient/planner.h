// mjpc::GpuGradientPlanner -- the Gradient planner with its device work on an MI355X.
//
// Drop-in for mjpc::GradientPlanner (mjpc/planners/gradient/planner.{h,cc}), settings.max_rollout = 1 as shipped. Behind
// include/mjpcx.h:
//   NominalTrajectory / Rollouts        gradient/planner.cc:300-311, 384-418 -> mjpcx_rollout_splines (one launch each)
//   ModelDerivatives::Compute           model_derivatives.cc:45-165         -> mjpcx_transition_fd (GpuModelDerivatives)
//   CostDerivatives::Compute            cost_derivatives.cc:112-230         -> mjpcx_cost_derivatives
//   Gradient::Compute + M^T k           gradient.cc:43-108, spline_mapping.cc -> mjpcx_gradient_pass (one launch)
// On the host, as in the reference: ResamplePolicy (planner.cc:355-381), the line-search steps, the winner selection and the
// policy bookkeeping. Deliberate differences:
//   * failed rollouts are skipped in the selection (the reference has no failure concept), as GpuILQGPlanner::BestRollout does;
//   * gradient_spline_points is clamped to [1, kMaxGradientSplinePoints = 25] (the size the reference's mappings have); with one
//     point there is no node spacing to compute (the reference's time_shift is x / 0 there, and unused);
//   * num_trajectory is not capped at kMaxTrajectory = 128;
//   * the policy samples its spline as the rollout kernels do (GpuGradientPolicy::Action).
#pragma once
#include <cstdint>
#include <memory>
#include <shared_mutex>
#include <vector>

#include "../../gpu/context.h"
#include "../gpu_model_derivatives.h"
#include "../planner.h"
#include "policy.h"
#include "settings.h"

namespace mjpc {

class GpuGradientPlanner : public Planner {
 public:
  explicit GpuGradientPlanner(int device = 0, int precision = 64) : device_(device), precision_(precision) {}
  ~GpuGradientPlanner() override = default;

  void Initialize(mjModel* model, const Task& task) override;
  void Allocate() override;
  void Reset(int horizon, const double* initial_repeated_action = nullptr) override;
  void SetState(const State& state) override;
  void OptimizePolicy(int horizon, ThreadPool& pool) override;
  void NominalTrajectory(int horizon, ThreadPool& pool) override;
  void ActionFromPolicy(double* action, const double* state, double time, bool use_previous = false) override;
  void ResamplePolicy(int horizon);
  void Rollouts(int horizon, ThreadPool& pool);
  const Trajectory* BestTrajectory() override;
  void Traces(mjvScene* scn) override {}
  void GUI(mjUI& ui) override {}
  void Plots(mjvFigure* fig_planner, mjvFigure* fig_timer, int planner_shift, int timer_shift, int planning,
             int* shift) override {}
  int NumParameters() override { return policy.num_spline_points * policy.model->nu; }
  gpu::Context* context() { return ctx_.get(); }

  // ----- members (names as in the reference) ----- //
  mjModel* model = nullptr;
  const Task* task = nullptr;
  std::vector<double> state, mocap, userdata;
  double time = 0;
  GpuGradientPolicy policy;             // guarded by mtx_
  GpuGradientPolicy previous_policy;
  GpuGradientPolicy candidate_policy0;  // candidate_policy[0]: the resampled nominal, then the winner
  Trajectory trajectory0;               // trajectory[0]: the nominal rollout, then the winner's
  int dim_state = 0, dim_state_derivative = 0, dim_action = 0, dim_sensor = 0;
  int num_trajectory = 0;
  std::vector<double> linesearch_steps;
  int winner = -1;
  GradientPlannerSettings settings;
  double dV[2] = {0, 0};
  double action_step = 0, expected = 0, improvement = 0, surprise = 0;
  double nominal_compute_time = 0, model_derivative_compute_time = 0, cost_derivative_compute_time = 0,
         rollouts_compute_time = 0, gradient_compute_time = 0, policy_update_compute_time = 0;
  double gradient_kernel_ms = 0;  // HIP-event time of the last mjpcx_gradient_pass
  int derivative_skip_ = 0;
  mutable std::shared_mutex mtx_;

 private:
  int device_, precision_;
  std::unique_ptr<gpu::Context> ctx_;
  GpuModelDerivatives model_derivative_;
  std::vector<double> cx_, cu_, cxx_, cxu_, cuu_, Vx_;
  std::vector<double> parameters_scratch_, times_scratch_, nodes_, returns_;
  std::vector<std::int32_t> failure_;
};

}  // namespace mjpc
