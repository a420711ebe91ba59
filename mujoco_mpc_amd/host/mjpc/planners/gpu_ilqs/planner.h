// mjpc::GpuILQSPlanner -- iLQS, the sampling / iLQG hybrid, on the device planners.
//
// Drop-in for mjpc::iLQSPlanner (mjpc/planners/ilqs/planner.{h,cc}). Both halves are the device planners, each with its own
// context: GpuSamplingPlanner (noise + rollouts + argmin, one launch) and GpuILQGPlanner (feedback rollouts, FD and cost
// derivatives, the MFMA Riccati pass). iLQS itself launches nothing: it drives NominalTrajectory / Iteration of the iLQG half
// directly, and the one piece of new arithmetic -- the least-squares fit of the sampling spline to iLQG's nominal actions
// (SplineFit) -- runs on the host. Both halves plan on one model: agent_differentiable (default 1, agent.cc:156-164) is read once
// and handed to both. Deliberate differences:
//   * the conversion takes effect: without a sliding plan the fit is installed as winner_policy.plan, which
//     GpuSamplingPlanner::UpdateNominalPolicy resamples, at the node times that update uses (spacing /P zero-order, /(P-1)
//     otherwise, nominal_time += shift), so candidate 0 of the next sampling launch is exactly the fit. The reference writes
//     sampling.policy.plan (planner.cc:162-169), which UpdateNominalPolicy then overwrites with its own stale winner. With
//     sampling_sliding_plan = 1 the reference's conversion already works and is followed: policy.plan, (P-1) spacing;
//   * rank-deficient fits are defined: an unreached node (SplineFit::kUnreachedTolerance) takes the nominal action at the nearest
//     step time and the others solve the reduced system; if that is still not positive definite the sampling nominal of this
//     iteration is kept and fit_status says so (the reference's mju_cholFactor(..., 0) gives non-finite parameters -- Particle,
//     11 cubic nodes for 10 actions, is one such task);
//   * an iLQG iteration that stops early (failed backward pass, every line-search rollout failed) never makes iLQG active
//     (GpuILQGPlanner::iteration_completed); the reference compares stale returns there;
//   * no cap on the number of spline points (the reference's mappings hold 25).
#pragma once
#include <atomic>
#include <cstdint>
#include <vector>

#include "../gpu_ilqg/planner.h"
#include "../gpu_sampling/planner.h"
#include "../planner.h"
#include "spline_fit.h"

namespace mjpc {

class GpuILQSPlanner : public Planner {
 public:
  enum ActivePolicy : int { kSampling = 0, kiLQG = 1 };

  explicit GpuILQSPlanner(int device = 0, int precision = 64, std::uint64_t seed = 0)
      : sampling(device, precision, seed), ilqg(device, precision) {}
  ~GpuILQSPlanner() override = default;

  void Initialize(mjModel* model, const Task& task) override;
  void Allocate() override;
  void Reset(int horizon, const double* initial_repeated_action = nullptr) override;
  void SetState(const State& state) override;
  void OptimizePolicy(int horizon, ThreadPool& pool) override;
  void NominalTrajectory(int horizon, ThreadPool& pool) override;
  void ActionFromPolicy(double* action, const double* state, double time, bool use_previous = false) override;
  const Trajectory* BestTrajectory() override;
  void Traces(mjvScene* scn) override {}
  void GUI(mjUI& ui) override {}
  void Plots(mjvFigure* fig_planner, mjvFigure* fig_timer, int planner_shift, int timer_shift, int planning,
             int* shift) override {}
  int NumParameters() override { return sampling.NumParameters() + ilqg.NumParameters(); }

  // ----- members (names as in the reference) ----- //
  GpuSamplingPlanner sampling;
  GpuILQGPlanner ilqg;
  std::atomic<int> active_policy{kSampling}, previous_active_policy{kSampling};  // read by the agent thread

  // the last OptimizePolicy
  bool ilqg_ran = false;            // sampling did not win, so the iLQG iteration ran
  int fit_status = kSplineFitNone;  // SplineFitStatus of the conversion (kSplineFitNone: iLQG was not active before)
  int fit_unreached = 0;
  // the last conversion: node times (P) and values (P x nu), and the step times (T-1) and actions ((T-1) x nu) it fitted
  std::vector<double> fit_times, fit_values, fit_step_times, fit_actions;
  // per-stage times [us]: iLQG nominal, the fit, sampling, the sampling -> iLQG handoff, the iLQG iteration
  double nominal_compute_time = 0, fit_compute_time = 0, sampling_compute_time = 0, handoff_compute_time = 0,
         iteration_compute_time = 0;

 private:
  void Optimize(int horizon, ThreadPool& pool);
  void ConvertPolicy(int horizon);
  SplineFit fit_;
};

}  // namespace mjpc
