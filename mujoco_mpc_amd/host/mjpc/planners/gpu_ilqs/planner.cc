#include "planner.h"

#include <chrono>
#include <mutex>

#include "../../utilities.h"

namespace mjpc {

using spline::TimeSpline;

void GpuILQSPlanner::Initialize(mjModel* model, const Task& task) {
  sampling.Initialize(model, task);
  ilqg.Initialize(model, task);
}

void GpuILQSPlanner::Allocate() {
  // iLQS is gradient-based (agent.cc:156-164): both halves plan on the differentiable copy unless the task says otherwise
  const bool differentiable = GetNumberOrDefault(1, sampling.model, "agent_differentiable") != 0;
  sampling.differentiable = differentiable;
  ilqg.differentiable = differentiable ? 1 : 0;
  sampling.Allocate();
  ilqg.Allocate();
}

void GpuILQSPlanner::Reset(int horizon, const double* initial_repeated_action) {
  sampling.Reset(horizon, initial_repeated_action);
  ilqg.Reset(horizon, initial_repeated_action);
  active_policy = kSampling;
  previous_active_policy = kSampling;
  ilqg_ran = false;
  fit_status = kSplineFitNone;
  fit_unreached = 0;
  fit_times.clear(); fit_values.clear(); fit_step_times.clear(); fit_actions.clear();
  nominal_compute_time = fit_compute_time = sampling_compute_time = handoff_compute_time = iteration_compute_time = 0.0;
}

void GpuILQSPlanner::SetState(const State& state) {
  sampling.SetState(state);
  ilqg.SetState(state);
}

// iLQG's nominal actions -> sampling spline (ilqs/planner.cc:90-170), at the node times the sampling update uses
void GpuILQSPlanner::ConvertPolicy(int horizon) {
  const mjModel* m = sampling.model;
  const int nu = m->nu, P = sampling.policy.num_spline_points, steps = horizon - 1;
  const spline::SplineInterpolation interpolation = sampling.interpolation_;
  const double time_horizon = (horizon - 1) * sampling.PlanningTimestep();
  const double shift = !sampling.sliding_plan_ && interpolation == spline::kZeroSpline ? mju_max(time_horizon / P, 1.0e-5)
                                                                                      : mju_max(time_horizon / (P - 1), 1.0e-5);
  fit_times.resize(P);
  double nominal_time = sampling.time;
  for (int k = 0; k < P; k++) {
    fit_times[k] = nominal_time;
    nominal_time += shift;
  }
  const Trajectory& tr = ilqg.candidate_policy0.trajectory;
  fit_step_times.assign(tr.times.begin(), tr.times.begin() + steps);
  fit_actions.assign(tr.actions.begin(), tr.actions.begin() + (size_t)steps * nu);
  fit_values.assign((size_t)P * nu, 0.0);
  fit_status = fit_.Fit(interpolation, P, fit_times.data(), steps, fit_step_times.data(), fit_actions.data(), nu,
                        m->actuator_ctrlrange, fit_values.data());
  fit_unreached = fit_.num_unreached;
  if (fit_status == kSplineFitNotPositiveDefinite) return;  // keep this iteration's sampling nominal

  TimeSpline plan(nu, interpolation);
  plan.Reserve(P);
  for (int k = 0; k < P; k++) plan.AddNode(fit_times[k], spline::Span<const double>(fit_values.data() + (size_t)k * nu, nu));
  if (sampling.sliding_plan_) {
    const std::unique_lock<std::shared_mutex> lock(sampling.mtx_);
    sampling.policy.plan = plan;
  } else {
    sampling.winner_policy.plan = plan;
    sampling.winner_policy.num_spline_points = P;
  }
}

// A stage that throws (the iLQG kernels of the wavefront family are fp64 only, so an fp32 A1 fails after its sampling launch) leaves
// the policies as they were: the sampling half's are restored and the iLQG half only writes its own at the end of Iteration.
void GpuILQSPlanner::OptimizePolicy(int horizon, ThreadPool& pool) {
  const int active = active_policy.load(), previous = previous_active_policy.load();
  SamplingPolicy policy, previous_policy, winner_policy;
  {
    const std::shared_lock<std::shared_mutex> lock(sampling.mtx_);
    policy = sampling.policy;
    previous_policy = sampling.previous_policy;
  }
  winner_policy = sampling.winner_policy;
  try {
    Optimize(horizon, pool);
  } catch (...) {
    {
      const std::unique_lock<std::shared_mutex> lock(sampling.mtx_);
      sampling.policy = policy;
      sampling.previous_policy = previous_policy;
    }
    sampling.winner_policy = winner_policy;
    active_policy = active;
    previous_active_policy = previous;
    throw;
  }
}

// ilqs/planner.cc:87-214
void GpuILQSPlanner::Optimize(int horizon, ThreadPool& pool) {
  const int previous = active_policy.load();
  previous_active_policy = previous;
  ilqg.num_trajectory_ = ilqg.num_rollouts_gui_;  // UpdateNumTrajectoriesFromGUI, as GpuILQGPlanner::OptimizePolicy does
  ilqg_ran = false;
  fit_status = kSplineFitNone;
  fit_unreached = 0;
  nominal_compute_time = fit_compute_time = handoff_compute_time = iteration_compute_time = 0.0;

  if (previous == kiLQG) {
    auto start = std::chrono::steady_clock::now();
    ilqg.NominalTrajectory(horizon, pool);
    nominal_compute_time = GetDuration(start);
    start = std::chrono::steady_clock::now();
    ConvertPolicy(horizon);
    fit_compute_time = GetDuration(start);
  }

  auto start = std::chrono::steady_clock::now();
  sampling.OptimizePolicy(horizon, pool);
  sampling_compute_time = GetDuration(start);

  // winner 0 is the nominal: surely no improvement
  const double sampling_reference =
      previous == kSampling ? sampling.nominal_return : ilqg.candidate_policy0.trajectory.total_return;
  if (sampling.winner > 0 && sampling.best_return < sampling_reference) {
    if (active_policy == kSampling) ilqg.nominal_compute_time = 0.0;
    ilqg.model_derivative_compute_time = ilqg.cost_derivative_compute_time = ilqg.backward_pass_compute_time = 0.0;
    ilqg.rollouts_compute_time = ilqg.policy_update_compute_time = 0.0;
    active_policy = kSampling;
    return;
  }

  if (previous == kSampling) {  // iLQG starts from the sampling nominal: trajectory[0] of the sampling launch
    start = std::chrono::steady_clock::now();
    sampling.context()->FetchTrajectory(0, &ilqg.candidate_policy0.trajectory);
    // its NominalTrajectory did not run, so its context has not seen this plan's state (the derivatives read its mocap)
    gpu::Context* ctx = ilqg.context();
    ctx->Check(mjpcx_set_state(ctx->handle(), ilqg.state.data(), ilqg.time, ilqg.mocap.data(), ilqg.userdata.data()));
    handoff_compute_time = GetDuration(start);
  }

  start = std::chrono::steady_clock::now();
  ilqg.Iteration(horizon, pool);
  iteration_compute_time = GetDuration(start);
  ilqg_ran = true;

  const double ilqg_reference = previous == kSampling ? sampling.best_return : ilqg.linesearch0_return;
  if (ilqg.iteration_completed && ilqg.winner_return < ilqg_reference) active_policy = kiLQG;
  // no improvement either way: both policies were updated, the active one stays
}

void GpuILQSPlanner::NominalTrajectory(int horizon, ThreadPool& pool) {
  if (active_policy == kSampling) sampling.NominalTrajectory(horizon, pool);
  else ilqg.NominalTrajectory(horizon, pool);
}

// ilqs/planner.cc:228-253
void GpuILQSPlanner::ActionFromPolicy(double* action, const double* state, double time, bool use_previous) {
  const int active = active_policy.load(), previous = previous_active_policy.load();
  if (use_previous) {
    if (previous == kSampling) {
      // sampling.OptimizePolicy always ran and always updated the sampling policy
      sampling.ActionFromPolicy(action, state, time, true);
    } else if (active == kSampling) {
      // the last plan stopped after sampling: iLQG was not updated, its current policy is the previous one
      ilqg.ActionFromPolicy(action, state, time, false);
    } else {
      ilqg.ActionFromPolicy(action, state, time, true);
    }
  } else if (active == kSampling) {
    sampling.ActionFromPolicy(action, state, time, false);
  } else {
    ilqg.ActionFromPolicy(action, state, time, false);
  }
}

const Trajectory* GpuILQSPlanner::BestTrajectory() {
  return active_policy == kSampling ? sampling.BestTrajectory() : ilqg.BestTrajectory();
}

}  // namespace mjpc
