#include "planner.h"

#include <algorithm>
#include <chrono>
#include <mutex>

#include "../../utilities.h"

namespace mjpc {

// gradient/planner.cc:40-62
void GpuGradientPlanner::Initialize(mjModel* m, const Task& t) {
  model = m;
  task = &t;
  dim_state = m->nq + m->nv + m->na;
  dim_state_derivative = 2 * m->nv + m->na;
  dim_action = m->nu;
  dim_sensor = t.num_residual;
  num_trajectory = GetNumberOrDefault(32, m, "gradient_num_trajectory");
}

// gradient/planner.cc:65-105
void GpuGradientPlanner::Allocate() {
  state.resize(dim_state);
  mocap.resize(7 * (size_t)model->nmocap);
  userdata.resize(model->nuserdata);
  for (GpuGradientPolicy* p : {&policy, &previous_policy, &candidate_policy0}) p->Allocate(model, *task, kMaxTrajectoryHorizon);
  trajectory0.Initialize(dim_state, dim_action, task->num_residual, task->num_trace, kMaxTrajectoryHorizon);
  trajectory0.Allocate(kMaxTrajectoryHorizon);
  parameters_scratch_.resize((size_t)model->nu * kMaxTrajectoryHorizon);
  times_scratch_.resize(kMaxTrajectoryHorizon);
  // gradient-based planners plan on the differentiable model copy unless agent_differentiable says otherwise (agent.cc:156-164)
  const bool differentiable = GetNumberOrDefault(1, model, "agent_differentiable") != 0;
  ctx_ = std::make_unique<gpu::Context>(model, *task, device_, precision_, differentiable);
}

// gradient/planner.cc:108-149
void GpuGradientPlanner::Reset(int horizon, const double* initial_repeated_action) {
  std::fill(state.begin(), state.end(), 0.0);
  std::fill(mocap.begin(), mocap.end(), 0.0);
  std::fill(userdata.begin(), userdata.end(), 0.0);
  time = 0.0;
  {
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    policy.Reset(horizon, initial_repeated_action);
    previous_policy.Reset(horizon, initial_repeated_action);
  }
  candidate_policy0.Reset(horizon, initial_repeated_action);
  std::fill(parameters_scratch_.begin(), parameters_scratch_.end(), 0.0);
  std::fill(times_scratch_.begin(), times_scratch_.end(), 0.0);
  trajectory0.Reset(horizon);
  dV[0] = dV[1] = 0;
  action_step = expected = improvement = surprise = 0.0;
  winner = -1;
  derivative_skip_ = GetNumberOrDefault(0, model, "derivative_skip");
}

void GpuGradientPlanner::SetState(const State& s) { s.CopyTo(state.data(), mocap.data(), userdata.data(), &time); }

// gradient/planner.cc:159-327 (settings.max_rollout = 1)
void GpuGradientPlanner::OptimizePolicy(int horizon, ThreadPool& pool) {
  if (num_trajectory < 1) return;  // the reference clamps to kMaxTrajectory = 128 here (lifted)
  const int T = horizon, n = dim_state_derivative, m = dim_action, nu = model->nu;

  // ---- nominal rollout of the resampled policy
  auto start = std::chrono::steady_clock::now();
  policy.num_parameters = nu * policy.num_spline_points;
  {
    const std::shared_lock<std::shared_mutex> lock(mtx_);
    candidate_policy0.CopyFrom(policy, policy.num_spline_points);
  }
  ResamplePolicy(horizon);
  NominalTrajectory(horizon, pool);
  const double c_prev = trajectory0.total_return;
  nominal_compute_time = GetDuration(start);
  double c_best = c_prev;

  // ---- model derivatives (with derivative_skip), then cost derivatives
  start = std::chrono::steady_clock::now();
  model_derivative_.Compute(ctx_.get(), trajectory0, T, derivative_skip_, settings.fd_tolerance, settings.fd_mode != 0, n, m,
                            dim_sensor, dim_state);
  model_derivative_compute_time = GetDuration(start);
  start = std::chrono::steady_clock::now();
  cx_.resize((size_t)T * n); cu_.resize((size_t)T * m); cxx_.resize((size_t)T * n * n); cxu_.resize((size_t)T * n * m);
  cuu_.resize((size_t)T * m * m);
  ctx_->Check(mjpcx_cost_derivatives(ctx_->handle(), T, trajectory0.residual.data(), model_derivative_.C.data(),
                                     model_derivative_.D.data(), cx_.data(), cu_.data(), cxx_.data(), cxu_.data(), cuu_.data()));
  cost_derivative_compute_time = GetDuration(start);

  // ---- Gradient::Compute and parameter_update = M^T k in one launch
  start = std::chrono::steady_clock::now();
  GpuGradientPolicy& c0 = candidate_policy0;
  Vx_.resize((size_t)T * n);
  ctx_->Check(mjpcx_gradient_pass(ctx_->handle(), n, m, T, model_derivative_.A.data(), model_derivative_.B.data(), cx_.data(),
                                  cu_.data(), (int)c0.representation, c0.num_spline_points, c0.times.data(),
                                  trajectory0.times.data(), Vx_.data(), c0.k.data(), dV, c0.parameter_update.data(),
                                  &gradient_kernel_ms));
  gradient_compute_time = GetDuration(start);

  // ---- line search: theta + s_i * parameter_update, s = LogScale(1, min_linesearch_step, N - 1) and a zero step
  start = std::chrono::steady_clock::now();
  const int N = num_trajectory;
  linesearch_steps.assign(N, 0.0);
  if (N > 1) LogScale(linesearch_steps.data(), 1.0, settings.min_linesearch_step, N - 1);
  linesearch_steps[N - 1] = 0.0;
  Rollouts(horizon, pool);
  returns_.resize(N);
  failure_.resize(N);
  ctx_->Check(mjpcx_get_returns(ctx_->handle(), returns_.data(), failure_.data()));
  // strict < from the last candidate down, starting from the nominal's return; failed rollouts never win
  winner = N - 1;
  for (int j = N - 1; j >= 0; j--) {
    if (failure_[j]) continue;
    if (returns_[j] < c_best) {
      c_best = returns_[j];
      winner = j;
    }
  }
  const int P = c0.num_spline_points;
  if (c_best < c_prev) {
    for (int i = 0; i < P * nu; i++) c0.parameters[i] = nodes_[(size_t)winner * P * nu + i];
    ctx_->FetchTrajectory(winner, &trajectory0);
  }
  action_step = linesearch_steps[winner];
  expected = -action_step * dV[0] - 1.0e-16;
  improvement = c_prev - c_best;
  surprise = mju_min(mju_max(0, improvement / expected), 2);
  rollouts_compute_time = GetDuration(start);

  // ---- policy update (winner = N - 1, the zero step, leaves the resampled nominal)
  start = std::chrono::steady_clock::now();
  if (c_best >= c_prev) winner = N - 1;
  {
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    previous_policy.CopyFrom(policy, policy.num_spline_points);
    policy.CopyParametersFrom(c0.parameters, c0.times);
  }
  policy_update_compute_time = GetDuration(start);
}

// gradient/planner.cc:300-311: the resampled nominal policy, rolled out on the device
void GpuGradientPlanner::NominalTrajectory(int horizon, ThreadPool& pool) {
  const GpuGradientPolicy& c0 = candidate_policy0;
  ctx_->SyncTask(*task);  // the per-plan frozen ResidualFn copy (agent.cc:319)
  ctx_->Check(mjpcx_set_state(ctx_->handle(), state.data(), time, mocap.data(), userdata.data()));
  ctx_->Check(mjpcx_rollout_splines(ctx_->handle(), 1, horizon, c0.num_spline_points, (int)c0.representation, c0.times.data(),
                                    c0.parameters.data()));
  trajectory0.horizon = horizon;
  ctx_->FetchTrajectory(0, &trajectory0);
}

// gradient/planner.cc:355-381
void GpuGradientPlanner::ResamplePolicy(int horizon) {
  GpuGradientPolicy& c0 = candidate_policy0;
  const int P = c0.num_spline_points, nu = model->nu;
  double nominal_time = time;
  // the planning model's opt.timestep is agent_timestep (agent.cc); with one point there is no spacing (the reference divides by 0)
  const double timestep = GetNumberOrDefault(model->opt.timestep, model, "agent_timestep");
  const double time_shift = P > 1 ? mju_max((horizon - 1) * timestep / (P - 1), 1.0e-5) : 0.0;
  for (int t = 0; t < P; t++) {
    times_scratch_[t] = nominal_time;
    c0.Action(parameters_scratch_.data() + (size_t)t * nu, nullptr, nominal_time);
    nominal_time += time_shift;
  }
  std::copy_n(parameters_scratch_.begin(), (size_t)P * nu, c0.parameters.begin());
  for (int t = 0; t < P; t++) c0.times[t] = times_scratch_[0] + t * time_shift;  // LinearRange
}

// gradient/planner.cc:384-418: every candidate in one launch
void GpuGradientPlanner::Rollouts(int horizon, ThreadPool& pool) {
  const GpuGradientPolicy& c0 = candidate_policy0;
  const int N = num_trajectory, P = c0.num_spline_points, nu = model->nu;
  nodes_.resize((size_t)N * P * nu);
  for (int i = 0; i < N; i++)
    for (int k = 0; k < P * nu; k++) nodes_[(size_t)i * P * nu + k] = c0.parameters[k] + linesearch_steps[i] * c0.parameter_update[k];
  ctx_->Check(mjpcx_set_state(ctx_->handle(), state.data(), time, mocap.data(), userdata.data()));
  ctx_->Check(mjpcx_rollout_splines(ctx_->handle(), N, horizon, P, (int)c0.representation, c0.times.data(), nodes_.data()));
}

void GpuGradientPlanner::ActionFromPolicy(double* action, const double* s, double t, bool use_previous) {
  const std::shared_lock<std::shared_mutex> lock(mtx_);
  (use_previous ? previous_policy : policy).Action(action, s, t);
}

const Trajectory* GpuGradientPlanner::BestTrajectory() { return winner >= 0 ? &trajectory0 : nullptr; }

}  // namespace mjpc
