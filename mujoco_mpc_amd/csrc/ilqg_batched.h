// ilqg_batched.h -- the gather kernel of the batched derivative chains (mjpcx_ilqg_step_batched, mjpcx_gradient_step_batched). iLQG's
// chain and backward pass for E environments, every stage on the device ("iLQG's derivative chain and backward pass for
// the fleet"):
//   gather_candidates_kernel   local candidate cands[e] of environment e of the last batched rollout -- iLQG's nominal is the best of
//                              each environment's own nominal rollouts, the Gradient planner's the same candidate of every environment
//                              -- out of the Trajectory buffers in whichever layout the rollout kernel left them, into the
//                              environment-major arrays the stages below read. Per step, whichever the caller asks for: the actions of
//                              ALL T steps (iLQG: the box-QP of the backward pass needs them), the step times (Gradient: the spline
//                              projection needs them). With `from_alt` (mjpcx_ilqg_step_batched_from) an environment reads a SECOND
//                              rollout instead -- another context's, with its own batch size, horizon, candidates per environment and
//                              layout: the selector is per environment, the launch is one
//   transition_fd_kernel<ENVS> / transition_fd_wave_kernel, fd_assemble_kernel, fd_interpolate_kernel as in gradient_batched.h
//   cost_derivatives_kernel (ilqg_dense.h) on E x T workgroups: workgroup e * T + t forms step t of environment e
//   backward_pass_batched_kernel (ilqg_dense.h) on E workgroups
#pragma once
#include "device_common.h"

namespace mjpcx {

template <typename T>
struct GatherRollout {
  const T *states, *actions, *times, *residual;  // a rollout's Trajectory buffers
  const double* total_return;                    // [N]
  int N, H, n_per_env, candidate_major;
};

template <typename T>
struct GatherCandidatesArgs {
  const T *states, *actions, *times, *residual;  // the rollout's Trajectory buffers
  const double* total_return;                    // [N]
  int N, H, n_per_env, candidate_major;          // environment e reads global candidate source[e] * n_per_env + cands[e]
  GatherRollout<T> alt;                          // the second rollout, read by the environments with from_alt[e] != 0
  const int* from_alt;                           // [E], the value of the environment it rides on for one that takes no part; nullptr: nobody
  const int* source;                             // [E] e itself; for an environment that takes no part, the first active one
  const int* cands;                              // [E] local candidates of the source, every one within [0, n_per_env) of the rollout it reads
  const int* active;                             // [E]: 0 = the environment takes no part (its nominal_return is 0)
  int E, Tn, ne;                                 // environments, steps, evaluated steps
  const int* evaluate;                           // [ne]
  int ds_roll, ds, nu, nr;                       // state row of the rollout (nq + nv + na), its leading nq + nv, controls, residuals
  T *fd_times, *fd_states, *fd_actions;          // [E][ne], [E][ne][ds], [E][ne][nu]: the finite-difference kernels' inputs
  double *residual_out, *nominal_return;         // [E][Tn][nr], [E]
  double *step_times, *actions_out;              // [E][Tn], [E][Tn][nu]; nullptr: the row is not written
};

template <typename T>
__global__ __launch_bounds__(256) void gather_candidates_kernel(const GatherCandidatesArgs<T> g) {
  const int nst = g.step_times ? 1 : 0, per_fd = 1 + g.ds + g.nu, per_t = g.nr + nst + (g.actions_out ? g.nu : 0);
  const size_t per_env = (size_t)g.ne * per_fd + (size_t)g.Tn * per_t + 1, total = per_env * g.E;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int e = (int)(idx / per_env);
    size_t r = idx - (size_t)e * per_env;
    const bool alt = g.from_alt && g.from_alt[e];
    const int N = alt ? g.alt.N : g.N, H = alt ? g.alt.H : g.H, major = alt ? g.alt.candidate_major : g.candidate_major;
    const size_t c = (size_t)g.source[e] * (alt ? g.alt.n_per_env : g.n_per_env) + g.cands[e];
    const T *states = alt ? g.alt.states : g.states, *actions = alt ? g.alt.actions : g.actions, *times = alt ? g.alt.times : g.times;
    const T* residual = alt ? g.alt.residual : g.residual;
    // [(cand * H + t) * width + k] (wavefront-per-candidate kernels) or [(t * width + k) * N + cand] (lane kernels): gather_traj_kernel
    auto load = [&](const T* src, int width, int t, int k) {
      return major ? src[(c * H + t) * width + k] : src[((size_t)t * width + k) * N + c];
    };
    if (r < (size_t)g.ne * per_fd) {
      const int i = (int)(r / per_fd), j = (int)(r % per_fd), t = g.evaluate[i];
      const size_t row = (size_t)e * g.ne + i;
      if (j == 0) g.fd_times[row] = load(times, 1, t, 0);
      else if (j <= g.ds) g.fd_states[row * g.ds + (j - 1)] = load(states, g.ds_roll, t, j - 1);
      else g.fd_actions[row * g.nu + (j - 1 - g.ds)] = load(actions, g.nu, t, j - 1 - g.ds);
    } else if ((r -= (size_t)g.ne * per_fd) < (size_t)g.Tn * per_t) {
      const int t = (int)(r / per_t), j = (int)(r % per_t);
      const size_t row = (size_t)e * g.Tn + t;
      if (j < g.nr) g.residual_out[row * g.nr + j] = (double)load(residual, g.nr, t, j);
      else if (j < g.nr + nst) g.step_times[row] = (double)load(times, 1, t, 0);
      else g.actions_out[row * g.nu + (j - g.nr - nst)] = (double)load(actions, g.nu, t, j - g.nr - nst);
    } else {
      g.nominal_return[e] = g.active[e] ? (alt ? g.alt.total_return : g.total_return)[c] : 0.0;
    }
  }
}

}  // namespace mjpcx
