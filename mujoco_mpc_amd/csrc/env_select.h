// env_select.h -- several environments in one launch (mjpcx_rollout_*_batched): what every rollout kernel's wrapper uses to find the plan
// record of its candidates' environment. The request structs (RolloutArgs, quad::QArgs, limb::LArgs) carry env_n, the candidates per
// environment (0: one environment), and env_stride, the bytes between the records [node_times | nominal | variance | blob] of consecutive
// environments; node_times, nominal, the CE variance and the blob pointer are environment 0's. env_n is a multiple of 64: the environment is uniform over
// a wavefront, and over a workgroup of the lane, quad and limb kernels, so it lives in SGPRs and selects with scalar arithmetic.
// The feedback kernels of mjpcx_rollout_feedback_batched take ANY env_n >= 1: on rollout_feedback_quad_kernel and the wave / tree feedback
// kernels a 64-thread workgroup is one candidate (cpw = 1), so its environment is blockIdx.x / env_n; rollout_feedback_kernel<ENVS> of the
// lane family pads every environment to whole wavefronts instead (FeedbackArgs::env_waves).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mjpcx {
// the environment of a wavefront whose first candidate is `cand`, in an SGPR
template <class A> __device__ __forceinline__ int env_of(const A& a, int cand) {
  return a.env_n > 0 ? __builtin_amdgcn_readfirstlane(cand) / a.env_n : 0;
}
// a pointer into environment 0's record, moved to the same place in environment `env`'s
template <typename P> __device__ __forceinline__ const P* env_ptr(const P* p, int env, unsigned stride) {
  return reinterpret_cast<const P*>(reinterpret_cast<const char*>(p) + (size_t)env * stride);
}
// the node times and the nominal spline of environment `env`; the wrapper also gives it the noise stream of a single-environment call
// with seed + env, counted from the environment's first candidate (include/mjpcx.h), and moves the cross-entropy variance pointer
// with env_ptr: mjpcx_rollout_noise_batched stages one shared row into every record, mjpcx_rollout_noise_batched_ce a row per
// environment. Candidate indices stay global.
template <class A> __device__ __forceinline__ void env_rebase(A& a, int env) {
  a.node_times = env_ptr(a.node_times, env, a.env_stride);
  a.nominal = env_ptr(a.nominal, env, a.env_stride);
}
}  // namespace mjpcx
