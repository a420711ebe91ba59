// mppi_update.h -- the MPPI (model predictive path integral) update of E environments (mjpcx_mppi_update_batched): where the other
// selection kernels choose (the argmin of best_segmented_kernel, the n_elite best of ce_update_kernel), this one averages -- every
// candidate's spline enters the new policy with the weight exp(-(R - R_min) / lambda). Per environment e over its n returns R[i], its
// spline parameters p[i][j] = nodes[j * N + first + i] and lambda = temperature[e]:
//   winner   the argmin in less_ri's order (ascending, ties to the lower index, NaN last): the reads and the reduction of
//            best_segmented_kernel, so index and beta = best_return are mjpcx_best_batched's. valid = beta is a number below +inf.
//   weights  w[i] = 0 if R[i] is NaN; 1 if R[i] == beta (ties at the minimum, +-0, beta = -inf); else exp(-((R[i] - beta) / lambda)):
//            one fp64 subtraction, one fp64 division, the negation, the device library's double-precision exp. Not valid: every w[i] = 0.
//   sums     eta = sum w, Q = sum w^2, S[j] = sum w[i] p[i][j] (the node cast to double first), each in elite_reduce's shape (mjpcx.hip):
//            256 strided partial sums in index order from zero, then the halving tree. Contraction is off in both kernels, so no product
//            joins an addition in an fma: tests/mppi_cases.py repeats these sums operation for operation. No atomics.
//   outputs  weight_sum = eta, effective_samples = eta * eta / Q, mean[j] = S[j] / eta; not valid: 0, 0 and ref_candidate's spline (NaN
//            without one). ref_return = R[ref_candidate] (NaN without one).
//
// Two kernels on the context's stream. The arithmetic is small; the n x np node values are the traffic (one robot x 16384 candidates x 72
// parameters in fp64: 9 MB), and one workgroup per environment would pull them through a single CU -- eight of 256 busy for a fleet of
// eight. So:
//   mppi_weights_kernel  one workgroup of 256 per environment: the segmented argmin, then w[] into the environment's device slab
//                        [eta | w[0..n)] with eta and Q reduced on the way, and the record's header.
//   mppi_mean_kernel     a grid of (np, E) workgroups of 256: workgroup (j, e) reads the coalesced row nodes + j * N + first and the
//                        slab's weights (n doubles, L2-resident after the first j) and reduces S[j] once.
// A workgroup sees its own environment only, so environment e's bits do not depend on E or on the other environments.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_argmin.h"

namespace mjpcx {
// the environment's record (pinned, device-mapped): header, then the np means; the optional weights of all environments follow the E records
struct MppiRecord { double best_return, ref_return, weight_sum, effective_samples; int best_index, valid; double mean[1]; };
constexpr size_t kMppiHeader = 40;  // bytes of an MppiRecord before `mean`

// elite_reduce's tree over the 256 partial sums `acc` of a workgroup of 256 (every thread calls it; sm: 256 doubles)
__device__ __forceinline__ double mppi_tree_sum(double acc, int t, double* sm) {
  __syncthreads();  // (sm may still be read from the previous sum)
  sm[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sm[t] += sm[t + s];
    __syncthreads();
  }
  return sm[0];
}

// slab: E x (n_env + 1) doubles, environment e's [eta | w]; weights_out (may be null): E x n_env, in mapped host memory
__global__ __launch_bounds__(256) void mppi_weights_kernel(const double* __restrict__ ret, const double* __restrict__ temperature, int n_env, int ref,
                                                           double* __restrict__ slab, unsigned char* out, unsigned rec_bytes, double* weights_out) {
#pragma clang fp contract(off)
  __shared__ RetIdx smi[4];
  __shared__ double sm[256];
  const int env = blockIdx.x, first = env * n_env, t = threadIdx.x;
  RetIdx best{NAN, 0x7fffffff};  // (sorts behind every candidate)
  for (int i = t; i < n_env; i += 256) {
    const RetIdx c{ret[first + i], i};
    if (less_ri(c, best)) best = c;
  }
  best = wave_argmin(best);
  const int wave = t >> 6, lane = t & 63;
  if (lane == 0) smi[wave] = best;
  __syncthreads();
  best = wave_argmin(lane < 4 ? smi[lane] : RetIdx{NAN, 0x7fffffff});  // (every wavefront: the winner without a second barrier)
  const double beta = best.r, lambda = temperature[env];
  const bool valid = beta == beta && beta < INFINITY;
  double* w_env = slab + (size_t)env * (n_env + 1) + 1;
  double eta = 0, q = 0;
  for (int i = t; i < n_env; i += 256) {
    const double r = ret[first + i];
    double w = 0;
    if (valid && r == r) {
      if (r == beta) w = 1.0;
      else { const double x = (r - beta) / lambda; w = exp(-x); }
    }
    w_env[i] = w;
    if (weights_out) weights_out[(size_t)first + i] = w;
    const double w2 = w * w;
    eta += w;
    q += w2;
  }
  eta = mppi_tree_sum(eta, t, sm);
  q = mppi_tree_sum(q, t, sm);
  if (t == 0) {
    MppiRecord* rec = reinterpret_cast<MppiRecord*>(out + (size_t)env * rec_bytes);
    const double eta2 = eta * eta;
    w_env[-1] = valid ? eta : 0.0;  // (0: mppi_mean_kernel hands out the reference spline instead)
    rec->best_return = beta;
    rec->best_index = best.i;  // local to the environment
    rec->ref_return = (ref >= 0 && ref < n_env) ? ret[first + ref] : NAN;
    rec->valid = valid ? 1 : 0;
    rec->weight_sum = valid ? eta : 0.0;
    rec->effective_samples = valid ? eta2 / q : 0.0;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mppi_mean_kernel(const T* __restrict__ nodes, const double* __restrict__ slab, int N, int n_env, int ref,
                                                        unsigned char* out, unsigned rec_bytes) {
#pragma clang fp contract(off)
  __shared__ double sm[256];
  const int j = blockIdx.x, env = blockIdx.y, first = env * n_env, t = threadIdx.x;
  const double* w_env = slab + (size_t)env * (n_env + 1) + 1;
  const T* nodes_j = nodes + (size_t)j * N + first;
  MppiRecord* rec = reinterpret_cast<MppiRecord*>(out + (size_t)env * rec_bytes);
  const double eta = w_env[-1];
  if (!(eta > 0)) {  // not valid (the same for the whole workgroup)
    if (t == 0) rec->mean[j] = (ref >= 0 && ref < n_env) ? (double)nodes_j[ref] : (double)NAN;
    return;
  }
  double acc = 0;
  for (int i = t; i < n_env; i += 256) {
    const double wp = w_env[i] * (double)nodes_j[i];
    acc += wp;
  }
  const double s = mppi_tree_sum(acc, t, sm);
  if (t == 0) rec->mean[j] = s / eta;
}
}  // namespace mjpcx
