// gradient_batched.h -- the interpolation kernel of the batched derivative chain (mjpcx_gradient_step_batched, mjpcx_ilqg_step_batched).
// The Gradient planner's chain for E environments, every stage on the device:
//   gather_candidates_kernel (ilqg_batched.h)   local candidate `cand` of every environment of the last batched rollout, out of the
//                           Trajectory buffers, into the environment-major arrays the stages below read, with the step times
//   transition_fd_kernel<ENVS> / transition_fd_wave_kernel (ilqg_kernels.h, wave_ilqg.h), fd_assemble_kernel over E x num_eval steps
//   fd_interpolate_kernel   ModelDerivatives::Compute's skip interpolation (model_derivatives.cc:108-165) to all T steps, and the
//                           zeroed last step of A, B, D (gradient/planner.cc:211-216)
//   cost_gradient_kernel (ilqg_dense.h) on E x T workgroups, gradient_pass_batched_kernel (gradient_pass.h) on E
#pragma once
#include "device_common.h"

namespace mjpcx {

// X[e][t] = X_eval[e][i0] (1 - w) + X_eval[e][i1] w for X = A, B, C, D, with i0 the last evaluated step <= t, i1 the next one (the last:
// itself) and w = (t - evaluate[i0]) / (evaluate[i1] - evaluate[i0]); an evaluated step is copied. Two products and a sum, not
// contracted: the operations of planners.model_derivatives. A, B and D of step T - 1, which has no transition, are zero.
__global__ __launch_bounds__(256) void fd_interpolate_kernel(const double* __restrict__ Ae, const double* __restrict__ Be,
                                                             const double* __restrict__ Ce, const double* __restrict__ De,
                                                             const int* __restrict__ evaluate, int E, int ne, int T, int sA, int sB, int sC,
                                                             int sD, double* A, double* B, double* C, double* D) {
#pragma clang fp contract(off)
  const int per_t = sA + sB + sC + sD;
  const size_t total = (size_t)E * T * per_t;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t et = idx / per_t;
    int r = (int)(idx - et * per_t);
    const int e = (int)(et / T), t = (int)(et - (size_t)e * T);
    const double* src; double* dst; int sz; bool zero_last = true;
    if (r < sA) { src = Ae; dst = A; sz = sA; }
    else if ((r -= sA) < sB) { src = Be; dst = B; sz = sB; }
    else if ((r -= sB) < sC) { src = Ce; dst = C; sz = sC; zero_last = false; }
    else { r -= sC; src = De; dst = D; sz = sD; }
    double v = 0.0;
    if (!(zero_last && t == T - 1)) {
      int lo = 0, hi = ne - 1;  // the last evaluated step <= t (evaluate[0] = 0)
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (evaluate[mid] <= t) lo = mid; else hi = mid - 1; }
      const int i0 = lo, i1 = lo + 1 < ne ? lo + 1 : ne - 1;
      const double x0 = src[((size_t)e * ne + i0) * sz + r];
      if (evaluate[i0] >= t || i0 == i1) v = x0;  // (also a step before the first or after the last evaluated one)
      else {
        const double w = (double)(t - evaluate[i0]) / (double)(evaluate[i1] - evaluate[i0]);
        const double x1 = src[((size_t)e * ne + i1) * sz + r];
        v = x0 * (1.0 - w) + x1 * w;
      }
    }
    dst[et * sz + r] = v;
  }
}

}  // namespace mjpcx
