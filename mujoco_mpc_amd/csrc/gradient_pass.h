// gradient_pass.h -- the first-order half of the Gradient planner on gfx950 (mjpc/planners/gradient):
//   * the adjoint sweep of Gradient::Compute (gradient.cc:43-108): Vx[T-1] = cx[T-1]; for t = T-1..1
//       Qx = cx[t-1] + A[t-1]^T Vx[t], Qu = cu[t-1] + B[t-1]^T Vx[t], k[t-1] = -Qu, Vx[t-1] = Qx, dV[0] += k[t-1] . Qu;
//     then k[T-1] = k[T-2]
//   * the projection parameter_update = M^T k onto the spline parameters (gradient/planner.cc:247-257), where M is the
//     Zero / Linear / CubicSplineMapping of spline_mapping.cc. M is block-diagonal in the control index, so
//     gradient[p][j] = sum_t w(t, p) k[t][j]; the weights come from FindInterval / CubicCoefficients at the step times and the
//     finite-difference point_slope_mapping, evaluated here -- the nu(T-1) x nu P matrix is never formed.
// ONE wavefront: lane i < n owns Qx_i, lane n + i owns Qu_i, so a step is one (n + m) x n transposed mat-vec whose loads
// A[t][j][lane] / B[t][j][lane - n] are coalesced along the lane index; Vx[t] is broadcast from LDS. The sweep is a chain of T
// dependent steps (latency-bound): the next step's column is loaded into registers while the current dot product runs, which
// hides little of a global load's latency -- measured 3-4 us per step on MI355X even at n = 4.
// Results leave through per-lane (vector) global stores.
#pragma once
#include "device_common.h"

namespace mjpcx {

constexpr int kGradMaxN = 48, kGradMaxM = 16, kGradMaxP = 25, kGradMaxT = 512;  // P: kMaxGradientSplinePoints, T: kMaxTrajectoryHorizon

struct GradientArgs {
  int n, m, T, P, representation;
  const double *A, *B, *cx, *cu;             // T x n x n, T x n x m, T x n, T x m
  const double *node_times, *step_times;     // P, T
  double *Vx, *k, *dV, *gradient;            // T x n, T x m, 2, P x m
};

// LDS carve (doubles first): Vx[48] | k[T][m] | coef[T-1][4] | ps[P][3] | bounds[T-1][2] (int)
inline size_t gradient_pass_lds_bytes(int T, int m, int P) {
  return (size_t)(kGradMaxN + (size_t)T * m + 4 * (size_t)T + 3 * (size_t)P) * 8 + 2 * (size_t)T * 4;
}

namespace grad_detail {
// FindInterval (utilities.h:124-144): bounds of the grid interval holding x (both ends the same index outside the grid)
__device__ __forceinline__ void find_interval(int& b0, int& b1, const double* xs, double x, int length) {
  int upper = 0;
  while (upper < length && !(x < xs[upper])) upper++;
  const int lower = upper - 1;
  if (lower < 0) { b0 = 0; b1 = 0; }
  else { b0 = lower; b1 = upper < length - 1 ? upper : length - 1; }
}
template <int CTRL> __device__ __forceinline__ double dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane(double v, int src) {  // src must be wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// sum over the 64 lanes: row_shr 1, 2, 4, 8 leaves each row's total in its lane 15, then the four rows meet through v_readlane
__device__ __forceinline__ double wave_sum64(double v) {
  v += dpp<0x111>(v); v += dpp<0x112>(v); v += dpp<0x114>(v); v += dpp<0x118>(v);
  return readlane(v, 15) + readlane(v, 31) + readlane(v, 47) + readlane(v, 63);
}
__device__ __forceinline__ void lds_sync() {  // LDS ordering inside one wavefront (ilqg_dense.h: wave_sync)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
}  // namespace grad_detail

__device__ __forceinline__ void gradient_pass_body(const GradientArgs& a, double* lds) {
  const int lane = threadIdx.x, n = a.n, m = a.m, T = a.T, P = a.P;
  double* vx = lds;                                    // Vx[t], broadcast to every lane
  double* ks = vx + kGradMaxN;                         // k, T x m
  double* coef = ks + (size_t)T * m;                   // per output step: weights of the points b0, b1 and slopes b0, b1
  double* ps = coef + 4 * (size_t)T;                   // per node i: slope = ps0 p[i-1] + ps1 p[i] + ps2 p[i+1]
  int* bnd = (int*)(ps + 3 * P);                       // per output step: b0, b1

  // ---- sweep (Gradient::Compute)
  const bool is_x = lane < n, is_u = lane >= n && lane < n + m;
  const int col = is_x ? lane : lane - n;              // column of A (lane < n) or of B (n <= lane < n + m)
  const int ld = is_x ? n : m;
  if (is_x) {
    const double v = a.cx[(size_t)(T - 1) * n + lane];
    vx[lane] = v;
    a.Vx[(size_t)(T - 1) * n + lane] = v;
  }
  grad_detail::lds_sync();
  // column of step t - 1 in registers; the next one is loaded while this one is used
  auto load_col = [&](double (&c)[kGradMaxN], int t) {
    const double* base = (is_x ? a.A + (size_t)t * n * n : a.B + (size_t)t * n * m) + col;
#pragma unroll
    for (int j = 0; j < kGradMaxN; j++) c[j] = (j < n && (is_x || is_u)) ? base[(size_t)j * ld] : 0.0;
  };
  double cur[kGradMaxN], nxt[kGradMaxN];
  load_col(cur, T - 2);
  double dv = 0.0;
  for (int t = T - 1; t > 0; t--) {
    if (t > 1) load_col(nxt, t - 2);
    const double c0 = is_x ? a.cx[(size_t)(t - 1) * n + col] : (is_u ? a.cu[(size_t)(t - 1) * m + col] : 0.0);
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < kGradMaxN; j++)
      if (j < n) q = fma(cur[j], vx[j], q);
    q += c0;
    grad_detail::lds_sync();                                       // every lane has read Vx[t] before it is overwritten
    if (is_x) {
      vx[lane] = q;
      a.Vx[(size_t)(t - 1) * n + lane] = q;
    } else if (is_u) {
      ks[(size_t)(t - 1) * m + col] = -q;
      a.k[(size_t)(t - 1) * m + col] = -q;
      dv += -q * q;
    }
    grad_detail::lds_sync();
    if (t > 1) {
#pragma unroll
      for (int j = 0; j < kGradMaxN; j++) cur[j] = nxt[j];
    }
  }
  if (is_u) {
    const double kl = ks[(size_t)(T - 2) * m + col];
    ks[(size_t)(T - 1) * m + col] = kl;
    a.k[(size_t)(T - 1) * m + col] = kl;
  }
  dv = grad_detail::wave_sum64(dv);
  if (lane == 0) { a.dV[0] = dv; a.dV[1] = 0.0; }

  // ---- spline mapping weights (spline_mapping.cc): rows are the T - 1 step times
  const double* xs = a.node_times;
  for (int t = lane; t < T - 1; t += 64) {
    int b0, b1;
    const double x = a.step_times[t];
    grad_detail::find_interval(b0, b1, xs, x, P);
    double w0 = 1.0, w1 = 0.0, s0 = 0.0, s1 = 0.0;
    if (b0 != b1) {
      const double span = xs[b1] - xs[b0], s = (x - xs[b0]) / span;
      if (a.representation == 1) { w0 = 1.0 - s; w1 = s; }
      else if (a.representation == 2) {          // CubicCoefficients (utilities.cc:337-359)
        w0 = 2.0 * s * s * s - 3.0 * s * s + 1.0;
        s0 = (s * s * s - 2.0 * s * s + s) * span;
        w1 = -2.0 * s * s * s + 3 * s * s;
        s1 = (s * s * s - s * s) * span;
      }
    }
    if (a.representation == 0) b1 = b0;          // ZeroSplineMapping: the left node only
    coef[4 * t + 0] = w0; coef[4 * t + 1] = w1; coef[4 * t + 2] = s0; coef[4 * t + 3] = s1;
    bnd[2 * t] = b0; bnd[2 * t + 1] = b1;
  }
  // point_slope_mapping: one-sided differences at the ends of the grid, the mean of the two secants inside
  for (int i = lane; i < P; i += 64) {
    double dt1 = i > 0 ? 1.0 / (xs[i] - xs[i - 1]) : 0.0;
    double dt2 = i < P - 1 ? 1.0 / (xs[i + 1] - xs[i]) : 0.0;
    if (i > 0 && i < P - 1) { dt1 *= 0.5; dt2 *= 0.5; }
    ps[3 * i] = -dt1; ps[3 * i + 1] = dt1 - dt2; ps[3 * i + 2] = dt2;
  }
  grad_detail::lds_sync();

  // ---- projection: gradient[p][j] = sum_t w(t, p) k[t][j]
  for (int o = lane; o < P * m; o += 64) {
    const int p = o / m, j = o - p * m;
    double g = 0.0;
    for (int t = 0; t < T - 1; t++) {
      const int b0 = bnd[2 * t], b1 = bnd[2 * t + 1];
      if (p < b0 - 1 || p > b1 + 1) continue;    // outside the support of row t
      const double* c = coef + 4 * t;
      double w = (p == b0 ? c[0] : 0.0) + (p == b1 && b1 != b0 ? c[1] : 0.0);
      if (a.representation == 2) {               // the slope columns of the cubic output mapping times point_slope_mapping
        auto slope_weight = [&](int i) { const int d = p - i; return (d >= -1 && d <= 1) ? ps[3 * i + d + 1] : 0.0; };
        w += c[2] * slope_weight(b0);
        if (b1 != b0) w += c[3] * slope_weight(b1);
      }
      g = fma(w, ks[(size_t)t * m + j], g);
    }
    a.gradient[o] = g;
  }
}

__global__ __launch_bounds__(64) void gradient_pass_kernel(const GradientArgs a) {
  extern __shared__ double lds[];
  gradient_pass_body(a, lds);
}

// E trajectories in one launch (mjpcx_gradient_step_batched): workgroup e, one wavefront, runs the pass above on environment e's block of
// every array -- A, B, cx, cu, step_times, Vx and k are E x T x ..., node_times E x P, dV E x 2, gradient E x P x m. The environments
// are independent, so the grid hides the latency of the T dependent steps that one trajectory alone exposes.
__global__ __launch_bounds__(64) void gradient_pass_batched_kernel(const GradientArgs a0) {
  extern __shared__ double lds[];
  const size_t e = blockIdx.x, n = a0.n, m = a0.m, T = a0.T, P = a0.P;
  GradientArgs a = a0;
  a.A += e * T * n * n; a.B += e * T * n * m; a.cx += e * T * n; a.cu += e * T * m;
  a.node_times += e * P; a.step_times += e * T;
  a.Vx += e * T * n; a.k += e * T * m; a.dV += e * 2; a.gradient += e * P * m;
  gradient_pass_body(a, lds);
}

}  // namespace mjpcx
