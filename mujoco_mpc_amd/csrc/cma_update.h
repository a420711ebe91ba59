// cma_update.h -- CMA-ES (covariance matrix adaptation) for E environments: the candidates of mjpcx_rollout_cma_batched and the update of
// mjpcx_cma_update_batched, in the Cholesky form with positive recombination weights. The search distribution N(m, sigma^2 D C D),
// D = diag(half control range), lives on the device: per environment sigma, the evolution paths p_sigma and p_c, C and its lower factor
// A (C = A A^T), all fp64 whatever the context's precision; the mean m is the nominal spline the host hands in with every rollout.
// Parameter j = node * nu + actuator, d = P * nu <= kCmaMaxParams.
//
// The one departure from Hansen's tutorial: the sigma path takes A^-1 where the tutorial has C^-1/2. A^-1 (m' - m) / sigma is exactly
// the weighted mean z_w of the ranked standard normals, so no eigendecomposition and no triangular solve are needed; A^-1 differs from
// C^-1/2 by a rotation, which leaves |p_sigma|'s distribution under random selection -- all the step-size rule relies on -- unchanged.
//
// Everything here has contraction off: every product and every sum rounds on its own, in the order include/mjpcx.h states, which
// planners.cma_update repeats in numpy. No atomics; a workgroup sees its own environment only, so environment e's bits do not depend
// on E or on its neighbours.
//
// The state of environment e, `stride` = 2 + 2 d + 2 d^2 doubles: [sigma | - | p_sigma d | p_c d | C d x d | A d x d], row-major, A with
// zeros above the diagonal. Kernels:
//   cma_candidates_kernel  workgroups of 256 over (16 candidates, environment): the candidates' normals go through LDS (a thread cannot
//                          hold 128 of them), thread (candidate r, row a) forms y[a] = sum_{b <= a} A[a][b] z[b] and stores the node.
//   cma_draw_kernel        the same for the mu ranked candidates of the update: y_(i) -> Y[e][a][i], unclamped (z is drawn again from
//                          the counter, never stored).
//   cma_sums_kernel        workgroups over (a, b, environment): b <= a the entry S[a][b] = sum_i (w_i y_(i)[a]) y_(i)[b] over the
//                          coalesced rows of Y; b == a + 1 (one spare workgroup per pair of rows) the pair z_w[2q], z_w[2q + 1],
//                          q = a / 2, with the normals drawn once more. Both in sg_tree256's shape.
//   cma_advance_kernel     one workgroup per environment: y_w, the mean, both paths, h_sigma, C', sigma', and the factorisation.
//   cma_factor_kernel      the factorisation alone (mjpcx_cma_set_state_batched).
// The factor is built column by column in LDS as a packed lower triangle, d (d + 1) / 2 doubles: 64.5 KiB at d = 128 of the CU's
// 160 KiB, which is what caps d -- a column costs two barriers and a row of LDS reads per thread, and the d(d+1)/2 sums of S one small
// workgroup each. C, A and Y stay in global memory (L2-resident: 128 KiB each per environment at d = 128).
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "wave_argmin.h"

namespace mjpcx {
constexpr int kCmaMaxParams = 128;
constexpr int kCmaGroup = 16;  // candidates per workgroup of cma_candidates_kernel / cma_draw_kernel

// the environment's record (pinned, device-mapped): header, then the d entries of the new mean
struct CmaRecord { double best_return, nominal_return, improvement, sigma; int index, valid, restarted, pad; double mean[1]; };
constexpr size_t kCmaHeader = 48;  // bytes of a CmaRecord before `mean`

__host__ __device__ inline size_t cma_state_stride(int d) { return 2 + 2 * (size_t)d + 2 * (size_t)d * d; }
__host__ __device__ inline size_t cma_tri_bytes(int d) { return (size_t)d * (d + 1) / 2 * sizeof(double); }

struct CmaCandArgs {
  int n, d, nu, num_envs;
  const double *nominal, *range, *state;  // E x d, 2 nu, E x stride
  uint64_t seed;
  uint32_t iteration;
};
struct CmaUpdateArgs {
  int n, d, nu, mu;
  const double *nominal, *range, *weights, *hs_den;  // E x d, 2 nu, mu, E (sqrt(1 - (1 - c_sigma)^(2 g)), the host's)
  double *state, *y, *zw, *s;                        // E x stride, E x d x mu, E x d, E x d x d
  const int* rank;                                   // E x (1 + mu): [valid | order]
  double one_m_cs, cs_root, one_m_cc, cc_root, decay[2], c_one, c_mu, cs_ds, chi, hs_rhs, sigma_min, sigma_max, pivot_floor;
  uint64_t seed;
  uint32_t iteration;
};

// zs[b * kCmaGroup + r] = z[b] of candidate cand(r) (cand(r) < 1: left alone, never read), for the whole workgroup of 256
template <class Cand>
__device__ __forceinline__ void cma_stage_normals(double* zs, int d, uint64_t seed, uint32_t iteration, Cand&& cand) {
  const int npairs = (d + 1) >> 1;
  for (int w = threadIdx.x; w < kCmaGroup * npairs; w += 256) {
    const int r = w & (kCmaGroup - 1), q = w >> 4, c = cand(r);
    if (c < 1) continue;
    double z[2];
    gaussian_pair(seed, (uint32_t)c, (uint32_t)q, iteration, z);
    zs[(2 * q) * kCmaGroup + r] = z[0];
    zs[(2 * q + 1) * kCmaGroup + r] = z[1];
  }
  __syncthreads();
}
// y[a] = sum_{b <= a} A[a][b] z[b], b ascending from 0.0
__device__ __forceinline__ double cma_row(const double* A, int d, int a, const double* zs, int r) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int b = 0; b <= a; b++) {
    const double p = A[(size_t)a * d + b] * zs[b * kCmaGroup + r];
    acc += p;
  }
  return acc;
}
__device__ __forceinline__ double cma_tree256(double v, int t, double* sm) {  // sg_tree256's shape; every thread of the workgroup calls it
#pragma clang fp contract(off)
  sm[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sm[t] += sm[t + s];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}

template <typename T>
__global__ __launch_bounds__(256) void cma_candidates_kernel(const CmaCandArgs a, T* __restrict__ nodes) {
#pragma clang fp contract(off)
  __shared__ double zs[kCmaMaxParams * kCmaGroup];
  const int env = blockIdx.y, c0 = blockIdx.x * kCmaGroup, d = a.d;  // n is a multiple of 64: every group is full
  const double* st = a.state + (size_t)env * cma_state_stride(d);
  const double sigma = st[0];
  const double* A = st + 2 + 2 * (size_t)d + (size_t)d * d;
  cma_stage_normals(zs, d, a.seed + (uint64_t)env, a.iteration, [&](int r) { return c0 + r; });
  const size_t N = (size_t)a.num_envs * a.n, at = (size_t)env * a.n + c0;
  for (int item = threadIdx.x; item < kCmaGroup * d; item += 256) {  // consecutive threads consecutive candidates of one node row
    const int r = item & (kCmaGroup - 1), j = item >> 4;
    double v = a.nominal[(size_t)env * d + j];
    if (c0 + r > 0) {
      const int k = j % a.nu;
      const double lo = a.range[2 * k], hi = a.range[2 * k + 1];
      const double half = 0.5 * (hi - lo), step = sigma * half;
      const double y = cma_row(A, d, j, zs, r), sy = step * y;
      v = clampv(v + sy, lo, hi);
    }
    nodes[(size_t)j * N + at + r] = (T)v;
  }
}

__global__ __launch_bounds__(256) void cma_draw_kernel(const CmaUpdateArgs a) {
#pragma clang fp contract(off)
  __shared__ double zs[kCmaMaxParams * kCmaGroup];
  const int env = blockIdx.y, i0 = blockIdx.x * kCmaGroup, d = a.d, mu = a.mu;
  const int* rank = a.rank + (size_t)env * (1 + mu);
  if (!rank[0]) return;  // not valid (the same for the whole workgroup)
  const double* A = a.state + (size_t)env * cma_state_stride(d) + 2 + 2 * (size_t)d + (size_t)d * d;
  cma_stage_normals(zs, d, a.seed + (uint64_t)env, a.iteration, [&](int r) { return i0 + r < mu ? rank[1 + i0 + r] : 0; });
  double* Y = a.y + (size_t)env * d * mu;
  for (int item = threadIdx.x; item < kCmaGroup * d; item += 256) {
    const int r = item & (kCmaGroup - 1), j = item >> 4;
    if (i0 + r < mu) Y[(size_t)j * mu + i0 + r] = cma_row(A, d, j, zs, r);
  }
}

__global__ __launch_bounds__(256) void cma_sums_kernel(const CmaUpdateArgs a) {
#pragma clang fp contract(off)
  __shared__ double sm[2][256];
  const int ra = blockIdx.x, rb = blockIdx.y, env = blockIdx.z, d = a.d, mu = a.mu, t = threadIdx.x;
  const int* rank = a.rank + (size_t)env * (1 + mu);
  if (!rank[0]) return;
  if (rb <= ra) {
    const double* ya = a.y + ((size_t)env * d + ra) * mu;
    const double* yb = a.y + ((size_t)env * d + rb) * mu;
    double acc = 0.0;
    for (int i = t; i < mu; i += 256) {
      const double wy = a.weights[i] * ya[i], term = wy * yb[i];
      acc += term;
    }
    const double s = cma_tree256(acc, t, sm[0]);
    if (t == 0) a.s[((size_t)env * d + ra) * d + rb] = s;
    return;
  }
  if (rb != ra + 1 || (ra & 1)) return;  // (a, a + 1), a even: the pair q = a / 2 of z_w; d odd: its last pair is (d - 1, d), grid y = d + 1
  const int q = ra >> 1;
  double acc0 = 0.0, acc1 = 0.0;
  for (int i = t; i < mu; i += 256) {
    double z[2];
    gaussian_pair(a.seed + (uint64_t)env, (uint32_t)rank[1 + i], (uint32_t)q, a.iteration, z);
    const double t0 = a.weights[i] * z[0], t1 = a.weights[i] * z[1];
    acc0 += t0;
    acc1 += t1;
  }
  const double s0 = cma_tree256(acc0, t, sm[0]), s1 = cma_tree256(acc1, t, sm[1]);
  if (t == 0) {
    a.zw[(size_t)env * d + 2 * q] = s0;
    if (2 * q + 1 < d) a.zw[(size_t)env * d + 2 * q + 1] = s1;
  }
}

// The factor of the d x d matrix C (row-major, its lower triangle is read) by columns into the packed lower triangle `tri`
// (tri[a (a + 1) / 2 + b]): per column b, acc = sum_{k < b} A[a][k] A[b][k] ascending from 0.0, s = C[a][b] - acc; the diagonal needs
// s > pivot_floor * C[b][b] (a NaN fails), A[b][b] = sqrt(s); below it A[a][b] = s / A[b][b]. Every thread of a workgroup of >= d
// threads calls it; false: a pivot failed (`tri` is then incomplete). sh: two doubles of LDS.
__device__ __forceinline__ bool cma_factor(const double* C, int d, double pivot_floor, double* tri, double* sh) {
#pragma clang fp contract(off)
  const int a = threadIdx.x;
  if (a == 0) sh[1] = 1.0;
  __syncthreads();
  for (int b = 0; b < d; b++) {
    double s = 0.0;
    if (a >= b && a < d) {
      const double *ra = tri + (size_t)a * (a + 1) / 2, *rb = tri + (size_t)b * (b + 1) / 2;
      double acc = 0.0;
      for (int k = 0; k < b; k++) {
        const double p = ra[k] * rb[k];
        acc += p;
      }
      s = C[(size_t)a * d + b] - acc;
      if (a == b) {
        const double floor = pivot_floor * C[(size_t)b * d + b];
        if (s > floor) sh[0] = sqrt(s);
        else sh[1] = 0.0;
      }
    }
    __syncthreads();
    if (sh[1] == 0.0) return false;  // (the same for the whole workgroup)
    if (a >= b && a < d) tri[(size_t)a * (a + 1) / 2 + b] = a == b ? sh[0] : s / sh[0];
    __syncthreads();
  }
  return true;
}
// the state after a factorisation: A from `tri`, or the restart C = A = I with both paths zero (sigma is the caller's)
__device__ __forceinline__ void cma_store_factor(double* st, int d, const double* tri, bool ok) {
  double *ps = st + 2, *pc = ps + d, *C = pc + d, *A = C + (size_t)d * d;
  for (int i = threadIdx.x; i < d * d; i += blockDim.x) {
    const int r = i / d, c = i - r * d;
    if (ok) A[i] = c <= r ? tri[(size_t)r * (r + 1) / 2 + c] : 0.0;
    else C[i] = A[i] = r == c ? 1.0 : 0.0;
  }
  if (!ok)
    for (int j = threadIdx.x; j < d; j += blockDim.x) ps[j] = pc[j] = 0.0;
}

// mjpcx_cma_set_state_batched: factor C as it was uploaded (pivot_floor 0: s > 0); failed[e] = 1 where a pivot fails (the state is
// then left without a factor: the host drops it)
__global__ __launch_bounds__(256) void cma_factor_kernel(double* state, int d, int* failed) {
  extern __shared__ __attribute__((aligned(16))) double cma_tri[];
  __shared__ double sh[2];
  const int env = blockIdx.x;
  double* st = state + (size_t)env * cma_state_stride(d);
  const bool ok = cma_factor(st + 2 + 2 * (size_t)d, d, 0.0, cma_tri, sh);
  if (ok) cma_store_factor(st, d, cma_tri, true);
  if (threadIdx.x == 0) failed[env] = ok ? 0 : 1;
}

__global__ __launch_bounds__(256) void cma_advance_kernel(const CmaUpdateArgs a, unsigned char* out, unsigned rec_bytes) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double cma_tri[];
  __shared__ double szw[kCmaMaxParams], syw[kCmaMaxParams], sps[kCmaMaxParams], spc[kCmaMaxParams], sh[2], snorm;
  __shared__ int shs;
  const int env = blockIdx.x, d = a.d, t = threadIdx.x;
  CmaRecord* rec = reinterpret_cast<CmaRecord*>(out + (size_t)env * rec_bytes);
  double* st = a.state + (size_t)env * cma_state_stride(d);
  double *ps = st + 2, *pc = ps + d, *C = pc + d, *A = C + (size_t)d * d;
  const double* nominal = a.nominal + (size_t)env * d;
  const double sigma = st[0];
  if (!a.rank[(size_t)env * (1 + a.mu)]) {  // one of the mu best is NaN: the state stays, the mean is the nominal
    for (int j = t; j < d; j += 256) rec->mean[j] = nominal[j];
    if (t == 0) { rec->valid = 0; rec->restarted = 0; rec->sigma = sigma; }
    return;
  }
  if (t < d) szw[t] = a.zw[(size_t)env * d + t];
  __syncthreads();
  if (t < d) {
    double acc = 0.0;  // y_w = A z_w by rows
    for (int b = 0; b <= t; b++) {
      const double p = A[(size_t)t * d + b] * szw[b];
      acc += p;
    }
    syw[t] = acc;
    const int k = t % a.nu;
    const double lo = a.range[2 * k], hi = a.range[2 * k + 1];
    const double half = 0.5 * (hi - lo), step = sigma * half, sy = step * acc;
    rec->mean[t] = clampv(nominal[t] + sy, lo, hi);
    const double keep = a.one_m_cs * ps[t], push = a.cs_root * szw[t];
    sps[t] = keep + push;
  }
  __syncthreads();
  if (t == 0) {
    double n2 = 0.0;
    for (int j = 0; j < d; j++) {
      const double p = sps[j] * sps[j];
      n2 += p;
    }
    const double norm = sqrt(n2);
    snorm = norm;
    shs = norm / a.hs_den[env] < a.hs_rhs ? 1 : 0;
  }
  __syncthreads();
  const int hs = shs;
  if (t < d) {
    const double hc = hs ? a.cc_root : 0.0;
    const double keep = a.one_m_cc * pc[t], push = hc * syw[t];
    spc[t] = keep + push;
  }
  __syncthreads();
  const double decay = hs ? a.decay[1] : a.decay[0];
  const double* S = a.s + (size_t)env * d * d;
  for (int i = t; i < d * d; i += 256) {
    const int r = i / d, c = i - r * d;
    if (c > r) continue;
    const double old = decay * C[i], pp = spc[r] * spc[c], rank1 = a.c_one * pp, rankmu = a.c_mu * S[i];
    const double v = (old + rank1) + rankmu;
    C[i] = v;
    C[(size_t)c * d + r] = v;
  }
  __syncthreads();  // (C' is read back by other threads of this workgroup)
  const bool ok = cma_factor(C, d, a.pivot_floor, cma_tri, sh);
  if (ok && t < d) { ps[t] = sps[t]; pc[t] = spc[t]; }
  cma_store_factor(st, d, cma_tri, ok);
  if (t == 0) {
    const double ratio = snorm / a.chi, x = a.cs_ds * (ratio - 1.0);
    const double grown = sigma * exp(x);
    const double next = grown < a.sigma_min ? a.sigma_min : (grown > a.sigma_max ? a.sigma_max : grown);
    st[0] = next;
    rec->sigma = next;
    rec->valid = 1;
    rec->restarted = ok ? 0 : 1;
  }
}
}  // namespace mjpcx
