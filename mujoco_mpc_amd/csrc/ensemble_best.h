// ensemble_best.h -- the selection of an ensemble (mjpcx_ensemble_best): the last batched rollout holds the returns R[h][i] of ONE set of
// n candidates under M hypotheses (mjpcx_rollout_noise_ensemble: hypothesis-major, R[h][i] = total_return[h * n + i]); a candidate's score
// is the mean of the `tail` largest of its M returns, and the winner is the argmin of the scores.
//   the M returns descending, equal values with the lower h first; the first `tail` summed in that order in fp64 with plain adds (the sum
//   starts AT the first, not at zero: a candidate of -0.0 returns scores -0.0), divided by tail; any NaN among the M: the score is NaN
//   tail = M: the mean over the hypotheses; tail = 1: the worst case; in between the tail mean (CVaR)
// The argmin is in less_ri's order (ascending, ties to the lower index, NaN last), reduced with wave_argmin as best_segmented_kernel does.
//
// One workgroup of kEnsembleThreads, one thread per candidate and pass: n is a multiple of 64, so a wavefront's reads of R[h][i .. i + 63] are
// one contiguous row segment for every h. A thread keeps its candidate's `tail` largest returns, descending, in its own column of dynamic
// LDS -- col[k * kEnsembleThreads + thread], so a wavefront's accesses to one k hit 64 consecutive doubles -- by insertion: at most tail
// (<= 32) moves per return, no private array, nothing spilled. 32 x 128 doubles are 32 KB.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_argmin.h"

namespace mjpcx {
constexpr int kEnsembleMaxHypotheses = 32;  // MJPCX_MAX_HYPOTHESES of include/mjpcx.h
constexpr int kEnsembleThreads = 128;
// the record the kernel writes (pinned, device-mapped): header, the winner's M returns, its spline values (np), the n scores (if asked for)
struct EnsembleRecord { double best_score, ref_score; int best_index, pad; double member[kEnsembleMaxHypotheses]; double rest[1]; };
constexpr size_t kEnsembleHeader = 16 + 8 + 8 * kEnsembleMaxHypotheses;  // bytes of an EnsembleRecord before `rest`

// the score of candidate i; col: the calling thread's LDS column, of `tail` entries kEnsembleThreads doubles apart
__device__ __forceinline__ double ensemble_score(const double* __restrict__ ret, int n, int M, int tail, int i, double* col) {
  bool nan = false;
  int held = 0;  // col[0 .. held) holds the largest returns so far, descending
  for (int h = 0; h < M; h++) {
    const double v = ret[(size_t)h * n + i];
    nan = nan || v != v;
    int p = held;
    // v goes in front of the strictly smaller ones: an equal return of a lower h stays ahead of it
    while (p > 0 && col[(p - 1) * kEnsembleThreads] < v) {
      if (p < tail) col[p * kEnsembleThreads] = col[(p - 1) * kEnsembleThreads];
      p--;
    }
    if (p < tail) col[p * kEnsembleThreads] = v;
    if (held < tail) held++;
  }
  double s = col[0];
  for (int k = 1; k < tail; k++) s += col[k * kEnsembleThreads];
  return nan ? __longlong_as_double(0x7ff8000000000000ll) : s / (double)tail;
}

// ret: M x n returns, hypothesis-major; nodes: [np][N] spline values with N = M * n (the winner's are read from hypothesis 0's copy);
// scores_on != 0: the n scores are written behind the spline values
template <typename T>
__global__ __launch_bounds__(kEnsembleThreads) void ensemble_best_kernel(const double* __restrict__ ret, const T* __restrict__ nodes, int n, int M, int tail,
                                                                         int np, int ref, int scores_on, unsigned char* out) {
  extern __shared__ __attribute__((aligned(16))) double ens_cols[];
  __shared__ RetIdx sm[kEnsembleThreads / 64];
  EnsembleRecord* rec = reinterpret_cast<EnsembleRecord*>(out);
  double* col = ens_cols + threadIdx.x;
  RetIdx best{NAN, 0x7fffffff};  // (sorts behind every candidate)
  if (threadIdx.x == 0 && ref < 0) rec->ref_score = NAN;
  for (int i = threadIdx.x; i < n; i += kEnsembleThreads) {
    const RetIdx c{ensemble_score(ret, n, M, tail, i, col), i};
    if (scores_on) rec->rest[np + i] = c.r;
    if (i == ref) rec->ref_score = c.r;
    if (less_ri(c, best)) best = c;
  }
  best = wave_argmin(best);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sm[wave] = best;
  __syncthreads();
  best = wave_argmin(lane < kEnsembleThreads / 64 ? sm[lane] : RetIdx{NAN, 0x7fffffff});  // (every wavefront: the winner without a second barrier)
  const int w = best.i;
  if (threadIdx.x == 0) { rec->best_score = best.r; rec->best_index = w; rec->pad = 0; }
  if (w >= 0 && w < n) {
    if ((int)threadIdx.x < M) rec->member[threadIdx.x] = ret[(size_t)threadIdx.x * n + w];
    const size_t N = (size_t)M * n;
    for (int j = threadIdx.x; j < np; j += kEnsembleThreads) rec->rest[j] = (double)nodes[(size_t)j * N + w];
  }
}
}  // namespace mjpcx
