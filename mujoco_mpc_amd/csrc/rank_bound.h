// rank_bound.h -- the bound of a quad launch in rank mode (mjpcx_set_prune_rank, QArgs::keep_bound): T, the K-th smallest return among the
// candidates that have COMPLETED, written into the environment's bound word. It runs on the stream between rollout_quad_kernel, whose
// completions left the word at +inf, and the settling pass (park_settle.h), which judges the parked candidates against the word.
//   C = the candidates with failure == 0 and a finite return >= 0 (handed-on, parked and retired ones carry a marker: they have not
//       completed, and a negative or NaN return is not one the bound word can hold)
//   T = the K-th smallest return of C; +inf if C has fewer than K members
// K candidates hold returns <= T, so a candidate whose partial return -- a lower bound of its return -- is strictly above T is not among the
// first K of the launch in less_ri order, and T can only be above the launch's final K-th return, never below it.
//
// One workgroup per environment, any env_n >= 1 (a plain launch is one environment of N candidates). Non-negative doubles order as their
// bit patterns, so T is a radix select on the 64-bit keys: eight passes of eight bits from the top, each a 256-bin histogram in LDS of the
// keys that share the digits chosen so far, then a scan of the bins by the first wavefront for the bin that holds the k-th of them. The
// keys are re-read from global memory in every pass (a return and a failure word per candidate, out of L2 after the first), so no size of
// environment is special. The histogram's counts are integers: the result does not depend on the order of the atomics. -0.0 counts as 0.
#pragma once
#include <hip/hip_runtime.h>

#include "env_select.h"

namespace mjpcx {
constexpr int kRankBoundThreads = 1024;
constexpr unsigned long long kRankBoundInf = 0x7ff0000000000000ull;

// whether a candidate is in C, and its key
__device__ __forceinline__ bool rank_bound_key(double r, int f, unsigned long long& key) {
  if (f != 0 || !(r >= 0) || !(r <= 1.79769313486231570815e308)) return false;
  key = r == 0 ? 0ull : (unsigned long long)__double_as_longlong(r);
  return true;
}

// total_return, failure: environment 0's first candidate; bound: environment 0's word, rec_stride bytes between consecutive environments'
__global__ __launch_bounds__(kRankBoundThreads) void rank_bound_kernel(const double* __restrict__ total_return, const int* __restrict__ failure, int env_n, int K,
                                                                       unsigned long long* __restrict__ bound, unsigned rec_stride) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_k;
  const int env = blockIdx.x, tid = threadIdx.x, lane = threadIdx.x & 63;
  total_return += (size_t)env * env_n;
  failure += (size_t)env * env_n;
  unsigned long long prefix = 0;  // the digits of T chosen so far
  unsigned k = K > 0 ? (unsigned)K : 1u;  // T is the k-th smallest of the keys that start with them (0: C has fewer than K members)
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < env_n; i += kRankBoundThreads) {
      unsigned long long key;
      if (!rank_bound_key(total_return[i], failure[i], key)) continue;
      if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // (the first wavefront: lane l owns bins 4 l .. 4 l + 3)
      unsigned h[4], own = 0;
      for (int j = 0; j < 4; j++) { h[j] = hist[4 * lane + j]; own += h[j]; }
      unsigned incl = own;
      for (int o = 1; o < 64; o <<= 1) { const unsigned up = __shfl_up(incl, o); if (lane >= o) incl += up; }
      const unsigned total = __shfl(incl, 63);
      if (total < k) {
        if (lane == 0) { s_k = 0; s_prefix = 0; }  // (the first pass only: later passes count the k-th's own bin, which holds it)
      } else if (incl - own < k && k <= incl) {    // (one lane: the bins' running count passes k inside its four)
        unsigned before = incl - own;
        int b = 0;
        while (b < 3 && before + h[b] < k) { before += h[b]; b++; }
        s_prefix = prefix | ((unsigned long long)(4 * lane + b) << shift);
        s_k = k - before;
      }
    }
    __syncthreads();
    k = s_k; prefix = s_prefix;
    if (k == 0) break;  // (workgroup-uniform)
  }
  if (tid == 0) *const_cast<unsigned long long*>(env_ptr(bound, env, rec_stride)) = k == 0 ? kRankBoundInf : prefix;
}
}  // namespace mjpcx
