// park_settle.h -- the settling pass of a quad launch with a park hint (QArgs::park_hint, quad_abi.h). It runs on the stream right after
// rollout_quad_kernel, so the bound word holds its final value Bf: the least return a candidate of the launch completed with (or the
// caller's initial bound). A candidate parked on the unproven hint is now judged by the proven rule:
//   stored partial return > Bf  ->  retired: kQPruned | (step << 8), counted with the kernel's own retirements (prune_stats [0], [1])
//   otherwise                   ->  its index is appended to the resume list (rollout_quad_resume_kernel continues it from its record)
// words[0] += candidates parked, words[1] += candidates to resume (the two free words of the 64-byte stats block: they come back with the
// copy that fetches the hand-on count). A wavefront counts its candidates with ballots and adds each total once (most of a launch is
// parked: one atomic per candidate would be 15 k on one word). The resume list's order is the order of the wavefronts' appends, candidates
// of a wavefront in index order; no result depends on it.
//
// A launch with a bound per environment (mjpcx_set_pruning_batched: rec_stride != 0, env_n candidates per environment) keeps the
// environments apart here too. env_n is a multiple of 64, so a wavefront of this pass is one environment: it reads that environment's
// bound, adds to that environment's counters and words (its record: quad_abi.h, kQEnvRec*) and appends to that environment's segment of
// the resume list, which starts env_n entries after the one before -- `bound`, `prune_stats` and `words` are environment 0's.
#pragma once
#include <hip/hip_runtime.h>

#include "env_select.h"
#include "quad_abi.h"

namespace mjpcx {
__global__ __launch_bounds__(256) void park_settle_kernel(int N, const double* __restrict__ total_return, int* __restrict__ failure,
                                                          const unsigned long long* __restrict__ bound, int* __restrict__ prune_stats,
                                                          int* __restrict__ resume_list, int* __restrict__ words, int env_n, unsigned rec_stride) {
  const int cand = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // (the grid is whole workgroups of 256 and N only a multiple of 64: a wavefront wholly past N has no environment and no record to read.
  // It leaves here, before any pointer moves -- wavefront-uniform, so no ballot below misses a lane)
  if (__builtin_amdgcn_readfirstlane(cand) >= N) return;
  if (rec_stride) {  // (wavefront-uniform: the environment of the wavefront's first candidate)
    const int env = env_n > 0 ? __builtin_amdgcn_readfirstlane(cand) / env_n : 0;
    bound = env_ptr(bound, env, rec_stride);
    prune_stats = const_cast<int*>(env_ptr(prune_stats, env, rec_stride));
    words = const_cast<int*>(env_ptr(words, env, rec_stride));
    resume_list += (size_t)env * env_n;
  }
  // (no lane leaves before the ballots and shuffles: a candidate index past N is simply not parked)
  const int f = cand < N ? failure[cand] : 0;
  const bool parked = (f & kQParked) != 0 && (f & (kQFallback | kQPruned)) == 0;
  const double bf = __longlong_as_double((long long)*bound);
  const bool retire = parked && total_return[cand] > bf;
  const bool resume = parked && !retire;
  const unsigned long long m_parked = __ballot(parked), m_retire = __ballot(retire), m_resume = __ballot(resume);
  if (m_parked == 0) return;  // (wavefront-uniform)
  int steps = retire ? (f >> 8) & 0xFFFF : 0;
  for (int o = 32; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
  int base = 0;
  if (lane == 0) {
    atomicAdd(words, __popcll(m_parked));
    if (m_retire) { atomicAdd(prune_stats, __popcll(m_retire)); atomicAdd(prune_stats + 1, steps); }
    if (m_resume) base = atomicAdd(words + 1, __popcll(m_resume));  // (at most N appends in all, at most env_n to a segment: one per candidate)
  }
  base = __shfl(base, 0);
  if (retire) failure[cand] = (f & ~kQParked) | kQPruned;
  if (resume) resume_list[base + __popcll(m_resume & ((1ull << lane) - 1ull))] = cand;
}
}  // namespace mjpcx
