// mjpcx.hip -- implementation of the C ABI in include/mjpcx.h for gfx950.
//
// Host side of the drop-in boundary: validates the flat model, selects the rollout kernel
// instantiation whose static topology matches it, owns all device buffers, and exposes
// results in the reference's Trajectory layout. No CPU fallback exists: if no kernel
// matches the model, mjpcx_create fails with MJPCX_EUNSUPPORTED.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mjpcx.h"
#include "rollout_lane.h"
#include "lane_registry.h"
#include "ilqg_dense.h"
#include "gradient_pass.h"
#include "gradient_batched.h"
#include "ilqg_batched.h"
#include "rollout_wave.h"
#include "quad_launch.h"
#include "park_settle.h"
#include "rank_bound.h"
#include "wave_argmin.h"
#include "ensemble_best.h"
#include "mppi_update.h"
#include "cma_update.h"
#include "limb_launch.h"
#include "wave32_launch.h"
#include <type_traits>
#include <dlfcn.h>
#include <mutex>
#include <chrono>
#include <memory>
#include <thread>
#include <condition_variable>
#include <rccl/rccl.h>

using namespace mjpcx;

// ===================================================================== kernel registry
namespace {

struct TopoKey {
  int nb, nv, nu, nsite, nmocap;
  uint64_t parent, mocap, jtype, jbody, jlimited, actj, siteb;
  bool operator==(const TopoKey& o) const {
    return nb == o.nb && nv == o.nv && nu == o.nu && nsite == o.nsite && nmocap == o.nmocap && parent == o.parent &&
           mocap == o.mocap && jtype == o.jtype && jbody == o.jbody && jlimited == o.jlimited && actj == o.actj &&
           siteb == o.siteb;
  }
};
struct TaskKey {
  int rid, nr, nterm, ntrace;
  uint64_t termdim, tracesite;
  bool operator==(const TaskKey& o) const {
    return rid == o.rid && nr == o.nr && nterm == o.nterm && ntrace == o.ntrace && termdim == o.termdim &&
           tracesite == o.tracesite;
  }
};
template <class TP> constexpr TopoKey topo_key() {
  return {TP::NB, TP::NV, TP::NU, TP::NSITE, TP::NMOCAP, TP::kParent, TP::kMocap, TP::kJtype,
          TP::kJbody, TP::kJlimited, TP::kActj, TP::kSiteb};
}
template <class TK> constexpr TaskKey task_key() {
  return {TK::RID, TK::NR, TK::NTERM, TK::NTRACE, TK::kTermDim, TK::kTraceSite};
}

template <class TP, class TK, typename T>
hipError_t launch_lane(const LaneModel<T>& m, const LaneTask<T>& tk, const RolloutArgs<T>& a, hipStream_t s) {
  return launch_lane_impl<TP, TK, T, RuntimeModel>(m, tk, a, s);
}

struct KernelEntry {
  const char* name;
  TopoKey topo;
  TaskKey task;
  const LaneModel<double>* static_model;  // non-null: instantiation specialised for exactly these constants
  hipError_t (*launch64)(const LaneModel<double>&, const LaneTask<double>&, const RolloutArgs<double>&, hipStream_t);
  hipError_t (*launch32)(const LaneModel<float>&, const LaneTask<float>&, const RolloutArgs<float>&, hipStream_t);
  hipError_t (*feedback64)(const LaneModel<double>&, const LaneTask<double>&, const RolloutArgs<double>&, const FeedbackArgs<double>&, hipStream_t);
  hipError_t (*feedback32)(const LaneModel<float>&, const LaneTask<float>&, const RolloutArgs<float>&, const FeedbackArgs<float>&, hipStream_t);
  hipError_t (*fd64)(const LaneModel<double>&, const LaneTask<double>&, const FdArgs<double>&, hipStream_t);
  hipError_t (*fd32)(const LaneModel<float>&, const LaneTask<float>&, const FdArgs<float>&, hipStream_t);
};
template <class TP, class TK, typename T>
hipError_t launch_feedback(const LaneModel<T>& m, const LaneTask<T>& tk, const RolloutArgs<T>& a, const FeedbackArgs<T>& fb, hipStream_t s) {
  return launch_feedback_impl<TP, TK, T, RuntimeModel>(m, tk, a, fb, s);
}
template <class TP, class TK, typename T>
hipError_t launch_fd(const LaneModel<T>& m, const LaneTask<T>& tk, const FdArgs<T>& f, hipStream_t s) {
  return launch_fd_impl<TP, TK, T, RuntimeModel>(m, tk, f, s);
}
#define MJPCX_LANE_ENTRY(TP, TK) \
  { "rollout_lane<" #TP "," #TK ">", topo_key<TP>(), task_key<TK>(), nullptr, &launch_lane<TP, TK, double>, &launch_lane<TP, TK, float>, \
    &launch_feedback<TP, TK, double>, &launch_feedback<TP, TK, float>, &launch_fd<TP, TK, double>, &launch_fd<TP, TK, float> }
#define MJPCX_STATIC_ENTRY(TP, TK, GEN, FN) \
  { "rollout_lane<" #TP "," #TK "," #GEN ">", topo_key<TP>(), task_key<TK>(), &kHost##GEN, &FN##_f64, &FN##_f32, \
    &FN##_fb_f64, &FN##_fb_f32, &FN##_fd_f64, &FN##_fd_f32 }
const LaneModel<double> kHostStaticCartpole = make_Cartpole<double>();
const LaneModel<double> kHostStaticParticle = make_Particle<double>();
// specialised entries first: mjpcx_create takes the first entry whose key (and constants) match
const KernelEntry kKernels[] = {
    MJPCX_STATIC_ENTRY(TopoCartpole, TaskCartpole, StaticCartpole, launch_static_cartpole),
    MJPCX_STATIC_ENTRY(TopoParticle, TaskParticle, StaticParticle, launch_static_particle),
    MJPCX_STATIC_ENTRY(TopoParticle, TaskParticleCopy, StaticParticle, launch_static_particle_copy),
    MJPCX_LANE_ENTRY(TopoCartpole, TaskCartpole),
    MJPCX_LANE_ENTRY(TopoParticle, TaskParticle),
    MJPCX_LANE_ENTRY(TopoParticle, TaskParticleCopy),
};

// the wavefront-per-candidate family is selected by model FEATURES (free/ball joints, friction loss, contacts),
// not by topology: one generic kernel that reads the model through WaveModel
const KernelEntry kTreeEntryA1 = {"rollout_tree_kernel<A1> (registered model: hot arrays staged in LDS behind compile-time offsets, persistent wavefronts, "
                                   "Jacobian-free Newton contact solver)", TopoKey{}, TaskKey{}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
const KernelEntry kTreeEntryHumanoid = {"rollout_tree_kernel<Humanoid> (registered model: hot arrays staged in LDS behind compile-time offsets, persistent wavefronts, "
                                         "Jacobian-free Newton contact solver: pyramidal cones, tendon limits)", TopoKey{}, TaskKey{}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
const KernelEntry kQuadEntryA1 = {"rollout_quad_kernel (four lanes per candidate, one per leg: 16 candidates per wavefront, arrowhead Newton contact solver; "
                                   "candidates it hands on run rollout_tree_kernel<A1>)", TopoKey{}, TaskKey{}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
const KernelEntry kLimbEntryHumanoid = {"rollout_limb_kernel (four lanes per candidate, one per limb: up to 16 candidates per wavefront, arrowhead Newton contact solver with "
                                         "Woodbury terms for contacts between moving geoms; candidates it hands on run rollout_tree_kernel<Humanoid>)",
                                         TopoKey{}, TaskKey{}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
const KernelEntry kWaveEntry = {"rollout_wave_kernel (wavefront per candidate, model in LDS/L1; Newton contact solver)",
                                TopoKey{}, TaskKey{}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

// ===================================================================== small kernels
// argmin / top-k over total_return: replaces std::partial_sort (sampling/planner.cc:184-188).
// Keys are (return, index) with ties broken by index, so the result is deterministic.
// (RetIdx, less_ri: wave_argmin.h)
__global__ __launch_bounds__(1024) void argmin_kernel(const double* __restrict__ ret, int n, RetIdx* out) {
  __shared__ RetIdx sm[16];
  RetIdx best{INFINITY, 0x7fffffff};
  best.r = ret[0] != ret[0] ? ret[0] : INFINITY;  // keep NaN ordering consistent when everything is NaN
  best.i = 0x7fffffff;
  bool have = false;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    RetIdx c{ret[i], i};
    if (!have || less_ri(c, best)) { best = c; have = true; }
  }
  if (!have) { best.r = NAN; best.i = 0x7fffffff; }
  // wave-level reduction over 64 lanes
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    RetIdx o;
    o.r = __shfl_down(best.r, off, 64);
    o.i = __shfl_down(best.i, off, 64);
    if (less_ri(o, best)) best = o;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sm[wave] = best;
  __syncthreads();
  if (wave == 0) {
    const int nw = blockDim.x >> 6;
    best = lane < nw ? sm[lane] : RetIdx{NAN, 0x7fffffff};
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      RetIdx o;
      o.r = __shfl_down(best.r, off, 64);
      o.i = __shfl_down(best.i, off, 64);
      if (less_ri(o, best)) best = o;
    }
    if (lane == 0) out[0] = best;
  }
}
// The policy update of Predictive Sampling needs, from one rollout batch: the winner's index
// and return, its spline values (candidate_policy[winner], sampling/planner.cc:534-543) and the
// nominal candidate's return (`improvement`, planner.cc:207-208). One launch writes them all
// into a pinned, device-mapped host record, so the host pays exactly one stream sync per plan step.
struct BestRecord { double best_return, ref_return; int best_index, ref_failure; double spline[1]; };
static_assert(offsetof(BestRecord, spline) == 24, "mjpcx_best_batched packs the records at 24 bytes + the spline values");
template <typename T>
__global__ __launch_bounds__(1024) void best_kernel(const double* __restrict__ ret, const int* __restrict__ fail,
                                                     const T* __restrict__ nodes, int n, int np, int ref, BestRecord* out) {
  __shared__ RetIdx sm[16];
  __shared__ int winner;
  RetIdx best{NAN, 0x7fffffff};
  bool have = false;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    RetIdx c{ret[i], i};
    if (!have || less_ri(c, best)) { best = c; have = true; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    RetIdx o;
    o.r = __shfl_down(best.r, off, 64);
    o.i = __shfl_down(best.i, off, 64);
    if (less_ri(o, best)) best = o;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sm[wave] = best;
  __syncthreads();
  if (wave == 0) {
    const int nw = blockDim.x >> 6;
    best = lane < nw ? sm[lane] : RetIdx{NAN, 0x7fffffff};
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      RetIdx o;
      o.r = __shfl_down(best.r, off, 64);
      o.i = __shfl_down(best.i, off, 64);
      if (less_ri(o, best)) best = o;
    }
    if (lane == 0) {
      winner = best.i;
      out->best_return = best.r;
      out->best_index = best.i;
      out->ref_return = (ref >= 0 && ref < n) ? ret[ref] : NAN;
      out->ref_failure = (ref >= 0 && ref < n) ? fail[ref] : 0;
    }
  }
  __syncthreads();
  const int w = winner;
  if (w >= 0 && w < n)
    for (int j = threadIdx.x; j < np; j += blockDim.x) out->spline[j] = (double)nodes[(size_t)j * n + w];
}

// The same reads for E environments in one launch (mjpcx_best_batched): one workgroup per environment over its n_env returns,
// environment-major, reduced with wave_argmin (wave_argmin.h).
constexpr size_t kBestHeader = 24;  // bytes of a BestRecord before its spline values
template <typename T>
__global__ __launch_bounds__(256) void best_segmented_kernel(const double* __restrict__ ret, const int* __restrict__ fail, const T* __restrict__ nodes,
                                                              int N, int n_env, int np, int ref, unsigned char* out, unsigned rec_bytes) {
  __shared__ RetIdx sm[4];
  const int env = blockIdx.x, first = env * n_env;
  RetIdx best{NAN, 0x7fffffff};  // (sorts behind every candidate)
  for (int i = threadIdx.x; i < n_env; i += 256) {
    const RetIdx c{ret[first + i], i};
    if (less_ri(c, best)) best = c;
  }
  best = wave_argmin(best);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sm[wave] = best;
  __syncthreads();
  best = wave_argmin(lane < 4 ? sm[lane] : RetIdx{NAN, 0x7fffffff});  // (every wavefront: the winner without a second barrier)
  BestRecord* rec = reinterpret_cast<BestRecord*>(out + (size_t)env * rec_bytes);
  if (threadIdx.x == 0) {
    rec->best_return = best.r;
    rec->best_index = best.i;  // local to the environment
    rec->ref_return = (ref >= 0 && ref < n_env) ? ret[first + ref] : NAN;
    rec->ref_failure = (ref >= 0 && ref < n_env) ? fail[first + ref] : 0;
  }
  const int w = best.i;
  if (w >= 0 && w < n_env)
    for (int j = threadIdx.x; j < np; j += 256) rec->spline[j] = (double)nodes[(size_t)j * N + first + w];
}

// elite moments: one workgroup per spline parameter j, fixed-shape tree reduction (deterministic). elite_reduce is the reduction of
// both elite kernels (this one and ce_update_kernel): 256 strided partial sums over the elites in rank order, then the halving tree.
// `t` is the thread's place among the 256 of its reduction, `sm` their 256 doubles; every thread of the workgroup calls it. The
// candidate indices are relative to `nodes_j` (row j of the [P*nu][N] spline nodes) and `ret`; mean_j == nullptr: plain sums.
template <typename T>
__device__ __forceinline__ double elite_reduce(const T* __restrict__ nodes_j, const double* __restrict__ ret, const int* cand, int n,
                                               const double* mean_j, int t, double* sm) {
  double acc = 0;
  for (int i = t; i < n; i += 256) {
    const int c = cand[i];
    if (nodes_j) {
      const double p = (double)nodes_j[c];
      if (mean_j) { const double d = p - mean_j[0]; acc += d * d; } else acc += p;
    } else {
      acc += ret[c];
    }
  }
  sm[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sm[t] += sm[t + s];
    __syncthreads();
  }
  return sm[0];
}
template <typename T>
__global__ __launch_bounds__(256) void elite_moments_kernel(const T* __restrict__ nodes, const double* __restrict__ ret,
                                                            const int* __restrict__ cand, int n, int N, int np,
                                                            const double* __restrict__ mean, double* out) {
  __shared__ double sm[256];
  const int j = blockIdx.x;  // j == np: the return sum
  const double r = elite_reduce<T>(j < np ? nodes + (size_t)j * N : nullptr, ret, cand, n, mean && j < np ? mean + j : nullptr, threadIdx.x, sm);
  if (threadIdx.x == 0) out[j] = r;
}

// The cross-entropy update of E environments in one launch (mjpcx_ce_update_batched): one workgroup of 16 wavefronts per environment.
//  1. Selection: a bitonic sort of the environment's (return, local index) keys by less_ri, padded to n2 = 2^m >= 1024 with keys that
//     sort last; the candidate to skip (the nominal rollout) is one of them. Split layout, returns [n2] then indices [n2]: 12 bytes a
//     key, so n2 <= 8192 sorts in 96 KiB of LDS (IN_LDS); larger environments sort in a global scratch slab of the same layout.
//     Element i belongs to thread i % 1024, so a compare-exchange at distance j < 64 pairs two lanes of one wavefront: those steps run
//     on registers -- DPP quad_perm for j = 1, 2, ds_bpermute above -- six of them between two barriers. Only the steps at distance
//     >= 64 go through memory with a barrier each: 45 barriers for 16384 keys instead of 105.
//  2. Moments: the elites are the first n_elite keys. The four quarters of the workgroup take the parameters j in turn, each with
//     elite_reduce -- the sum, the mean from it, then the squares about that mean, all fp64 -- so the result equals
//     mjpcx_topk + 2 x mjpcx_elite_moments + the host's divisions. No atomics: a second call gives the same bits.
// Everything goes to the environment's pinned, device-mapped record [avg_return | index | total_return | mean | variance].
template <int JJ> __device__ __forceinline__ RetIdx lane_xor_ri(const RetIdx& v) {
  if constexpr (JJ == 1) return dpp_ri<0xB1>(v);       // quad_perm:[1,0,3,2]
  else if constexpr (JJ == 2) return dpp_ri<0x4E>(v);  // quad_perm:[2,3,0,1]
  else { RetIdx o; o.r = __shfl_xor(v.r, JJ, 64); o.i = __shfl_xor(v.i, JJ, 64); return o; }
}
// compare-exchange of element i with element i ^ JJ (a lane of the same wavefront) in the merge of blocks of k
template <int JJ> __device__ __forceinline__ void lane_cmpx(RetIdx& v, int i, int k) {
  const RetIdx o = lane_xor_ri<JJ>(v);
  const bool keep_min = ((i & JJ) == 0) == ((i & k) == 0);
  if (keep_min ? less_ri(o, v) : less_ri(v, o)) v = o;
}
__device__ __forceinline__ void lane_merge(RetIdx& v, int i, int k) {  // the steps of distance < 64 of the merge of blocks of k
  if (k > 32) lane_cmpx<32>(v, i, k);
  if (k > 16) lane_cmpx<16>(v, i, k);
  if (k > 8) lane_cmpx<8>(v, i, k);
  if (k > 4) lane_cmpx<4>(v, i, k);
  if (k > 2) lane_cmpx<2>(v, i, k);
  lane_cmpx<1>(v, i, k);
}
constexpr int kSortKeyBytes = sizeof(double) + sizeof(int);  // env_sort_keys' layout: n2 returns, then n2 indices
constexpr int kCeLdsKeys = 8192;  // 12 bytes a key: 96 KiB of a CU's 160 KiB of LDS
static_assert(kCeLdsKeys * kSortKeyBytes == 96 * 1024, "the keys sorted in LDS take 96 KiB");
struct CeRecord { size_t bytes, off_index, off_ret, off_mean, off_var; };  // avg_return at 0
// The selection (step 1 above), shared by ce_update_kernel and robust_select_kernel: every thread of a workgroup of 1024 calls it; on
// return keys[0..n2) / idx[0..n2) hold the environment's returns and local indices in less_ri order, visible to the whole workgroup.
__device__ __forceinline__ void env_sort_keys(const double* __restrict__ ret, int first, int n_env, int n2, int skip, double* keys, int* idx, int tid) {
  // n2 is a multiple of 1024: every lane is active in every round of the loops over i
  for (int i = tid; i < n2; i += 1024) {
    RetIdx v = i < n_env && i != skip ? RetIdx{ret[first + i], i} : RetIdx{NAN, 0x7fffffff};
    for (int k = 2; k <= 64; k <<= 1) lane_merge(v, i, k);
    keys[i] = v.r; idx[i] = v.i;
  }
  __syncthreads();
  for (int k = 128; k <= n2; k <<= 1) {
    for (int j = k >> 1; j >= 64; j >>= 1) {
      for (int i = tid; i < n2; i += 1024) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & k) == 0;
          const RetIdx a{keys[i], idx[i]}, b{keys[l], idx[l]};
          if (less_ri(b, a) == up) { keys[i] = b.r; idx[i] = b.i; keys[l] = a.r; idx[l] = a.i; }
        }
      }
      __syncthreads();
    }
    for (int i = tid; i < n2; i += 1024) {
      RetIdx v{keys[i], idx[i]};
      lane_merge(v, i, k);
      keys[i] = v.r; idx[i] = v.i;
    }
    __syncthreads();
  }
}
template <typename T, bool IN_LDS>
__global__ __launch_bounds__(1024) void ce_update_kernel(const double* __restrict__ ret, const T* __restrict__ nodes, int N, int n_env, int n2, int np,
                                                          int n_elite, int skip, double* scratch, unsigned char* out, CeRecord rec) {
  extern __shared__ __attribute__((aligned(16))) double ce_lds[];
  __shared__ double sm[4][256];
  __shared__ double sm_mean[4];
  const int env = blockIdx.x, first = env * n_env, tid = threadIdx.x;
  double* keys;
  int* idx;
  if constexpr (IN_LDS) { keys = ce_lds; idx = reinterpret_cast<int*>(ce_lds + n2); }
  else { keys = scratch + (size_t)env * (n2 + n2 / 2); idx = reinterpret_cast<int*>(keys + n2); }
  env_sort_keys(ret, first, n_env, n2, skip, keys, idx, tid);
  unsigned char* r = out + (size_t)env * rec.bytes;
  int* o_index = reinterpret_cast<int*>(r + rec.off_index);
  double* o_ret = reinterpret_cast<double*>(r + rec.off_ret);
  double* o_mean = reinterpret_cast<double*>(r + rec.off_mean);
  double* o_var = reinterpret_cast<double*>(r + rec.off_var);
  for (int i = tid; i < n_elite; i += 1024) { o_index[i] = idx[i]; o_ret[i] = keys[i]; }
  const int g = tid >> 8, t = tid & 255;  // quarter g reduces parameter j0 + g; j == np: the returns
  for (int j0 = 0; j0 <= np; j0 += 4) {
    const int j = j0 + g;
    const bool live = j <= np;
    const T* nodes_j = live && j < np ? nodes + (size_t)j * N + first : nullptr;
    const double sum = elite_reduce<T>(nodes_j, ret + first, idx, live ? n_elite : 0, nullptr, t, sm[g]);
    if (t == 0) sm_mean[g] = sum / n_elite;
    __syncthreads();
    const double sq = elite_reduce<T>(nodes_j, ret + first, idx, live && j < np ? n_elite : 0, &sm_mean[g], t, sm[g]);
    if (t == 0 && live) {
      if (j < np) { o_mean[j] = sm_mean[g]; o_var[j] = sq / (n_elite - 1); }
      else reinterpret_cast<double*>(r)[0] = sm_mean[g];
    }
    __syncthreads();
  }
}

// The Robust planner's plan step for E environments (mjpcx_robust_step_batched), two kernels around the batched noisy rollout; one
// workgroup per environment each. The environment's record, pinned and device-mapped:
// [best (i32) | candidate (k i32) | candidate_return (k f64) | perturbed_score (k f64) | valid (k i32) | spline (np f64)].
struct RobustRecord { size_t bytes, off_index, off_ret, off_score, off_valid, off_spline; };
//  1. Select and expand: the k best of the environment's n_src returns of the SOURCE context, in the order of ce_update_kernel without
//     a skip (env_sort_keys), -> the record; every chosen spline R times into this context's node buffer ([node * nu][candidate], what
//     scatter_nodes_kernel writes; both contexts hold one precision: a copy). Local rollout j = rank * R + rep; the share is padded to
//     n_pad, a multiple of 64, with the last rank's spline.
template <typename T, bool IN_LDS>
__global__ __launch_bounds__(1024) void robust_select_kernel(const double* __restrict__ src_ret, const T* __restrict__ src_nodes, int N_src, int n_src,
                                                              int n2, int np, int k, int R, int n_pad, double* scratch, T* nodes, unsigned char* out,
                                                              RobustRecord rec) {
  extern __shared__ __attribute__((aligned(16))) double ce_lds[];
  const int env = blockIdx.x, first = env * n_src, tid = threadIdx.x;
  double* keys;
  int* idx;
  if constexpr (IN_LDS) { keys = ce_lds; idx = reinterpret_cast<int*>(ce_lds + n2); }
  else { keys = scratch + (size_t)env * (n2 + n2 / 2); idx = reinterpret_cast<int*>(keys + n2); }
  env_sort_keys(src_ret, first, n_src, n2, -1, keys, idx, tid);
  unsigned char* r = out + (size_t)env * rec.bytes;
  int* o_index = reinterpret_cast<int*>(r + rec.off_index);
  double* o_ret = reinterpret_cast<double*>(r + rec.off_ret);
  for (int i = tid; i < k; i += 1024) { o_index[i] = idx[i]; o_ret[i] = keys[i]; }
  const size_t N = (size_t)gridDim.x * n_pad, to = (size_t)env * n_pad;
  for (int i = tid; i < np * n_pad; i += 1024) {  // consecutive threads write consecutive rollouts of one node row
    const int j = i / n_pad, slot = i - j * n_pad;
    const int rank = min(slot / R, k - 1);
    nodes[(size_t)j * N + to + slot] = src_nodes[(size_t)j * N_src + first + idx[rank]];
  }
}
//  2. Score: per rank the running mean of RobustPlanner::OptimizePolicy in its order of operations -- from the candidate's unperturbed
//     return, mean = (valid * mean + ret) / (valid + 1) over the repetitions that did not fail, plain fp64, nothing contracted --, then
//     the planner's argmin: strict < from rank 0 up, so the lowest rank wins a tie and a NaN never beats an earlier rank (rank 0 stays
//     when its own score is NaN; otherwise that is less_ri's minimum). The winner's spline is gathered in the same launch.
template <typename T>
__global__ __launch_bounds__(256) void robust_score_kernel(const double* __restrict__ ret, const int* __restrict__ fail, const T* __restrict__ nodes,
                                                            int np, int k, int R, int n_pad, unsigned char* out, RobustRecord rec) {
#pragma clang fp contract(off)
  __shared__ RetIdx sm[4];
  __shared__ double score0;
  const int env = blockIdx.x, tid = threadIdx.x;
  const size_t N = (size_t)gridDim.x * n_pad, first = (size_t)env * n_pad;
  unsigned char* r = out + (size_t)env * rec.bytes;
  const double* o_ret = reinterpret_cast<const double*>(r + rec.off_ret);
  double* o_score = reinterpret_cast<double*>(r + rec.off_score);
  int* o_valid = reinterpret_cast<int*>(r + rec.off_valid);
  RetIdx best{NAN, 0x7fffffff};  // (sorts behind every rank)
  for (int c = tid; c < k; c += 256) {
    double mean = o_ret[c];
    int valid = 0;
    for (int j = 0; j < R; j++) {
      if (fail[first + (size_t)c * R + j]) continue;
      const double total = ret[first + (size_t)c * R + j];
      mean = (valid * mean + total) / (valid + 1);
      valid++;
    }
    o_score[c] = mean;
    o_valid[c] = valid;
    if (c == 0) score0 = mean;
    const RetIdx v{mean, c};
    if (less_ri(v, best)) best = v;
  }
  best = wave_argmin(best);
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) sm[wave] = best;
  __syncthreads();
  best = wave_argmin(lane < 4 ? sm[lane] : RetIdx{NAN, 0x7fffffff});
  const int w = score0 != score0 ? 0 : best.i;
  if (tid == 0) reinterpret_cast<int*>(r)[0] = w;
  double* o_spline = reinterpret_cast<double*>(r + rec.off_spline);
  for (int j = tid; j < np; j += 256) o_spline[j] = (double)nodes[(size_t)j * N + first + (size_t)w * R];
}

// The Sample-Gradient planner's plan step for E environments (mjpcx_rollout_sample_gradient_batched, mjpcx_sample_gradient_update_batched):
// two kernels around the batched rollout. Everything is fp64 with nothing contracted, whatever the context's precision: the same
// additions, multiplications and divisions in numpy (planners.sample_gradient_update) give the same bits from the same normals.
struct SgCandArgs {
  int n, num_noisy, P, nu, interp, num_envs, blocks_per_env;
  const double *times, *nominal, *range;   // this step's node times E x P, nominals E x P*nu, ctrlrange 2 nu
  const double *grad_times, *grad_values;  // the gradient candidates: their node times E x P, values E x G x P*nu
  double noise_exploration;
  uint64_t seed;
  uint32_t iteration;
};
// TimeSpline::Sample (spline.cc:103-156) of actuator k of one spline at `time`: std::upper_bound, the end nodes held outside the grid,
// zero / linear / cubic Hermite with the finite-difference slopes of spline.cc:269-287, in the order of operations of spline.py.
__device__ __forceinline__ double sg_spline_sample(const double* __restrict__ ts, const double* __restrict__ vs, int P, int nu, int k, int interp, double time) {
#pragma clang fp contract(off)
  int up = 0;
  while (up < P && !(time < ts[up])) up++;
  if (up == P) return vs[(size_t)(P - 1) * nu + k];
  if (up == 0) return vs[k];
  const int lo = up - 1;
  const double tl = ts[lo], tu = ts[up], t = (time - tl) / (tu - tl);
  const double vl = vs[(size_t)lo * nu + k], vu = vs[(size_t)up * nu + k];
  if (interp == 0) return vl;
  if (interp == 1) return vl * (1 - t) + vu * t;
  auto slope = [&](int node) {
    const double v = vs[(size_t)node * nu + k];
    if (node == 0) return (vs[(size_t)nu + k] - v) / (ts[1] - ts[0]);
    if (node == P - 1) return (v - vs[(size_t)(node - 1) * nu + k]) / (ts[node] - ts[node - 1]);
    return 0.5 * (vs[(size_t)(node + 1) * nu + k] - v) / (ts[node + 1] - ts[node]) + 0.5 * (v - vs[(size_t)(node - 1) * nu + k]) / (ts[node] - ts[node - 1]);
  };
  const double c0 = 2.0 * t * t * t - 3.0 * t * t + 1.0;
  const double c1 = (t * t * t - 2.0 * t * t + t) * (tu - tl);
  const double c2 = -2.0 * t * t * t + 3 * t * t;
  const double c3 = (t * t * t - t * t) * (tu - tl);
  return c0 * vl + c1 * slope(lo) + c2 * vu + c3 * slope(up);
}
//  1. Candidates (sample_gradient/planner.cc:355-400, 290-352): one thread per (local candidate c, parameter pair q) of an environment
//     (blocks_per_env workgroups each), consecutive threads consecutive candidates, so the stores into the [parameter][candidate] node rows are coalesced.
//     c = 0 the nominal as it came; 0 < c < num_noisy clamp(nominal + noise_exploration z), z = gaussian_pair(seed + e, c, q, iteration)
//     -- ONE Philox + Box-Muller for the two parameters of the pair, not scaled by the control range --; c >= num_noisy the gradient
//     candidate c - num_noisy, its own spline over grad_times, sampled at this step's node times and clamped (ResamplePolicy).
template <typename T>
__global__ __launch_bounds__(256) void sg_candidates_kernel(const SgCandArgs a, T* __restrict__ nodes) {
#pragma clang fp contract(off)
  const int env = blockIdx.x / a.blocks_per_env, n = a.n, np = a.P * a.nu, G = n - a.num_noisy;
  const int work = (blockIdx.x - env * a.blocks_per_env) * 256 + threadIdx.x;
  const int q = work / n, c = work - q * n;
  if (2 * q >= np) return;
  const size_t N = (size_t)a.num_envs * n, at = (size_t)env * n + c;
  const double* nominal = a.nominal + (size_t)env * np;
  double z[2] = {0.0, 0.0};
  if (c > 0 && c < a.num_noisy) gaussian_pair(a.seed + (uint64_t)env, (uint32_t)c, (uint32_t)q, a.iteration, z);
  for (int e = 0; e < 2; e++) {
    const int j = 2 * q + e;
    if (j >= np) break;
    const int p = j / a.nu, k = j - p * a.nu;
    const double lo = a.range[2 * k], hi = a.range[2 * k + 1];
    double v = nominal[j];
    if (c >= a.num_noisy)
      v = clampv(sg_spline_sample(a.grad_times + (size_t)env * a.P, a.grad_values + ((size_t)env * G + (c - a.num_noisy)) * np, a.P, a.nu, k, a.interp,
                                  a.times[(size_t)env * a.P + p]), lo, hi);
    else if (c > 0)
      v = clampv(v + a.noise_exploration * z[e], lo, hi);
    nodes[(size_t)j * N + at] = (T)v;
  }
}
//  2. Update (planner.cc:168-264, 401-493): workgroups (environment, chunk of four parameter pairs) of 1024 threads. Every workgroup
//     sorts its environment's returns with env_sort_keys -- all n of them, or with MJPCX_SG_COMPUTE_WEIGHTS the first num_noisy only,
//     as the reference does in that step; chunk 0 then finds the winner as the less_ri minimum of the sorted head and the rest.
//     The reference's behaviour is kept exactly, not repaired: the shaping weight of sorted position i takes the logarithm of the
//     CANDIDATE INDEX at that position, log(order[i] + 1), not of the rank; the weights are cached and on later steps pair with the
//     first num_noisy entries of the order over ALL candidates, where the nominal and the gradient candidates carry zero noise.
//     Summation order (den and every gradient entry alike): thread t of a quarter of the workgroup adds the terms of the sorted
//     positions t, t + 256, t + 512, ... in that order, starting from 0; the 256 partial sums meet in a halving tree,
//     s = 128, 64, ..., 1: sum[t] += sum[t + s]. The quarters take one pair each; z is re-drawn from the counter, never stored.
//     log(k + 1) comes from a table the host computed (`logs`), so the device adds, multiplies and divides only.
struct SgRecord { size_t bytes, off_spline, off_grad; };  // [index (i32) | winner_type (i32) | best | nominal | improvement | spline (np) | gradient (np)]
struct SgUpdateArgs {
  int n, n2, P, nu, G, num_noisy, flags;
  double filter, noise_exploration, f0;
  uint64_t seed;
  uint32_t iteration;
  const double *times, *nominal, *range, *logs, *steps;  // E x P, E x P*nu, 2 nu, log(k + 1) for k < num_noisy, LogScale step sizes G
  double *gradient, *gradient_previous, *weights, *grad_times, *grad_values;  // the context's: E x P*nu (two), E x num_noisy, E x P, E x G x P*nu
};
__device__ __forceinline__ double sg_tree256(double v, int t, double* sm) {  // every thread of the workgroup calls it
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
template <typename T, bool IN_LDS>
__global__ __launch_bounds__(1024) void sg_update_kernel(const double* __restrict__ ret, const T* __restrict__ nodes, const SgUpdateArgs a, double* scratch,
                                                          unsigned char* out, SgRecord rec) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double ce_lds[];
  __shared__ double sm[2][4][256];
  __shared__ RetIdx smin[16];
  const int env = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x, n = a.n, nn = a.num_noisy, np = a.P * a.nu, first = env * n;
  const size_t N = (size_t)gridDim.x * n;
  double* keys;
  int* idx;
  if constexpr (IN_LDS) { keys = ce_lds; idx = reinterpret_cast<int*>(ce_lds + a.n2); }
  else { keys = scratch + ((size_t)env * gridDim.y + chunk) * (a.n2 + a.n2 / 2); idx = reinterpret_cast<int*>(keys + a.n2); }
  const bool compute = a.G > 0 && (a.flags & MJPCX_SG_COMPUTE_WEIGHTS), zero = (a.flags & MJPCX_SG_ZERO_GRADIENT) != 0;
  const int sorted = compute ? nn : n;
  env_sort_keys(ret, first, sorted, a.n2, -1, keys, idx, tid);
  unsigned char* r = out + (size_t)env * rec.bytes;
  double* o_grad = reinterpret_cast<double*>(r + rec.off_grad);
  if (chunk == 0) {
    RetIdx rest{NAN, 0x7fffffff};  // (sorts behind every candidate)
    for (int c = sorted + tid; c < n; c += 1024) {
      const RetIdx v{ret[first + c], c};
      if (less_ri(v, rest)) rest = v;
    }
    rest = wave_argmin(rest);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) smin[wave] = rest;
    __syncthreads();
    rest = wave_argmin(lane < 16 ? smin[lane] : RetIdx{NAN, 0x7fffffff});
    RetIdx best{keys[0], idx[0]};
    if (less_ri(rest, best)) best = rest;
    const double r0 = ret[first];
    const int w = best.r < r0 ? best.i : 0;  // a strict improvement on the nominal, or the nominal
    if (tid == 0) {
      const double rw = ret[first + w], d = r0 - rw;
      reinterpret_cast<int*>(r)[0] = w;
      reinterpret_cast<int*>(r)[1] = w == 0 ? 0 : (w < nn ? 1 : 2);
      reinterpret_cast<double*>(r)[1] = rw;
      reinterpret_cast<double*>(r)[2] = r0;
      reinterpret_cast<double*>(r)[3] = d > 0 ? d : 0.0;
    }
    double* o_spline = reinterpret_cast<double*>(r + rec.off_spline);
    for (int j = tid; j < np; j += 1024) o_spline[j] = (double)nodes[(size_t)j * N + first + w];
    if (a.G < 1) {  // GradientCandidates returns at once: the gradient stays as it is (or as Reset left it)
      for (int j = tid; j < np; j += 1024) {
        const double g = zero ? 0.0 : a.gradient[(size_t)env * np + j];
        if (zero) a.gradient[(size_t)env * np + j] = 0.0;
        o_grad[j] = g;
      }
    } else {
      for (int p = tid; p < a.P; p += 1024) a.grad_times[(size_t)env * a.P + p] = a.times[(size_t)env * a.P + p];
    }
  }
  if (a.G < 1) return;
  const int quarter = tid >> 8, t = tid & 255;
  double den = 0.0;
  if (compute) {
    double acc = 0.0;
    for (int i = t; i < nn; i += 256) {
      const double f = a.f0 - a.logs[idx[i]];
      acc += f > 0 ? f : 0.0;
    }
    den = sg_tree256(acc, t, sm[0][quarter]);
  }
  double* weights = a.weights + (size_t)env * nn;
  auto weight = [&](int i) {
    if (!compute) return weights[i];
    const double f = a.f0 - a.logs[idx[i]];
    return (f > 0 ? f : 0.0) / den - 1.0 / nn;
  };
  if (compute && chunk == 0)
    for (int i = tid; i < nn; i += 1024) weights[i] = weight(i);
  const int q = chunk * 4 + quarter;
  const bool live = 2 * q < np;
  double acc0 = 0.0, acc1 = 0.0;
  if (live)
    for (int i = t; i < nn; i += 256) {
      const int c = idx[i];
      if (c < 1 || c >= nn) continue;  // the nominal and the gradient candidates carry no noise: a zero term
      const double wi = weight(i) / nn;
      double z[2];
      gaussian_pair(a.seed + (uint64_t)env, (uint32_t)c, (uint32_t)q, a.iteration, z);
      acc0 += z[0] * wi;
      acc1 += z[1] * wi;
    }
  const double sum[2] = {sg_tree256(acc0, t, sm[0][quarter]), sg_tree256(acc1, t, sm[1][quarter])};
  double old[2] = {0.0, 0.0};
  for (int e = 0; e < 2; e++) {
    const int j = 2 * q + e;
    if (live && j < np && !zero) old[e] = a.gradient[(size_t)env * np + j];
  }
  __syncthreads();  // every thread has the gradient of the step before
  for (int e = 0; e < 2; e++) {
    const int j = 2 * q + e;
    if (!live || j >= np) continue;
    if (t == 0) {
      a.gradient_previous[(size_t)env * np + j] = old[e];
      a.gradient[(size_t)env * np + j] = sum[e];
      o_grad[j] = sum[e];
    }
    // the next gradient candidates (planner.cc:463-480): two rounded additions per node, then the clamp
    const int k = j % a.nu;
    const double lo = a.range[2 * k], hi = a.range[2 * k + 1], nominal = a.nominal[(size_t)env * np + j];
    for (int g = t; g < a.G; g += 256) {
      const double scaling = a.steps[g] / a.noise_exploration;
      double v = nominal;
      v += -scaling * a.filter * sum[e];
      v += -scaling * (1.0 - a.filter) * old[e];
      a.grad_values[((size_t)env * a.G + g) * np + j] = clampv(v, lo, hi);
    }
  }
}

// CMA-ES (mjpcx_cma_update_batched, csrc/cma_update.h), the ranking: one workgroup of 1024 per environment sorts the returns of the
// candidates 1..n-1 with env_sort_keys (candidate 0, the mean, is skipped) -> rank[e] = [valid | the mu best, LOCAL indices]; valid = none
// of them is NaN (NaN sorts last: the mu-th key decides). The argmin over all n is the head of that order or candidate 0, by less_ri.
template <bool IN_LDS>
__global__ __launch_bounds__(1024) void cma_rank_kernel(const double* __restrict__ ret, int n, int n2, int mu, double* scratch, int* rank,
                                                         unsigned char* out, unsigned rec_bytes) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double ce_lds[];
  const int env = blockIdx.x, first = env * n, tid = threadIdx.x;
  double* keys;
  int* idx;
  if constexpr (IN_LDS) { keys = ce_lds; idx = reinterpret_cast<int*>(ce_lds + n2); }
  else { keys = scratch + (size_t)env * (n2 + n2 / 2); idx = reinterpret_cast<int*>(keys + n2); }
  env_sort_keys(ret, first, n, n2, 0, keys, idx, tid);
  int* r = rank + (size_t)env * (1 + mu);
  for (int i = tid; i < mu; i += 1024) r[1 + i] = idx[i];
  if (tid == 0) {
    r[0] = keys[mu - 1] == keys[mu - 1] ? 1 : 0;
    const RetIdx head{keys[0], idx[0]}, mean{ret[first], 0};
    const RetIdx best = less_ri(mean, head) ? mean : head;
    const double gain = mean.r - best.r;
    CmaRecord* rec = reinterpret_cast<CmaRecord*>(out + (size_t)env * rec_bytes);
    rec->index = best.i;
    rec->best_return = best.r;
    rec->nominal_return = mean.r;
    rec->improvement = gain > 0 ? gain : 0.0;
  }
}

// single-workgroup bitonic sort of (return, index) pairs in global memory (n2 = pow2 >= n)
__global__ __launch_bounds__(1024) void sort_kernel(const double* __restrict__ ret, int n, int n2, RetIdx* buf) {
  for (int i = threadIdx.x; i < n2; i += blockDim.x) buf[i] = i < n ? RetIdx{ret[i], i} : RetIdx{NAN, 0x7fffffff};
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & k) == 0;
          RetIdx a = buf[i], b = buf[l];
          if (less_ri(b, a) == up) { buf[i] = b; buf[l] = a; }
        }
      }
      __threadfence_block();
      __syncthreads();
    }
}

// gather one candidate out of the [t][field][candidate] SoA into a packed row-major staging
// buffer: [states H*DS | actions H*NU | times H | residual H*NR | costs H | trace H*3*NTR]
template <typename T>
__global__ void gather_traj_kernel(const T* states, const T* actions, const T* times, const T* residual,
                                   const T* costs, const T* trace, int N, int H, int ds, int nu, int nr, int ntr3,
                                   int cand, double* out, int candidate_major) {
  const int row = ds + nu + 1 + nr + 1 + ntr3;
  const int total = H * row;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    // i indexes the packed output
    int o = i;
    const T* src; int width;
    if (o < H * ds) { src = states; width = ds; }
    else if ((o -= H * ds) < H * nu) { src = actions; width = nu; }
    else if ((o -= H * nu) < H) { src = times; width = 1; }
    else if ((o -= H) < H * nr) { src = residual; width = nr; }
    else if ((o -= H * nr) < H) { src = costs; width = 1; }
    else { o -= H; src = trace; width = ntr3; }
    // o = t*width + k -> [(t*width+k)*N + cand] (lane-per-candidate kernels: a wavefront stores 64 consecutive candidates),
    // or [(cand*H + t)*width + k] (wavefront-per-candidate kernels: a wavefront stores one candidate's row)
    out[i] = (double)(candidate_major ? src[(size_t)cand * H * width + o] : src[(size_t)o * N + cand]);
  }
}
template <typename T>
__global__ void gather_spline_kernel(const T* nodes, int N, int np, int cand, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) out[i] = (double)nodes[(size_t)i * N + cand];
}
template <typename T>
__global__ void scatter_nodes_kernel(const double* __restrict__ in, T* nodes, int N, int np) {
  // in: candidate-major [N][np] (the reference's per-candidate TimeSpline values) -> [np][N]
  const size_t total = (size_t)N * np;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t j = i / N, c = i % N;
    nodes[i] = (T)in[c * np + j];
  }
}

}  // namespace

// ===================================================================== context
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
// Grow-only pinned host block that asynchronous copies read from (or write to). A call that ends in a stream sync may simply rewrite it;
// a call that does not mark()s the block after enqueueing its last reader, and whoever rewrites the block wait()s first.
struct PinnedBlock {
  void* p = nullptr;
  size_t cap = 0;
  hipEvent_t last = nullptr;  // the last reader, while `pending`
  bool pending = false;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  hipError_t wait() {
    if (!pending) return hipSuccess;
    pending = false;
    return hipEventSynchronize(last);
  }
  hipError_t mark(hipStream_t s) {
    hipError_t e = last ? hipSuccess : hipEventCreateWithFlags(&last, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(last, s);
    pending = e == hipSuccess;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    if (last) (void)hipEventDestroy(last);
    p = nullptr; cap = 0; last = nullptr; pending = false;
  }
};
// Grow-only pinned host block that kernels write through its device mapping (`dev`): the result records of the selection entry points,
// each of which ends in a stream sync before it reads `p`.
struct MappedBlock {
  void* p = nullptr; void* dev = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, p, 0);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() { if (p) (void)hipHostFree(p); p = dev = nullptr; cap = 0; }
};

struct mjpcx_ctx {
  int device = 0, precision = 64;
  const KernelEntry* kernel = nullptr;
  hipStream_t stream = nullptr;
  std::string last_error;
  // model/task dims
  int nq = 0, nv = 0, nu = 0, na = 0, nmocap = 0, nr = 0, nterm = 0, ntrace = 0, nparam = 0;
  std::vector<int> num_norm_parameter, dim_norm_residual;
  std::vector<int> ctrllimited;
  std::vector<double> ctrlrange;
  // host mirrors of the device structs (both precisions kept; only one uploaded)
  LaneModel<double> hm64{}; LaneModel<float> hm32{};
  LaneTask<double> ht64{}; LaneTask<float> ht32{};
  const void* cur_times = nullptr; const void* cur_nominal = nullptr;  // device views of the last plan inputs
  // plan inputs (node times, nominal spline, CE variances) go through a small ring of pinned
  // staging slots: one truly asynchronous H2D copy per rollout, no host sync
  static constexpr int kSlots = 4;
  struct Slot { PinnedBlock host; DevBuf dev; };  // host is marked behind the kernel that reads dev
  Slot slots[kSlots];
  int next_slot = 0;
  MappedBlock result;  // the result record(s) of mjpcx_best and of the batched selection entry points
  hipEvent_t source_done = nullptr;  // mjpcx_robust_step_batched, mjpcx_ilqg_step_batched_from: orders this stream behind the source context's
  // the Sample-Gradient planner's state between plan steps (mjpcx_rollout_sample_gradient_batched / mjpcx_sample_gradient_update_batched)
  struct SampleGradient {
    PinnedBlock h_in, h_up;       // pinned sides of d_in (marked: the rollout call does not sync) and d_up (the update ends in a sync)
    DevBuf d_in;                  // the rollout's [node_times E x P | nominal E x np | ctrlrange 2 nu | uploaded gradient times E x P, values E x G x np]
    DevBuf d_state;               // [gradient E x np | gradient_previous E x np | gradient candidates' times E x P | values E x G x np]
    DevBuf d_weights;             // the cached shaping weights, E x num_noisy
    DevBuf d_up;                  // [log(k + 1), k < n | LogScale step sizes G]
    int E = 0, G = -1, P = 0;     // shape of d_state
    int n = 0;                    // of the last rollout
    bool candidates = false;      // d_state holds the gradient candidates an update of this shape left
    int weights_E = 0, weights_n = 0;  // shape the cached weights were computed for (0: none)
    unsigned long long serial = 0;     // rollout_serial of the last Sample-Gradient rollout
    uint64_t seed = 0; uint32_t iteration = 0;
    int logs_n = 0, steps_G = -1; double steps_max = 0, steps_min = 0;  // what d_up holds
    void release() { h_in.release(); h_up.release(); d_in.release(); d_state.release(); d_weights.release(); d_up.release(); }
  } sg;
  // CMA-ES (mjpcx_cma_set_state_batched, mjpcx_rollout_cma_batched, mjpcx_cma_update_batched; csrc/cma_update.h)
  struct Cma {
    DevBuf d_state;               // E x cma_state_stride(d): [sigma | - | p_sigma | p_c | C | A]
    DevBuf d_in;                  // the rollout's [nominal E x d | ctrlrange 2 nu], read again by the update
    PinnedBlock h_in;             // its pinned side (marked: the rollout call does not sync)
    DevBuf d_y, d_s, d_zw, d_rank, d_w;  // the update's Y E x d x mu, S E x d x d, z_w E x d, [valid | order] E x (1 + mu), weights mu
    std::vector<double> weights;  // what d_w holds
    std::vector<long long> generation;  // E: updates applied since the state was set
    int E = 0, d = 0;             // shape of d_state (0: no state)
    int n = 0;                    // of the last CMA rollout
    unsigned long long serial = 0;      // rollout_serial of the last CMA rollout
    uint64_t seed = 0; uint32_t iteration = 0;
    void release() { d_state.release(); d_in.release(); h_in.release(); d_y.release(); d_s.release(); d_zw.release(); d_rank.release(); d_w.release(); }
  } cma;
  unsigned long long rollout_serial = 0;  // counts the rollouts of every kind
  // rollout buffers
  DevBuf d_nodes, d_in_nodes, d_ilqg, d_ilqg_out;
  PinnedBlock h_ilqg;  // host side of d_ilqg: the input arrays of the iLQG / Gradient entry points (upload_arrays; one H2D copy, marked: the feedback rollouts do not sync)
  DevBuf d_grad;       // workspace of mjpcx_gradient_step_batched / mjpcx_ilqg_step_batched: inputs, every intermediate, the result block
  PinnedBlock h_grad;  // its pinned [inputs | result block] (those calls end in a sync)
  DevBuf d_states, d_actions, d_times, d_residual, d_costs, d_trace, d_ret, d_fail, d_sort, d_stage;
  DevBuf d_mppi;  // mjpcx_mppi_update_batched: every environment's [weight sum | weights] between its two kernels (mppi_update.h)
  bool traj_candidate_major = false;  // layout of the last rollout's Trajectory buffers (true: wavefront-per-candidate kernels)
  int nsite_model = 0;
  int N = 0, H = 0, P = 0;  // shape of the last rollout
  // several environments (mjpcx_set_states): E x [state | time | mocap] and, when given, E x the frozen residual state
  int env_E = 0;
  std::vector<double> env_state, env_time, env_mocap, env_rreal;
  std::vector<int32_t> env_rint;
  // and, when given, E x the task parameters (mjpcx_set_task_params_batched; an empty vector: that field is the context's for every environment).
  // Only the batched entry points read them; mjpcx_set_task_params neither reads nor clears them.
  std::vector<double> env_weight, env_normp, env_normq, env_param, env_risk;  // E x nterm (three), E x nparam, E
  int env_n = 0;  // candidates per environment of the last rollout (0: not a batched one)
  // and, when given, a model per environment (mjpcx_set_models_batched): E records of every image the context holds for its own model, back
  // to back on the device. Only the batched rollouts read them. own_model / own_task: deep copies of what mjpcx_create was given (the
  // builders run on them again, once per environment's model; every model is compared with own_model field by field).
  struct OwnedModel {
    mjpcx_model m{};
    mjpcx_task t{};
    int given_integrator = 0;  // (before mjpcx_create's implicitfast -> Euler rewrite)
    std::vector<std::vector<unsigned char>> store;
  } own;
  struct EnvModels {
    int E = 0;
    DevBuf cold, image, qmodel, qtab, limb;  // WaveModel allocations | LdsLayout images | QuadModel | QuadTables | LimbModelT, E of each
    unsigned cold_stride = 0, image_stride = 0, qmodel_stride = 0, qtab_stride = 0, limb_stride = 0;
    std::vector<double> meaninertia;  // E (the generic kernel's by-value copy, per launch)
    void release() { cold.release(); image.release(); qmodel.release(); qtab.release(); limb.release(); E = 0; }
  } em;
  bool have_rollout = false;
  // wavefront-per-candidate family
  bool wave = false;
  WaveHost wh;
  std::vector<double> h_stage;
  // tuning aids read from the environment ONCE, in mjpcx_create: MJPCX_STAMPS=<step> (phase cycle stamps of candidate 0)
  int stamp_step = -1;
  bool no_tree = false;  // MJPCX_NO_TREE=1: keep the row-table constraint path (A/B runs)
  bool no_lds_model = false;  // MJPCX_NO_LDS_MODEL=1: generic kernel even for a registered model (A/B runs)
  int max_waves = 8;          // MJPCX_TREE_WAVES=<1..8, fp32: 1..12>: wavefronts per workgroup of the registered-model kernel (fp32 default 12: wave32.hip)
  int tree_mode = 16;         // tree_kernel.h mode bits: 16 dynamic candidate hand-out (default), 8 arena poison, 2 image self-check (MJPCX_TREE_MODE)
  bool no_second_pass = false;  // MJPCX_TREE_ONE_PASS=1: leave list overflows as failures (tuning: counts them)
  // multi-GPU (mjpcx_comm_*): the RCCL communicator of this context's rank and its staging buffers
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  DevBuf d_comm_send, d_comm_recv;
  std::vector<double> h_comm;
  DevBuf d_work;              // its self-check counter
  DevBuf d_ovf;               // its global slabs for cones beyond the LDS list
  bool no_cone_slabs = false; // MJPCX_TREE_NO_SLABS=1: overflow goes to the second pass instead (A/B runs)
  int num_cu = 256;
  // quad kernel (quad_kernel.h): four lanes per candidate; fp64 contexts of a model quad_build accepts
  bool quad_ok = false;       // MJPCX_NO_QUAD=1 keeps the wavefront-per-candidate kernels (A/B runs)
  bool quad_stamps = false;   // MJPCX_QUAD_STAMPS=1: phase cycle stamps of wavefront 0 (tuning aid; synchronises every rollout)
  int quad_min_n = 2048;          // batches below this go to rollout_tree_kernel<A1> (MJPCX_QUAD_MIN_N). 2048 = a rank's share of configs[2]'s 16384 candidates over 8 GPUs: there the
                                  // two kernels are level (gait steps, same box: 39.7 ms here at 4 candidates per wavefront, 37.8 there), and a sharded run then executes the
                                  // SAME kernel as one rank -- equal results bit for bit, not to a tolerance
  int quad_cpw = 0;               // candidates per wavefront of the quad kernel (0: chosen from the batch size; MJPCX_QUAD_CPW)
  int quad_con_cap = 0;           // MJPCX_QUAD_CON_CAP=<n>: hand on candidates with more than n contacts in a lane (tests of the hand-on path)
  bool quad_no_fallback = false;  // MJPCX_QUAD_NO_FALLBACK=1: leave the handed-on candidates flagged (tuning: failure[] then carries reason and step)
  bool no_quad_feedback = false;  // MJPCX_NO_QUAD_FEEDBACK=1: the iLQG rollouts stay on the wavefront-per-candidate kernel (A/B runs, tests)
  bool quad_stats = false;    // MJPCX_QUAD_STATS=1: print how many candidates each rollout handed to the fallback kernel, by reason
  std::string quad_why;       // why quad_build declined (mjpcx_create_error after MJPCX_OK carries it when MJPCX_QUAD_STATS is set)
  // limb kernel (limb_kernel.h): four lanes per candidate, one per limb of the Humanoid class limb_build accepts; both precisions
  bool limb_ok = false;       // MJPCX_NO_LIMB=1 keeps the wavefront-per-candidate kernel (A/B runs)
  int limb_min_n = 2560;      // batches below this go to rollout_tree_kernel<Humanoid> (MJPCX_LIMB_MIN_N). The limb kernel's launch is one wavefront's latency, ~20 ms for
                              // any batch up to 8192; the tree kernel takes 13.2 / 13.9 / 15.5 ms at 512 / 1024 / 2048 candidates and 27.1 at 3072 (limb: 18.9), fp32 on MI355X
  int limb_cpw = 0;           // candidates per wavefront (0: chosen from the batch size; MJPCX_LIMB_CPW)
  bool limb_no_fallback = false;  // MJPCX_LIMB_NO_FALLBACK=1: leave the handed-on candidates flagged (tuning)
  std::string limb_why;       // why limb_build declined
  int limb_ids[32];           // residual_int[2..33] the limb model was built for (tracking sites, mocap bodies)
  DevBuf d_limb;              // the model image in the context's precision
  int quad_ids[7] = {0, 0, 0, 0, 0, 0, 0};  // residual_int[1..7] the quad model was built for (torso, head site, goal mocap, feet)
  DevBuf d_qmodel, d_qtab, d_qstats, d_qstamps, d_qwave, d_qovf, d_qclass;
  void* h_qstats = nullptr;       // pinned copy of d_qstats (whether the hand-on pass has anything to do)
  // retiring candidates that can no longer be the argmin (mjpcx_set_pruning; quad kernel, one environment). d_qstats is 64 bytes: the 8
  // hand-on counters, then the bound word (byte 32) and the 4 pruning counters (byte 40) of QArgs::prune_bound / prune_stats
  bool prune_allowed = true;      // MJPCX_PRUNE=0 at creation: mjpcx_set_pruning does nothing
  bool prune_on = false;
  double prune_initial = 0;
  bool last_pruned = false;       // the last rollout was launched with a bound: its returns hold lower bounds, only the argmin is exact
  int prune_h[4] = {0, 0, 0, 0};  // ... and its counters, read back with the hand-on count
  double prune_final = 0;         // ... and the bound word after the launch: min(initial bound, the returns completed inside the launch)
  // rank mode (mjpcx_set_prune_rank): the bound of a pruned launch is the K-th smallest completed return (rank_bound.h), not the least
  int prune_rank = 1;             // K; 1: the bound of the argmin, as ever
  int last_prune_rank = 1;        // the K the last pruned rollout was launched with: its first K stored returns are exact (1: only the argmin)
  // parking on an unproven estimate of the launch's best return (mjpcx_set_park_hint; pruned launches only): the candidates the estimate
  // condemns are set aside with their state, settled against the final bound (park_settle.h) and, if not retired, resumed in a second launch
  bool park_allowed = true;       // MJPCX_PARK=0 at creation: mjpcx_set_park_hint does nothing
  double park_hint = HUGE_VAL;    // +inf: off
  DevBuf d_park_rec, d_resume;    // QArgs::park_records, the resume list
  int64_t park_h[3] = {0, 0, 0};  // the last rollout's: candidates parked, retired by the settling pass, resumed
  double park_resume_ms = 0;      // ... and its resume launch's event time
  hipEvent_t park_ev[2] = {nullptr, nullptr};
  // a bound, a hint and a set of counters per environment (mjpcx_set_pruning_batched; mjpcx_rollout_noise_batched on the quad kernel). The
  // environments' records (quad_abi.h, kQEnvRec*) follow the 64 bytes above in d_qstats and come back with them in one copy
  bool bprune_on = false;         // the switch, for launches of bprune_E environments
  int bprune_E = 0;
  std::vector<double> bprune_initial, bprune_hint;  // E each
  bool bprune_req = false;        // do_rollout: the rollout under way is mjpcx_rollout_noise_batched's (the one batched launch the switch applies to)
  bool last_pruned_batched = false;  // the last rollout was such a launch (last_pruned is set too: prune_h and park_h hold the sums over the environments)
  std::vector<int64_t> env_prune_h, env_park_h;  // E x 4, E x 3: the last rollout's counters per environment
  std::vector<double> env_prune_final;            // E: its final bounds
  PinnedBlock h_envrec;           // [the readback: 64 bytes + E records | the E records as uploaded]
  DevBuf d_resume_groups;         // the resume launch's workgroup table (resume_table.h)
  std::vector<quad::ResumeGroup> resume_groups;
  std::vector<int> resume_count;
  // timing
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<hipEvent_t> events_main;  // recorded right after the rollout's FIRST (dominant) kernel: events[i].first .. events_main[i] is that kernel alone
  hipEvent_t cur_main = nullptr;
  size_t events_used = 0;
};

namespace {
int fail(mjpcx_ctx* c, int code, const std::string& msg) {
  if (c) c->last_error = msg;
  return code;
}
#define HIPCHK(c, expr)                                                                      \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess)                                                                   \
      return fail(c, e__ == hipErrorOutOfMemory ? MJPCX_ENOMEM : MJPCX_EDEVICE,              \
                  std::string(#expr) + ": " + hipGetErrorString(e__));                       \
  } while (0)

size_t esize(const mjpcx_ctx* c) { return c->precision == 64 ? 8 : 4; }

// Every array of mjpcx_model with its length: X(I | D, name, count, may_differ). may_differ: a field the models of a fleet may differ in
// (mjpcx_set_models_batched, include/mjpcx.h) -- the inertial, passive, actuation and contact parameters and what mj_setConst derives from them.
#define MJPCX_MODEL_ARRAYS(X)                                                                                                              \
  X(I, body_parentid, m->nbody, 0) X(I, body_rootid, m->nbody, 0) X(I, body_jntnum, m->nbody, 0) X(I, body_jntadr, m->nbody, 0)           \
  X(I, body_dofnum, m->nbody, 0) X(I, body_dofadr, m->nbody, 0) X(I, body_mocapid, m->nbody, 0) X(D, body_pos, 3 * m->nbody, 0)           \
  X(D, body_quat, 4 * m->nbody, 0) X(D, body_ipos, 3 * m->nbody, 1) X(D, body_iquat, 4 * m->nbody, 0) X(D, body_mass, m->nbody, 1)        \
  X(D, body_inertia, 3 * m->nbody, 1) X(I, jnt_type, m->njnt, 0) X(I, jnt_qposadr, m->njnt, 0) X(I, jnt_dofadr, m->njnt, 0)               \
  X(I, jnt_bodyid, m->njnt, 0) X(I, jnt_limited, m->njnt, 0) X(D, jnt_pos, 3 * m->njnt, 0) X(D, jnt_axis, 3 * m->njnt, 0)                 \
  X(D, jnt_stiffness, m->njnt, 1) X(D, jnt_range, 2 * m->njnt, 0) X(D, jnt_margin, m->njnt, 0) X(D, jnt_solref, 2 * m->njnt, 0)           \
  X(D, jnt_solimp, 5 * m->njnt, 0) X(I, dof_bodyid, m->nv, 0) X(I, dof_jntid, m->nv, 0) X(I, dof_parentid, m->nv, 0)                      \
  X(D, dof_armature, m->nv, 1) X(D, dof_damping, m->nv, 1) X(D, dof_frictionloss, m->nv, 1) X(D, dof_invweight0, m->nv, 1)                \
  X(D, qpos0, m->nq, 0) X(D, qpos_spring, m->nq, 0) X(I, site_bodyid, m->nsite, 0) X(D, site_pos, 3 * m->nsite, 0)                        \
  X(D, site_quat, 4 * m->nsite, 0) X(I, actuator_trnid, m->nu, 0) X(I, actuator_gaintype, m->nu, 0) X(I, actuator_biastype, m->nu, 0)     \
  X(I, actuator_ctrllimited, m->nu, 0) X(I, actuator_forcelimited, m->nu, 0) X(D, actuator_gear, m->nu, 1)                                \
  X(D, actuator_gainprm, 3 * m->nu, 1) X(D, actuator_biasprm, 3 * m->nu, 1) X(D, actuator_ctrlrange, 2 * m->nu, 0)                        \
  X(D, actuator_forcerange, 2 * m->nu, 0) X(I, geom_type, m->ngeom, 0) X(I, geom_bodyid, m->ngeom, 0) X(I, geom_contype, m->ngeom, 0)     \
  X(I, geom_conaffinity, m->ngeom, 0) X(I, geom_condim, m->ngeom, 0) X(I, geom_priority, m->ngeom, 0) X(I, geom_group, m->ngeom, 0)       \
  X(D, geom_size, 3 * m->ngeom, 0) X(D, geom_pos, 3 * m->ngeom, 0) X(D, geom_quat, 4 * m->ngeom, 0) X(D, geom_friction, 3 * m->ngeom, 1)  \
  X(D, geom_solref, 2 * m->ngeom, 1) X(D, geom_solimp, 5 * m->ngeom, 1) X(D, geom_margin, m->ngeom, 0) X(D, geom_gap, m->ngeom, 0)        \
  X(D, geom_solmix, m->ngeom, 0) X(D, body_invweight0, 2 * m->nbody, 1) X(D, body_subtreemass, m->nbody, 1) X(D, dof_solref, 2 * m->nv, 0) \
  X(D, dof_solimp, 5 * m->nv, 0) X(D, key_qpos, (size_t)m->nkey * m->nq, 0) X(I, tendon_adr, m->ntendon, 0) X(I, tendon_num, m->ntendon, 0) \
  X(I, tendon_limited, m->ntendon, 0) X(I, wrap_objid, m->nwrap, 0) X(D, wrap_prm, m->nwrap, 0) X(D, tendon_range, 2 * m->ntendon, 0)     \
  X(D, tendon_margin, m->ntendon, 0) X(D, tendon_solref_lim, 2 * m->ntendon, 0) X(D, tendon_solimp_lim, 5 * m->ntendon, 0)                \
  X(D, tendon_invweight0, m->ntendon, 1) X(I, exclude_signature, m->nexclude, 0) X(I, body_weldid, m->nbody, 0)                           \
  X(D, key_mpos, (size_t)m->nkey * m->nmocap * 3, 0)
#define MJPCX_TASK_ARRAYS(X)                                                                                                          \
  X(I, dim_norm_residual, t->num_term) X(I, norm, t->num_term) X(I, num_norm_parameter, t->num_term) X(D, weight, t->num_term)        \
  X(D, parameters, t->num_parameter) X(I, trace_site, t->num_trace) X(I, residual_int, t->num_residual_int)                           \
  X(D, residual_real, t->num_residual_real)

// deep copies of a caller's model and task headers (a NULL array stays NULL)
template <typename E>
const E* own_array(mjpcx_ctx::OwnedModel& o, const E* p, size_t n) {
  if (!p) return nullptr;
  o.store.emplace_back(n * sizeof(E) + 8);
  if (n) std::memcpy(o.store.back().data(), p, n * sizeof(E));
  return reinterpret_cast<const E*>(o.store.back().data());
}
void own_copy(mjpcx_ctx::OwnedModel& o, const mjpcx_model* m, const mjpcx_task* t, int given_integrator) {
  o.store.clear();
  o.m = *m; o.t = *t; o.given_integrator = given_integrator;
#define X(kind, name, count, differ) o.m.name = own_array(o, m->name, (size_t)(count));
  MJPCX_MODEL_ARRAYS(X)
#undef X
#define X(kind, name, count) o.t.name = own_array(o, t->name, (size_t)(count));
  MJPCX_TASK_ARRAYS(X)
#undef X
  size_t nnorm = 0;
  for (int k = 0; k < t->num_term; k++) nnorm += t->num_norm_parameter[k];
  o.t.norm_parameter = own_array(o, t->norm_parameter, nnorm);
}

// "" if model `m` may serve an environment of a context created on `ref` (include/mjpcx.h, mjpcx_set_models_batched): every size, option,
// integer array and real array equal, except the fields a fleet's models may differ in -- and those with the zeros and the signs where ref has them
std::string compare_env_model(const mjpcx_model* ref, const mjpcx_model* m, int given_integrator) {
#define S(name) if (ref->name != m->name) return std::string(#name) + " differs from the context's model";
  S(nq) S(nv) S(nu) S(na) S(nbody) S(njnt) S(nsite) S(nmocap) S(nuserdata) S(timestep) S(gravity[0]) S(gravity[1]) S(gravity[2])
  S(disableflags) S(solver_iterations) S(solver_tolerance) S(ngeom) S(nkey) S(cone) S(impratio) S(ntendon) S(nwrap) S(nexclude)
#undef S
  if (m->integrator != given_integrator) return "integrator differs from the context's model";
  if (!(m->meaninertia > 0) != !(ref->meaninertia > 0)) return "meaninertia changes sign or zero pattern";
  auto same = [](const void* a, const void* b, size_t bytes) { return (!a && !b) || (a && b && std::memcmp(a, b, bytes) == 0); };
  auto pattern = [](const double* a, const double* b, size_t n) {
    if (!a || !b) return !a && !b;
    for (size_t i = 0; i < n; i++) {
      if (!(b[i] == b[i])) return false;
      if ((a[i] == 0) != (b[i] == 0) || (a[i] > 0) != (b[i] > 0)) return false;
    }
    return true;
  };
  static const char* const shared = " differs from the context's model (only the inertial, passive, actuation and contact parameters may)";
  // (the sizes are equal by now: the counts, written in terms of m, hold for both)
#define CMP_FIELD_I(name, n, differ) if (!same(ref->name, m->name, sizeof(int32_t) * (n))) return std::string(#name) + shared;
#define CMP_FIELD_D(name, n, differ)                                                                                                \
  if (differ) { if (!pattern(ref->name, m->name, (n))) return std::string(#name) + " changes which entries are zero, or their sign"; } \
  else if (!same(ref->name, m->name, sizeof(double) * (n))) return std::string(#name) + shared;
#define X(kind, name, count, differ) CMP_FIELD_##kind(name, (size_t)(count), differ)
  MJPCX_MODEL_ARRAYS(X)
#undef X
#undef CMP_FIELD_I
#undef CMP_FIELD_D
  return "";
}

template <typename T>
void fill_model(LaneModel<T>& d, const mjpcx_model* m) {
  std::memset(&d, 0, sizeof d);
  d.timestep = (T)m->timestep;
  for (int k = 0; k < 3; k++) d.gravity[k] = (T)m->gravity[k];
  d.solver_tolerance = (T)m->solver_tolerance;
  d.meaninertia = (T)m->meaninertia;
  d.disableflags = m->disableflags;
  d.solver_iterations = m->solver_iterations;
  std::vector<double> sub(m->nbody);
  for (int b = 0; b < m->nbody; b++) sub[b] = m->body_mass[b];
  for (int b = m->nbody - 1; b > 0; b--) sub[m->body_parentid[b]] += sub[b];
  for (int b = 0; b < m->nbody; b++) {
    for (int k = 0; k < 3; k++) {
      d.body_pos[b][k] = (T)m->body_pos[3 * b + k];
      d.body_ipos[b][k] = (T)m->body_ipos[3 * b + k];
      d.body_inertia[b][k] = (T)m->body_inertia[3 * b + k];
    }
    for (int k = 0; k < 4; k++) {
      d.body_quat[b][k] = (T)m->body_quat[4 * b + k];
      d.body_iquat[b][k] = (T)m->body_iquat[4 * b + k];
    }
    d.body_mass[b] = (T)m->body_mass[b];
    d.root_invmass[b] = (T)(sub[b] > kMinVal ? 1.0 / sub[b] : 0.0);
  }
  d.any_damping = 0;
  d.integrator = m->integrator;
  for (int j = 0; j < m->njnt; j++) {
    for (int k = 0; k < 3; k++) { d.jnt_pos[j][k] = (T)m->jnt_pos[3 * j + k]; d.jnt_axis[j][k] = (T)m->jnt_axis[3 * j + k]; }
    d.jnt_stiffness[j] = (T)m->jnt_stiffness[j];
    d.jnt_range[j][0] = (T)m->jnt_range[2 * j]; d.jnt_range[j][1] = (T)m->jnt_range[2 * j + 1];
    d.jnt_margin[j] = (T)m->jnt_margin[j];
    d.jnt_solref[j][0] = (T)m->jnt_solref[2 * j]; d.jnt_solref[j][1] = (T)m->jnt_solref[2 * j + 1];
    for (int k = 0; k < 5; k++) d.jnt_solimp[j][k] = (T)m->jnt_solimp[5 * j + k];
    d.qpos0[j] = (T)m->qpos0[j]; d.qpos_spring[j] = (T)m->qpos_spring[j];
    d.dof_armature[j] = (T)m->dof_armature[j]; d.dof_damping[j] = (T)m->dof_damping[j];
    d.dof_invweight0[j] = (T)m->dof_invweight0[j];
    if (m->dof_damping[j] > 0) d.any_damping = 1;
  }
  for (int s = 0; s < m->nsite; s++)
    for (int k = 0; k < 3; k++) d.site_pos[s][k] = (T)m->site_pos[3 * s + k];
  for (int u = 0; u < m->nu; u++) {
    d.act_gear[u] = (T)m->actuator_gear[u];
    d.act_gain[u] = (T)m->actuator_gainprm[3 * u];
    for (int k = 0; k < 3; k++) d.act_bias[u][k] = (T)m->actuator_biasprm[3 * u + k];
    for (int k = 0; k < 2; k++) {
      d.act_ctrlrange[u][k] = (T)m->actuator_ctrlrange[2 * u + k];
      d.act_forcerange[u][k] = (T)m->actuator_forcerange[2 * u + k];
    }
    d.act_biastype[u] = m->actuator_biastype[u];
    d.act_ctrllimited[u] = m->actuator_ctrllimited[u];
    d.act_forcelimited[u] = m->actuator_forcelimited[u];
  }
}

bool same_model(const LaneModel<double>& a, const LaneModel<double>& b) {
  // both objects are fully zero-initialised before being filled, so a byte comparison of the
  // value representation is exact equality of every constant (the structs have no padding holes
  // between doubles; the two int members before arrays of doubles are compared as stored)
  return std::memcmp(&a, &b, sizeof a) == 0;
}

template <typename TD, typename TS>
void convert_task(LaneTask<TD>& d, const LaneTask<TS>& s) {
  for (int k = 0; k < kLaneMaxTerm; k++) {
    d.norm[k] = s.norm[k]; d.weight[k] = (TD)s.weight[k]; d.norm_p[k] = (TD)s.norm_p[k]; d.norm_q[k] = (TD)s.norm_q[k];
  }
  for (int k = 0; k < kLaneMaxParam; k++) d.parameters[k] = (TD)s.parameters[k];
  d.risk = (TD)s.risk;
  for (int k = 0; k < kLaneMaxDof; k++) { d.qpos[k] = (TD)s.qpos[k]; d.qvel[k] = (TD)s.qvel[k]; }
  d.time = (TD)s.time;
  for (int i = 0; i < kLaneMaxMocap; i++) {
    for (int k = 0; k < 3; k++) d.mocap_pos[i][k] = (TD)s.mocap_pos[i][k];
    for (int k = 0; k < 4; k++) d.mocap_quat[i][k] = (TD)s.mocap_quat[i][k];
  }
}

void set_norm_params(mjpcx_ctx* c, const double* norm_parameter) {
  int shift = 0;
  for (int k = 0; k < c->nterm; k++) {
    const int np = c->num_norm_parameter[k];
    const double p = np > 0 ? norm_parameter[shift] : 0.0, q = np > 1 ? norm_parameter[shift + 1] : 0.0;
    if (c->wave) { c->wh.norm_p[k] = p; c->wh.norm_q[k] = q; }
    else { c->ht64.norm_p[k] = p; c->ht64.norm_q[k] = q; }
    shift += np;
  }
}
void clear_env_task_params(mjpcx_ctx* c) {
  c->env_weight.clear(); c->env_normp.clear(); c->env_normq.clear(); c->env_param.clear(); c->env_risk.clear();
}
bool has_env_task_params(const mjpcx_ctx* c) {
  return !(c->env_weight.empty() && c->env_normp.empty() && c->env_normq.empty() && c->env_param.empty() && c->env_risk.empty());
}
}  // namespace

namespace {
int reserve_rollout(mjpcx_ctx* c, int N, int H, int P) {
  const size_t w = esize(c);
  const size_t ds = c->nq + c->nv + c->na;
  HIPCHK(c, c->d_nodes.reserve((size_t)N * P * c->nu * w));
  HIPCHK(c, c->d_states.reserve((size_t)N * H * ds * w));
  HIPCHK(c, c->d_actions.reserve((size_t)N * H * c->nu * w));
  HIPCHK(c, c->d_times.reserve((size_t)N * H * w));
  HIPCHK(c, c->d_residual.reserve((size_t)N * H * c->nr * w));
  HIPCHK(c, c->d_costs.reserve((size_t)N * H * w));
  HIPCHK(c, c->d_trace.reserve((size_t)N * H * 3 * std::max(c->ntrace, 1) * w));
  HIPCHK(c, c->d_ret.reserve((size_t)N * 8));
  HIPCHK(c, c->d_fail.reserve((size_t)N * 4));
  return MJPCX_OK;
}

// Stage E records [node_times (T) | nominal (T) | variance (f64) | blob] into the next pinned slot, `*stride` bytes apart, and enqueue ONE
// asynchronous H2D copy. The slot is recycled only after the kernel that reads it has finished. The blob is the per-plan blob of the
// wavefront-per-candidate family (wave_model.h) or the lane family's initial condition (LaneInit). E = 0: the plain call -- one record
// from the state of mjpcx_set_state; E >= 1: node_times is E x P, nominal E x P*nu, the states are those of mjpcx_set_states.
// variance: one row of P*nu copied into every record, or (variance_rows) E rows, row e into record e.
template <typename T>
int stage_plan_inputs(mjpcx_ctx* c, int P, int E, const double* node_times, const double* nominal, const double* variance, bool variance_rows,
                      const T** d_times, const T** d_nominal, const double** d_variance, mjpcx_ctx::Slot** used,
                      const void** d_blob, unsigned* stride) {
  const int np = P * c->nu, nrec = E > 0 ? E : 1;
  const size_t off_nom = ((size_t)P * sizeof(T) + 15) & ~(size_t)15;
  const size_t off_var = (off_nom + (size_t)np * sizeof(T) + 15) & ~(size_t)15;
  const size_t off_blob = (off_var + (size_t)np * 8 + 15) & ~(size_t)15;
  const size_t rec = (off_blob + (c->wave ? (sizeof(T) == 4 ? c->wh.blob_bytes32 : c->wh.blob_bytes) : sizeof(LaneInit<T>)) + 15) & ~(size_t)15;
  const size_t bytes = rec * nrec;
  mjpcx_ctx::Slot& s = c->slots[c->next_slot];
  c->next_slot = (c->next_slot + 1) % mjpcx_ctx::kSlots;
  HIPCHK(c, s.host.wait());
  HIPCHK(c, s.host.reserve(bytes));
  HIPCHK(c, s.dev.reserve(bytes));
  const int nst = c->nq + c->nv;
  for (int e = 0; e < nrec; e++) {
    char* h = (char*)s.host.p + rec * e;
    T* ht = (T*)h;
    for (int p = 0; p < P; p++) ht[p] = (T)node_times[(size_t)e * P + p];
    T* hn = (T*)(h + off_nom);
    if (nominal) for (int j = 0; j < np; j++) hn[j] = (T)nominal[(size_t)e * np + j];
    if (variance) std::memcpy(h + off_var, variance + (variance_rows ? (size_t)e * np : 0), (size_t)np * 8);
    T* hb = (T*)(h + off_blob);
    const double* st = E > 0 ? c->env_state.data() + (size_t)e * nst : nullptr;
    const double* mo = E > 0 && !c->env_mocap.empty() ? c->env_mocap.data() + (size_t)e * 7 * c->nmocap : nullptr;
    if (c->wave) {
      if (sizeof(T) == 4) c->wh.fill_blob32(hb); else c->wh.fill_blob(hb);
      if (E > 0) {  // the environment's own state, clock, mocap pose and (if given) frozen residual state over the context's
        const WaveTask& t = c->wh.t;
        for (int i = 0; i < nst; i++) hb[i] = (T)st[i];
        hb[t.off_time] = (T)c->env_time[e];
        if (mo) for (int i = 0; i < 7 * c->nmocap; i++) hb[t.off_mocap + i] = (T)mo[i];
        if (!c->env_rreal.empty()) for (int i = 0; i < t.nrr; i++) hb[t.off_rreal + i] = (T)c->env_rreal[(size_t)e * t.nrr + i];
        if (!c->env_rint.empty()) std::memcpy(hb + t.off_rint, c->env_rint.data() + (size_t)e * t.nri, sizeof(int32_t) * t.nri);
        // and its own task parameters (mjpcx_set_task_params_batched), field by field, over the context's
        const size_t nt = c->nterm, npar = c->nparam;
        if (!c->env_weight.empty()) for (size_t i = 0; i < nt; i++) hb[t.off_weight + i] = (T)c->env_weight[e * nt + i];
        if (!c->env_normp.empty()) for (size_t i = 0; i < nt; i++) hb[t.off_normp + i] = (T)c->env_normp[e * nt + i];
        if (!c->env_normq.empty()) for (size_t i = 0; i < nt; i++) hb[t.off_normq + i] = (T)c->env_normq[e * nt + i];
        if (!c->env_param.empty()) for (size_t i = 0; i < npar; i++) hb[t.off_param + i] = (T)c->env_param[e * npar + i];
        if (!c->env_risk.empty()) hb[t.off_risk] = (T)c->env_risk[e];
      }
    } else {
      LaneInit<T>& li = *reinterpret_cast<LaneInit<T>*>(hb);
      const LaneTask<double>& k = c->ht64;
      for (int i = 0; i < kLaneMaxDof; i++) {
        li.qpos[i] = (T)(st && i < c->nq ? st[i] : k.qpos[i]);
        li.qvel[i] = (T)(st && i < c->nv ? st[c->nq + i] : k.qvel[i]);
      }
      li.time = (T)(E > 0 ? c->env_time[e] : k.time);
      for (int i = 0; i < kLaneMaxMocap; i++) {
        const bool own = mo && i < c->nmocap;
        for (int q = 0; q < 3; q++) li.mocap_pos[i][q] = (T)(own ? mo[7 * i + q] : k.mocap_pos[i][q]);
        for (int q = 0; q < 4; q++) li.mocap_quat[i][q] = (T)(own ? mo[7 * i + 3 + q] : k.mocap_quat[i][q]);
      }
      // the task parameters: the context's (the casts of convert_task), or with several environments the environment's own where given
      const size_t nt = c->nterm, npar = c->nparam;
      for (size_t i = 0; i < (size_t)kLaneMaxTerm; i++) {
        const bool own = E > 0 && i < nt;
        li.weight[i] = (T)(own && !c->env_weight.empty() ? c->env_weight[e * nt + i] : k.weight[i]);
        li.norm_p[i] = (T)(own && !c->env_normp.empty() ? c->env_normp[e * nt + i] : k.norm_p[i]);
        li.norm_q[i] = (T)(own && !c->env_normq.empty() ? c->env_normq[e * nt + i] : k.norm_q[i]);
      }
      for (size_t i = 0; i < (size_t)kLaneMaxParam; i++)
        li.parameters[i] = (T)(E > 0 && i < npar && !c->env_param.empty() ? c->env_param[e * npar + i] : k.parameters[i]);
      li.risk = (T)(E > 0 && !c->env_risk.empty() ? c->env_risk[e] : k.risk);
    }
  }
  HIPCHK(c, hipMemcpyAsync(s.dev.p, s.host.p, bytes, hipMemcpyHostToDevice, c->stream));
  *d_times = (const T*)s.dev.p;
  *d_nominal = (const T*)((char*)s.dev.p + off_nom);
  *d_variance = (const double*)((char*)s.dev.p + off_var);
  *d_blob = (const char*)s.dev.p + off_blob;
  *stride = (unsigned)rec;
  *used = &s;
  return MJPCX_OK;
}

// tuning aid (MJPCX_STAMPS=<step>): phase cycle stamps of candidate 0 at one step of the wavefront-per-candidate kernel
void print_wave_stamps(mjpcx_ctx* c, long long* stamps, int stamp_step, size_t lds, bool tree = false) {
  long long h[48];
  (void)hipStreamSynchronize(c->stream);
  (void)hipMemcpy(h, stamps, sizeof h, hipMemcpyDeviceToHost);
  static const char* nm[] = {"policy", "kinematics", "compos", "crb", "cholM", "collision", "comvel", "make_constraint", "smooth", "solve",
                             "newton", "residual", "cost+record", "euler"};
  static const char* nt[] = {"policy", "kinematics", "compos", "crb", "cholM", "comvel", "smooth", "solve", "collision", "make_constraint",
                             "newton", "residual", "cost+record", "euler"};
  std::fprintf(stderr, "wave kernel phase cycles (step %d, candidate 0; LDS %zu B):", stamp_step, lds);
  for (int k = 0; k < 14; k++) std::fprintf(stderr, " %s %lld", tree ? nt[k] : nm[k], h[k + 1] - h[k]);
  std::fprintf(stderr, " | newton iters %lld: grad %lld hess %lld chol+solve %lld linesearch %lld\n", h[20], h[21] - h[10], h[22] - h[21],
               h[23] - h[22], h[24] - h[23]);
  std::fprintf(stderr, "  newton totals over iterations: grad %lld coneblocks %lld hess %lld chol+solve %lld jv+q %lld linesearch %lld (%lld trials) update+cost %lld\n",
               h[32], h[33], h[34], h[35], h[36], h[37], h[39], h[38]);
  std::fprintf(stderr, "  hessian parts: copy M %lld diagonal rows %lld row facts %lld simple rows (MFMA) %lld cones = hess - these\n", h[40], h[41], h[42], h[43]);
}

// registered model (lds_model.h / tree_kernel.h): [image | blob | W arenas] of LDS per workgroup, W <= 8 wavefronts, persistent.
// Two launches: the batch with the small contact lists, then the candidates that overflowed them with the large lists.
template <class C, typename T, bool BIG>
hipError_t launch_tree_pass(mjpcx_ctx* c, const WaveModelT<T>& wm, const WaveTaskT<T>& wt, const RolloutArgs<T>& a, const void* image, size_t blob_bytes,
                            int N, int P, bool only_flagged = false) {
  const int caps = BIG ? (sizeof(T) == 8 ? w64::kTreeMaxSimpleBig : w32::kTreeMaxSimpleBig) : (sizeof(T) == 8 ? w64::kTreeMaxSimple : w32::kTreeMaxSimple);
  const int capc = BIG ? (sizeof(T) == 8 ? w64::kTreeMaxConeBig : w32::kTreeMaxConeBig) : (sizeof(T) == 8 ? w64::kTreeMaxCone : w32::kTreeMaxCone);
  const size_t arena = sizeof(T) == 8
      ? (8 * w64::wave_lds_elems_tree(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, wt.nr, wt.nterm, P, a.xfrc_scale > 0, caps, capc) + 15) & ~(size_t)15
      : (4 * w32::wave_lds_elems_tree(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, wt.nr, wt.nterm, P, a.xfrc_scale > 0, caps, capc) + 15) & ~(size_t)15;
  const size_t fixed = LdsLayout<C, T>::kBytes + blob_bytes;
  if (fixed + arena > 160 * 1024) return hipErrorInvalidValue;
  int W = (int)std::min<size_t>((size_t)c->max_waves, (160 * 1024 - fixed) / arena);
  W = std::max(1, std::min(W, (N + c->num_cu - 1) / c->num_cu));  // small batches: spread over the CUs first
  int grid = std::min(c->num_cu, (N + W - 1) / W);
  if (BIG) grid = std::min(grid, 64);  // the second pass scans the failure flags; a handful of rollouts at most
  // several environments: a workgroup holds ONE environment's blob, so the workgroups are dealt to the environments in equal shares
  // (tree_kernel.h) -- a chip's worth of them over all environments, one each at least
  const int E = a.env_n > 0 ? N / a.env_n : 1;
  if (E > 1) grid = E * std::max(1, std::min(grid / E, (a.env_n + W - 1) / W));
  const int mode = (BIG ? (c->tree_mode & 8) : c->tree_mode) | (only_flagged && !BIG ? 32 : 0);  // 32: only the candidates the quad kernel handed on
  const size_t lds = fixed + (size_t)W * arena;
  const size_t work_bytes = (8 + 4 * (size_t)E + 15) & ~(size_t)15;  // [-, self-check count, one work counter per environment]
  hipError_t e = c->d_work.reserve(work_bytes);
  if (e != hipSuccess) return e;
  if (mode & (2 | 16)) if ((e = hipMemsetAsync(c->d_work.p, 0, work_bytes, c->stream)) != hipSuccess) return e;  // self-check count / work counters
  // first pass: one slab per wavefront for the cones beyond the LDS list (wave_tree.h; a few tens of MB, never touched in the common case)
  void* slabs = nullptr;
  if (!BIG && !c->no_cone_slabs) {
    const size_t per_wave = (size_t)(w64::kTreeMaxConeTotal - capc) * w64::kConeRec * sizeof(T);
    if ((e = c->d_ovf.reserve((size_t)grid * W * per_wave)) != hipSuccess) return e;
    slabs = c->d_ovf.p;
  }
  if constexpr (sizeof(T) == 8) {
    auto kern = w64::rollout_tree_kernel<C, BIG>;
    if ((e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * W), lds, c->stream, wm, wt, a, (const unsigned char*)image, (unsigned)blob_bytes, (unsigned)arena,
                       (int*)c->d_work.p, mode, (T*)slabs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  } else {  // (the fp32 kernels live in wave32.hip)
    if ((e = launch_tree_kernel_f32(std::is_same<C, TreeCfgA1>::value ? 0 : 1, BIG, grid, 64 * W, lds, wm, wt, a, (const unsigned char*)image,
                                    (unsigned)blob_bytes, (unsigned)arena, (int*)c->d_work.p, mode, (float*)slabs, c->stream)) != hipSuccess) return e;
  }
  if (c->stamp_step >= 0) std::fprintf(stderr, "rollout_tree_kernel%s: %d wavefronts per workgroup, grid %d, LDS %zu B (arena %zu B)\n", BIG ? " (second pass)" : "", W, grid, lds, arena);
  if (mode & 2) {  // self-check launch: report the mismatch count
    int h[2] = {0, 0};
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h, c->d_work.p, 8, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "rollout_tree_kernel self-check: %d mismatching entries between the LDS image and the model (W = %d, grid = %d, lds = %zu B)\n", h[1], W, grid, lds);
  }
  return hipSuccess;
}
template <class C, typename T>
hipError_t launch_tree(mjpcx_ctx* c, const WaveModelT<T>& wm, const WaveTaskT<T>& wt, const RolloutArgs<T>& a, const void* image, size_t blob_bytes,
                       int N, int P, bool only_flagged = false) {
  hipError_t e = launch_tree_pass<C, T, false>(c, wm, wt, a, image, blob_bytes, N, P, only_flagged);
  // (mjpcx_timing_read_main: the first pass is the kernel that rolls the batch out; the pass over the quad kernel's hand-ons does not own the stamp)
  if (e == hipSuccess && !only_flagged && c->timing && c->cur_main) { if ((e = hipEventRecord(c->cur_main, c->stream)) == hipSuccess) c->cur_main = nullptr; }
  if (e != hipSuccess || (c->tree_mode & 2) || c->no_second_pass) return e;
  RolloutArgs<T> a2 = a;
  a2.noise.mode = -1;  // the first pass left every candidate's spline nodes in a.nodes
  WaveTaskT<T> wt2 = wt;
  wt2.stamps = nullptr;
  return launch_tree_pass<C, T, true>(c, wm, wt2, a2, image, blob_bytes, N, P);
}

// The model records a rollout launch reads: the context's own (strides of 0), or -- a batched rollout while mjpcx_set_models_batched's models
// are set -- environment 0's of the E records, with the bytes between consecutive environments'. do_rollout decides and hands it down to launch_wave.
struct ModelRecords {
  bool per_env;
  const void *qmodel, *qtab, *limb, *image;
  unsigned qmodel_stride, qtab_stride, limb_stride;
};
ModelRecords model_records(const mjpcx_ctx* c, bool per_env, bool f32) {
  if (per_env) return {true, c->em.qmodel.p, c->em.qtab.p, c->em.limb.p, c->em.image.p, c->em.qmodel_stride, c->em.qtab_stride, c->em.limb_stride};
  return {false, c->d_qmodel.p, c->d_qtab.p, c->d_limb.p, f32 ? c->wh.dev_image32 : c->wh.dev_image, 0u, 0u, 0u};
}

// quad kernel (quad_kernel.h), then the wavefront-per-candidate kernel for the candidates it handed on
// plain: mjpcx_rollout_noise / mjpcx_rollout_splines (E = 0), the launches mjpcx_set_pruning applies to
hipError_t launch_quad(mjpcx_ctx* c, const WaveModel& wm, const WaveTask& wt, const RolloutArgs<double>& a, int N, int P, const ModelRecords& mr, bool plain) {
  quad::QArgs q{};
  q.N = a.N; q.H = a.H; q.P = a.P; q.interp = a.interp; q.node_times = a.node_times; q.nodes = a.nodes; q.nominal = a.nominal;
  q.noise_mode = a.noise.mode; q.seed = a.noise.seed; q.iteration = a.noise.iteration; q.candidate_offset = a.noise.candidate_offset;
  q.nominal_candidate = a.noise.nominal_candidate; q.explore_count = a.noise.explore_count; q.std0 = a.noise.std0; q.std1 = a.noise.std1;
  q.param_variance = a.noise.param_variance;
  q.states = a.states; q.actions = a.actions; q.times = a.times; q.residual = a.residual; q.costs = a.costs; q.trace = a.trace;
  q.total_return = a.total_return; q.failure = a.failure; q.con_cap = c->quad_con_cap; q.cpw = c->quad_cpw;
  q.env_n = a.env_n; q.env_stride = a.env_stride; q.seed_shared = a.seed_shared;
  q.model_stride = mr.qmodel_stride; q.tables_stride = mr.qtab_stride;  // (a model per environment; 0: the one model)
  const quad::QBlob bo{wt.off_time, wt.off_mocap, wt.off_weight, wt.off_normp, wt.off_normq, wt.off_param, wt.off_risk, wt.off_rreal, wt.off_rint};
  hipError_t e;
  if (quad::quad_uses_ovf_slab()) {  // (a build with QEXP_OVF_SLAB: contacts beyond a lane's LDS slots in global memory, 150 KB per wavefront)
    if ((e = c->d_qovf.reserve((size_t)quad::quad_waves(N, c->quad_cpw) * quad::quad_ovf_doubles_per_wave() * sizeof(double))) != hipSuccess) return e;
    q.ovf_slab = (double*)c->d_qovf.p;
  }
  // (mjpcx_set_pruning: the plain launches only -- a batched one, of one environment too, needs a bound per environment and has a switch
  // of its own for that. Not with MJPCX_QUAD_NO_FALLBACK either: that tuning switch skips the readback the counters ride on)
  // (mjpcx_set_pruning_batched: mjpcx_rollout_noise_batched only, with a record per environment behind the 64 bytes of the plain launch)
  const bool bpruned = c->bprune_on && c->bprune_req && !plain && !c->quad_no_fallback && c->bprune_E > 0 && N % c->bprune_E == 0;
  const int bE = bpruned ? c->bprune_E : 0, bn = bpruned ? N / bE : 0;
  const size_t brec = (size_t)bE * quad::kQEnvRec;
  const bool pruned = (c->prune_on && plain && !c->quad_no_fallback) || bpruned;
  if (bpruned && (e = c->d_qstats.reserve(64 + brec)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(c->d_qstats.p, 0, pruned ? 64 : 32, c->stream)) != hipSuccess) return e;  // (how many candidates are handed on, by reason: mjpcx_quad_stats)
  bool bparking = false;
  if (bpruned) {
    // every environment's record starts at its own bound and hint, with its counters at zero: one copy on the stream. (The staged records
    // are the second half of the pinned block; the launch ends in a synchronisation, so the next one may rewrite them.)
    if ((e = c->h_envrec.reserve(64 + 2 * brec)) != hipSuccess) return e;
    char* up = (char*)c->h_envrec.p + 64 + brec;
    std::memset(up, 0, brec);
    for (int k = 0; k < bE; k++) {
      const double hint = c->park_allowed ? c->bprune_hint[k] : HUGE_VAL;
      bparking = bparking || hint < HUGE_VAL;
      std::memcpy(up + (size_t)k * quad::kQEnvRec + quad::kQEnvRecBound, &c->bprune_initial[k], 8);
      std::memcpy(up + (size_t)k * quad::kQEnvRec + quad::kQEnvRecHint, &hint, 8);
    }
    char* w = (char*)c->d_qstats.p + 64;
    if ((e = hipMemcpyAsync(w, up, brec, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return e;
    q.prune_bound = (unsigned long long*)(w + quad::kQEnvRecBound);
    q.prune_stats = (int*)(w + quad::kQEnvRecStats);
    q.rec_stride = quad::kQEnvRec;
    c->env_prune_h.assign((size_t)bE * 4, 0); c->env_park_h.assign((size_t)bE * 3, 0); c->env_prune_final.assign(bE, 0.0);
  } else if (pruned) {  // the bound word starts at the caller's bound (+inf: 0x7ff00000 over a low word of zeros), on the stream like the counters
    unsigned long long bits;
    std::memcpy(&bits, &c->prune_initial, 8);
    char* w = (char*)c->d_qstats.p + 32;
    if ((unsigned)bits != 0 && (e = hipMemsetD32Async((hipDeviceptr_t)w, (int)(unsigned)bits, 1, c->stream)) != hipSuccess) return e;
    if ((e = hipMemsetD32Async((hipDeviceptr_t)(w + 4), (int)(unsigned)(bits >> 32), 1, c->stream)) != hipSuccess) return e;
    q.prune_bound = (unsigned long long*)w;
    q.prune_stats = (int*)(w + 8);
    if (a.noise.mode < 0) q.nominal_candidate = -1;  // (given splines have no nominal: no candidate is exempt)
  }
  c->last_pruned = pruned; c->last_pruned_batched = bpruned;
  // (mjpcx_set_prune_rank: completions leave the word at +inf -- the setters refuse a finite initial bound in rank mode -- and rank_bound_kernel
  // writes the K-th smallest completed return into it behind the main launch)
  const bool ranked = pruned && c->prune_rank > 1;
  q.keep_bound = ranked;
  c->last_prune_rank = ranked ? c->prune_rank : 1;
  // (mjpcx_set_park_hint: a pruned launch only -- the settling pass needs its bound word. A batched one parks on its environments' own hints)
  const bool parking = bpruned ? bparking : pruned && c->park_allowed && c->park_hint < HUGE_VAL;
  c->park_h[0] = c->park_h[1] = c->park_h[2] = 0; c->park_resume_ms = 0;
  // the most workgroups a batched resume launch can have (resume_table.h): every environment's own ceil on top of what resume_cpw aims at
  const size_t group_cap = bpruned ? (size_t)std::min<long long>(N, std::max<long long>(1024, N / 16) + bE) : 0;
  if (parking) {
    if ((e = c->d_park_rec.reserve((size_t)N * quad::kQParkRec * sizeof(double))) != hipSuccess || (e = c->d_resume.reserve((size_t)N * sizeof(int))) != hipSuccess) return e;
    if (bpruned && (e = c->d_resume_groups.reserve(group_cap * sizeof(quad::ResumeGroup))) != hipSuccess) return e;
    if (!bpruned) q.park_hint = c->park_hint;  // (a batched launch reads each environment's hint from its record)
    q.park_records = (double*)c->d_park_rec.p;
    // (a resumed candidate may get a wavefront of its own: a slab build needs one slab per candidate then)
    // (the fleet's resume launch gives every environment whole workgroups of its own: up to 4 wavefronts per environment more than candidates)
    if (quad::quad_uses_ovf_slab() && (e = c->d_qovf.reserve(((size_t)N + 4 * (size_t)bE) * quad::quad_ovf_doubles_per_wave() * sizeof(double))) != hipSuccess) return e;
    if (quad::quad_uses_ovf_slab()) q.ovf_slab = (double*)c->d_qovf.p;
  }
  if (c->quad_stamps) {
    if ((e = hipMemsetAsync(c->d_qstamps.p, 0, 512, c->stream)) != hipSuccess) return e;
    q.stamps = (long long*)c->d_qstamps.p;
    const size_t wb = (size_t)N * 32;  // (one wavefront per candidate at most)
    if ((e = c->d_qwave.reserve(wb)) != hipSuccess || (e = hipMemsetAsync(c->d_qwave.p, 0, wb, c->stream)) != hipSuccess) return e;
    q.wave_times = (long long*)c->d_qwave.p;
  }
  static const bool classes = getenv("MJPCX_QUAD_CLASSES") != nullptr;  // (tuning aid: cycles by class of wavefront-step, printed after every launch)
  const int nwave = quad::quad_waves(N, c->quad_cpw);
  if (classes) {
    const size_t wb = (size_t)nwave * 64 * 8;
    if ((e = c->d_qclass.reserve(wb)) != hipSuccess || (e = hipMemsetAsync(c->d_qclass.p, 0, wb, c->stream)) != hipSuccess) return e;
    q.wave_class = (long long*)c->d_qclass.p;
  }
  if ((e = quad::launch_rollout_quad(mr.qmodel, mr.qtab, wt.blob, bo, q,
                                     (int*)c->d_qstats.p, c->stream)) != hipSuccess) return e;
  if (classes) {
    std::vector<long long> w((size_t)nwave * 64), tot(64, 0);
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(w.data(), c->d_qclass.p, w.size() * 8, hipMemcpyDeviceToHost);
    for (int i = 0; i < nwave; i++) for (int k = 0; k < 64; k++) tot[k] += w[(size_t)i * 64 + k];
    long long steps = 0, cyc = 0, scyc = 0;
    for (int k = 0; k < 16; k++) { steps += tot[32 + 2 * k]; cyc += tot[32 + 2 * k + 1]; scyc += tot[2 * k + 1]; }
    std::fprintf(stderr, "rollout_quad_kernel wavefront-steps by class (rel = a contact between two moving geoms in some candidate, leg = a leg-leg one, ovf = a lane beyond its "
                         "LDS slots, bey = beyond the line-search slots): %lld steps, %.0f cycles per step, %.0f of them in the solve\n", steps, steps ? (double)cyc / steps : 0.0,
                 steps ? (double)scyc / steps : 0.0);
    for (int k = 0; k < 16; k++)
      if (tot[32 + 2 * k] > 0)
        std::fprintf(stderr, "  %s%s%s%s%s: %5.1f %% of the steps, %5.1f %% of the cycles; per step %.0f cycles, solve %.0f\n", k == 0 ? "plain" : "", (k & 1) ? "rel " : "", (k & 2) ? "leg " : "",
                     (k & 4) ? "ovf " : "", (k & 8) ? "bey " : "", 100.0 * tot[32 + 2 * k] / steps, 100.0 * tot[32 + 2 * k + 1] / cyc, (double)tot[32 + 2 * k + 1] / tot[32 + 2 * k],
                     tot[2 * k] ? (double)tot[2 * k + 1] / tot[2 * k] : 0.0);
  }
  if (c->timing && c->cur_main) { if ((e = hipEventRecord(c->cur_main, c->stream)) != hipSuccess) return e; c->cur_main = nullptr; }
  // rank mode: every environment's bound word becomes the K-th smallest return its candidates have completed with (+inf: fewer than K have)
  if (ranked) {
    hipLaunchKernelGGL(rank_bound_kernel, dim3(bpruned ? bE : 1), dim3(kRankBoundThreads), 0, c->stream, (const double*)a.total_return, (const int*)a.failure,
                       bpruned ? bn : N, c->prune_rank, q.prune_bound, q.rec_stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  // the settling pass: parked candidates against the launch's final bound; its two counts ride on the readback below (words 14 and 15)
  if (parking) {
    hipLaunchKernelGGL(park_settle_kernel, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, (const double*)a.total_return, a.failure,
                       (const unsigned long long*)q.prune_bound, q.prune_stats, (int*)c->d_resume.p,
                       bpruned ? (int*)((char*)c->d_qstats.p + 64 + quad::kQEnvRecWords) : (int*)c->d_qstats.p + 14, bn, q.rec_stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (c->quad_stamps) {
    long long h[64];
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h, c->d_qstamps.p, 512, hipMemcpyDeviceToHost);
    static const char* nm[13] = {"policy", "kin..rne", "collision", "pairs", "factor+rows", "residual+record", "newton", "euler", "n:grad", "n:hessian", "n:factor+solve",
                                 "n:linesearch", "n:update+eval"};
    std::fprintf(stderr, "rollout_quad_kernel cycles of wavefront 0 (H = %d):", a.H);
    for (int k = 0; k < 13; k++) std::fprintf(stderr, " %s %lld", nm[k], h[k]);
    std::fprintf(stderr, " | newton iterations %lld, line-search trials %lld\n", h[16], h[17]);
    std::fprintf(stderr, "  raw counters 40..63:");
    for (int k = 40; k < 64; k++) std::fprintf(stderr, " %lld", h[k]);
    std::fprintf(stderr, "\n");
    std::fprintf(stderr, "  newton: entry %lld, first pass %lld, warm start %lld; line search: entry %lld, coefficients %lld, trials %lld\n", h[13], h[14], h[15], h[40], h[41], h[42]);
    {
      const int W = quad::quad_waves(N, c->quad_cpw);
      std::vector<long long> w((size_t)W * 4);
      (void)hipMemcpy(w.data(), c->d_qwave.p, w.size() * 8, hipMemcpyDeviceToHost);
      std::vector<int> order(W);
      for (int i = 0; i < W; i++) order[i] = i;
      std::sort(order.begin(), order.end(), [&](int x, int y) { return w[4 * x] < w[4 * y]; });
      std::fprintf(stderr, "  wavefronts by cycles (Newton iterations run, steps in the general solver, sum of largest per-lane contact counts):");
      const double qs[7] = {0.0, 0.1, 0.5, 0.9, 0.99, 0.999, 1.0};
      for (double qq : qs) { const int i = order[(size_t)(qq * (W - 1))]; std::fprintf(stderr, " p%g %lld (%lld, %lld, %lld)", 100 * qq, w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]); }
      std::fprintf(stderr, "\n");
    }
    std::fprintf(stderr, "  steps at which some lane of the wavefront holds > 0 1 2 3 4 6 8 12 contacts: %lld %lld %lld %lld %lld %lld %lld %lld; contacts per lane-step %.2f; "
                 "Newton iterations per candidate-step %.2f (the wavefront runs the slowest's: %.2f)\n", h[18], h[19], h[20], h[21], h[22], h[23], h[24], h[25],
                 (double)h[26] / (64.0 * a.H), (double)h[36] / (64.0 * a.H), (double)h[37] / a.H);
  }
  if (c->quad_no_fallback) return hipSuccess;
  // the pass over the candidates the quad kernel handed on is 16384 wavefronts that each find their candidate unflagged (0.24 ms) when
  // nothing was handed on -- the usual case: the count comes back first (32 bytes, one synchronisation the plan step pays anyway a moment later)
  // (a pruned launch's counters ride on the same copy: mjpcx_best and mjpcx_prune_stats need no synchronisation of their own for them)
  if (bpruned) {
    // the environments' records come back behind the hand-on counters, in the one copy and the one synchronisation of the plan step
    char* const hb = (char*)c->h_envrec.p;
    auto rec_int = [&](int env, unsigned off, int k) { int v; std::memcpy(&v, hb + 64 + (size_t)env * quad::kQEnvRec + off + 4 * k, 4); return v; };
    if ((e = hipMemcpyAsync(hb, c->d_qstats.p, 64 + brec, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    long long resumed_all = 0;
    c->resume_count.assign(bE, 0);
    for (int k = 0; k < bE && parking; k++) {
      const int parked = rec_int(k, quad::kQEnvRecWords, 0), resumed = rec_int(k, quad::kQEnvRecWords, 1);
      if (parked < 0 || parked > bn || resumed < 0 || resumed > parked) return hipErrorUnknown;  // (these counts size a launch: never past an environment's segment)
      c->resume_count[k] = resumed; resumed_all += resumed;
      c->env_park_h[3 * k] = parked; c->env_park_h[3 * k + 1] = parked - resumed; c->env_park_h[3 * k + 2] = resumed;
    }
    if (resumed_all > 0) {
      // ONE resume launch for the fleet: every environment's list gets whole workgroups of its own (a workgroup stages one environment's
      // model, poses and blob), and the table that tells a workgroup its environment and its slice of that list goes up ahead of the launch
      const int cpw = quad::resume_cpw(resumed_all), W = quad::resume_wpg(quad::resume_waves(c->resume_count.data(), bE, cpw));
      c->resume_groups.resize(group_cap);
      const long long grid = quad::resume_table_build(c->resume_count.data(), bE, cpw, W, c->resume_groups.data(), (long long)group_cap);
      if (grid <= 0) return hipErrorUnknown;
      if ((e = hipMemcpyAsync(c->d_resume_groups.p, c->resume_groups.data(), (size_t)grid * sizeof(quad::ResumeGroup), hipMemcpyHostToDevice, c->stream)) != hipSuccess) return e;
      quad::QArgs r = q;
      r.resume_list = (const int*)c->d_resume.p; r.resume_n = (int)resumed_all; r.cpw = cpw;
      r.resume_groups = (const quad::ResumeGroup*)c->d_resume_groups.p;
      for (int k = 0; k < 2; k++) if (!c->park_ev[k] && (e = hipEventCreate(&c->park_ev[k])) != hipSuccess) return e;
      if ((e = hipEventRecord(c->park_ev[0], c->stream)) != hipSuccess) return e;
      if ((e = quad::launch_resume_quad_groups(mr.qmodel, mr.qtab, wt.blob, bo, r, W, (int)grid, (int*)c->d_qstats.p, c->stream)) != hipSuccess) return e;
      if ((e = hipEventRecord(c->park_ev[1], c->stream)) != hipSuccess) return e;
      if ((e = hipMemcpyAsync(hb, c->d_qstats.p, 64 + brec, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
      float ms = 0;
      if (hipEventElapsedTime(&ms, c->park_ev[0], c->park_ev[1]) == hipSuccess) c->park_resume_ms = ms;
    }
    for (int k = 0; k < 4; k++) c->prune_h[k] = 0;
    c->prune_final = HUGE_VAL;
    for (int k = 0; k < bE; k++) {
      for (int j = 0; j < 4; j++) { c->env_prune_h[4 * k + j] = rec_int(k, quad::kQEnvRecStats, j); c->prune_h[j] += rec_int(k, quad::kQEnvRecStats, j); }
      for (int j = 0; j < 3; j++) c->park_h[j] += c->env_park_h[3 * k + j];
      std::memcpy(&c->env_prune_final[k], hb + 64 + (size_t)k * quad::kQEnvRec + quad::kQEnvRecBound, 8);
      c->prune_final = std::min(c->prune_final, c->env_prune_final[k]);
    }
    int h0;
    std::memcpy(&h0, hb, 4);
    if (h0 == 0 && !c->quad_stats) return hipSuccess;
  } else if (!c->quad_stats || pruned) {
    if (!c->h_qstats && hipHostMalloc(&c->h_qstats, 64, hipHostMallocDefault) != hipSuccess) c->h_qstats = nullptr;
    if (c->h_qstats) {
      if ((e = hipMemcpyAsync(c->h_qstats, c->d_qstats.p, pruned ? 64 : 32, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
      const int* h = static_cast<const int*>(c->h_qstats);
      if (parking && h[15] > 0) {
        // what the settling pass could not retire goes on from its records, pruned against the same bound word and never parked again; its
        // hand-ons, retirements and the bound it may lower come back with a second copy of the block
        const int parked = h[14], resumed = h[15];
        quad::QArgs r = q;
        r.park_hint = HUGE_VAL; r.resume_list = (const int*)c->d_resume.p; r.resume_n = resumed; r.cpw = 0;
        for (int k = 0; k < 2; k++) if (!c->park_ev[k] && (e = hipEventCreate(&c->park_ev[k])) != hipSuccess) return e;
        if ((e = hipEventRecord(c->park_ev[0], c->stream)) != hipSuccess) return e;
        if ((e = quad::launch_resume_quad(mr.qmodel, mr.qtab, wt.blob, bo, r, (int*)c->d_qstats.p, c->stream)) != hipSuccess) return e;
        if ((e = hipEventRecord(c->park_ev[1], c->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(c->h_qstats, c->d_qstats.p, 64, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->park_ev[0], c->park_ev[1]) == hipSuccess) c->park_resume_ms = ms;
        c->park_h[0] = parked; c->park_h[1] = parked - resumed; c->park_h[2] = resumed;
      } else if (parking) { c->park_h[0] = c->park_h[1] = h[14]; }
      if (pruned) { for (int k = 0; k < 4; k++) c->prune_h[k] = h[10 + k]; std::memcpy(&c->prune_final, h + 8, 8); }
      if (h[0] == 0 && !c->quad_stats) return hipSuccess;
    } else if (pruned) return hipErrorOutOfMemory;
  }
  RolloutArgs<double> a2 = a;
  a2.noise.mode = -1;  // the quad kernel left every candidate's spline nodes in a.nodes
  e = launch_tree<TreeCfgA1, double>(c, wm, wt, a2, mr.image, c->wh.blob_bytes, N, P, /*only_flagged=*/true);
  if (e == hipSuccess && c->quad_stats) {
    int h[8] = {0};
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h, c->d_qstats.p, 32, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "rollout_quad_kernel: %d of %d candidates handed to rollout_tree_kernel (contact list full %d, moving-geom pair %d, indefinite Hessian %d, "
                 "non-finite %d, both joint limits %d, trunk-leg pair %d)\n", h[0], N, h[1], h[2], h[3], h[4], h[5], h[6]);
  }
  return e;
}

// limb kernel (limb_kernel.h), then the wavefront-per-candidate kernel for the candidates it handed on
template <typename T>
hipError_t launch_limb(mjpcx_ctx* c, const WaveModelT<T>& wm, const WaveTaskT<T>& wt, const RolloutArgs<T>& a, int N, int P, const ModelRecords& mr) {
  limb::LArgs<T> q{};
  q.N = a.N; q.H = a.H; q.P = a.P; q.interp = a.interp; q.node_times = a.node_times; q.nodes = a.nodes; q.nominal = a.nominal;
  q.noise_mode = a.noise.mode; q.seed = a.noise.seed; q.iteration = a.noise.iteration; q.candidate_offset = a.noise.candidate_offset;
  q.nominal_candidate = a.noise.nominal_candidate; q.explore_count = a.noise.explore_count; q.std0 = a.noise.std0; q.std1 = a.noise.std1;
  q.param_variance = a.noise.param_variance;
  q.states = a.states; q.actions = a.actions; q.times = a.times; q.residual = a.residual; q.costs = a.costs; q.trace = a.trace;
  q.total_return = a.total_return; q.failure = a.failure; q.cpw = c->limb_cpw;
  q.env_n = a.env_n; q.env_stride = a.env_stride; q.seed_shared = a.seed_shared;
  const limb::LBlob bo{wt.off_time, wt.off_mocap, wt.off_weight, wt.off_normp, wt.off_normq, wt.off_param, wt.off_risk, wt.off_rreal, wt.off_rint};
  hipError_t e;
  if ((e = hipMemsetAsync(c->d_qstats.p, 0, 32, c->stream)) != hipSuccess) return e;  // (how many candidates are handed on, by reason: mjpcx_quad_stats)
  static const bool stamps = getenv("MJPCX_LIMB_STAMPS") != nullptr;  // (tuning aid: phase cycles of wavefront 0, Newton iterations; synchronises every rollout)
  if (stamps) {
    if ((e = c->d_qstamps.reserve(512)) != hipSuccess || (e = hipMemsetAsync(c->d_qstamps.p, 0, 512, c->stream)) != hipSuccess) return e;
    q.stamps = (long long*)c->d_qstamps.p;
    if ((e = c->d_qwave.reserve((size_t)N * 4)) != hipSuccess) return e;
    q.iters = (int*)c->d_qwave.p;
  }
  if ((e = limb::launch_rollout_limb(mr.limb, wt.blob, bo, q, wm.key_mpos, (int*)c->d_qstats.p, mr.limb_stride, c->stream)) != hipSuccess) return e;
  if (stamps) {
    long long h[64];
    std::vector<int> it((size_t)N);
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h, c->d_qstamps.p, sizeof h, hipMemcpyDeviceToHost);
    (void)hipMemcpy(it.data(), c->d_qwave.p, (size_t)N * 4, hipMemcpyDeviceToHost);
    long long sum = 0; int mx = 0;
    for (int v : it) { sum += v; mx = v > mx ? v : mx; }
    std::fprintf(stderr, "rollout_limb_kernel cycles of wavefront 0 (H = %d): policy %lld forward %lld residual+record %lld newton %lld euler %lld | Newton iterations per candidate-step %.2f (most over a rollout: %d)\n",
                 a.H, h[0], h[1], h[2], h[3], h[4], (double)sum / ((double)N * (a.H > 1 ? a.H - 1 : 1)), mx);
    std::fprintf(stderr, "  newton: setup %lld | per iteration (the wavefront ran %lld): hessian %lld factor+solve %lld woodbury %lld mul+dots %lld linesearch %lld update+eval %lld\n",
                 h[8], h[15], h[9], h[10], h[11], h[12], h[13], h[14]);
    std::fprintf(stderr, "  line-search derivative evaluations of candidate 0: %lld\n", h[16]);
    std::fprintf(stderr, "  forward: kinematics+inertias %lld M %lld velocity+bias %lld factor+solve %lld sites %lld rows %lld floor %lld pairs %lld pair list %lld\n",
                 h[20], h[21], h[22], h[23], h[24], h[25], h[26], h[27], h[28]);
    std::fprintf(stderr, "  residual: joint entries %lld marker averages %lld marker entries %lld\n", h[29], h[30], h[31]);
    if (h[32] | h[33] | h[34] | h[35] | h[36] | h[37] | h[38] | h[39])  // (stamps a tuning build adds: -DLEXP_XSTAMPS)
      std::fprintf(stderr, "  raw 32..39: %lld %lld %lld %lld %lld %lld %lld %lld\n", h[32], h[33], h[34], h[35], h[36], h[37], h[38], h[39]);
  }
  if (c->timing && c->cur_main) { if ((e = hipEventRecord(c->cur_main, c->stream)) == hipSuccess) c->cur_main = nullptr; else return e; }
  if (c->limb_no_fallback) return hipSuccess;
  if (!c->quad_stats) {  // the count of hand-ons comes back first: nothing handed on (the usual case) -> no second launch
    if (!c->h_qstats && hipHostMalloc(&c->h_qstats, 64, hipHostMallocDefault) != hipSuccess) c->h_qstats = nullptr;
    if (c->h_qstats) {
      if ((e = hipMemcpyAsync(c->h_qstats, c->d_qstats.p, 32, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
      if (static_cast<const int*>(c->h_qstats)[0] == 0) return hipSuccess;
    }
  }
  RolloutArgs<T> a2 = a;
  a2.noise.mode = -1;  // the limb kernel left every candidate's spline nodes in a.nodes
  e = launch_tree<TreeCfgHumanoid, T>(c, wm, wt, a2, mr.image,
                                      sizeof(T) == 8 ? c->wh.blob_bytes : c->wh.blob_bytes32, N, P, /*only_flagged=*/true);
  if (e == hipSuccess && c->quad_stats) {
    int h[8] = {0};
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(h, c->d_qstats.p, 32, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "rollout_limb_kernel: %d of %d candidates handed to rollout_tree_kernel (floor contact list full %d, more moving-geom contacts than slots %d, "
                 "indefinite matrix %d, non-finite %d, both limits %d, trunk on the floor %d)\n", h[0], N, h[1], h[2], h[3], h[4], h[5], h[6]);
  }
  return e;
}

// the context's WaveModel with every pointer moved from the context's own model allocation to environment 0's record of c->em.cold (the
// records have the allocation's layout; the kernel adds its environment's offset, RolloutArgs::model_stride)
template <typename T>
WaveModelT<T> env_models_view(const mjpcx_ctx* c, const WaveModelT<T>& own, int env = 0) {
  WaveModelT<T> wm = own;
  const char* from = (const char*)own.base;
  const char* to = (const char*)c->em.cold.p + (size_t)env * c->em.cold_stride;
  wm.meaninertia = c->em.meaninertia[env];  // (read by the generic kernel alone, which is launched per environment)
#define X(name) wm.name = reinterpret_cast<decltype(wm.name)>(to + ((const char*)own.name - from));
  MJPCX_WAVE_MODEL_POINTERS(X)
#undef X
  wm.base = (const unsigned char*)to;
  return wm;
}

// What launch_wave takes from the context in one precision, and the one step that differs between the two: launching a generic kernel
// (rollout_wave_kernel) by its id of wave32_launch.h over n candidates. fp64: this translation unit's instantiations; fp32: wave32.hip's.
template <typename T> struct WaveSide;
template <> struct WaveSide<double> {
  static const WaveModel& model(const mjpcx_ctx* c) { return c->wh.m; }
  static const WaveTask& task(const mjpcx_ctx* c) { return c->wh.t; }
  static size_t blob_bytes(const mjpcx_ctx* c) { return c->wh.blob_bytes; }
  static hipError_t launch(int which, int n, size_t lds, const WaveModel& m, const WaveTask& wt, const RolloutArgs<double>& a, hipStream_t stream) {
    auto kern = which == kW32Rk4 ? w64::rollout_wave_kernel<32, false, true>
              : which == kW32TreeRk4 ? w64::rollout_wave_kernel<32, true, true>
              : which == kW32Tree ? w64::rollout_wave_kernel<32, true>
              : which == kW32TreeSmall ? w64::rollout_wave_kernel<32, true, false, true>
              : which == kW32Rows18 ? w64::rollout_wave_kernel<18> : which == kW32Rows20 ? w64::rollout_wave_kernel<20>
              : which == kW32Rows28 ? w64::rollout_wave_kernel<28> : w64::rollout_wave_kernel<32>;
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(n), dim3(64), lds, stream, m, wt, a);
    return hipGetLastError();
  }
};
template <> struct WaveSide<float> {
  static const WaveModelT<float>& model(const mjpcx_ctx* c) { return c->wh.m32; }
  static const WaveTaskT<float>& task(const mjpcx_ctx* c) { return c->wh.t32; }
  static size_t blob_bytes(const mjpcx_ctx* c) { return c->wh.blob_bytes32; }
  template <class... Args> static hipError_t launch(Args&&... args) { return launch_wave_kernel_f32(args...); }
};

int reserve_wave_stamps(mjpcx_ctx* c) {  // (MJPCX_STAMPS: 48 zeroed cycle stamps)
  HIPCHK(c, c->d_stage.reserve(48 * 8));
  HIPCHK(c, hipMemsetAsync(c->d_stage.p, 0, 48 * 8, c->stream));
  return MJPCX_OK;
}

// The rollout of a wavefront-per-candidate context (c->wave), both precisions: the kernel family is chosen and launched, and c->cur_main
// recorded behind its first (dominant) kernel -- by launch_quad, launch_limb, launch_tree's first pass (unless only_flagged), here behind
// the first of two generic passes, otherwise by do_rollout. *refused: a refusal that is no launch error, already reported through fail().
template <typename T>
hipError_t launch_wave(mjpcx_ctx* c, const RolloutArgs<T>& a, const void* d_blob, const ModelRecords& mr, int E, int* refused) {
  using Side = WaveSide<T>;
  constexpr bool f64 = sizeof(T) == 8;
  const int N = a.N, P = a.P, registered = c->wh.registered;
  WaveTaskT<T> wt = Side::task(c);
  wt.blob = (const T*)d_blob;
  wt.stamps = nullptr;
  if (c->stamp_step >= 0) {
    if ((*refused = reserve_wave_stamps(c)) != MJPCX_OK) return hipSuccess;
    wt.stamps = (long long*)c->d_stage.p;
    wt.stamp_step = c->stamp_step;
  }
  const WaveModelT<T> wm = mr.per_env ? env_models_view(c, Side::model(c)) : Side::model(c);
  const size_t blob_bytes = Side::blob_bytes(c);
  const bool packed = a.xfrc_scale == 0 && !wt.stamps;  // the quad and limb kernels draw no force noise and carry no stamps
  // A rank's share of the batch decides the kernel: the quad kernel packs 16 candidates into a wavefront, which fills the 1024 SIMDs
  // at N = 16384 but leaves most of them idle below a quarter of that, where one wavefront per candidate (a third of the latency per
  // step) is quicker -- measured cross-over on MI355X: N = 4096 (tools/quad_n_sweep.py; MJPCX_QUAD_MIN_N moves it)
  if constexpr (f64)  // (the quad kernel is fp64 only: quad_ok is never set on an fp32 context)
    if (registered == 0 && c->quad_ok && packed && N >= c->quad_min_n) return launch_quad(c, wm, wt, a, N, P, mr, /*plain=*/E == 0);
  if (registered == 1 && c->limb_ok && packed && N >= c->limb_min_n) return launch_limb<T>(c, wm, wt, a, N, P, mr);
  if (registered == 0 || (registered == 1 && wm.integrator != MJPCX_INT_RK4)) {
    // mjpcx_quad_stats reports the LAST rollout, so a context that owns a hand-on counter (quad_ok: fp64 contexts only; limb_ok: either
    // precision) clears it whenever it rolls out on the tree kernel instead: nothing was handed on in this one. An fp32 context of the A1
    // has no counter and no mjpcx_quad_stats output to go stale, so one rule serves both precisions.
    if (registered == 0 ? c->quad_ok : c->limb_ok) (void)hipMemsetAsync(c->d_qstats.p, 0, 32, c->stream);
    const hipError_t le = registered == 0 ? launch_tree<TreeCfgA1, T>(c, wm, wt, a, mr.image, blob_bytes, N, P)
                                          : launch_tree<TreeCfgHumanoid, T>(c, wm, wt, a, mr.image, blob_bytes, N, P);
    if (wt.stamps && le == hipSuccess) print_wave_stamps(c, wt.stamps, wt.stamp_step, 0, true);
    return le;
  }
  // the generic kernels. The Jacobian-free constraint path for the models it covers: in two passes under Euler -- short contact lists for
  // everybody, the long ones for the candidates that overflowed -- in one with the long lists under RK4 (one NMAX = 32 instantiation per
  // kernel family carries mj_RungeKutta; the row-table kernel's lists overflow on a folded Humanoid)
  const bool tree = c->wh.tree_ok && !c->no_tree;
  const bool rk4 = wm.integrator == MJPCX_INT_RK4;
  const bool two_pass = tree && !rk4 && !c->no_second_pass;
  auto tree_lds = [&](bool big) {
    const int caps = big ? (f64 ? w64::kTreeMaxSimpleBig : w32::kTreeMaxSimpleBig) : (f64 ? w64::kTreeMaxSimple : w32::kTreeMaxSimple);
    const int capc = big ? (f64 ? w64::kTreeMaxConeBig : w32::kTreeMaxConeBig) : (f64 ? w64::kTreeMaxCone : w32::kTreeMaxCone);
    const size_t elems = f64 ? w64::wave_lds_elems_tree(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, wt.nr, wt.nterm, P, a.xfrc_scale > 0, caps, capc)
                             : w32::wave_lds_elems_tree(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, wt.nr, wt.nterm, P, a.xfrc_scale > 0, caps, capc);
    return (sizeof(T) * elems + 15) & ~(size_t)15;
  };
  const size_t rows_elems = f64 ? w64::wave_lds_elems(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, wt.nr, wt.nterm, P, wm.cone, /*nodes_in_lds=*/false, a.xfrc_scale > 0)
                                : w32::wave_lds_elems(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, wt.nr, wt.nterm, P, wm.cone, /*nodes_in_lds=*/false, a.xfrc_scale > 0);
  const size_t lds_big = tree ? tree_lds(true) : (sizeof(T) * rows_elems + 15) & ~(size_t)15;
  const size_t lds = two_pass ? tree_lds(false) : lds_big;
  if (lds_big > 160 * 1024) { *refused = fail(c, MJPCX_EUNSUPPORTED, "model state does not fit the 160 KB LDS of a CU"); return hipSuccess; }
  // the register-resident Cholesky is unrolled to NMAX columns: instantiations that fit the registered models exactly (A1:
  // nv = 18, humanoid: 27) skip the padding columns' updates (humanoid: 30 % of the factorisation's instructions); the shipped tree
  // models are registered, so one width serves the unregistered ones
  const int kern_big = rk4 ? (tree ? kW32TreeRk4 : kW32Rk4) : tree ? kW32Tree
                     : wm.nv <= 18 ? kW32Rows18 : wm.nv <= 20 ? kW32Rows20 : wm.nv <= 28 ? kW32Rows28 : kW32Rows32;
  // one launch over the N candidates -- or, with a model per environment, one per environment on its model (this kernel reads the model
  // through the pointers of its arguments: RolloutArgs::cand_base)
  auto launch_generic = [&](int which, size_t lds_bytes, const RolloutArgs<T>& args) -> hipError_t {
    if (!mr.per_env) return Side::launch(which, N, lds_bytes, wm, wt, args, c->stream);
    const int n = N / E;
    for (int e = 0; e < E; e++) {
      RolloutArgs<T> ae = args;
      ae.cand_base = e * n;
      const hipError_t he = Side::launch(which, n, lds_bytes, env_models_view(c, Side::model(c), e), wt, ae, c->stream);
      if (he != hipSuccess) return he;
    }
    return hipSuccess;
  };
  hipError_t le = launch_generic(two_pass ? kW32TreeSmall : kern_big, lds, a);
  if (two_pass && le == hipSuccess) {
    if (c->timing && c->cur_main) { if ((le = hipEventRecord(c->cur_main, c->stream)) == hipSuccess) c->cur_main = nullptr; }
    RolloutArgs<T> a2 = a;
    a2.noise.mode = -1;  // the first pass left every candidate's spline nodes in a.nodes
    a2.only_overflowed = 1;
    if (le == hipSuccess) le = launch_generic(kern_big, lds_big, a2);
  }
  if (wt.stamps && le == hipSuccess) print_wave_stamps(c, wt.stamps, wt.stamp_step, lds, tree);
  return le;
}

// an event pair around one launch (kernel_ms of mjpcx_backward_pass / mjpcx_gradient_pass); destroyed on every way out of the call
struct LaunchTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~LaunchTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  hipError_t start(hipStream_t s) {
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    return e == hipSuccess ? hipEventRecord(e0, s) : e;
  }
  hipError_t stop(hipStream_t s) { return hipEventRecord(e1, s); }
  double ms() const { float t = 0; (void)hipEventElapsedTime(&t, e0, e1); return t; }  // (after the call's sync)
};
// The rollouts' timer (mjpcx_timing_*) keeps its events: with c->timing the context's next triple, created on first use, is this rollout's.
// The first is recorded here, c->cur_main behind the rollout's first (dominant) kernel by whoever launches it, *e1 by do_rollout at the end.
int begin_rollout_timing(mjpcx_ctx* c, hipEvent_t* e1) {
  *e1 = nullptr;
  if (!c->timing) return MJPCX_OK;
  if (c->events_used == c->events.size()) {
    hipEvent_t x, y, z;
    HIPCHK(c, hipEventCreate(&x));
    HIPCHK(c, hipEventCreate(&y));
    c->events.emplace_back(x, y);
    HIPCHK(c, hipEventCreate(&z));
    c->events_main.push_back(z);
  }
  const hipEvent_t e0 = c->events[c->events_used].first;
  *e1 = c->events[c->events_used].second;
  c->cur_main = c->events_main[c->events_used];
  c->events_used++;
  HIPCHK(c, hipEventRecord(e0, c->stream));
  return MJPCX_OK;
}

// One rollout, as every entry point asks for it. Exactly one source of the N splines: node_values, nominal + noise, or nodes_on_device.
struct RolloutRequest {
  int N, H, P, interp;
  const double* node_times;  // P, or E x P
  // 0: the plain entry points (one environment, the state of mjpcx_set_state). E >= 1: N = E x n_per_env candidates, environment-major,
  // from the states of mjpcx_set_states; node_times is E x P and nominal E x P*nu. Same launch code, same kernels.
  int E = 0;
  const double* node_values = nullptr;  // N x P*nu host splines, candidate-major: scattered onto the device, and the call syncs
  const double* nominal = nullptr; const mjpcx_noise_spec* noise = nullptr;  // the spline the device draws the candidates around, and how
  // (mjpcx_rollout_noise_batched_ce) E x P*nu cross-entropy variances, one row per environment, instead of noise->param_variance for all
  const double* variance_rows = nullptr;
  // (mjpcx_robust_step_batched, mjpcx_rollout_sample_gradient_batched) a kernel enqueued on this stream has already written the N splines
  // into d_nodes, which the caller reserved for this shape -- no host splines, no scatter, no sync
  bool nodes_on_device = false;
  // NoisyRollout: force noise of this standard deviation and rate (0: plain Rollout); given splines draw candidate j's stream at xfrc_offset + j
  double xfrc_std = 0, xfrc_rate = 1; uint64_t xfrc_seed = 0; int xfrc_offset = 0;
  // (mjpcx_rollout_noise_batched) the one batched launch mjpcx_set_pruning_batched applies to
  bool prune_batched = false;
  // (mjpcx_rollout_noise_ensemble) every environment draws the noise stream of noise->seed itself: the environments roll out the same candidates
  bool seed_shared = false;
  // (mjpcx_rollout_cma_batched) the caller began this launch's timing in front of the kernel that wrote the splines and recorded c->cur_main
  // behind it: that kernel is the launch's first, the one mjpcx_timing_read_main singles out. timing_e1: what begin_rollout_timing gave.
  bool timing_begun = false;
  hipEvent_t timing_e1 = nullptr;
};

template <typename T>
int do_rollout(mjpcx_ctx* c, const RolloutRequest& r) {
  const int N = r.N, H = r.H, P = r.P, E = r.E;
  const double *const node_values = r.node_values, *const variance_rows = r.variance_rows;
  const mjpcx_noise_spec* const ns = r.noise;
  int rc;
  if ((rc = reserve_rollout(c, N, H, P)) != MJPCX_OK) return rc;
  c->last_pruned = false; c->last_pruned_batched = false;  // (launch_quad sets them)
  c->bprune_req = r.prune_batched;
  const int np = P * c->nu;
  RolloutArgs<T> a{};
  a.N = N; a.H = H; a.P = P; a.interp = r.interp;
  // a model per environment (mjpcx_set_models_batched; check_batched_args has compared the two E): the batched launches read the
  // environments' records, with their strides; everything else the context's own model, with strides of 0
  const ModelRecords mr = model_records(c, E > 0 && c->em.E > 0, sizeof(T) == 4);
  if (mr.per_env) { a.model_stride = c->em.cold_stride; a.image_stride = c->em.image_stride; }
  a.nodes = (T*)c->d_nodes.p;
  a.noise.mode = -1;
  a.seed_shared = r.seed_shared ? 1 : 0;
  const double* d_var = nullptr;
  mjpcx_ctx::Slot* slot = nullptr;
  const bool ce = ns && ns->mode == MJPCX_NOISE_CROSS_ENTROPY;
  if (ce && !ns->param_variance && !variance_rows) return fail(c, MJPCX_EINVAL, "cross-entropy noise needs param_variance");
  const void* d_blob = nullptr;
  if ((rc = stage_plan_inputs<T>(c, P, E, r.node_times, r.nominal, !ce ? nullptr : variance_rows ? variance_rows : ns->param_variance, variance_rows != nullptr, &a.node_times,
                                 &a.nominal, &d_var, &slot, &d_blob, &a.env_stride)) != MJPCX_OK) return rc;
  a.env_n = E > 1 ? N / E : 0;
  if (!c->wave) a.init = (const LaneInit<T>*)d_blob;
  if (node_values) {
    // candidate-major host splines -> [node][actuator][candidate] on the device (not the hot path:
    // the planner generates candidates on the device; this entry serves tests and NominalTrajectory)
    HIPCHK(c, c->d_in_nodes.reserve((size_t)N * np * 8));
    HIPCHK(c, hipMemcpyAsync(c->d_in_nodes.p, node_values, (size_t)N * np * 8, hipMemcpyHostToDevice, c->stream));
    const size_t total = (size_t)N * np;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL((scatter_nodes_kernel<T>), dim3(blocks), dim3(256), 0, c->stream,
                       (const double*)c->d_in_nodes.p, (T*)c->d_nodes.p, N, np);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // pageable source buffer: make caller reuse safe
  } else if (!r.nodes_on_device) {
    a.noise.mode = ns->mode;
    a.noise.seed = ns->seed; a.noise.iteration = ns->iteration;
    a.noise.candidate_offset = ns->candidate_offset; a.noise.nominal_candidate = ns->nominal_candidate;
    a.noise.explore_count = ns->explore_count; a.noise.std0 = ns->std0; a.noise.std1 = ns->std1;
    a.noise.param_variance = ce ? d_var : nullptr;
  }
  a.states = (T*)c->d_states.p; a.actions = (T*)c->d_actions.p; a.times = (T*)c->d_times.p;
  a.residual = (T*)c->d_residual.p; a.costs = (T*)c->d_costs.p; a.trace = (T*)c->d_trace.p;
  a.total_return = (double*)c->d_ret.p; a.failure = (int*)c->d_fail.p;
  a.xfrc_decay = 0; a.xfrc_scale = 0; a.xfrc_seed = 0;
  if (r.xfrc_std > 0) {  // Ornstein-Uhlenbeck in discrete time (trajectory.cc:149-150), at the planning timestep
    a.xfrc_decay = std::exp(-(c->wave ? c->wh.m.timestep : c->hm64.timestep) / r.xfrc_rate);
    a.xfrc_scale = r.xfrc_std * std::sqrt(1 - a.xfrc_decay * a.xfrc_decay);
    a.xfrc_seed = r.xfrc_seed;
    if (a.noise.mode < 0) a.noise.candidate_offset = r.xfrc_offset;
  }

  hipEvent_t e1 = r.timing_e1;
  if (!r.timing_begun && (rc = begin_rollout_timing(c, &e1)) != MJPCX_OK) return rc;
  hipError_t le;
  if (c->wave) {
    int refused = MJPCX_OK;
    le = launch_wave<T>(c, a, d_blob, mr, E, &refused);
    if (refused != MJPCX_OK) return refused;
  } else if constexpr (sizeof(T) == 8) {
    le = c->kernel->launch64(c->hm64, c->ht64, a, c->stream);
  } else {
    convert_task(c->ht32, c->ht64);
    le = c->kernel->launch32(c->hm32, c->ht32, a, c->stream);
  }
  if (le != hipSuccess) return fail(c, MJPCX_EDEVICE, std::string("rollout kernel launch: ") + hipGetErrorString(le));
  if (c->timing && c->cur_main) { HIPCHK(c, hipEventRecord(c->cur_main, c->stream)); c->cur_main = nullptr; }  // (paths with one kernel, or whose first pass is not singled out)
  if (c->timing) HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, slot->host.mark(c->stream));
  c->N = N; c->H = H; c->P = P;
  c->env_n = E > 0 ? N / E : 0;
  c->have_rollout = true;
  c->rollout_serial++;
  c->traj_candidate_major = c->wave;
  return MJPCX_OK;
}
int rollout(mjpcx_ctx* c, const RolloutRequest& r) { return c->precision == 64 ? do_rollout<double>(c, r) : do_rollout<float>(c, r); }

// run(double{}) or run(float{}): one launch in the context's precision, for kernels that differ only in the element type of their buffers
template <class Run>
auto by_precision(const mjpcx_ctx* c, Run&& run) { return c->precision == 64 ? run(double{}) : run(float{}); }

// A sort of every environment's n candidates by env_sort_keys (ce_update_kernel, robust_select_kernel, sg_update_kernel), one workgroup of
// 1024 threads per environment and chunk: n2 keys (a power of two and a multiple of the workgroup) in dynamic LDS up to kCeLdsKeys, beyond
// that in slabs of c->d_sort, the slab of (environment e, chunk k) at (e * chunks + k) * n2 keys.
struct EnvSort {
  int n2 = 1024;
  bool in_lds;
  size_t lds;
  hipError_t reserve(mjpcx_ctx* c, int n, int E, int chunks = 1) {
    while (n2 < n) n2 <<= 1;
    in_lds = n2 <= kCeLdsKeys;
    lds = in_lds ? (size_t)n2 * kSortKeyBytes : 0;
    return in_lds ? hipSuccess : c->d_sort.reserve((size_t)E * chunks * n2 * kSortKeyBytes);
  }
  double* slabs(const mjpcx_ctx* c) const { return in_lds ? nullptr : (double*)c->d_sort.p; }
  // launch(kernel, T{}) once kernel = pick(T{}, IN_LDS{}), a generic lambda that names the caller's Kernel<T, IN_LDS>, is allowed its LDS
  template <class Pick, class Launch>
  hipError_t dispatch(const mjpcx_ctx* c, Pick&& pick, Launch&& launch) const {
    auto go = [&](auto tag, auto kern) {
      const hipError_t e = in_lds ? hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
      if (e != hipSuccess) return e;
      launch(kern, tag);
      return hipGetLastError();
    };
    return by_precision(c, [&](auto tag) { return in_lds ? go(tag, pick(tag, std::true_type{})) : go(tag, pick(tag, std::false_type{})); });
  }
};

int check_rollout_args(mjpcx_ctx* c, int N, int H, int P, int interp, const double* node_times) {
  if (!c || !node_times) return fail(c, MJPCX_EINVAL, "null argument");
  if (N < 1 || H < 1 || P < 1) return fail(c, MJPCX_EINVAL, "num_candidates, horizon and num_nodes must be >= 1");
  if (interp < 0 || interp > 2) return fail(c, MJPCX_EINVAL, "unknown interpolation");
  for (int p = 1; p < P; p++)
    if (!(node_times[p] > node_times[p - 1])) return fail(c, MJPCX_EINVAL, "node_times must be strictly increasing");
  const size_t shmem = c->wave ? 0 : ((size_t)P * c->nu * 64 + P) * esize(c);
  if (shmem > 64 * 1024) return fail(c, MJPCX_EUNSUPPORTED, "num_nodes * nu too large for the LDS spline stage");
  if (hipSetDevice(c->device) != hipSuccess) return fail(c, MJPCX_EDEVICE, "hipSetDevice failed");
  return MJPCX_OK;
}

}  // namespace

// ===================================================================== C ABI
extern "C" {

const char* mjpcx_error_string(int code) {
  switch (code) {
    case MJPCX_OK: return "ok";
    case MJPCX_EINVAL: return "invalid argument";
    case MJPCX_EUNSUPPORTED: return "model or task not supported by any device kernel";
    case MJPCX_EDEVICE: return "HIP runtime error";
    case MJPCX_ENOMEM: return "out of memory";
    case MJPCX_ESTATE: return "call out of order";
    default: return "unknown error";
  }
}
const char* mjpcx_last_error(const mjpcx_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }
const char* mjpcx_kernel_name(const mjpcx_ctx* ctx) { return ctx && ctx->kernel ? ctx->kernel->name : ""; }

static thread_local std::string g_create_error;
// the environment is read when a context is created, never on the launch path
static int env_stamp_step() { const char* e = getenv("MJPCX_STAMPS"); return e ? std::atoi(e) : -1; }
const char* mjpcx_create_error(void) { return g_create_error.c_str(); }

int mjpcx_create(const mjpcx_model* m, const mjpcx_task* t, int device, int precision, mjpcx_ctx** out) {
  g_create_error.clear();
  auto bad = [&](int code, const std::string& msg) { g_create_error = msg; return code; };
  if (!m || !t || !out) return bad(MJPCX_EINVAL, "null argument");
  *out = nullptr;
  if (precision != 64 && precision != 32) return bad(MJPCX_EINVAL, "precision must be 64 or 32");
  // ---- features the device kernels cover today
  if (m->na != 0) return bad(MJPCX_EUNSUPPORTED, "actuator activations (na > 0) unsupported");
  const int given_integrator = m->integrator;
  mjpcx_model m_euler;
  if (m->integrator == MJPCX_INT_IMPLICITFAST) {
    // mj_implicit with qDeriv = d qfrc_smooth / d qvel restricted to passive damping + actuator velocity terms: without the latter the
    // matrix is M + h diag(damping), mj_Euler's own (include/mjpcx.h). The context then runs the Euler path on a copy of the header.
    for (int i = 0; i < m->nu; i++)
      if (m->actuator_biasprm && m->actuator_biastype && m->actuator_biastype[i] == MJPCX_BIAS_AFFINE && m->actuator_biasprm[3 * i + 2] != 0)
        return bad(MJPCX_EUNSUPPORTED, "implicitfast with a velocity-dependent actuator (affine bias, biasprm[2] != 0): only models whose velocity-dependent smooth "
                                       "force is joint damping are integrated (as mj_Euler, which is the same update there)");
    // mj_implicit ignores mjDSBL_EULERDAMP, mj_Euler switches to explicit damping under it: the two updates differ then
    if (m->disableflags & MJPCX_DSBL_EULERDAMP)
      return bad(MJPCX_EUNSUPPORTED, "implicitfast with eulerdamp disabled: mj_implicit keeps the damping implicit, the Euler path this context would run does not");
    m_euler = *m;
    m_euler.integrator = MJPCX_INT_EULER;
    m = &m_euler;
  }
  if (m->integrator != MJPCX_INT_EULER && m->integrator != MJPCX_INT_RK4)
    return bad(MJPCX_EUNSUPPORTED, "integrators: Euler, RK4 and (damping-only models) implicitfast; implicit is not implemented");
  // ---- wavefront-per-candidate family: free/ball joints, friction loss, contacts
  bool needs_wave = false;
  for (int j = 0; j < m->njnt; j++) needs_wave |= m->jnt_type[j] == MJPCX_JNT_FREE || m->jnt_type[j] == MJPCX_JNT_BALL;
  for (int i = 0; i < m->nv; i++) needs_wave |= m->dof_frictionloss[i] > 0 && !(m->disableflags & MJPCX_DSBL_FRICTIONLOSS);
  if (!(m->disableflags & MJPCX_DSBL_CONTACT) && m->ngeom > 0) {
    bool st = false, dy = false;
    for (int g = 0; g < m->ngeom; g++) {
      if (!(m->geom_contype[g] || m->geom_conaffinity[g])) continue;
      bool moving = false;
      for (int b = m->geom_bodyid[g]; b > 0; b = m->body_parentid[b]) moving |= m->body_dofnum[b] > 0;
      (moving ? dy : st) = true;
    }
    needs_wave |= st && dy;
  }
  for (int k = 0; k < m->ntendon; k++) needs_wave |= m->tendon_limited[k] != 0;
  if (needs_wave) {

    for (int j = 0; j < m->njnt; j++)
      if (m->jnt_limited[j] && (m->jnt_type[j] == MJPCX_JNT_FREE || m->jnt_type[j] == MJPCX_JNT_BALL))
        return bad(MJPCX_EUNSUPPORTED, "limits on free/ball joints are not implemented");
    if (t->num_trace * 3 > 64 || m->nu > 64 || t->num_term > 64 || t->num_residual > kWaveMaxEfc * m->nv)
      return bad(MJPCX_EUNSUPPORTED, "task exceeds the wave kernel capacity");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bad(MJPCX_EDEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return bad(MJPCX_EINVAL, "device index out of range");
    if (hipSetDevice(device) != hipSuccess) return bad(MJPCX_EDEVICE, "hipSetDevice failed");
    mjpcx_ctx* c = new (std::nothrow) mjpcx_ctx();
    if (!c) return bad(MJPCX_ENOMEM, "host allocation failed");
    c->device = device; c->precision = precision; c->stamp_step = env_stamp_step(); c->no_tree = getenv("MJPCX_NO_TREE") != nullptr; c->no_lds_model = getenv("MJPCX_NO_LDS_MODEL") != nullptr;
    if (precision == 32) c->max_waves = 12;
    if (const char* e = getenv("MJPCX_TREE_WAVES")) c->max_waves = std::max(1, std::min(precision == 32 ? 12 : 8, std::atoi(e)));
    if (const char* e = getenv("MJPCX_TREE_MODE")) c->tree_mode = std::atoi(e);
    c->no_second_pass = getenv("MJPCX_TREE_ONE_PASS") != nullptr;
    c->no_cone_slabs = getenv("MJPCX_TREE_NO_SLABS") != nullptr;
    c->kernel = &kWaveEntry; c->wave = true;
    c->nq = m->nq; c->nv = m->nv; c->nu = m->nu; c->na = m->na; c->nmocap = m->nmocap; c->nsite_model = m->nsite;
    c->nr = t->num_residual; c->nterm = t->num_term; c->ntrace = t->num_trace; c->nparam = t->num_parameter;
    c->num_norm_parameter.assign(t->num_norm_parameter, t->num_norm_parameter + t->num_term);
    c->dim_norm_residual.assign(t->dim_norm_residual, t->dim_norm_residual + t->num_term);
    c->ctrllimited.assign(m->actuator_ctrllimited, m->actuator_ctrllimited + m->nu);
    c->ctrlrange.assign(m->actuator_ctrlrange, m->actuator_ctrlrange + 2 * m->nu);
    const std::string err = c->wh.build(m, t, precision == 32);
    if (!err.empty()) { mjpcx_destroy(c); return bad(MJPCX_EUNSUPPORTED, err); }
    own_copy(c->own, m, t, given_integrator);  // (mjpcx_set_models_batched builds and compares against them)
    if (c->wh.tree_ok && !c->no_tree && !c->no_lds_model && lds_model_matches<TreeCfgA1>(m, t, c->wh)) {
      // registered model: the LDS image of its hot arrays (lds_model.h), in the context's precision
      std::vector<unsigned char> img = precision == 64 ? lds_model_image<TreeCfgA1, double>(m, t, c->wh) : lds_model_image<TreeCfgA1, float>(m, t, c->wh);
      void** slot = precision == 64 ? &c->wh.dev_image : &c->wh.dev_image32;
      if (hipMalloc(slot, img.size()) != hipSuccess || hipMemcpy(*slot, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
        mjpcx_destroy(c);
        return bad(MJPCX_ENOMEM, "upload of the model's LDS image failed");
      }
      c->wh.registered = 0;
      c->kernel = &kTreeEntryA1;
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cu = prop.multiProcessorCount;
      c->quad_stats = getenv("MJPCX_QUAD_STATS") != nullptr;
      c->quad_stamps = getenv("MJPCX_QUAD_STAMPS") != nullptr;
      c->quad_no_fallback = getenv("MJPCX_QUAD_NO_FALLBACK") != nullptr;
      c->no_quad_feedback = getenv("MJPCX_NO_QUAD_FEEDBACK") != nullptr;
      if (const char* e = getenv("MJPCX_QUAD_CON_CAP")) c->quad_con_cap = std::atoi(e);
      if (const char* e = getenv("MJPCX_PARK")) c->park_allowed = std::atoi(e) != 0;    // (0: mjpcx_set_park_hint does nothing)
      if (const char* e = getenv("MJPCX_PRUNE")) c->prune_allowed = std::atoi(e) != 0;  // (0: mjpcx_set_pruning does nothing -- the same binary, A/B)
      if (const char* e = getenv("MJPCX_QUAD_MIN_N")) c->quad_min_n = std::atoi(e);
      if (const char* e = getenv("MJPCX_QUAD_CPW")) { const int v = std::atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) c->quad_cpw = v; }
      if (precision == 64 && !getenv("MJPCX_NO_QUAD")) {
        // the quad kernel family (four lanes per candidate): models of the legged class quad_build accepts
        std::vector<unsigned char> hq, ht;
        c->quad_why = quad::build_images(m, t, hq, ht);
        if (c->quad_why.empty()) {
          if (c->d_qmodel.reserve(hq.size()) != hipSuccess || c->d_qtab.reserve(ht.size()) != hipSuccess || c->d_qstats.reserve(64) != hipSuccess ||
              c->d_qstamps.reserve(512) != hipSuccess || hipMemset(c->d_qstats.p, 0, 64) != hipSuccess ||
              hipMemcpy(c->d_qmodel.p, hq.data(), hq.size(), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(c->d_qtab.p, ht.data(), ht.size(), hipMemcpyHostToDevice) != hipSuccess) {
            mjpcx_destroy(c);
            return bad(MJPCX_ENOMEM, "upload of the quad kernel's model failed");
          }
          c->quad_ok = true;
          c->kernel = &kQuadEntryA1;
          for (int k = 0; k < 7; k++) c->quad_ids[k] = t->residual_int[1 + k];
        }
      }
    }
    else if (c->wh.tree_ok && !c->no_tree && !c->no_lds_model && lds_model_matches<TreeCfgHumanoid>(m, t, c->wh)) {
      std::vector<unsigned char> img = precision == 64 ? lds_model_image<TreeCfgHumanoid, double>(m, t, c->wh) : lds_model_image<TreeCfgHumanoid, float>(m, t, c->wh);
      void** slot = precision == 64 ? &c->wh.dev_image : &c->wh.dev_image32;
      if (hipMalloc(slot, img.size()) != hipSuccess || hipMemcpy(*slot, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
        mjpcx_destroy(c);
        return bad(MJPCX_ENOMEM, "upload of the model's LDS image failed");
      }
      c->wh.registered = 1;
      c->kernel = &kTreeEntryHumanoid;
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cu = prop.multiProcessorCount;
      c->quad_stats = getenv("MJPCX_QUAD_STATS") != nullptr;
      c->limb_no_fallback = getenv("MJPCX_LIMB_NO_FALLBACK") != nullptr;
      if (const char* e = getenv("MJPCX_LIMB_MIN_N")) c->limb_min_n = std::atoi(e);
      if (const char* e = getenv("MJPCX_LIMB_CPW")) { const int v = std::atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) c->limb_cpw = v; }
      if (!getenv("MJPCX_NO_LIMB")) {   // (both precisions: the fp64 instantiation spills more but is still ahead of the tree kernel, 78 against 95 ms on configs[3]'s share)
        // the limb kernel family (four lanes per candidate, one per limb): models of the class limb_build accepts
        std::vector<unsigned char> h32, h64;
        c->limb_why = limb::build_images(m, t, h32, h64);
        if (c->limb_why.empty()) {
          const std::vector<unsigned char>& img = precision == 64 ? h64 : h32;
          if (c->d_limb.reserve(img.size()) != hipSuccess || c->d_qstats.reserve(32) != hipSuccess || hipMemset(c->d_qstats.p, 0, 32) != hipSuccess ||
              hipMemcpy(c->d_limb.p, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
            mjpcx_destroy(c);
            return bad(MJPCX_ENOMEM, "upload of the limb kernel's model failed");
          }
          c->limb_ok = true;
          c->kernel = &kLimbEntryHumanoid;
          for (int k = 0; k < 32; k++) c->limb_ids[k] = t->residual_int[2 + k];
        }
      }
    }
    set_norm_params(c, t->norm_parameter);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { mjpcx_destroy(c); return bad(MJPCX_EDEVICE, "hipStreamCreate failed"); }
    g_create_error = c->wh.warning;  // (empty, or what this context does NOT model of the caller's mjModel)
    if (!c->wh.warning.empty() && getenv("MJPCX_STRICT_PAIRS")) {  // strict callers (tests, parity runs) refuse a model whose physics is not fully reproduced
      const std::string why = c->wh.warning;
      mjpcx_destroy(c);
      return bad(MJPCX_EUNSUPPORTED, why.c_str());
    }
    // a model the Jacobian-free path could serve, but with no registered configuration (dimensions in tree_registry.h): it runs -- on the
    // generic kernel, at a fraction of the registered kernel's rate. Say so instead of leaving the caller to find out from the clock.
    if (c->wh.tree_ok && c->wh.registered < 0 && !c->no_tree && !c->no_lds_model)
    {
      char dims[320];
      std::snprintf(dims, sizeof dims, " (a configuration for it would read NQ = %d, NV = %d, NU = %d, NB = %d, NJ = %d, NS = %d, NG = %d, NKEY = %d, NMOCAP = %d, "
                    "NSG = %d, NDG = %d, NRAY = %d, NR = %d, NTERM = %d, NTRACE = %d, NT = %d)", m->nq, m->nv, m->nu, c->wh.m.nbody, m->njnt, c->wh.m.nsite, m->ngeom,
                    m->nkey, m->nmocap, (int)c->wh.h_static_geom.size(), (int)c->wh.h_dynamic_geom.size(), (int)c->wh.h_ray_geom.size(), t->num_residual,
                    t->num_term, t->num_trace, m->ntendon);
      g_create_error += std::string(g_create_error.empty() ? "" : "; ") + "note: no registered kernel configuration for this model's dimensions (tree_registry.h): "
                        "served by the generic wavefront-per-candidate kernel" + dims;
    }
    *out = c;
    return MJPCX_OK;
  }
  if (m->nq != m->nv || m->njnt != m->nv) return bad(MJPCX_EUNSUPPORTED, "only slide/hinge joints are implemented (nq == nv == njnt)");
  if (m->ntendon > 0) return bad(MJPCX_EUNSUPPORTED, "tendons are only implemented in the wavefront-per-candidate kernel (limited fixed tendons)");
  if (m->nbody > kLaneMaxBody || m->nv > kLaneMaxDof || m->nu > kLaneMaxAct || m->nsite > kLaneMaxSite ||
      m->nmocap > kLaneMaxMocap || t->num_term > kLaneMaxTerm || t->num_parameter > kLaneMaxParam)
    return bad(MJPCX_EUNSUPPORTED, "model exceeds the small-model kernel capacity");
  for (int j = 0; j < m->njnt; j++) {
    if (m->jnt_type[j] != MJPCX_JNT_SLIDE && m->jnt_type[j] != MJPCX_JNT_HINGE)
      return bad(MJPCX_EUNSUPPORTED, "only slide/hinge joints are implemented");
    if (m->jnt_dofadr[j] != j || m->jnt_qposadr[j] != j) return bad(MJPCX_EINVAL, "joint/dof addressing is not 1:1");
    if (m->dof_frictionloss[j] > 0) return bad(MJPCX_EUNSUPPORTED, "joint frictionloss unsupported");
    if (m->jnt_limited[j] && !(m->jnt_range[2 * j + 1] - m->jnt_range[2 * j] > 2 * m->jnt_margin[j]))
      return bad(MJPCX_EUNSUPPORTED, "joint range narrower than twice its margin");
  }
  if (!(m->disableflags & MJPCX_DSBL_CONTACT)) return bad(MJPCX_EUNSUPPORTED, "contacts are not implemented: the model must disable them");
  for (int u = 0; u < m->nu; u++)
    if (m->actuator_trnid[u] < 0 || m->actuator_trnid[u] >= m->njnt) return bad(MJPCX_EINVAL, "actuator transmission out of range");

  // ---- static-topology key of the runtime model
  TopoKey tk{m->nbody, m->nv, m->nu, m->nsite, m->nmocap, 0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < m->nbody; b++) {
    tk.parent |= (uint64_t)(m->body_parentid[b] & 15) << (4 * b);
    tk.mocap |= (uint64_t)((m->body_mocapid[b] < 0 ? 15 : m->body_mocapid[b]) & 15) << (4 * b);
  }
  for (int j = 0; j < m->njnt; j++) {
    tk.jtype |= (uint64_t)(m->jnt_type[j] & 3) << (2 * j);
    tk.jbody |= (uint64_t)(m->jnt_bodyid[j] & 15) << (4 * j);
    tk.jlimited |= (uint64_t)(m->jnt_limited[j] ? 1 : 0) << j;
  }
  for (int u = 0; u < m->nu; u++) tk.actj |= (uint64_t)(m->actuator_trnid[u] & 15) << (4 * u);
  for (int s = 0; s < m->nsite; s++) tk.siteb |= (uint64_t)(m->site_bodyid[s] & 15) << (4 * s);
  TaskKey kk{t->residual_id, t->num_residual, t->num_term, t->num_trace, 0, 0};
  for (int k = 0; k < t->num_term; k++) kk.termdim |= (uint64_t)(t->dim_norm_residual[k] & 15) << (4 * k);
  for (int k = 0; k < t->num_trace; k++) kk.tracesite |= (uint64_t)(t->trace_site[k] & 15) << (4 * k);
  const KernelEntry* entry = nullptr;
  LaneModel<double> probe;
  fill_model(probe, m);
  for (const KernelEntry& e : kKernels)
    if (e.topo == tk && e.task == kk && (!e.static_model || (!getenv("MJPCX_NO_STATIC") && same_model(*e.static_model, probe)))) {
      entry = &e;
      break;
    }
  if (!entry) {
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "no rollout kernel is instantiated for this model/task topology: Topo<%d,%d,%d,%d,%d,0x%llx,0x%llx,0x%llx,"
                  "0x%llx,0x%llx,0x%llx,0x%llx> TaskTopo<%d,%d,%d,0x%llx,%d,0x%llx> (add it to kKernels in csrc/mjpcx.hip)",
                  tk.nb, tk.nv, tk.nu, tk.nsite, tk.nmocap, (unsigned long long)tk.parent, (unsigned long long)tk.mocap,
                  (unsigned long long)tk.jtype, (unsigned long long)tk.jbody, (unsigned long long)tk.jlimited,
                  (unsigned long long)tk.actj, (unsigned long long)tk.siteb, kk.rid, kk.nr, kk.nterm,
                  (unsigned long long)kk.termdim, kk.ntrace, (unsigned long long)kk.tracesite);
    return bad(MJPCX_EUNSUPPORTED, buf);
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bad(MJPCX_EDEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return bad(MJPCX_EINVAL, "device index out of range");
  if (hipSetDevice(device) != hipSuccess) return bad(MJPCX_EDEVICE, "hipSetDevice failed");

  mjpcx_ctx* c = new (std::nothrow) mjpcx_ctx();
  if (!c) return bad(MJPCX_ENOMEM, "host allocation failed");
  c->device = device; c->precision = precision; c->stamp_step = env_stamp_step(); c->kernel = entry;
  c->nq = m->nq; c->nv = m->nv; c->nu = m->nu; c->na = m->na; c->nmocap = m->nmocap;
  c->nr = t->num_residual; c->nterm = t->num_term; c->ntrace = t->num_trace; c->nparam = t->num_parameter;
  c->num_norm_parameter.assign(t->num_norm_parameter, t->num_norm_parameter + t->num_term);
  c->dim_norm_residual.assign(t->dim_norm_residual, t->dim_norm_residual + t->num_term);
  c->ctrllimited.assign(m->actuator_ctrllimited, m->actuator_ctrllimited + m->nu);
  c->ctrlrange.assign(m->actuator_ctrlrange, m->actuator_ctrlrange + 2 * m->nu);
  fill_model(c->hm64, m);
  fill_model(c->hm32, m);
  std::memset(&c->ht64, 0, sizeof c->ht64);
  for (int k = 0; k < t->num_term; k++) { c->ht64.norm[k] = t->norm[k]; c->ht64.weight[k] = t->weight[k]; }
  set_norm_params(c, t->norm_parameter);
  for (int k = 0; k < t->num_parameter; k++) c->ht64.parameters[k] = t->parameters[k];
  c->ht64.risk = t->risk;
  for (int j = 0; j < m->nq; j++) c->ht64.qpos[j] = m->qpos0[j];
  for (int b = 0; b < m->nbody; b++)
    if (m->body_mocapid[b] >= 0) {
      for (int k = 0; k < 3; k++) c->ht64.mocap_pos[m->body_mocapid[b]][k] = m->body_pos[3 * b + k];
      for (int k = 0; k < 4; k++) c->ht64.mocap_quat[m->body_mocapid[b]][k] = m->body_quat[4 * b + k];
    }
  auto cleanup = [&](int code, const std::string& msg) { mjpcx_destroy(c); return bad(code, msg); };
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return cleanup(MJPCX_EDEVICE, "hipStreamCreate failed");
  *out = c;
  return MJPCX_OK;
}

void mjpcx_destroy(mjpcx_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& ev : c->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  for (auto& ev : c->events_main) (void)hipEventDestroy(ev);
  for (auto& sl : c->slots) { sl.host.release(); sl.dev.release(); }
  c->h_ilqg.release();
  c->h_grad.release();
  c->h_envrec.release();
  c->result.release();
  if (c->h_qstats) (void)hipHostFree(c->h_qstats);
  for (hipEvent_t ev : c->park_ev) if (ev) (void)hipEventDestroy(ev);
  if (c->source_done) (void)hipEventDestroy(c->source_done);
  c->sg.release();
  c->cma.release();
  c->em.release();
  (void)mjpcx_comm_destroy(c);
  c->wh.release();
  DevBuf* bufs[] = {&c->d_nodes, &c->d_in_nodes, &c->d_grad, &c->d_ilqg, &c->d_ilqg_out, &c->d_work, &c->d_ovf, &c->d_qmodel, &c->d_qtab, &c->d_qstats, &c->d_qstamps, &c->d_qwave, &c->d_qovf, &c->d_qclass, &c->d_park_rec, &c->d_resume, &c->d_resume_groups, &c->d_limb, &c->d_comm_send, &c->d_comm_recv,
                    &c->d_states, &c->d_actions, &c->d_times, &c->d_residual, &c->d_costs, &c->d_trace, &c->d_ret,
                    &c->d_fail, &c->d_sort, &c->d_stage, &c->d_mppi};
  for (DevBuf* b : bufs) b->release();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int mjpcx_set_state(mjpcx_ctx* c, const double* state, double time, const double* mocap, const double* userdata) {
  if (!c || !state) return fail(c, MJPCX_EINVAL, "null argument");
  (void)userdata;  // nuserdata == 0 for every supported model
  if (c->wave) {
    std::memcpy(c->wh.state.data(), state, sizeof(double) * (c->nq + c->nv));
    c->wh.time = time;
    if (mocap) std::memcpy(c->wh.mocap.data(), mocap, sizeof(double) * 7 * c->nmocap);
    return MJPCX_OK;
  }
  for (int j = 0; j < c->nq; j++) c->ht64.qpos[j] = state[j];
  for (int j = 0; j < c->nv; j++) c->ht64.qvel[j] = state[c->nq + j];
  c->ht64.time = time;
  if (mocap)
    for (int i = 0; i < c->nmocap; i++) {  // trajectory.cc:121-124
      for (int k = 0; k < 3; k++) c->ht64.mocap_pos[i][k] = mocap[7 * i + k];
      for (int k = 0; k < 4; k++) c->ht64.mocap_quat[i][k] = mocap[7 * i + 3 + k];
    }
  return MJPCX_OK;
}

int mjpcx_set_task_params(mjpcx_ctx* c, const double* weight, const double* norm_parameter,
                          const double* parameters, double risk) {
  if (!c) return MJPCX_EINVAL;
  if (c->wave) {
    if (weight) c->wh.weight.assign(weight, weight + c->nterm);
    if (norm_parameter) set_norm_params(c, norm_parameter);
    if (parameters) c->wh.parameters.assign(parameters, parameters + c->nparam);
    c->wh.risk = risk;
    return MJPCX_OK;
  }
  if (weight) for (int k = 0; k < c->nterm; k++) c->ht64.weight[k] = weight[k];
  if (norm_parameter) set_norm_params(c, norm_parameter);
  if (parameters) for (int k = 0; k < c->nparam; k++) c->ht64.parameters[k] = parameters[k];
  c->ht64.risk = risk;
  return MJPCX_OK;
}

int mjpcx_set_residual_state(mjpcx_ctx* c, const int32_t* residual_int, const double* residual_real) {
  if (!c) return MJPCX_EINVAL;
  if (!c->wave) return (residual_int || residual_real) ? fail(c, MJPCX_EUNSUPPORTED, "this task's residual has no frozen state") : MJPCX_OK;
  if (residual_int) { c->wh.residual_int.assign(residual_int, residual_int + c->wh.t.nri); c->env_rint.clear(); }  // (all environments again)
  if (residual_real) c->env_rreal.clear();
  if (residual_int && c->quad_ok)  // the quad model bakes the ids Task::Reset resolves; a caller that changes them gets the generic path
    for (int k = 0; k < 7; k++) if (residual_int[1 + k] != c->quad_ids[k]) { c->quad_ok = false; c->kernel = &kTreeEntryA1; }
  if (residual_int && c->limb_ok)  // likewise the limb model: the tracking sites and mocap bodies (the motion's first / last key may change)
    for (int k = 0; k < 32; k++) if (residual_int[2 + k] != c->limb_ids[k]) { c->limb_ok = false; c->kernel = &kTreeEntryHumanoid; }
  if (residual_real) c->wh.residual_real.assign(residual_real, residual_real + c->wh.t.nrr);
  return MJPCX_OK;
}

int mjpcx_rollout_splines(mjpcx_ctx* c, int N, int H, int P, int interp, const double* node_times,
                          const double* node_values) {
  int rc = check_rollout_args(c, N, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!node_values) return fail(c, MJPCX_EINVAL, "null node_values");
  RolloutRequest r{N, H, P, interp, node_times};
  r.node_values = node_values;
  return rollout(c, r);
}

int mjpcx_rollout_splines_noisy(mjpcx_ctx* c, int N, int H, int P, int interp, const double* node_times, const double* node_values,
                                double xfrc_std, double xfrc_rate, uint64_t seed, int candidate_offset) {
  int rc = check_rollout_args(c, N, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!node_values) return fail(c, MJPCX_EINVAL, "null node_values");
  if (!(xfrc_std >= 0) || !(xfrc_rate > 0)) return fail(c, MJPCX_EINVAL, "xfrc_std must be >= 0 and xfrc_rate > 0");
  RolloutRequest r{N, H, P, interp, node_times};
  r.node_values = node_values;
  r.xfrc_std = xfrc_std; r.xfrc_rate = xfrc_rate; r.xfrc_seed = seed; r.xfrc_offset = candidate_offset;
  return rollout(c, r);
}

int mjpcx_rollout_noise(mjpcx_ctx* c, int N, int H, int P, int interp, const double* node_times,
                        const double* nominal, const mjpcx_noise_spec* ns) {
  int rc = check_rollout_args(c, N, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!nominal || !ns) return fail(c, MJPCX_EINVAL, "null argument");
  if (ns->mode != MJPCX_NOISE_SAMPLING && ns->mode != MJPCX_NOISE_CROSS_ENTROPY) return fail(c, MJPCX_EINVAL, "unknown noise mode");
  RolloutRequest r{N, H, P, interp, node_times};
  r.nominal = nominal; r.noise = ns;
  return rollout(c, r);
}

// ---- several environments per launch
int mjpcx_set_states(mjpcx_ctx* c, int E, const double* states, const double* times, const double* mocap, const double* userdata) {
  if (!c || !states || !times) return fail(c, MJPCX_EINVAL, "null argument");
  if (E < 1) return fail(c, MJPCX_EINVAL, "mjpcx_set_states: the number of environments must be >= 1");
  (void)userdata;  // nuserdata == 0 for every supported model
  const size_t nst = (size_t)c->nq + c->nv + c->na;
  c->env_state.assign(states, states + nst * E);
  c->env_time.assign(times, times + E);
  if (mocap) c->env_mocap.assign(mocap, mocap + (size_t)7 * c->nmocap * E);  // (NULL: every environment keeps the context's pose)
  else c->env_mocap.clear();
  if (c->env_E != E) { c->env_rint.clear(); c->env_rreal.clear(); clear_env_task_params(c); }  // (per-environment residual state and task parameters of another fleet size)
  c->env_E = E;
  return MJPCX_OK;
}

int mjpcx_set_residual_states(mjpcx_ctx* c, int E, const int32_t* residual_int, const double* residual_real) {
  if (!c) return MJPCX_EINVAL;
  if (E < 1) return fail(c, MJPCX_EINVAL, "mjpcx_set_residual_states: the number of environments must be >= 1");
  if (!c->wave) return (residual_int || residual_real) ? fail(c, MJPCX_EUNSUPPORTED, "this task's residual has no frozen state") : MJPCX_OK;
  if (E != c->env_E) return fail(c, MJPCX_EINVAL, "mjpcx_set_residual_states: " + std::to_string(E) + " environments, but mjpcx_set_states gave " + std::to_string(c->env_E));
  const int nri = c->wh.t.nri, nrr = c->wh.t.nrr;
  if (residual_int) {
    c->env_rint.assign(residual_int, residual_int + (size_t)nri * E);
    // the quad / limb models bake the ids Task::Reset resolves; a caller that changes them in any environment gets the generic path
    for (int e = 0; e < E; e++) {
      const int32_t* ri = residual_int + (size_t)e * nri;
      if (c->quad_ok) for (int k = 0; k < 7; k++) if (ri[1 + k] != c->quad_ids[k]) { c->quad_ok = false; c->kernel = &kTreeEntryA1; break; }
      if (c->limb_ok) for (int k = 0; k < 32; k++) if (ri[2 + k] != c->limb_ids[k]) { c->limb_ok = false; c->kernel = &kTreeEntryHumanoid; break; }
    }
  }
  if (residual_real) c->env_rreal.assign(residual_real, residual_real + (size_t)nrr * E);
  return MJPCX_OK;
}

int mjpcx_set_task_params_batched(mjpcx_ctx* c, int E, const double* weight, const double* norm_parameter, const double* parameters,
                                  const double* risk) {
  if (!c) return MJPCX_EINVAL;
  if (E < 1) return fail(c, MJPCX_EINVAL, "mjpcx_set_task_params_batched: the number of environments must be >= 1");
  if (E != c->env_E)
    return fail(c, MJPCX_EINVAL, "mjpcx_set_task_params_batched: " + std::to_string(E) + " environments, but mjpcx_set_states gave " + std::to_string(c->env_E));
  const size_t nt = c->nterm, npar = c->nparam;
  if (weight) c->env_weight.assign(weight, weight + nt * E); else c->env_weight.clear();
  if (norm_parameter) {  // split into p and q per term, as set_norm_params does
    c->env_normp.assign(nt * E, 0.0); c->env_normq.assign(nt * E, 0.0);
    size_t shift = 0;
    for (int e = 0; e < E; e++)
      for (size_t k = 0; k < nt; k++) {
        const int np = c->num_norm_parameter[k];
        if (np > 0) c->env_normp[e * nt + k] = norm_parameter[shift];
        if (np > 1) c->env_normq[e * nt + k] = norm_parameter[shift + 1];
        shift += np;
      }
  } else { c->env_normp.clear(); c->env_normq.clear(); }
  if (parameters && npar > 0) c->env_param.assign(parameters, parameters + npar * E); else c->env_param.clear();
  if (risk) c->env_risk.assign(risk, risk + E); else c->env_risk.clear();
  return MJPCX_OK;
}

namespace {
hipError_t upload_records(DevBuf& d, const std::vector<unsigned char>& h) {
  hipError_t e = d.reserve(h.size());
  return e != hipSuccess ? e : hipMemcpy(d.p, h.data(), h.size(), hipMemcpyHostToDevice);
}
}  // namespace

int mjpcx_set_models_batched(mjpcx_ctx* c, int E, const mjpcx_model* const* models) {
  if (!c) return MJPCX_EINVAL;
  const std::string who = "mjpcx_set_models_batched: ";
  if (E < 0) return fail(c, MJPCX_EINVAL, who + "the number of environments must be >= 0");
  if (!models || E == 0) {  // the context's one model for every environment again (a context that can hold none has none: nothing to do)
    if (c->em.E == 0) return MJPCX_OK;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, MJPCX_EDEVICE, "hipSetDevice failed");
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (a launch in flight may be reading the records)
    c->em.release();
    return MJPCX_OK;
  }
  if (!c->wave)
    return fail(c, MJPCX_EUNSUPPORTED, who + "this context runs a lane-per-candidate kernel, whose model constants are fixed when the library is built "
                                             "(generated/static_models.h): a model per environment needs a context of the contact family");
  if (c->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, who + "not implemented on a context sharded with mjpcx_comm_init (the batched rollouts are not either)");
  if (hipSetDevice(c->device) != hipSuccess) return fail(c, MJPCX_EDEVICE, "hipSetDevice failed");
  const mjpcx_model* ref = &c->own.m;
  const mjpcx_task* t = &c->own.t;
  for (int e = 0; e < E; e++) {
    if (!models[e]) return fail(c, MJPCX_EINVAL, who + "environment " + std::to_string(e) + ": null model");
    const std::string why = compare_env_model(ref, models[e], c->own.given_integrator);
    if (!why.empty()) return fail(c, MJPCX_EINVAL, who + "environment " + std::to_string(e) + ": " + why);
  }
  // the context's builders once per model, into host records of the layouts the context holds; nothing of the context changes before all succeeded
  const bool want32 = c->precision == 32;
  const size_t cold_bytes = (size_t)(want32 ? c->wh.m32.bytes : c->wh.m.bytes);
  std::vector<unsigned char> h_cold, h_image, h_qmodel, h_qtab, h_limb, one, two;
  size_t image_bytes = 0, qmodel_bytes = 0, qtab_bytes = 0, limb_bytes = 0;
  std::vector<double> meaninertia;
  for (int e = 0; e < E; e++) {
    const std::string env = who + "environment " + std::to_string(e) + ": ";
    mjpcx_model m = *models[e];
    if (m.integrator == MJPCX_INT_IMPLICITFAST) m.integrator = MJPCX_INT_EULER;  // (as mjpcx_create: the velocity-dependent terms are the context's model's, compared above)
    WaveHost wh;
    std::string why = wh.build(&m, t, want32, &one);
    if (!why.empty()) return fail(c, MJPCX_EUNSUPPORTED, env + why);
    const WaveModel& w0 = c->wh.m;
    if (one.size() != cold_bytes || wh.m.nbody != w0.nbody || wh.m.nsite != w0.nsite || wh.m.npair != w0.npair || wh.m.full != w0.full ||
        wh.m.nlevel != w0.nlevel || wh.m.any_damping != w0.any_damping || wh.tree_ok != c->wh.tree_ok)
      return fail(c, MJPCX_EUNSUPPORTED, env + "the model bakes to another layout than the context's (pair list, constraint classes or sizes)");
    h_cold.insert(h_cold.end(), one.begin(), one.end());
    meaninertia.push_back(m.meaninertia);
    if (c->wh.registered < 0) continue;  // (the generic kernel: the model allocation is all it reads)
    if (!(c->wh.registered == 0 ? lds_model_matches<TreeCfgA1>(&m, t, wh) : lds_model_matches<TreeCfgHumanoid>(&m, t, wh)))
      return fail(c, MJPCX_EUNSUPPORTED, env + "the model does not match the registered configuration the context's does (tree_registry.h)");
    if (c->wh.registered == 0) one = want32 ? lds_model_image<TreeCfgA1, float>(&m, t, wh) : lds_model_image<TreeCfgA1, double>(&m, t, wh);
    else one = want32 ? lds_model_image<TreeCfgHumanoid, float>(&m, t, wh) : lds_model_image<TreeCfgHumanoid, double>(&m, t, wh);
    image_bytes = one.size();
    h_image.insert(h_image.end(), one.begin(), one.end());
    if (c->d_qmodel.p) {  // (the context built the quad kernel's images)
      why = quad::build_images(&m, t, one, two);
      if (!why.empty()) return fail(c, MJPCX_EUNSUPPORTED, env + "the quad kernel's builder: " + why);
      qmodel_bytes = one.size(); qtab_bytes = two.size();
      h_qmodel.insert(h_qmodel.end(), one.begin(), one.end());
      h_qtab.insert(h_qtab.end(), two.begin(), two.end());
    }
    if (c->d_limb.p) {
      why = limb::build_images(&m, t, one, two);
      if (!why.empty()) return fail(c, MJPCX_EUNSUPPORTED, env + "the limb kernel's builder: " + why);
      const std::vector<unsigned char>& img = want32 ? one : two;
      limb_bytes = img.size();
      h_limb.insert(h_limb.end(), img.begin(), img.end());
    }
  }
  // upload into fresh buffers (synchronous copies: the records are on the device when this call returns), then wait for the work already
  // enqueued on the context's stream, which may read the records being replaced, and swap
  mjpcx_ctx::EnvModels em;
  hipError_t he = upload_records(em.cold, h_cold);
  if (he == hipSuccess && !h_image.empty()) he = upload_records(em.image, h_image);
  if (he == hipSuccess && !h_qmodel.empty()) he = upload_records(em.qmodel, h_qmodel);
  if (he == hipSuccess && !h_qtab.empty()) he = upload_records(em.qtab, h_qtab);
  if (he == hipSuccess && !h_limb.empty()) he = upload_records(em.limb, h_limb);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (he != hipSuccess) {
    em.release();
    return fail(c, he == hipErrorOutOfMemory ? MJPCX_ENOMEM : MJPCX_EDEVICE, who + "upload of the models: " + hipGetErrorString(he));
  }
  em.E = E;
  em.meaninertia = meaninertia;
  em.cold_stride = (unsigned)cold_bytes; em.image_stride = (unsigned)image_bytes;
  em.qmodel_stride = (unsigned)qmodel_bytes; em.qtab_stride = (unsigned)qtab_bytes; em.limb_stride = (unsigned)limb_bytes;
  c->em.release();
  c->em = em;  // (DevBuf is a plain pair: the records now belong to the context)
  return MJPCX_OK;
}

namespace {
int check_batched_args(mjpcx_ctx* c, int E, int n, int H, int P, int interp, const double* node_times) {
  if (!c || !node_times) return fail(c, MJPCX_EINVAL, "null argument");
  if (E < 1) return fail(c, MJPCX_EINVAL, "batched rollout: the number of environments must be >= 1");
  if (n < 64 || n % 64 != 0)
    return fail(c, MJPCX_EINVAL, "batched rollout: n_per_env = " + std::to_string(n) + " must be a positive multiple of 64 (a wavefront serves one environment)");
  if ((long long)E * n > 0x7fffffffLL / 64) return fail(c, MJPCX_EINVAL, "batched rollout: too many candidates");
  if (c->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, "batched rollouts on a context sharded with mjpcx_comm_init are not implemented");
  if (c->env_E != E)
    return fail(c, MJPCX_EINVAL, c->env_E == 0 ? std::string("batched rollout before mjpcx_set_states")
                                               : "batched rollout of " + std::to_string(E) + " environments after mjpcx_set_states of " + std::to_string(c->env_E));
  // (planning silently on the wrong physics is worse than an error: unlike the task rows, the models of another fleet size are not dropped)
  if (c->em.E > 0 && c->em.E != E)
    return fail(c, MJPCX_EINVAL, "batched rollout of " + std::to_string(E) + " environments on a context that holds " + std::to_string(c->em.E) +
                                     " models (mjpcx_set_models_batched)");
  for (int e = 0; e < E; e++) {
    const int rc = check_rollout_args(c, E * n, H, P, interp, node_times + (size_t)e * (P > 0 ? P : 0));
    if (rc != MJPCX_OK) return rc;
  }
  return MJPCX_OK;
}
// which candidates a pruned launch (mjpcx_set_pruning, mjpcx_set_pruning_batched) retires, and when, depends on the order its wavefronts finish in: only the argmin is exact
const char* const kPrunedRanking = "the last rollout was pruned (mjpcx_set_pruning): beyond the argmin its returns are lower bounds that depend on timing";
// ... and in rank mode (mjpcx_set_prune_rank) beyond the first K
int fail_ranking(mjpcx_ctx* c, const std::string& who = "") {
  if (c->last_prune_rank <= 1) return fail(c, MJPCX_ESTATE, who + kPrunedRanking);
  return fail(c, MJPCX_ESTATE, who + "the last rollout was pruned at rank " + std::to_string(c->last_prune_rank) + " (mjpcx_set_prune_rank): beyond its first " +
                                   std::to_string(c->last_prune_rank) + " its returns are lower bounds");
}
}  // namespace

int mjpcx_rollout_splines_batched(mjpcx_ctx* c, int E, int n, int H, int P, int interp, const double* node_times, const double* node_values) {
  int rc = check_batched_args(c, E, n, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!node_values) return fail(c, MJPCX_EINVAL, "null node_values");
  RolloutRequest r{E * n, H, P, interp, node_times, E};
  r.node_values = node_values;
  return rollout(c, r);
}

int mjpcx_rollout_splines_noisy_batched(mjpcx_ctx* c, int E, int n, int H, int P, int interp, const double* node_times, const double* node_values,
                                        double xfrc_std, double xfrc_rate, uint64_t seed, int candidate_offset) {
  int rc = check_batched_args(c, E, n, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!node_values) return fail(c, MJPCX_EINVAL, "null node_values");
  if (!(xfrc_std >= 0) || !(xfrc_rate > 0)) return fail(c, MJPCX_EINVAL, "xfrc_std must be >= 0 and xfrc_rate > 0");
  RolloutRequest r{E * n, H, P, interp, node_times, E};
  r.node_values = node_values;
  r.xfrc_std = xfrc_std; r.xfrc_rate = xfrc_rate; r.xfrc_seed = seed; r.xfrc_offset = candidate_offset;
  return rollout(c, r);
}

int mjpcx_rollout_noise_batched(mjpcx_ctx* c, int E, int n, int H, int P, int interp, const double* node_times, const double* nominal,
                                const mjpcx_noise_spec* ns) {
  int rc = check_batched_args(c, E, n, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!nominal || !ns) return fail(c, MJPCX_EINVAL, "null argument");
  if (ns->mode != MJPCX_NOISE_SAMPLING && ns->mode != MJPCX_NOISE_CROSS_ENTROPY) return fail(c, MJPCX_EINVAL, "unknown noise mode");
  RolloutRequest r{E * n, H, P, interp, node_times, E};
  r.nominal = nominal; r.noise = ns;
  // (a switch set for another fleet size is an error, not a launch that quietly rolls everything out: the rule of mjpcx_set_models_batched)
  if (c->bprune_on && c->bprune_E != E)
    return fail(c, MJPCX_EINVAL, "batched rollout of " + std::to_string(E) + " environments while mjpcx_set_pruning_batched is set for " + std::to_string(c->bprune_E));
  r.prune_batched = true;
  return rollout(c, r);
}

int mjpcx_rollout_noise_batched_ce(mjpcx_ctx* c, int E, int n, int H, int P, int interp, const double* node_times, const double* nominal,
                                   const double* variance, const mjpcx_noise_spec* ns) {
  int rc = check_batched_args(c, E, n, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!nominal || !variance || !ns) return fail(c, MJPCX_EINVAL, "null argument");
  if (ns->mode != MJPCX_NOISE_CROSS_ENTROPY) return fail(c, MJPCX_EINVAL, "mjpcx_rollout_noise_batched_ce: the noise mode must be MJPCX_NOISE_CROSS_ENTROPY");
  RolloutRequest r{E * n, H, P, interp, node_times, E};
  r.nominal = nominal; r.noise = ns; r.variance_rows = variance;
  // (rank mode only: with the bound of the argmin a pruned launch could not feed mjpcx_ce_update_batched, so at rank 1 the switch stays ignored)
  if (c->prune_rank > 1) {
    if (c->bprune_on && c->bprune_E != E)
      return fail(c, MJPCX_EINVAL, "batched rollout of " + std::to_string(E) + " environments while mjpcx_set_pruning_batched is set for " + std::to_string(c->bprune_E));
    r.prune_batched = true;
  }
  return rollout(c, r);
}

int mjpcx_ce_update_batched(mjpcx_ctx* c, int E, int n_elite, int skip_candidate, int32_t* index, double* total_return, double* mean,
                            double* variance, double* avg_return) {
  if (!c || !index) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (E < 1 || c->env_n < 1 || (long long)E * c->env_n != c->N)
    return fail(c, MJPCX_EINVAL, "mjpcx_ce_update_batched: the last rollout was not a batched one of " + std::to_string(E) + " environments");
  const int n = c->env_n, left = n - (skip_candidate >= 0 && skip_candidate < n ? 1 : 0);
  if (n_elite < 1 || n_elite > left)
    return fail(c, MJPCX_EINVAL, "mjpcx_ce_update_batched: n_elite = " + std::to_string(n_elite) + " outside 1.." + std::to_string(left) +
                                 " (the candidates of an environment without the skipped one)");
  // (after a launch in rank mode the first K of every environment's stored order are exact: the elites and the skipped candidate must fit in them)
  if (c->last_pruned && !(c->last_pruned_batched && c->last_prune_rank > 1 && n_elite + (skip_candidate >= 0 ? 1 : 0) <= c->last_prune_rank)) return fail_ranking(c);
  if (c->last_pruned) {
    std::string named;
    for (int e = 0; e < E && (size_t)e * 4 + 2 < c->env_prune_h.size(); e++) if (c->env_prune_h[4 * (size_t)e + 2]) named += (named.empty() ? "" : ", ") + std::to_string(e);
    if (!named.empty())
      return fail(c, MJPCX_ESTATE, "pruned batched rollout: a step's cost was negative in environment(s) " + named +
                                       ", so partial returns are no lower bounds there (roll out again with pruning off)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int np = c->P * c->nu;
  CeRecord rec;
  rec.off_index = 8;
  rec.off_ret = (rec.off_index + (size_t)n_elite * 4 + 7) & ~(size_t)7;
  rec.off_mean = rec.off_ret + (size_t)n_elite * 8;
  rec.off_var = rec.off_mean + (size_t)np * 8;
  rec.bytes = rec.off_var + (size_t)np * 8;
  HIPCHK(c, c->result.reserve(rec.bytes * E));
  EnvSort sort;
  HIPCHK(c, sort.reserve(c, n, E));
  const hipError_t le = sort.dispatch(c, [](auto t, auto in_lds) { return ce_update_kernel<decltype(t), decltype(in_lds)::value>; }, [&](auto kern, auto t) {
    hipLaunchKernelGGL(kern, dim3(E), dim3(1024), sort.lds, c->stream, (const double*)c->d_ret.p, (const decltype(t)*)c->d_nodes.p, c->N, n, sort.n2, np,
                       n_elite, skip_candidate, sort.slabs(c), (unsigned char*)c->result.dev, rec);
  });
  HIPCHK(c, le);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int e = 0; e < E; e++) {
    const char* r = (const char*)c->result.p + rec.bytes * e;
    std::memcpy(index + (size_t)e * n_elite, r + rec.off_index, (size_t)n_elite * 4);
    if (total_return) std::memcpy(total_return + (size_t)e * n_elite, r + rec.off_ret, (size_t)n_elite * 8);
    if (mean) std::memcpy(mean + (size_t)e * np, r + rec.off_mean, (size_t)np * 8);
    if (variance) std::memcpy(variance + (size_t)e * np, r + rec.off_var, (size_t)np * 8);
    if (avg_return) std::memcpy(avg_return + e, r, 8);
  }
  return MJPCX_OK;
}

int mjpcx_best_batched(mjpcx_ctx* c, int E, int ref_candidate, int32_t* index, double* best_return, double* ref_return, double* spline_values) {
  if (!c || !index) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (E < 1 || c->env_n < 1 || (long long)E * c->env_n != c->N)
    return fail(c, MJPCX_EINVAL, "mjpcx_best_batched: the last rollout was not a batched one of " + std::to_string(E) + " environments");
  // after a launch with a bound per environment (mjpcx_set_pruning_batched): the two rules of pruned_launch_valid and pruned_argmin_valid
  // below, applied to every environment with its own counters and final bound. Exact per environment, or MJPCX_ESTATE naming the environments
  const bool per_env_bounds = c->last_pruned_batched && (int)c->env_prune_final.size() == E;
  if (per_env_bounds) {
    std::string named;
    for (int e = 0; e < E; e++) if (c->env_prune_h[4 * (size_t)e + 2]) named += (named.empty() ? "" : ", ") + std::to_string(e);
    if (!named.empty())
      return fail(c, MJPCX_ESTATE, "pruned batched rollout: a step's cost was negative in environment(s) " + named +
                                       ", so partial returns are no lower bounds there (roll out again with pruning off)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int np = c->P * c->nu;
  const size_t rec = kBestHeader + (size_t)np * 8;
  HIPCHK(c, c->result.reserve(rec * E));
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((best_segmented_kernel<T>), dim3(E), dim3(256), 0, c->stream, (const double*)c->d_ret.p, (const int*)c->d_fail.p,
                       (const T*)c->d_nodes.p, c->N, c->env_n, np, ref_candidate, (unsigned char*)c->result.dev, (unsigned)rec);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (per_env_bounds) {
    std::string named;
    for (int e = 0; e < E; e++) {
      const BestRecord* r = (const BestRecord*)((const char*)c->result.p + rec * e);
      if (c->env_prune_h[4 * (size_t)e] > 0 && !(r->best_return <= c->env_prune_final[e])) named += (named.empty() ? "" : ", ") + std::to_string(e);
    }
    if (!named.empty())
      return fail(c, MJPCX_ESTATE, "pruned batched rollout: every stored return of environment(s) " + named +
                                       " is above its bound, so the initial bound was below every return there (roll out again with pruning off)");
  }
  for (int e = 0; e < E; e++) {
    const BestRecord* r = (const BestRecord*)((const char*)c->result.p + rec * e);
    index[e] = r->best_index;
    if (best_return) best_return[e] = r->best_return;
    if (ref_return) ref_return[e] = r->ref_return;
    if (spline_values) std::memcpy(spline_values + (size_t)e * np, r->spline, (size_t)np * 8);
  }
  return MJPCX_OK;
}

int mjpcx_mppi_update_batched(mjpcx_ctx* c, int E, const double* temperature, int ref_candidate, int32_t* index, double* best_return, double* ref_return,
                              double* weight_sum, double* effective_samples, int32_t* valid, double* mean, double* weights) {
  const std::string who = "mjpcx_mppi_update_batched: ";
  if (!c || !index || !temperature) return fail(c, MJPCX_EINVAL, who + "null argument");
  if (c->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, who + "not implemented on a context sharded with mjpcx_comm_init");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (E < 1 || c->env_n < 1 || (long long)E * c->env_n != c->N)
    return fail(c, MJPCX_EINVAL, who + "the last rollout was not a batched one of " + std::to_string(E) + " environments");
  const int n = c->env_n;
  for (int e = 0; e < E; e++)
    if (!std::isfinite(temperature[e]) || !(temperature[e] > 0))
      return fail(c, MJPCX_EINVAL, who + "the temperature of environment " + std::to_string(e) + " is " + std::to_string(temperature[e]) + "; it must be finite and > 0");
  if (ref_candidate < -1 || ref_candidate >= n)
    return fail(c, MJPCX_EINVAL, who + "ref_candidate = " + std::to_string(ref_candidate) + " outside -1.." + std::to_string(n - 1));
  if (c->last_pruned) return fail(c, MJPCX_ESTATE, who + kPrunedRanking);  // (stored partial returns are no returns: the rule of mjpcx_ce_update_batched)
  HIPCHK(c, hipSetDevice(c->device));
  const int np = c->P * c->nu;
  // the mapped block: E records, the E temperatures (the host writes them, mppi_weights_kernel reads them), then the E x n weights if asked for
  const size_t rec = kMppiHeader + (size_t)np * 8, off_temp = rec * E, off_w = off_temp + (size_t)E * 8;
  static_assert(offsetof(MppiRecord, mean) == kMppiHeader, "the record of mppi_weights_kernel");
  HIPCHK(c, c->result.reserve(off_w + (weights ? (size_t)E * n * 8 : 0)));
  HIPCHK(c, c->d_mppi.reserve((size_t)E * (n + 1) * 8));
  std::memcpy((char*)c->result.p + off_temp, temperature, (size_t)E * 8);
  // (with the timer on this call is one of its launches: its first kernel, the weights, is what mjpcx_timing_read_main singles out)
  hipEvent_t e1 = nullptr;
  int rc = begin_rollout_timing(c, &e1);
  if (rc != MJPCX_OK) return rc;
  hipLaunchKernelGGL(mppi_weights_kernel, dim3(E), dim3(256), 0, c->stream, (const double*)c->d_ret.p, (const double*)((char*)c->result.dev + off_temp), n,
                     ref_candidate, (double*)c->d_mppi.p, (unsigned char*)c->result.dev, (unsigned)rec,
                     weights ? (double*)((char*)c->result.dev + off_w) : (double*)nullptr);
  HIPCHK(c, hipGetLastError());
  if (c->timing && c->cur_main) { HIPCHK(c, hipEventRecord(c->cur_main, c->stream)); c->cur_main = nullptr; }
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((mppi_mean_kernel<T>), dim3(np, E), dim3(256), 0, c->stream, (const T*)c->d_nodes.p, (const double*)c->d_mppi.p, c->N, n, ref_candidate,
                       (unsigned char*)c->result.dev, (unsigned)rec);
  });
  HIPCHK(c, hipGetLastError());
  if (c->timing) HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int e = 0; e < E; e++) {
    const MppiRecord* r = (const MppiRecord*)((const char*)c->result.p + rec * e);
    index[e] = r->best_index;
    if (best_return) best_return[e] = r->best_return;
    if (ref_return) ref_return[e] = r->ref_return;
    if (weight_sum) weight_sum[e] = r->weight_sum;
    if (effective_samples) effective_samples[e] = r->effective_samples;
    if (valid) valid[e] = r->valid;
    if (mean) std::memcpy(mean + (size_t)e * np, r->mean, (size_t)np * 8);
  }
  if (weights) std::memcpy(weights, (const char*)c->result.p + off_w, (size_t)E * n * 8);
  return MJPCX_OK;
}

int mjpcx_rollout_noise_ensemble(mjpcx_ctx* c, int M, int n, int H, int P, int interp, const double* node_times, const double* nominal,
                                 const mjpcx_noise_spec* ns) {
  if (!c || !node_times) return fail(c, MJPCX_EINVAL, "null argument");
  if (M < 1) return fail(c, MJPCX_EINVAL, "mjpcx_rollout_noise_ensemble: the number of hypotheses must be >= 1");
  if (P < 1) return check_rollout_args(c, n, H, P, interp, node_times);
  // the one row of node times and the one nominal, as every hypothesis's row of the batched launch
  const size_t np = (size_t)P * c->nu;
  std::vector<double> times((size_t)M * P), nom;
  for (int h = 0; h < M; h++) std::memcpy(times.data() + (size_t)h * P, node_times, (size_t)P * 8);
  int rc = check_batched_args(c, M, n, H, P, interp, times.data());
  if (rc != MJPCX_OK) return rc;
  if (!nominal || !ns) return fail(c, MJPCX_EINVAL, "null argument");
  if (ns->mode != MJPCX_NOISE_SAMPLING && ns->mode != MJPCX_NOISE_CROSS_ENTROPY) return fail(c, MJPCX_EINVAL, "unknown noise mode");
  nom.resize((size_t)M * np);
  for (int h = 0; h < M; h++) std::memcpy(nom.data() + (size_t)h * np, nominal, np * 8);
  RolloutRequest r{M * n, H, P, interp, times.data(), M};
  r.nominal = nom.data(); r.noise = ns;
  r.seed_shared = true;  // (and no prune_batched: the score needs every return, so mjpcx_set_pruning_batched is ignored)
  return rollout(c, r);
}

int mjpcx_ensemble_best(mjpcx_ctx* c, int M, int tail, int ref_candidate, int32_t* index, double* best_score, double* ref_score,
                        double* member_returns, double* spline_values, double* scores) {
  const std::string who = "mjpcx_ensemble_best: ";
  if (!c || !index) return fail(c, MJPCX_EINVAL, who + "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (M > MJPCX_MAX_HYPOTHESES) return fail(c, MJPCX_EUNSUPPORTED, who + std::to_string(M) + " hypotheses; at most " + std::to_string(MJPCX_MAX_HYPOTHESES));
  if (M < 1 || c->env_n < 1 || (long long)M * c->env_n != c->N)
    return fail(c, MJPCX_EINVAL, who + "the last rollout was not a batched one of " + std::to_string(M) + " environments");
  const int n = c->env_n;
  if (tail < 1 || tail > M) return fail(c, MJPCX_EINVAL, who + "tail = " + std::to_string(tail) + " outside 1.." + std::to_string(M));
  if (ref_candidate < -1 || ref_candidate >= n)
    return fail(c, MJPCX_EINVAL, who + "ref_candidate = " + std::to_string(ref_candidate) + " outside -1.." + std::to_string(n - 1));
  if (c->last_pruned) return fail(c, MJPCX_ESTATE, who + kPrunedRanking);  // (stored partial returns are no returns: the rule of mjpcx_ce_update_batched)
  static_assert(kEnsembleMaxHypotheses == MJPCX_MAX_HYPOTHESES && offsetof(EnsembleRecord, rest) == kEnsembleHeader, "the record of ensemble_best_kernel");
  HIPCHK(c, hipSetDevice(c->device));
  const int np = c->P * c->nu;
  HIPCHK(c, c->result.reserve(kEnsembleHeader + ((size_t)np + (scores ? n : 0)) * 8));
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((ensemble_best_kernel<T>), dim3(1), dim3(kEnsembleThreads), (size_t)tail * kEnsembleThreads * 8, c->stream, (const double*)c->d_ret.p,
                       (const T*)c->d_nodes.p, n, M, tail, np, ref_candidate, scores ? 1 : 0, (unsigned char*)c->result.dev);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const EnsembleRecord* r = (const EnsembleRecord*)c->result.p;
  *index = r->best_index;
  if (best_score) *best_score = r->best_score;
  if (ref_score) *ref_score = r->ref_score;
  if (member_returns) std::memcpy(member_returns, r->member, (size_t)M * 8);
  if (spline_values) std::memcpy(spline_values, r->rest, (size_t)np * 8);
  if (scores) std::memcpy(scores, r->rest + np, (size_t)n * 8);
  return MJPCX_OK;
}

int mjpcx_robust_step_batched(mjpcx_ctx* c, mjpcx_ctx* src, int E, int k, int R, int H, int interp, const double* node_times, double xfrc_std,
                              double xfrc_rate, uint64_t seed, int candidate_offset, int32_t* best, int32_t* candidate, double* candidate_return,
                              double* perturbed_score, int32_t* valid, double* spline_values) {
  const std::string who = "mjpcx_robust_step_batched: ";
  if (!c || !src || !node_times || !best) return fail(c, MJPCX_EINVAL, who + "null argument");
  if (src == c) return fail(c, MJPCX_EINVAL, who + "the source of the candidates must be another context (its rollout stays fetchable)");
  if (c->comm_world > 1 || src->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, who + "not implemented on a context sharded with mjpcx_comm_init");
  if (src->device != c->device || src->precision != c->precision || src->nq != c->nq || src->nv != c->nv || src->nu != c->nu)
    return fail(c, MJPCX_EINVAL, who + "the two contexts differ in device, precision or model dimensions");
  if (E < 1 || !src->have_rollout || src->env_n < 1 || (long long)E * src->env_n != src->N)
    return fail(c, MJPCX_EINVAL, who + "the source's last rollout was not a batched one of " + std::to_string(E) + " environments");
  if (src->last_pruned) return fail(c, MJPCX_ESTATE, who + kPrunedRanking);
  if (k < 1 || k > src->env_n || R < 1)
    return fail(c, MJPCX_EINVAL, who + "num_candidates = " + std::to_string(k) + " outside 1.." + std::to_string(src->env_n) + " or repetitions = " + std::to_string(R) + " < 1");
  if (!(xfrc_std >= 0) || !(xfrc_rate > 0)) return fail(c, MJPCX_EINVAL, who + "xfrc_std must be >= 0 and xfrc_rate > 0");
  const long long share = (long long)k * R;
  if (share > 0x7fffffffLL / 64) return fail(c, MJPCX_EINVAL, who + "too many perturbed rollouts");
  const int n_pad = (int)((share + 63) / 64 * 64), P = src->P, np = P * c->nu, n_src = src->env_n;
  int rc = check_batched_args(c, E, n_pad, H, P, interp, node_times);  // (set_states(E) on this context, the rows of node_times, the batch size)
  if (rc != MJPCX_OK) return rc;
  if ((long long)np * n_pad > 0x7fffffffLL) return fail(c, MJPCX_EINVAL, who + "too many perturbed rollouts");
  const int N = E * n_pad;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = reserve_rollout(c, N, H, P)) != MJPCX_OK) return rc;  // (before the first kernel writes d_nodes: do_rollout's own call then moves nothing)
  RobustRecord rec;
  rec.off_index = 8;
  rec.off_ret = (rec.off_index + (size_t)k * 4 + 7) & ~(size_t)7;
  rec.off_score = rec.off_ret + (size_t)k * 8;
  rec.off_valid = rec.off_score + (size_t)k * 8;
  rec.off_spline = (rec.off_valid + (size_t)k * 4 + 7) & ~(size_t)7;
  rec.bytes = rec.off_spline + (size_t)np * 8;
  HIPCHK(c, c->result.reserve(rec.bytes * E));
  EnvSort sort;
  HIPCHK(c, sort.reserve(c, n_src, E));
  // everything below is enqueued on this context's stream, behind what the source's stream holds now
  if (!c->source_done) HIPCHK(c, hipEventCreateWithFlags(&c->source_done, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->source_done, src->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->source_done, 0));
  const hipError_t le = sort.dispatch(c, [](auto t, auto in_lds) { return robust_select_kernel<decltype(t), decltype(in_lds)::value>; }, [&](auto kern, auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(kern, dim3(E), dim3(1024), sort.lds, c->stream, (const double*)src->d_ret.p, (const T*)src->d_nodes.p, src->N, n_src, sort.n2, np, k, R,
                       n_pad, sort.slabs(c), (T*)c->d_nodes.p, (unsigned char*)c->result.dev, rec);
  });
  HIPCHK(c, le);
  // local rollout j of environment e draws the stream (seed + e, candidate_offset + j): one launch of k x R rollouts per environment
  RolloutRequest noisy{N, H, P, interp, node_times, E};
  noisy.nodes_on_device = true;
  noisy.xfrc_std = xfrc_std; noisy.xfrc_rate = xfrc_rate; noisy.xfrc_seed = seed; noisy.xfrc_offset = candidate_offset;
  if ((rc = rollout(c, noisy)) != MJPCX_OK) return rc;
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((robust_score_kernel<T>), dim3(E), dim3(256), 0, c->stream, (const double*)c->d_ret.p, (const int*)c->d_fail.p,
                       (const T*)c->d_nodes.p, np, k, R, n_pad, (unsigned char*)c->result.dev, rec);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int e = 0; e < E; e++) {
    const char* r = (const char*)c->result.p + rec.bytes * e;
    std::memcpy(best + e, r, 4);
    if (candidate) std::memcpy(candidate + (size_t)e * k, r + rec.off_index, (size_t)k * 4);
    if (candidate_return) std::memcpy(candidate_return + (size_t)e * k, r + rec.off_ret, (size_t)k * 8);
    if (perturbed_score) std::memcpy(perturbed_score + (size_t)e * k, r + rec.off_score, (size_t)k * 8);
    if (valid) std::memcpy(valid + (size_t)e * k, r + rec.off_valid, (size_t)k * 4);
    if (spline_values) std::memcpy(spline_values + (size_t)e * np, r + rec.off_spline, (size_t)np * 8);
  }
  return MJPCX_OK;
}

// sample_gradient/planner.cc:290-400 (ResamplePolicy of the gradient candidates, AddNoiseToPolicy, Rollouts) for E environments
int mjpcx_rollout_sample_gradient_batched(mjpcx_ctx* c, int E, int n, int G, int H, int P, int interp, const double* node_times, const double* nominal,
                                          double noise_exploration, uint64_t seed, int iteration, const double* gradient_values,
                                          const double* gradient_times) {
  const std::string who = "mjpcx_rollout_sample_gradient_batched: ";
  int rc = check_batched_args(c, E, n, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!nominal) return fail(c, MJPCX_EINVAL, who + "null nominal_values");
  if (G < 0 || G > n - 1) return fail(c, MJPCX_EINVAL, who + "num_gradient = " + std::to_string(G) + " outside 0.." + std::to_string(n - 1));
  if (!(noise_exploration > 0)) return fail(c, MJPCX_EINVAL, who + "noise_exploration must be > 0");
  if ((gradient_values == nullptr) != (gradient_times == nullptr)) return fail(c, MJPCX_EINVAL, who + "gradient_values and gradient_times come together");
  auto& s = c->sg;
  const bool same = s.E == E && s.G == G && s.P == P, upload = G > 0 && gradient_values;
  if (G > 0 && !upload && !(same && s.candidates))
    return fail(c, MJPCX_EINVAL, who + "no gradient candidates on the device: no update with this num_envs, num_gradient and num_nodes has run");
  if (upload)
    for (int e = 0; e < E; e++)
      for (int p = 1; p < P; p++)
        if (!(gradient_times[(size_t)e * P + p] > gradient_times[(size_t)e * P + p - 1])) return fail(c, MJPCX_EINVAL, who + "gradient_times must be strictly increasing");
  const int nu = c->nu, np = P * nu, npairs = (np + 1) / 2;
  const long long per_env = ((long long)npairs * n + 255) / 256;
  if (per_env * E > 0x7fffffffLL || (long long)npairs * n > 0x7fffffffLL - 256) return fail(c, MJPCX_EINVAL, who + "too many candidates");  // (the kernel's int indices)
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = reserve_rollout(c, E * n, H, P)) != MJPCX_OK) return rc;  // (before the kernel writes d_nodes: do_rollout's own call then moves nothing)
  const size_t sE = E, o_gt = 2 * sE * np, o_gv = o_gt + sE * P;
  if (!same) {  // another shape: nothing of the old state carries over; the gradient starts from zero as after Planner::Reset
    HIPCHK(c, s.d_state.reserve((o_gv + sE * G * np) * 8));
    HIPCHK(c, hipMemsetAsync(s.d_state.p, 0, o_gt * 8, c->stream));
    s.E = E; s.G = G; s.P = P; s.candidates = false;
  }
  const size_t i_nom = sE * P, i_range = i_nom + sE * np, i_gt = i_range + 2 * (size_t)nu, i_gv = i_gt + sE * P;
  const size_t bytes = (upload ? i_gv + sE * G * np : i_gt) * 8;
  HIPCHK(c, s.h_in.wait());
  HIPCHK(c, s.h_in.reserve(bytes));
  HIPCHK(c, s.d_in.reserve(bytes));
  double* h = (double*)s.h_in.p;
  std::memcpy(h, node_times, sE * P * 8);
  std::memcpy(h + i_nom, nominal, sE * np * 8);
  std::memcpy(h + i_range, c->ctrlrange.data(), 2 * (size_t)nu * 8);
  if (upload) {
    std::memcpy(h + i_gt, gradient_times, sE * P * 8);
    std::memcpy(h + i_gv, gradient_values, sE * G * np * 8);
  }
  HIPCHK(c, hipMemcpyAsync(s.d_in.p, h, bytes, hipMemcpyHostToDevice, c->stream));
  const double* din = (const double*)s.d_in.p;
  const double* dst = (const double*)s.d_state.p;
  SgCandArgs a{};
  a.n = n; a.num_noisy = n - G; a.P = P; a.nu = nu; a.interp = interp; a.num_envs = E; a.blocks_per_env = (int)per_env;
  a.times = din; a.nominal = din + i_nom; a.range = din + i_range;
  a.grad_times = upload ? din + i_gt : dst + o_gt;
  a.grad_values = upload ? din + i_gv : dst + o_gv;
  a.noise_exploration = noise_exploration; a.seed = seed; a.iteration = (uint32_t)iteration;
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((sg_candidates_kernel<T>), dim3((unsigned)(per_env * E)), dim3(256), 0, c->stream, a, (T*)c->d_nodes.p);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, s.h_in.mark(c->stream));
  RolloutRequest r{E * n, H, P, interp, node_times, E};
  r.nodes_on_device = true;
  if ((rc = rollout(c, r)) != MJPCX_OK) return rc;
  s.serial = c->rollout_serial; s.n = n; s.seed = seed; s.iteration = (uint32_t)iteration;
  return MJPCX_OK;
}

// sample_gradient/planner.cc:168-264 (the sort, the winner, the improvement) and 401-493 (GradientCandidates) for E environments
int mjpcx_sample_gradient_update_batched(mjpcx_ctx* c, int E, int G, int flags, double filter, double max_step, double min_step, double noise_exploration,
                                         int32_t* index, int32_t* winner_type, double* best_return, double* nominal_return, double* improvement,
                                         double* spline_values, double* gradient) {
  const std::string who = "mjpcx_sample_gradient_update_batched: ";
  if (!c || !index) return fail(c, MJPCX_EINVAL, who + "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (c->last_pruned) return fail(c, MJPCX_ESTATE, who + kPrunedRanking);
  auto& s = c->sg;
  if (E < 1 || s.serial == 0 || s.serial != c->rollout_serial || c->env_n < 1 || (long long)E * c->env_n != c->N || s.E != E || s.G != G)
    return fail(c, MJPCX_EINVAL, who + "the last rollout was not a mjpcx_rollout_sample_gradient_batched of " + std::to_string(E) + " environments with num_gradient = " + std::to_string(G));
  if (flags & ~(MJPCX_SG_COMPUTE_WEIGHTS | MJPCX_SG_ZERO_GRADIENT)) return fail(c, MJPCX_EINVAL, who + "unknown flags");
  if (G > 0 && (!(max_step > 0) || !(min_step > 0) || !(noise_exploration > 0) || !std::isfinite(filter)))
    return fail(c, MJPCX_EINVAL, who + "max_step, min_step and noise_exploration must be > 0 and filter finite");
  const int n = c->env_n, nn = n - G, P = c->P, nu = c->nu, np = P * nu, npairs = (np + 1) / 2;
  const bool compute = G > 0 && (flags & MJPCX_SG_COMPUTE_WEIGHTS);
  if (G > 0 && !compute && !(s.weights_E == E && s.weights_n == nn))
    return fail(c, MJPCX_EINVAL, who + "no shaping weights for " + std::to_string(E) + " environments of " + std::to_string(nn) + " noisy candidates: pass MJPCX_SG_COMPUTE_WEIGHTS");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t sE = E;
  if (G > 0) {
    HIPCHK(c, s.d_weights.reserve(sE * nn * 8));
    if (s.steps_G != G || s.steps_max != max_step || s.steps_min != min_step || s.logs_n != nn) {  // LogScale (utilities.cc:819-826) and log(k + 1), on the host
      const size_t bytes = ((size_t)G + nn) * 8;
      HIPCHK(c, s.h_up.reserve(bytes));
      HIPCHK(c, s.d_up.reserve(bytes));
      double* h = (double*)s.h_up.p;
      const double step = (std::log(max_step) - std::log(min_step)) / (G > 1 ? G - 1 : 1);
      for (int i = 0; i < G; i++) h[i] = std::exp(std::log(min_step) + i * step);
      for (int k = 0; k < nn; k++) h[G + k] = std::log(k + 1);
      HIPCHK(c, hipMemcpyAsync(s.d_up.p, h, bytes, hipMemcpyHostToDevice, c->stream));
      s.steps_G = G; s.steps_max = max_step; s.steps_min = min_step; s.logs_n = nn;
    }
  }
  SgRecord rec;
  rec.off_spline = 32;
  rec.off_grad = rec.off_spline + (size_t)np * 8;
  rec.bytes = rec.off_grad + (size_t)np * 8;
  HIPCHK(c, c->result.reserve(rec.bytes * E));
  const int chunks = G > 0 ? (npairs + 3) / 4 : 1;
  EnvSort sort;
  HIPCHK(c, sort.reserve(c, n, E, chunks));
  const double* din = (const double*)s.d_in.p;
  double* dst = (double*)s.d_state.p;
  SgUpdateArgs a{};
  a.n = n; a.n2 = sort.n2; a.P = P; a.nu = nu; a.G = G; a.num_noisy = nn; a.flags = flags;
  a.filter = filter; a.noise_exploration = noise_exploration; a.f0 = std::log(0.5 * nn + 1.0);
  a.seed = s.seed; a.iteration = s.iteration;
  a.times = din; a.nominal = din + sE * P; a.range = din + sE * P + sE * np;
  a.steps = (const double*)s.d_up.p; a.logs = a.steps + G;
  a.gradient = dst; a.gradient_previous = dst + sE * np; a.weights = (double*)s.d_weights.p;
  a.grad_times = dst + 2 * sE * np; a.grad_values = a.grad_times + sE * P;
  const hipError_t le = sort.dispatch(c, [](auto t, auto in_lds) { return sg_update_kernel<decltype(t), decltype(in_lds)::value>; }, [&](auto kern, auto t) {
    hipLaunchKernelGGL(kern, dim3(E, chunks), dim3(1024), sort.lds, c->stream, (const double*)c->d_ret.p, (const decltype(t)*)c->d_nodes.p, a, sort.slabs(c),
                       (unsigned char*)c->result.dev, rec);
  });
  HIPCHK(c, le);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (G > 0) {
    s.candidates = true;
    if (compute) { s.weights_E = E; s.weights_n = nn; }
  }
  for (int e = 0; e < E; e++) {
    const char* r = (const char*)c->result.p + rec.bytes * e;
    std::memcpy(index + e, r, 4);
    if (winner_type) std::memcpy(winner_type + e, r + 4, 4);
    if (best_return) std::memcpy(best_return + e, r + 8, 8);
    if (nominal_return) std::memcpy(nominal_return + e, r + 16, 8);
    if (improvement) std::memcpy(improvement + e, r + 24, 8);
    if (spline_values) std::memcpy(spline_values + (size_t)e * np, r + rec.off_spline, (size_t)np * 8);
    if (gradient) std::memcpy(gradient + (size_t)e * np, r + rec.off_grad, (size_t)np * 8);
  }
  return MJPCX_OK;
}

// ---- CMA-ES for E environments (csrc/cma_update.h): the state, the candidates and their rollout, the update
static_assert(kCmaMaxParams == MJPCX_CMA_MAX_PARAMS && offsetof(CmaRecord, mean) == kCmaHeader, "the header documents the kernels' cap; the record of cma_rank_kernel");

// the two factorising kernels may take the packed triangle of d = MJPCX_CMA_MAX_PARAMS in dynamic LDS (64.5 KiB); asked for once per
// device, in mjpcx_cma_set_state_batched, which every update has behind it
static hipError_t cma_allow_lds() {
  static std::mutex mtx;
  static std::vector<int> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mtx);
  if (std::find(done.begin(), done.end(), dev) != done.end()) return hipSuccess;
  const int bytes = (int)cma_tri_bytes(MJPCX_CMA_MAX_PARAMS);
  e = hipFuncSetAttribute((const void*)cma_factor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)cma_advance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.push_back(dev);
  return e;
}

int mjpcx_cma_set_state_batched(mjpcx_ctx* c, int E, int d, const double* sigma, const double* C, const double* p_sigma, const double* p_c) {
  const std::string who = "mjpcx_cma_set_state_batched: ";
  if (!c || !sigma) return fail(c, MJPCX_EINVAL, who + "null argument");
  if (c->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, who + "not implemented on a context sharded with mjpcx_comm_init");
  if (E < 1 || d < 1 || d % c->nu != 0) return fail(c, MJPCX_EINVAL, who + "num_envs must be >= 1 and num_params a positive multiple of nu = " + std::to_string(c->nu));
  if (d > MJPCX_CMA_MAX_PARAMS)
    return fail(c, MJPCX_EUNSUPPORTED, who + std::to_string(d) + " parameters (num_nodes x nu); the dense covariance is kept for at most " +
                                           std::to_string(MJPCX_CMA_MAX_PARAMS) + " (fewer spline points, or a separable variant: not implemented)");
  const size_t sd = d, dd = sd * sd, stride = cma_state_stride(d);
  for (int e = 0; e < E; e++) {
    if (!std::isfinite(sigma[e]) || !(sigma[e] > 0))
      return fail(c, MJPCX_EINVAL, who + "sigma of environment " + std::to_string(e) + " is " + std::to_string(sigma[e]) + "; it must be finite and > 0");
    for (size_t j = 0; j < sd; j++)
      if ((p_sigma && !std::isfinite(p_sigma[e * sd + j])) || (p_c && !std::isfinite(p_c[e * sd + j])))
        return fail(c, MJPCX_EINVAL, who + "an evolution path of environment " + std::to_string(e) + " is not finite");
    if (C)
      for (size_t a = 0; a < sd; a++)
        for (size_t b = 0; b <= a; b++) {
          const double x = C[e * dd + a * sd + b], y = C[e * dd + b * sd + a];
          if (!std::isfinite(x) || x != y)
            return fail(c, MJPCX_EINVAL, who + "C of environment " + std::to_string(e) + " is not symmetric (or not finite) at [" + std::to_string(a) + "][" + std::to_string(b) + "]");
        }
  }
  HIPCHK(c, hipSetDevice(c->device));
  auto& s = c->cma;
  s.E = s.d = 0;  // (until the factorisation has succeeded)
  std::vector<double> img((size_t)E * stride, 0.0);
  for (int e = 0; e < E; e++) {
    double* st = img.data() + e * stride;
    st[0] = sigma[e];
    if (p_sigma) std::memcpy(st + 2, p_sigma + e * sd, sd * 8);
    if (p_c) std::memcpy(st + 2 + sd, p_c + e * sd, sd * 8);
    double* Ce = st + 2 + 2 * sd;
    if (C) std::memcpy(Ce, C + e * dd, dd * 8);
    else for (size_t a = 0; a < sd; a++) Ce[a * sd + a] = 1.0;
  }
  HIPCHK(c, s.d_state.reserve(img.size() * 8));
  HIPCHK(c, c->result.reserve((size_t)E * 4));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (a setup call: nothing in flight reads the old state afterwards)
  HIPCHK(c, hipMemcpy(s.d_state.p, img.data(), img.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(c, cma_allow_lds());
  hipLaunchKernelGGL(cma_factor_kernel, dim3(E), dim3(256), cma_tri_bytes(d), c->stream, (double*)s.d_state.p, d, (int*)c->result.dev);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int e = 0; e < E; e++)
    if (((const int*)c->result.p)[e])
      return fail(c, MJPCX_EINVAL, who + "C of environment " + std::to_string(e) + " is not positive definite (a pivot of its Cholesky factorisation is <= 0); no state is set");
  s.E = E; s.d = d;
  s.generation.assign(E, 0);
  return MJPCX_OK;
}

int mjpcx_cma_get_state_batched(mjpcx_ctx* c, int E, int d, double* sigma, int64_t* generation, double* C, double* A, double* p_sigma, double* p_c) {
  const std::string who = "mjpcx_cma_get_state_batched: ";
  if (!c) return MJPCX_EINVAL;
  auto& s = c->cma;
  if (s.E < 1 || s.E != E || s.d != d)
    return fail(c, MJPCX_ESTATE, who + "no state of " + std::to_string(E) + " environments x " + std::to_string(d) + " parameters is set (mjpcx_cma_set_state_batched)");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t sd = d, dd = sd * sd, stride = cma_state_stride(d);
  std::vector<double> img((size_t)E * stride);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(img.data(), s.d_state.p, img.size() * 8, hipMemcpyDeviceToHost));
  for (int e = 0; e < E; e++) {
    const double* st = img.data() + e * stride;
    if (sigma) sigma[e] = st[0];
    if (generation) generation[e] = s.generation[e];
    if (p_sigma) std::memcpy(p_sigma + e * sd, st + 2, sd * 8);
    if (p_c) std::memcpy(p_c + e * sd, st + 2 + sd, sd * 8);
    if (C) std::memcpy(C + e * dd, st + 2 + 2 * sd, dd * 8);
    if (A) std::memcpy(A + e * dd, st + 2 + 2 * sd + dd, dd * 8);
  }
  return MJPCX_OK;
}

int mjpcx_rollout_cma_batched(mjpcx_ctx* c, int E, int n, int H, int P, int interp, const double* node_times, const double* nominal, uint64_t seed,
                              int iteration) {
  const std::string who = "mjpcx_rollout_cma_batched: ";
  int rc = check_batched_args(c, E, n, H, P, interp, node_times);
  if (rc != MJPCX_OK) return rc;
  if (!nominal) return fail(c, MJPCX_EINVAL, who + "null nominal_values");
  auto& s = c->cma;
  const int nu = c->nu, d = P * nu;
  if (s.E != E || s.d != d)
    return fail(c, MJPCX_ESTATE, who + "no state of " + std::to_string(E) + " environments x " + std::to_string(d) + " parameters is set (mjpcx_cma_set_state_batched)");
  if ((long long)d * n * E > 0x7fffffffLL) return fail(c, MJPCX_EINVAL, who + "too many candidates");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = reserve_rollout(c, E * n, H, P)) != MJPCX_OK) return rc;  // (before the kernel writes d_nodes: do_rollout's own call then moves nothing)
  const size_t sE = E, i_range = sE * d, bytes = (i_range + 2 * (size_t)nu) * 8;
  HIPCHK(c, s.h_in.wait());
  HIPCHK(c, s.h_in.reserve(bytes));
  HIPCHK(c, s.d_in.reserve(bytes));
  double* h = (double*)s.h_in.p;
  std::memcpy(h, nominal, sE * d * 8);
  std::memcpy(h + i_range, c->ctrlrange.data(), 2 * (size_t)nu * 8);
  HIPCHK(c, hipMemcpyAsync(s.d_in.p, h, bytes, hipMemcpyHostToDevice, c->stream));
  CmaCandArgs a{};
  a.n = n; a.d = d; a.nu = nu; a.num_envs = E;
  a.nominal = (const double*)s.d_in.p; a.range = a.nominal + i_range; a.state = (const double*)s.d_state.p;
  a.seed = seed; a.iteration = (uint32_t)iteration;
  // (with the timer on the candidate kernel is the launch's first kernel: mjpcx_timing_read_main gives its time, mjpcx_timing_read the
  // candidates' and the rollout's together)
  RolloutRequest r{E * n, H, P, interp, node_times, E};
  r.nodes_on_device = true;
  if ((rc = begin_rollout_timing(c, &r.timing_e1)) != MJPCX_OK) return rc;
  r.timing_begun = true;
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((cma_candidates_kernel<T>), dim3(n / kCmaGroup, E), dim3(256), 0, c->stream, a, (T*)c->d_nodes.p);
  });
  HIPCHK(c, hipGetLastError());
  if (c->timing && c->cur_main) { HIPCHK(c, hipEventRecord(c->cur_main, c->stream)); c->cur_main = nullptr; }
  HIPCHK(c, s.h_in.mark(c->stream));
  if ((rc = rollout(c, r)) != MJPCX_OK) return rc;
  s.serial = c->rollout_serial; s.n = n; s.seed = seed; s.iteration = (uint32_t)iteration;
  return MJPCX_OK;
}

int mjpcx_cma_update_batched(mjpcx_ctx* c, int E, const mjpcx_cma_params* prm, int32_t* index, double* best_return, double* nominal_return, double* improvement,
                             int32_t* valid, int32_t* restarted, double* sigma, double* mean, int32_t* order) {
  const std::string who = "mjpcx_cma_update_batched: ";
  if (!c || !prm || !index || !prm->weights) return fail(c, MJPCX_EINVAL, who + "null argument");
  if (c->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, who + "not implemented on a context sharded with mjpcx_comm_init");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (c->last_pruned) return fail(c, MJPCX_ESTATE, who + kPrunedRanking);
  auto& s = c->cma;
  if (E < 1 || s.serial == 0 || s.serial != c->rollout_serial || c->env_n < 1 || (long long)E * c->env_n != c->N || s.E != E || s.d != c->P * c->nu)
    return fail(c, MJPCX_EINVAL, who + "the last rollout was not a mjpcx_rollout_cma_batched of " + std::to_string(E) + " environments");
  const int n = c->env_n, nu = c->nu, d = s.d, mu = prm->mu;
  if (mu < 1 || mu > n - 1) return fail(c, MJPCX_EINVAL, who + "mu = " + std::to_string(mu) + " outside 1.." + std::to_string(n - 1));
  const double consts[] = {prm->c_sigma, prm->d_sigma, prm->c_c, prm->c_one, prm->c_mu, prm->mu_eff, prm->chi, prm->sigma_min, prm->sigma_max, prm->pivot_floor};
  for (double x : consts)
    if (!std::isfinite(x)) return fail(c, MJPCX_EINVAL, who + "a constant is not finite");
  for (int i = 0; i < mu; i++)
    if (!std::isfinite(prm->weights[i]) || !(prm->weights[i] > 0)) return fail(c, MJPCX_EINVAL, who + "weight " + std::to_string(i) + " is not finite and > 0");
  if (!(prm->c_one >= 0) || !(prm->c_mu >= 0) || prm->c_one + prm->c_mu > 1) return fail(c, MJPCX_EINVAL, who + "c_one and c_mu must be >= 0 with c_one + c_mu <= 1");
  if (!(prm->c_sigma > 0) || prm->c_sigma > 1 || !(prm->c_c > 0) || prm->c_c > 1 || !(prm->d_sigma > 0) || !(prm->mu_eff > 0) || !(prm->chi > 0) ||
      !(prm->sigma_min > 0) || prm->sigma_max < prm->sigma_min || prm->pivot_floor < 0)
    return fail(c, MJPCX_EINVAL, who + "c_sigma and c_c must be in (0, 1], d_sigma, mu_eff, chi > 0, 0 < sigma_min <= sigma_max, pivot_floor >= 0");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t sE = E, sd = d, rec = kCmaHeader + sd * 8, off_den = rec * sE;
  HIPCHK(c, c->result.reserve(off_den + sE * 8));
  HIPCHK(c, s.d_y.reserve(sE * sd * mu * 8));
  HIPCHK(c, s.d_s.reserve(sE * sd * sd * 8));
  HIPCHK(c, s.d_zw.reserve(sE * sd * 8));
  HIPCHK(c, s.d_rank.reserve(sE * (1 + (size_t)mu) * 4));
  if (s.weights.size() != (size_t)mu || std::memcmp(s.weights.data(), prm->weights, (size_t)mu * 8) != 0) {
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (another set of weights: rare; nothing in flight may still read the old ones)
    s.weights.assign(prm->weights, prm->weights + mu);
    HIPCHK(c, s.d_w.reserve((size_t)mu * 8));
    HIPCHK(c, hipMemcpy(s.d_w.p, s.weights.data(), (size_t)mu * 8, hipMemcpyHostToDevice));
  }
  // h_sigma's normalisation, per environment: sqrt(1 - (1 - c_sigma)^(2 g)), g = generation + 1 (the device neither raises powers nor counts)
  double* den = (double*)((char*)c->result.p + off_den);
  for (int e = 0; e < E; e++) den[e] = std::sqrt(1.0 - std::pow(1.0 - prm->c_sigma, 2.0 * (double)(s.generation[e] + 1)));
  CmaUpdateArgs a{};
  a.n = n; a.d = d; a.nu = nu; a.mu = mu;
  a.nominal = (const double*)s.d_in.p; a.range = a.nominal + sE * sd; a.weights = (const double*)s.d_w.p;
  a.hs_den = (const double*)((char*)c->result.dev + off_den);
  a.state = (double*)s.d_state.p; a.y = (double*)s.d_y.p; a.zw = (double*)s.d_zw.p; a.s = (double*)s.d_s.p; a.rank = (const int*)s.d_rank.p;
  a.one_m_cs = 1.0 - prm->c_sigma; a.cs_root = std::sqrt((prm->c_sigma * (2.0 - prm->c_sigma)) * prm->mu_eff);
  a.one_m_cc = 1.0 - prm->c_c; a.cc_root = std::sqrt((prm->c_c * (2.0 - prm->c_c)) * prm->mu_eff);
  a.decay[1] = (1.0 - prm->c_one) - prm->c_mu;
  a.decay[0] = a.decay[1] + (prm->c_one * prm->c_c) * (2.0 - prm->c_c);
  a.c_one = prm->c_one; a.c_mu = prm->c_mu; a.cs_ds = prm->c_sigma / prm->d_sigma; a.chi = prm->chi;
  a.hs_rhs = (1.4 + 2.0 / (d + 1.0)) * prm->chi;
  a.sigma_min = prm->sigma_min; a.sigma_max = prm->sigma_max; a.pivot_floor = prm->pivot_floor;
  a.seed = s.seed; a.iteration = s.iteration;
  EnvSort sort;
  HIPCHK(c, sort.reserve(c, n, E));
  // (with the timer on this call is one of its launches: its first kernel, the ranking, is what mjpcx_timing_read_main singles out)
  hipEvent_t e1 = nullptr;
  int rc = begin_rollout_timing(c, &e1);
  if (rc != MJPCX_OK) return rc;
  const hipError_t le = sort.dispatch(c, [](auto, auto in_lds) { return cma_rank_kernel<decltype(in_lds)::value>; }, [&](auto kern, auto) {
    hipLaunchKernelGGL(kern, dim3(E), dim3(1024), sort.lds, c->stream, (const double*)c->d_ret.p, n, sort.n2, mu, sort.slabs(c), (int*)s.d_rank.p,
                       (unsigned char*)c->result.dev, (unsigned)rec);
  });
  HIPCHK(c, le);
  if (c->timing && c->cur_main) { HIPCHK(c, hipEventRecord(c->cur_main, c->stream)); c->cur_main = nullptr; }
  hipLaunchKernelGGL(cma_draw_kernel, dim3((mu + kCmaGroup - 1) / kCmaGroup, E), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(cma_sums_kernel, dim3(d, d + 1, E), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(cma_advance_kernel, dim3(E), dim3(256), cma_tri_bytes(d), c->stream, a, (unsigned char*)c->result.dev, (unsigned)rec);
  HIPCHK(c, hipGetLastError());
  if (order)
    for (int e = 0; e < E; e++)
      HIPCHK(c, hipMemcpyAsync(order + (size_t)e * mu, (const int*)s.d_rank.p + (size_t)e * (1 + mu) + 1, (size_t)mu * 4, hipMemcpyDeviceToHost, c->stream));
  if (c->timing) HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int e = 0; e < E; e++) {
    const CmaRecord* r = (const CmaRecord*)((const char*)c->result.p + rec * e);
    index[e] = r->index;
    if (best_return) best_return[e] = r->best_return;
    if (nominal_return) nominal_return[e] = r->nominal_return;
    if (improvement) improvement[e] = r->improvement;
    if (valid) valid[e] = r->valid;
    if (restarted) restarted[e] = r->restarted;
    if (sigma) sigma[e] = r->sigma;
    if (mean) std::memcpy(mean + (size_t)e * sd, r->mean, sd * 8);
    if (r->valid) s.generation[e]++;
  }
  return MJPCX_OK;
}

int mjpcx_sync(mjpcx_ctx* c) {
  if (!c) return MJPCX_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MJPCX_OK;
}

int mjpcx_get_returns(mjpcx_ctx* c, double* total_return, int32_t* failure) {
  if (!c) return MJPCX_EINVAL;
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  HIPCHK(c, hipSetDevice(c->device));
  if (total_return) HIPCHK(c, hipMemcpyAsync(total_return, c->d_ret.p, (size_t)c->N * 8, hipMemcpyDeviceToHost, c->stream));
  if (failure) HIPCHK(c, hipMemcpyAsync(failure, c->d_fail.p, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MJPCX_OK;
}

int mjpcx_get_return_at(mjpcx_ctx* c, int cand, double* total_return, int32_t* failure) {
  if (!c) return MJPCX_EINVAL;
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (cand < 0 || cand >= c->N) return fail(c, MJPCX_EINVAL, "candidate out of range");
  HIPCHK(c, hipSetDevice(c->device));
  if (total_return) HIPCHK(c, hipMemcpyAsync(total_return, (const double*)c->d_ret.p + cand, 8, hipMemcpyDeviceToHost, c->stream));
  if (failure) HIPCHK(c, hipMemcpyAsync(failure, (const int*)c->d_fail.p + cand, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MJPCX_OK;
}

// which candidates a pruned launch (mjpcx_set_pruning) retires, and when, depends on the order its wavefronts finish in: only the argmin is exact
static_assert(MJPCX_FAILURE_PRUNED == mjpcx::kQPruned, "the header documents the kernel's marker");
// The argmin of a pruned launch, before and after it is known. The counters and the final bound came back with the launch's hand-on count:
// no synchronisation here.
//   before: a negative step cost means the partial returns were no lower bounds.
//   after: the smallest STORED return r* (partial returns for the retired candidates) must be <= the final bound Bf = min(initial bound,
//   the returns completed inside the launch). Every retired candidate's return >= its partial > the bound at that time >= Bf, so r* <= Bf
//   says that r* belongs to a candidate that completed and that every retired candidate is strictly above it: the argmin is exact, ties
//   included. With +inf as the initial bound r* <= Bf always holds (r* is <= every completed return). With a caller's bound it fails exactly
//   when no stored return reaches down to the bound -- a wrong bound always shows, also when a candidate slipped past it at the last step.
static int pruned_launch_valid(mjpcx_ctx* c) {
  if (c->last_pruned && c->prune_h[2])
    return fail(c, MJPCX_ESTATE, "pruned rollout: a step's cost was negative, so partial returns are no lower bounds (roll out again with pruning off)");
  return MJPCX_OK;
}
static int pruned_argmin_valid(mjpcx_ctx* c, double best_return) {
  if (c->last_pruned && c->prune_h[0] > 0 && !(best_return <= c->prune_final))
    return fail(c, MJPCX_ESTATE, "pruned rollout: every stored return is above the bound, so the initial bound was below every return (roll out again with pruning off)");
  return MJPCX_OK;
}

int mjpcx_best(mjpcx_ctx* c, int ref_candidate, int32_t* index, double* best_return, double* ref_return,
               double* spline_values) {
  if (!c || !index) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (c->last_pruned_batched) return fail(c, MJPCX_ESTATE, kPrunedRanking);  // (bounds per environment: mjpcx_best_batched)
  int rc;
  if ((rc = pruned_launch_valid(c)) != MJPCX_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const int np = c->P * c->nu;
  HIPCHK(c, c->result.reserve(sizeof(BestRecord) + (size_t)np * 8));
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((best_kernel<T>), dim3(1), dim3(1024), 0, c->stream, (const double*)c->d_ret.p, (const int*)c->d_fail.p,
                       (const T*)c->d_nodes.p, c->N, np, ref_candidate, (BestRecord*)c->result.dev);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const BestRecord* r = (const BestRecord*)c->result.p;
  if ((rc = pruned_argmin_valid(c, r->best_return)) != MJPCX_OK) return rc;
  *index = r->best_index;
  if (best_return) *best_return = r->best_return;
  if (ref_return) *ref_return = r->ref_return;
  if (spline_values) std::memcpy(spline_values, r->spline, (size_t)np * 8);
  return MJPCX_OK;
}

int mjpcx_topk(mjpcx_ctx* c, int k, int32_t* index, double* total_return) {
  if (!c || !index) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (k < 1 || k > c->N) return fail(c, MJPCX_EINVAL, "k out of range");
  if ((c->last_pruned && k > c->last_prune_rank) || c->last_pruned_batched) return fail_ranking(c);  // (rank 1: only the argmin is exact)
  int rc;
  if ((rc = pruned_launch_valid(c)) != MJPCX_OK) return rc;  // (k = 1 is the argmin: mjpcx_best's checks)
  HIPCHK(c, hipSetDevice(c->device));
  int n2 = 1;
  while (n2 < c->N) n2 <<= 1;
  HIPCHK(c, c->d_sort.reserve((size_t)n2 * sizeof(RetIdx)));
  if (k == 1) {
    hipLaunchKernelGGL(argmin_kernel, dim3(1), dim3(1024), 0, c->stream, (const double*)c->d_ret.p, c->N, (RetIdx*)c->d_sort.p);
  } else {
    hipLaunchKernelGGL(sort_kernel, dim3(1), dim3(1024), 0, c->stream, (const double*)c->d_ret.p, c->N, n2, (RetIdx*)c->d_sort.p);
  }
  HIPCHK(c, hipGetLastError());
  std::vector<RetIdx> h(k);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->d_sort.p, (size_t)k * sizeof(RetIdx), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = pruned_argmin_valid(c, h[0].r)) != MJPCX_OK) return rc;
  for (int i = 0; i < k; i++) {
    index[i] = h[i].i;
    if (total_return) total_return[i] = h[i].r;
  }
  return MJPCX_OK;
}

int mjpcx_elite_moments(mjpcx_ctx* c, int n, const int32_t* candidates, const double* mean, double* out,
                        double* sum_return) {
  if (!c || !candidates || !out) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (n < 0) return fail(c, MJPCX_EINVAL, "negative count");
  for (int i = 0; i < n; i++)
    if (candidates[i] < 0 || candidates[i] >= c->N) return fail(c, MJPCX_EINVAL, "candidate out of range");
  // (after a plain launch in rank mode: at most K candidates, none of them retired -- what is not retired equals the unpruned launch's, and
  // the first K of the stored order, mjpcx_topk's, never are)
  if (c->last_pruned && (c->last_pruned_batched || c->last_prune_rank <= 1 || n > c->last_prune_rank)) return fail_ranking(c);
  int rc;
  if ((rc = pruned_launch_valid(c)) != MJPCX_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->last_pruned && n > 0) {
    std::vector<int> f(c->N);  // (one copy of the launch's failure words: a copy per candidate costs 10 us each, and a planner passes a tenth of the batch)
    HIPCHK(c, hipMemcpyAsync(f.data(), c->d_fail.p, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++)
      if (f[candidates[i]] & kQPruned) return fail(c, MJPCX_ESTATE, "candidate " + std::to_string(candidates[i]) + " was retired: it is not among the first " + std::to_string(c->last_prune_rank));
  }
  const int np = c->P * c->nu;
  // staging: [cand (n i32) | mean (np f64) | out (np+1 f64)]
  const size_t off_mean = (((size_t)n * 4) + 15) & ~(size_t)15;
  const size_t off_out = off_mean + (size_t)np * 8;
  const size_t bytes = off_out + (size_t)(np + 1) * 8;
  HIPCHK(c, c->d_stage.reserve(bytes));
  char* d = (char*)c->d_stage.p;
  if (n) HIPCHK(c, hipMemcpyAsync(d, candidates, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if (mean) HIPCHK(c, hipMemcpyAsync(d + off_mean, mean, (size_t)np * 8, hipMemcpyHostToDevice, c->stream));
  const double* dmean = mean ? (const double*)(d + off_mean) : nullptr;
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((elite_moments_kernel<T>), dim3(np + 1), dim3(256), 0, c->stream, (const T*)c->d_nodes.p, (const double*)c->d_ret.p,
                       (const int*)d, n, c->N, np, dmean, (double*)(d + off_out));
  });
  HIPCHK(c, hipGetLastError());
  std::vector<double> h(np + 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), d + off_out, (size_t)(np + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, h.data(), (size_t)np * 8);
  if (sum_return) *sum_return = h[np];
  return MJPCX_OK;
}

int mjpcx_fetch_trajectory(mjpcx_ctx* c, int cand, mjpcx_traj_view* out) {
  if (!c || !out) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (cand < 0 || cand >= c->N) return fail(c, MJPCX_EINVAL, "candidate out of range");
  if (out->horizon < c->H) return fail(c, MJPCX_EINVAL, "trajectory view too short");
  HIPCHK(c, hipSetDevice(c->device));
  const int H = c->H, ds = c->nq + c->nv + c->na, nu = c->nu, nr = c->nr, ntr3 = 3 * c->ntrace;
  const int row = ds + nu + 1 + nr + 1 + ntr3;
  const size_t total = (size_t)H * row;
  HIPCHK(c, c->d_stage.reserve((total + 2) * 8));
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 1024);
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((gather_traj_kernel<T>), dim3(blocks), dim3(256), 0, c->stream, (const T*)c->d_states.p, (const T*)c->d_actions.p,
                       (const T*)c->d_times.p, (const T*)c->d_residual.p, (const T*)c->d_costs.p, (const T*)c->d_trace.p, c->N, H, ds, nu, nr, ntr3, cand,
                       (double*)c->d_stage.p, c->traj_candidate_major ? 1 : 0);
  });
  HIPCHK(c, hipGetLastError());
  c->h_stage.resize(total);
  double ret = 0; int32_t fl = 0;
  HIPCHK(c, hipMemcpyAsync(c->h_stage.data(), c->d_stage.p, total * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&ret, (const double*)c->d_ret.p + cand, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&fl, (const int*)c->d_fail.p + cand, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double* s = c->h_stage.data();
  if (out->states) std::memcpy(out->states, s, sizeof(double) * H * ds);
  s += (size_t)H * ds;
  if (out->actions) std::memcpy(out->actions, s, sizeof(double) * H * nu);
  s += (size_t)H * nu;
  if (out->times) std::memcpy(out->times, s, sizeof(double) * H);
  s += H;
  if (out->residual) std::memcpy(out->residual, s, sizeof(double) * H * nr);
  s += (size_t)H * nr;
  if (out->costs) std::memcpy(out->costs, s, sizeof(double) * H);
  s += H;
  if (out->trace && ntr3) std::memcpy(out->trace, s, sizeof(double) * H * ntr3);
  out->horizon = H;
  out->total_return = ret;
  out->failure = fl;
  return MJPCX_OK;
}

int mjpcx_fetch_spline(mjpcx_ctx* c, int cand, double* node_values) {
  if (!c || !node_values) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (cand < 0 || cand >= c->N) return fail(c, MJPCX_EINVAL, "candidate out of range");
  HIPCHK(c, hipSetDevice(c->device));
  const int np = c->P * c->nu;
  HIPCHK(c, c->d_stage.reserve((size_t)np * 8));
  by_precision(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((gather_spline_kernel<T>), dim3((np + 63) / 64), dim3(64), 0, c->stream, (const T*)c->d_nodes.p, c->N, np, cand, (double*)c->d_stage.p);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(node_values, c->d_stage.p, (size_t)np * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MJPCX_OK;
}

int mjpcx_timing_reset(mjpcx_ctx* c) {
  if (!c) return MJPCX_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->events_used = 0;
  c->timing = true;
  return MJPCX_OK;
}

int mjpcx_timing_read(mjpcx_ctx* c, double* kernel_ms, int64_t* launches) {
  if (!c) return MJPCX_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double total = 0;
  for (size_t i = 0; i < c->events_used; i++) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->events[i].first, c->events[i].second));
    total += ms;
  }
  if (kernel_ms) *kernel_ms = total;
  if (launches) *launches = (int64_t)c->events_used;
  c->timing = false;
  return MJPCX_OK;
}

int mjpcx_timing_read_main(mjpcx_ctx* c, double* main_kernel_ms, int64_t* launches) {
  if (!c) return MJPCX_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double total = 0;
  for (size_t i = 0; i < c->events_used; i++) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->events[i].first, c->events_main[i]));
    total += ms;
  }
  if (main_kernel_ms) *main_kernel_ms = total;
  if (launches) *launches = (int64_t)c->events_used;
  return MJPCX_OK;
}

// rank mode (mjpcx_set_prune_rank): the bound is the K-th smallest completed return, which no caller can know ahead of the launch
static const char* const kRankInitialBound = "in rank mode (mjpcx_set_prune_rank > 1) the initial bound must be +inf: nobody can vouch for a K-th return";

int mjpcx_set_pruning(mjpcx_ctx* c, int enabled, double initial_bound) {
  if (!c) return MJPCX_EINVAL;
  if (enabled && !(initial_bound >= 0)) return fail(c, MJPCX_EINVAL, "the initial bound is a return: >= 0 (+inf for none)");
  if (enabled && c->prune_allowed && c->prune_rank > 1 && initial_bound < HUGE_VAL) return fail(c, MJPCX_EINVAL, kRankInitialBound);
  c->prune_on = enabled != 0 && c->prune_allowed;
  c->prune_initial = initial_bound;
  return MJPCX_OK;
}

int mjpcx_set_prune_rank(mjpcx_ctx* c, int rank) {
  if (!c) return MJPCX_EINVAL;
  if (rank < 1) return fail(c, MJPCX_EINVAL, "the rank is a count of candidates: >= 1");
  if (rank > 1) {
    bool vouched = c->prune_on && c->prune_initial < HUGE_VAL;
    for (double b : c->bprune_initial) vouched = vouched || b < HUGE_VAL;
    if (vouched) return fail(c, MJPCX_EINVAL, kRankInitialBound);
  }
  c->prune_rank = rank;
  return MJPCX_OK;
}

int mjpcx_rank_bound_batched(mjpcx_ctx* c, int num_envs, int rank, double* bound) {
  if (!c || !bound) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (num_envs < 1 || rank < 1 || c->N % num_envs != 0)
    return fail(c, MJPCX_EINVAL, "mjpcx_rank_bound_batched: rank < 1, or the last rollout's " + std::to_string(c->N) + " candidates are not " + std::to_string(num_envs) + " equal environments");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->result.reserve((size_t)num_envs * 8));
  hipLaunchKernelGGL(rank_bound_kernel, dim3(num_envs), dim3(kRankBoundThreads), 0, c->stream, (const double*)c->d_ret.p, (const int*)c->d_fail.p, c->N / num_envs, rank,
                     (unsigned long long*)c->result.dev, 8u);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(bound, c->result.p, (size_t)num_envs * 8);
  return MJPCX_OK;
}

int mjpcx_set_pruning_batched(mjpcx_ctx* c, int enabled, int num_envs, const double* initial_bound, const double* park_hint) {
  if (!c) return MJPCX_EINVAL;
  if (!enabled) { c->bprune_on = false; c->bprune_E = 0; c->bprune_initial.clear(); c->bprune_hint.clear(); return MJPCX_OK; }
  if (num_envs < 1) return fail(c, MJPCX_EINVAL, "mjpcx_set_pruning_batched: the number of environments must be >= 1");
  for (int e = 0; e < num_envs; e++) {
    if (initial_bound && !(initial_bound[e] >= 0)) return fail(c, MJPCX_EINVAL, "environment " + std::to_string(e) + ": the initial bound is a return: >= 0 (+inf for none)");
    if (park_hint && !(park_hint[e] >= 0)) return fail(c, MJPCX_EINVAL, "environment " + std::to_string(e) + ": the park hint is an estimate of a return: >= 0 (+inf for none)");
    if (initial_bound && c->prune_allowed && c->prune_rank > 1 && initial_bound[e] < HUGE_VAL) return fail(c, MJPCX_EINVAL, "environment " + std::to_string(e) + ": " + kRankInitialBound);
  }
  if (!c->prune_allowed) return MJPCX_OK;  // (MJPCX_PRUNE=0: the call does nothing)
  c->bprune_on = true; c->bprune_E = num_envs;
  c->bprune_initial.assign(num_envs, HUGE_VAL);
  c->bprune_hint.assign(num_envs, HUGE_VAL);
  if (initial_bound) std::copy(initial_bound, initial_bound + num_envs, c->bprune_initial.begin());
  if (park_hint && c->park_allowed) std::copy(park_hint, park_hint + num_envs, c->bprune_hint.begin());  // (MJPCX_PARK=0: the hints are ignored)
  return MJPCX_OK;
}

int mjpcx_prune_stats_batched(mjpcx_ctx* c, int num_envs, int64_t* prune, int64_t* park, double* final_bound) {
  if (!c || !prune || num_envs < 1) return MJPCX_EINVAL;
  const bool have = c->last_pruned_batched && (int)c->env_prune_final.size() == num_envs;
  if (c->last_pruned_batched && !have)
    return fail(c, MJPCX_EINVAL, "mjpcx_prune_stats_batched: the last rollout was a pruned one of " + std::to_string(c->env_prune_final.size()) + " environments");
  for (int k = 0; k < 4 * num_envs; k++) prune[k] = have ? c->env_prune_h[k] : 0;
  if (park) for (int k = 0; k < 3 * num_envs; k++) park[k] = have ? c->env_park_h[k] : 0;
  if (final_bound) for (int k = 0; k < num_envs; k++) final_bound[k] = have ? c->env_prune_final[k] : 0.0;
  return MJPCX_OK;
}

int mjpcx_set_park_hint(mjpcx_ctx* c, double hint) {
  if (!c) return MJPCX_EINVAL;
  if (!(hint >= 0)) return fail(c, MJPCX_EINVAL, "the park hint is an estimate of a return: >= 0 (+inf for none)");
  c->park_hint = c->park_allowed ? hint : HUGE_VAL;
  return MJPCX_OK;
}

int mjpcx_park_stats(mjpcx_ctx* c, int64_t* counts, double* resume_ms) {
  if (!c || !counts) return MJPCX_EINVAL;
  for (int k = 0; k < 3; k++) counts[k] = c->last_pruned ? c->park_h[k] : 0;
  if (resume_ms) *resume_ms = c->last_pruned ? c->park_resume_ms : 0.0;
  return MJPCX_OK;
}

int mjpcx_park_resumed(mjpcx_ctx* c, int32_t* index, int32_t* step, int cap) {
  if (!c || cap < 0 || (cap > 0 && (!index || !step))) return MJPCX_EINVAL;
  const int n = c->last_pruned ? (int)c->park_h[2] : 0;
  if (n == 0 || cap == 0) return n;
  const int m = std::min(n, cap);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->last_pruned_batched) {  // (a segment of env_n entries per environment; the indices in them are global)
    int got = 0;
    for (size_t e = 0; e < c->env_prune_final.size() && got < m; e++) {
      const int take = std::min((int)c->env_park_h[3 * e + 2], m - got);
      if (take > 0) HIPCHK(c, hipMemcpy(index + got, (const int*)c->d_resume.p + e * (size_t)c->env_n, (size_t)take * sizeof(int), hipMemcpyDeviceToHost));
      got += take;
    }
  } else {
    HIPCHK(c, hipMemcpy(index, c->d_resume.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
  }
  std::vector<double> rec(quad::kQParkRec);
  for (int i = 0; i < m; i++) {  // (a test's call: one small copy per resumed candidate)
    HIPCHK(c, hipMemcpy(rec.data(), (const double*)c->d_park_rec.p + (size_t)index[i] * quad::kQParkRec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    step[i] = (int32_t)rec[21];
  }
  return n;
}

int mjpcx_prune_stats(mjpcx_ctx* c, int64_t* out) {
  if (!c || !out) return MJPCX_EINVAL;
  for (int k = 0; k < 4; k++) out[k] = c->last_pruned ? c->prune_h[k] : 0;
  return MJPCX_OK;
}

int mjpcx_quad_stats(mjpcx_ctx* c, int32_t* handed_on) {
  if (!c || !handed_on) return MJPCX_EINVAL;
  for (int k = 0; k < 8; k++) handed_on[k] = 0;
  if (!c->quad_ok && !c->limb_ok) return MJPCX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(handed_on, c->d_qstats.p, 32, hipMemcpyDeviceToHost));
  return MJPCX_OK;
}

int64_t mjpcx_algorithmic_bytes(const mjpcx_ctx* c, int H, int P) {
  if (!c) return 0;
  const int64_t w = c->precision == 64 ? 8 : 4;
  const int64_t ds = c->nq + c->nv + c->na;
  return w * ((int64_t)H * (ds + c->nu + 1 + c->nr + 3 * c->ntrace + 1) + (int64_t)P * c->nu + P + 2);
}

int mjpcx_device_buffer(mjpcx_ctx* c, int which, void** ptr, size_t* bytes) {
  if (!c || !ptr) return MJPCX_EINVAL;
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (which == 0) { *ptr = c->d_ret.p; if (bytes) *bytes = (size_t)c->N * 8; }
  else if (which == 1) { *ptr = c->d_fail.p; if (bytes) *bytes = (size_t)c->N * 4; }
  else return fail(c, MJPCX_EINVAL, "unknown buffer");
  return MJPCX_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ iLQG entry points
// One host code path, as for the rollouts (do_rollout): every function below takes E, and E = 0 is the plain entry point -- one
// environment, the state of mjpcx_set_state, the plain kernel instantiations; E >= 1 is the batched one -- the states of mjpcx_set_states,
// the instantiations that select an environment.
namespace {
// One upload for an iLQG / Gradient entry point: host arrays -- fp64 converted to T, int32 as they are -- into the pinned block h_ilqg,
// each on a 16-byte boundary (whole groups of 4 elements), ONE asynchronous copy into d_ilqg, and the block marked. No sync: the block is
// rewritten only after the copy out of it has completed. dev[k]: array k on the device.
struct HostArray {
  const void* src; size_t n; bool ints;
  HostArray(const double* p, size_t n_) : src(p), n(n_), ints(false) {}
  HostArray(const int32_t* p, size_t n_) : src(p), n(n_), ints(true) {}
};
template <typename T>
int upload_arrays(mjpcx_ctx* c, std::initializer_list<HostArray> arrays, const T** dev) {
  auto room = [](const HostArray& a) { return ((a.n + 3) & ~(size_t)3) * (a.ints ? 4 : sizeof(T)); };
  size_t bytes = 0, off = 0;
  for (auto& a : arrays) bytes += room(a);
  HIPCHK(c, c->h_ilqg.wait());
  HIPCHK(c, c->h_ilqg.reserve(bytes));
  HIPCHK(c, c->d_ilqg.reserve(bytes));
  for (auto& a : arrays) {
    char* h = (char*)c->h_ilqg.p + off;
    if (a.ints) std::memcpy(h, a.src, a.n * 4);
    else for (size_t i = 0; i < a.n; i++) ((T*)h)[i] = (T)((const double*)a.src)[i];
    *dev++ = (const T*)((char*)c->d_ilqg.p + off);
    off += room(a);
  }
  HIPCHK(c, hipMemcpyAsync(c->d_ilqg.p, c->h_ilqg.p, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, c->h_ilqg.mark(c->stream));
  return MJPCX_OK;
}
// the tail of a call that returns arrays: the requested ones (dst != nullptr) copied to the host, then the call's ONE sync
struct Download { void* dst; const void* src; size_t bytes; };
int download(mjpcx_ctx* c, const Download* list, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (list[k].dst) HIPCHK(c, hipMemcpyAsync(list[k].dst, list[k].src, list[k].bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MJPCX_OK;
}
int download(mjpcx_ctx* c, std::initializer_list<Download> list) { return download(c, list.begin(), list.size()); }

// The plan records alone, for the entry points that bring no spline: state, clock, mocap pose and task blob of the one environment
// (E = 0) or of each of E, `stride` bytes apart (stage_plan_inputs). The caller marks slot->host behind the last kernel that reads them.
struct PlanRecords { mjpcx_ctx::Slot* slot; const void* blob; unsigned stride; };
template <typename T>
int stage_records(mjpcx_ctx* c, int E, PlanRecords* r) {
  const T *times, *nominal;
  const double* variance;
  return stage_plan_inputs<T>(c, 0, E, nullptr, nullptr, nullptr, false, &times, &nominal, &variance, &r->slot, &r->blob, &r->stride);
}
WaveTask wave_task(const mjpcx_ctx* c, const void* d_blob) {
  WaveTask wt = c->wh.t;
  wt.blob = (const double*)d_blob;
  wt.stamps = nullptr;
  wt.stamp_step = 0;
  return wt;
}
// tree: the iLQG kernels of a model wave_tree.h covers run its forward pass (P = the scratch elements kept in the node-time slot)
size_t wave_lds_bytes(const mjpcx_ctx* c, int P, bool tree = false) {
  const WaveModel& wm = c->wh.m;
  if (tree)
    return (8 * w64::wave_lds_elems_tree(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, c->wh.t.nr, c->wh.t.nterm, P, false, w64::kTreeMaxSimpleBig,
                                         w64::kTreeMaxConeBig) + 15) & ~(size_t)15;
  return (8 * w64::wave_lds_elems(wm.nq, wm.nv, wm.nu, wm.nbody, wm.njnt, wm.nsite, c->wh.t.nr, c->wh.t.nterm, P, wm.cone) + 15) & ~(size_t)15;
}

// mjpcx_rollout_feedback (E = 0: n candidates) and mjpcx_rollout_feedback_batched (E >= 1: n per environment, the five nominal arrays
// E x Tn steps) after validation: the plan records, the six policy arrays in one upload, the family's kernel. No sync on the lane family.
template <typename T>
int do_feedback(mjpcx_ctx* c, int E, int n, int H, int mode, int representation, int use_state, int Tn, const double* times,
                const double* states, const double* actions, const double* gains, const double* improvement, const double* alpha) {
  int rc;
  const int N = (E > 0 ? E : 1) * n, env_n = E > 0 ? n : 0;
  if ((rc = reserve_rollout(c, N, H, 1)) != MJPCX_OK) return rc;
  const size_t ds = c->nq + c->nv, ndx = 2 * (size_t)c->nv, nu = c->nu, sET = (size_t)(E > 0 ? E : 1) * Tn;
  PlanRecords rec;
  if ((rc = stage_records<T>(c, E, &rec)) != MJPCX_OK) return rc;
  if (E == 0) rec.stride = 0;
  const T* d[6];
  if ((rc = upload_arrays<T>(c, {{times, sET}, {states, sET * ds}, {actions, sET * nu}, {gains, sET * nu * ndx}, {improvement, sET * nu},
                                 {alpha, (size_t)N}}, d)) != MJPCX_OK) return rc;
  RolloutArgs<T> a{};
  a.N = N; a.H = H; a.P = c->wave ? 1 : 0; a.interp = 0; a.nodes = (T*)c->d_nodes.p; a.noise.mode = -1;
  a.states = (T*)c->d_states.p; a.actions = (T*)c->d_actions.p; a.times = (T*)c->d_times.p;
  a.residual = (T*)c->d_residual.p; a.costs = (T*)c->d_costs.p; a.trace = (T*)c->d_trace.p;
  a.total_return = (double*)c->d_ret.p; a.failure = (int*)c->d_fail.p;
  if (!c->wave) {
    FeedbackArgs<T> fb{d[0], d[1], d[2], d[3], d[4], d[5], Tn, mode, representation, use_state};
    if (E > 0) { fb.env_n = n; fb.env_waves = (n + 63) / 64; fb.env_stride = rec.stride; fb.init = (const LaneInit<T>*)rec.blob; }
    hipError_t le;
    if constexpr (sizeof(T) == 8) le = c->kernel->feedback64(c->hm64, c->ht64, a, fb, c->stream);
    else { convert_task(c->ht32, c->ht64); le = c->kernel->feedback32(c->hm32, c->ht32, a, fb, c->stream); }
    if (le != hipSuccess) return fail(c, MJPCX_EDEVICE, std::string("feedback kernel launch: ") + hipGetErrorString(le));
  } else if constexpr (sizeof(T) == 8) {
    const WaveTask wt = wave_task(c, rec.blob);
    w64::FeedbackWaveArgs fb{d[0], d[1], d[2], d[3], d[4], d[5], Tn, mode, representation, use_state, 0, env_n, rec.stride};
    // a model of the quad kernel's class: the iLQG rollouts are one or ten candidates of pure per-step latency, and the quad form's step is the
    // shortest (one candidate per wavefront; MJPCX_NO_QUAD_FEEDBACK=1 keeps the wavefront-per-candidate kernel for A/B runs). Candidates it
    // hands on -- of whichever environments -- are rolled out by that kernel afterwards, as for the sampling rollouts.
    bool handed_on = true;
    if (c->quad_ok && !c->no_quad_feedback && c->wh.m.integrator == MJPCX_INT_EULER) {
      quad::QArgs q{};
      q.N = N; q.H = H; q.P = 1; q.noise_mode = -1; q.nodes = (double*)c->d_nodes.p;
      q.states = a.states; q.actions = a.actions; q.times = a.times; q.residual = a.residual; q.costs = a.costs; q.trace = a.trace;
      q.total_return = a.total_return; q.failure = a.failure; q.con_cap = c->quad_con_cap; q.cpw = 1;
      q.env_n = env_n; q.env_stride = rec.stride;
      const quad::QBlob bo{wt.off_time, wt.off_mocap, wt.off_weight, wt.off_normp, wt.off_normq, wt.off_param, wt.off_risk, wt.off_rreal, wt.off_rint};
      const quad::QFeedback qf{d[0], d[1], d[2], d[3], d[4], d[5], Tn, mode, representation, use_state};
      HIPCHK(c, hipMemsetAsync(c->d_qstats.p, 0, 32, c->stream));
      HIPCHK(c, quad::launch_feedback_quad(c->d_qmodel.p, c->d_qtab.p, wt.blob, bo, q, qf, (int*)c->d_qstats.p, c->stream));
      if (!c->h_qstats && hipHostMalloc(&c->h_qstats, 64, hipHostMallocDefault) != hipSuccess) c->h_qstats = nullptr;
      if (c->h_qstats) {  // (the one sync of the call: the hand-on count)
        HIPCHK(c, hipMemcpyAsync(c->h_qstats, c->d_qstats.p, 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        handed_on = static_cast<const int*>(c->h_qstats)[0] != 0;
      }
      fb.only_flagged = 1;
    }
    if (handed_on) {
      const bool tree = c->wh.tree_ok && !c->no_tree;
      const int Ppolicy = tree ? (int)(ndx + 2 * ds) : (int)((ndx + 2 * ds + nu - 1) / nu + 1);
      HIPCHK(c, launch_feedback_wave(c->wh.m, wt, a, fb, N, wave_lds_bytes(c, Ppolicy, tree), tree, c->wh.m.integrator == MJPCX_INT_RK4,
                                     c->wh.registered == 0 ? c->wh.dev_image : nullptr, c->wh.blob_bytes, c->stream));
    }
  } else {
    return fail(c, MJPCX_EUNSUPPORTED, "the iLQG kernels of the wavefront-per-candidate family are fp64 only");
  }
  HIPCHK(c, rec.slot->host.mark(c->stream));
  c->N = N; c->H = H; c->P = a.P;
  c->env_n = env_n;
  c->last_pruned = false; c->last_pruned_batched = false;
  c->have_rollout = true;
  c->rollout_serial++;
  c->traj_candidate_major = c->wave;
  return MJPCX_OK;
}
// the checks mjpcx_rollout_feedback and mjpcx_rollout_feedback_batched share (`who`: the prefix of the batched call's messages)
int check_feedback_args(mjpcx_ctx* c, const std::string& who, int H, int Tn, int mode, int representation) {
  if (mode == 0 && H > Tn) return fail(c, MJPCX_EINVAL, who + "index policy needs a nominal trajectory at least as long as the horizon");
  if (mode != 0 && mode != 1) return fail(c, MJPCX_EINVAL, who + "unknown feedback policy mode");
  if (mode == 1 && (representation < 0 || representation > 2))
    return fail(c, MJPCX_EINVAL, who + "iLQG policy representation must be 0 (zero-order), 1 (linear) or 2 (cubic)");
  if (c->wave && c->precision != 64) return fail(c, MJPCX_EUNSUPPORTED, "the iLQG kernels of the wavefront-per-candidate family are fp64 only");
  const size_t shmem = (size_t)Tn * (1 + 2 * c->nv + 2 * c->nu + c->nu * 2 * c->nv) * esize(c);
  if (!c->wave && shmem > 120 * 1024) return fail(c, MJPCX_EUNSUPPORTED, "nominal trajectory too large for the LDS stage");
  return MJPCX_OK;
}

// ModelDerivatives::Compute at `ne` steps of the one environment (E = 0) or of each of E, enqueued on the context's stream: the finite
// differences -- every environment's with its own plan record -- and their assembly into A, B, C, D at those steps. The workspace is
// carved by carve_fd out of a buffer of the caller's: next | tangent (wave family) | sensor | A | B | C | D.
struct FdCarve { size_t next, tan, sens, A, B, C, D; };
template <typename T, class Carve>
FdCarve carve_fd(const mjpcx_ctx* c, size_t rows, Carve&& carve) {
  const size_t ds = c->nq + c->nv, ndx = 2 * (size_t)c->nv, nu = c->nu, nr = c->nr, nc = 1 + 2 * (ndx + nu);
  FdCarve w;
  w.next = carve(rows * nc * (c->wave ? ds : ndx) * sizeof(T)); w.tan = carve(c->wave ? rows * nc * ndx * 8 : 0); w.sens = carve(rows * nc * nr * sizeof(T));
  w.A = carve(rows * ndx * ndx * 8); w.B = carve(rows * ndx * nu * 8); w.C = carve(rows * nr * ndx * 8); w.D = carve(rows * nr * nu * 8);
  return w;
}
template <typename T>
struct FdIn {
  const T *times, *states, *actions;   // [rows], [rows][nq + nv], [rows][nu], environment-major
  const T* range; const int* limited;  // ctrlrange [2 nu], ctrllimited [nu]
};
template <typename T>
int enqueue_fd(mjpcx_ctx* c, int E, int ne, double eps, int centered, const PlanRecords& rec, const FdIn<T>& in, char* base, const FdCarve& w) {
  const size_t ndx = 2 * (size_t)c->nv, nu = c->nu, nr = c->nr, nc = 1 + 2 * (ndx + nu), rows = (size_t)(E > 0 ? E : 1) * ne;
  T *next = (T*)(base + w.next), *sens = (T*)(base + w.sens);
  const T* fd_next = next;
  if (c->wave) {
    if constexpr (sizeof(T) == 8) {
      w64::FdWaveArgs fa{in.times, in.states, in.actions, (int)rows, (int)nc, eps, next, sens, E > 0 ? ne : 0, E > 0 ? rec.stride : 0};
      const bool tree = c->wh.tree_ok && !c->no_tree;
      HIPCHK(c, launch_transition_fd_wave(c->wh.m, wave_task(c, rec.blob), fa, (unsigned)(rows * nc), wave_lds_bytes(c, 1, tree), tree,
                                          c->wh.m.integrator == MJPCX_INT_RK4, c->stream));
      HIPCHK(c, launch_fd_tangent(c->wh.m, next, (double*)(base + w.tan), (int)rows, (int)nc, c->stream));
      fd_next = (const T*)(base + w.tan);
    } else {
      return fail(c, MJPCX_EUNSUPPORTED, "the iLQG kernels of the wavefront-per-candidate family are fp64 only");
    }
  } else {
    FdArgs<T> fa{in.times, in.states, in.actions, ne, (T)eps, next, sens};
    if (E > 0) { fa.num_envs = E; fa.env_items = (int)(((size_t)ne * nc + 63) / 64 * 64); fa.env_stride = rec.stride; fa.init = (const LaneInit<T>*)rec.blob; }
    hipError_t le;
    if constexpr (sizeof(T) == 8) le = c->kernel->fd64(c->hm64, c->ht64, fa, c->stream);
    else { convert_task(c->ht32, c->ht64); le = c->kernel->fd32(c->hm32, c->ht32, fa, c->stream); }
    if (le != hipSuccess) return fail(c, MJPCX_EDEVICE, std::string("fd kernel launch: ") + hipGetErrorString(le));
  }
  const size_t items = rows * (ndx + nr) * (ndx + nu);
  hipLaunchKernelGGL((fd_assemble_kernel<T>), dim3((unsigned)std::min<size_t>((items + 255) / 256, 1024)), dim3(256), 0, c->stream, fd_next, (const T*)sens,
                     in.actions, in.range, in.limited, (int)rows, (int)ndx, (int)nu, (int)nr, (T)eps, centered, (double*)(base + w.A),
                     (double*)(base + w.B), (double*)(base + w.C), (double*)(base + w.D));
  HIPCHK(c, hipGetLastError());
  return MJPCX_OK;
}

// the context's current cost specification as the cost-derivative kernel takes it
int make_cost_spec(mjpcx_ctx* c, CostSpec* out) {
  if (c->nterm > 32) return fail(c, MJPCX_EUNSUPPORTED, "more than 32 cost terms");
  CostSpec& cs = *out;
  cs.num_term = c->nterm; cs.num_residual = c->nr; cs.risk = c->wave ? c->wh.risk : c->ht64.risk;
  for (int k = 0; k < c->nterm; k++) {
    if (c->dim_norm_residual[k] > 32) return fail(c, MJPCX_EUNSUPPORTED, "cost term wider than 32 residuals");
    cs.dim[k] = c->dim_norm_residual[k];
    if (c->wave) { cs.norm[k] = c->wh.norm_types[k]; cs.weight[k] = c->wh.weight[k]; cs.p[k] = c->wh.norm_p[k]; cs.q[k] = c->wh.norm_q[k]; }
    else { cs.norm[k] = c->ht64.norm[k]; cs.weight[k] = c->ht64.weight[k]; cs.p[k] = c->ht64.norm_p[k]; cs.q[k] = c->ht64.norm_q[k]; }
  }
  return MJPCX_OK;
}
// backward_pass_kernel / backward_pass_batched_kernel: the m x m factorisation / box-QP of a step is unrolled to 12 or 16 columns at
// compile time (the A1 has 12 controls); dynamic LDS: the carve of backward_sweep (ilqg_dense.h), with slack
template <class Kernel, class Args>
int launch_backward(mjpcx_ctx* c, Kernel kernel12, Kernel kernel16, int n, int m, unsigned grid, const Args& args) {
  const int NP = (n + 15) & ~15;
  const size_t lds = (size_t)(5 * NP * NP + 3 * NP + 6 * NP * 16 + 5 * 256 + 16 * 23 + 16 * 13) * 8;
  Kernel kernel = m <= 12 ? kernel12 : kernel16;
  HIPCHK(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBackwardThreads), lds, c->stream, args);
  HIPCHK(c, hipGetLastError());
  return MJPCX_OK;
}
}  // namespace

extern "C" {

int mjpcx_rollout_feedback(mjpcx_ctx* c, int N, int H, int mode, int representation, int use_state, int Tn,
                           const double* times, const double* states, const double* actions, const double* gains,
                           const double* improvement, const double* alpha) {
  if (!c || !times || !states || !actions || !gains || !improvement || !alpha) return fail(c, MJPCX_EINVAL, "null argument");
  if (N < 1 || H < 1 || Tn < 1) return fail(c, MJPCX_EINVAL, "N, H and Tn must be >= 1");
  int rc;
  if ((rc = check_feedback_args(c, "", H, Tn, mode, representation)) != MJPCX_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return c->precision == 64 ? do_feedback<double>(c, 0, N, H, mode, representation, use_state, Tn, times, states, actions, gains, improvement, alpha)
                            : do_feedback<float>(c, 0, N, H, mode, representation, use_state, Tn, times, states, actions, gains, improvement, alpha);
}

int mjpcx_rollout_feedback_batched(mjpcx_ctx* c, int E, int n, int H, int mode, int representation, int use_state, int Tn, const double* times,
                                   const double* states, const double* actions, const double* gains, const double* improvement,
                                   const double* alpha) {
  const std::string who = "mjpcx_rollout_feedback_batched: ";
  if (!c || !times || !states || !actions || !gains || !improvement || !alpha) return fail(c, MJPCX_EINVAL, who + "null argument");
  if (c->em.E > 0) return fail(c, MJPCX_EUNSUPPORTED, who + "the derivative chain on a model per environment (mjpcx_set_models_batched) is not implemented: clear the models, or plan these environments on contexts of their own");
  if (E < 1) return fail(c, MJPCX_EINVAL, who + "the number of environments must be >= 1");
  if (n < 1 || H < 1 || Tn < 1) return fail(c, MJPCX_EINVAL, who + "n_per_env, H and Tn must be >= 1");
  if ((long long)E * n > 0x7fffffffLL / 64 || (long long)E * Tn * (1 + 2 * c->nv * c->nu) > 0x7fffffffLL / 64)
    return fail(c, MJPCX_EINVAL, who + "too many candidates or steps");
  int rc;
  if ((rc = check_feedback_args(c, who, H, Tn, mode, representation)) != MJPCX_OK) return rc;
  if (c->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, who + "not implemented on a context sharded with mjpcx_comm_init");
  if (c->env_E != E)
    return fail(c, MJPCX_EINVAL, c->env_E == 0 ? who + "before mjpcx_set_states"
                                               : who + std::to_string(E) + " environments after mjpcx_set_states of " + std::to_string(c->env_E));
  HIPCHK(c, hipSetDevice(c->device));
  return c->precision == 64 ? do_feedback<double>(c, E, n, H, mode, representation, use_state, Tn, times, states, actions, gains, improvement, alpha)
                            : do_feedback<float>(c, E, n, H, mode, representation, use_state, Tn, times, states, actions, gains, improvement, alpha);
}

int mjpcx_transition_fd(mjpcx_ctx* c, int Tn, const double* times, const double* states, const double* actions, double eps,
                        int centered, double* A, double* B, double* C, double* D) {
  if (!c || !times || !states || !actions) return fail(c, MJPCX_EINVAL, "null argument");
  if (Tn < 1 || !(eps > 0)) return fail(c, MJPCX_EINVAL, "bad horizon or epsilon");
  HIPCHK(c, hipSetDevice(c->device));
  if (c->wave && c->precision != 64) return fail(c, MJPCX_EUNSUPPORTED, "the iLQG kernels of the wavefront-per-candidate family are fp64 only");
  auto run = [&](auto precision) {
    using T = decltype(precision);
    int rc;
    const size_t ds = c->nq + c->nv, ndx = 2 * (size_t)c->nv, nu = c->nu, nr = c->nr, sT = Tn;
    PlanRecords rec;
    if ((rc = stage_records<T>(c, 0, &rec)) != MJPCX_OK) return rc;
    const T* d[5];
    if ((rc = upload_arrays<T>(c, {{times, sT}, {states, sT * ds}, {actions, sT * nu}, {c->ctrlrange.data(), 2 * nu}, {c->ctrllimited.data(), nu}}, d)) != MJPCX_OK)
      return rc;
    size_t off = 0;
    const FdCarve w = carve_fd<T>(c, sT, [&](size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; });
    HIPCHK(c, c->d_ilqg_out.reserve(off));
    char* base = (char*)c->d_ilqg_out.p;
    if ((rc = enqueue_fd<T>(c, 0, Tn, eps, centered, rec, FdIn<T>{d[0], d[1], d[2], d[3], (const int*)d[4]}, base, w)) != MJPCX_OK) return rc;
    HIPCHK(c, rec.slot->host.mark(c->stream));
    return download(c, {{A, base + w.A, sT * ndx * ndx * 8}, {B, base + w.B, sT * ndx * nu * 8}, {C, base + w.C, sT * nr * ndx * 8}, {D, base + w.D, sT * nr * nu * 8}});
  };
  return by_precision(c, run);
}

int mjpcx_kinematics(mjpcx_ctx* c, double* xpos, double* xquat, double* xmat, double* xipos, double* site_xpos, double* subtree_com,
                     double* subtree_linvel) {
  if (!c) return MJPCX_EINVAL;
  if (!c->wave) return fail(c, MJPCX_EUNSUPPORTED, "mjpcx_kinematics is implemented for the wavefront-per-candidate models only");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  PlanRecords rec;
  if ((rc = stage_records<double>(c, 0, &rec)) != MJPCX_OK) return rc;  // (the fp64 blob in either precision: the kernel is fp64)
  const size_t nb = (size_t)c->wh.m.nbody_model, ns = (size_t)c->nsite_model;
  const size_t total = 3 * nb + 4 * nb + 9 * nb + 3 * nb + 3 * ns + 3 * nb + 3 * nb;
  HIPCHK(c, c->d_ilqg_out.reserve(total * 8));
  HIPCHK(c, hipMemsetAsync(c->d_ilqg_out.p, 0, total * 8, c->stream));
  const size_t lds = wave_lds_bytes(c, 1);
  HIPCHK(c, launch_kinematics_wave(c->wh.m, wave_task(c, rec.blob), (double*)c->d_ilqg_out.p, (int)nb, (int)ns, lds, c->stream));
  HIPCHK(c, rec.slot->host.mark(c->stream));
  std::vector<double> h(total);
  if ((rc = download(c, {{h.data(), c->d_ilqg_out.p, total * 8}})) != MJPCX_OK) return rc;
  const double* p = h.data();
  auto take = [&](double* dst, size_t n) { if (dst) std::memcpy(dst, p, n * 8); p += n; };
  take(xpos, 3 * nb); take(xquat, 4 * nb); take(xmat, 9 * nb); take(xipos, 3 * nb); take(site_xpos, 3 * ns); take(subtree_com, 3 * nb);
  take(subtree_linvel, 3 * nb);
  return MJPCX_OK;
}

int mjpcx_cost_derivatives(mjpcx_ctx* c, int T, const double* residual, const double* C, const double* D, double* cx,
                           double* cu, double* cxx, double* cxu, double* cuu) {
  if (!c || !residual || !C || !D || !cx || !cu || !cxx || !cxu || !cuu) return fail(c, MJPCX_EINVAL, "null argument");
  if (T < 1) return fail(c, MJPCX_EINVAL, "T must be >= 1");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t ndx = 2 * (size_t)c->nv, nu = c->nu, nr = c->nr;
  CostSpec cs{};
  int rc;
  if ((rc = make_cost_spec(c, &cs)) != MJPCX_OK) return rc;
  const double* d[3];
  if ((rc = upload_arrays<double>(c, {{residual, T * nr}, {C, T * nr * ndx}, {D, T * nr * nu}}, d)) != MJPCX_OK) return rc;
  const size_t n_out = T * (ndx + nu + ndx * ndx + ndx * nu + nu * nu);
  HIPCHK(c, c->d_ilqg_out.reserve(n_out * 8));
  double* o = (double*)c->d_ilqg_out.p;
  double *dcx = o, *dcu = dcx + T * ndx, *dcxx = dcu + T * nu, *dcxu = dcxx + T * ndx * ndx, *dcuu = dcxu + T * ndx * nu;
  const size_t shmem = (32 + 32 * 32 + 32 * ndx + 32 * nu) * 8;
  hipLaunchKernelGGL(cost_derivatives_kernel, dim3(T), dim3(64), shmem, c->stream, cs, d[0], d[1], d[2], T, (int)ndx, (int)nu, dcx, dcu, dcxx, dcxu, dcuu, (const CostRow*)nullptr, 1);
  HIPCHK(c, hipGetLastError());
  return download(c, {{cx, dcx, T * ndx * 8}, {cu, dcu, T * nu * 8}, {cxx, dcxx, T * ndx * ndx * 8}, {cxu, dcxu, T * ndx * nu * 8}, {cuu, dcuu, T * nu * nu * 8}});
}

int mjpcx_backward_pass(mjpcx_ctx* c, int n, int m, int T, double mu, int reg_type, int use_limits, const double* A,
                        const double* B, const double* cx, const double* cu, const double* cxx, const double* cxu,
                        const double* cuu, const double* actions, const double* limits, double* Vx, double* Vxx, double* K,
                        double* du, double* dV, int32_t* status, double* kernel_ms) {
  if (!c || !A || !B || !cx || !cu || !cxx || !cxu || !cuu || !actions || !limits || !Vx || !Vxx || !K || !du || !dV || !status)
    return fail(c, MJPCX_EINVAL, "null argument");
  if (n < 1 || n > 48 || m < 1 || m > 16 || T < 2) return fail(c, MJPCX_EUNSUPPORTED, "backward pass kernel covers 1 <= n <= 48, 1 <= m <= 16, T >= 2");
  if (reg_type < 0 || reg_type > 2) return fail(c, MJPCX_EINVAL, "unknown regularization type");
  HIPCHK(c, hipSetDevice(c->device));
  const double* d[9];
  int rc;
  const size_t sn = n, sm = m, sT = T;
  if ((rc = upload_arrays<double>(c, {{A, sT * sn * sn}, {B, sT * sn * sm}, {cx, sT * sn}, {cu, sT * sm}, {cxx, sT * sn * sn},
                                      {cxu, sT * sn * sm}, {cuu, sT * sm * sm}, {actions, sT * sm}, {limits, 2 * sm}}, d)) != MJPCX_OK)
    return rc;
  const size_t n_out = sT * (sn + sn * sn + sm * sn + sm) + 2 + 2 + 16;
  HIPCHK(c, c->d_ilqg_out.reserve(n_out * 8));
  double* o = (double*)c->d_ilqg_out.p;
  BackwardArgs a{};
  a.n = n; a.m = m; a.T = T; a.mu = mu; a.reg_type = reg_type; a.use_limits = use_limits;
  a.A = d[0]; a.B = d[1]; a.cx = d[2]; a.cu = d[3]; a.cxx = d[4]; a.cxu = d[5]; a.cuu = d[6]; a.actions = d[7]; a.limits = d[8];
  a.Vx = o; a.Vxx = a.Vx + sT * sn; a.K = a.Vxx + sT * sn * sn; a.du = a.K + sT * sm * sn; a.dV = a.du + sT * sm;
  a.status = (int*)(a.dV + 2);
  a.stamps = c->stamp_step >= 0 ? (long long*)(a.dV + 4) : nullptr;
  LaunchTimer timer;
  HIPCHK(c, timer.start(c->stream));
  if ((rc = launch_backward(c, backward_pass_kernel<12>, backward_pass_kernel<16>, n, m, 1, a)) != MJPCX_OK) return rc;
  HIPCHK(c, timer.stop(c->stream));
  if ((rc = download(c, {{Vx, a.Vx, sT * sn * 8}, {Vxx, a.Vxx, sT * sn * sn * 8}, {K, a.K, sT * sm * sn * 8}, {du, a.du, sT * sm * 8}, {dV, a.dV, 16},
                         {status, a.status, 4}})) != MJPCX_OK)
    return rc;
  if (a.stamps) {
    long long h[9];
    (void)hipMemcpy(h, a.stamps, sizeof h, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "backward_pass phase cycles (second step): stage %lld gemm %lld reg %lld du/qp %lld Kcols %lld update %lld write %lld\n",
                 h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[5] - h[4], h[6] - h[5], h[7] - h[6]);
  }
  if (kernel_ms) *kernel_ms = timer.ms();
  return MJPCX_OK;
}

int mjpcx_gradient_pass(mjpcx_ctx* c, int n, int m, int T, const double* A, const double* B, const double* cx, const double* cu,
                        int representation, int P, const double* node_times, const double* step_times, double* Vx, double* k,
                        double* dV, double* gradient, double* kernel_ms) {
  if (!c || !A || !B || !cx || !cu || !node_times || !step_times || !Vx || !k || !dV || !gradient)
    return fail(c, MJPCX_EINVAL, "null argument");
  if (n < 1 || m < 1 || T < 2 || P < 1) return fail(c, MJPCX_EINVAL, "gradient pass needs n >= 1, m >= 1, T >= 2, P >= 1");
  if (n > kGradMaxN || m > kGradMaxM || P > kGradMaxP || T > kGradMaxT)
    return fail(c, MJPCX_EUNSUPPORTED, "gradient pass kernel covers n <= 48, m <= 16, P <= 25 (kMaxGradientSplinePoints), T <= 512 (kMaxTrajectoryHorizon)");
  if (representation < 0 || representation > 2) return fail(c, MJPCX_EINVAL, "representation must be 0 (zero-order), 1 (linear) or 2 (cubic)");
  for (int i = 1; i < P; i++)
    if (!(node_times[i] > node_times[i - 1])) return fail(c, MJPCX_EINVAL, "node times must be strictly increasing");
  HIPCHK(c, hipSetDevice(c->device));
  const double* d[6];
  int rc;
  const size_t sn = n, sm = m, sT = T, sP = P;
  if ((rc = upload_arrays<double>(c, {{A, sT * sn * sn}, {B, sT * sn * sm}, {cx, sT * sn}, {cu, sT * sm}, {node_times, sP}, {step_times, sT}}, d)) != MJPCX_OK)
    return rc;
  const size_t n_out = sT * (sn + sm) + 2 + sP * sm;
  HIPCHK(c, c->d_ilqg_out.reserve(n_out * 8));
  GradientArgs a{};
  a.n = n; a.m = m; a.T = T; a.P = P; a.representation = representation;
  a.A = d[0]; a.B = d[1]; a.cx = d[2]; a.cu = d[3]; a.node_times = d[4]; a.step_times = d[5];
  a.Vx = (double*)c->d_ilqg_out.p; a.k = a.Vx + sT * sn; a.dV = a.k + sT * sm; a.gradient = a.dV + 2;
  const size_t lds = gradient_pass_lds_bytes(T, m, P);
  HIPCHK(c, hipFuncSetAttribute((const void*)gradient_pass_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  LaunchTimer timer;
  HIPCHK(c, timer.start(c->stream));
  hipLaunchKernelGGL(gradient_pass_kernel, dim3(1), dim3(64), lds, c->stream, a);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, timer.stop(c->stream));
  if ((rc = download(c, {{Vx, a.Vx, sT * sn * 8}, {k, a.k, sT * sm * 8}, {dV, a.dV, 16}, {gradient, a.gradient, sP * sm * 8}})) != MJPCX_OK) return rc;
  if (kernel_ms) *kernel_ms = timer.ms();
  return MJPCX_OK;
}

}  // extern "C"

namespace {
// The shared front and tail of mjpcx_gradient_step_batched and mjpcx_ilqg_step_batched: ModelDerivatives::Compute for E environments from
// the last batched rollout, enqueued on the context's stream, and the one download. One device workspace (d_grad), carved in this order:
//   [evaluate | ctrllimited | ctrlrange | candidates | sources | active | from | cost rows | the caller's inputs]  one upload from h_grad
//   [gathered nominal | finite-difference workspace | A, B, C, D at all T steps | the caller's arrays]
//   [nominal_return | the caller's results]                                                                 one download into h_grad
// The caller carves its own fields with carve() after the constructor, after carve_work() and after carve_results(); then stage(), its
// inputs into hin, run(), its own kernels, finish().
struct StepResult { size_t at, bytes_per_env; void* dst; };  // a field of the result block and where it goes (nullptr: nowhere)
template <typename T>
struct StepChain {
  mjpcx_ctx* c;
  int E, Tn, ne;
  size_t ds, ndx, nu, nr, nc, sE, sT, rows, sA, sB, sC, sD;
  size_t off = 0, in_bytes = 0, o_out = 0;
  size_t o_eval, o_lim, o_range, o_cand, o_src, o_act, o_from, o_rows, o_ft = 0, o_fs = 0, o_fa = 0, o_res = 0, o_A = 0, o_B = 0, o_C = 0, o_D = 0, o_ret = 0;
  FdCarve fd{};
  PlanRecords rec{};
  char *base = nullptr, *hin = nullptr, *hout = nullptr;
  // mjpcx_ilqg_step_batched_from: the environments with from[e] != 0 take their nominal from the last batched rollout of `other`
  mjpcx_ctx* other = nullptr;
  const int32_t* from = nullptr;

  size_t carve(size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; }
  double* f64(size_t o) const { return (double*)(base + o); }
  int* i32(size_t o) const { return (int*)(base + o); }
  T* real(size_t o) const { return (T*)(base + o); }
  StepChain(mjpcx_ctx* c_, int E_, int Tn_, int ne_) : c(c_), E(E_), Tn(Tn_), ne(ne_) {
    ds = c->nq + c->nv; ndx = 2 * (size_t)c->nv; nu = c->nu; nr = c->nr; nc = 1 + 2 * (ndx + nu);
    sE = E; sT = Tn; rows = sE * ne; sA = ndx * ndx; sB = ndx * nu; sC = nr * ndx; sD = nr * nu;
    o_eval = carve((size_t)ne * 4); o_lim = carve(nu * 4); o_range = carve(2 * nu * sizeof(T));
    o_cand = carve(sE * 4); o_src = carve(sE * 4); o_act = carve(sE * 4); o_from = carve(sE * 4);
    o_rows = carve(has_env_task_params(c) ? sE * sizeof(CostRow) : 0);  // (mjpcx_set_task_params_batched: each environment's cost parameters)
  }
  // what the cost kernels take as their rows: nullptr while every environment shares the context's task parameters
  const CostRow* cost_rows() const { return has_env_task_params(c) ? (const CostRow*)(base + o_rows) : nullptr; }
  bool too_large() const { return sE * std::max((size_t)ne * nc, sT) * (ndx + nr) * (ndx + nu) > 0x7fffffffULL; }  // (the kernels index with int)
  void carve_work() {
    in_bytes = off;
    o_ft = carve(rows * sizeof(T)); o_fs = carve(rows * ds * sizeof(T)); o_fa = carve(rows * nu * sizeof(T)); o_res = carve(sE * sT * nr * 8);
    fd = carve_fd<T>(c, rows, [this](size_t bytes) { return carve(bytes); });
    o_A = carve(sE * sT * sA * 8); o_B = carve(sE * sT * sB * 8); o_C = carve(sE * sT * sC * 8); o_D = carve(sE * sT * sD * 8);
  }
  void carve_results() { o_out = off; o_ret = carve(sE * 8); }
  // the buffers, the environments' plan records restaged (the preceding rollout's slot may have been recycled since) and the shared
  // inputs. candidate[e] < 0: environment e takes no part and rides along on the first active one's nominal (its finite differences
  // need SOME valid trajectory); at least one takes part.
  int stage(const int32_t* candidate, const int32_t* evaluate, const CostSpec& cs) {
    int rc;
    if ((rc = stage_records<T>(c, E, &rec)) != MJPCX_OK) return rc;
    HIPCHK(c, c->d_grad.reserve(off));
    HIPCHK(c, c->h_grad.reserve(in_bytes + off - o_out));
    base = (char*)c->d_grad.p; hin = (char*)c->h_grad.p; hout = hin + in_bytes;
    std::memcpy(hin + o_eval, evaluate, (size_t)ne * 4);
    std::memcpy(hin + o_lim, c->ctrllimited.data(), nu * 4);
    for (size_t i = 0; i < 2 * nu; i++) ((T*)(hin + o_range))[i] = (T)c->ctrlrange[i];
    int first = 0;
    while (candidate[first] < 0) first++;
    for (int e = 0; e < E; e++) {
      const bool on = candidate[e] >= 0;
      ((int*)(hin + o_cand))[e] = candidate[on ? e : first];
      ((int*)(hin + o_src))[e] = on ? e : first;
      ((int*)(hin + o_act))[e] = on ? 1 : 0;
      ((int*)(hin + o_from))[e] = from && from[on ? e : first] ? 1 : 0;
    }
    if (has_env_task_params(c)) {  // the environment's own fields where given, the context's (cs) elsewhere
      const size_t nt = c->nterm;
      for (int e = 0; e < E; e++) {
        CostRow& row = ((CostRow*)(hin + o_rows))[e];
        std::memcpy(row.weight, cs.weight, sizeof row.weight); std::memcpy(row.p, cs.p, sizeof row.p); std::memcpy(row.q, cs.q, sizeof row.q);
        row.risk = c->env_risk.empty() ? cs.risk : c->env_risk[e];
        for (size_t k = 0; k < nt; k++) {
          if (!c->env_weight.empty()) row.weight[k] = c->env_weight[e * nt + k];
          if (!c->env_normp.empty()) { row.p[k] = c->env_normp[e * nt + k]; row.q[k] = c->env_normq[e * nt + k]; }
        }
      }
    }
    return MJPCX_OK;
  }
  // the upload; the nominal candidates gathered (with the rows the caller asks for); the finite differences at the evaluated steps of
  // every environment, interpolated to all Tn steps with A, B, D of the last one zeroed
  int run(double eps, int centered, double* step_times, double* actions_out) {
    HIPCHK(c, hipMemcpyAsync(base, hin, in_bytes, hipMemcpyHostToDevice, c->stream));
    GatherCandidatesArgs<T> g{};
    g.states = (const T*)c->d_states.p; g.actions = (const T*)c->d_actions.p; g.times = (const T*)c->d_times.p; g.residual = (const T*)c->d_residual.p;
    g.total_return = (const double*)c->d_ret.p;
    g.N = c->N; g.H = c->H; g.n_per_env = c->env_n; g.candidate_major = c->traj_candidate_major ? 1 : 0;
    if (other) {
      g.alt.states = (const T*)other->d_states.p; g.alt.actions = (const T*)other->d_actions.p; g.alt.times = (const T*)other->d_times.p;
      g.alt.residual = (const T*)other->d_residual.p; g.alt.total_return = (const double*)other->d_ret.p;
      g.alt.N = other->N; g.alt.H = other->H; g.alt.n_per_env = other->env_n; g.alt.candidate_major = other->traj_candidate_major ? 1 : 0;
      g.from_alt = i32(o_from);
    }
    g.cands = i32(o_cand); g.source = i32(o_src); g.active = i32(o_act);
    g.E = E; g.Tn = Tn; g.ne = ne; g.evaluate = i32(o_eval);
    g.ds_roll = c->nq + c->nv + c->na; g.ds = (int)ds; g.nu = (int)nu; g.nr = (int)nr;
    g.fd_times = real(o_ft); g.fd_states = real(o_fs); g.fd_actions = real(o_fa);
    g.residual_out = f64(o_res); g.nominal_return = f64(o_ret); g.step_times = step_times; g.actions_out = actions_out;
    const size_t g_items = sE * ((size_t)ne * (1 + ds + nu) + sT * (nr + (step_times ? 1 : 0) + (actions_out ? nu : 0)) + 1);
    hipLaunchKernelGGL((gather_candidates_kernel<T>), dim3((unsigned)std::min<size_t>((g_items + 255) / 256, 2048)), dim3(256), 0, c->stream, g);
    HIPCHK(c, hipGetLastError());
    int rc;
    const FdIn<T> in{g.fd_times, g.fd_states, g.fd_actions, real(o_range), i32(o_lim)};
    if ((rc = enqueue_fd<T>(c, E, ne, eps, centered, rec, in, base, fd)) != MJPCX_OK) return rc;
    const size_t i_items = sE * sT * (sA + sB + sC + sD);
    hipLaunchKernelGGL(fd_interpolate_kernel, dim3((unsigned)std::min<size_t>((i_items + 255) / 256, 4096)), dim3(256), 0, c->stream, f64(fd.A),
                       f64(fd.B), f64(fd.C), f64(fd.D), i32(o_eval), E, ne, Tn, (int)sA, (int)sB,
                       (int)sC, (int)sD, f64(o_A), f64(o_B), f64(o_C), f64(o_D));
    HIPCHK(c, hipGetLastError());
    return MJPCX_OK;
  }
  // the result block into pinned memory, the optional arrays straight to the caller, ONE sync, and the block's fields to where they go
  int finish(const Download* optional, size_t n_optional, std::initializer_list<StepResult> results) {
    HIPCHK(c, rec.slot->host.mark(c->stream));
    HIPCHK(c, hipMemcpyAsync(hout, base + o_out, off - o_out, hipMemcpyDeviceToHost, c->stream));
    int rc;
    if ((rc = download(c, optional, n_optional)) != MJPCX_OK) return rc;
    for (auto& r : results)
      if (r.dst) std::memcpy(r.dst, hout + (r.at - o_out), sE * r.bytes_per_env);
    return MJPCX_OK;
  }
};

// mjpcx_gradient_step_batched after validation
template <typename T>
int do_gradient_step_batched(mjpcx_ctx* c, int E, int cand, int Tn, int ne, const int32_t* evaluate, double eps, int centered, int representation,
                             int P, const double* node_times, double* nominal_return, double* k, double* gradient, double* dV, double* A,
                             double* B, double* cx, double* cu) {
  int rc;
  CostSpec cs{};
  if ((rc = make_cost_spec(c, &cs)) != MJPCX_OK) return rc;
  StepChain<T> s(c, E, Tn, ne);
  if (s.too_large()) return fail(c, MJPCX_EUNSUPPORTED, "mjpcx_gradient_step_batched: too many environments x steps");
  const size_t sE = E, sT = Tn, sP = P, ndx = s.ndx, nu = s.nu;
  const size_t o_nodes = s.carve(sE * sP * 8);
  s.carve_work();
  const size_t o_st = s.carve(sE * sT * 8), o_cx = s.carve(sE * sT * ndx * 8), o_cu = s.carve(sE * sT * nu * 8), o_Vx = s.carve(sE * sT * ndx * 8);
  s.carve_results();
  const size_t o_k = s.carve(sE * sT * nu * 8), o_g = s.carve(sE * sP * nu * 8), o_dV = s.carve(sE * 2 * 8);
  const std::vector<int32_t> cands(E, cand);  // the same local candidate of every environment; every environment takes part
  if ((rc = s.stage(cands.data(), evaluate, cs)) != MJPCX_OK) return rc;
  std::memcpy(s.hin + o_nodes, node_times, sE * sP * 8);
  if ((rc = s.run(eps, centered, s.f64(o_st), nullptr)) != MJPCX_OK) return rc;
  // ---- CostDerivatives::Compute (first order) and Gradient::Compute with the projection, per environment
  double *dA = s.f64(s.o_A), *dB = s.f64(s.o_B), *dcx = s.f64(o_cx), *dcu = s.f64(o_cu);
  hipLaunchKernelGGL(cost_gradient_kernel, dim3((unsigned)(sE * sT)), dim3(64), (32 + 32 * 32) * 8, c->stream, cs, s.f64(s.o_res),
                     s.f64(s.o_C), s.f64(s.o_D), Tn, (int)ndx, (int)nu, dcx, dcu, s.cost_rows());
  HIPCHK(c, hipGetLastError());
  GradientArgs ga{};
  ga.n = (int)ndx; ga.m = (int)nu; ga.T = Tn; ga.P = P; ga.representation = representation;
  ga.A = dA; ga.B = dB; ga.cx = dcx; ga.cu = dcu; ga.node_times = s.f64(o_nodes); ga.step_times = s.f64(o_st);
  ga.Vx = s.f64(o_Vx); ga.k = s.f64(o_k); ga.dV = s.f64(o_dV); ga.gradient = s.f64(o_g);
  const size_t lds = gradient_pass_lds_bytes(Tn, (int)nu, P);
  HIPCHK(c, hipFuncSetAttribute((const void*)gradient_pass_batched_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(gradient_pass_batched_kernel, dim3(E), dim3(64), lds, c->stream, ga);
  HIPCHK(c, hipGetLastError());
  const Download optional[4] = {{A, dA, sE * sT * s.sA * 8}, {B, dB, sE * sT * s.sB * 8}, {cx, dcx, sE * sT * ndx * 8}, {cu, dcu, sE * sT * nu * 8}};
  return s.finish(optional, 4, {{s.o_ret, 8, nominal_return}, {o_k, sT * nu * 8, k}, {o_g, sP * nu * 8, gradient}, {o_dV, 16, dV}});
}

// mjpcx_ilqg_step_batched and mjpcx_ilqg_step_batched_from (other, from: StepChain; nullptr for the former) after validation
template <typename T>
int do_ilqg_step_batched(mjpcx_ctx* c, mjpcx_ctx* other, const int32_t* from, int E, const int32_t* candidate, int Tn, int ne, const int32_t* evaluate, double eps, int centered, int reg_type,
                         int use_limits, const double* mu, const double* rate, double factor, double min_reg, double max_reg, int max_iter, double* K,
                         double* du, double* dV, int32_t* status, double* mu_out, double* rate_out, int32_t* retries, double* nominal_return,
                         double* const (&opt)[9]) {
  int rc;
  CostSpec cs{};
  if ((rc = make_cost_spec(c, &cs)) != MJPCX_OK) return rc;
  StepChain<T> s(c, E, Tn, ne);
  s.other = other; s.from = from;
  if (s.too_large()) return fail(c, MJPCX_EUNSUPPORTED, "mjpcx_ilqg_step_batched: too many environments x steps");
  const size_t sE = E, sT = Tn, ndx = s.ndx, nu = s.nu, sA = s.sA, sB = s.sB;
  // the optional outputs A, B, cx, cu, cxx, cxu, cuu, Vx, Vxx: elements per environment
  const size_t per[9] = {sT * sA, sT * sB, sT * ndx, sT * nu, sT * sA, sT * sB, sT * nu * nu, sT * ndx, sT * sA};
  // an environment that takes no part gets zeros and status -1
  auto unpack_inactive = [&](int e) {
    std::memset(K + (size_t)e * sT * sB, 0, sT * sB * 8); std::memset(du + (size_t)e * sT * nu, 0, sT * nu * 8); std::memset(dV + (size_t)e * 2, 0, 16);
    status[e] = -1; mu_out[e] = 0; rate_out[e] = 0; retries[e] = 0;
    if (nominal_return) nominal_return[e] = 0;
    for (int k = 0; k < 9; k++) if (opt[k]) std::memset(opt[k] + (size_t)e * per[k], 0, per[k] * 8);
  };
  if (std::all_of(candidate, candidate + E, [](int32_t x) { return x < 0; })) {  // nobody takes part: nothing to launch
    for (int e = 0; e < E; e++) unpack_inactive(e);
    return MJPCX_OK;
  }
  const size_t o_mu = s.carve(sE * 8), o_rate = s.carve(sE * 8), o_limits = s.carve(2 * nu * 8);
  s.carve_work();
  const size_t o_actions = s.carve(sE * sT * nu * 8);
  const size_t o_cx = s.carve(sE * per[2] * 8), o_cu = s.carve(sE * per[3] * 8), o_cxx = s.carve(sE * per[4] * 8), o_cxu = s.carve(sE * per[5] * 8);
  const size_t o_cuu = s.carve(sE * per[6] * 8), o_Vx = s.carve(sE * per[7] * 8), o_Vxx = s.carve(sE * per[8] * 8);
  s.carve_results();
  const size_t o_K = s.carve(sE * sT * sB * 8), o_du = s.carve(sE * sT * nu * 8), o_dV = s.carve(sE * 2 * 8);
  const size_t o_muo = s.carve(sE * 8), o_rateo = s.carve(sE * 8), o_status = s.carve(sE * 4), o_retries = s.carve(sE * 4);
  if ((rc = s.stage(candidate, evaluate, cs)) != MJPCX_OK) return rc;
  std::memcpy(s.hin + o_mu, mu, sE * 8);
  std::memcpy(s.hin + o_rate, rate, sE * 8);
  std::memcpy(s.hin + o_limits, c->ctrlrange.data(), 2 * nu * 8);
  // (Vx .. retries are contiguous: what a failed sweep or an environment that takes no part does not write reads as zero)
  HIPCHK(c, hipMemsetAsync(s.base + o_Vx, 0, s.off - o_Vx, c->stream));
  if (other && other != c) {  // the gather reads the other context's rollout: this stream goes behind what that one holds now
    if (!c->source_done) HIPCHK(c, hipEventCreateWithFlags(&c->source_done, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->source_done, other->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->source_done, 0));
  }
  if ((rc = s.run(eps, centered, nullptr, s.f64(o_actions))) != MJPCX_OK) return rc;
  // ---- CostDerivatives::Compute: workgroup e * Tn + t forms step t of environment e (every array is environment-major)
  const size_t at[9] = {s.o_A, s.o_B, o_cx, o_cu, o_cxx, o_cxu, o_cuu, o_Vx, o_Vxx};
  double* w[9];
  for (int k = 0; k < 9; k++) w[k] = s.f64(at[k]);
  hipLaunchKernelGGL(cost_derivatives_kernel, dim3((unsigned)(sE * sT)), dim3(64), (32 + 32 * 32 + 32 * ndx + 32 * nu) * 8, c->stream, cs,
                     s.f64(s.o_res), s.f64(s.o_C), s.f64(s.o_D), Tn, (int)ndx, (int)nu,
                     w[2], w[3], w[4], w[5], w[6], s.cost_rows(), Tn);
  HIPCHK(c, hipGetLastError());
  // ---- the backward pass with its regularisation retries, one workgroup per environment
  BackwardBatchedArgs b{};
  b.base.n = (int)ndx; b.base.m = (int)nu; b.base.T = Tn; b.base.reg_type = reg_type; b.base.use_limits = use_limits;
  b.base.A = w[0]; b.base.B = w[1]; b.base.cx = w[2]; b.base.cu = w[3]; b.base.cxx = w[4]; b.base.cxu = w[5]; b.base.cuu = w[6];
  b.base.actions = s.f64(o_actions); b.base.limits = s.f64(o_limits);
  b.base.Vx = w[7]; b.base.Vxx = w[8]; b.base.K = s.f64(o_K); b.base.du = s.f64(o_du); b.base.dV = s.f64(o_dV);
  b.active = s.i32(s.o_act); b.mu = s.f64(o_mu); b.rate = s.f64(o_rate);
  b.factor = factor; b.min_reg = min_reg; b.max_reg = max_reg; b.max_iter = max_iter;
  b.status = s.i32(o_status); b.retries = s.i32(o_retries); b.mu_out = s.f64(o_muo); b.rate_out = s.f64(o_rateo);
  if ((rc = launch_backward(c, backward_pass_batched_kernel<12>, backward_pass_batched_kernel<16>, (int)ndx, (int)nu, (unsigned)E, b)) != MJPCX_OK) return rc;
  Download optional[9];
  for (int k = 0; k < 9; k++) optional[k] = {opt[k], w[k], sE * per[k] * 8};
  if ((rc = s.finish(optional, 9, {{s.o_ret, 8, nominal_return}, {o_K, sT * sB * 8, K}, {o_du, sT * nu * 8, du}, {o_dV, 16, dV}, {o_muo, 8, mu_out},
                                   {o_rateo, 8, rate_out}, {o_status, 4, status}, {o_retries, 4, retries}})) != MJPCX_OK)
    return rc;
  for (int e = 0; e < E; e++) if (candidate[e] < 0) unpack_inactive(e);
  return MJPCX_OK;
}

// mjpcx_ilqg_step_batched (src == nullptr, from == nullptr) and mjpcx_ilqg_step_batched_from (some from[e] == 1, src given): validation
int ilqg_step_batched_entry(const char* who_, mjpcx_ctx* c, mjpcx_ctx* src, const int32_t* from, int E, const int32_t* candidate, int T, int ne,
                            const int32_t* evaluate, double eps, int centered, int reg_type, int use_limits, const double* mu, const double* rate,
                            double factor, double min_reg, double max_reg, int max_iter, double* K, double* du, double* dV, int32_t* status,
                            double* mu_out, double* rate_out, int32_t* retries, double* nominal_return, double* const (&opt)[9]) {
  const std::string who = who_;
  if (!c || !candidate || !evaluate || !mu || !rate || !K || !du || !dV || !status || !mu_out || !rate_out || !retries)
    return fail(c, MJPCX_EINVAL, who + "null argument");
  if (src && (src->device != c->device || src->precision != c->precision || src->nq != c->nq || src->nv != c->nv || src->na != c->na ||
              src->nu != c->nu || src->nr != c->nr))
    return fail(c, MJPCX_EINVAL, who + "the two contexts differ in device, precision or model dimensions (nq, nv, na, nu, nr)");
  // which context the active environments name: this one (also with nobody active, as mjpcx_ilqg_step_batched), the source
  bool own = !from, other = false, active = false;
  for (int e = 0; from && e < E; e++)
    if (candidate[e] >= 0) { active = true; (from[e] ? other : own) = true; }
  if (from && !active) own = true;
  if (own) {
    if (!c->have_rollout && from)  // (somebody names the source, somebody this context, which has none)
      return fail(c, MJPCX_EINVAL, who + "the last rollout was not a batched one of " + std::to_string(E) + " environments (there is none)");
    if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
    if (E < 1 || c->env_n < 1 || (long long)E * c->env_n != c->N || c->env_E != E)
      return fail(c, MJPCX_EINVAL, who + "the last rollout was not a batched one of " + std::to_string(E) + " environments");
  } else if (c->env_E != E) {  // every nominal comes from the source: this context brings the plan records alone
    return fail(c, MJPCX_EINVAL, c->env_E == 0 ? who + "before mjpcx_set_states"
                                               : who + std::to_string(E) + " environments after mjpcx_set_states of " + std::to_string(c->env_E));
  }
  if (other && (!src->have_rollout || src->env_n < 1 || (long long)E * src->env_n != src->N))
    return fail(c, MJPCX_EINVAL, who + "the source's last rollout was not a batched one of " + std::to_string(E) + " environments");
  for (int e = 0; e < E; e++) {
    const mjpcx_ctx* x = from && from[e] ? src : c;
    if (candidate[e] < -1 || (candidate[e] >= 0 && candidate[e] >= x->env_n))
      return fail(c, MJPCX_EINVAL, who + "candidate outside [-1, n_per_env) (environment " + std::to_string(e) + ")");
  }
  if (T < 2 || (own && T > c->H)) return fail(c, MJPCX_EINVAL, who + "T must be >= 2 and within the rollout's horizon");
  if (other && T > src->H) return fail(c, MJPCX_EINVAL, who + "T must be within the horizon of the source's rollout");
  if (ne < 1 || ne > T) return fail(c, MJPCX_EINVAL, who + "num_eval outside [1, T]");
  for (int i = 0; i < ne; i++)
    if (evaluate[i] < 0 || evaluate[i] >= T || (i > 0 && evaluate[i] <= evaluate[i - 1]))
      return fail(c, MJPCX_EINVAL, who + "the evaluate list must be strictly increasing and within [0, T)");
  if (!(eps > 0)) return fail(c, MJPCX_EINVAL, who + "epsilon must be > 0");
  if (reg_type < 0 || reg_type > 2) return fail(c, MJPCX_EINVAL, who + "unknown regularization type");
  if (max_iter < 1 || max_iter > 64) return fail(c, MJPCX_EINVAL, who + "max_iter outside [1, 64]");
  for (int e = 0; e < E; e++)
    if (!std::isfinite(mu[e]) || !(mu[e] > 0) || !std::isfinite(rate[e]) || !(rate[e] > 0))
      return fail(c, MJPCX_EINVAL, who + "mu and rate must be finite and > 0 (environment " + std::to_string(e) + ")");
  if (!std::isfinite(factor) || !(factor > 0)) return fail(c, MJPCX_EINVAL, who + "factor must be finite and > 0");
  if (!std::isfinite(min_reg) || !std::isfinite(max_reg) || !(min_reg <= max_reg))
    return fail(c, MJPCX_EINVAL, who + "min_reg and max_reg must be finite, min_reg <= max_reg");
  if (c->comm_world > 1 || (src && src->comm_world > 1)) return fail(c, MJPCX_EUNSUPPORTED, who + "not implemented on a context sharded with mjpcx_comm_init");
  if (c->em.E > 0 || (src && src->em.E > 0)) return fail(c, MJPCX_EUNSUPPORTED, who + "the derivative chain on a model per environment (mjpcx_set_models_batched) is not implemented: clear the models, or plan these environments on contexts of their own");
  if ((c->wave && c->precision != 64) || (src && src->wave && src->precision != 64))
    return fail(c, MJPCX_EUNSUPPORTED, (from ? who : std::string()) + "the iLQG kernels of the wavefront-per-candidate family are fp64 only");
  if (2 * c->nv > kGradMaxN || c->nu > kGradMaxM || T > kGradMaxT)
    return fail(c, MJPCX_EUNSUPPORTED, who + "covers n <= 48, m <= 16, T <= 512 (kMaxTrajectoryHorizon)");
  HIPCHK(c, hipSetDevice(c->device));
  return c->precision == 64 ? do_ilqg_step_batched<double>(c, src, from, E, candidate, T, ne, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor,
                                                           min_reg, max_reg, max_iter, K, du, dV, status, mu_out, rate_out, retries, nominal_return, opt)
                            : do_ilqg_step_batched<float>(c, src, from, E, candidate, T, ne, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor,
                                                          min_reg, max_reg, max_iter, K, du, dV, status, mu_out, rate_out, retries, nominal_return, opt);
}
}  // namespace

extern "C" {

int mjpcx_gradient_step_batched(mjpcx_ctx* c, int E, int cand, int T, int ne, const int32_t* evaluate, double eps, int centered, int representation,
                                int P, const double* node_times, double* nominal_return, double* k, double* gradient, double* dV, double* A,
                                double* B, double* cx, double* cu) {
  const char* who = "mjpcx_gradient_step_batched: ";
  if (!c || !evaluate || !node_times || !k || !gradient || !dV) return fail(c, MJPCX_EINVAL, std::string(who) + "null argument");
  if (c->em.E > 0) return fail(c, MJPCX_EUNSUPPORTED, std::string(who) + "the derivative chain on a model per environment (mjpcx_set_models_batched) is not implemented: clear the models, or plan these environments on contexts of their own");
  if (!c->have_rollout) return fail(c, MJPCX_ESTATE, "no rollout has been run");
  if (E < 1 || c->env_n < 1 || (long long)E * c->env_n != c->N || c->env_E != E)
    return fail(c, MJPCX_EINVAL, std::string(who) + "the last rollout was not a batched one of " + std::to_string(E) + " environments");
  if (cand < 0 || cand >= c->env_n) return fail(c, MJPCX_EINVAL, std::string(who) + "candidate outside [0, n_per_env)");
  if (T < 2 || T > c->H) return fail(c, MJPCX_EINVAL, std::string(who) + "T must be >= 2 and within the rollout's horizon");
  if (ne < 1 || ne > T) return fail(c, MJPCX_EINVAL, std::string(who) + "num_eval outside [1, T]");
  for (int i = 0; i < ne; i++)
    if (evaluate[i] < 0 || evaluate[i] >= T || (i > 0 && evaluate[i] <= evaluate[i - 1]))
      return fail(c, MJPCX_EINVAL, std::string(who) + "the evaluate list must be strictly increasing and within [0, T)");
  if (!(eps > 0)) return fail(c, MJPCX_EINVAL, std::string(who) + "epsilon must be > 0");
  if (representation < 0 || representation > 2) return fail(c, MJPCX_EINVAL, std::string(who) + "representation must be 0 (zero-order), 1 (linear) or 2 (cubic)");
  if (P < 1) return fail(c, MJPCX_EINVAL, std::string(who) + "P must be >= 1");
  for (int e = 0; e < E; e++)
    for (int i = 1; i < P; i++)
      if (!(node_times[(size_t)e * P + i] > node_times[(size_t)e * P + i - 1]))
        return fail(c, MJPCX_EINVAL, std::string(who) + "node times must be strictly increasing (environment " + std::to_string(e) + ")");
  if (c->comm_world > 1) return fail(c, MJPCX_EUNSUPPORTED, std::string(who) + "not implemented on a context sharded with mjpcx_comm_init");
  if (c->wave && c->precision != 64) return fail(c, MJPCX_EUNSUPPORTED, "the iLQG kernels of the wavefront-per-candidate family are fp64 only");
  if (2 * c->nv > kGradMaxN || c->nu > kGradMaxM || P > kGradMaxP || T > kGradMaxT)
    return fail(c, MJPCX_EUNSUPPORTED, std::string(who) + "covers n <= 48, m <= 16, P <= 25 (kMaxGradientSplinePoints), T <= 512 (kMaxTrajectoryHorizon)");
  HIPCHK(c, hipSetDevice(c->device));
  return c->precision == 64 ? do_gradient_step_batched<double>(c, E, cand, T, ne, evaluate, eps, centered, representation, P, node_times, nominal_return, k,
                                                               gradient, dV, A, B, cx, cu)
                            : do_gradient_step_batched<float>(c, E, cand, T, ne, evaluate, eps, centered, representation, P, node_times, nominal_return, k,
                                                              gradient, dV, A, B, cx, cu);
}

int mjpcx_ilqg_step_batched(mjpcx_ctx* c, int E, const int32_t* candidate, int T, int ne, const int32_t* evaluate, double eps, int centered, int reg_type,
                            int use_limits, const double* mu, const double* rate, double factor, double min_reg, double max_reg, int max_iter, double* K,
                            double* du, double* dV, int32_t* status, double* mu_out, double* rate_out, int32_t* retries, double* nominal_return, double* A,
                            double* B, double* cx, double* cu, double* cxx, double* cxu, double* cuu, double* Vx, double* Vxx) {
  double* const opt[9] = {A, B, cx, cu, cxx, cxu, cuu, Vx, Vxx};
  return ilqg_step_batched_entry("mjpcx_ilqg_step_batched: ", c, nullptr, nullptr, E, candidate, T, ne, evaluate, eps, centered, reg_type, use_limits, mu,
                                 rate, factor, min_reg, max_reg, max_iter, K, du, dV, status, mu_out, rate_out, retries, nominal_return, opt);
}

int mjpcx_ilqg_step_batched_from(mjpcx_ctx* c, mjpcx_ctx* source, const int32_t* from_source, int E, const int32_t* candidate, int T, int ne,
                                 const int32_t* evaluate, double eps, int centered, int reg_type, int use_limits, const double* mu, const double* rate,
                                 double factor, double min_reg, double max_reg, int max_iter, double* K, double* du, double* dV, int32_t* status,
                                 double* mu_out, double* rate_out, int32_t* retries, double* nominal_return, double* A, double* B, double* cx,
                                 double* cu, double* cxx, double* cxu, double* cuu, double* Vx, double* Vxx) {
  const char* who = "mjpcx_ilqg_step_batched_from: ";
  if (!c || !from_source || !candidate) return fail(c, MJPCX_EINVAL, std::string(who) + "null argument");
  if (E < 1) return fail(c, MJPCX_EINVAL, std::string(who) + "num_envs must be >= 1");
  bool any = false;
  for (int e = 0; e < E; e++) {
    if (from_source[e] != 0 && from_source[e] != 1)
      return fail(c, MJPCX_EINVAL, std::string(who) + "from_source must be 0 or 1 (environment " + std::to_string(e) + ")");
    any = any || from_source[e] == 1;
  }
  if (any && !source) return fail(c, MJPCX_EINVAL, std::string(who) + "from_source names a source, but source is NULL");
  double* const opt[9] = {A, B, cx, cu, cxx, cxu, cuu, Vx, Vxx};
  // nobody reads the source: mjpcx_ilqg_step_batched, whatever the source is
  return ilqg_step_batched_entry(who, c, any ? source : nullptr, any ? from_source : nullptr, E, candidate, T, ne, evaluate, eps, centered, reg_type,
                                 use_limits, mu, rate, factor, min_reg, max_reg, max_iter, K, du, dV, status, mu_out, rate_out, retries, nominal_return,
                                 opt);
}

}  // extern "C"

// ===================================================================== multi-GPU exchange over RCCL
namespace {
// librccl.so.1 is resolved at run time: the library loads (and every single-GPU entry point works) without it
struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclBroadcast) Broadcast = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string error;
};
RcclApi* rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (!api.lib) { const char* why = dlerror(); api.error = std::string("librccl.so.1 not found: ") + (why ? why : ""); return; }  // (dlerror() clears itself: one call)
#define MJPCX_SYM(field, sym)                                                              \
    api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.lib, #sym));                \
    if (!api.field) api.error = std::string("RCCL symbol missing: ") + #sym;
    MJPCX_SYM(GetUniqueId, ncclGetUniqueId) MJPCX_SYM(CommInitRank, ncclCommInitRank) MJPCX_SYM(CommDestroy, ncclCommDestroy)
    MJPCX_SYM(AllGather, ncclAllGather) MJPCX_SYM(AllReduce, ncclAllReduce) MJPCX_SYM(Broadcast, ncclBroadcast)
    MJPCX_SYM(GetErrorString, ncclGetErrorString)
#undef MJPCX_SYM
  });
  return &api;
}
#define NCCLCHK(c, expr)                                                                                   \
  do {                                                                                                     \
    ncclResult_t r__ = (expr);                                                                             \
    if (r__ != ncclSuccess) return fail(c, MJPCX_EDEVICE, std::string(#expr) + ": " + rccl()->GetErrorString(r__)); \
  } while (0)

// all-gather of `n` doubles per rank: host in -> host out [world][n]
int comm_all_gather(mjpcx_ctx* c, const double* in, int n, std::vector<double>* out) {
  RcclApi* R = rccl();
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_comm_send.reserve((size_t)n * 8));
  HIPCHK(c, c->d_comm_recv.reserve((size_t)n * 8 * c->comm_world));
  HIPCHK(c, hipMemcpyAsync(c->d_comm_send.p, in, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  NCCLCHK(c, R->AllGather(c->d_comm_send.p, c->d_comm_recv.p, (size_t)n, ncclFloat64, (ncclComm_t)c->comm, c->stream));
  out->resize((size_t)n * c->comm_world);
  HIPCHK(c, hipMemcpyAsync(out->data(), c->d_comm_recv.p, (size_t)n * 8 * c->comm_world, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MJPCX_OK;
}
}  // namespace

extern "C" {

int mjpcx_comm_unique_id(void* id_out) {
  if (!id_out) return MJPCX_EINVAL;
  RcclApi* R = rccl();
  if (!R->lib || !R->error.empty()) { g_create_error = R->error; return MJPCX_EUNSUPPORTED; }
  static_assert(sizeof(ncclUniqueId) == MJPCX_COMM_ID_BYTES, "unique id size");
  ncclUniqueId id;
  if (R->GetUniqueId(&id) != ncclSuccess) { g_create_error = "ncclGetUniqueId failed"; return MJPCX_EDEVICE; }
  std::memcpy(id_out, &id, sizeof id);
  return MJPCX_OK;
}

int mjpcx_comm_init(mjpcx_ctx* c, const void* unique_id, int rank, int world) {
  if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return fail(c, MJPCX_EINVAL, "bad communicator arguments");
  RcclApi* R = rccl();
  if (!R->lib || !R->error.empty()) return fail(c, MJPCX_EUNSUPPORTED, R->error);
  if (c->comm) return fail(c, MJPCX_ESTATE, "the context already has a communicator");
  HIPCHK(c, hipSetDevice(c->device));
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof id);
  // ncclCommInitRank blocks until every rank of the world has joined: a rank that never arrives (a crashed peer, a mismatched id) would
  // hang the planner for good. The call runs on a helper thread with a deadline (MJPCX_COMM_TIMEOUT_S, default 120 s); past it the
  // context stays without a communicator, the caller gets MJPCX_EDEVICE and can fall back to its own transport (bench.py does).
  // A communicator that arrives AFTER the deadline is destroyed by the helper thread itself (the peers' next collective then fails
  // instead of waiting for a rank that has moved on); callers must agree on the fallback collectively, as bench.py does.
  double deadline = 120.0;
  if (const char* e = getenv("MJPCX_COMM_TIMEOUT_S")) {  // (validated BEFORE the helper thread exists: nothing to abandon on a bad value)
    char* end = nullptr;
    const double v = std::strtod(e, &end);
    if (end == e || !(v > 0)) return fail(c, MJPCX_EINVAL, "MJPCX_COMM_TIMEOUT_S must be a positive number of seconds");
    deadline = v;
  }
  struct InitState { std::mutex m; std::condition_variable cv; bool done = false, abandoned = false; ncclResult_t rc = ncclSuccess; ncclComm_t comm = nullptr; };
  auto st = std::make_shared<InitState>();
  const int device = c->device;
  std::thread([st, R, world, id, rank, device]() {
    (void)hipSetDevice(device);
    ncclComm_t comm = nullptr;
    const ncclResult_t rc = R->CommInitRank(&comm, world, id, rank);
    bool late;
    {
      std::lock_guard<std::mutex> lk(st->m);
      st->rc = rc; st->comm = comm; st->done = true;
      late = st->abandoned;
      st->cv.notify_all();
    }
    if (late && rc == ncclSuccess && comm) (void)R->CommDestroy(comm);
  }).detach();
  {
    std::unique_lock<std::mutex> lk(st->m);
    if (!st->cv.wait_for(lk, std::chrono::duration<double>(deadline), [&] { return st->done; })) {
      st->abandoned = true;
      return fail(c, MJPCX_EDEVICE, "ncclCommInitRank did not complete within MJPCX_COMM_TIMEOUT_S: a rank of the world is missing");
    }
  }
  NCCLCHK(c, st->rc);
  ncclComm_t comm = st->comm;
  c->comm = comm;
  c->comm_rank = rank;
  c->comm_world = world;
  return MJPCX_OK;
}

int mjpcx_comm_info(const mjpcx_ctx* c, int* rank, int* world) {
  if (!c) return MJPCX_EINVAL;
  if (rank) *rank = c->comm_rank;
  if (world) *world = c->comm_world;
  return MJPCX_OK;
}

int mjpcx_comm_destroy(mjpcx_ctx* c) {
  if (!c) return MJPCX_EINVAL;
  if (c->comm) {
    (void)hipSetDevice(c->device);
    (void)rccl()->CommDestroy((ncclComm_t)c->comm);
    c->comm = nullptr;
  }
  c->comm_rank = 0;
  c->comm_world = 1;
  return MJPCX_OK;
}

int mjpcx_exchange_best(mjpcx_ctx* c, int32_t* index, double* best_return, double* nominal_return, double* spline_values, int n) {
  if (!c || !index || !best_return || !nominal_return || (n > 0 && !spline_values) || n < 0) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->comm) return c->comm_world == 1 ? MJPCX_OK : fail(c, MJPCX_ESTATE, "mjpcx_comm_init has not been called");  // no communicator: one rank
  const double rec[3] = {*best_return, (double)*index, *nominal_return};
  int rc;
  if ((rc = comm_all_gather(c, rec, 3, &c->h_comm)) != MJPCX_OK) return rc;
  int owner = 0;
  auto key = [&](int r) { const double v = c->h_comm[3 * r]; return v != v ? (double)INFINITY : v; };
  for (int r = 1; r < c->comm_world; r++)
    if (key(r) < key(owner) || (key(r) == key(owner) && c->h_comm[3 * r + 1] < c->h_comm[3 * owner + 1])) owner = r;
  *best_return = c->h_comm[3 * owner];
  *index = (int32_t)c->h_comm[3 * owner + 1];
  *nominal_return = c->h_comm[2];  // global candidate 0 lives on rank 0
  if (n > 0) {
    RcclApi* R = rccl();
    HIPCHK(c, c->d_comm_send.reserve((size_t)n * 8));
    if (c->comm_rank == owner) HIPCHK(c, hipMemcpyAsync(c->d_comm_send.p, spline_values, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, R->Broadcast(c->d_comm_send.p, c->d_comm_send.p, (size_t)n, ncclFloat64, owner, (ncclComm_t)c->comm, c->stream));
    HIPCHK(c, hipMemcpyAsync(spline_values, c->d_comm_send.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return MJPCX_OK;
}

int mjpcx_merge_topk(mjpcx_ctx* c, int k, int64_t* index, double* total_return) {
  if (!c || k < 1 || !index || !total_return) return fail(c, MJPCX_EINVAL, "null argument");
  if (c->last_pruned && (c->last_prune_rank <= 1 || k > c->last_prune_rank)) return fail_ranking(c);  // (each rank's first K are exact: so are the merged first k <= K)
  if (!c->comm) return c->comm_world == 1 ? MJPCX_OK : fail(c, MJPCX_ESTATE, "mjpcx_comm_init has not been called");
  std::vector<double> mine(2 * (size_t)k);
  for (int i = 0; i < k; i++) {
    const bool used = index[i] >= 0;
    mine[2 * i] = used && total_return[i] == total_return[i] ? total_return[i] : (double)INFINITY;  // (NaN ranks last, and keeps the comparator a strict weak order)
    mine[2 * i + 1] = used ? (double)index[i] : 4503599627370496.0;  // 2^52: sorts after every real index
  }
  int rc;
  if ((rc = comm_all_gather(c, mine.data(), 2 * k, &c->h_comm)) != MJPCX_OK) return rc;
  const int total = k * c->comm_world;
  std::vector<int> order(total);
  for (int i = 0; i < total; i++) order[i] = i;
  const std::vector<double>& all = c->h_comm;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    if (all[2 * a] != all[2 * b]) return all[2 * a] < all[2 * b];
    return all[2 * a + 1] < all[2 * b + 1];
  });
  for (int i = 0; i < k; i++) {
    const int o = order[i];
    const bool used = all[2 * o + 1] < 4503599627370496.0;
    index[i] = used ? (int64_t)all[2 * o + 1] : -1;
    total_return[i] = used ? all[2 * o] : 1.0e300;
  }
  return MJPCX_OK;
}

int mjpcx_elite_allreduce(mjpcx_ctx* c, double* values, int n) {
  if (!c || !values || n < 1) return fail(c, MJPCX_EINVAL, "null argument");
  if (!c->comm) return c->comm_world == 1 ? MJPCX_OK : fail(c, MJPCX_ESTATE, "mjpcx_comm_init has not been called");
  RcclApi* R = rccl();
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_comm_send.reserve((size_t)n * 8));
  HIPCHK(c, hipMemcpyAsync(c->d_comm_send.p, values, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  NCCLCHK(c, R->AllReduce(c->d_comm_send.p, c->d_comm_send.p, (size_t)n, ncclFloat64, ncclSum, (ncclComm_t)c->comm, c->stream));
  HIPCHK(c, hipMemcpyAsync(values, c->d_comm_send.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MJPCX_OK;
}

int mjpcx_comm_barrier(mjpcx_ctx* c) {
  if (!c) return MJPCX_EINVAL;
  double one = 1.0;
  return mjpcx_elite_allreduce(c, &one, 1);
}

}  // extern "C"
