// quad_abi.h -- the part of the quad kernel family that the rest of the library sees (mjpcx.hip, tree_kernel.h): the rollout request, the
// failure[] marker of a candidate handed to the wavefront-per-candidate kernel, and the host entry points of the quad kernel's own
// translation unit (quad_kernel.hip). Kept apart from quad_model.h so that a change of the quad kernel's model layout does not
// re-compile the wavefront-per-candidate kernels.
#pragma once
#include <stdint.h>

#include "resume_table.h"

namespace mjpcx {
constexpr int kQFallback = 0x40000000;  // failure[] marker of a candidate the quad kernel handed on (cleared by the fallback pass)
constexpr int kQPruned = 0x20000000;   // failure[] marker of a candidate retired because it could no longer be the argmin (QArgs::prune_bound): | (retire step << 8);
                                        // a bit of its own -- the fallback pass does not re-roll it and the hand-on statistics do not count it
constexpr int kQParked = 0x10000000;   // failure[] marker of a candidate set aside on QArgs::park_hint: | (park step << 8). Never outlives a launch_quad: the settling pass
                                        // (park_settle.h) rewrites it to kQPruned or puts the candidate on the resume list
namespace quad {
// doubles of a parked candidate's record (QArgs::park_records): trunk qpos 0-6, qvel 7-12, warm start 13-18, time 19, the total BEFORE the park
// step's cost 20, the park step 21; then per leg l at 22 + 9 l: joint positions, velocities, warm start. What a candidate carries into a step
constexpr int kQParkRec = 58;
// the rollout request (RolloutArgs<double> of rollout_lane.h, flattened so that the CPU emulator can fill it too)
struct QArgs {
  int N, H, P, interp;
  const double* node_times;  // P
  double* nodes;             // [P][nu][N]
  const double* nominal;     // [P][nu]
  int noise_mode;            // -1: candidates given in `nodes`
  uint64_t seed; uint32_t iteration;
  int candidate_offset, nominal_candidate, explore_count;
  double std0, std1;
  const double* param_variance;
  double *states, *actions, *times, *residual, *costs, *trace, *total_return;  // [candidate][step][field]
  int* failure;
  long long* stamps;  // nullptr, or 64 counters: phase cycles of wavefront 0 (tuning aid, MJPCX_QUAD_STAMPS=1)
  long long* wave_times;  // nullptr, or [wavefront][4] (tuning aid, with stamps): cycles; Newton iterations run (each step the slowest candidate's); steps through the general solver; the largest per-lane contact count, summed over the steps
  long long* wave_class;  // nullptr, or [wavefront][64] (tuning aid, MJPCX_QUAD_CLASSES=1): per class of wavefront-step -- bit 0 some candidate has a contact between
                          // two moving geoms, bit 1 a leg-leg one, bit 2 some lane holds more contacts than LDS slots, bit 3 more than line-search slots --
                          // [2 c] steps, [2 c + 1] cycles in the constraint solve, [32 + 2 c] steps, [32 + 2 c + 1] cycles of the whole step
  int cpw;            // candidates per wavefront (1, 2, 4, 8 or 16: the first 4 * cpw lanes of a wavefront work; 0 = 16). Small batches spread over more wavefronts: the lock-step is over fewer candidates and every SIMD gets one
  double* ovf_slab;   // builds with QEXP_OVF_SLAB only (nullptr otherwise): per wavefront, (kQMaxCon - kQLdsSlots) x kQConRec x 64 doubles ([slot][field][lane], as the
                      // LDS store): a lane's contacts beyond the LDS slots (quad_ovf_doubles_per_wave / quad_waves: quad_launch.h)
  int con_cap;        // a lane that collects more contacts than this hands its candidate on (0: kQMaxCon, the store's capacity; MJPCX_QUAD_CON_CAP lowers it, for tests of the hand-on)
  int env_n;          // several environments in one launch (env_select.h): candidates per environment, a multiple of 64 (0: one environment) ...
  unsigned env_stride;  // ... and the bytes between the plan records of consecutive environments (node_times, nominal and the blob are environment 0's)
  unsigned model_stride, tables_stride;  // a model per environment (mjpcx_set_models_batched): the bytes between consecutive environments' QuadModel / QuadTables
                                         // records (0: the one model for every environment; the kernel's model pointers are environment 0's)
  unsigned long long* prune_bound;  // nullptr: every candidate is rolled to the horizon. Otherwise one word holding the bits of a non-negative double in RETURN units (for those the
                                    // unsigned order of the bits is the numeric order): a return some candidate of this launch has achieved, or the caller's initial bound. A
                                    // candidate whose partial return strictly exceeds it is retired (kQPruned); one that completes lowers it. rollout_quad_kernel with env_n == 0 only
  double park_hint = __builtin_huge_val();  // an UNPROVEN estimate of the launch's best return (+inf: off). A prunable candidate whose partial return strictly exceeds it, and
                      // that prune_bound does not retire, writes its record, stores its partial return, is flagged kQParked and leaves; it never touches the bound word
  double* park_records;  // [N][kQParkRec]; needed when park_hint is finite or resume_list is set
  const int* resume_list;  // nullptr: every candidate from the plan state. Otherwise rollout_quad_resume_kernel: resume_n candidate indices; each continues from its record,
  int resume_n;            // at the recorded step, with its nodes as they stand in `nodes`, pruned against prune_bound and never parked
  int* prune_stats;   // nullptr, or 4 ints: [0] candidates retired, [1] the sum of their retire steps, [2] != 0 if a step's cost was negative (the partial return is then no lower
                      // bound: the launch's pruning is invalid), [3] wavefronts all of whose candidates left before the last step
  unsigned rec_stride = 0;  // a pruned launch of several environments (mjpcx_set_pruning_batched): the bytes between consecutive environments' records (kQEnvRec*);
                            // prune_bound and prune_stats are environment 0's and move with the workgroup's environment, and park_hint is read from the record.
                            // 0: the one record of a plain launch, park_hint as given above
  const ResumeGroup* resume_groups = nullptr;  // rollout_quad_resume_kernel of such a launch: one entry per workgroup (resume_table.h); resume_list then holds a segment of
                                               // env_n entries per environment and resume_n is not read. nullptr: the one list of resume_n entries
  bool keep_bound = false;  // rank mode (mjpcx_set_prune_rank): a completed rollout leaves the bound word alone. The word then stays where the host put it (+inf: nothing is
                            // retired in the main launch) until rank_bound_kernel (rank_bound.h) writes the K-th smallest completed return into it; the resume launch prunes
                            // against that and leaves it alone too. false: a completed rollout lowers the word to its return (the bound of the argmin)
  int seed_shared = 0;      // mjpcx_rollout_noise_ensemble: every environment draws the noise stream of `seed` itself, so local candidate i is the same spline in all of
                            // them. 0: environment e draws the stream of seed + e. Read by rollout_quad_env_kernel alone, where the launcher sends such a launch
};
// an environment's record of a pruned batched launch, byte offsets: the bound word; prune_stats' four ints; the settling pass's two counts (candidates parked, candidates
// to resume); the environment's park hint. The first 32 bytes are what a plain launch keeps behind its hand-on counters, in the same order
constexpr unsigned kQEnvRecBound = 0, kQEnvRecStats = 8, kQEnvRecWords = 24, kQEnvRecHint = 32, kQEnvRec = 64;

// the feedback policy of the iLQG rollouts (FeedbackArgs of ilqg_kernels.h): nullptr members = the spline policy of QArgs
struct QFeedback {
  const double *times, *states, *actions, *gains, *improvement, *alpha;  // [Tn], [Tn][nq + nv], [Tn][nu], [Tn][nu][2 nv], [Tn][nu], [N]
  int Tn, mode, representation, use_state;  // mode 0: index policy (RolloutDiscrete, planner.cc:630-692); 1: iLQGPolicy::Action at the time (policy.cc:82-161)
};

// offsets into the per-plan blob (WaveTaskT: wave_model.h)
struct QBlob { int off_time, off_mocap, off_weight, off_normp, off_normq, off_param, off_risk, off_rreal, off_rint; };
}  // namespace quad
}  // namespace mjpcx
