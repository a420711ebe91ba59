// quademu_prune.cc -- TEST INFRASTRUCTURE: the emulator (quademu.cc, included whole) with the two words of a pruned launch
// (QArgs::prune_bound, prune_stats: quad_abi.h) as plain host memory. The step function's atomics are plain operations on the host
// (quad_step.h), and the emulator's wavefront is one quad (QArgs::cpw = 1), so "the wavefront ended early" is "the candidate left early".
// tests/test_quad_prune_emulator.py drives it.
#include "quademu.cc"

extern "C" {

// quademu_rollout with given candidates, plus: bound_bits in/out (the bits of the initial bound; the final bound afterwards), or NULL for
// an unpruned launch (both pointers null); prune_stats[4] out; nominal_candidate: the candidate that is never retired (-1: none)
int quademu_rollout_pruned(const mjpcx_model* model, const mjpcx_task* task, const double* state, double time, const double* mocap, int N, int H, int P,
                           int interp, const double* node_times, const double* node_values, int nominal_candidate, unsigned long long* bound_bits,
                           int* prune_stats, double* states, double* actions, double* times, double* residual, double* costs, double* trace,
                           double* total_return, int* failure) {
  Built* b = new Built;
  if (!build(model, task, mocap, *b).empty()) { delete b; return -1; }
  const int nu = model->nu;
  std::vector<double> nodes((size_t)P * nu * N, 0.0);  // [P][nu][N]
  for (int c = 0; c < N; c++) for (int j = 0; j < P * nu; j++) nodes[(size_t)j * N + c] = node_values[(size_t)c * P * nu + j];
  QArgs a{};
  a.N = N; a.H = H; a.P = P; a.interp = interp; a.node_times = node_times; a.nodes = nodes.data();
  a.noise_mode = -1; a.nominal_candidate = nominal_candidate; a.cpw = 1;
  a.states = states; a.actions = actions; a.times = times; a.residual = residual; a.costs = costs; a.trace = trace; a.total_return = total_return; a.failure = failure;
  a.prune_bound = bound_bits; a.prune_stats = bound_bits ? prune_stats : nullptr;
  for (int s = 0; s < b->qm.nstatic; s++) static_pose(b->qm, mocap, s, b->sp[s]);
  std::atomic<int> next{0};
  const unsigned hw = std::thread::hardware_concurrency();
  const int nquads = (int)std::max(1u, std::min(hw / 4, (unsigned)N));
  std::vector<std::thread> pool;
  for (int q = 0; q < nquads; q++)
    pool.emplace_back([&] {
      for (;;) {
        const int cand = next.fetch_add(1);
        if (cand >= N) break;
        run_quad([&](int leg) {
          QContact con[kQMaxCon];
          EmuStore cs{con};
          EmuProf pf;
          EmuM ms;
          (void)rollout<false>(b->qm, b->qt, b->sp, b->tk, state, time, a, QFeedback{}, cand, leg, cs, ms, pf);
        });
      }
    });
  for (auto& t : pool) t.join();
  delete b;
  return 0;
}

}  // extern "C"
