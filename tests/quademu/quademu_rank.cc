// quademu_rank.cc -- TEST INFRASTRUCTURE: the emulator (quademu.cc, included whole) running the four stages of a launch in rank mode
// (QArgs::keep_bound, quad_abi.h; mjpcx_set_prune_rank) on the host: the main pass (rollout<false>) with a bound word that completions leave
// alone, the rank bound of csrc/rank_bound.h as a plain loop, the settling rule of csrc/park_settle.h as a plain loop, and the resume pass
// (rollout<false, true>) over the candidates the rule could not retire. The emulator's wavefront is one quad, so each candidate may be given
// a hint of its own, as in quademu_park.cc. tests/test_quad_rank_emulator.py drives it.
#include <algorithm>

#include "quademu.cc"

extern "C" {

// Given candidates, the bound word at +inf. rank: K. hints[N]: each candidate's park hint (+inf: never parked). con_cap: QArgs::con_cap.
// Out: prune_stats[4]; park_step[N] (-1: never parked); resumed[N] (1: went through the resume pass); counts[4] parked, retired by the
// settling rule, resumed, candidates the rank bound counted (|C|); bounds[3]: the word after the main pass, T as the settling rule read it,
// the word after the resume pass.
int quademu_rollout_ranked(const mjpcx_model* model, const mjpcx_task* task, const double* state, double time, const double* mocap, int N, int H, int P,
                           int interp, const double* node_times, const double* node_values, int nominal_candidate, int rank, const double* hints,
                           int con_cap, int* prune_stats, int* park_step, int* resumed, int* counts, double* bounds, double* states, double* actions,
                           double* times, double* residual, double* costs, double* trace, double* total_return, int* failure) {
  Built* b = new Built;
  if (!build(model, task, mocap, *b).empty()) { delete b; return -1; }
  const int nu = model->nu;
  std::vector<double> nodes((size_t)P * nu * N, 0.0);  // [P][nu][N]
  for (int c = 0; c < N; c++) for (int j = 0; j < P * nu; j++) nodes[(size_t)j * N + c] = node_values[(size_t)c * P * nu + j];
  std::vector<double> records((size_t)N * kQParkRec, 0.0);
  unsigned long long word = q_bits(__builtin_huge_val());
  QArgs a{};
  a.N = N; a.H = H; a.P = P; a.interp = interp; a.node_times = node_times; a.nodes = nodes.data();
  a.noise_mode = -1; a.nominal_candidate = nominal_candidate; a.cpw = 1; a.con_cap = con_cap;
  a.states = states; a.actions = actions; a.times = times; a.residual = residual; a.costs = costs; a.trace = trace; a.total_return = total_return; a.failure = failure;
  a.prune_bound = &word; a.prune_stats = prune_stats; a.park_records = records.data();
  a.keep_bound = true;
  for (int s = 0; s < b->qm.nstatic; s++) static_pose(b->qm, mocap, s, b->sp[s]);
  // (at most 16 threads: a GPU test runs this on a machine that reports far more CPUs than the process may use)
  const unsigned hw = std::min(std::thread::hardware_concurrency(), 16u);
  const int nquads = (int)std::max(1u, std::min(hw / 4, (unsigned)N));
  auto pass = [&](int count, auto&& one) {
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int q = 0; q < nquads; q++)
      pool.emplace_back([&] {
        for (;;) {
          const int slot = next.fetch_add(1);
          if (slot >= count) break;
          run_quad([&](int leg) {
            QContact con[kQMaxCon];
            EmuStore cs{con};
            EmuProf pf;
            EmuM ms;
            one(slot, leg, cs, ms, pf);
          });
        }
      });
    for (auto& t : pool) t.join();
  };
  pass(N, [&](int cand, int leg, EmuStore& cs, EmuM& ms, EmuProf& pf) {
    QArgs mine = a;
    mine.park_hint = hints[cand];
    (void)rollout<false>(b->qm, b->qt, b->sp, b->tk, state, time, mine, QFeedback{}, cand, leg, cs, ms, pf);
  });
  bounds[0] = q_from_bits(word);
  // the rank bound (csrc/rank_bound.h): the K-th smallest return of the candidates that completed
  std::vector<double> done;
  for (int c = 0; c < N; c++)
    if (failure[c] == 0 && total_return[c] >= 0 && total_return[c] <= 1.79769313486231570815e308) done.push_back(total_return[c] == 0 ? 0.0 : total_return[c]);
  counts[3] = (int)done.size();
  double T = __builtin_huge_val();
  if ((int)done.size() >= rank && rank >= 1) { std::nth_element(done.begin(), done.begin() + (rank - 1), done.end()); T = done[rank - 1]; }
  word = q_bits(T);
  bounds[1] = T;
  // the settling rule (csrc/park_settle.h), against that word
  counts[0] = counts[1] = counts[2] = 0;
  std::vector<int> list;
  for (int c = 0; c < N; c++) {
    park_step[c] = -1; resumed[c] = 0;
    const int f = failure[c];
    if (!(f & kQParked) || (f & (kQFallback | kQPruned))) continue;
    counts[0]++;
    park_step[c] = (f >> 8) & 0xFFFF;
    if (total_return[c] > T) { failure[c] = (f & ~kQParked) | kQPruned; prune_stats[0] += 1; prune_stats[1] += park_step[c]; counts[1]++; }
    else { list.push_back(c); resumed[c] = 1; counts[2]++; }
  }
  QArgs r = a;
  r.resume_list = list.data(); r.resume_n = (int)list.size();
  pass((int)list.size(), [&](int slot, int leg, EmuStore& cs, EmuM& ms, EmuProf& pf) {
    (void)rollout<false, true>(b->qm, b->qt, b->sp, b->tk, state, time, r, QFeedback{}, r.resume_list[slot], leg, cs, ms, pf);
  });
  bounds[2] = q_from_bits(word);
  delete b;
  return 0;
}

}  // extern "C"
