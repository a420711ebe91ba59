// The resume launch's workgroup table (csrc/resume_table.h) on the host: a C entry for tests/test_resume_table.py, and -- with
// -DRESUME_TABLE_MAIN -- a stand-alone sweep that walks every table the way rollout_quad_resume_kernel does (quad_kernel.h: slot =
// first + wavefront * cpw + quad, served if < count) and checks each read against the lists' sizes. Built with
// -fsanitize=address,undefined the sweep also checks the builder's own stores.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mujoco_mpc_amd/csrc/resume_table.h"

using mjpcx::quad::ResumeGroup;

extern "C" {
int rt_cpw(long long total) { return mjpcx::quad::resume_cpw(total); }
long long rt_waves(const int* count, int E, int cpw) { return mjpcx::quad::resume_waves(count, E, cpw); }
int rt_wpg(long long waves) { return mjpcx::quad::resume_wpg(waves); }
// table: 4 ints per workgroup (env, first, count, 0), room for cap workgroups; returns the grid or -1
long long rt_build(const int* count, int E, int cpw, int W, int* table, long long cap) {
  return mjpcx::quad::resume_table_build(count, E, cpw, W, reinterpret_cast<ResumeGroup*>(table), cap);
}
}

#ifdef RESUME_TABLE_MAIN
// every slot of every environment's list served exactly once, by a workgroup of that environment, never past the list's count
static int walk(const std::vector<int>& count, int cpw, int W) {
  const int E = (int)count.size();
  const long long need = mjpcx::quad::resume_table_build(count.data(), E, cpw, W, nullptr, 0);
  if (need < 0) return 1;
  std::vector<ResumeGroup> table((size_t)need);   // (exactly as many entries as the grid: one more store is a heap overflow)
  if (mjpcx::quad::resume_table_build(count.data(), E, cpw, W, table.data(), need) != need) return 2;
  if (need > 0 && mjpcx::quad::resume_table_build(count.data(), E, cpw, W, table.data(), need - 1) != -1) return 3;
  std::vector<std::vector<int>> served(E);
  for (int e = 0; e < E; e++) served[e].assign(count[e], 0);
  for (long long b = 0; b < need; b++) {
    const ResumeGroup g = table[(size_t)b];
    if (g.env < 0 || g.env >= E || g.count != count[g.env] || g.first < 0 || g.first >= g.count) return 4;   // (no workgroup is wholly empty)
    for (int w = 0; w < W; w++)
      for (int quad = 0; quad < 16; quad++) {
        const int slot = g.first + w * cpw + quad;
        if (quad >= cpw || slot >= g.count) continue;
        served[g.env][slot]++;   // (the kernel's read of resume_list[env * env_n + slot])
      }
  }
  for (int e = 0; e < E; e++) for (int s : served[e]) if (s != 1) return 5;
  if (E == 1) {  // the plain path's grid
    const long long waves = ((long long)count[0] + cpw - 1) / cpw;
    if (need != (waves + W - 1) / W) return 6;
  }
  return 0;
}

int main() {
  const int cpws[] = {1, 2, 4, 8, 16}, Ws[] = {1, 4};
  std::vector<std::vector<int>> cases = {{0}, {1}, {64}, {0, 5, 7}, {5, 7, 0}, {0, 0, 0}, {1, 0, 0}, {0, 0, 1}, {63, 1, 17}, {64, 64, 64}, {2048, 0, 2047, 1}, {65, 129, 3, 0, 31}};
  unsigned s = 12345;
  for (int k = 0; k < 200; k++) {
    std::vector<int> c(1 + k % 9);
    for (int& v : c) { s = s * 1664525u + 1013904223u; v = (s >> 16) % 3 == 0 ? 0 : (int)((s >> 8) % 300); }
    cases.push_back(c);
  }
  int checked = 0;
  for (const auto& c : cases)
    for (int cpw : cpws)
      for (int W : Ws) {
        const int rc = walk(c, cpw, W);
        if (rc) { std::printf("FAILED: case of %zu environments, cpw %d, W %d: check %d\n", c.size(), cpw, W, rc); return 1; }
        checked++;
      }
  const int bad[] = {3, -1};
  if (mjpcx::quad::resume_table_build(bad, 2, 4, 1, nullptr, 0) != -1) { std::printf("FAILED: a negative count was accepted\n"); return 1; }
  std::printf("resume table: %d tables walked, all candidates served exactly once\n", checked);
  return 0;
}
#endif
