// resume_table.h -- the launch shape of rollout_quad_resume_kernel (quad_kernel.h), worked out on the host from the counts the settling pass
// (park_settle.h) sent back. No HIP in here: tests/test_resume_table.py compiles it for the CPU, because a mistake in this file is an
// out-of-range read on the device.
//
// A pruned launch of E environments (mjpcx_set_pruning_batched) keeps one resume list per environment: environment e's segment holds
// count[e] candidate indices. A workgroup of the resume launch stages ONE environment's model, static poses and blob, so candidates of two
// environments never share a workgroup: every environment gets whole workgroups of its own, W wavefronts of cpw candidates each, and the
// last workgroup of an environment may be partly (never wholly) empty. The table has one entry per workgroup; the grid is the sum of the
// environments' workgroup counts. E = 1 is the plain launch's shape: ceil(ceil(count / cpw) / W) workgroups.
#pragma once

namespace mjpcx { namespace quad {
// what workgroup b of the resume launch serves: slots first .. min(first + W * cpw, count) - 1 of environment env's list, of count entries
struct ResumeGroup { int env, first, count, pad; };

// candidates per wavefront from the number of resumed candidates: as many as it takes to give each of the 1024 SIMDs one wavefront, 16 at
// most and down to ONE -- the list is what is left of a launch, the machine is otherwise empty, and the candidates of a resumed wavefront
// are at different steps. (The choice between 2 and 4 per wavefront for lists of 1025 .. 4096 has not been measured on this path.)
inline int resume_cpw(long long total) {
  int cpw = 16;
  while (cpw > 1 && (total + cpw / 2 - 1) / (cpw / 2) <= 1024) cpw >>= 1;
  return cpw;
}
// wavefronts of cpw candidates that the E lists need in all (each environment's own ceil: a wavefront serves one environment)
inline long long resume_waves(const int* count, int E, int cpw) {
  long long waves = 0;
  for (int e = 0; e < E; e++) if (count[e] > 0) waves += ((long long)count[e] + cpw - 1) / cpw;
  return waves;
}
// four wavefronts per workgroup (one per SIMD of a CU, sharing one model image) once every CU has one; below that one each
inline int resume_wpg(long long waves) { return waves >= 4 * 256 ? 4 : 1; }

// Fills table[0 .. grid) (table == nullptr: counts only) and returns the grid: the number of workgroups. cap: the entries `table` has
// room for; -1 if the grid would exceed it or an argument is out of range (nothing may be launched then).
inline long long resume_table_build(const int* count, int E, int cpw, int W, ResumeGroup* table, long long cap) {
  if (E < 0 || cpw < 1 || W < 1) return -1;
  const long long per_group = (long long)cpw * W;
  long long grid = 0;
  for (int e = 0; e < E; e++) {
    if (count[e] < 0) return -1;
    for (long long first = 0; first < count[e]; first += per_group) {
      if (table) {
        if (grid >= cap) return -1;
        table[grid] = ResumeGroup{e, (int)first, count[e], 0};
      }
      grid++;
    }
  }
  return grid;
}
} }  // namespace mjpcx::quad
