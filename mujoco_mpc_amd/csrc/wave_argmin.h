// wave_argmin.h -- the (return, index) key of the selection kernels and its reduction over a wavefront: what best_kernel, best_segmented_kernel
// (mjpcx.hip) and ensemble_best_kernel (ensemble_best.h) share.
#pragma once
#include <hip/hip_runtime.h>

namespace mjpcx {
// Keys are (return, index) with ties broken by index, so the result is deterministic.
struct RetIdx { double r; int i; };
__device__ __forceinline__ bool less_ri(const RetIdx& a, const RetIdx& b) {
  // NaN returns sort last (the reference's operator< would make the order unspecified)
  const bool an = a.r != a.r, bn = b.r != b.r;
  if (an != bn) return bn;
  if (a.r != b.r && !an) return a.r < b.r;
  return a.i < b.i;
}

// The wavefront reduction is a butterfly of (return, index) minima: the steps inside a row of 16 lanes are DPP moves (no LDS traffic) --
// quad_perm [1,0,3,2] and [2,3,0,1] leave a quad's minimum in its four lanes, row_half_mirror and row_mirror then pair whole quads and
// whole halves -- and the two steps across rows go through the LDS crossbar. less_ri is a total order (NaN last, ties to the lower
// index), so every lane ends with the same minimum whatever the pairing.
template <int CTRL> __device__ __forceinline__ RetIdx dpp_ri(const RetIdx& v) {
  RetIdx o;
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v.r), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v.r), CTRL, 0xf, 0xf, true);
  o.r = __hiloint2double(hi, lo);
  o.i = __builtin_amdgcn_update_dpp(0, v.i, CTRL, 0xf, 0xf, true);
  return o;
}
__device__ __forceinline__ RetIdx wave_argmin(RetIdx best) {  // every lane of the wavefront active
  RetIdx o;
  o = dpp_ri<0xB1>(best); if (less_ri(o, best)) best = o;   // quad_perm:[1,0,3,2]
  o = dpp_ri<0x4E>(best); if (less_ri(o, best)) best = o;   // quad_perm:[2,3,0,1]
  o = dpp_ri<0x141>(best); if (less_ri(o, best)) best = o;  // row_half_mirror
  o = dpp_ri<0x140>(best); if (less_ri(o, best)) best = o;  // row_mirror
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    o.r = __shfl_xor(best.r, off, 64);
    o.i = __shfl_xor(best.i, off, 64);
    if (less_ri(o, best)) best = o;
  }
  return best;
}
}  // namespace mjpcx
