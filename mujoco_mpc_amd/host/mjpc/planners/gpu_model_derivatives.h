// mjpc::GpuModelDerivatives -- ModelDerivatives::Compute (mjpc/planners/model_derivatives.cc:45-165) over mjpcx_transition_fd:
// the finite-difference Jacobians at every (derivative_skip + 1)-th step plus the last two, linearly interpolated in between.
// Shared by the gradient-based planners (GpuILQGPlanner, GpuGradientPlanner).
#pragma once
#include <vector>

#include "../gpu/context.h"
#include "../trajectory.h"

namespace mjpc {

class GpuModelDerivatives {
 public:
  // n = ndx, m = nu, nr = num_residual, ds = dim_state; skip = derivative_skip. The last step has no transition:
  // model_derivatives.cc:88-92 computes only C there, so A, B and D are zero at T - 1.
  void Compute(gpu::Context* ctx, const Trajectory& tr, int T, int skip, double fd_tolerance, bool centered, int n, int m, int nr,
               int ds);

  std::vector<double> A, B, C, D;  // T x n x n, T x n x m, T x nr x n, T x nr x m

 private:
  std::vector<double> eA_, eB_, eC_, eD_, etimes_, estates_, eactions_;
};

}  // namespace mjpc
