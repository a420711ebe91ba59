// The policy conversion of the iLQS planner (ilqs/planner.cc:90-170): spline nodes fitted to a sequence of actions by least
// squares. Row t of the mapping M holds the weights TimeSpline::Sample gives each node at step time t -- the interpolation the
// rollout kernels apply -- and M is the same for every control, so one P x P factorisation of M^T M serves all of them.
#pragma once
#include <vector>

#include "../../spline/spline.h"

namespace mjpc {

enum SplineFitStatus : int {
  kSplineFitNone = -1,                // no conversion ran
  kSplineFitOk = 0,
  kSplineFitUnreached = 1,            // some nodes reach no step time; the others solved the reduced system
  kSplineFitNotPositiveDefinite = 2,  // the (reduced) normal equations are not positive definite: nothing was written
};

class SplineFit {
 public:
  // A node is unreached when its column of M has at most this fraction of the largest column norm. Node and step times both
  // come from repeated addition, so a node past the last step can keep weights of about 1e-16 rather than exact zeros.
  static constexpr double kUnreachedTolerance = 1.0e-9;

  // values (num_nodes x nu) = argmin |M values - actions| per control, actions (num_steps x nu) at step_times; node_times strictly
  // increasing. An unreached node takes the action at the step time nearest to it (the earlier one on a tie) and the other nodes
  // fit what it leaves. With ctrlrange (nu x 2) the result is clamped to it. Returns a SplineFitStatus; on
  // kSplineFitNotPositiveDefinite `values` is left as it was. Throws std::invalid_argument on empty or unordered input.
  int Fit(spline::SplineInterpolation interpolation, int num_nodes, const double* node_times, int num_steps,
          const double* step_times, const double* actions, int nu, const double* ctrlrange, double* values);

  int num_unreached = 0;       // of the last Fit
  std::vector<int> reached;    // of the last Fit, per node

 private:
  std::vector<double> mapping_, normal_, rhs_, solution_, unit_;
  std::vector<int> index_;
};

}  // namespace mjpc
