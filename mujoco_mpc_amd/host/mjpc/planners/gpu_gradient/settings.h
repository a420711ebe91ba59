// GradientPlannerSettings (mjpc/planners/gradient/settings.h)
#pragma once
namespace mjpc {
struct GradientPlannerSettings {
  int max_rollout = 1;                  // planner iterations per OptimizePolicy (the reference ships 1; so does this port)
  double min_linesearch_step = 1.0e-8;  // minimum step size for the line search
  double fd_tolerance = 1.0e-5;         // finite-difference tolerance
  double fd_mode = 0;                   // 0: one-sided, 1: centred
  int action_limits = 1;
};
}  // namespace mjpc
