/* mjpcx.h -- C ABI of the MI355X rollout-and-evaluate library (libmjpcx.so).
 *
 * This is the drop-in boundary for the batched rollout hot path of
 * google-deepmind/mujoco_mpc: everything the reference does between
 * `SamplingPlanner::Rollouts` (mjpc/planners/sampling/planner.cc:355-393) and
 * the `partial_sort` on total_return (planner.cc:184-188), i.e. N x
 * `Trajectory::Rollout` (mjpc/trajectory.cc:92-210) + `UpdateReturn`
 * (trajectory.cc:312-326), runs behind these entry points on one gfx950 GPU.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success, a negative MJPCX_E* code otherwise;
 *     no exceptions cross the boundary; `mjpcx_error_string` maps codes.
 *   - the caller owns all host buffers; the library owns device buffers inside
 *     the opaque context and deep-copies model/task at create time.
 *   - calls on ONE context are serialised by the caller (the planning thread,
 *     cf. mjpc/agent.cc:283-357); different contexts are independent.
 *   - all host-side reals are fp64 (mjtNum=double in the reference), whatever
 *     precision the device kernels compute in.
 */
#ifndef MJPCX_H_
#define MJPCX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJPCX_VERSION 1

/* ---- error codes ------------------------------------------------------- */
enum {
  MJPCX_OK = 0,
  MJPCX_EINVAL = -1,       /* bad argument / size mismatch                   */
  MJPCX_EUNSUPPORTED = -2, /* model feature / size has no device kernel      */
  MJPCX_EDEVICE = -3,      /* HIP runtime error (see mjpcx_last_hip_error)   */
  MJPCX_ENOMEM = -4,       /* host or device allocation failed               */
  MJPCX_ESTATE = -5,       /* call out of order (e.g. fetch before rollout)  */
};

/* ---- enums shared with the reference ------------------------------------ */
/* mjtJoint (MuJoCo) */
enum { MJPCX_JNT_FREE = 0, MJPCX_JNT_BALL = 1, MJPCX_JNT_SLIDE = 2, MJPCX_JNT_HINGE = 3 };
/* mjtIntegrator (MuJoCo). Euler (with implicit joint damping) and RK4 are integrated as such. IMPLICITFAST is accepted for models whose
 * only velocity-dependent smooth force is joint damping (no actuator with a velocity term in its bias, which is all this ABI carries
 * besides damping): there MuJoCo's M - h dqfrc_smooth/dqvel is M + h diag(damping), i.e. mj_implicit's update IS mj_Euler's -- the
 * context integrates with the Euler path. IMPLICIT (Coriolis derivatives) and other IMPLICITFAST models are refused by mjpcx_create. */
enum { MJPCX_INT_EULER = 0, MJPCX_INT_RK4 = 1, MJPCX_INT_IMPLICIT = 2, MJPCX_INT_IMPLICITFAST = 3 };
/* mjpc::spline::SplineInterpolation, mjpc/spline/spline.h:29-33 */
enum { MJPCX_SPLINE_ZERO = 0, MJPCX_SPLINE_LINEAR = 1, MJPCX_SPLINE_CUBIC = 2 };
/* mjpc::NormType, mjpc/norm.h:24-35 */
enum {
  MJPCX_NORM_NULL = -1, MJPCX_NORM_QUADRATIC = 0, MJPCX_NORM_L22 = 1, MJPCX_NORM_L2 = 2,
  MJPCX_NORM_COSH = 3, MJPCX_NORM_POWER_LOSS = 5, MJPCX_NORM_SMOOTH_ABS = 6,
  MJPCX_NORM_SMOOTH_ABS2 = 7, MJPCX_NORM_RECTIFY = 8,
};
/* actuator gain / bias types (mjtGain / mjtBias subset) */
enum { MJPCX_GAIN_FIXED = 0 };
enum { MJPCX_BIAS_NONE = 0, MJPCX_BIAS_AFFINE = 1 };
/* opt.disableflags bits used by the hot path (MuJoCo mjtDisableBit subset) */
enum {
  MJPCX_DSBL_CONSTRAINT = 1 << 0, MJPCX_DSBL_FRICTIONLOSS = 1 << 2, MJPCX_DSBL_LIMIT = 1 << 3, MJPCX_DSBL_CONTACT = 1 << 4,
  MJPCX_DSBL_PASSIVE = 1 << 5, MJPCX_DSBL_GRAVITY = 1 << 6, MJPCX_DSBL_CLAMPCTRL = 1 << 7,
  MJPCX_DSBL_ACTUATION = 1 << 10, MJPCX_DSBL_REFSAFE = 1 << 11, MJPCX_DSBL_EULERDAMP = 1 << 14,
};

/* Device residual functions = the `ResidualFn::Residual` overrides of the
 * reference tasks, resolved to an id at task-bake time. */
enum {
  MJPCX_RESIDUAL_PARTICLE = 1,      /* mjpc/test/testdata/particle_residual.h:33-43   */
  MJPCX_RESIDUAL_PARTICLE_COPY = 2, /* mjpc/test/agent/rollout_test.cc:37-42          */
  MJPCX_RESIDUAL_CARTPOLE = 3,      /* mjpc/tasks/cartpole/cartpole.cc:36-49          */
  MJPCX_RESIDUAL_QUADRUPED_FLAT = 4,/* mjpc/tasks/quadruped/quadruped.cc:33-226       */
  MJPCX_RESIDUAL_HUMANOID_TRACK = 5,/* mjpc/tasks/humanoid/tracking/tracking.cc:94-216 */
};

/* ---- flat model ("mjModel" subset, compiled) ----
 * Array sizes are given next to each pointer. All arrays are host memory,
 * row-major, and are deep-copied by mjpcx_create. */
typedef struct mjpcx_model {
  /* sizes */
  int32_t nq, nv, nu, na, nbody, njnt, nsite, nmocap, nuserdata;
  /* options (mjOption) */
  double timestep;
  double gravity[3];
  int32_t integrator;   /* MJPCX_INT_*                                        */
  int32_t disableflags; /* MJPCX_DSBL_* bits                                  */
  int32_t solver_iterations; /* opt.iterations (default 100)                  */
  double solver_tolerance;   /* opt.tolerance (default 1e-8)                  */
  double meaninertia;        /* stat.meaninertia                              */
  /* bodies (nbody, body 0 = world) */
  const int32_t* body_parentid; /* nbody */
  const int32_t* body_rootid;   /* nbody */
  const int32_t* body_jntnum;   /* nbody */
  const int32_t* body_jntadr;   /* nbody (-1: none) */
  const int32_t* body_dofnum;   /* nbody */
  const int32_t* body_dofadr;   /* nbody (-1: none) */
  const int32_t* body_mocapid;  /* nbody (-1: not mocap) */
  const double* body_pos;       /* nbody x 3 */
  const double* body_quat;      /* nbody x 4 */
  const double* body_ipos;      /* nbody x 3 */
  const double* body_iquat;     /* nbody x 4 */
  const double* body_mass;      /* nbody */
  const double* body_inertia;   /* nbody x 3 */
  /* joints (njnt) */
  const int32_t* jnt_type;    /* njnt */
  const int32_t* jnt_qposadr; /* njnt */
  const int32_t* jnt_dofadr;  /* njnt */
  const int32_t* jnt_bodyid;  /* njnt */
  const int32_t* jnt_limited; /* njnt */
  const double* jnt_pos;      /* njnt x 3 */
  const double* jnt_axis;     /* njnt x 3 */
  const double* jnt_stiffness;/* njnt */
  const double* jnt_range;    /* njnt x 2 */
  const double* jnt_margin;   /* njnt */
  const double* jnt_solref;   /* njnt x 2 */
  const double* jnt_solimp;   /* njnt x 5 */
  /* dofs (nv) */
  const int32_t* dof_bodyid;   /* nv */
  const int32_t* dof_jntid;    /* nv */
  const int32_t* dof_parentid; /* nv (-1: none) */
  const double* dof_armature;  /* nv */
  const double* dof_damping;   /* nv */
  const double* dof_frictionloss; /* nv */
  const double* dof_invweight0;   /* nv */
  /* reference configuration */
  const double* qpos0;       /* nq */
  const double* qpos_spring; /* nq */
  /* sites (nsite) */
  const int32_t* site_bodyid; /* nsite */
  const double* site_pos;     /* nsite x 3 */
  const double* site_quat;    /* nsite x 4 */
  /* actuators (nu): joint transmission only */
  const int32_t* actuator_trnid;      /* nu: joint id */
  const int32_t* actuator_gaintype;   /* nu */
  const int32_t* actuator_biastype;   /* nu */
  const int32_t* actuator_ctrllimited;  /* nu */
  const int32_t* actuator_forcelimited; /* nu */
  const double* actuator_gear;       /* nu (gear[0]) */
  const double* actuator_gainprm;    /* nu x 3 */
  const double* actuator_biasprm;    /* nu x 3 */
  const double* actuator_ctrlrange;  /* nu x 2 */
  const double* actuator_forcerange; /* nu x 2 */
  /* ---- contacts and constraint options (all zero / NULL for contact-free models) ---- */
  int32_t ngeom;
  int32_t nkey;
  int32_t cone;            /* opt.cone: 0 pyramidal, 1 elliptic                */
  double impratio;         /* opt.impratio                                     */
  const int32_t* geom_type;        /* ngeom, MJPCX_GEOM_* (= mjtGeom)          */
  const int32_t* geom_bodyid;      /* ngeom */
  const int32_t* geom_contype;     /* ngeom */
  const int32_t* geom_conaffinity; /* ngeom */
  const int32_t* geom_condim;      /* ngeom */
  const int32_t* geom_priority;    /* ngeom */
  const int32_t* geom_group;       /* ngeom */
  const double* geom_size;     /* ngeom x 3 */
  const double* geom_pos;      /* ngeom x 3 (body frame) */
  const double* geom_quat;     /* ngeom x 4 */
  const double* geom_friction; /* ngeom x 3 (sliding, torsional, rolling) */
  const double* geom_solref;   /* ngeom x 2 */
  const double* geom_solimp;   /* ngeom x 5 */
  const double* geom_margin;   /* ngeom */
  const double* geom_gap;      /* ngeom */
  const double* geom_solmix;   /* ngeom */
  const double* body_invweight0;  /* nbody x 2 (translational, rotational) */
  const double* body_subtreemass; /* nbody */
  const double* dof_solref;       /* nv x 2 (friction loss) */
  const double* dof_solimp;       /* nv x 5 */
  const double* key_qpos;         /* nkey x nq (residuals that read keyframes) */
  /* ---- fixed tendons (limits only), body-pair collision filter, mocap keyframes: the Humanoid class of models.
   * All zero / NULL for models without them. Spatial tendons are not supported (mjpcx_create: MJPCX_EUNSUPPORTED). */
  int32_t ntendon;
  int32_t nwrap;
  int32_t nexclude;
  const int32_t* tendon_adr;        /* ntendon: first wrap entry                                   */
  const int32_t* tendon_num;        /* ntendon: number of wrap entries                             */
  const int32_t* tendon_limited;    /* ntendon                                                     */
  const int32_t* wrap_objid;        /* nwrap: joint id (mjWRAP_JOINT entries only)                 */
  const double* wrap_prm;           /* nwrap: coefficient                                          */
  const double* tendon_range;       /* ntendon x 2                                                 */
  const double* tendon_margin;      /* ntendon                                                     */
  const double* tendon_solref_lim;  /* ntendon x 2                                                 */
  const double* tendon_solimp_lim;  /* ntendon x 5                                                 */
  const double* tendon_invweight0;  /* ntendon                                                     */
  const int32_t* exclude_signature; /* nexclude: (body1 << 16) + body2, body1 < body2 (mjModel)    */
  const int32_t* body_weldid;       /* nbody: the body this one is welded to (mjModel.body_weldid) */
  const double* key_mpos;           /* nkey x nmocap x 3 (Humanoid tracking residual)              */
} mjpcx_model;

/* moving-geom pairs (self-collision) are built for sphere and capsule geoms; other pairs are skipped */
enum { MJPCX_GEOM_PLANE = 0, MJPCX_GEOM_SPHERE = 2, MJPCX_GEOM_CAPSULE = 3, MJPCX_GEOM_CYLINDER = 5, MJPCX_GEOM_BOX = 6 };

/* ---- task / cost specification (mjpc::Task after Task::Reset,
 * mjpc/task.cc:147-248, plus the frozen ResidualFn copy of agent.cc:319) ---- */
#define MJPCX_MAX_COST_TERMS 128 /* kMaxCostTerms, mjpc/task.h:31 */
typedef struct mjpcx_task {
  int32_t residual_id;  /* MJPCX_RESIDUAL_*                                   */
  int32_t num_residual; /* Task::num_residual                                 */
  int32_t num_term;     /* Task::num_term                                     */
  int32_t num_trace;    /* Task::num_trace                                    */
  int32_t num_parameter;/* Task::parameters.size()                            */
  const int32_t* dim_norm_residual;  /* num_term */
  const int32_t* norm;               /* num_term, MJPCX_NORM_* */
  const int32_t* num_norm_parameter; /* num_term */
  const double* weight;              /* num_term */
  const double* norm_parameter;      /* sum(num_norm_parameter) */
  const double* parameters;          /* num_parameter (residual_* numerics) */
  const int32_t* trace_site;         /* num_trace: site id of sensor "trace%i", or -1 - body id for a body frame */
  double risk;                       /* Task::risk */
  /* task-specific frozen ResidualFn state (the members Transition manages and Reset resolves, e.g.
   * QuadrupedFlat::ResidualFn, quadruped.h:186-246); layout documented per residual in csrc/residuals.h */
  int32_t num_residual_int;
  int32_t num_residual_real;
  const int32_t* residual_int;
  const double* residual_real;
} mjpcx_task;

/* ---- outputs ---------------------------------------------------------------
 * One candidate trajectory in the reference's own layout (mjpc::Trajectory,
 * mjpc/trajectory.h:74-86): row-major by time. Any pointer may be NULL to skip
 * that buffer. */
typedef struct mjpcx_traj_view {
  int32_t horizon;   /* in: capacity in steps; out: trajectory length         */
  double* states;    /* horizon x dim_state                                   */
  double* actions;   /* horizon x nu                                          */
  double* times;     /* horizon                                               */
  double* residual;  /* horizon x num_residual                                */
  double* costs;     /* horizon                                               */
  double* trace;     /* horizon x 3*num_trace                                 */
  double total_return; /* out */
  int32_t failure;     /* out */
} mjpcx_traj_view;

/* Noise specification for device-side candidate generation: the counter-based
 * replacement of the function-local absl::BitGen in
 * SamplingPlanner::AddNoiseToPolicy (sampling/planner.cc:326-352) and
 * CrossEntropyPlanner::AddNoiseToPolicy (cross_entropy/planner.cc:351-385).
 * Philox4x32-10, key = (seed_lo, seed_hi), counter = (i, c, iteration, stream)
 * for global candidate i. stream 0: the four words of counter c give two 53-bit
 * uniforms u1,u2 in (0,1) and Box-Muller gives z0 = sqrt(-2 ln u1) cos(2 pi u2),
 * z1 = ... sin(...); parameter j = node*nu + actuator uses pair c = j/2, z(j%2).
 * stream 1, c = 0: u1 < 0.2 is the per-candidate Bernoulli choosing std1. */
enum {
  /* sigma(k) = 0.5*(ctrlrange_hi-lo)(k) * std, std = std0, or std1 w.p. 0.2 per
   * candidate when std1 > 0 (sampling/planner.cc:331-345) */
  MJPCX_NOISE_SAMPLING = 0,
  /* sigma(j) = max(sqrt(param_variance[j]), floor), floor = std0 (std_initial)
   * for global candidates < explore_count, else std1 (std_min); not scaled by
   * ctrlrange (cross_entropy/planner.cc:351-385, 399-405) */
  MJPCX_NOISE_CROSS_ENTROPY = 1,
};
typedef struct mjpcx_noise_spec {
  uint64_t seed;
  uint32_t iteration;        /* plan-iteration counter                          */
  int32_t mode;              /* MJPCX_NOISE_*                                   */
  int32_t candidate_offset;  /* global index of local candidate 0 (rank sharding) */
  int32_t nominal_candidate; /* global candidate left un-noised (PS: 0, planner.cc:374); -1: none (CE) */
  int32_t explore_count;     /* CE only                                         */
  double std0;
  double std1;
  const double* param_variance; /* CE only: P*nu                                */
} mjpcx_noise_spec;

typedef struct mjpcx_ctx mjpcx_ctx;

/* ---- lifecycle --------------------------------------------------------------
 * precision: 64 (fp64, the reference's mjtNum) or 32 (every rollout kernel family has a float instantiation; Trajectory
 * buffers come back as doubles either way; the iLQG entry points of the contact-model family are fp64 only). Replaces
 * Planner::Initialize/Allocate/ResizeMjData (planners/planner.cc:23-33). */
int mjpcx_create(const mjpcx_model* model, const mjpcx_task* task, int device,
                 int precision, mjpcx_ctx** out);
void mjpcx_destroy(mjpcx_ctx* ctx);
const char* mjpcx_create_error(void); /* detail of the calling thread's last failed mjpcx_create; after a successful one: "" or a
                                         non-fatal warning naming what of the model the device does not reproduce (e.g. collidable
                                         pairs of non-sphere/capsule geoms between two moving bodies, which are left out) */
const char* mjpcx_error_string(int code);
const char* mjpcx_last_error(const mjpcx_ctx* ctx); /* detail of last failure */
const char* mjpcx_kernel_name(const mjpcx_ctx* ctx); /* rollout kernel variant */

/* Planner::SetState (sampling/planner.cc:150-153, State::CopyTo
 * states/state.cc:128-135): state = [qpos,qvel,act], mocap = 7*nmocap. */
int mjpcx_set_state(mjpcx_ctx* ctx, const double* state, double time,
                    const double* mocap, const double* userdata);

/* Per-plan frozen copy of weights/parameters (BaseResidualFn::Update,
 * task.cc:112-123). Any pointer may be NULL to keep the current value. */
int mjpcx_set_task_params(mjpcx_ctx* ctx, const double* weight,
                          const double* norm_parameter, const double* parameters,
                          double risk);

/* ---- the hot path -----------------------------------------------------------
 * Roll out N candidate spline policies for `horizon` steps from the state set
 * by mjpcx_set_state and evaluate their returns. Equivalent to N x
 * Trajectory::Rollout + UpdateReturn with SamplingPolicy::Action
 * (sampling/policy.cc:52-59) as the policy. Asynchronous on the context's
 * stream; results are read with the getters below (which synchronise).
 *   node_times : P                (shared by all candidates)
 *   node_values: N x P x nu       (candidate-major, each block = the reference's
 *                                  TimeSpline values, already noised+clamped) */
int mjpcx_rollout_splines(mjpcx_ctx* ctx, int num_candidates, int horizon,
                          int num_nodes, int interpolation, const double* node_times,
                          const double* node_values);

/* Trajectory::NoisyRollout (mjpc/trajectory.cc:100-210; RobustPlanner::OptimizePolicy, planners/robust/robust_planner.cc:
 * 120-140): as mjpcx_rollout_splines, with Ornstein-Uhlenbeck force / torque noise on every body's xfrc_applied,
 * xfrc[i] <- exp(-dt / xfrc_rate) xfrc[i] + N(0, xfrc_std sqrt(1 - exp(-2 dt / xfrc_rate))) before every step (starting
 * from zero). The normals are counter-based, keyed on (seed, candidate_offset + candidate, step, entry) -- the reference's
 * absl::BitGen is unseeded, so there is no stream to reproduce. Both kernel families. Exactly:
 *   - xfrc is the model's 6 nbody array, body-major, force then torque; nbody is the MODEL's body count, the world body and
 *     bodies a kernel leaves out of its own loops (inert trailing mocap bodies) included. A kernel that skips a body skips its
 *     draws, not their counters.
 *   - The Philox4x32-10 key is (low, high word of seed); the counter of a pair is
 *       (candidate_offset + candidate, step * 3 * nbody + j, 0x58465243, 0),   j = 0 .. 3 nbody - 1,
 *     the words in this order (word 2 is "XFRC", word 3 is 0); uniforms and Box-Muller as in mjpcx_noise_spec. Entry 2 j of
 *     xfrc takes z0 of pair j, entry 2 j + 1 takes z1.
 *   - Step t = 0 .. horizon - 2 draws before its mj_step: x[t] = decay x[t - 1] + scale z, x[-1] = 0; nothing is drawn before
 *     the final mj_forward of row horizon - 1, which sees x[horizon - 2].
 *   - decay = exp(-dt / xfrc_rate), scale = xfrc_std sqrt(1 - decay^2), both formed in double on the host, dt the timestep of
 *     the mjpcx_model the context was created with (the planning timestep, agent_timestep where the task defines one -- not the
 *     XML's option timestep). A 32-bit context rounds decay and scale z to float and runs the recursion in float.
 *   - Force and torque act at the body's centre of mass (xipos), in the world frame, on every dof the body hangs under
 *     (mj_xfrcAccumulate). */
int mjpcx_rollout_splines_noisy(mjpcx_ctx* ctx, int num_candidates, int horizon, int num_nodes, int interpolation,
                                const double* node_times, const double* node_values, double xfrc_std, double xfrc_rate,
                                uint64_t seed, int candidate_offset);

/* Same, but candidates are generated on the device: nominal spline (P x nu)
 * + clamped Gaussian noise per mjpcx_noise_spec. */
int mjpcx_rollout_noise(mjpcx_ctx* ctx, int num_candidates, int horizon,
                        int num_nodes, int interpolation, const double* node_times,
                        const double* nominal_values, const mjpcx_noise_spec* noise);

/* The task-specific frozen ResidualFn state (mjpcx_task::residual_int / residual_real) for the next rollouts: what
 * Task::Transition changed since the context was created (mode, gait phase origin, Walk/Flip state of the Quadruped).
 * Either pointer may be NULL (keep). */
int mjpcx_set_residual_state(mjpcx_ctx* ctx, const int32_t* residual_int, const double* residual_real);

/* ---- several environments in one launch ---------------------------------------
 * An environment is one robot: its own state, clock, mocap pose, userdata and nominal spline. All environments of a context
 * share the model, the norm kinds and term dimensions, the horizon and the spline shape (P nodes, interpolation); the task weights,
 * norm parameters, parameters and risk are shared unless mjpcx_set_task_params_batched gives each environment its own, and the frozen
 * residual state is shared unless mjpcx_set_residual_states gives one per environment. Candidates are environment-major: global
 * candidate c = e * n_per_env + i, and every getter (mjpcx_get_returns, mjpcx_get_return_at, mjpcx_fetch_trajectory,
 * mjpcx_fetch_spline, mjpcx_device_buffer) takes the global index. The rollout kernel is chosen from the TOTAL E * n_per_env, by the
 * thresholds of the plain calls: a fleet's shares run together on the kernel a batch of that size runs on.
 *   - n_per_env must be a positive multiple of 64 (every wavefront then serves one environment) and E >= 1: MJPCX_EINVAL otherwise
 *     (mjpcx_rollout_feedback_batched alone takes any n_per_env >= 1);
 *   - a batched rollout needs a preceding mjpcx_set_states with the same E: MJPCX_EINVAL otherwise;
 *   - on a context sharded with mjpcx_comm_init (world > 1): MJPCX_EUNSUPPORTED.
 * Force noise (Trajectory::NoisyRollout) is batched too: mjpcx_rollout_splines_noisy_batched on the lane (NOISY), wave and tree kernels.
 * The quad and limb kernels draw no force noise, so a noisy batch of any size runs on the wavefront-per-candidate kernels, as the
 * plain noisy call does.
 * The plain entry points are the one-environment case of the same launch code and kernels; they keep using the state of
 * mjpcx_set_state, which mjpcx_set_states does not touch. */

/* E x Planner::SetState: states E x (nq+nv+na), times E, mocap E x 7*nmocap (NULL: every environment keeps the context's
 * pose), userdata E x nuserdata. */
int mjpcx_set_states(mjpcx_ctx* ctx, int num_envs, const double* states, const double* times, const double* mocap,
                     const double* userdata);

/* mjpcx_set_residual_state per environment (E x residual_int, E x residual_real; either may be NULL: keep), for fleets whose
 * robots are not in the same mode or gait phase. After mjpcx_set_states with the same E. A later plain
 * mjpcx_set_residual_state applies to all environments again. */
int mjpcx_set_residual_states(mjpcx_ctx* ctx, int num_envs, const int32_t* residual_int, const double* residual_real);

/* mjpcx_set_task_params per environment: weight E x num_term, norm_parameter E x (sum of num_norm_parameter), parameters
 * E x num_parameter, risk E. Any pointer may be NULL: that field is the context's (mjpcx_set_task_params) for every environment.
 * All four NULL: everything shared again. After mjpcx_set_states with the same E (MJPCX_EINVAL otherwise).
 *   - Every batched entry point reads the rows: mjpcx_rollout_splines_batched, mjpcx_rollout_splines_noisy_batched,
 *     mjpcx_rollout_noise_batched, mjpcx_rollout_noise_batched_ce, mjpcx_robust_step_batched, mjpcx_rollout_sample_gradient_batched,
 *     mjpcx_sample_gradient_update_batched, mjpcx_rollout_feedback_batched, mjpcx_gradient_step_batched, mjpcx_ilqg_step_batched and
 *     mjpcx_ilqg_step_batched_from (ctx's rows, not the source's).
 *     Environment e of such a call behaves exactly like the plain call after mjpcx_set_task_params(row e): equal bits.
 *   - mjpcx_set_task_params and the plain entry points neither read nor clear the rows: plain and batched values live side by
 *     side, as the states of mjpcx_set_state and mjpcx_set_states do (NOT the rule of mjpcx_set_residual_state above: a plain
 *     chain run for one robot between two batched launches leaves the fleet's rows alone).
 *   - Every call replaces all four fields. The rows persist across plan steps until replaced; mjpcx_set_states with a different
 *     E drops them, as it drops the per-environment residual state.
 *   - The norm kinds, the term dimensions and the model stay shared. */
int mjpcx_set_task_params_batched(mjpcx_ctx* ctx, int num_envs, const double* weight, const double* norm_parameter,
                                  const double* parameters, const double* risk);

/* A model per environment: robots of one fleet that differ PHYSICALLY (a payload, ice under the feet, weaker motors). models[e] serves
 * environment e of mjpcx_rollout_splines_batched, mjpcx_rollout_noise_batched, mjpcx_rollout_noise_batched_ce,
 * mjpcx_rollout_splines_noisy_batched, mjpcx_rollout_sample_gradient_batched and of the rollout inside mjpcx_robust_step_batched:
 * environment e of such a call behaves exactly like the plain call on a context CREATED on models[e]: equal bits.
 *   - Everything is deep-copied. Call it after mjpcx_create, between launches; it waits for the work already enqueued on the context's
 *     stream. It is a setup call: the context's builders run once per model on the host (milliseconds each) -- not for a plan loop.
 *   - models == NULL or num_envs == 0: the context's one model for every environment again (on any context: one that can hold no
 *     models has none, and the call does nothing). The models persist until replaced.
 *   - A batched call with another E than num_envs fails with MJPCX_EINVAL (unlike the task rows, nothing is dropped silently).
 *   - The plain entry points and mjpcx_kinematics keep using the context's own model.
 *   - Every model must equal the context's in all sizes, options, integer arrays and real arrays, EXCEPT
 *       inertial   body_mass, body_inertia, body_ipos
 *       passive    dof_armature, dof_damping, dof_frictionloss, jnt_stiffness
 *       actuation  actuator_gear, actuator_gainprm, actuator_biasprm
 *       contact    geom_friction, geom_solref, geom_solimp
 *       derived    body_subtreemass, body_invweight0, dof_invweight0, tendon_invweight0, meaninertia (the caller supplies them consistent)
 *     and there a value may change, but not whether it is zero, nor its sign: constraint rows, friction sets and every decision a
 *     kernel's builder takes stay equal across the fleet. A violation is MJPCX_EINVAL; the message names the environment and the field.
 *   - A model one of the context's builders refuses is MJPCX_EUNSUPPORTED, with the builder's text and the environment.
 *   - All or nothing: on any failure the context keeps what it had.
 *   - MJPCX_EUNSUPPORTED on a context of the lane-per-candidate family (its model constants are fixed when the library is built) and on
 *     one sharded with mjpcx_comm_init.
 *   - The quad, limb and registered-model kernels serve the fleet in the one launch they always make: each workgroup stages its
 *     environment's model image. The generic wavefront-per-candidate kernel (no registered configuration, RK4) reads its model through
 *     its kernel arguments and is launched once per environment instead, back to back on the context's stream.
 *   - While models are set, mjpcx_rollout_feedback_batched, mjpcx_gradient_step_batched, mjpcx_ilqg_step_batched and
 *     mjpcx_ilqg_step_batched_from fail with MJPCX_EUNSUPPORTED: the derivative chain on a model per environment is not implemented. */
int mjpcx_set_models_batched(mjpcx_ctx* ctx, int num_envs, const mjpcx_model* const* models);

/* mjpcx_rollout_splines for E environments: node_times E x P, node_values E x n_per_env x P x nu. */
int mjpcx_rollout_splines_batched(mjpcx_ctx* ctx, int num_envs, int n_per_env, int horizon, int num_nodes, int interpolation,
                                  const double* node_times, const double* node_values);

/* mjpcx_rollout_splines_noisy for E environments: node_times E x P, node_values E x n_per_env x P x nu. Environment e behaves exactly
 * like mjpcx_rollout_splines_noisy after mjpcx_set_state(state e) with seed + e and the same candidate_offset, which is local to the
 * environment (local candidate i draws the stream of candidate_offset + i) -- so E plain calls reproduce a batched one bit for bit.
 * Validation as mjpcx_rollout_splines_batched, plus xfrc_std >= 0 and xfrc_rate > 0 (MJPCX_EINVAL). */
int mjpcx_rollout_splines_noisy_batched(mjpcx_ctx* ctx, int num_envs, int n_per_env, int horizon, int num_nodes, int interpolation,
                                        const double* node_times, const double* node_values, double xfrc_std, double xfrc_rate,
                                        uint64_t seed, int candidate_offset);

/* mjpcx_rollout_noise for E environments: node_times E x P, nominal_values E x P x nu. Environment e draws exactly the noise
 * that mjpcx_rollout_noise draws with noise->seed + e and the same remaining fields; candidate_offset and nominal_candidate
 * are local to the environment -- so E plain calls reproduce a batched one. noise->param_variance (CE) is shared by all
 * environments; mjpcx_rollout_noise_batched_ce takes one row per environment. */
int mjpcx_rollout_noise_batched(mjpcx_ctx* ctx, int num_envs, int n_per_env, int horizon, int num_nodes, int interpolation,
                                const double* node_times, const double* nominal_values, const mjpcx_noise_spec* noise);

/* mjpcx_rollout_noise_batched for a cross-entropy fleet: every environment has its own variance. param_variance is E x P*nu, row e
 * for environment e; noise->mode must be MJPCX_NOISE_CROSS_ENTROPY (MJPCX_EINVAL otherwise) and noise->param_variance is ignored.
 * Environment e draws exactly the noise mjpcx_rollout_noise draws with noise->seed + e, row e as param_variance and the same
 * remaining fields; candidate_offset, nominal_candidate and explore_count are local to the environment. Validation and error
 * codes as mjpcx_rollout_noise_batched. */
int mjpcx_rollout_noise_batched_ce(mjpcx_ctx* ctx, int num_envs, int n_per_env, int horizon, int num_nodes, int interpolation,
                                   const double* node_times, const double* nominal_values, const double* param_variance,
                                   const mjpcx_noise_spec* noise);

/* The cross-entropy update, segmented: one launch and one sync give, per environment over the n_per_env returns of the last
 * batched rollout (either kind), what mjpcx_topk(n_elite + 1) without the nominal, 2 x mjpcx_elite_moments and the host's
 * divisions give for one:
 *   index (E x n_elite, LOCAL), total_return (E x n_elite): the n_elite best candidates, ascending (NaN last, ties to the lower
 *     index); local candidate skip_candidate (the nominal rollout; -1: none) is never one of them;
 *   mean (E x P*nu): the elites' spline parameters, summed in rank order in fp64 and divided by n_elite;
 *   variance (E x P*nu): the sum of (p - mean)^2 divided by n_elite - 1 (n_elite == 1: inf / NaN, as the reference);
 *   avg_return (E): the elites' mean return.
 * Any output but index may be NULL. Deterministic: two calls on the same rollout give the same bits. MJPCX_EINVAL when the last
 * rollout was not a batched one of num_envs environments, when n_elite < 1, or when n_elite exceeds the candidates of an
 * environment that are left after the skip. */
int mjpcx_ce_update_batched(mjpcx_ctx* ctx, int num_envs, int n_elite, int skip_candidate, int32_t* index, double* total_return,
                            double* mean, double* variance, double* avg_return);

/* mjpcx_best, segmented: one launch and one sync give, per environment, the argmin over its n_per_env returns (mjpcx_topk's
 * order: ties to the lower index, NaN last) as a LOCAL index -> index[E], best_return[E]; the return of local candidate ref_candidate (-1: skip) -> ref_return[E];
 * the winner's spline values -> spline_values (E x P x nu). Any output but index may be NULL. */
int mjpcx_best_batched(mjpcx_ctx* ctx, int num_envs, int ref_candidate, int32_t* index, double* best_return,
                       double* ref_return, double* spline_values);

/* The MPPI (model predictive path integral) update, segmented: where mjpcx_best_batched takes the argmin and mjpcx_ce_update_batched
 * the mean of the n_elite best, this takes the softmin -- every candidate's spline weighted by exp(-(R - R_min) / temperature). One
 * launch sequence (two kernels) and one sync, over the n_per_env stored returns R[i] and spline parameters p[i][j] (j < P*nu) of every
 * environment of the last batched rollout (mjpcx_rollout_noise_batched, _splines_batched or _noise_ensemble). The failure words are
 * not consulted, as in mjpcx_best: a failed rollout's 1e6 loses by itself. Per environment e, with lambda = temperature[e]:
 *   index, best_return: the argmin in mjpcx_topk's order (ascending, ties to the lower index, NaN last) as a LOCAL index and its
 *     return beta -- exactly what mjpcx_best_batched gives. valid = 1 iff beta is a number below +inf.
 *   w[i] = 0 if R[i] is NaN; 1 if R[i] == beta (ties at the minimum, +-0, beta = -inf); otherwise exp(-((R[i] - beta) / lambda)): one
 *     fp64 subtraction, one fp64 division by lambda, the negation and the device library's double-precision exp. valid == 0: every
 *     w[i] = 0.
 *   eta = sum w[i], Q = sum w[i]^2, S[j] = sum w[i] p[i][j]: fp64 (the node cast to double first in a 32-bit context), each over
 *     the candidates in index order in the shape of mjpcx_elite_moments' sums -- 256 strided partial sums from zero, then a halving
 *     tree; products and additions round separately (no fma); no atomics.
 *   weight_sum = eta (>= 1 when valid: the winner weighs 1), effective_samples = eta * eta / Q, mean (E x P*nu) = S[j] / eta.
 *     valid == 0: weight_sum = effective_samples = 0 and mean is the spline of ref_candidate (NaN when ref_candidate == -1).
 *   ref_return = R[ref_candidate] (-1: skipped, NaN).
 *   weights (E x n_per_env, may be NULL): every w[i].
 * Any output but index may be NULL. Deterministic: two calls on the same rollout give the same bits, and environment e's outputs do
 * not depend on num_envs or on the other environments' data. With the timer on (mjpcx_timing_reset) the call counts as one launch
 * whose first kernel is the weights kernel. Validated before any device call: MJPCX_EINVAL when the last rollout was not a batched one
 * of num_envs environments, when a temperature is not finite or is <= 0 (the message names the environment), or when ref_candidate
 * is outside -1..n_per_env-1; MJPCX_ESTATE when the last rollout was pruned (stored partial returns are no returns: the rule of
 * mjpcx_ce_update_batched); MJPCX_EUNSUPPORTED on a context sharded with mjpcx_comm_init. */
int mjpcx_mppi_update_batched(mjpcx_ctx* ctx, int num_envs, const double* temperature /* E */, int ref_candidate,
                              int32_t* index, double* best_return, double* ref_return, double* weight_sum,
                              double* effective_samples, int32_t* valid, double* mean /* E x P*nu */,
                              double* weights /* E x n or NULL */);

/* An ensemble: ONE set of n candidates rolled out under M hypotheses about one robot, in the batched launch of M environments.
 * Hypothesis h is environment h of the preceding mjpcx_set_states(M, ...): its state, its task row if mjpcx_set_task_params_batched
 * gave one, its residual state, and its model if mjpcx_set_models_batched(M, ...) gave one. The hypotheses share node_times (P),
 * nominal_values (P x nu) and the noise stream: local candidate i of every hypothesis is the same spline. Hypothesis h behaves
 * exactly like mjpcx_rollout_noise with noise->seed (NOT + h) on a context created on models[h], after mjpcx_set_state(state h) and
 * mjpcx_set_task_params(row h): equal bits in the returns, the failure words and all six Trajectory buffers.
 *   - Afterwards the context's last rollout is a batched one of M x n, hypothesis-major (candidate h * n + i): every getter,
 *     mjpcx_best_batched (the argmin per hypothesis) and mjpcx_ensemble_best work on it.
 *   - Validation and error codes as mjpcx_rollout_noise_batched: n a positive multiple of 64, mjpcx_set_states with the same M first,
 *     M models if any are set (MJPCX_EINVAL; the context keeps its last rollout), MJPCX_EUNSUPPORTED on a sharded context. Both noise
 *     modes; noise->param_variance (CE) is shared.
 *   - mjpcx_set_pruning_batched is ignored: everything is rolled out to the horizon (the score needs every return). */
int mjpcx_rollout_noise_ensemble(mjpcx_ctx* ctx, int num_hypotheses, int n, int horizon, int num_nodes, int interpolation,
                                 const double* node_times, const double* nominal_values, const mjpcx_noise_spec* noise);

/* The selection of an ensemble, one launch and one sync, over the M x n stored returns R[h][i] (candidate h * n + i) of the last
 * batched rollout. The failure words are not consulted, as in mjpcx_best: a failed rollout's 1e6 makes the candidate lose.
 *   score[i] = the mean of the `tail` largest of R[0][i] .. R[M-1][i], 1 <= tail <= M: the M values ordered descending, equal values
 *     with the lower h first, the first `tail` summed in that order in fp64 with plain adds (starting at the first) and divided by
 *     tail; NaN if any of the M values is NaN. tail = M: the mean over the hypotheses; tail = 1: the worst case; in between the
 *     tail mean (CVaR).
 *   index: the argmin of the scores in mjpcx_topk's order (ascending, ties to the lower index, NaN last) -> best_score;
 *   member_returns (M): the winner's returns R[h][index]; ref_score: the score of ref_candidate (-1: skipped, NaN);
 *   spline_values (P x nu): the winner's spline, hypothesis 0's copy; scores (n, may be NULL): every candidate's score.
 * Any output but index may be NULL. Deterministic: two calls give the same bits. MJPCX_EINVAL when the last rollout was not a
 * batched one of num_hypotheses environments, tail is outside 1..M or ref_candidate outside -1..n-1; MJPCX_EUNSUPPORTED for
 * M > MJPCX_MAX_HYPOTHESES; MJPCX_ESTATE when the last rollout was pruned (stored partial returns are no returns: the rule of
 * mjpcx_ce_update_batched). */
#define MJPCX_MAX_HYPOTHESES 32
int mjpcx_ensemble_best(mjpcx_ctx* ctx, int num_hypotheses, int tail, int ref_candidate, int32_t* index, double* best_score,
                        double* ref_score, double* member_returns, double* spline_values, double* scores);

/* The Robust planner's plan step (RobustPlanner::OptimizePolicy after the delegate's rollout) for E environments: select, replicate,
 * roll out under force noise and score, enqueued on ctx's stream behind source's (an event; nothing goes through the host), ONE sync.
 * `source` is the context of the delegate's rollout -- the same model, device and precision; its last rollout a batched one of num_envs
 * environments, of either kind -- and is left unchanged, so the winner's unperturbed trajectory stays fetchable there. ctx has had
 * mjpcx_set_states(num_envs, ...) (its own task rows are optional). Per environment:
 *   1. the k = num_candidates best of source's n_per_env returns, in the order of mjpcx_ce_update_batched(skip_candidate = -1)
 *      (ascending, ties to the lower index, NaN last) -> candidate (E x k, LOCAL index in source's rollout), candidate_return (E x k);
 *   2. every chosen spline R = repetitions times under force noise, as mjpcx_rollout_splines_noisy_batched of the replicated splines:
 *      local rollout j = rank * R + rep draws the stream (seed + e, candidate_offset + j). The share is padded to
 *      n_pad = 64 * ceil(k R / 64) rollouts with the last rank's spline; the padding is rolled out and never scored.
 *      P is source's, node_times E x P;
 *   3. per rank, from the candidate's unperturbed return, mean = (valid * mean + return) / (valid + 1) over the repetitions that
 *      did not fail, in that order of fp64 operations -> perturbed_score (E x k), valid (E x k: how many counted); the argmin with
 *      strict < from rank 0 up (the lowest rank wins a tie, a NaN never beats an earlier rank) -> best (E: rank in 0..k-1), and the
 *      winner's spline -> spline_values (E x P x nu).
 * Any output but best may be NULL. Afterwards ctx's last rollout is the batched noisy one with n_per_env = n_pad: every getter works
 * on it. A failed perturbed rollout is the planner's ordinary failure flag, not an error.
 * MJPCX_EINVAL: source == ctx; different device, precision, nq / nv / nu; source's last rollout not batched with num_envs;
 * k < 1, k > source's n_per_env or R < 1; ctx without mjpcx_set_states(num_envs); a row of node_times not strictly increasing;
 * xfrc_std < 0 or xfrc_rate <= 0. Either context sharded: MJPCX_EUNSUPPORTED. */
int mjpcx_robust_step_batched(mjpcx_ctx* ctx, mjpcx_ctx* source, int num_envs, int num_candidates, int repetitions, int horizon,
                              int interpolation, const double* node_times, double xfrc_std, double xfrc_rate, uint64_t seed,
                              int candidate_offset, int32_t* best, int32_t* candidate, double* candidate_return,
                              double* perturbed_score, int32_t* valid, double* spline_values);

/* The Sample-Gradient planner (mjpc/planners/sample_gradient/planner.cc:168-493) for E environments: two entry points per plan step, the
 * second ends in the step's ONE sync. n = n_per_env, G = num_gradient in 0..n-1, num_noisy = n - G.
 *
 * mjpcx_rollout_sample_gradient_batched replaces planner.cc:290-400 (ResamplePolicy of the gradient candidates, AddNoiseToPolicy, Rollouts):
 * a kernel writes every candidate's spline nodes on the device, then the batched rollout runs from them; nothing is read back, no sync.
 * Local candidate 0 is the nominal (nominal_values E x P x nu, as given); candidates 1..num_noisy-1 are
 * clamp(nominal + noise_exploration * z, ctrlrange), z = gaussian_pair(seed + e, local candidate, j >> 1, iteration)[j & 1] for parameter
 * j = node * nu + actuator (standard normals, not scaled by the control range); candidates num_noisy..n-1 are the gradient candidates the
 * previous mjpcx_sample_gradient_update_batched left on the device, each its own spline over that step's node times, sampled at
 * node_times by TimeSpline::Sample (zero / linear / cubic) and clamped. gradient_values (E x G x P x nu) with gradient_times (E x P)
 * uploads them instead -- after a reset, on the first step -- ; both NULL takes the device's. Environment e of a call equals a
 * one-environment call with seed + e, bit for bit. Validation and error codes as mjpcx_rollout_noise_batched, plus MJPCX_EINVAL for G
 * outside 0..n-1, noise_exploration <= 0, one of the two gradient arrays without the other, gradient_times not strictly increasing, and
 * NULL gradient arrays with G >= 1 when no update with the same E, G, P has run on this context. */
int mjpcx_rollout_sample_gradient_batched(mjpcx_ctx* ctx, int num_envs, int n_per_env, int num_gradient, int horizon, int num_nodes,
                                          int interpolation, const double* node_times, const double* nominal_values, double noise_exploration,
                                          uint64_t seed, int iteration, const double* gradient_values, const double* gradient_times);

#define MJPCX_SG_COMPUTE_WEIGHTS 1 /* recompute the shaping weights (planner.cc: return_weight_.size() != num_noisy) */
#define MJPCX_SG_ZERO_GRADIENT 2   /* the gradient of the step before is zero (after Planner::Reset) */
/* mjpcx_sample_gradient_update_batched replaces planner.cc:168-264 and 401-493 after that rollout, per environment, in one launch:
 *   - the order is ascending returns, ties to the lower index, NaN last; winner = order[0] if its return is < the nominal's, else 0
 *     -> index (E, LOCAL); winner_type 0 nominal / 1 perturbed / 2 gradient; best_return = return[winner]; nominal_return = return[0];
 *     improvement = max(nominal_return - best_return, 0); spline_values (E x P x nu) the winner's nodes as mjpcx_best_batched gives them;
 *   - for G >= 1 the gradient estimate, kept exactly as the reference has it: gradient_previous <- gradient; with
 *     MJPCX_SG_COMPUTE_WEIGHTS the weights w[i] = max(0, f0 - log(order_noisy[i] + 1)) / den - 1 / num_noisy, f0 = log(num_noisy / 2 + 1),
 *     den the sum of the numerators, from the order of the first num_noisy returns ALONE -- the logarithm takes the candidate index at
 *     sorted position i, not i -- and that step pairs them with that order; otherwise the cached weights pair with the first num_noisy
 *     entries of the order over all n candidates. gradient[j] = sum_i (w[i] / num_noisy) z[order[i]][j], fp64 in every context, z
 *     re-drawn from the counter; the nominal and the gradient candidates carry zero noise (the reference's stale noise rows after a
 *     change of G are not reproduced). Summation: partial sum t of 256 takes positions t, t + 256, ... in order; then
 *     sum[t] += sum[t + s] for s = 128, 64, ..., 1;
 *   - the next gradient candidates g < G: per parameter nominal + (-s filter) gradient + (-s (1 - filter)) gradient_previous, two
 *     rounded additions in that order, clamped, with s = LogScale(max_step, min_step, G)[g] / noise_exploration; they stay on the
 *     device with this step's node times.
 * The weights, both gradients and the candidates live in the context. gradient (E x P*nu) and every other output but index may be
 * NULL. Deterministic: two calls on the same rollout with MJPCX_SG_ZERO_GRADIENT give the same bits. MJPCX_EINVAL when the last
 * rollout was not a mjpcx_rollout_sample_gradient_batched of num_envs environments with this num_gradient, for unknown flags,
 * max_step / min_step / noise_exploration <= 0, and without MJPCX_SG_COMPUTE_WEIGHTS when no weights for this E and num_noisy exist. */
int mjpcx_sample_gradient_update_batched(mjpcx_ctx* ctx, int num_envs, int num_gradient, int flags, double filter, double max_step,
                                         double min_step, double noise_exploration, int32_t* index, int32_t* winner_type,
                                         double* best_return, double* nominal_return, double* improvement, double* spline_values,
                                         double* gradient);

/* CMA-ES (covariance matrix adaptation evolution strategy) for E environments, beside the reference's planners: the search distribution
 * N(m, sigma^2 D C D) over the d = num_nodes x nu spline parameters (j = node * nu + actuator) lives in the context and is advanced on
 * the device. D = diag(s_k), s_k = 0.5 (hi_k - lo_k) the half control range of actuator k, so sigma and C are in normalised
 * coordinates. Per environment the context holds sigma (the step size), C (d x d, symmetric), A (its lower Cholesky factor, C = A A^T),
 * the evolution paths p_sigma and p_c, and generation (the updates applied since the state was set) -- all fp64 whatever the context's
 * precision. The mean m is NOT in the context: it is the nominal spline, which the host owns and resamples at every plan step's node
 * times. A plan step is mjpcx_rollout_cma_batched, then mjpcx_cma_update_batched, which ends in the step's ONE sync; no candidate
 * spline, no normal and no covariance crosses the host.
 * The variant is the Cholesky form with positive recombination weights, no eigendecomposition. Deviations, on purpose:
 *   - the sigma path uses A^-1 where Hansen's tutorial has C^-1/2: A^-1 (m' - m) / sigma is exactly the weighted mean z_w of the
 *     ranked standard normals, so p_sigma accumulates z_w (a rotation of the tutorial's vector: the same length distribution);
 *   - C, A, the paths and sigma are not shifted in time when the node times move on between plan steps (mjpcx_ce_update_batched's
 *     variance is not either);
 *   - candidate 0, the mean itself, is rolled out and can be the argmin, but is not ranked: the update sees candidates 1..n-1.
 *
 * mjpcx_cma_set_state_batched sets the state of num_envs environments of num_params = d parameters: sigma[E]; C (E x d x d, row-major;
 * NULL: the identity), p_sigma and p_c (E x d; NULL: zeros); generation = 0. C is factored on the device by the update's routine
 * (below, with pivot_floor = 0). A setup call: it synchronises. MJPCX_EINVAL: a sigma that is not finite or is <= 0, a path or C that is
 * not finite, a C that is not symmetric (C[a][b] != C[b][a]) or not positive definite (a pivot <= 0) -- the message names the
 * environment, and no state is set afterwards --, d not a multiple of nu. MJPCX_EUNSUPPORTED: d > MJPCX_CMA_MAX_PARAMS (the message
 * names d: the dense factor is built in LDS; a separable variant for wider models is not implemented), or a sharded context. */
#define MJPCX_CMA_MAX_PARAMS 128
int mjpcx_cma_set_state_batched(mjpcx_ctx* ctx, int num_envs, int num_params, const double* sigma /* E */, const double* C,
                                const double* p_sigma, const double* p_c);
/* The state as it stands: sigma[E], generation[E], C and A (E x d x d; A has zeros above the diagonal), p_sigma and p_c (E x d). Any
 * output may be NULL. Synchronises. MJPCX_ESTATE when no state of this num_envs and num_params is set. */
int mjpcx_cma_get_state_batched(mjpcx_ctx* ctx, int num_envs, int num_params, double* sigma, int64_t* generation, double* C,
                                double* A, double* p_sigma, double* p_c);

/* The candidates, written on the device, and their batched rollout; nothing is read back, no sync. m = nominal_values (E x P x nu).
 * Local candidate 0 is m as given (not clamped). Candidate c = 1..n-1 of environment e, in fp64 with every product and sum rounded
 * on its own (no fma):
 *   z[j]  = gaussian_pair(seed + e, c, j >> 1, iteration)[j & 1]            (the counters of mjpcx_rollout_sample_gradient_batched)
 *   y[a]  = sum_{b <= a} A[a][b] * z[b], b ascending, starting from 0.0
 *   node  = clamp(m[a] + (sigma * s_k) * y[a], lo_k, hi_k), k = a % nu, s_k = 0.5 * (hi_k - lo_k), cast to the context's type.
 * Environment e of a call equals a one-environment call with seed + e, bit for bit. Afterwards the context's last rollout is a batched
 * one of E x n: every getter works on it. Validation and error codes as mjpcx_rollout_noise_batched, plus MJPCX_ESTATE when no state
 * of num_envs environments and num_nodes x nu parameters is set. mjpcx_set_pruning_batched does not apply. With the timer on
 * (mjpcx_timing_reset) the call is one launch whose first kernel is the candidate kernel: mjpcx_timing_read_main gives its time. */
int mjpcx_rollout_cma_batched(mjpcx_ctx* ctx, int num_envs, int n_per_env, int horizon, int num_nodes, int interpolation,
                              const double* node_times /* E x P */, const double* nominal_values /* E x P x nu */, uint64_t seed,
                              int iteration);

/* The constants of an update; the host computes all of them (Hansen's defaults: planners.cma_parameters), so the device only adds,
 * multiplies and divides, takes square roots and one exp. */
typedef struct mjpcx_cma_params {
  int32_t mu;            /* ranked candidates, 1..n-1 */
  const double* weights; /* mu recombination weights, each > 0, best first (summing to 1 is the caller's business) */
  double c_sigma, d_sigma, c_c, c_one, c_mu, mu_eff, chi;
  double sigma_min, sigma_max; /* sigma is clamped to this range */
  double pivot_floor;    /* a pivot of the factorisation must exceed pivot_floor * C'[a][a]; otherwise the covariance restarts */
} mjpcx_cma_params;

/* The update after mjpcx_rollout_cma_batched: one launch sequence, one sync, over the stored returns R[0..n) of every environment.
 * The state used is the context's as it stands at this call; it is advanced in place (a second call advances it again). With
 * fp64 operations in exactly this order, every product and sum rounded on its own:
 *   order    candidates 1..n-1 in mjpcx_topk's order (ascending, ties to the lower index, NaN last); (i) is the i-th of them, i < mu.
 *   valid    = none of the mu best is NaN. valid == 0: state and generation stay untouched, mean = nominal_values, sigma as it was.
 *   z_(i), y_(i)  re-drawn from the counter and multiplied as in the rollout (y_(i) unclamped).
 *   z_w[j]   = sum_i w_i * z_(i)[j] over the ranks: 256 strided partial sums from 0.0 (partial t takes ranks t, t + 256, ...), then the
 *              halving tree sum[t] += sum[t + s], s = 128 .. 1 -- the shape of mjpcx_sample_gradient_update_batched's sums.
 *   y_w[a]   = sum_{b <= a} A[a][b] * z_w[b], as above.
 *   mean[a]  = clamp(m[a] + (sigma * s_k) * y_w[a], lo_k, hi_k)
 *   p_sigma[j] <- ((1 - c_sigma) * p_sigma[j]) + (sqrt((c_sigma * (2 - c_sigma)) * mu_eff) * z_w[j])         (the host's square root)
 *   norm     = sqrt(sum_j p_sigma[j] * p_sigma[j]), j ascending from 0.0
 *   h_sigma  = [ norm / sqrt(1 - (1 - c_sigma)^(2 g)) < (1.4 + 2 / (d + 1)) * chi ], g = generation + 1      (both sides' constants the host's)
 *   p_c[a]   <- ((1 - c_c) * p_c[a]) + (h * y_w[a]), h = h_sigma ? sqrt((c_c * (2 - c_c)) * mu_eff) : 0
 *   C'[a][b] = ((decay * C[a][b]) + c_one * (p_c[a] * p_c[b])) + c_mu * S[a][b] for a >= b, mirrored, with
 *              decay = ((1 - c_one) - c_mu) [+ (c_one * c_c) * (2 - c_c) when h_sigma == 0] and
 *              S[a][b] = sum_i (w_i * y_(i)[a]) * y_(i)[b] in the tree shape above.
 *   sigma'   = clamp(sigma * exp((c_sigma / d_sigma) * ((norm / chi) - 1)), sigma_min, sigma_max)
 *   A'       by columns b = 0..d-1: acc = sum_{k < b} A'[a][k] * A'[b][k], k ascending from 0.0; s = C'[a][b] - acc; the diagonal needs
 *            s > pivot_floor * C'[b][b] and is sqrt(s); below it A'[a][b] = s / A'[b][b].
 *   restart  a failed pivot: C = A = I, both paths zero, sigma' kept, restarted = 1 (the generation still counts).
 * Outputs per environment: index (the argmin over ALL n returns, candidate 0 included, LOCAL), best_return, nominal_return = R[0],
 * improvement = max(R[0] - best_return, 0), valid, restarted, sigma (the new one), mean (E x d), order (E x mu, may be NULL). Any
 * output but index may be NULL. Deterministic, no atomics: two calls from the same state and rollout give the same bits; environment
 * e's outputs do not depend on num_envs or on the other environments. With the timer on the call counts as one launch whose first
 * kernel is the ranking. MJPCX_EINVAL: the last rollout was not a mjpcx_rollout_cma_batched of num_envs environments (or the state
 * was set for another shape since); mu outside 1..n-1; c_one + c_mu > 1; a constant or weight that is not finite or is outside its
 * range (weights, d_sigma, mu_eff, chi, sigma_min > 0; c_sigma, c_c in (0, 1]; c_one, c_mu, pivot_floor >= 0; sigma_max >= sigma_min).
 * MJPCX_ESTATE when the last rollout was pruned; MJPCX_EUNSUPPORTED on a sharded context. */
int mjpcx_cma_update_batched(mjpcx_ctx* ctx, int num_envs, const mjpcx_cma_params* params, int32_t* index, double* best_return,
                             double* nominal_return, double* improvement, int32_t* valid, int32_t* restarted, double* sigma,
                             double* mean /* E x P*nu */, int32_t* order /* E x mu or NULL */);

/* Block until everything queued on the context's stream has finished. */
int mjpcx_sync(mjpcx_ctx* ctx);

/* total_return[N], failure[N] (Trajectory::total_return / failure). failure: 0 = the rollout completed, non-zero = it
 * stopped at a warning (trajectory.cc:169-173). The wavefront-per-candidate kernels put diagnostics above the low
 * byte: (warning bits << 8) | (failing step << 16); bits: 16 = Hessian not positive definite, 32 = contact list full. */
int mjpcx_get_returns(mjpcx_ctx* ctx, double* total_return, int32_t* failure);

/* total_return / failure of one candidate (e.g. trajectory[0], the nominal,
 * for `improvement`, sampling/planner.cc:207-208). */
int mjpcx_get_return_at(mjpcx_ctx* ctx, int candidate, double* total_return, int32_t* failure);

/* Device-side selection replacing std::partial_sort (sampling/planner.cc:184):
 * indices and returns of the k best candidates, ascending, ties to the lower index, NaN (of either sign) last and among
 * themselves by index; -0.0 and +0.0 are equal and tie by index. This is the order of every selection below (mjpcx_best,
 * mjpcx_best_batched, mjpcx_ce_update_batched, the select step of mjpcx_robust_step_batched). Returns come back with the
 * bits the rollout wrote. All NaN: index 0 first. */
int mjpcx_topk(mjpcx_ctx* ctx, int k, int32_t* index, double* total_return);

/* The reads one Predictive-Sampling policy update needs, fused into one launch and one sync:
 * argmin over total_return (the first of mjpcx_topk's order: ties to the lower index, a NaN only when every return is
 * one) -> *index, *best_return; the winner's spline values
 * (P x nu, may be NULL); and the return of `ref_candidate` (the nominal, candidate 0; -1: skip)
 * for `improvement` (sampling/planner.cc:197-212, 534-543). */
int mjpcx_best(mjpcx_ctx* ctx, int ref_candidate, int32_t* index, double* best_return, double* ref_return,
               double* spline_values);

/* Cross-Entropy elite statistics (cross_entropy/planner.cc:231-270) over the spline parameters
 * of `n` local candidates: out[j] = sum_i p_ij when mean == NULL, else sum_i (p_ij - mean[j])^2,
 * j < P*nu; *sum_return = sum_i total_return_i. The caller divides (n_elite, n_elite - 1) -- and, when
 * the candidates are sharded, all-reduces the partial sums first. */
int mjpcx_elite_moments(mjpcx_ctx* ctx, int n, const int32_t* candidates, const double* mean,
                        double* out, double* sum_return);

/* Gather one candidate into the reference's Trajectory layout. */
int mjpcx_fetch_trajectory(mjpcx_ctx* ctx, int candidate, mjpcx_traj_view* out);

/* The (noised, clamped) spline values of one candidate: P x nu. This is
 * candidate_policy[i].plan of the reference (sampling/planner.cc:534-543). */
int mjpcx_fetch_spline(mjpcx_ctx* ctx, int candidate, double* node_values);

/* ---- iLQG (mjpc/planners/ilqg, model_derivatives.cc, cost_derivatives.cc) -------------------------
 * All arrays are host fp64, row-major, time-major as in the reference's std::vectors; dim_state = nq+nv,
 * ndx = 2*nv (state-derivative dimension), nr = num_residual. */

/* N candidate rollouts under a feedback policy built on a shared nominal trajectory of Tn steps.
 *   mode 0: Trajectory::RolloutDiscrete with the index policy of iLQGPlanner::ActionRollouts
 *           (ilqg/planner.cc:630-692): u = clamp(actions[t] + alpha_i * improvement[t] + gains[t] (x - states[t]))
 *   mode 1: Trajectory::Rollout with iLQGPolicy::Action (ilqg/policy.cc:82-161), representation 0 / 1 / 2 (zero-order, linear, cubic)
 *           (zero-order / linear interpolation over `times`), feedback scaled by alpha_i, applied iff use_state
 *           (FeedbackRollouts, ilqg/planner.cc:695-724)
 * gains: Tn x nu x ndx (feedback_gain), improvement: Tn x nu (action_improvement), alpha: N. */
int mjpcx_rollout_feedback(mjpcx_ctx* ctx, int num_candidates, int horizon, int mode, int representation,
                           int use_state, int nominal_horizon, const double* times, const double* states,
                           const double* actions, const double* gains, const double* improvement,
                           const double* alpha);

/* ModelDerivatives::Compute (model_derivatives.cc:45-106) = Tn x mjd_transitionFD(eps, centered): A (Tn x ndx x ndx),
 * B (Tn x ndx x nu) of the next state, C (Tn x nr x ndx), D (Tn x nr x nu) of the residual sensors. Any output may be NULL. */
int mjpcx_transition_fd(mjpcx_ctx* ctx, int nominal_horizon, const double* times, const double* states,
                        const double* actions, double eps, int centered, double* A, double* B, double* C, double* D);

/* CostDerivatives::Compute (cost_derivatives.cc:112-230) with the context's current cost specification:
 * residual (T x nr), C, D as above -> cx (T x ndx), cu (T x nu), cxx, cxu (T x ndx x nu), cuu. */
int mjpcx_cost_derivatives(mjpcx_ctx* ctx, int T, const double* residual, const double* C, const double* D,
                           double* cx, double* cu, double* cxx, double* cxu, double* cuu);

/* One Riccati sweep at regularisation mu (iLQGBackwardPass::RiccatiStep for t = T-2..0, backward_pass.cc:65-250;
 * reg_type 0 control / 1 state-control / 2 value; use_limits: box-QP on ctrlrange `limits` (nu x 2)).
 * Outputs Vx (T x n), Vxx, K = feedback_gain (T x m x n), du = action_improvement (T x m), dV[2];
 * *status = 1 on success, 0 if some Quu was not positive definite (the caller scales mu and retries,
 * ilqg/planner.cc:429-520). n <= 48, m <= 16. kernel_ms (optional): HIP-event time of the kernel. */
int mjpcx_backward_pass(mjpcx_ctx* ctx, int n, int m, int T, double mu, int reg_type, int use_limits,
                        const double* A, const double* B, const double* cx, const double* cu, const double* cxx,
                        const double* cxu, const double* cuu, const double* actions, const double* limits,
                        double* Vx, double* Vxx, double* K, double* du, double* dV, int32_t* status,
                        double* kernel_ms);

/* The Gradient planner's first-order pass (mjpc/planners/gradient): Gradient::Compute (gradient.cc:43-108) -- Vx[T-1] = cx[T-1],
 * Qx = cx[t] + A[t]^T Vx[t+1], Qu = cu[t] + B[t]^T Vx[t+1], k[t] = -Qu, Vx[t] = Qx, dV[0] += k[t] . Qu for t = T-2..0, k[T-1] = k[T-2] --
 * and its projection onto the spline parameters, gradient = M^T k (gradient/planner.cc:247-257), M the representation's spline
 * mapping (spline_mapping.cc; 0 zero-order, 1 linear, 2 cubic) from the P node_times to the first T-1 step_times. A, B, cx, cu as
 * for mjpcx_backward_pass; outputs Vx (T x n), k (T x m), dV[2] (dV[1] = 0), gradient (P x m). One launch, fp64 on every context.
 * MJPCX_EUNSUPPORTED beyond n <= 48, m <= 16, P <= 25, T <= 512; MJPCX_EINVAL for n, m, P < 1, T < 2, another representation, or
 * node_times not strictly increasing. kernel_ms (optional): HIP-event time of the kernel. */
int mjpcx_gradient_pass(mjpcx_ctx* ctx, int n, int m, int T, const double* A, const double* B, const double* cx,
                        const double* cu, int representation, int P, const double* node_times, const double* step_times,
                        double* Vx, double* k, double* dV, double* gradient, double* kernel_ms);

/* The Gradient planner's derivative chain for E environments, chained on the device after a batched rollout (mjpcx_rollout_splines_batched
 * or mjpcx_rollout_noise_batched) of num_envs environments with horizon >= T: for every environment e, local candidate `candidate` of that
 * rollout is the nominal trajectory; its times, states, actions and residual are read from the device Trajectory buffers in whichever
 * layout the rollout kernel left them -- nothing of it passes through the host. Enqueued on the context's stream:
 *   ModelDerivatives::Compute (mjpcx_transition_fd: eps, centered) at the num_eval steps of `evaluate` (strictly increasing, within
 *     [0, T); the list of model_derivatives.cc:45-106 for derivative_skip), every environment's items with that environment's record
 *     from mjpcx_set_states / mjpcx_set_residual_states (clock, mocap pose, frozen residual state), restaged by this call;
 *   their linear interpolation to all T steps (model_derivatives.cc:108-165; a step outside the list's range takes the nearest
 *     evaluated one), two products and a sum, not contracted; A, B and D of step T - 1 set to zero (gradient/planner.cc:211-216);
 *   CostDerivatives::Compute (mjpcx_cost_derivatives; cx and cu only) on the rollout's residual;
 *   Gradient::Compute with the projection M^T k (mjpcx_gradient_pass), per environment with its node times (E x P) and step times.
 * ONE sync at the end. Outputs: nominal_return (E, may be NULL), k (E x T x m), gradient (E x P x m), dV (E x 2); A (E x T x n x n),
 * B (E x T x n x m), cx (E x T x n), cu (E x T x m) are optional (NULL: they never visit the host), n = 2 nv, m = nu.
 * With every step evaluated the results equal, bit for bit, those of mjpcx_transition_fd -> mjpcx_cost_derivatives ->
 * mjpcx_gradient_pass fed with mjpcx_fetch_trajectory of the same candidates. Deterministic. Both precisions of the lane family
 * (fp32: the finite differences in fp32, the rest in fp64, as the plain calls); fp32 contexts of the wavefront-per-candidate family
 * are refused like mjpcx_transition_fd refuses them.
 * MJPCX_EINVAL: the last rollout was not a batched one of num_envs environments, candidate outside [0, n_per_env), T < 2 or beyond the
 * rollout's horizon, a bad evaluate list, eps <= 0, an unknown representation, P < 1, node times of any environment not strictly
 * increasing. MJPCX_EUNSUPPORTED: beyond n <= 48, m <= 16, P <= 25, T <= 512, 32 cost terms of 32 residuals; a context sharded with
 * mjpcx_comm_init (world > 1); fp32 contexts of the wavefront-per-candidate family. */
int mjpcx_gradient_step_batched(mjpcx_ctx* ctx, int num_envs, int candidate, int T, int num_eval, const int32_t* evaluate, double eps,
                                int centered, int representation, int P, const double* node_times, double* nominal_return, double* k,
                                double* gradient, double* dV, double* A, double* B, double* cx, double* cu);

/* iLQG's derivative chain and backward pass for E environments (the middle of iLQGPlanner::Iteration, ilqg/planner.cc:377-520, with
 * model_derivatives.cc:45-165, cost_derivatives.cc:112-230 and backward_pass.cc:65-356), chained on the device after a batched rollout of
 * num_envs environments with horizon >= T -- in practice mjpcx_rollout_feedback_batched, the nominal phase. Environment e's nominal is
 * local candidate candidate[e] of that rollout, read from the device Trajectory buffers; candidate[e] == -1: the environment takes no part.
 * Enqueued on the context's stream, in order:
 *   the gather of every environment's candidate (times, states, actions at the evaluated steps; residual and actions at all T steps);
 *   ModelDerivatives::Compute (mjpcx_transition_fd: eps, centered) at the num_eval steps of `evaluate`, every environment's items with
 *     that environment's record from mjpcx_set_states / mjpcx_set_residual_states, restaged by this call; the assembly; the
 *     interpolation to all T steps with A, B, D of step T - 1 set to zero -- the stages of mjpcx_gradient_step_batched;
 *   CostDerivatives::Compute in full (mjpcx_cost_derivatives: cx, cu, cxx, cxu, cuu) on the rollout's residual, E x T workgroups;
 *   the backward pass (mjpcx_backward_pass: reg_type, use_limits, the model's control ranges) with its regularisation retries inside
 *     the kernel, one workgroup per environment, from mu[e] and rate[e]:
 *       retries = 0; while retries < max_iter and not ok: sweep at mu; if not ok and mu <= max_reg: rate = factor > 1 ?
 *       max(rate factor, factor) : min(rate factor, factor), mu = min(max(mu rate, min_reg), max_reg), retries += 1; elif not ok: break
 *     (ilqg/planner.cc:429-520 with ScaleRegularization, backward_pass.cc:327-340).
 * Then ONE device-to-host block and ONE sync. Outputs: K (E x T x m x n), du (E x T x m), dV (E x 2) of the last sweep; status (E: 1 ok,
 * 0 failed every retry, -1 took no part); mu_out, rate_out (E: the regularisation after the retries), retries (E: the number of
 * scalings); nominal_return (E, may be NULL); optional (NULL: they never visit the host) A, B, cx, cu, cxx, cxu, cuu, Vx, Vxx, shaped as
 * the plain calls' with a leading E; n = 2 nv, m = nu. With status 0, K, du, Vx and Vxx hold the steps the sweeps reached (zero where
 * none did) and mean nothing. An environment that takes no part is computed on a copy of the first active environment's nominal and
 * ignored -- the finite-difference launch keeps its shape -- and every output of it is zero, its status -1; with no active environment
 * nothing is launched. With every step evaluated the results equal, bit for bit, those of mjpcx_transition_fd ->
 * mjpcx_cost_derivatives -> the retry loop over mjpcx_backward_pass fed with mjpcx_fetch_trajectory of the same candidates; the
 * interpolation is two products and a sum, not contracted. Deterministic. Both precisions of the lane family (fp32: the finite
 * differences in fp32, the rest in fp64, as the plain calls).
 * MJPCX_EINVAL: the last rollout was not a batched one of num_envs environments, a candidate outside [-1, n_per_env), T < 2 or beyond
 * the rollout's horizon, a bad evaluate list, eps <= 0, reg_type outside 0..2, max_iter outside [1, 64], a non-finite or non-positive
 * mu, rate or factor, min_reg / max_reg non-finite or min_reg > max_reg. MJPCX_EUNSUPPORTED: beyond n <= 48, m <= 16, T <= 512, 32 cost
 * terms of 32 residuals; a context sharded with mjpcx_comm_init (world > 1); fp32 contexts of the wavefront-per-candidate family. */
int mjpcx_ilqg_step_batched(mjpcx_ctx* ctx, int num_envs, const int32_t* candidate, int T, int num_eval, const int32_t* evaluate, double eps,
                            int centered, int reg_type, int use_limits, const double* mu, const double* rate, double factor, double min_reg,
                            double max_reg, int max_iter, double* K, double* du, double* dV, int32_t* status, double* mu_out, double* rate_out,
                            int32_t* retries, double* nominal_return, double* A, double* B, double* cx, double* cu, double* cxx, double* cxu,
                            double* cuu, double* Vx, double* Vxx);

/* mjpcx_ilqg_step_batched for a fleet whose nominals lie in TWO contexts: the middle of iLQSPlanner::OptimizePolicy
 * (ilqs/planner.cc:87-214) for E environments. In iLQS a robot whose active policy was sampling hands sampling's rollout to iLQG --
 * ilqg.candidate_policy[0].trajectory = sampling.trajectory[0] -- and that trajectory is in the device buffers of the sampling
 * context, while a robot whose active policy was iLQG has its nominal among the feedback rollouts of the iLQG context. Environment e's
 * nominal is
 *   from_source[e] == 0: local candidate candidate[e] of the last batched rollout of ctx (mjpcx_ilqg_step_batched);
 *   from_source[e] == 1: local candidate candidate[e] of the last batched rollout of `source` -- of any kind, with its own number of
 *     candidates per environment, its own horizon >= T and whichever Trajectory layout its kernel left.
 * candidate[e] == -1 keeps its meaning: the environment takes no part and rides on the first active environment's nominal, read from
 * whichever context that one names. ONE gather launch reads both sets of buffers with a per-environment selector; nothing of a nominal
 * passes through the host. Everything after the gather is mjpcx_ilqg_step_batched's chain (ilqg/planner.cc:377-520 with
 * model_derivatives.cc:45-165, cost_derivatives.cc:112-230 and backward_pass.cc:65-356) on ctx's stream, which is put behind what
 * source's stream holds at the call by an event, with ctx's plan records from mjpcx_set_states / mjpcx_set_residual_states and ctx's
 * task parameters: ONE device-to-host block, ONE sync, the same outputs.
 *   - With every from_source[e] == 0 the call is mjpcx_ilqg_step_batched, bit for bit, whatever `source` is (NULL included).
 *   - With every active environment on the source, ctx needs mjpcx_set_states of num_envs environments and no rollout of its own.
 *   - source == ctx is allowed.
 * MJPCX_EINVAL, beyond mjpcx_ilqg_step_batched's: a from_source value other than 0 or 1; source NULL while some from_source[e] == 1;
 * the two contexts differ in device, precision or in nq, nv, na, nu, nr; the last rollout of a context an active environment names was
 * not a batched one of num_envs environments, or its horizon is shorter than T; a candidate outside [-1, n_per_env) of the context its
 * environment names; ctx without mjpcx_set_states of num_envs environments. MJPCX_EUNSUPPORTED: what mjpcx_ilqg_step_batched refuses,
 * of either context (sharded with mjpcx_comm_init, fp32 on the wavefront-per-candidate family). */
int mjpcx_ilqg_step_batched_from(mjpcx_ctx* ctx, mjpcx_ctx* source, const int32_t* from_source, int num_envs, const int32_t* candidate, int T,
                                 int num_eval, const int32_t* evaluate, double eps, int centered, int reg_type, int use_limits, const double* mu,
                                 const double* rate, double factor, double min_reg, double max_reg, int max_iter, double* K, double* du,
                                 double* dV, int32_t* status, double* mu_out, double* rate_out, int32_t* retries, double* nominal_return,
                                 double* A, double* B, double* cx, double* cu, double* cxx, double* cxu, double* cuu, double* Vx, double* Vxx);

/* mjpcx_rollout_feedback for E environments in one launch: for every environment e exactly mjpcx_rollout_feedback(n_per_env, ...) with
 * row e of every array -- times E x Tn, states E x Tn x (nq+nv), actions E x Tn x nu, gains E x Tn x nu x ndx, improvement E x Tn x nu,
 * alpha E x n_per_env -- from the state, clock, mocap pose, userdata and frozen residual state mjpcx_set_states /
 * mjpcx_set_residual_states gave environment e (restaged by this call). Candidates are environment-major, c = e * n_per_env + i, and
 * every getter takes the global index afterwards. n_per_env is ANY positive number here (iLQG uses 10), not a multiple of 64: the lane
 * family pads every environment to whole wavefronts, and on the other feedback kernels a workgroup is one candidate. E plain calls
 * reproduce a batched one bit for bit. The six arrays travel through one pinned block in one H2D copy; no sync, except the one the
 * quad feedback kernel needs to read its hand-on count (candidates it hands on, of whichever environments, are rolled out by the
 * wavefront-per-candidate kernel afterwards, as in the plain call). The plain calls keep using the state of mjpcx_set_state.
 * MJPCX_EINVAL: no preceding mjpcx_set_states with the same E, E < 1, n_per_env < 1, horizon < 1, nominal_horizon < 1, mode 0 with
 * horizon > nominal_horizon, an unknown mode or representation. MJPCX_EUNSUPPORTED: a context sharded with mjpcx_comm_init (world > 1);
 * fp32 contexts of the wavefront-per-candidate family, as the plain call refuses them. */
int mjpcx_rollout_feedback_batched(mjpcx_ctx* ctx, int num_envs, int n_per_env, int horizon, int mode, int representation,
                                   int use_state, int nominal_horizon, const double* times, const double* states,
                                   const double* actions, const double* gains, const double* improvement, const double* alpha);

/* ---- measurement --------------------------------------------------------------
 * HIP-event timing of the rollout kernel on the context's own stream.
 * mjpcx_timing_reset zeroes the accumulators; mjpcx_timing_read synchronises and
 * returns the summed kernel time [ms] and launch count since the reset. */
int mjpcx_timing_reset(mjpcx_ctx* ctx);
int mjpcx_timing_read(mjpcx_ctx* ctx, double* kernel_ms, int64_t* launches);
/* The same accumulation for the rollout's FIRST kernel alone -- the one that rolls the batch out (rollout_quad_kernel, the first pass
 * of rollout_tree_kernel, the time loop of the lane family); what follows it (the pass over the candidates it handed on, the sensor
 * stage of the lane family) is in mjpcx_timing_read's total only. Call before mjpcx_timing_read (which ends the timing window). */
int mjpcx_timing_read_main(mjpcx_ctx* ctx, double* main_kernel_ms, int64_t* launches);
/* rollout_quad_kernel only (zeros otherwise): of the last rollout, [0] candidates handed to the wavefront-per-candidate kernel, then by
 * reason: [1] contact list full [2] contact between two legs [3] indefinite Hessian [4] non-finite value [5] both limits of a joint
 * [6] contact between the trunk and a leg [7] a joint beyond the range over which the geom pairs the kernel leaves out are proven
 * apart (csrc/pair_cull.h). Synchronises. */
int mjpcx_quad_stats(mjpcx_ctx* ctx, int32_t* handed_on /* 8 */);

/* ---- pruning: candidates that can no longer win the plan step are not rolled to the horizon ---------------------
 * A step's cost is >= 0 (weights >= 0, norms >= 0, the risk transform maps [0, inf) to [0, inf)), so a candidate's running
 * sum is a lower bound of its return. With pruning on, rollout_quad_kernel keeps the smallest return that a candidate of
 * the launch has completed with (the bound, starting at `initial_bound`) and retires every candidate other than the nominal
 * whose partial return STRICTLY exceeds it: it can neither be nor tie the argmin.
 *
 * Sticky. Applies to the following mjpcx_rollout_noise / mjpcx_rollout_splines launches that go to rollout_quad_kernel
 * (mjpcx_rollout_splines has no nominal: no candidate is exempt there); every other launch (the batched entry points,
 * with one environment too, the feedback rollouts, the limb, tree and lane kernel families, batches below
 * MJPCX_QUAD_MIN_N, any launch under the tuning switch MJPCX_QUAD_NO_FALLBACK) ignores it and rolls everything out.
 * A fleet prunes with mjpcx_set_pruning_batched below: a switch of its own, with a bound per environment.
 * initial_bound: +inf for normal use; a finite value is a bound the caller vouches for (some candidate's return is <= it).
 * Negative or NaN: MJPCX_EINVAL. MJPCX_PRUNE=0 in the environment, read when the context is created, makes this call do
 * nothing.
 *
 * After a pruned launch:
 *   - a retired candidate's failure is MJPCX_FAILURE_PRUNED | (retire step << 8), its total_return the partial return at
 *     that step (a lower bound of the return, strictly above the best), and its trajectory rows after that step are not
 *     written. It is not handed to another kernel and mjpcx_quad_stats does not count it. Which candidates are retired,
 *     and when, depends on the order the wavefronts finish in; every candidate not marked equals the unpruned launch's.
 *   - mjpcx_best (and mjpcx_topk with k = 1) is exact (index, returns, spline), or MJPCX_ESTATE: a step's cost was negative
 *     (partial returns were no lower bounds), or something was retired and the smallest stored return is above the final
 *     bound = min(initial_bound, the returns completed inside the launch). With +inf the latter cannot happen. With a
 *     caller's bound it happens exactly when no stored return reaches down to the bound, i.e. the bound was below every
 *     return: a wrong bound always shows, also when a candidate passed its last check under the bound and completed above
 *     it (the last step is not checked). Otherwise every retired candidate is strictly above the winner. Roll out again
 *     with pruning off after MJPCX_ESTATE.
 *   - mjpcx_topk with k > 1, mjpcx_elite_moments and mjpcx_merge_topk return MJPCX_ESTATE: their answers would depend on
 *     timing (mjpcx_set_prune_rank below gives a launch whose first K returns are exact). mjpcx_get_returns,
 *     mjpcx_fetch_trajectory and mjpcx_fetch_spline stay usable. */
#define MJPCX_FAILURE_PRUNED 0x20000000
int mjpcx_set_pruning(mjpcx_ctx* ctx, int enabled, double initial_bound);
/* Of the last rollout (zeros unless it was pruned): [0] candidates retired, [1] the sum of their retire steps, [2] != 0 if a
 * step's cost was negative, [3] wavefronts all of whose candidates left before the last step. No synchronisation: the
 * counters came back with the launch. */
int mjpcx_prune_stats(mjpcx_ctx* ctx, int64_t* out /* 4 */);

/* ---- parking: an UNPROVEN estimate of the launch's best return, used from the first step on ------------------------------
 * Pruning's bound exists only once some candidate has completed. `hint` is the caller's guess of the best return the launch
 * will find (a planner's previous best, say); nobody vouches for it. In a pruned launch a candidate other than the nominal
 * whose partial return strictly exceeds the hint, and which the proven bound does not retire, is PARKED: it saves what it
 * carries from step to step and leaves its wavefront. A settling pass on the stream right after the launch reads the final
 * bound: a parked candidate whose partial return is strictly above it is retired exactly as pruning retires (same marker,
 * same counters); every other one is resumed from its saved state in a second, smaller launch, pruned against the same
 * bound, and ends bit-identical to an uninterrupted rollout. So the hint changes no result: a good one lets the likely
 * losers leave before they slow their wavefronts, a bad one costs the remaining work of the candidates it parked, never
 * a second rollout of the batch and never MJPCX_ESTATE. All of "After a pruned launch" above holds unchanged.
 *
 * Sticky. +inf turns it off (the default); negative or NaN: MJPCX_EINVAL. Ignored unless pruning is on and applies to the
 * launch (mjpcx_set_pruning lists the launches that ignore pruning; they ignore the hint too). MJPCX_PARK=0 in the
 * environment, read when the context is created, makes this call do nothing. */
int mjpcx_set_park_hint(mjpcx_ctx* ctx, double hint);
/* Of the last rollout (zeros unless it was pruned with a hint): counts [0] candidates parked, [1] of them retired by the
 * settling pass, [2] resumed ([0] = [1] + [2]); resume_ms (may be NULL): the resume launch's time between two stream events,
 * 0 if there was none. mjpcx_prune_stats counts [1] among its retirements, and those of the resume launch too. No
 * synchronisation. */
int mjpcx_park_stats(mjpcx_ctx* ctx, int64_t* counts /* 3 */, double* resume_ms);
/* Which candidates the last rollout resumed and the step each was parked at (the first min(count, cap) of them, in the order of the
 * resume list, which is not defined). Returns the count (>= 0), or a negative error code. For tests and tools: synchronises and copies
 * candidate by candidate. */
int mjpcx_park_resumed(mjpcx_ctx* ctx, int32_t* index, int32_t* step, int cap);

/* ---- pruning and parking for a fleet: a bound, a hint and a set of counters per environment ------------------------------
 * Sticky. Applies to the following mjpcx_rollout_noise_batched launches of num_envs environments that go to
 * rollout_quad_kernel. Environment e of such a launch behaves like the plain pruned launch (mjpcx_set_pruning,
 * mjpcx_set_park_hint) of that environment alone: its bound starts at initial_bound[e] (NULL: +inf each), is lowered only
 * by returns that candidates of e complete with and is compared only with partial returns of candidates of e; its nominal
 * (the LOCAL nominal_candidate) is exempt; park_hint[e] (NULL: +inf each = no parking) parks only its own candidates, which
 * are settled against e's final bound and resumed, all environments' in one launch. No comparison crosses environments.
 *
 * What stays exact: every candidate not marked MJPCX_FAILURE_PRUNED equals the unpruned batched launch's bit for bit; a
 * retired candidate's total_return is its partial return, strictly above its environment's final bound; no hint changes
 * any result. It composes with mjpcx_set_task_params_batched and mjpcx_set_models_batched (costs stay >= 0 per
 * environment).
 *
 * After such a launch:
 *   - mjpcx_best_batched is exact per environment (local index, best return, ref return, spline), or returns MJPCX_ESTATE
 *     and names the environments in mjpcx_last_error: those where a step's cost was negative, or where something was
 *     retired and the smallest stored return is above the environment's final bound (the caller's bound was below every
 *     return) -- the two rules of mjpcx_best above, per environment. Roll out again with the switch off then.
 *   - mjpcx_ce_update_batched, mjpcx_robust_step_batched (when this context is its source),
 *     mjpcx_sample_gradient_update_batched, mjpcx_best, mjpcx_topk, mjpcx_elite_moments and mjpcx_merge_topk return
 *     MJPCX_ESTATE: their answers would depend on timing. mjpcx_get_returns, mjpcx_fetch_trajectory and
 *     mjpcx_fetch_spline stay usable.
 *   - mjpcx_prune_stats and mjpcx_park_stats report the sums over the environments, mjpcx_park_resumed global candidate
 *     indices (environment by environment).
 *
 * Negative or NaN bounds or hints: MJPCX_EINVAL. A mjpcx_rollout_noise_batched of another number of environments while
 * the switch is set: MJPCX_EINVAL (the rule of mjpcx_set_models_batched: nothing is dropped silently). enabled == 0 clears
 * the switch (the other arguments are not read). MJPCX_PRUNE=0 in the environment makes this call do nothing, MJPCX_PARK=0
 * makes it ignore the hints.
 *
 * Launches that ignore the switch and roll everything out: mjpcx_rollout_splines_batched,
 * mjpcx_rollout_noise_batched_ce (at rank 1; in rank mode, mjpcx_set_prune_rank below, it obeys the switch), the noisy, sample-gradient and feedback launches, and any launch that does not reach
 * rollout_quad_kernel (a total below MJPCX_QUAD_MIN_N, a limb, tree or lane context, MJPCX_QUAD_NO_FALLBACK). The plain
 * launches ignore it too, as the batched ones keep ignoring mjpcx_set_pruning and mjpcx_set_park_hint. */
int mjpcx_set_pruning_batched(mjpcx_ctx* ctx, int enabled, int num_envs, const double* initial_bound /* E, or NULL */,
                              const double* park_hint /* E, or NULL */);
/* Of the last rollout, per environment (zeros unless it was a pruned batched one): prune[4 e ..] as mjpcx_prune_stats,
 * park[3 e ..] as mjpcx_park_stats' counts (may be NULL), final_bound[e] the environment's bound after the launch (may be
 * NULL). No synchronisation. */
int mjpcx_prune_stats_batched(mjpcx_ctx* ctx, int num_envs, int64_t* prune /* E x 4 */, int64_t* park /* E x 3 */,
                              double* final_bound /* E */);

/* ---- rank mode: the bound of the K best, for planners that read more than the argmin -----------------------------------
 * Pruning's bound is the least completed return: "cannot be the argmin" says nothing about "cannot be an elite", which is why
 * the ranking entry points refuse a pruned launch. With rank K > 1 the bound is T, the K-th smallest return among the
 * candidates that have completed, and the launch runs in four stages on the stream:
 *   1. the main launch. The bound word starts at +inf and completed rollouts do NOT lower it, so nothing is retired here. A
 *      candidate other than the nominal whose partial return strictly exceeds the park hint is parked, as ever.
 *   2. rank_bound_kernel (csrc/rank_bound.h), one workgroup per environment: C = the candidates whose failure word is 0 and
 *      whose return is finite and >= 0 (-0.0 counts as 0; handed-on candidates have not completed: not in C). T = the K-th
 *      smallest return of C, +inf if C has fewer than K members; T goes into the environment's bound word.
 *   3. the settling pass, unchanged: parked with partial return > T: retired (MJPCX_FAILURE_PRUNED); otherwise resumed.
 *   4. the resume launch, unchanged but for leaving the word alone: it prunes against T.
 * Exact: a retired candidate's return >= its stored partial return > T, and K candidates hold returns <= T, stored and true
 * alike. So in the order of mjpcx_topk (ascending, ties to the lower index, NaN last) the first K of the stored returns are the
 * first K of the unpruned launch's, bit for bit. T is the K-th smallest of a subset of the launch, so it is >= the final K-th
 * smallest: candidates that complete later (hand-ons, resumed ones) only move the true K-th down. With several ranks each
 * settles on its own K-th, again >= the global one, so the K that mjpcx_merge_topk takes from each stay exact.
 * A completed candidate other than the nominal stayed at or below the hint up to its last check, so when C has K members T
 * lies at or close above the hint (the last step is not checked, and the nominal is exempt) and the settling pass retires the
 * parked candidates; one whose partial return lies between the hint and T is resumed and pruned against T. When the hint was
 * too low fewer than K complete, T = +inf and every parked candidate is resumed unpruned. A bad hint costs the parked
 * candidates' remaining work, never a second rollout and never a wrong answer. Without a hint nothing is parked and nothing
 * is saved.
 *
 * Sticky. rank < 1: MJPCX_EINVAL. rank == 1 (the default): everything behaves as described above. rank == K > 1 applies to
 * the launches mjpcx_set_pruning + mjpcx_set_park_hint apply to, to those mjpcx_set_pruning_batched applies to, and to
 * mjpcx_rollout_noise_batched_ce under mjpcx_set_pruning_batched (which at rank 1 keeps ignoring that switch). In rank mode a
 * finite initial_bound is MJPCX_EINVAL, here and in the two setters: nobody can vouch for a K-th return. MJPCX_PRUNE=0 and
 * MJPCX_PARK=0 keep their meaning.
 *
 * After a launch at rank K, bit-identical to the unpruned launch: mjpcx_topk(k <= K); mjpcx_merge_topk(k <= K);
 * mjpcx_elite_moments of at most K candidates none of which was retired (the first K never are); mjpcx_best /
 * mjpcx_best_batched; mjpcx_ce_update_batched with n_elite + (skip_candidate >= 0) <= K. A larger k or n_elite, the Robust
 * and Sample-Gradient updates and a negative step cost return MJPCX_ESTATE as before. mjpcx_prune_stats_batched's
 * final_bound reports T. */
int mjpcx_set_prune_rank(mjpcx_ctx* ctx, int rank);
/* For tests and tools: rank_bound_kernel over the last rollout's returns and failure words, taken as num_envs equal
 * environments. bound[e] = T of environment e at this rank (+inf: fewer than `rank` qualify). Synchronises; touches no state
 * of the last rollout, its bound words included. */
int mjpcx_rank_bound_batched(mjpcx_ctx* ctx, int num_envs, int rank, double* bound /* E */);

/* Algorithmic bytes of one candidate rollout:
 * w*[H*(dim_state+nu+1+nr+3*ntrace+1) + P*nu + P + 2]. */
int64_t mjpcx_algorithmic_bytes(const mjpcx_ctx* ctx, int horizon, int num_nodes);

/* mjData kinematics of the state last given to mjpcx_set_state (mj_kinematics, mj_comPos, mj_comVel, mj_subtreeVel), for
 * Task::Transition implementations that read them (QuadrupedFlat::TransitionLocked: torso pose, subtree centre of mass and
 * linear velocity, head site; quadruped.cc:229-391) when the host has no physics of its own. Any output may be NULL; sizes
 * follow the model (nbody x 3 / 4 / 9, nsite x 3). Contact-model kernel family only. Synchronous. */
int mjpcx_kinematics(mjpcx_ctx* ctx, double* xpos, double* xquat, double* xmat, double* xipos, double* site_xpos,
                     double* subtree_com, double* subtree_linvel);

/* Raw device pointers (for zero-copy wrapping, e.g. torch tensors feeding an
 * RCCL collective). which: 0 = total_return (N x fp64), 1 = failure (N x i32). */
int mjpcx_device_buffer(mjpcx_ctx* ctx, int which, void** ptr, size_t* bytes);

/* ---- multi-GPU: one process per GPU, candidates partitioned by rank (candidate_offset in the noise spec), ONE small
 * exchange per plan iteration over RCCL (xGMI). SURVEY.md 8b / 8e. The library resolves librccl.so.1 at the first call
 * (MJPCX_EUNSUPPORTED if it is absent); every rank must make the same sequence of collective calls.
 *   mjpcx_comm_unique_id : rank 0 only; the caller ships the 128 bytes to the other ranks (any side channel)
 *   mjpcx_comm_init      : every rank; ncclCommInitRank on the context's device
 *   mjpcx_exchange_best  : Predictive Sampling (replaces the partial_sort over one process's candidates,
 *                          sampling/planner.cc:184-188): all-gather of (best return, global index, nominal return), winner =
 *                          lowest return, ties to the lowest global index, NaN ranked last; then the winner's owner broadcasts
 *                          its n spline values. In/out: this rank's record -> the global winner's. nominal_return is rank 0's
 *                          (global candidate 0 lives there).
 *   mjpcx_merge_topk     : Cross-Entropy (cross_entropy/planner.cc:240-250): in = this rank's k best (global index, return),
 *                          unused slots index -1; out = the global k best, identical on every rank (ties by global index)
 *   mjpcx_elite_allreduce: in-place sum over the ranks of a small fp64 vector (the elite moments)
 *   mjpcx_comm_barrier   : all ranks reach it (a 1-element all-reduce + stream sync)
 */
#define MJPCX_COMM_ID_BYTES 128
int mjpcx_comm_unique_id(void* id_out);
int mjpcx_comm_init(mjpcx_ctx* ctx, const void* unique_id, int rank, int world);
int mjpcx_comm_info(const mjpcx_ctx* ctx, int* rank, int* world); /* world = 1, rank = 0 before mjpcx_comm_init */
int mjpcx_exchange_best(mjpcx_ctx* ctx, int32_t* index, double* best_return, double* nominal_return, double* spline_values, int n);
int mjpcx_merge_topk(mjpcx_ctx* ctx, int k, int64_t* index, double* total_return);
int mjpcx_elite_allreduce(mjpcx_ctx* ctx, double* values, int n);
int mjpcx_comm_barrier(mjpcx_ctx* ctx);
int mjpcx_comm_destroy(mjpcx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MJPCX_H_ */
