"""ctypes binding of the C ABI (include/mjpcx.h) exported by libmjpcx.so.

There is no fallback: if the HIP library is missing or fails to load, importing
the binding raises. The library is built in-tree by `__graft_entry__.build()` /
`mujoco_mpc_amd.build.build_native()`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .cstructs import (MjpcxModel, MjpcxNoiseSpec, MjpcxTask, MjpcxTrajView, PackedModel, PackedTask, as_f64p,
                       as_i32p, c_f64p, c_i32p)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmjpcx.so")

SPLINE_ZERO, SPLINE_LINEAR, SPLINE_CUBIC = 0, 1, 2
NOISE_SAMPLING, NOISE_CROSS_ENTROPY = 0, 1

# every symbol include/mjpcx.h declares
EXPORTS = [
    "mjpcx_create", "mjpcx_destroy", "mjpcx_create_error", "mjpcx_error_string", "mjpcx_last_error",
    "mjpcx_kernel_name", "mjpcx_set_state", "mjpcx_set_task_params", "mjpcx_set_residual_state", "mjpcx_rollout_splines",
    "mjpcx_rollout_noise", "mjpcx_rollout_splines_noisy", "mjpcx_kinematics", "mjpcx_sync", "mjpcx_get_returns", "mjpcx_get_return_at", "mjpcx_best", "mjpcx_topk", "mjpcx_elite_moments", "mjpcx_fetch_trajectory",
    "mjpcx_fetch_spline", "mjpcx_rollout_feedback", "mjpcx_transition_fd", "mjpcx_cost_derivatives",
    "mjpcx_backward_pass", "mjpcx_gradient_pass", "mjpcx_timing_reset", "mjpcx_timing_read", "mjpcx_timing_read_main", "mjpcx_quad_stats", "mjpcx_algorithmic_bytes",
    "mjpcx_device_buffer", "mjpcx_comm_unique_id", "mjpcx_comm_init", "mjpcx_comm_info", "mjpcx_exchange_best", "mjpcx_merge_topk",
    "mjpcx_elite_allreduce", "mjpcx_comm_barrier", "mjpcx_comm_destroy",
    "mjpcx_set_states", "mjpcx_set_residual_states", "mjpcx_set_task_params_batched", "mjpcx_rollout_splines_batched", "mjpcx_rollout_noise_batched", "mjpcx_best_batched",
    "mjpcx_rollout_noise_batched_ce", "mjpcx_ce_update_batched", "mjpcx_gradient_step_batched",
    "mjpcx_rollout_feedback_batched", "mjpcx_ilqg_step_batched", "mjpcx_ilqg_step_batched_from",
    "mjpcx_rollout_splines_noisy_batched", "mjpcx_robust_step_batched",
    "mjpcx_rollout_sample_gradient_batched", "mjpcx_sample_gradient_update_batched",
    "mjpcx_set_models_batched", "mjpcx_set_pruning", "mjpcx_prune_stats",
    "mjpcx_set_park_hint", "mjpcx_park_stats", "mjpcx_park_resumed",
    "mjpcx_set_pruning_batched", "mjpcx_prune_stats_batched",
    "mjpcx_set_prune_rank", "mjpcx_rank_bound_batched",
    "mjpcx_rollout_noise_ensemble", "mjpcx_ensemble_best",
    "mjpcx_mppi_update_batched",
    "mjpcx_cma_set_state_batched", "mjpcx_cma_get_state_batched", "mjpcx_rollout_cma_batched", "mjpcx_cma_update_batched",
]

MAX_HYPOTHESES = 32                           # MJPCX_MAX_HYPOTHESES of mjpcx_ensemble_best
SG_COMPUTE_WEIGHTS, SG_ZERO_GRADIENT = 1, 2   # MJPCX_SG_* flags of mjpcx_sample_gradient_update_batched
CMA_MAX_PARAMS = 128                          # MJPCX_CMA_MAX_PARAMS of mjpcx_cma_set_state_batched


class MjpcxCmaParams(C.Structure):
    """mjpcx_cma_params (include/mjpcx.h)"""
    _fields_ = ([("mu", C.c_int32), ("weights", C.POINTER(C.c_double))] +
                [(k, C.c_double) for k in ("c_sigma", "d_sigma", "c_c", "c_one", "c_mu", "mu_eff", "chi", "sigma_min", "sigma_max", "pivot_floor")])


CMA_CONSTANTS = tuple(f[0] for f in MjpcxCmaParams._fields_[2:])

_LIB = None


class MjpcxError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        super().__init__(f"mjpcx error {code} ({lib().mjpcx_error_string(code).decode()}): {detail}")


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build the HIP library first "
                              "(python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.mjpcx_create.argtypes = [C.POINTER(MjpcxModel), C.POINTER(MjpcxTask), C.c_int, C.c_int, C.POINTER(vp)]
        L.mjpcx_destroy.argtypes = [vp]
        L.mjpcx_destroy.restype = None
        for f in ("mjpcx_create_error",):
            getattr(L, f).restype = C.c_char_p
            getattr(L, f).argtypes = []
        L.mjpcx_error_string.restype = C.c_char_p
        L.mjpcx_error_string.argtypes = [C.c_int]
        L.mjpcx_last_error.restype = C.c_char_p
        L.mjpcx_last_error.argtypes = [vp]
        L.mjpcx_kernel_name.restype = C.c_char_p
        L.mjpcx_kernel_name.argtypes = [vp]
        L.mjpcx_set_state.argtypes = [vp, c_f64p, C.c_double, c_f64p, c_f64p]
        L.mjpcx_set_task_params.argtypes = [vp, c_f64p, c_f64p, c_f64p, C.c_double]
        L.mjpcx_set_residual_state.argtypes = [vp, c_i32p, c_f64p]
        L.mjpcx_rollout_splines.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, c_f64p, c_f64p]
        L.mjpcx_rollout_noise.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, c_f64p, c_f64p, C.POINTER(MjpcxNoiseSpec)]
        L.mjpcx_rollout_splines_noisy.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, c_f64p, c_f64p, C.c_double, C.c_double,
                                                  C.c_uint64, C.c_int]
        L.mjpcx_kinematics.argtypes = [vp] + [c_f64p] * 7
        L.mjpcx_set_states.argtypes = [vp, C.c_int, c_f64p, c_f64p, c_f64p, c_f64p]
        L.mjpcx_set_residual_states.argtypes = [vp, C.c_int, c_i32p, c_f64p]
        L.mjpcx_set_task_params_batched.argtypes = [vp, C.c_int, c_f64p, c_f64p, c_f64p, c_f64p]
        L.mjpcx_set_models_batched.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(MjpcxModel))]
        L.mjpcx_rollout_splines_batched.argtypes = [vp] + [C.c_int] * 5 + [c_f64p, c_f64p]
        L.mjpcx_rollout_splines_noisy_batched.argtypes = [vp] + [C.c_int] * 5 + [c_f64p, c_f64p, C.c_double, C.c_double, C.c_uint64, C.c_int]
        L.mjpcx_robust_step_batched.argtypes = ([vp, vp] + [C.c_int] * 5 + [c_f64p, C.c_double, C.c_double, C.c_uint64, C.c_int] +
                                                [c_i32p, c_i32p, c_f64p, c_f64p, c_i32p, c_f64p])
        L.mjpcx_rollout_noise_batched.argtypes = [vp] + [C.c_int] * 5 + [c_f64p, c_f64p, C.POINTER(MjpcxNoiseSpec)]
        L.mjpcx_rollout_sample_gradient_batched.argtypes = [vp] + [C.c_int] * 6 + [c_f64p, c_f64p, C.c_double, C.c_uint64, C.c_int, c_f64p, c_f64p]
        L.mjpcx_sample_gradient_update_batched.argtypes = ([vp] + [C.c_int] * 3 + [C.c_double] * 4 + [c_i32p, c_i32p] + [c_f64p] * 5)
        L.mjpcx_best_batched.argtypes = [vp, C.c_int, C.c_int, c_i32p, c_f64p, c_f64p, c_f64p]
        L.mjpcx_mppi_update_batched.argtypes = [vp, C.c_int, c_f64p, C.c_int, c_i32p] + [c_f64p] * 4 + [c_i32p, c_f64p, c_f64p]
        L.mjpcx_cma_set_state_batched.argtypes = [vp, C.c_int, C.c_int] + [c_f64p] * 4
        L.mjpcx_cma_get_state_batched.argtypes = [vp, C.c_int, C.c_int, c_f64p, C.POINTER(C.c_int64)] + [c_f64p] * 4
        L.mjpcx_rollout_cma_batched.argtypes = [vp] + [C.c_int] * 5 + [c_f64p, c_f64p, C.c_uint64, C.c_int]
        L.mjpcx_cma_update_batched.argtypes = ([vp, C.c_int, C.POINTER(MjpcxCmaParams), c_i32p] + [c_f64p] * 3 + [c_i32p, c_i32p, c_f64p, c_f64p,
                                                                                                                  c_i32p])
        L.mjpcx_rollout_noise_ensemble.argtypes = [vp] + [C.c_int] * 5 + [c_f64p, c_f64p, C.POINTER(MjpcxNoiseSpec)]
        L.mjpcx_ensemble_best.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_i32p] + [C.POINTER(C.c_double)] * 2 + [c_f64p] * 3
        L.mjpcx_rollout_noise_batched_ce.argtypes = [vp] + [C.c_int] * 5 + [c_f64p, c_f64p, c_f64p, C.POINTER(MjpcxNoiseSpec)]
        L.mjpcx_ce_update_batched.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_i32p, c_f64p, c_f64p, c_f64p, c_f64p]
        L.mjpcx_gradient_step_batched.argtypes = ([vp] + [C.c_int] * 4 + [c_i32p, C.c_double] + [C.c_int] * 3 + [c_f64p] * 9)
        L.mjpcx_ilqg_step_batched.argtypes = ([vp, C.c_int, c_i32p, C.c_int, C.c_int, c_i32p, C.c_double] + [C.c_int] * 3 + [c_f64p] * 2 +
                                              [C.c_double] * 3 + [C.c_int] + [c_f64p] * 3 + [c_i32p] + [c_f64p] * 2 + [c_i32p] + [c_f64p] * 10)
        L.mjpcx_ilqg_step_batched_from.argtypes = [vp, vp, c_i32p] + L.mjpcx_ilqg_step_batched.argtypes[1:]
        L.mjpcx_sync.argtypes = [vp]
        L.mjpcx_get_returns.argtypes = [vp, c_f64p, c_i32p]
        L.mjpcx_get_return_at.argtypes = [vp, C.c_int, C.POINTER(C.c_double), c_i32p]
        L.mjpcx_best.argtypes = [vp, C.c_int, c_i32p, C.POINTER(C.c_double), C.POINTER(C.c_double), c_f64p]
        L.mjpcx_topk.argtypes = [vp, C.c_int, c_i32p, c_f64p]
        L.mjpcx_elite_moments.argtypes = [vp, C.c_int, c_i32p, c_f64p, c_f64p, C.POINTER(C.c_double)]
        L.mjpcx_fetch_trajectory.argtypes = [vp, C.c_int, C.POINTER(MjpcxTrajView)]
        L.mjpcx_fetch_spline.argtypes = [vp, C.c_int, c_f64p]
        L.mjpcx_rollout_feedback.argtypes = [vp] + [C.c_int] * 6 + [c_f64p] * 6
        L.mjpcx_rollout_feedback_batched.argtypes = [vp] + [C.c_int] * 7 + [c_f64p] * 6
        L.mjpcx_transition_fd.argtypes = [vp, C.c_int, c_f64p, c_f64p, c_f64p, C.c_double, C.c_int, c_f64p, c_f64p, c_f64p, c_f64p]
        L.mjpcx_cost_derivatives.argtypes = [vp, C.c_int] + [c_f64p] * 8
        L.mjpcx_backward_pass.argtypes = ([vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int] + [c_f64p] * 14 +
                                          [c_i32p, C.POINTER(C.c_double)])
        L.mjpcx_gradient_pass.argtypes = ([vp, C.c_int, C.c_int, C.c_int] + [c_f64p] * 4 + [C.c_int, C.c_int] + [c_f64p] * 6 +
                                          [C.POINTER(C.c_double)])
        L.mjpcx_timing_reset.argtypes = [vp]
        L.mjpcx_timing_read.argtypes = [vp, c_f64p, C.POINTER(C.c_int64)]
        L.mjpcx_timing_read_main.argtypes = [vp, c_f64p, C.POINTER(C.c_int64)]
        L.mjpcx_quad_stats.argtypes = [vp, c_i32p]
        L.mjpcx_set_pruning.argtypes = [vp, C.c_int, C.c_double]
        L.mjpcx_prune_stats.argtypes = [vp, C.POINTER(C.c_int64)]
        L.mjpcx_set_park_hint.argtypes = [vp, C.c_double]
        L.mjpcx_park_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.mjpcx_park_resumed.argtypes = [vp, c_i32p, c_i32p, C.c_int]
        L.mjpcx_set_pruning_batched.argtypes = [vp, C.c_int, C.c_int, c_f64p, c_f64p]
        L.mjpcx_prune_stats_batched.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), c_f64p]
        L.mjpcx_set_prune_rank.argtypes = [vp, C.c_int]
        L.mjpcx_rank_bound_batched.argtypes = [vp, C.c_int, C.c_int, c_f64p]
        L.mjpcx_algorithmic_bytes.restype = C.c_int64
        L.mjpcx_algorithmic_bytes.argtypes = [vp, C.c_int, C.c_int]
        L.mjpcx_device_buffer.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
        _LIB = L
    return _LIB


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def make_noise_spec(seed=0, iteration=0, mode=NOISE_SAMPLING, candidate_offset=0, nominal_candidate=0,
                    explore_count=0, std0=0.1, std1=0.0, param_variance=None):
    ns = MjpcxNoiseSpec()
    ns.seed, ns.iteration, ns.mode = int(seed), int(iteration), int(mode)
    ns.candidate_offset, ns.nominal_candidate, ns.explore_count = int(candidate_offset), int(nominal_candidate), int(explore_count)
    ns.std0, ns.std1 = float(std0), float(std1)
    keep = None
    if param_variance is not None:
        keep = _f(param_variance).reshape(-1)
        ns.param_variance = as_f64p(keep)
    ns._keep = keep
    return ns


class Trajectory:
    """mjpc::Trajectory buffers in the reference layout (mjpc/trajectory.h:74-86)."""

    def __init__(self, dim_state, nu, nr, ntrace, horizon):
        self.horizon = horizon
        self.dim_state, self.dim_action, self.dim_residual, self.dim_trace = dim_state, nu, nr, 3 * ntrace
        self.states = np.zeros((horizon, dim_state))
        self.actions = np.zeros((horizon, nu))
        self.times = np.zeros(horizon)
        self.residual = np.zeros((horizon, nr))
        self.costs = np.zeros(horizon)
        self.trace = np.zeros((horizon, 3 * ntrace))
        self.total_return = 0.0
        self.failure = False


class Context:
    """One (model, task, device) rollout context = `mjpcx_ctx`."""

    def __init__(self, packed_model: PackedModel, packed_task: PackedTask, device=0, precision=64):
        self._pm, self._pt = packed_model, packed_task
        self.handle = C.c_void_p()
        rc = lib().mjpcx_create(packed_model.ptr, packed_task.ptr, int(device), int(precision), C.byref(self.handle))
        if rc != 0:
            raise MjpcxError(rc, lib().mjpcx_create_error().decode())
        self.create_warning = lib().mjpcx_create_error().decode()  # "" or what of the model the device does not reproduce
        m, t = packed_model.struct, packed_task.struct
        self.nq, self.nv, self.nu, self.na = m.nq, m.nv, m.nu, m.na
        self.dim_state = m.nq + m.nv + m.na
        self.num_residual, self.num_trace = t.num_residual, t.num_trace
        self.precision = precision
        self.device = device
        self.N = self.H = self.P = 0

    def close(self):
        if self.handle:
            lib().mjpcx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MjpcxError(rc, lib().mjpcx_last_error(self.handle).decode())

    @property
    def kernel_name(self):
        return lib().mjpcx_kernel_name(self.handle).decode()

    def set_state(self, state, time=0.0, mocap=None, userdata=None):
        st = _f(state)
        assert st.size == self.dim_state
        mc = None if mocap is None else as_f64p(_f(mocap))
        ud = None if userdata is None else as_f64p(_f(userdata))
        self._chk(lib().mjpcx_set_state(self.handle, as_f64p(st), float(time), mc, ud))

    def set_task_params(self, weight=None, norm_parameter=None, parameters=None, risk=0.0):
        w = None if weight is None else as_f64p(_f(weight))
        n = None if norm_parameter is None else as_f64p(_f(norm_parameter))
        p = None if parameters is None else as_f64p(_f(parameters))
        self._chk(lib().mjpcx_set_task_params(self.handle, w, n, p, float(risk)))

    def set_residual_state(self, residual_int=None, residual_real=None):
        ri = None if residual_int is None else np.ascontiguousarray(residual_int, dtype=np.int32)
        rr = None if residual_real is None else _f(residual_real)
        self._chk(lib().mjpcx_set_residual_state(self.handle, None if ri is None else ri.ctypes.data_as(c_i32p),
                                                 None if rr is None else as_f64p(rr)))

    def rollout_splines(self, horizon, interp, node_times, node_values):
        nt = _f(node_times)
        nv = _f(node_values)
        P = nt.size
        N = nv.size // (P * self.nu)
        assert nv.size == N * P * self.nu
        self._chk(lib().mjpcx_rollout_splines(self.handle, N, int(horizon), P, int(interp), as_f64p(nt), as_f64p(nv)))
        self.N, self.H, self.P = N, int(horizon), P

    def rollout_splines_noisy(self, horizon, interp, node_times, node_values, xfrc_std, xfrc_rate, seed=0, candidate_offset=0):
        """Trajectory::NoisyRollout for every candidate spline (Ornstein-Uhlenbeck xfrc_applied noise)."""
        nt = _f(node_times)
        nv = _f(node_values)
        P = nt.size
        N = nv.size // (P * self.nu)
        assert nv.size == N * P * self.nu
        self._chk(lib().mjpcx_rollout_splines_noisy(self.handle, N, int(horizon), P, int(interp), as_f64p(nt), as_f64p(nv),
                                                    float(xfrc_std), float(xfrc_rate), int(seed), int(candidate_offset)))
        self.N, self.H, self.P = N, int(horizon), P

    def kinematics(self, nbody, nsite):
        """mjData kinematics of the state given to set_state: dict of xpos, xquat, xmat, xipos, site_xpos, subtree_com, subtree_linvel."""
        out = dict(xpos=np.zeros((nbody, 3)), xquat=np.zeros((nbody, 4)), xmat=np.zeros((nbody, 9)), xipos=np.zeros((nbody, 3)),
                   site_xpos=np.zeros((nsite, 3)), subtree_com=np.zeros((nbody, 3)), subtree_linvel=np.zeros((nbody, 3)))
        self._chk(lib().mjpcx_kinematics(self.handle, *[as_f64p(out[k]) for k in ("xpos", "xquat", "xmat", "xipos", "site_xpos", "subtree_com",
                                                                                   "subtree_linvel")]))
        return out

    def rollout_noise(self, num_candidates, horizon, interp, node_times, nominal, noise_spec):
        nt, nom = _f(node_times), _f(nominal)
        P = nt.size
        assert nom.size == P * self.nu
        self._chk(lib().mjpcx_rollout_noise(self.handle, int(num_candidates), int(horizon), P, int(interp),
                                            as_f64p(nt), as_f64p(nom), C.byref(noise_spec)))
        self.N, self.H, self.P = int(num_candidates), int(horizon), P

    # ---- several environments in one launch (candidates environment-major: global c = e * n_per_env + i)
    def set_states(self, states, times, mocap=None, userdata=None):
        """E x set_state: states E x dim_state, times E, mocap E x 7*nmocap (None: the context's pose for all)."""
        st = _f(states).reshape(-1, self.dim_state)
        E = st.shape[0]
        tm = _f(times).reshape(-1)
        assert tm.size == E
        mc = None if mocap is None else _f(mocap).reshape(E, -1)
        ud = None if userdata is None else _f(userdata).reshape(E, -1)
        self._chk(lib().mjpcx_set_states(self.handle, E, as_f64p(st), as_f64p(tm), None if mc is None else as_f64p(mc),
                                         None if ud is None else as_f64p(ud)))
        self.E = E

    def set_residual_states(self, residual_int=None, residual_real=None):
        """set_residual_state per environment: E x residual_int, E x residual_real (None: keep)."""
        ri = None if residual_int is None else np.ascontiguousarray(residual_int, dtype=np.int32)
        rr = None if residual_real is None else _f(residual_real)
        E = (ri if ri is not None else rr).shape[0] if (ri is not None or rr is not None) else getattr(self, "E", 0)
        self._chk(lib().mjpcx_set_residual_states(self.handle, int(E), None if ri is None else ri.ctypes.data_as(c_i32p),
                                                  None if rr is None else as_f64p(rr)))

    def set_task_params_batched(self, weight=None, norm_parameter=None, parameters=None, risk=None):
        """set_task_params per environment of the last set_states: weight E x num_term, norm_parameter E x (sum of num_norm_parameter),
        parameters E x num_parameter, risk E. None: that field is the context's (set_task_params) for every environment; all four
        None: everything shared again. Only the batched calls read the rows; they persist until replaced."""
        E = int(getattr(self, "E", 0))
        arrs = []
        for name, a, ndim in (("weight", weight, 2), ("norm_parameter", norm_parameter, 2), ("parameters", parameters, 2), ("risk", risk, 1)):
            if a is not None:
                a = _f(a)
                if a.ndim != ndim or a.shape[0] != E:
                    raise ValueError(f"set_task_params_batched: {name} has shape {a.shape} for the {E} environments of set_states")
                if a.size == 0:
                    a = None
            arrs.append(a)
        t = self._pt.struct
        want = (t.num_term, int(sum(t.num_norm_parameter[k] for k in range(t.num_term))), t.num_parameter)
        for name, a, n in zip(("weight", "norm_parameter", "parameters"), arrs, want):
            if a is not None and a.shape[1] != n:
                raise ValueError(f"set_task_params_batched: {name} has {a.shape[1]} columns, the task has {n}")
        self._chk(lib().mjpcx_set_task_params_batched(self.handle, E, *[None if a is None else as_f64p(a) for a in arrs]))

    def set_models_batched(self, packed_models):
        """A model per environment (mjpcx_set_models_batched): one PackedModel per environment of the batched rollouts, each the context's
        model but for its inertial, passive, actuation and contact parameters (mjcf.variant). None, or an empty list: the context's one model
        for every environment again. A setup call (the builders run once per model on the host); the models persist until replaced."""
        models = list(packed_models) if packed_models is not None else []
        if not models:
            self._chk(lib().mjpcx_set_models_batched(self.handle, 0, None))
            return
        ptrs = (C.POINTER(MjpcxModel) * len(models))(*[C.pointer(pm.struct) for pm in models])
        self._chk(lib().mjpcx_set_models_batched(self.handle, len(models), ptrs))

    def rollout_splines_batched(self, horizon, interp, node_times, node_values, num_envs=None, n_per_env=None):
        """node_times E x P, node_values E x n_per_env x P x nu."""
        nt = _f(node_times)
        nv = _f(node_values)
        E = int(num_envs) if num_envs is not None else (nt.shape[0] if nt.ndim == 2 else 1)
        P = nt.size // E if E > 0 else nt.size
        n = int(n_per_env) if n_per_env is not None else nv.size // max(E * P * self.nu, 1)
        assert nv.size == E * n * P * self.nu
        self._chk(lib().mjpcx_rollout_splines_batched(self.handle, E, n, int(horizon), P, int(interp), as_f64p(nt), as_f64p(nv)))
        self.N, self.H, self.P, self.n_per_env = E * n, int(horizon), P, n

    def rollout_splines_noisy_batched(self, horizon, interp, node_times, node_values, xfrc_std, xfrc_rate, seed=0, candidate_offset=0,
                                      num_envs=None, n_per_env=None):
        """rollout_splines_noisy for E environments: node_times E x P, node_values E x n_per_env x P x nu; environment e draws the
        force noise of a plain call with seed + e, candidate_offset local to the environment."""
        nt = _f(node_times)
        nv = _f(node_values)
        E = int(num_envs) if num_envs is not None else (nt.shape[0] if nt.ndim == 2 else 1)
        P = nt.size // E if E > 0 else nt.size
        n = int(n_per_env) if n_per_env is not None else nv.size // max(E * P * self.nu, 1)
        assert nv.size == E * n * P * self.nu
        self._chk(lib().mjpcx_rollout_splines_noisy_batched(self.handle, E, n, int(horizon), P, int(interp), as_f64p(nt), as_f64p(nv),
                                                            float(xfrc_std), float(xfrc_rate), int(seed), int(candidate_offset)))
        self.N, self.H, self.P, self.n_per_env = E * n, int(horizon), P, n

    def robust_step_batched(self, source, num_envs, num_candidates, repetitions, horizon, interp, node_times, xfrc_std, xfrc_rate, seed=0,
                            candidate_offset=0):
        """the Robust planner's plan step for every environment, behind `source`'s last batched rollout, one sync
        (mjpcx_robust_step_batched): the k best candidates of each environment of `source`, each rolled out R times under force
        noise on this context, scored by the planner's running mean. Dict of best (E: rank), candidate (E x k, local index in
        source's rollout), candidate_return, perturbed_score (E x k), valid (E x k) and spline (E x P x nu: the winner's). This
        context's last rollout is then the noisy one, 64 * ceil(k R / 64) per environment."""
        E, k, R = int(num_envs), int(num_candidates), int(repetitions)
        nt = _f(node_times)
        P = int(source.P)
        Ea, ka = max(E, 1), max(k, 1)
        out = dict(best=np.zeros(Ea, np.int32), candidate=np.zeros((Ea, ka), np.int32), candidate_return=np.zeros((Ea, ka)),
                   perturbed_score=np.zeros((Ea, ka)), valid=np.zeros((Ea, ka), np.int32), spline=np.zeros((Ea, max(P, 1), self.nu)))
        if E >= 1 and nt.size != E * P:
            raise ValueError(f"robust_step_batched: node_times has {nt.size} entries for {E} environments x {P} nodes of the source's rollout")
        self._chk(lib().mjpcx_robust_step_batched(self.handle, source.handle, E, k, R, int(horizon), int(interp), as_f64p(nt), float(xfrc_std),
                                                  float(xfrc_rate), int(seed), int(candidate_offset), as_i32p(out["best"]),
                                                  as_i32p(out["candidate"]), as_f64p(out["candidate_return"]),
                                                  as_f64p(out["perturbed_score"]), as_i32p(out["valid"]), as_f64p(out["spline"])))
        n_pad = 64 * ((k * R + 63) // 64)
        self.N, self.H, self.P, self.n_per_env = E * n_pad, int(horizon), P, n_pad
        return out

    def rollout_noise_batched(self, n_per_env, horizon, interp, node_times, nominal, noise_spec, num_envs=None):
        """node_times E x P, nominal E x P x nu; environment e draws the noise of a plain call with seed + e."""
        nt, nom = _f(node_times), _f(nominal)
        E = int(num_envs) if num_envs is not None else (nt.shape[0] if nt.ndim == 2 else 1)
        P = nt.size // E if E > 0 else nt.size
        assert E < 1 or nom.size == E * P * self.nu
        self._chk(lib().mjpcx_rollout_noise_batched(self.handle, E, int(n_per_env), int(horizon), P, int(interp), as_f64p(nt),
                                                    as_f64p(nom), C.byref(noise_spec)))
        self.N, self.H, self.P, self.n_per_env = E * int(n_per_env), int(horizon), P, int(n_per_env)

    def rollout_noise_batched_ce(self, n_per_env, horizon, interp, node_times, nominal, param_variance, noise_spec, num_envs=None):
        """rollout_noise_batched in cross-entropy mode with one variance row per environment: param_variance E x P x nu
        (noise_spec.param_variance is ignored)."""
        nt, nom, var = _f(node_times), _f(nominal), _f(param_variance)
        E = int(num_envs) if num_envs is not None else (nt.shape[0] if nt.ndim == 2 else 1)
        P = nt.size // E if E > 0 else nt.size
        assert E < 1 or (nom.size == E * P * self.nu and var.size == E * P * self.nu)
        self._chk(lib().mjpcx_rollout_noise_batched_ce(self.handle, E, int(n_per_env), int(horizon), P, int(interp), as_f64p(nt),
                                                       as_f64p(nom), as_f64p(var), C.byref(noise_spec)))
        self.N, self.H, self.P, self.n_per_env = E * int(n_per_env), int(horizon), P, int(n_per_env)

    def ce_update_batched(self, num_envs, n_elite, skip_candidate=-1):
        """the cross-entropy update of every environment in one launch / one sync: the n_elite best local candidates (without
        skip_candidate) and their returns (E x n_elite), the elites' mean and variance (E x P x nu), their mean return (E)."""
        E, k = int(num_envs), int(n_elite)
        shape = (max(E, 1), max(k, 1))
        idx, ret = np.zeros(shape, np.int32), np.zeros(shape)
        mean, var = np.zeros((max(E, 1), self.P, self.nu)), np.zeros((max(E, 1), self.P, self.nu))
        avg = np.zeros(max(E, 1))
        self._chk(lib().mjpcx_ce_update_batched(self.handle, E, k, int(skip_candidate), as_i32p(idx), as_f64p(ret), as_f64p(mean),
                                                as_f64p(var), as_f64p(avg)))
        return idx, ret, mean, var, avg

    def gradient_step_batched(self, num_envs, candidate, T, evaluate, eps, centered, representation, node_times, with_matrices=False):
        """the Gradient planner's derivative chain for every environment of the last batched rollout, on the device, one sync
        (mjpcx_gradient_step_batched): dict of nominal_return (E), k (E x T x nu), gradient (E x P x nu), dV (E x 2) and, with
        with_matrices (tests), A, B, cx, cu."""
        E, T = int(num_envs), int(T)
        ev = np.ascontiguousarray(evaluate, dtype=np.int32).reshape(-1)
        nt = _f(node_times)
        P = nt.size // max(E, 1)
        n, m, Ea = 2 * self.nv, self.nu, max(E, 1)
        out = dict(nominal_return=np.zeros(Ea), k=np.zeros((Ea, max(T, 1), m)), gradient=np.zeros((Ea, max(P, 1), m)), dV=np.zeros((Ea, 2)))
        if with_matrices:
            out.update(A=np.zeros((Ea, max(T, 1), n, n)), B=np.zeros((Ea, max(T, 1), n, m)), cx=np.zeros((Ea, max(T, 1), n)),
                       cu=np.zeros((Ea, max(T, 1), m)))
        opt = [as_f64p(out[key]) if with_matrices else None for key in ("A", "B", "cx", "cu")]
        self._chk(lib().mjpcx_gradient_step_batched(self.handle, E, int(candidate), T, ev.size, as_i32p(ev) if ev.size else as_i32p(np.zeros(1, np.int32)),
                                                    float(eps), int(centered), int(representation), P, as_f64p(nt),
                                                    as_f64p(out["nominal_return"]), as_f64p(out["k"]), as_f64p(out["gradient"]),
                                                    as_f64p(out["dV"]), *opt))
        return out

    def rollout_sample_gradient_batched(self, n_per_env, num_gradient, horizon, interp, node_times, nominal, noise_exploration, seed=0, iteration=0,
                                        gradient_values=None, gradient_times=None, num_envs=None):
        """the Sample-Gradient planner's candidates, generated on the device, and their rollout (mjpcx_rollout_sample_gradient_batched):
        node_times E x P, nominal E x P x nu; local candidate 0 the nominal, 1..n-G-1 clamp(nominal + noise_exploration z) with the normals
        of (seed + e, candidate, pair, iteration), the last G the gradient candidates -- gradient_values E x G x P x nu over
        gradient_times E x P, or (both None) those the last sample_gradient_update_batched left on the device -- sampled at node_times."""
        nt, nom = _f(node_times), _f(nominal)
        E = int(num_envs) if num_envs is not None else (nt.shape[0] if nt.ndim == 2 else 1)
        P = nt.size // E if E > 0 else nt.size
        n, G = int(n_per_env), int(num_gradient)
        assert E < 1 or nom.size == E * P * self.nu
        gv = gt = None
        if gradient_values is not None or gradient_times is not None:
            gv, gt = _f(gradient_values), _f(gradient_times)
            if gv.size != max(E, 0) * max(G, 0) * P * self.nu or gt.size != max(E, 0) * P:
                raise ValueError(f"rollout_sample_gradient_batched: gradient_values of {gv.size} and gradient_times of {gt.size} entries for "
                                 f"{E} environments x {G} gradient candidates x {P} nodes")
            if gv.size == 0:
                gv = np.zeros(1)   # (G = 0: a pointer the library never reads)
        self._chk(lib().mjpcx_rollout_sample_gradient_batched(self.handle, E, n, G, int(horizon), P, int(interp), as_f64p(nt), as_f64p(nom),
                                                              float(noise_exploration), int(seed), int(iteration),
                                                              as_f64p(gv) if gv is not None else None, as_f64p(gt) if gt is not None else None))
        self.N, self.H, self.P, self.n_per_env = E * n, int(horizon), P, n

    def sample_gradient_update_batched(self, num_envs, num_gradient, flags, gradient_filter, max_step, min_step, noise_exploration):
        """the Sample-Gradient update of every environment after rollout_sample_gradient_batched, one launch / one sync
        (mjpcx_sample_gradient_update_batched): dict of index (E: the winner, local), winner_type (E: 0 nominal, 1 perturbed, 2 gradient),
        best_return, nominal_return, improvement (E), spline (E x P x nu: the winner's) and gradient (E x P*nu). The weights, the gradient
        and the next gradient candidates stay in the context."""
        E = int(num_envs)
        Ea, P = max(E, 1), max(self.P, 1)
        out = dict(index=np.zeros(Ea, np.int32), winner_type=np.zeros(Ea, np.int32), best_return=np.zeros(Ea), nominal_return=np.zeros(Ea),
                   improvement=np.zeros(Ea), spline=np.zeros((Ea, P, self.nu)), gradient=np.zeros((Ea, P * self.nu)))
        self._chk(lib().mjpcx_sample_gradient_update_batched(self.handle, E, int(num_gradient), int(flags), float(gradient_filter), float(max_step),
                                                             float(min_step), float(noise_exploration), as_i32p(out["index"]),
                                                             as_i32p(out["winner_type"]), as_f64p(out["best_return"]),
                                                             as_f64p(out["nominal_return"]), as_f64p(out["improvement"]),
                                                             as_f64p(out["spline"]), as_f64p(out["gradient"])))
        return out

    def best_batched(self, num_envs, ref_candidate=0, with_spline=True):
        """per environment: local argmin, its return, the return of local ref_candidate, the winner's spline (E x P x nu)."""
        E = int(num_envs)
        idx = np.zeros(max(E, 1), np.int32)
        br, rr = np.zeros(max(E, 1)), np.zeros(max(E, 1))
        sp = np.zeros((max(E, 1), self.P, self.nu)) if with_spline else None
        self._chk(lib().mjpcx_best_batched(self.handle, E, int(ref_candidate), as_i32p(idx), as_f64p(br), as_f64p(rr),
                                           as_f64p(sp) if with_spline else None))
        return idx, br, rr, sp

    def mppi_update_batched(self, num_envs, temperature, ref_candidate=-1, want_weights=False):
        """the MPPI update of every environment in one launch sequence / one sync (mjpcx_mppi_update_batched): dict of index (E: the
        argmin, local), best_return, ref_return (NaN without a ref_candidate), weight_sum, effective_samples (E), valid (E: the best
        return is a number below +inf), mean (E x P x nu: the splines weighted by exp(-(R - best) / temperature[e]); an invalid
        environment's is ref_candidate's spline) and, want_weights, weights (E x n; else None). temperature: E values, or one for all."""
        E = int(num_envs)
        Ea = max(E, 1)
        temp = np.ascontiguousarray(temperature, dtype=np.float64).reshape(-1)
        if temp.size == 1:
            temp = np.full(Ea, temp[0])
        if temp.size != Ea:
            raise ValueError(f"mppi_update_batched: {temp.size} temperatures for {E} environments")
        out = dict(index=np.zeros(Ea, np.int32), best_return=np.zeros(Ea), ref_return=np.zeros(Ea), weight_sum=np.zeros(Ea),
                   effective_samples=np.zeros(Ea), valid=np.zeros(Ea, np.int32), mean=np.zeros((Ea, self.P, self.nu)),
                   weights=np.zeros((Ea, max(self.N // Ea, 1))) if want_weights else None)
        self._chk(lib().mjpcx_mppi_update_batched(self.handle, E, as_f64p(temp), int(ref_candidate), as_i32p(out["index"]),
                                                  as_f64p(out["best_return"]), as_f64p(out["ref_return"]), as_f64p(out["weight_sum"]),
                                                  as_f64p(out["effective_samples"]), as_i32p(out["valid"]), as_f64p(out["mean"]),
                                                  as_f64p(out["weights"]) if want_weights else None))
        return out

    def cma_set_state_batched(self, num_envs, num_params, sigma, C_=None, p_sigma=None, p_c=None):
        """the CMA-ES state of every environment (mjpcx_cma_set_state_batched): sigma E (or one for all), C E x d x d (None: the identity),
        p_sigma / p_c E x d (None: zeros); C is factored on the device, generation = 0"""
        E, d = int(num_envs), int(num_params)
        sig = _f(sigma).reshape(-1)
        if sig.size == 1:
            sig = np.full(max(E, 1), sig[0])
        opt = []
        for name, a, size in (("C", C_, E * d * d), ("p_sigma", p_sigma, E * d), ("p_c", p_c, E * d)):
            a = None if a is None else _f(a)
            if a is not None and a.size != max(size, 0):
                raise ValueError(f"cma_set_state_batched: {name} of {a.size} entries for {E} environments x {d} parameters")
            opt.append(a)
        if sig.size != max(E, 1):
            raise ValueError(f"cma_set_state_batched: {sig.size} step sizes for {E} environments")
        self._chk(lib().mjpcx_cma_set_state_batched(self.handle, E, d, as_f64p(sig), *[as_f64p(a) if a is not None else None for a in opt]))

    def cma_get_state_batched(self, num_envs, num_params):
        """dict of sigma (E), generation (E), C, A (E x d x d), p_sigma, p_c (E x d) as the context holds them"""
        E, d = int(num_envs), int(num_params)
        Ea, da = max(E, 1), max(d, 1)
        out = dict(sigma=np.zeros(Ea), generation=np.zeros(Ea, np.int64), C=np.zeros((Ea, da, da)), A=np.zeros((Ea, da, da)),
                   p_sigma=np.zeros((Ea, da)), p_c=np.zeros((Ea, da)))
        self._chk(lib().mjpcx_cma_get_state_batched(self.handle, E, d, as_f64p(out["sigma"]), out["generation"].ctypes.data_as(C.POINTER(C.c_int64)),
                                                    as_f64p(out["C"]), as_f64p(out["A"]), as_f64p(out["p_sigma"]), as_f64p(out["p_c"])))
        return out

    def rollout_cma_batched(self, n_per_env, horizon, interp, node_times, nominal, seed=0, iteration=0, num_envs=None):
        """the CMA-ES candidates, generated on the device from the context's state, and their rollout (mjpcx_rollout_cma_batched):
        node_times E x P, nominal (the mean) E x P x nu; local candidate 0 the mean, c >= 1 clamp(mean + sigma s (A z)) with the normals of
        (seed + e, c, pair, iteration)"""
        nt, nom = _f(node_times), _f(nominal)
        E = int(num_envs) if num_envs is not None else (nt.shape[0] if nt.ndim == 2 else 1)
        P = nt.size // E if E > 0 else nt.size
        n = int(n_per_env)
        assert E < 1 or nom.size == E * P * self.nu
        self._chk(lib().mjpcx_rollout_cma_batched(self.handle, E, n, int(horizon), P, int(interp), as_f64p(nt), as_f64p(nom), int(seed), int(iteration)))
        self.N, self.H, self.P, self.n_per_env = E * n, int(horizon), P, n

    def cma_update_batched(self, num_envs, params, want_order=False):
        """the CMA-ES update of every environment after rollout_cma_batched, one launch sequence / one sync (mjpcx_cma_update_batched).
        params: dict of mu, weights (mu) and the constants CMA_CONSTANTS (planners.cma_parameters plus sigma_min, sigma_max, pivot_floor).
        -> dict of index (E: the argmin over all candidates, local), best_return, nominal_return, improvement, valid, restarted, sigma
        (E), mean (E x P x nu) and, want_order, order (E x mu; else None). The distribution itself stays in the context."""
        E, mu = int(num_envs), int(params["mu"])
        Ea = max(E, 1)
        w = np.ascontiguousarray(params["weights"], dtype=np.float64).reshape(-1)
        if w.size != max(mu, 0):
            raise ValueError(f"cma_update_batched: {w.size} weights for mu = {mu}")
        if w.size == 0:
            w = np.zeros(1)
        prm = MjpcxCmaParams(mu, as_f64p(w), *[float(params[k]) for k in CMA_CONSTANTS])
        out = dict(index=np.zeros(Ea, np.int32), best_return=np.zeros(Ea), nominal_return=np.zeros(Ea), improvement=np.zeros(Ea),
                   valid=np.zeros(Ea, np.int32), restarted=np.zeros(Ea, np.int32), sigma=np.zeros(Ea), mean=np.zeros((Ea, max(self.P, 1), self.nu)),
                   order=np.zeros((Ea, max(mu, 1)), np.int32) if want_order else None)
        self._chk(lib().mjpcx_cma_update_batched(self.handle, E, C.byref(prm), as_i32p(out["index"]), as_f64p(out["best_return"]),
                                                 as_f64p(out["nominal_return"]), as_f64p(out["improvement"]), as_i32p(out["valid"]),
                                                 as_i32p(out["restarted"]), as_f64p(out["sigma"]), as_f64p(out["mean"]),
                                                 as_i32p(out["order"]) if want_order else None))
        return out

    def rollout_noise_ensemble(self, n, horizon, interp, node_times, nominal, noise_spec, num_hypotheses):
        """ONE set of n candidates under num_hypotheses hypotheses (the environments of the preceding set_states, with their task rows and
        models): node_times P, nominal P x nu and the noise stream of noise_spec.seed are shared, so candidate h * n + i is the same spline
        for every h. The context's last rollout is then a batched one of M x n."""
        nt, nom = _f(node_times).reshape(-1), _f(nominal)
        M, P = int(num_hypotheses), nt.size
        assert nom.size == P * self.nu
        self._chk(lib().mjpcx_rollout_noise_ensemble(self.handle, M, int(n), int(horizon), P, int(interp), as_f64p(nt), as_f64p(nom),
                                                     C.byref(noise_spec)))
        self.N, self.H, self.P, self.n_per_env = M * int(n), int(horizon), P, int(n)

    def ensemble_best(self, num_hypotheses, tail, ref_candidate=0, with_scores=False):
        """the ensemble's selection in one launch / one sync (mjpcx_ensemble_best): a candidate's score is the mean of the `tail` largest
        of its num_hypotheses returns (tail = M: the mean, 1: the worst case). -> the argmin, its score, the score of ref_candidate
        (-1: NaN), the winner's M returns, its spline (P x nu) and, with_scores, the n scores (else None)."""
        M = int(num_hypotheses)
        idx = np.zeros(1, np.int32)
        bs, rs = C.c_double(), C.c_double()
        members, sp = np.zeros(max(M, 1)), np.zeros((self.P, self.nu))
        scores = np.zeros(max(self.N // max(M, 1), 1)) if with_scores else None
        self._chk(lib().mjpcx_ensemble_best(self.handle, M, int(tail), int(ref_candidate), as_i32p(idx), C.byref(bs), C.byref(rs),
                                            as_f64p(members), as_f64p(sp), as_f64p(scores) if with_scores else None))
        return int(idx[0]), bs.value, rs.value, members, sp, scores

    def sync(self):
        self._chk(lib().mjpcx_sync(self.handle))

    def returns(self):
        ret = np.zeros(self.N)
        fl = np.zeros(self.N, np.int32)
        self._chk(lib().mjpcx_get_returns(self.handle, as_f64p(ret), as_i32p(fl)))
        # non-zero = failed (Trajectory::failure); the wavefront kernels add diagnostics above the low byte
        # (warning bits << 8 | failing step << 16), kept for tools in failure_raw
        self.failure_raw = fl.copy()
        return ret, (fl != 0).astype(np.int32)

    def return_of(self, candidate):
        r = C.c_double()
        self._chk(lib().mjpcx_get_return_at(self.handle, int(candidate), C.byref(r), None))
        return r.value

    def best(self, ref_candidate=0, with_spline=True):
        """argmin + winner spline + reference candidate's return in one launch / one sync."""
        idx = np.zeros(1, np.int32)
        br, rr = C.c_double(), C.c_double()
        sp = np.zeros((self.P, self.nu)) if with_spline else None
        self._chk(lib().mjpcx_best(self.handle, int(ref_candidate), as_i32p(idx), C.byref(br), C.byref(rr),
                                   as_f64p(sp) if with_spline else None))
        return int(idx[0]), br.value, rr.value, sp

    def topk(self, k):
        idx = np.zeros(k, np.int32)
        ret = np.zeros(k)
        self._chk(lib().mjpcx_topk(self.handle, int(k), as_i32p(idx), as_f64p(ret)))
        return idx, ret

    def elite_moments(self, candidates, mean=None):
        """(sum over the listed local candidates of p, or of (p - mean)^2) per spline parameter, and sum of returns."""
        cand = np.ascontiguousarray(candidates, dtype=np.int32).reshape(-1)
        out = np.zeros(self.P * self.nu)
        sr = C.c_double()
        m = None if mean is None else as_f64p(_f(mean).reshape(-1))
        self._chk(lib().mjpcx_elite_moments(self.handle, cand.size, as_i32p(cand) if cand.size else as_i32p(np.zeros(1, np.int32)),
                                            m, as_f64p(out), C.byref(sr)))
        return out.reshape(self.P, self.nu), sr.value

    def fetch_trajectory(self, candidate) -> Trajectory:
        tr = Trajectory(self.dim_state, self.nu, self.num_residual, self.num_trace, self.H)
        v = MjpcxTrajView()
        v.horizon = self.H
        v.states, v.actions, v.times = as_f64p(tr.states), as_f64p(tr.actions), as_f64p(tr.times)
        v.residual, v.costs, v.trace = as_f64p(tr.residual), as_f64p(tr.costs), as_f64p(tr.trace)
        self._chk(lib().mjpcx_fetch_trajectory(self.handle, int(candidate), C.byref(v)))
        tr.total_return, tr.failure = v.total_return, bool(v.failure)
        return tr

    def fetch_spline(self, candidate):
        out = np.zeros((self.P, self.nu))
        self._chk(lib().mjpcx_fetch_spline(self.handle, int(candidate), as_f64p(out)))
        return out

    # ---- iLQG
    def rollout_feedback(self, horizon, mode, representation, use_state, times, states, actions, gains, improvement, alpha):
        arrs = [_f(x).reshape(-1) for x in (times, states, actions, gains, improvement, alpha)]
        N, Tn = arrs[5].size, arrs[0].size
        self._chk(lib().mjpcx_rollout_feedback(self.handle, N, int(horizon), int(mode), int(representation), int(use_state),
                                               Tn, *[as_f64p(a) for a in arrs]))
        self.N, self.H, self.P = N, int(horizon), 0

    def rollout_feedback_batched(self, horizon, mode, representation, use_state, times, states, actions, gains, improvement, alpha,
                                 num_envs=None, n_per_env=None):
        """rollout_feedback for E environments in one launch (mjpcx_rollout_feedback_batched), from the states of set_states: times
        E x Tn, states E x Tn x dim_state, actions E x Tn x nu, gains E x Tn x nu x ndx, improvement E x Tn x nu, alpha E x n_per_env
        (any n_per_env >= 1). E and n_per_env come from alpha's shape; candidates are environment-major."""
        al = _f(alpha)
        if al.ndim != 2 and (num_envs is None or n_per_env is None):
            raise ValueError("rollout_feedback_batched: alpha must be E x n_per_env")
        E = int(num_envs) if num_envs is not None else al.shape[0]
        n = int(n_per_env) if n_per_env is not None else al.shape[1]
        tm = _f(times)
        Tn = tm.size // max(E, 1)
        ndx = 2 * self.nv
        arrs = [_f(x).reshape(-1) for x in (tm, states, actions, gains, improvement, al)]
        if E >= 1 and n >= 1 and Tn >= 1:
            want = [E * Tn, E * Tn * self.dim_state, E * Tn * self.nu, E * Tn * self.nu * ndx, E * Tn * self.nu, E * n]
            if [a.size for a in arrs] != want:
                raise ValueError(f"rollout_feedback_batched: array sizes {[a.size for a in arrs]} for {E} environments x {Tn} steps x {n} "
                                 f"candidates, expected {want}")
        self._chk(lib().mjpcx_rollout_feedback_batched(self.handle, E, n, int(horizon), int(mode), int(representation), int(use_state),
                                                       Tn, *[as_f64p(a) for a in arrs]))
        self.N, self.H, self.P, self.n_per_env = E * n, int(horizon), 0, n

    def ilqg_step_batched(self, candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor, min_reg, max_reg, max_iter,
                          with_matrices=False, num_envs=None):
        """iLQG's derivative chain and backward pass, regularisation retries included, for every environment of the last batched
        rollout, on the device, one sync (mjpcx_ilqg_step_batched). candidate: E local indices, -1 = the environment takes no part.
        Dict of K (E x T x nu x ndx), du (E x T x nu), dV (E x 2), status (E: 1 ok, 0 failed every retry, -1 took no part), mu, rate,
        retries (E), nominal_return (E) and, with with_matrices (tests), A, B, cx, cu, cxx, cxu, cuu, Vx, Vxx."""
        return self._ilqg_step_batched(None, candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor, min_reg, max_reg,
                                       max_iter, with_matrices, num_envs)

    def ilqg_step_batched_from(self, source, from_source, candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor, min_reg,
                               max_reg, max_iter, with_matrices=False, num_envs=None):
        """ilqg_step_batched for a fleet whose nominals lie in two contexts (mjpcx_ilqg_step_batched_from): environment e's nominal is
        local candidate candidate[e] of the last batched rollout of this context (from_source[e] == 0) or of `source`'s (== 1), gathered
        on the device; the chain runs here, with this context's set_states. source: a Context or None (then every from_source is 0).
        The same dict."""
        frm = np.ascontiguousarray(from_source, dtype=np.int32).reshape(-1)
        return self._ilqg_step_batched((source, frm), candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor, min_reg,
                                       max_reg, max_iter, with_matrices, num_envs)

    def _ilqg_step_batched(self, frm, candidate, T, evaluate, eps, centered, reg_type, use_limits, mu, rate, factor, min_reg, max_reg, max_iter,
                           with_matrices, num_envs):
        name = "ilqg_step_batched" if frm is None else "ilqg_step_batched_from"
        cand = np.ascontiguousarray(candidate, dtype=np.int32).reshape(-1)
        E, T = (cand.size if num_envs is None else int(num_envs)), int(T)
        ev = np.ascontiguousarray(evaluate, dtype=np.int32).reshape(-1)
        mu_in, rate_in = _f(mu).reshape(-1), _f(rate).reshape(-1)
        if E >= 1 and (cand.size, mu_in.size, rate_in.size) != (E, E, E):
            raise ValueError(f"{name}: {cand.size} candidates, {mu_in.size} mu, {rate_in.size} rate for {E} environments")
        if frm is not None and E >= 1 and frm[1].size != E:
            raise ValueError(f"{name}: {frm[1].size} from_source entries for {E} environments")
        n, m, Ea, Ta = 2 * self.nv, self.nu, max(E, 1), max(T, 1)
        out = dict(K=np.zeros((Ea, Ta, m, n)), du=np.zeros((Ea, Ta, m)), dV=np.zeros((Ea, 2)), status=np.zeros(Ea, np.int32), mu=np.zeros(Ea),
                   rate=np.zeros(Ea), retries=np.zeros(Ea, np.int32), nominal_return=np.zeros(Ea))
        names = ("A", "B", "cx", "cu", "cxx", "cxu", "cuu", "Vx", "Vxx")
        if with_matrices:
            shapes = ((n, n), (n, m), (n,), (m,), (n, n), (n, m), (m, m), (n,), (n, n))
            out.update({k: np.zeros((Ea, Ta) + sh) for k, sh in zip(names, shapes)})
        opt = [as_f64p(out[k]) if with_matrices else None for k in names]
        args = (E, as_i32p(cand) if cand.size else as_i32p(np.zeros(1, np.int32)), T, ev.size,
                as_i32p(ev) if ev.size else as_i32p(np.zeros(1, np.int32)), float(eps), int(centered),
                int(reg_type), int(use_limits), as_f64p(mu_in), as_f64p(rate_in), float(factor), float(min_reg),
                float(max_reg), int(max_iter), as_f64p(out["K"]), as_f64p(out["du"]), as_f64p(out["dV"]),
                as_i32p(out["status"]), as_f64p(out["mu"]), as_f64p(out["rate"]), as_i32p(out["retries"]),
                as_f64p(out["nominal_return"]), *opt)
        if frm is None:
            self._chk(lib().mjpcx_ilqg_step_batched(self.handle, *args))
        else:
            self._chk(lib().mjpcx_ilqg_step_batched_from(self.handle, None if frm[0] is None else frm[0].handle,
                                                         as_i32p(frm[1]) if frm[1].size else as_i32p(np.zeros(1, np.int32)), *args))
        return out

    def transition_fd(self, times, states, actions, eps=1e-6, centered=0):
        T, ndx, nu, nr = len(times), 2 * self.nv, self.nu, self.num_residual
        A, B, Cm, D = np.zeros((T, ndx, ndx)), np.zeros((T, ndx, nu)), np.zeros((T, nr, ndx)), np.zeros((T, nr, nu))
        self._chk(lib().mjpcx_transition_fd(self.handle, T, as_f64p(_f(times)), as_f64p(_f(states).reshape(-1)),
                                            as_f64p(_f(actions).reshape(-1)), float(eps), int(centered), as_f64p(A),
                                            as_f64p(B), as_f64p(Cm), as_f64p(D)))
        return A, B, Cm, D

    def cost_derivatives(self, residual, Cm, D):
        T, ndx, nu = residual.shape[0], 2 * self.nv, self.nu
        cx, cu = np.zeros((T, ndx)), np.zeros((T, nu))
        cxx, cxu, cuu = np.zeros((T, ndx, ndx)), np.zeros((T, ndx, nu)), np.zeros((T, nu, nu))
        self._chk(lib().mjpcx_cost_derivatives(self.handle, T, as_f64p(_f(residual).reshape(-1)), as_f64p(_f(Cm).reshape(-1)),
                                               as_f64p(_f(D).reshape(-1)), as_f64p(cx), as_f64p(cu), as_f64p(cxx),
                                               as_f64p(cxu), as_f64p(cuu)))
        return cx, cu, cxx, cxu, cuu

    def backward_pass(self, mu, reg_type, use_limits, A, B, cx, cu, cxx, cxu, cuu, actions, limits):
        T, n, m = A.shape[0], A.shape[1], B.shape[2]
        Vx, Vxx, K, du, dV = np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T, m, n)), np.zeros((T, m)), np.zeros(2)
        st = np.zeros(1, np.int32)
        ms = C.c_double()
        args = [as_f64p(_f(x).reshape(-1)) for x in (A, B, cx, cu, cxx, cxu, cuu, actions, limits)]
        self._chk(lib().mjpcx_backward_pass(self.handle, n, m, T, float(mu), int(reg_type), int(use_limits), *args,
                                            as_f64p(Vx), as_f64p(Vxx), as_f64p(K), as_f64p(du), as_f64p(dV), as_i32p(st),
                                            C.byref(ms)))
        return dict(ok=bool(st[0]), Vx=Vx, Vxx=Vxx, K=K, du=du, dV=dV, kernel_ms=ms.value)

    def gradient_pass(self, A, B, cx, cu, representation, node_times, step_times):
        """Gradient::Compute + the spline-mapping projection (mjpcx_gradient_pass): Vx, k, dV, gradient (P x m)"""
        T, n, m, P = A.shape[0], A.shape[1], B.shape[2], len(node_times)
        Vx, k, dV, g = np.zeros((T, n)), np.zeros((T, m)), np.zeros(2), np.zeros((P, m))
        ms = C.c_double()
        args = [as_f64p(_f(x).reshape(-1)) for x in (A, B, cx, cu)]
        self._chk(lib().mjpcx_gradient_pass(self.handle, n, m, T, *args, int(representation), P, as_f64p(_f(node_times)),
                                            as_f64p(_f(step_times)), as_f64p(Vx), as_f64p(k), as_f64p(dV), as_f64p(g), C.byref(ms)))
        return dict(Vx=Vx, k=k, dV=dV, gradient=g, kernel_ms=ms.value)

    def timing_reset(self):
        self._chk(lib().mjpcx_timing_reset(self.handle))

    def timing_read(self):
        ms = C.c_double()
        n = C.c_int64()
        self._chk(lib().mjpcx_timing_read(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_read_main(self):
        """HIP-event time of the rollouts' first (dominant) kernel alone; call before timing_read"""
        ms = C.c_double()
        n = C.c_int64()
        self._chk(lib().mjpcx_timing_read_main(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def quad_stats(self):
        """rollout_quad_kernel: candidates of the last rollout handed to the wavefront-per-candidate kernel, total and by reason"""
        h = np.zeros(8, np.int32)
        self._chk(lib().mjpcx_quad_stats(self.handle, as_i32p(h)))
        return dict(handed_on=int(h[0]), contact_list_full=int(h[1]), leg_leg_contact=int(h[2]), indefinite_hessian=int(h[3]), non_finite=int(h[4]),
                    both_limits=int(h[5]), trunk_leg_contact=int(h[6]), out_of_proof_range=int(h[7]))

    def set_pruning(self, enabled, initial_bound=float("inf")):
        """mjpcx_set_pruning: the following plain rollouts on rollout_quad_kernel retire candidates that can no longer be the argmin (sticky)"""
        self._chk(lib().mjpcx_set_pruning(self.handle, int(bool(enabled)), float(initial_bound)))

    def prune_stats(self):
        """of the last rollout (zeros unless it was pruned): candidates retired, their mean retire step, the negative-cost flag, wavefronts that ended early"""
        h = (C.c_int64 * 4)()
        self._chk(lib().mjpcx_prune_stats(self.handle, h))
        return dict(retired=int(h[0]), retire_step_sum=int(h[1]), mean_retire_step=(h[1] / h[0] if h[0] else 0.0), negative_cost=bool(h[2]),
                    wavefronts_ended_early=int(h[3]))

    def set_park_hint(self, hint=float("inf")):
        """mjpcx_set_park_hint: an unproven estimate of the next pruned launches' best return (sticky; +inf: off). No result depends on it"""
        self._chk(lib().mjpcx_set_park_hint(self.handle, float(hint)))

    def park_stats(self):
        """of the last rollout (zeros unless it was pruned with a hint): candidates parked, of them retired by the settling pass / resumed, the resume launch's ms"""
        h = (C.c_int64 * 3)()
        ms = C.c_double(0.0)
        self._chk(lib().mjpcx_park_stats(self.handle, h, C.byref(ms)))
        return dict(parked=int(h[0]), settled_retired=int(h[1]), resumed=int(h[2]), resume_ms=float(ms.value))

    def park_resumed(self):
        """mjpcx_park_resumed: the candidates the last rollout resumed and the step each was parked at, sorted by candidate"""
        n = lib().mjpcx_park_resumed(self.handle, None, None, 0)
        if n < 0:
            self._chk(n)
        idx, step = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        if n > 0:
            self._chk(min(lib().mjpcx_park_resumed(self.handle, as_i32p(idx), as_i32p(step), n), 0))
        order = np.argsort(idx[:n])
        return idx[:n][order], step[:n][order]

    def set_pruning_batched(self, enabled, num_envs=0, initial_bound=None, park_hint=None):
        """mjpcx_set_pruning_batched: the following rollout_noise_batched launches of num_envs environments on rollout_quad_kernel prune, and park,
        with a bound and a hint per environment (sticky; None: +inf each). enabled false clears the switch"""
        if not enabled:
            self._chk(lib().mjpcx_set_pruning_batched(self.handle, 0, 0, None, None))
            return
        E = int(num_envs)

        def row(v, what):
            if v is None:
                return None
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (E,)) if np.ndim(v) == 0 else np.asarray(v, np.float64))
            if v.shape != (E,):
                raise ValueError(f"{what} must hold one value per environment ({E}), got shape {v.shape}")
            return v
        b, h = row(initial_bound, "initial_bound"), row(park_hint, "park_hint")
        self._chk(lib().mjpcx_set_pruning_batched(self.handle, 1, E, None if b is None else as_f64p(b), None if h is None else as_f64p(h)))

    def prune_stats_batched(self, num_envs):
        """mjpcx_prune_stats_batched: of the last rollout, per environment (zeros unless it was a pruned batched one): prune_stats' and park_stats'
        counts as arrays of length E, and each environment's final bound"""
        E = int(num_envs)
        pr, pk = (C.c_int64 * (4 * E))(), (C.c_int64 * (3 * E))()
        fb = np.zeros(E, np.float64)
        self._chk(lib().mjpcx_prune_stats_batched(self.handle, E, pr, pk, as_f64p(fb)))
        pr, pk = np.array(pr[:], np.int64).reshape(E, 4), np.array(pk[:], np.int64).reshape(E, 3)
        return dict(retired=pr[:, 0].copy(), retire_step_sum=pr[:, 1].copy(), negative_cost=pr[:, 2] != 0, wavefronts_ended_early=pr[:, 3].copy(),
                    parked=pk[:, 0].copy(), settled_retired=pk[:, 1].copy(), resumed=pk[:, 2].copy(), final_bound=fb)

    def set_prune_rank(self, rank=1):
        """mjpcx_set_prune_rank: the following pruned launches settle on the rank-th smallest completed return, so that their first `rank`
        stored returns are exact (sticky; 1: the bound of the argmin, the default)"""
        self._chk(lib().mjpcx_set_prune_rank(self.handle, int(rank)))

    def rank_bound_batched(self, num_envs, rank):
        """mjpcx_rank_bound_batched: rank_bound_kernel over the last rollout's returns and failure words as num_envs equal environments:
        per environment the rank-th smallest qualifying return (+inf: fewer qualify). For tests and tools"""
        out = np.zeros(int(num_envs), np.float64)
        self._chk(lib().mjpcx_rank_bound_batched(self.handle, int(num_envs), int(rank), as_f64p(out)))
        return out

    def algorithmic_bytes(self, horizon, num_nodes):
        return lib().mjpcx_algorithmic_bytes(self.handle, int(horizon), int(num_nodes))

    def device_buffer(self, which):
        p = C.c_void_p()
        n = C.c_size_t()
        self._chk(lib().mjpcx_device_buffer(self.handle, int(which), C.byref(p), C.byref(n)))
        return p.value, n.value
