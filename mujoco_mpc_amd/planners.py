"""Host-side planners over the C ABI: drop-in mirrors of the reference's
`mjpc::SamplingPlanner` (mjpc/planners/sampling/planner.{h,cc}) and
`mjpc::SamplingPolicy` (sampling/policy.{h,cc}).

Only `Rollouts(...)` (planner.cc:355-393) and the sort (planner.cc:184-188) are
replaced by device work; nominal resampling, policy copy and `ActionFromPolicy`
stay host-side with the reference's semantics. Differences, both forced by
SURVEY.md findings: the 128-candidate cap of kMaxTrajectory is lifted (F5) and
noise comes from a seedable counter-based generator (F4).
"""
from __future__ import annotations

import math
import threading
import time as _time

import numpy as np

from . import capi
from .cstructs import PackedModel
from .spline import CUBIC, LINEAR, ZERO, TimeSpline
from .task import NORM_L2, NORM_POWER_LOSS, NORM_QUADRATIC, NORM_RECTIFY, NORM_SMOOTH_ABS, Task

K_MAX_TRAJECTORY_HORIZON = 512  # mjpc/trajectory.h:27


def sync_task(ctx, task):
    """The per-plan frozen ResidualFn copy (Agent::PlanIteration, agent.cc:319): weights, norm / residual parameters,
    risk and the task-specific residual state reach the device before the plan's rollouts."""
    if hasattr(ctx, "set_task_params"):
        ctx.set_task_params(task.weight, task.norm_parameter, task.parameters, task.risk)
    if hasattr(ctx, "set_residual_state") and (task.residual_int or task.residual_real):
        ctx.set_residual_state(task.residual_int, task.residual_real)


def clamp(x, bounds):
    """Clamp, mjpc/utilities.cc:112-116 (mju_clip = max(lo, min(hi, x)))."""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
    np.maximum(b[:, 0], np.minimum(b[:, 1], x), out=x)
    return x


class State:
    """mjpc::State (mjpc/states/state.{h,cc}): the snapshot handed to Planner::SetState."""

    def __init__(self, model):
        self._lock = threading.RLock()
        self.state = np.zeros(model.nq + model.nv + model.na)
        self.mocap = np.zeros(7 * model.nmocap)
        self.userdata = np.zeros(model.nuserdata)
        self.time = 0.0
        # mocap bodies start at their model pose
        for b in range(model.nbody):
            i = int(model.body_mocapid[b])
            if i >= 0:
                self.mocap[7 * i:7 * i + 3] = model.body_pos[b]
                self.mocap[7 * i + 3:7 * i + 7] = model.body_quat[b]

    def set(self, qpos, qvel, act=(), mocap_pos=None, mocap_quat=None, userdata=None, time=0.0):
        with self._lock:
            self.state[:] = np.concatenate([np.asarray(qpos, float), np.asarray(qvel, float), np.asarray(act, float)])
            if mocap_pos is not None:
                mp, mq = np.asarray(mocap_pos, float).reshape(-1, 3), np.asarray(mocap_quat, float).reshape(-1, 4)
                for i in range(mp.shape[0]):
                    self.mocap[7 * i:7 * i + 3], self.mocap[7 * i + 3:7 * i + 7] = mp[i], mq[i]
            if userdata is not None:
                self.userdata[:] = userdata
            self.time = float(time)

    def copy_to(self):
        with self._lock:
            return self.state.copy(), self.mocap.copy(), self.userdata.copy(), self.time


class SamplingPolicy:
    """mjpc::SamplingPolicy (sampling/policy.{h,cc})."""

    def __init__(self):
        self.model = None
        self.plan = TimeSpline(0)
        self.num_spline_points = 0

    def allocate(self, model, task, horizon):
        self.model = model
        self.num_spline_points = int(model.get_number("sampling_spline_points", K_MAX_TRAJECTORY_HORIZON))
        self.plan = TimeSpline(model.nu)
        self.plan.reserve(self.num_spline_points)

    def reset(self, horizon, initial_repeated_action=None):
        self.plan.clear()
        if initial_repeated_action is not None:
            self.plan.add_node(0, initial_repeated_action)

    def action(self, action, state, time):
        self.plan.sample(time, action)
        return clamp(action, self.model.actuator_ctrlrange)

    def copy_from(self, policy, horizon=None):
        self.model = policy.model
        self.plan = policy.plan.copy()
        self.num_spline_points = policy.num_spline_points


def _agent_differentiable(model):
    """the gradient-based planners plan on the differentiable model copy unless agent_differentiable says otherwise (agent.cc:156-164)"""
    return bool(int(model.get_number("agent_differentiable", 1)))


class _ContextOwner:
    """what every planner with a context of its own shares, single or fleet: `device`, `precision`, `_backend_factory`, `model` and
    `task` are the planner's"""

    def _create_context(self, differentiable=False):
        """the one place a context is made: `backend_factory(task)` where the planner was given one (a fleet's member is handed the
        shared context; test backends: see tests/oracle_backend.py), else a device context on the task's planning model"""
        if self._backend_factory is not None:
            return self._backend_factory(self.task)
        return capi.Context(self.task.packed_model(differentiable=differentiable), self.task.packed(), self.device, self.precision)

    def _timestep(self):
        return self.model.get_number("agent_timestep", self.model.timestep)


class GpuSamplingPlanner(_ContextOwner):
    """mjpc::SamplingPlanner with the candidate fan-out on the GPU.

    `group`: optional rank group (see distributed.py) sharding the candidates over
    GPUs; every rank keeps an identical host policy."""

    def __init__(self, device=0, precision=64, seed=0, group=None, backend_factory=None, differentiable=False):
        self.device, self.precision, self.seed = device, precision, seed
        self.group = group
        self._backend_factory = backend_factory
        # plan on the differentiable model copy (agent.cc:156-164): off for sampling on its own, on in GpuILQSPlanner
        self.differentiable = differentiable
        self.model = None
        self.task = None
        self.ctx = None
        self.mtx_ = threading.RLock()
        self.best_return = self.nominal_return = 0.0    # the last optimize_policy's trajectory[winner] / trajectory[0] returns
        self.noise_exploration = [0.0, 0.0]
        self.iteration = 0
        self.winner = 0
        self.improvement = 0.0
        self.noise_compute_time = 0.0
        self.rollouts_compute_time = 0.0
        self.policy_update_compute_time = 0.0
        self.trajectory_order = []
        self._scores = []

    # ---- Planner::Initialize, planner.cc:41-77
    def initialize(self, model, task: Task):
        self.model, self.task = model, task
        self.noise_exploration[0] = model.get_number("sampling_exploration", 0.1)
        se = model.numeric.get("sampling_exploration")
        self.noise_exploration[1] = float(se[1]) if se is not None and len(se) > 1 else 0.0
        self.num_trajectory_ = int(model.get_number("sampling_trajectories", 10))
        self.interpolation_ = int(model.get_number("sampling_representation", CUBIC))
        self.sliding_plan_ = int(model.get_number("sampling_sliding_plan", 0))
        self.winner = 0

    # ---- Planner::Allocate, planner.cc:80-107
    def allocate(self):
        m = self.model
        self.state = np.zeros(m.nq + m.nv + m.na)
        self.mocap = np.zeros(7 * m.nmocap)
        self.userdata = np.zeros(m.nuserdata)
        self.time = 0.0
        self.policy, self.previous_policy = SamplingPolicy(), SamplingPolicy()
        self.policy.allocate(m, self.task, K_MAX_TRAJECTORY_HORIZON)
        self.previous_policy.allocate(m, self.task, K_MAX_TRAJECTORY_HORIZON)
        self.winner_policy = SamplingPolicy()  # candidate_policy[winner]
        self.winner_policy.allocate(m, self.task, K_MAX_TRAJECTORY_HORIZON)
        self.plan_scratch = TimeSpline(m.nu)
        self._best = None
        self.ctx = self._create_context(self.differentiable)

    # ---- Planner::Reset, planner.cc:110-147
    def reset(self, horizon, initial_repeated_action=None):
        self.state[:] = 0
        self.mocap[:] = 0
        self.userdata[:] = 0
        self.time = 0.0
        with self.mtx_:
            self.policy.reset(horizon, initial_repeated_action)
            self.previous_policy.reset(horizon, initial_repeated_action)
        self.winner_policy.reset(horizon, initial_repeated_action)
        self.plan_scratch.clear()
        self.improvement = 0.0
        self.winner = 0
        self._best = None

    # ---- Planner::SetState, planner.cc:150-153
    def set_state(self, state: State):
        self.state, self.mocap, self.userdata, self.time = state.copy_to()

    # ---- UpdateNominalPolicy, planner.cc:240-323
    def update_nominal_policy(self, horizon):
        num_spline_points = self.winner_policy.num_spline_points
        nominal_time = self.time
        time_horizon = (horizon - 1) * self._timestep()
        if self.sliding_plan_:
            extra = {ZERO: 1, LINEAR: 2, CUBIC: 4}[self.interpolation_]
            if num_spline_points > extra:
                time_shift = max(time_horizon / (num_spline_points - extra), 1.0e-5)
            else:
                time_shift = time_horizon
            with self.mtx_:
                plan = self.policy.plan
                if plan.size() and plan.node_at(0)[0] > nominal_time:
                    plan.shift_time(nominal_time)
                    self.previous_policy.plan.shift_time(nominal_time)
                plan.discard_before(nominal_time)
                if plan.size() == 0:
                    plan.add_node(nominal_time)
                while plan.size() < num_spline_points:
                    t_last, v_last = plan.node_at(plan.size() - 1)
                    plan.add_node(t_last + time_shift, v_last.copy())
        else:
            if self.interpolation_ == ZERO:
                time_shift = max(time_horizon / num_spline_points, 1.0e-5)
            else:
                time_shift = max(time_horizon / (num_spline_points - 1), 1.0e-5)
            self.plan_scratch.clear()
            self.plan_scratch.set_interpolation(self.interpolation_)
            for _ in range(num_spline_points):
                node = self.plan_scratch.add_node(nominal_time)
                self.winner_policy.action(node, None, nominal_time)
                nominal_time += time_shift
            with self.mtx_:
                self.policy.plan = self.plan_scratch.copy()

    # ---- Rollouts, planner.cc:355-393: the device fan-out
    def rollouts(self, num_trajectory, horizon):
        plan = self.policy.plan
        rank, world = (self.group.rank, self.group.world) if self.group else (0, 1)
        # candidates [rank*n, (rank+1)*n) of the global batch; candidate 0 is the un-noised nominal
        if world > num_trajectory:
            raise ValueError("more ranks than candidates: every rank needs at least one rollout")
        q, r = divmod(num_trajectory, world)   # contiguous ranges, the first (N % world) ranks take one more
        n_local = q + (1 if rank < r else 0)
        offset = rank * q + min(rank, r)
        if rank == world - 1:
            n_local = num_trajectory - offset
        ns = capi.make_noise_spec(seed=self.seed, iteration=self.iteration, mode=capi.NOISE_SAMPLING,
                                  candidate_offset=offset, nominal_candidate=0,
                                  std0=self.noise_exploration[0], std1=self.noise_exploration[1])
        sync_task(self.ctx, self.task)
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        self.ctx.rollout_noise(n_local, horizon, plan.interpolation(), plan.times(), plan.values(), ns)
        self._offset, self._n_local = offset, n_local

    # ---- OptimizePolicyCandidates, planner.cc:155-194
    def optimize_policy_candidates(self, ncandidates, horizon, pool=None):
        self.update_nominal_policy(horizon)
        num_trajectory = self.num_trajectory_
        ncandidates = min(ncandidates, num_trajectory)
        t0 = _time.perf_counter()
        self.policy.plan.set_interpolation(self.interpolation_)
        self.rollouts(num_trajectory, horizon)
        k = min(ncandidates, self._n_local)
        idx, ret = self.ctx.topk(k)  # device selection replaces std::partial_sort
        idx = idx + self._offset
        if self.group and self.group.world > 1:
            idx, ret = self.group.merge_topk(idx, ret, ncandidates)
        self.trajectory_order = [int(i) for i in idx]
        self._scores = [float(r) for r in ret]
        self.rollouts_compute_time = (_time.perf_counter() - t0) * 1e6
        self.iteration += 1
        return len(self.trajectory_order)

    # ---- OptimizePolicy, planner.cc:197-212
    def optimize_policy(self, horizon, pool=None):
        """OptimizePolicyCandidates(1) + CopyCandidateToPolicy(0), with the device selection, the
        winner's spline and the nominal's return fetched in ONE launch + ONE sync (mjpcx_best)."""
        self.update_nominal_policy(horizon)
        t0 = _time.perf_counter()
        self.policy.plan.set_interpolation(self.interpolation_)
        self.rollouts(self.num_trajectory_, horizon)
        ref = 0 if self._offset == 0 else -1                 # trajectory[0] lives on rank 0
        idx, best_ret, nominal_ret, values = self.ctx.best(ref)
        idx += self._offset
        if self.group and self.group.world > 1:
            idx, best_ret, nominal_ret, values = self.group.exchange_best(idx, best_ret, nominal_ret, values)
        self.trajectory_order = [int(idx)]
        self._scores = [float(best_ret)]
        self.rollouts_compute_time = (_time.perf_counter() - t0) * 1e6
        self.iteration += 1
        t0 = _time.perf_counter()
        self._set_winner(int(idx), values)
        self.best_return, self.nominal_return = float(best_ret), float(nominal_ret)
        self.improvement = max(nominal_ret - best_ret, 0.0)
        self.policy_update_compute_time = (_time.perf_counter() - t0) * 1e6

    def _set_winner(self, global_idx, values):
        """CopyCandidateToPolicy, planner.cc:534-543, given candidate_policy[winner]'s spline values."""
        self.winner = global_idx
        times = self.policy.plan.times()
        plan = TimeSpline(self.model.nu, self.policy.plan.interpolation())
        for t, v in zip(times, np.asarray(values).reshape(len(times), -1)):
            plan.add_node(t, v)
        self.winner_policy.model = self.model
        self.winner_policy.plan = plan
        self.winner_policy.num_spline_points = self.policy.num_spline_points
        self._best = None                                        # BestTrajectory() is fetched lazily
        with self.mtx_:
            self.previous_policy.copy_from(self.policy)
            self.policy.copy_from(self.winner_policy)

    # ---- NominalTrajectory, planner.cc:215-227
    def nominal_trajectory(self, horizon, pool=None):
        plan = self.winner_policy.plan if self.winner_policy.plan.size() else self.policy.plan
        sync_task(self.ctx, self.task)
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        if plan.size() == 0:
            times, values = np.array([self.time]), np.zeros((1, 1, self.model.nu))
        else:
            times, values = plan.times(), plan.values()[None]
        self.ctx.rollout_splines(horizon, plan.interpolation(), times, values)
        self._best = self.ctx.fetch_trajectory(0)
        return self._best

    # ---- ActionFromPolicy, planner.cc:230-238: never touches the GPU
    def action_from_policy(self, action, state, time, use_previous=False):
        with self.mtx_:
            return (self.previous_policy if use_previous else self.policy).action(action, state, time)

    # ---- BestTrajectory, planner.cc:396-398 (the reference returns &trajectory[winner]; here the
    # winner's buffers stay on the device until someone asks for them; with several ranks only the
    # owner of the winner has them)
    def best_trajectory(self):
        if self._best is None and self.ctx is not None and self.ctx.N > 0:
            local = self.winner - self._offset
            if 0 <= local < self._n_local:
                self._best = self.ctx.fetch_trajectory(local)
        return self._best

    def num_parameters(self):
        return self.policy.num_spline_points * self.model.nu

    # ---- RankedPlanner quartet, planner.cc:520-543
    def candidate_score(self, candidate):
        return self._scores[candidate]

    def action_from_candidate_policy(self, action, candidate, state, time):
        p = SamplingPolicy()
        p.copy_from(self.policy)
        self._load_candidate_plan(p, self.trajectory_order[candidate])
        return p.action(action, state, time)

    def _load_candidate_plan(self, policy, global_idx):
        """candidate_policy[i].plan: fetched from the rank that rolled it out."""
        local = global_idx - self._offset
        values = None
        owner = 0
        if 0 <= local < self._n_local:
            values = self.ctx.fetch_spline(local)
        if self.group and self.group.world > 1:
            owner = self.group.owner_of(global_idx, self.num_trajectory_)
            values = self.group.broadcast_array(values, (self.ctx.P, self.model.nu), src=owner)
        times = self.policy.plan.times()
        policy.plan = TimeSpline(self.model.nu, self.policy.plan.interpolation())
        for t, v in zip(times, values):
            policy.plan.add_node(t, v)

    def copy_candidate_to_policy(self, candidate):
        p = SamplingPolicy()
        self._load_candidate_plan(p, self.trajectory_order[candidate])
        self._set_winner(self.trajectory_order[candidate], p.plan.values())


MJPCX_ESTATE = -5              # include/mjpcx.h
DEFAULT_PARK_SLACK = 0.05      # kDefaultParkSlack of gpu_sampling/planner.h
K_PARK_MAX_RESUME_SHARE = 0.25  # kParkMaxResumeShare: a plan that resumed more of a robot's candidates ran on a stale hint


class _Fleet(_ContextOwner):
    """The fleet ("batched") planners' base: `num_envs` members in `envs`, one per environment and each the single planner of its
    kind, on ONE shared context. Here is everything per environment that does not depend on the kind of planner: the members'
    states, tasks and models and their way to the context, the pass-throughs to the members, and the two fetches of trajectories
    from a batched launch. A fleet planner supplies its members (`envs`, which are handed the shared context through their
    backend_factory), its launch and its selection (`optimize_policy`, and `nominal_trajectory` / `best_trajectory` where it has
    them), and `_reset_own` for what a reset clears beside the members."""
    derivative_chain = False     # Gradient, iLQG: the batched derivative calls use the context's one model, so no set_models
    differentiable = False       # plan on the differentiable model copy: GpuBatchILQSPlanner turns it on in its sampling half (a planner
                                 # with a derivative chain asks agent_differentiable instead)
    _n_advice = "set sampling_trajectories / num_trajectory_ accordingly"   # _check_n's last sentence: the setting behind n
    _last, _n = None, 0          # what the context's last rollout was: "plan" (_n candidates per environment) or "nominal" (64)

    def __init__(self, num_envs, device, precision, backend_factory):
        if int(num_envs) < 1:
            raise ValueError(f"{type(self).__name__} needs at least one environment")
        self.num_envs, self.device, self.precision = int(num_envs), device, precision
        self._backend_factory = backend_factory
        self.model = self.task = self.ctx = None

    def initialize(self, model, task: Task):
        self.model, self.task = model, task
        for p in self.envs:
            p.initialize(model, task)

    def allocate(self):
        self.ctx = self._create_context(_agent_differentiable(self.model) if self.derivative_chain else self.differentiable)
        for p in self.envs:
            p.allocate()
        self._push_models()

    def reset(self, horizon, initial_repeated_action=None):
        for p in self.envs:
            p.reset(horizon, initial_repeated_action)
        self._reset_own()

    def _reset_own(self):
        """what a reset clears in the fleet planner itself"""

    def _check_n(self, n):
        if n < 64 or n % 64 != 0:
            raise ValueError(f"{type(self).__name__}: {n} candidates per environment; a batched launch needs a positive multiple "
                             f"of 64 (every wavefront serves one environment) -- {self._n_advice}")

    def set_states(self, states):
        """one State per environment (Planner::SetState for each)"""
        if len(states) != self.num_envs:
            raise ValueError(f"{len(states)} states for {self.num_envs} environments")
        for p, st in zip(self.envs, states):
            p.set_state(st)

    def _push_states(self, members=None):
        """before every batched launch: the fleet's task, the members' states (another fleet's members for Robust, whose members sit
        on its delegate's), the task rows"""
        members = self.envs if members is None else members
        sync_task(self.ctx, self.task)
        self.ctx.set_states(np.stack([p.state for p in members]), np.array([p.time for p in members]),
                            np.stack([p.mocap for p in members]) if self.model.nmocap else None,
                            np.stack([p.userdata for p in members]) if self.model.nuserdata else None)
        self._push_task_rows()

    def _nominal_launch(self, horizon, interpolation, times, values, fetch=True):
        """NominalTrajectory of every environment in one launch: 64 candidates per environment, each carrying the environment's policy
        (`values` E x P x nu, so candidate 0 does); -> the E trajectories, unless the caller reads the rollout on the device instead"""
        self._push_states()
        values = np.stack([np.broadcast_to(v[None], (64,) + v.shape) for v in values])
        self.ctx.rollout_splines_batched(horizon, interpolation, times, values, num_envs=self.num_envs, n_per_env=64)
        self._last = "nominal"
        return [self.ctx.fetch_trajectory(64 * e) for e in range(self.num_envs)] if fetch else None

    def _fetch_planned(self, env, index):
        """candidate `index` of environment `env` in the plan launch (global candidate env * n + index), for a lazy best_trajectory;
        None once the context's last rollout is no longer that launch"""
        return self.ctx.fetch_trajectory(env * self._n + index) if self._last == "plan" else None

    @property
    def winners(self):
        return [p.winner for p in self.envs]

    def action_from_policy(self, env, action, state, time, use_previous=False):
        return self.envs[env].action_from_policy(action, state, time, use_previous)

    def num_parameters(self):
        return self.envs[0].num_parameters()

    # ---- a task per environment
    _tasks = None
    _rows_pushed = False

    def set_tasks(self, tasks):
        """One Task per environment -- the same model and residual, norm kinds and term dimensions; weights, norm parameters,
        parameters, risk and the frozen residual state (mode, gait phase) are each environment's own. Member e then plans with tasks[e]:
        every batched launch carries the tasks' current values as per-environment rows (`set_task_params_batched`,
        `set_residual_states`), so a task may be edited or `transition`ed between plan steps. After `initialize`. None: the fleet's one
        task for every environment again."""
        if tasks is None:
            self._tasks = None
            for p in self.envs:
                p.task = self.task
            return
        tasks = list(tasks)
        if len(tasks) != self.num_envs:
            raise ValueError(f"{len(tasks)} tasks for {self.num_envs} environments")
        if self.task is None:
            raise ValueError("set_tasks before initialize")
        ref = self.task
        for e, t in enumerate(tasks):
            same = (t.residual_id == ref.residual_id and t.model.source == ref.model.source and list(t.norm) == list(ref.norm) and
                    list(t.dim_norm_residual) == list(ref.dim_norm_residual) and len(t.parameters) == len(ref.parameters) and
                    len(t.residual_int) == len(ref.residual_int) and len(t.residual_real) == len(ref.residual_real))
            if not same:
                raise ValueError(f"set_tasks: the task of environment {e} differs from the fleet's in model, residual, norm kinds or dimensions")
        self._tasks = tasks
        for p, t in zip(self.envs, tasks):
            p.task = t

    # ---- a model per environment: robots that differ physically (mjcf.variant: a payload, another floor, weaker motors)
    _models = None
    _models_on = (None, None)    # the context and the models of the last successful push: a push of the same pair again is skipped
    _MODELS_FOLLOW_UP = ("a model per environment is not implemented for the planners with a derivative chain (Gradient, iLQG, iLQS): "
                         "their batched derivative calls use the context's one model -- plan such robots on planners of their own")

    def set_models(self, models):
        """One compiled model per environment -- the fleet's robot with other inertial, passive, actuation or contact parameters
        (`mjcf.variant`). Each is packed as `Task.packed_model` packs the fleet's (planning timestep and integrator, the differentiable
        flag) and handed to the context (`set_models_batched`, a setup call: not for a plan loop). Member e then plans exactly like the
        single planner of its kind created on models[e]. After `allocate`; the models are pushed again when `allocate` re-creates the
        context. None: the fleet's one model for every environment again. Composes with `set_tasks`."""
        if self.derivative_chain:
            raise NotImplementedError(self._MODELS_FOLLOW_UP)
        previous = self._models
        if models is None:
            self._models = None
        else:
            models = list(models)
            if len(models) != self.num_envs:
                raise ValueError(f"{len(models)} models for {self.num_envs} environments")
            if self.task is None or self.ctx is None:
                raise ValueError("set_models before allocate")
            for e, m in enumerate(models):
                if m.source != self.task.model.source:
                    raise ValueError(f"set_models: the model of environment {e} was compiled from {m.source!r}, the fleet's from "
                                     f"{self.task.model.source!r}")
            self._models = models
        try:
            self._push_models()
        except Exception:
            self._models = previous      # the context refused (all or nothing there): the planner keeps what it had as well
            raise

    def _push_models(self):
        """hand the environments' models to the context (from set_models, and from allocate when it made a new context: the builders run
        once per model, so a context that already holds these models is left alone)"""
        if self.ctx is None or (self._models_on[0] is self.ctx and self._models_on[1] is self._models):
            return
        if self._models is None:
            if self._models_on[0] is self.ctx:     # (a new context has none to clear)
                self.ctx.set_models_batched(None)
            self._models_on = (self.ctx, None)
            return
        ref = self.task.model
        ts = ref.get_number("agent_timestep", ref.timestep)
        integ = int(ref.get_number("agent_integrator", ref.integrator))
        self.ctx.set_models_batched([PackedModel(m, timestep=ts, integrator=integ, differentiable=bool(self.differentiable))
                                     for m in self._models])
        self._models_on = (self.ctx, self._models)

    def _push_task_rows(self):
        """after ctx.set_states: the environments' own task parameters and frozen residual state, or nothing without set_tasks"""
        ts = self._tasks
        if ts is None:
            if self._rows_pushed:     # set_tasks(None) after a fleet of unlike tasks: everything shared again
                self.ctx.set_task_params_batched()
                self._rows_pushed = False
            return
        rows = lambda name: np.array([getattr(t, name) for t in ts], dtype=np.float64).reshape(len(ts), -1)
        self.ctx.set_task_params_batched(rows("weight"), rows("norm_parameter"), rows("parameters"), np.array([float(t.risk) for t in ts]))
        self._rows_pushed = True
        if hasattr(self.ctx, "set_residual_states") and (ts[0].residual_int or ts[0].residual_real):
            self.ctx.set_residual_states(np.array([t.residual_int for t in ts], dtype=np.int32).reshape(len(ts), -1) if ts[0].residual_int else None,
                                         rows("residual_real") if ts[0].residual_real else None)


class GpuBatchSamplingPlanner(_Fleet):
    """Predictive Sampling for `num_envs` environments (robots) on ONE context: every plan step is one `set_states`, one
    `rollout_noise_batched` over all E x n candidates, one `best_batched` and one sync, instead of E plan steps one after the
    other. The environments share the model and the task (weights, parameters) unless `set_tasks` gives each its own; each has its own
    state, clock, mocap pose and policy. Environment e with seed s behaves exactly like a GpuSamplingPlanner with seed s + e: the per-environment
    logic (nominal resampling, policy copy, ActionFromPolicy) IS that planner's, one member per environment."""

    def __init__(self, num_envs, device=0, precision=64, seed=0, backend_factory=None):
        super().__init__(num_envs, device, precision, backend_factory)
        self.seed = seed
        self.iteration = 0
        self.rollouts_compute_time = self.policy_update_compute_time = 0.0
        # the members never roll out themselves: they are handed the shared context instead of creating their own
        self.envs = [GpuSamplingPlanner(device, precision, seed + e, backend_factory=lambda task: self.ctx) for e in range(self.num_envs)]
        # optimize_policy reads nothing of a launch but each robot's argmin, its nominal's return and the winner's spline -- what a pruned launch
        # keeps exact. pruning: the plan launch retires, per robot, the candidates that can no longer win (set_pruning_batched) and parks the ones
        # the robot's previous best return x (1 + park_slack) condemns (GpuSamplingPlanner::OptimizePolicy of gpu_sampling/planner.cc, per robot).
        # Off by default; the planners built on this one (Robust's delegate, iLQS's sampling half) rank every return and leave it off.
        self.pruning = False
        self.park_slack = DEFAULT_PARK_SLACK   # "sampling_park_slack" in the model; <= -1: no hints
        self.prune_stats = self.park_stats = None   # of the last plan, per robot (capi.Context.prune_stats_batched); None unless it was pruned
        self.park_hints_used = None                 # the hints the last plan's launch ran on (E; +inf: none), None unless it was pruned
        self.pruned_launch_repeated = False         # the last plan's pruned launch was refused (MJPCX_ESTATE) and repeated unpruned
        self._hint = [None] * self.num_envs         # per robot: (previous best return, task signature), or None -- no hint for the next plan

    def initialize(self, model, task: Task):
        super().initialize(model, task)
        self.park_slack = float(model.get_number("sampling_park_slack", DEFAULT_PARK_SLACK))
        self._hint = [None] * self.num_envs

    @property
    def num_trajectory_(self):
        return self.envs[0].num_trajectory_

    @num_trajectory_.setter
    def num_trajectory_(self, n):
        for p in self.envs:
            p.num_trajectory_ = int(n)

    def _reset_own(self):
        self._last = None
        self._hint = [None] * self.num_envs

    def _park_hints(self):
        """Robot e's park hint for the next launch: its previous best return x (1 + park_slack); +inf when it has no previous plan, when
        that plan's best was not finite or was negative or it resumed more than a quarter of its candidates (_hint[e] is None then), or
        when the robot's task row has changed since"""
        hints = np.full(self.num_envs, np.inf)
        if self.park_slack > -1.0:
            for e, p in enumerate(self.envs):
                if self._hint[e] is not None and self._hint[e][1] == task_signature(p.task):
                    hints[e] = self._hint[e][0] * (1.0 + self.park_slack)
        return hints

    def _launch(self, horizon, prune=False):
        """First half of a plan step: every environment's nominal resampled, states and task rows pushed, the E x n candidates
        enqueued in one launch -- nothing read back, no sync. Returns when the rollouts' clock started (rollouts_compute_time)."""
        n = self.num_trajectory_
        self._check_n(n)
        for p in self.envs:
            p.update_nominal_policy(horizon)
            p.policy.plan.set_interpolation(p.interpolation_)
        t0 = _time.perf_counter()
        self._enqueue(horizon, prune)
        return t0

    def _enqueue(self, horizon, prune):
        """the launch of _launch, with the members' nominals as they stand: optimize_policy repeats it unpruned, same seed and iteration,
        when the context refuses the pruned one's argmin"""
        n = self.num_trajectory_
        plans = [p.policy.plan for p in self.envs]
        exploration = self.envs[0].noise_exploration
        ns = capi.make_noise_spec(seed=self.seed, iteration=self.iteration, mode=capi.NOISE_SAMPLING, candidate_offset=0,
                                  nominal_candidate=0, std0=exploration[0], std1=exploration[1])
        self._push_states()
        # (a cost that can be negative in any robot's task row: no pruning for the launch -- partial returns would be no lower bounds there)
        self._pruned = bool(prune) and all(cost_is_non_negative(p.task) for p in self.envs)
        self.park_hints_used = self._park_hints() if self._pruned else None
        if self._pruned:
            self.ctx.set_pruning_batched(True, self.num_envs, None, self.park_hints_used)
        try:
            self.ctx.rollout_noise_batched(n, horizon, plans[0].interpolation(), np.stack([pl.times() for pl in plans]),
                                           np.stack([pl.values() for pl in plans]), ns, num_envs=self.num_envs)
        finally:
            if self._pruned:   # (the switch is sticky and the context is shared with the planners built on this one: on for this launch alone)
                self.ctx.set_pruning_batched(False)
        self._last = "plan"
        self._n = n

    def _finish(self, t0, ranked):
        """Second half: `ranked` yields, per environment, (trajectory_order, scores, winner's place in them, winner's spline values) of
        the rollout _launch enqueued; the members take them as their own planner's."""
        self.rollouts_compute_time = (_time.perf_counter() - t0) * 1e6
        self.iteration += 1
        t0 = _time.perf_counter()
        for p, (order, scores, place, values) in zip(self.envs, ranked):
            p._offset, p._n_local = 0, self._n
            p.trajectory_order, p._scores = [int(i) for i in order], [float(r) for r in scores]
            p.iteration = self.iteration
            p._set_winner(p.trajectory_order[place], values)
        self.policy_update_compute_time = (_time.perf_counter() - t0) * 1e6

    def optimize_policy(self, horizon, pool=None):
        t0 = self._launch(horizon, prune=self.pruning)
        pruned = self._pruned
        self.prune_stats = self.park_stats = None
        self.pruned_launch_repeated = False
        if pruned:
            st = self.ctx.prune_stats_batched(self.num_envs)
            self.prune_stats = {k: st[k] for k in ("retired", "retire_step_sum", "negative_cost", "wavefronts_ended_early", "final_bound")}
            self.park_stats = {k: st[k] for k in ("parked", "settled_retired", "resumed")}
        try:
            idx, best_ret, nominal_ret, values = self.ctx.best_batched(self.num_envs, 0)
        except capi.MjpcxError as err:
            if not pruned or err.code != MJPCX_ESTATE:
                raise
            # some robot's pruned argmin is not proven (a negative step cost; with +inf as the initial bound nothing else leads here): the
            # same candidates again, all to the horizon -- the policy stays exact
            self.pruned_launch_repeated = True
            self._enqueue(horizon, False)
            idx, best_ret, nominal_ret, values = self.ctx.best_batched(self.num_envs, 0)
        self._finish(t0, [([idx[e]], [best_ret[e]], 0, values[e]) for e in range(self.num_envs)])
        for e, p in enumerate(self.envs):
            p.best_return, p.nominal_return = float(best_ret[e]), float(nominal_ret[e])
            p.improvement = max(float(nominal_ret[e] - best_ret[e]), 0.0)
            # the next plan's hint, unless this plan's resume launch shows that the estimate it ran on was stale
            best = float(best_ret[e])
            stale = pruned and float(self.park_stats["resumed"][e]) > K_PARK_MAX_RESUME_SHARE * max(self._n, 1)
            self._hint[e] = (best, task_signature(p.task)) if pruned and np.isfinite(best) and best >= 0 and not stale else None

    def nominal_trajectory(self, horizon, pool=None):
        plans = [(p.winner_policy.plan if p.winner_policy.plan.size() else p.policy.plan) for p in self.envs]
        if any(pl.size() != plans[0].size() for pl in plans):
            raise ValueError("the environments' policies have different numbers of spline nodes")
        if plans[0].size() == 0:
            times = np.array([[p.time] for p in self.envs])
            values = np.zeros((self.num_envs, 1, self.model.nu))
        else:
            times = np.stack([pl.times() for pl in plans])
            values = [pl.values() for pl in plans]
        out = self._nominal_launch(horizon, plans[0].interpolation(), times, values)
        for p, tr in zip(self.envs, out):
            p._best = tr
        return out

    def best_trajectory(self, env):
        p = self.envs[env]
        if p._best is None:
            p._best = self._fetch_planned(env, p.winner)
        return p._best


class GpuEnsembleSamplingPlanner(_Fleet):
    """Predictive Sampling for ONE robot over `num_hypotheses` hypotheses about it -- its model (`set_models`: a payload, another floor,
    weaker motors), its task (`set_tasks`) or its state (`set_states`). Every plan step rolls the SAME n candidates out under every
    hypothesis in one launch (`rollout_noise_ensemble`: the M environments of a fleet's launch, with the noise stream shared) and takes
    the candidate whose score over the hypotheses is lowest (`ensemble_best`): the mean of the `tail` largest of its M returns -- tail
    None or M: the mean, 1: the worst case, in between the tail mean (CVaR). One `set_states`, one launch, one selection, one sync.

    The hypotheses are the fleet's members (`envs`), and what is per hypothesis -- state, task, model and their way to the context -- is
    _Fleet's. The robot has ONE policy, member 0's: nominal resampling, the policy copy and ActionFromPolicy are that GpuSamplingPlanner's
    own code (`member`); the other members hold a hypothesis's state and task and never plan. With one hypothesis, or M alike, the planner
    is GpuSamplingPlanner(seed) bit for bit. No pruning: the score needs every return."""

    def __init__(self, num_hypotheses, device=0, precision=64, seed=0, tail=None, backend_factory=None):
        super().__init__(num_hypotheses, device, precision, backend_factory)
        if self.num_envs > capi.MAX_HYPOTHESES:
            raise ValueError(f"{self.num_envs} hypotheses; mjpcx_ensemble_best takes at most {capi.MAX_HYPOTHESES}")
        self.num_hypotheses, self.seed = self.num_envs, seed
        self.tail = self.num_envs if tail is None else int(tail)
        if not 1 <= self.tail <= self.num_envs:
            raise ValueError(f"tail = {tail} outside 1..{self.num_envs} (the number of hypotheses)")
        self.envs = [GpuSamplingPlanner(device, precision, seed, backend_factory=lambda task: self.ctx) for _ in range(self.num_envs)]
        self.member = self.envs[0]
        self.best_score = self.nominal_score = 0.0      # the last plan's scores of the winner and of candidate 0, the nominal
        self.member_returns = np.zeros(self.num_envs)   # the winner's return under every hypothesis
        self.rollouts_compute_time = self.policy_update_compute_time = 0.0
        self._trajectories = {}

    @property
    def num_trajectory_(self):
        return self.member.num_trajectory_

    @num_trajectory_.setter
    def num_trajectory_(self, n):
        self.member.num_trajectory_ = int(n)

    @property
    def noise_exploration(self):
        return self.member.noise_exploration

    @noise_exploration.setter
    def noise_exploration(self, value):
        self.member.noise_exploration = list(value)

    policy = property(lambda self: self.member.policy)
    winner = property(lambda self: self.member.winner)

    @property
    def winners(self):
        """(_Fleet's list of a winner per robot has no meaning here: the members beside member 0 never plan)"""
        raise AttributeError("GpuEnsembleSamplingPlanner plans for one robot: `winner` is its candidate, `member_returns` its return under every hypothesis")
    improvement = property(lambda self: self.member.improvement)
    iteration = property(lambda self: self.member.iteration)

    def _reset_own(self):
        self._last = None
        self._trajectories = {}

    def set_state(self, state: State):
        """the one robot: every hypothesis starts from this state (set_states: a hypothesis each about the state, too)"""
        self.set_states([state] * self.num_envs)

    def optimize_policy(self, horizon, pool=None):
        m, M = self.member, self.num_envs
        n = m.num_trajectory_
        self._check_n(n)
        m.update_nominal_policy(horizon)
        t0 = _time.perf_counter()
        plan = m.policy.plan
        plan.set_interpolation(m.interpolation_)
        ns = capi.make_noise_spec(seed=self.seed, iteration=m.iteration, mode=capi.NOISE_SAMPLING, candidate_offset=0, nominal_candidate=0,
                                  std0=m.noise_exploration[0], std1=m.noise_exploration[1])
        self._push_states()
        self.ctx.rollout_noise_ensemble(n, horizon, plan.interpolation(), plan.times(), plan.values(), ns, num_hypotheses=M)
        self._last, self._n, self._trajectories = "plan", n, {}
        idx, best, nominal, members, values, _ = self.ctx.ensemble_best(M, self.tail, 0)
        self.rollouts_compute_time = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        m._offset, m._n_local = 0, n
        m.trajectory_order, m._scores = [int(idx)], [float(best)]
        m.iteration += 1
        m._set_winner(int(idx), values)
        self.best_score, self.nominal_score = float(best), float(nominal)
        self.member_returns = np.array(members[:M], float)
        m.best_return, m.nominal_return = self.best_score, self.nominal_score
        m.improvement = max(self.nominal_score - self.best_score, 0.0)
        self.policy_update_compute_time = (_time.perf_counter() - t0) * 1e6

    def action_from_policy(self, action, state, time, use_previous=False):
        """the one robot's action (GpuSamplingPlanner's signature, not the fleets': there is no environment to name)"""
        return self.member.action_from_policy(action, state, time, use_previous)

    def best_trajectory(self, hypothesis=0):
        """the winner rolled out under `hypothesis` (candidate hypothesis * n + winner of the plan launch)"""
        if not 0 <= hypothesis < self.num_envs:
            raise ValueError(f"hypothesis {hypothesis} outside 0..{self.num_envs - 1}")
        if hypothesis not in self._trajectories:
            tr = self._fetch_planned(hypothesis, self.member.winner)
            if tr is None:
                return None
            self._trajectories[hypothesis] = tr
        return self._trajectories[hypothesis]


def task_signature(task):
    """GpuSamplingPlanner::TaskSignature: what a robot's park hint is tied to -- weights, parameters, norm kinds and parameters, risk"""
    return ([float(x) for x in task.weight] + [float(x) for x in task.parameters] + [float(int(k)) for k in task.norm] +
            [float(x) for x in task.norm_parameter] + [float(task.risk)])


def _park_hint(hint, task, slack):
    """the park hint of the next launch from a planner's (previous return, task signature) record: the return x (1 + slack); +inf when there
    is no record, when slack <= -1, or when the task row has changed since"""
    if hint is None or not slack > -1.0 or hint[1] != task_signature(task):
        return np.inf
    return hint[0] * (1.0 + slack)


def cost_is_non_negative(task):
    """GpuSamplingPlanner::CostIsNonNegative: pruning needs every step's cost >= 0 in floating point -- weights >= 0, no risk transform, and
    the norm kinds whose computed value is shown to be >= 0"""
    if not abs(float(task.risk)) < 1.0e-6:
        return False
    ok = (NORM_QUADRATIC, NORM_L2, NORM_POWER_LOSS, NORM_SMOOTH_ABS, NORM_RECTIFY)
    return all(float(w) >= 0 for w in task.weight) and all(int(k) in ok for k in task.norm)


def _fleet_setting(name):
    """a planner setting that all environments of a batch planner share: read from the first member, written to every member"""
    def fget(self):
        return getattr(self.envs[0], name)

    def fset(self, value):
        for p in self.envs:
            setattr(p, name, value)
    return property(fget, fset)


def robust_scores(scores, returns, failure, repetitions):
    """RobustPlanner::OptimizePolicy's choice (robust_planner.cc:141-163), in its order of operations: per ranked candidate, from its
    unperturbed score, the running mean over the perturbed rollouts [candidate * repetitions, +repetitions) that did not fail; the
    lowest mean wins, strict < from candidate 0 up. -> (perturbed_score, valid rollouts per candidate, best_candidate)"""
    perturbed, valid, best, best_score = [], [], -1, 0.0
    for candidate, mean_return in enumerate(float(x) for x in scores):
        valid_rollouts = 0
        for j in range(repetitions * candidate, repetitions * (candidate + 1)):
            if failure[j]:
                continue
            mean_return = (valid_rollouts * mean_return + float(returns[j])) / (valid_rollouts + 1)
            valid_rollouts += 1
        perturbed.append(mean_return)
        valid.append(valid_rollouts)
        if best == -1 or mean_return < best_score:
            best, best_score = candidate, mean_return
    return perturbed, valid, best


class GpuRobustPlanner(_ContextOwner):
    """mjpc::RobustPlanner (mjpc/planners/robust/robust_planner.{h,cc}) with both fan-outs on the device, the mirror of the C++
    GpuRobustPlanner for one rank: the delegate (a GpuSamplingPlanner) ranks its candidates, the `robust_candidates` best are rolled
    out `robust_repetitions` times each under Ornstein-Uhlenbeck force noise in ONE launch on a second context (the delegate's
    rollout stays fetchable), and the candidate with the best mean perturbed return becomes the policy."""

    def __init__(self, delegate, device=0, precision=64, seed=0, backend_factory=None):
        if delegate.group is not None and delegate.group.world > 1:
            raise ValueError("GpuRobustPlanner plans on one rank; the sharded Robust planner is HostPlanner(kind='robust')")
        self.delegate = delegate
        self.device, self.precision, self.seed = device, precision, seed
        self._backend_factory = backend_factory
        self.model = self.task = self.ctx = None
        self.iteration = 0          # of the perturbed launches: the force noise of launch i is keyed on rollouts [i k R, (i + 1) k R)
        self.best_candidate = -1
        self.perturbed_score = []

    # ---- Initialize, robust_planner.cc:30-50
    def initialize(self, model, task: Task):
        self.delegate.initialize(model, task)
        self.model, self.task = model, task
        self.nrepetitions_ = int(model.get_number("robust_repetitions", 5))
        self.ncandidates_ = int(model.get_number("robust_candidates", -1))
        if self.ncandidates_ == -1:   # derived from the number of rollouts in the sampling config
            self.ncandidates_ = int(model.get_number("sampling_trajectories", 10)) // max(self.nrepetitions_, 1)
        self.xfrc_std_ = model.get_number("robust_xfrc", 0.1)
        self.xfrc_rate_ = model.get_number("robust_xfrc_rate", 0.1)

    def allocate(self):
        self.delegate.allocate()
        self.ctx = self._create_context()

    def reset(self, horizon, initial_repeated_action=None):
        self.delegate.reset(horizon, initial_repeated_action)
        self.best_candidate = -1

    def set_state(self, state: State):
        self.delegate.set_state(state)

    # ---- OptimizePolicy, robust_planner.cc:90-170
    def optimize_policy(self, horizon, pool=None):
        d = self.delegate
        k = d.optimize_policy_candidates(self.ncandidates_, horizon, pool)
        if not k:
            return
        if k == 1:   # a single candidate: nothing to compare
            self.best_candidate = 0
            d.copy_candidate_to_policy(0)
            return
        R = max(self.nrepetitions_, 1)
        plans = []
        for i in range(k):
            p = SamplingPolicy()
            d._load_candidate_plan(p, d.trajectory_order[i])
            plans.append(p.plan)
        values = np.stack([np.broadcast_to(pl.values()[None], (R,) + pl.values().shape) for pl in plans])   # rollout j = candidate * R + repetition
        sync_task(self.ctx, self.task)
        self.ctx.set_state(d.state, d.time, d.mocap, d.userdata)
        self.ctx.rollout_splines_noisy(horizon, plans[0].interpolation(), plans[0].times(), values, self.xfrc_std_, self.xfrc_rate_,
                                       seed=self.seed, candidate_offset=self.iteration * k * R)
        self.iteration += 1
        ret, fail = self.ctx.returns()
        self.perturbed_score, self.valid_rollouts, self.best_candidate = robust_scores(d._scores[:k], ret, fail, R)
        d.copy_candidate_to_policy(self.best_candidate)

    def nominal_trajectory(self, horizon, pool=None):
        return self.delegate.nominal_trajectory(horizon, pool)

    def action_from_policy(self, action, state, time, use_previous=False):
        return self.delegate.action_from_policy(action, state, time, use_previous)

    def best_trajectory(self):
        """the chosen candidate's UNPERTURBED trajectory, from the delegate's context"""
        return self.delegate.best_trajectory()

    def num_parameters(self):
        return self.delegate.num_parameters()


class GpuBatchRobustPlanner(_Fleet):
    """The Robust planner for `num_envs` robots on two contexts of one model: a plan step is the delegate fleet's launch
    (GpuBatchSamplingPlanner: states and task rows pushed, E x n candidates rolled out, nothing read back) and one
    `robust_step_batched` on the second context -- per environment the k best candidates selected, replicated R times, rolled out
    under force noise and scored on the device -- two launch sequences and ONE sync. Member e plans exactly like
    GpuRobustPlanner(GpuSamplingPlanner(seed = s + e), seed = s + e): the per-robot logic IS that planner's, one member per
    environment over the delegate fleet's member."""
    ncandidates_ = _fleet_setting("ncandidates_")
    nrepetitions_ = _fleet_setting("nrepetitions_")
    xfrc_std_ = _fleet_setting("xfrc_std_")
    xfrc_rate_ = _fleet_setting("xfrc_rate_")

    def __init__(self, num_envs, device=0, precision=64, seed=0, backend_factory=None):
        self.delegate = GpuBatchSamplingPlanner(num_envs, device, precision, seed, backend_factory)
        super().__init__(num_envs, device, precision, backend_factory)
        self.seed = seed
        self.iteration = 0
        # the members never roll out themselves: each sits on the delegate fleet's member and is handed the second context
        self.envs = [GpuRobustPlanner(p, device, precision, seed + e, backend_factory=lambda task: self.ctx) for e, p in enumerate(self.delegate.envs)]

    def initialize(self, model, task: Task):
        self.delegate.initialize(model, task)
        super().initialize(model, task)   # (a member initialises its delegate, the delegate fleet's member, once more: the same values)

    @property
    def num_trajectory_(self):
        return self.delegate.num_trajectory_

    @num_trajectory_.setter
    def num_trajectory_(self, n):
        self.delegate.num_trajectory_ = n

    def set_tasks(self, tasks):
        super().set_tasks(tasks)
        self.delegate.set_tasks(tasks)

    def allocate(self):
        self.delegate.allocate()
        self.ctx = self._create_context()
        for p in self.envs:
            p.ctx = self.ctx
        self._push_models()

    def set_models(self, models):
        """both contexts: the delegate fleet's candidates and the rollouts under force noise run on the environment's model"""
        previous = self._models
        super().set_models(models)           # (refused: nothing changed anywhere)
        try:
            self.delegate.set_models(models)
        except Exception:
            super().set_models(previous)     # the delegate's context kept what it had: this one goes back to the same
            raise

    def reset(self, horizon, initial_repeated_action=None):
        self.delegate.reset(horizon, initial_repeated_action)
        for p in self.envs:
            p.best_candidate = -1

    def set_states(self, states):
        self.delegate.set_states(states)

    def _push_states(self):
        """the delegate fleet's states and task rows, to the second context"""
        super()._push_states(self.delegate.envs)

    def optimize_policy(self, horizon, pool=None):
        d = self.delegate
        k, R = min(self.ncandidates_, d.num_trajectory_), max(self.nrepetitions_, 1)
        if k == 1:   # nothing to compare: the delegate fleet's ordinary step (OptimizePolicyCandidates(1) + CopyCandidateToPolicy(0))
            d.optimize_policy(horizon, pool)
            for p in self.envs:
                p.best_candidate = 0
            return
        t0 = d._launch(horizon)
        self._push_states()
        plans = [p.policy.plan for p in d.envs]
        out = self.ctx.robust_step_batched(d.ctx, self.num_envs, k, R, horizon, plans[0].interpolation(), np.stack([pl.times() for pl in plans]),
                                           self.xfrc_std_, self.xfrc_rate_, seed=self.seed, candidate_offset=self.iteration * k * R)
        self.iteration += 1
        d._finish(t0, [(out["candidate"][e], out["candidate_return"][e], int(out["best"][e]), out["spline"][e]) for e in range(self.num_envs)])
        for e, p in enumerate(self.envs):
            p.iteration = self.iteration
            p.best_candidate = int(out["best"][e])
            p.perturbed_score = [float(x) for x in out["perturbed_score"][e]]
            p.valid_rollouts = [int(x) for x in out["valid"][e]]

    @property
    def winners(self):
        return self.delegate.winners

    def nominal_trajectory(self, horizon, pool=None):
        return self.delegate.nominal_trajectory(horizon, pool)

    def action_from_policy(self, env, action, state, time, use_previous=False):
        return self.delegate.action_from_policy(env, action, state, time, use_previous)

    def best_trajectory(self, env):
        """the chosen candidate's unperturbed trajectory, fetched lazily from the delegate's context (global candidate env * n + winner)"""
        return self.delegate.best_trajectory(env)

    def num_parameters(self):
        return self.delegate.num_parameters()


def strided_tree_sum(terms):
    """The summation order of the device's Sample-Gradient update (sg_update_kernel), over the first axis of `terms`: partial sum t of
    256 adds the terms t, t + 256, t + 512, ... in that order from 0; then sum[t] += sum[t + s] for s = 128, 64, ..., 1."""
    terms = np.asarray(terms, dtype=np.float64)
    acc = np.zeros((256,) + terms.shape[1:])
    for k in range(0, terms.shape[0], 256):
        chunk = terms[k:k + 256]
        acc[:chunk.shape[0]] += chunk
    s = 128
    while s:
        acc[:s] += acc[s:2 * s]
        s >>= 1
    return acc[0]


def sample_gradient_update(returns, nominal, noise, num_gradient, ctrlrange, weights=None, gradient=None, compute_weights=True,
                           gradient_filter=1.0, max_step=2.0, min_step=1.0e-3, noise_exploration=0.1):
    """The Sample-Gradient planner's update after its rollouts (sample_gradient/planner.cc:168-264 and 401-493) for one robot, in the
    device's order of operations -- the single statement of the arithmetic of mjpcx_sample_gradient_update_batched.
    `returns` n, `nominal` the nominal's P*nu parameters, `noise` the standard normals n x P*nu of the candidates (the rows of the
    nominal and of the gradient candidates are taken as zero, whatever they hold), `weights` the cached shaping weights (needed without
    compute_weights), `gradient` the estimate of the step before (None: zero). The reference's behaviour is kept, not repaired: the
    shaping weight of sorted position i takes log(candidate index at that position + 1), not log(i + 1); weights computed in this step
    pair with the order of the first num_noisy returns alone, cached ones with the first num_noisy entries of the order over all n.
    -> dict of order (ascending returns, ties to the lower index, NaN last), winner, winner_type (0 nominal, 1 perturbed, 2 gradient),
    improvement, weights, gradient, gradient_previous, candidates (num_gradient x P*nu: the next gradient candidates)."""
    ret = np.asarray(returns, dtype=np.float64).reshape(-1)
    n, G = ret.size, int(num_gradient)
    nn = n - G
    if not 0 <= G <= n - 1:
        raise ValueError(f"num_gradient = {G} outside 0..{n - 1}")
    order = np.lexsort((np.arange(n), ret))
    winner = int(order[0]) if ret[order[0]] < ret[0] else 0
    d = ret[0] - ret[winner]
    out = dict(order=order, winner=winner, winner_type=0 if winner == 0 else (1 if winner < nn else 2),
               improvement=float(d) if d > 0 else 0.0, weights=weights, gradient=gradient, gradient_previous=None, candidates=None)
    if G < 1:
        return out
    nominal = np.asarray(nominal, dtype=np.float64).reshape(-1)
    previous = np.zeros(nominal.size) if gradient is None else np.asarray(gradient, dtype=np.float64).reshape(-1).copy()
    if compute_weights:
        used = np.lexsort((np.arange(nn), ret[:nn]))
        f0 = math.log(0.5 * nn + 1.0)
        f = np.array([max(0.0, f0 - math.log(int(c) + 1)) for c in used])
        weights = f / strided_tree_sum(f) - 1.0 / nn
    else:
        weights = np.asarray(weights, dtype=np.float64).reshape(-1)
        if weights.size != nn:
            raise ValueError(f"{weights.size} cached weights for {nn} noisy candidates")
        used = order[:nn]
    z = np.asarray(noise, dtype=np.float64).reshape(n, nominal.size)[used]
    z = np.where(((used > 0) & (used < nn))[:, None], z, 0.0)
    g = strided_tree_sum(z * (weights / nn)[:, None])
    b = np.asarray(ctrlrange, dtype=np.float64).reshape(-1, 2)
    lo, hi = np.resize(b[:, 0], nominal.size), np.resize(b[:, 1], nominal.size)   # parameter j belongs to actuator j % nu
    candidates = np.zeros((G, nominal.size))
    for i, step in enumerate(log_scale(max_step, min_step, G)):
        scaling = step / noise_exploration
        v = nominal.copy()
        v += -scaling * gradient_filter * g
        v += -scaling * (1.0 - gradient_filter) * previous
        candidates[i] = np.maximum(lo, np.minimum(hi, v))
    out.update(weights=weights, gradient=g, gradient_previous=previous, candidates=candidates)
    return out


class _SampleGradientMember:
    """what mjpc::SampleGradientPlanner keeps per robot: state, policies, winner, gradient"""

    def __init__(self, seed):
        self.seed = seed
        self.task = None
        self.mtx_ = threading.RLock()
        self.winner, self.winner_type_, self.improvement, self.iteration = 0, 0, 0.0, 0
        self.best_return = self.nominal_return = 0.0
        self.gradient = np.zeros(0)
        self._best = None

    def initialize(self, model, task: Task):
        self.model, self.task = model, task

    # ---- Allocate, planner.cc:73-112
    def allocate(self):
        m = self.model
        self.state, self.mocap, self.userdata, self.time = np.zeros(m.nq + m.nv + m.na), np.zeros(7 * m.nmocap), np.zeros(m.nuserdata), 0.0
        self.policy, self.previous_policy = SamplingPolicy(), SamplingPolicy()
        self.policy.allocate(m, self.task, K_MAX_TRAJECTORY_HORIZON)
        self.previous_policy.allocate(m, self.task, K_MAX_TRAJECTORY_HORIZON)
        self.gradient = np.zeros(self.policy.num_spline_points * m.nu)

    # ---- Reset, planner.cc:115-163: the gradient is zeroed
    def reset(self, horizon, initial_repeated_action=None):
        self.state[:] = 0
        self.mocap[:] = 0
        self.userdata[:] = 0
        self.time = 0.0
        with self.mtx_:
            self.policy.reset(horizon, initial_repeated_action)
            self.previous_policy.reset(horizon, initial_repeated_action)
        self.improvement, self.winner, self._best = 0.0, 0, None
        self.gradient = np.zeros_like(self.gradient)

    def set_state(self, state: State):
        self.state, self.mocap, self.userdata, self.time = state.copy_to()

    def action_from_policy(self, action, state, time, use_previous=False):
        with self.mtx_:
            return (self.previous_policy if use_previous else self.policy).action(action, state, time)

    def num_parameters(self):
        return self.policy.num_spline_points * self.model.nu


class GpuBatchSampleGradientPlanner(_Fleet):
    """mjpc::SampleGradientPlanner (mjpc/planners/sample_gradient/planner.{h,cc}) for `num_envs` robots on ONE context, the candidates,
    the sort, the fitness-shaped gradient estimate and the gradient-step candidates on the device: a plan step is the host resample of
    every nominal, one `set_states`, one `rollout_sample_gradient_batched`, one `sample_gradient_update_batched` and ONE sync. The
    shaping weights, the gradient and the next gradient candidates never leave the context. Member e plans exactly like
    GpuSampleGradientPlanner(seed = s + e), which is this class with one environment.
    Deviations from the reference, beside the seedable counter-based normals and the lifted candidate cap (F5): the noise rows
    of the nominal and of the gradient candidates are zero (the reference leaves stale rows behind a change of num_gradient_); a change
    of num_gradient_ or of the number of spline points starts the gradient candidates again from the zero spline, as a reset does."""

    def __init__(self, num_envs, device=0, precision=64, seed=0, backend_factory=None):
        super().__init__(num_envs, device, precision, backend_factory)
        self.seed = seed
        self.iteration = 0
        self.rollouts_compute_time = self.policy_update_compute_time = 0.0
        self.gradient_max_step_size, self.gradient_min_step_size = 2.0, 1.0e-3   # planner.h
        self.envs = [_SampleGradientMember(seed + e) for e in range(self.num_envs)]
        self._weights_for = None      # num_noisy the context's shaping weights were computed for (return_weight_.size())
        self._zero_gradient = True    # the context's gradient is to be taken as zero (Allocate / Reset)
        self._candidates_for = None   # (num_gradient, spline points) of the gradient candidates on the device; None: upload the zero spline

    # ---- Initialize, planner.cc:41-70
    def initialize(self, model, task: Task):
        super().initialize(model, task)
        self.noise_exploration = model.get_number("sampling_exploration", 0.1)
        self.num_trajectory_ = int(model.get_number("sampling_trajectories", 10))
        self.interpolation_ = int(model.get_number("sampling_representation", CUBIC))
        self.num_gradient_ = int(model.get_number("sample_gradient_trajectories", 0))
        self.gradient_filter_ = model.get_number("sample_gradient_filter", 1.0)

    def allocate(self):
        super().allocate()
        self._reset_own()

    def _reset_own(self):
        """the context's gradient and gradient candidates start again; its shaping weights are kept (planner.cc:115-163)"""
        self._zero_gradient, self._candidates_for = True, None

    # ---- ResamplePolicy, planner.cc:290-318
    def _resample(self, p, horizon):
        num_spline_points = p.policy.num_spline_points
        # model->opt.timestep as the C++ GpuSampleGradientPlanner reads it: the model's own timestep, where the sibling planners read
        # agent_timestep first. In the reference the planner's model is the Agent's planning copy, whose opt.timestep IS agent_timestep;
        # here a model that defines agent_timestep (Cartpole, Particle, the Humanoid) gets its nodes spaced by the model's own. Kept, so
        # that this class and the C++ planner stay one specification (deviations); to be changed in both together.
        timestep = self.model.timestep
        time_shift = max((horizon - 1) * timestep / (num_spline_points - 1), 1.0e-5) if num_spline_points > 1 else 1.0e-5
        plan = TimeSpline(self.model.nu, self.interpolation_)
        nominal_time = p.time
        with p.mtx_:
            for _ in range(num_spline_points):
                node = plan.add_node(nominal_time)
                p.policy.action(node, None, nominal_time)
                nominal_time += time_shift
        return plan

    # ---- OptimizePolicy, planner.cc:166-264
    def optimize_policy(self, horizon, pool=None):
        n = int(self.num_trajectory_)
        self._check_n(n)
        self.num_gradient_ = G = min(int(self.num_gradient_), n - 1)
        E, nu = self.num_envs, self.model.nu
        for p in self.envs:
            p.policy.plan.set_interpolation(self.interpolation_)
        plans = [self._resample(p, horizon) for p in self.envs]     # the nominal at the environment's clock: candidate 0
        times = np.stack([pl.times() for pl in plans])
        P = times.shape[1]
        t0 = _time.perf_counter()
        self._push_states()
        upload = G > 0 and self._candidates_for != (G, P)
        # the gradient candidates' splines before the first update are empty (candidate_policy[i].Reset): zero actions, clamped
        zero_spline = clamp(np.zeros((E, G, P, nu)), self.model.actuator_ctrlrange) if upload else None
        self.ctx.rollout_sample_gradient_batched(n, G, horizon, self.interpolation_, times, np.stack([pl.values() for pl in plans]),
                                                 self.noise_exploration, seed=self.seed, iteration=self.iteration,
                                                 gradient_values=zero_spline, gradient_times=times if upload else None, num_envs=E)
        flags = 0
        if G > 0 and self._weights_for != n - G:      # return_weight_.size() != num_noisy
            flags |= capi.SG_COMPUTE_WEIGHTS
        if self._zero_gradient:
            flags |= capi.SG_ZERO_GRADIENT
        out = self.ctx.sample_gradient_update_batched(E, G, flags, self.gradient_filter_, self.gradient_max_step_size,
                                                      self.gradient_min_step_size, self.noise_exploration)
        self.rollouts_compute_time = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        if G > 0:
            self._weights_for, self._candidates_for = n - G, (G, P)
        self._zero_gradient = False
        self._last, self._n = "plan", n
        self.iteration += 1
        for e, p in enumerate(self.envs):
            p.winner, p.winner_type_ = int(out["index"][e]), int(out["winner_type"][e])
            p.best_return, p.nominal_return = float(out["best_return"][e]), float(out["nominal_return"][e])
            p.improvement = float(out["improvement"][e])
            p.gradient = np.array(out["gradient"][e], dtype=np.float64).reshape(-1)
            p.iteration = self.iteration
            plan = TimeSpline(nu, self.interpolation_)
            for t, v in zip(times[e], np.asarray(out["spline"][e]).reshape(P, nu)):
                plan.add_node(t, v)
            with p.mtx_:
                p.previous_policy.copy_from(p.policy)
                p.policy.plan = plan                    # policy.SetPlan(candidate_policy[winner].plan)
            p._best = None
        self.policy_update_compute_time = (_time.perf_counter() - t0) * 1e6

    def best_trajectory(self, env):
        """the winner's trajectory, fetched lazily from the context"""
        p = self.envs[env]
        if p._best is None:
            p._best = self._fetch_planned(env, p.winner)
        return p._best


def _member_attr(name):
    def fget(self):
        return getattr(self.fleet.envs[0], name)
    return property(fget)


def _fleet_attr(name):
    def fget(self):
        return getattr(self.fleet, name)

    def fset(self, value):
        setattr(self.fleet, name, value)
    return property(fget, fset)


class GpuSampleGradientPlanner:
    """mjpc::SampleGradientPlanner with everything but the nominal's resampling on the device: the Python mirror of the C++
    GpuSampleGradientPlanner (host/mjpc/planners/gpu_sample_gradient), and GpuBatchSampleGradientPlanner with ONE environment -- the
    same code, so a fleet's member e IS this planner with seed s + e. The candidate count must be a multiple of 64."""
    winner, winner_type_, improvement, gradient = (_member_attr(k) for k in ("winner", "winner_type_", "improvement", "gradient"))
    best_return, nominal_return = _member_attr("best_return"), _member_attr("nominal_return")
    policy, previous_policy = _member_attr("policy"), _member_attr("previous_policy")
    iteration, ctx, model, task = (_fleet_attr(k) for k in ("iteration", "ctx", "model", "task"))
    num_trajectory_, num_gradient_, gradient_filter_ = (_fleet_attr(k) for k in ("num_trajectory_", "num_gradient_", "gradient_filter_"))
    noise_exploration, interpolation_ = _fleet_attr("noise_exploration"), _fleet_attr("interpolation_")
    gradient_max_step_size, gradient_min_step_size = _fleet_attr("gradient_max_step_size"), _fleet_attr("gradient_min_step_size")

    def __init__(self, device=0, precision=64, seed=0, backend_factory=None):
        self.fleet = GpuBatchSampleGradientPlanner(1, device, precision, seed, backend_factory)
        self.seed = seed

    def initialize(self, model, task: Task):
        self.fleet.initialize(model, task)

    def allocate(self):
        self.fleet.allocate()

    def reset(self, horizon, initial_repeated_action=None):
        self.fleet.reset(horizon, initial_repeated_action)

    def set_state(self, state: State):
        self.fleet.set_states([state])

    def optimize_policy(self, horizon, pool=None):
        self.fleet.optimize_policy(horizon, pool)

    def action_from_policy(self, action, state, time, use_previous=False):
        return self.fleet.action_from_policy(0, action, state, time, use_previous)

    def best_trajectory(self):
        return self.fleet.best_trajectory(0)

    def num_parameters(self):
        return self.fleet.num_parameters()


class GpuBatchMPPIPlanner(GpuBatchSamplingPlanner):
    """MPPI (model predictive path integral control) for `num_envs` environments on ONE context: Predictive Sampling's plan launch,
    unchanged -- the same noise, seeds (seed + e) and candidates, local candidate 0 the un-noised nominal -- followed by the softmin in
    place of the argmin (`mppi_update_batched`, one sync): member e's new policy is the mean of ALL its candidates' splines, the
    nominal's among them, weighted by exp(-(R - R_min) / temperature[e]). As the temperature goes to 0 this is Predictive Sampling, as
    it grows the plain mean of the candidates.

    `temperature`: a scalar or one value per environment, on the scale of the task's returns; settable between plan steps. None: read
    from the model's custom numeric `mppi_temperature` in `initialize` (ValueError when the model has none: there is no default that
    fits every task). Every return is needed, so there is no `pruning` here. A member whose best return is NaN or +inf (`valid` 0)
    keeps its policy. `best_trajectory(env)` is the rollout of the member's LOWEST-RETURN candidate (`winner`), not of the averaged
    policy, which was never rolled out; `nominal_trajectory` rolls the averaged policies out. Per member after a plan: `best_return`,
    `nominal_return`, `improvement` (as Predictive Sampling's), `effective_samples` ((sum w)^2 / sum w^2), `weight_sum`, `valid`."""

    def __init__(self, num_envs, device=0, precision=64, seed=0, temperature=None, backend_factory=None):
        super().__init__(num_envs, device, precision, seed, backend_factory)
        del self.pruning
        self._temperature = None
        self._temperature_given = temperature is not None
        if temperature is not None:
            self.temperature = temperature

    @property
    def temperature(self):
        """the E temperatures (None before `initialize` when none was given)"""
        return self._temperature

    @temperature.setter
    def temperature(self, value):
        t = np.asarray(value, dtype=np.float64).reshape(-1)
        if t.size == 1:
            t = np.full(self.num_envs, t[0])
        if t.size != self.num_envs:
            raise ValueError(f"{t.size} temperatures for {self.num_envs} environments")
        if not (np.all(np.isfinite(t)) and np.all(t > 0)):
            raise ValueError(f"temperature {t.tolist()}: every value must be finite and > 0")
        self._temperature, self._temperature_given = t.copy(), True

    def initialize(self, model, task: Task):
        super().initialize(model, task)
        if not self._temperature_given:
            if "mppi_temperature" not in model.numeric:
                raise ValueError(f"{type(self).__name__}: no temperature given and the model has no custom numeric mppi_temperature "
                                 "(its right value is on the scale of the task's returns)")
            self.temperature = model.get_number("mppi_temperature")
            self._temperature_given = False     # (the model's: read again by the next initialize)

    def optimize_policy(self, horizon, pool=None):
        t0 = self._launch(horizon)
        out = self.ctx.mppi_update_batched(self.num_envs, self._temperature, 0)
        # (a member that is not valid: its resampled nominal, whatever the context made of candidate 0's spline)
        values = [out["mean"][e] if out["valid"][e] else p.policy.plan.values() for e, p in enumerate(self.envs)]
        self._finish(t0, [([out["index"][e]], [out["best_return"][e]], 0, values[e]) for e in range(self.num_envs)])
        for e, p in enumerate(self.envs):
            p.best_return, p.nominal_return = float(out["best_return"][e]), float(out["ref_return"][e])
            p.improvement = max(p.nominal_return - p.best_return, 0.0)
            p.effective_samples, p.weight_sum = float(out["effective_samples"][e]), float(out["weight_sum"][e])
            p.valid = int(out["valid"][e])


class GpuMPPIPlanner:
    """MPPI for one robot: GpuBatchMPPIPlanner with ONE environment -- the same code, so a fleet's member e IS this planner with seed
    s + e. The candidate count must be a multiple of 64. `best_trajectory()` is the lowest-return candidate's rollout."""
    winner, improvement, best_return, nominal_return = (_member_attr(k) for k in ("winner", "improvement", "best_return", "nominal_return"))
    effective_samples, weight_sum, valid = (_member_attr(k) for k in ("effective_samples", "weight_sum", "valid"))
    policy, previous_policy, noise_exploration = (_member_attr(k) for k in ("policy", "previous_policy", "noise_exploration"))
    iteration, ctx, model, task, num_trajectory_ = (_fleet_attr(k) for k in ("iteration", "ctx", "model", "task", "num_trajectory_"))

    def __init__(self, device=0, precision=64, seed=0, temperature=None, backend_factory=None):
        self.fleet = GpuBatchMPPIPlanner(1, device, precision, seed, temperature, backend_factory)
        self.seed = seed

    @property
    def temperature(self):
        t = self.fleet.temperature
        return None if t is None else float(t[0])

    @temperature.setter
    def temperature(self, value):
        self.fleet.temperature = value

    def initialize(self, model, task: Task):
        self.fleet.initialize(model, task)

    def allocate(self):
        self.fleet.allocate()

    def reset(self, horizon, initial_repeated_action=None):
        self.fleet.reset(horizon, initial_repeated_action)

    def set_state(self, state: State):
        self.fleet.set_states([state])

    def optimize_policy(self, horizon, pool=None):
        self.fleet.optimize_policy(horizon, pool)

    def action_from_policy(self, action, state, time, use_previous=False):
        return self.fleet.action_from_policy(0, action, state, time, use_previous)

    def best_trajectory(self):
        return self.fleet.best_trajectory(0)

    def num_parameters(self):
        return self.fleet.num_parameters()


def cma_parameters(d, lam):
    """Hansen's default strategy parameters (The CMA Evolution Strategy: A Tutorial, table 1, positive weights only) for d parameters
    and lam ranked candidates: dict of mu = lam // 2, weights (mu, w_i proportional to ln((lam + 1) / 2) - ln i, summing to 1),
    mu_eff, c_sigma, d_sigma, c_c, c_one, c_mu = min(1 - c_one, .), chi = E|N(0, I_d)|."""
    d, lam = int(d), int(lam)
    mu = lam // 2
    if d < 1 or mu < 1:
        raise ValueError(f"cma_parameters: d = {d}, lam = {lam}; needs d >= 1 and lam >= 2")
    raw = np.array([math.log((lam + 1) / 2.0) - math.log(i) for i in range(1, mu + 1)])
    w = raw / raw.sum()
    mu_eff = float(1.0 / np.sum(w * w))
    c_sigma = (mu_eff + 2.0) / (d + mu_eff + 5.0)
    d_sigma = 1.0 + 2.0 * max(0.0, math.sqrt((mu_eff - 1.0) / (d + 1.0)) - 1.0) + c_sigma
    c_c = (4.0 + mu_eff / d) / (d + 4.0 + 2.0 * mu_eff / d)
    c_one = 2.0 / ((d + 1.3) ** 2 + mu_eff)
    c_mu = min(1.0 - c_one, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((d + 2.0) ** 2 + mu_eff))
    chi = math.sqrt(d) * (1.0 - 1.0 / (4.0 * d) + 1.0 / (21.0 * d * d))
    return dict(mu=mu, weights=w, mu_eff=mu_eff, c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_one=c_one, c_mu=c_mu, chi=chi)


def cma_lower_times(A, z):
    """y[..., a] = sum_{b <= a} A[a][b] z[..., b], b ascending from 0.0, every product and sum rounded on its own: the candidates' and
    the update's matrix-vector product (cma_row, csrc/cma_update.h)"""
    A, z = np.asarray(A, dtype=np.float64), np.asarray(z, dtype=np.float64)
    y = np.zeros(z.shape)
    for b in range(A.shape[0]):
        y[..., b:] += z[..., b:b + 1] * A[b:, b]
    return y


def cma_factor(C, pivot_floor=0.0):
    """The lower Cholesky factor by columns in the device's order (cma_factor, csrc/cma_update.h): acc = sum_{k < b} A[a][k] A[b][k]
    ascending from 0.0, s = C[a][b] - acc, the diagonal needs s > pivot_floor * C[b][b] and is sqrt(s), below it s / A[b][b].
    -> A, or None when a pivot fails."""
    C = np.asarray(C, dtype=np.float64)
    d = C.shape[0]
    A = np.zeros((d, d))
    for b in range(d):
        acc = np.zeros(d - b)
        for k in range(b):
            acc += A[b:, k] * A[b, k]
        s = C[b:, b] - acc
        if not s[0] > pivot_floor * C[b, b]:
            return None
        A[b, b] = np.sqrt(s[0])
        A[b + 1:, b] = s[1:] / A[b, b]
    return A


def cma_candidates(nominal, z, sigma, A, ctrlrange):
    """The n candidates of mjpcx_rollout_cma_batched in its order of operations: row 0 the mean as given, row c >= 1
    clamp(m + (sigma s) (A z[c])), s the half control range; nominal d (parameter j belongs to actuator j % nu), z n x d."""
    m = np.asarray(nominal, dtype=np.float64).reshape(-1)
    b = np.asarray(ctrlrange, dtype=np.float64).reshape(-1, 2)
    lo, hi = np.resize(b[:, 0], m.size), np.resize(b[:, 1], m.size)
    step = np.float64(sigma) * (0.5 * (hi - lo))
    out = np.maximum(lo, np.minimum(hi, m + step * cma_lower_times(A, np.asarray(z, dtype=np.float64).reshape(-1, m.size))))
    out[0] = m
    return out


def cma_update(returns, nominal, z, state, params, ctrlrange):
    """The CMA-ES update of one environment in the device's order of operations -- the single statement of the arithmetic of
    mjpcx_cma_update_batched (include/mjpcx.h), next to sample_gradient_update. `returns` n, `nominal` the mean's d parameters, `z` the
    standard normals n x d of the candidates (row 0 is not read), `state` dict of sigma, C, A, p_sigma, p_c, generation, `params`
    cma_parameters' dict plus sigma_min, sigma_max, pivot_floor. The Cholesky form: p_sigma accumulates z_w = A^-1 (m' - m) / sigma
    where Hansen's tutorial has C^-1/2 (m' - m) / sigma.
    -> dict of order (the mu best of candidates 1..n-1: ascending, ties to the lower index, NaN last), index (the argmin over all n),
    best_return, nominal_return, improvement, valid, restarted, sigma, mean, z_w, y_w, y (mu x d), S, C_new (before a restart), h_sigma,
    state (the new one; the old one untouched when not valid)."""
    ret = np.asarray(returns, dtype=np.float64).reshape(-1)
    m = np.asarray(nominal, dtype=np.float64).reshape(-1)
    n, d, mu = ret.size, m.size, int(params["mu"])
    if not 1 <= mu <= n - 1:
        raise ValueError(f"mu = {mu} outside 1..{n - 1}")
    w = np.asarray(params["weights"], dtype=np.float64).reshape(-1)
    order = (np.lexsort((np.arange(1, n), ret[1:])) + 1)[:mu]
    index = int(np.lexsort((np.arange(n), ret))[0])
    gain = ret[0] - ret[index]
    sigma = np.float64(state["sigma"])
    out = dict(order=order, index=index, best_return=ret[index], nominal_return=ret[0], improvement=float(gain) if gain > 0 else 0.0,
               valid=int(not np.isnan(ret[order]).any()), restarted=0, sigma=float(sigma), mean=m.copy(), state=state)
    if not out["valid"]:
        return out
    A, C = np.asarray(state["A"], dtype=np.float64), np.asarray(state["C"], dtype=np.float64)
    cs, cc, c1, cmu = (np.float64(params[k]) for k in ("c_sigma", "c_c", "c_one", "c_mu"))
    mu_eff, chi = np.float64(params["mu_eff"]), np.float64(params["chi"])
    b = np.asarray(ctrlrange, dtype=np.float64).reshape(-1, 2)
    lo, hi = np.resize(b[:, 0], d), np.resize(b[:, 1], d)
    zs = np.asarray(z, dtype=np.float64).reshape(n, d)[order]
    y = cma_lower_times(A, zs)
    z_w = strided_tree_sum(w[:, None] * zs)
    y_w = cma_lower_times(A, z_w)
    mean = np.maximum(lo, np.minimum(hi, m + (sigma * (0.5 * (hi - lo))) * y_w))
    p_sigma = (1.0 - cs) * np.asarray(state["p_sigma"], dtype=np.float64) + np.sqrt((cs * (2.0 - cs)) * mu_eff) * z_w
    n2 = np.float64(0.0)
    for v in p_sigma:
        n2 = n2 + v * v
    norm = np.sqrt(n2)
    g = int(state["generation"]) + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        h_sigma = bool(norm / np.float64(math.sqrt(1.0 - math.pow(1.0 - float(cs), 2.0 * g))) < (1.4 + 2.0 / (d + 1.0)) * chi)
    hc = np.sqrt((cc * (2.0 - cc)) * mu_eff) if h_sigma else np.float64(0.0)
    p_c = (1.0 - cc) * np.asarray(state["p_c"], dtype=np.float64) + hc * y_w
    decay = (1.0 - c1) - cmu
    if not h_sigma:
        decay = decay + (c1 * cc) * (2.0 - cc)
    S = strided_tree_sum((w[:, None] * y)[:, :, None] * y[:, None, :])
    full = (decay * C + c1 * (p_c[:, None] * p_c[None, :])) + cmu * S
    C_new = np.tril(full) + np.tril(full, -1).T           # the entries a >= b, mirrored
    grown = sigma * np.exp((cs / np.float64(params["d_sigma"])) * ((norm / chi) - 1.0))
    sigma_new = float(min(max(grown, np.float64(params["sigma_min"])), np.float64(params["sigma_max"])))
    A_new = cma_factor(C_new, float(params["pivot_floor"]))
    new = dict(sigma=sigma_new, generation=g)
    if A_new is None:
        new.update(C=np.eye(d), A=np.eye(d), p_sigma=np.zeros(d), p_c=np.zeros(d))
    else:
        new.update(C=C_new, A=A_new, p_sigma=p_sigma, p_c=p_c)
    out.update(restarted=int(A_new is None), sigma=sigma_new, mean=mean, z_w=z_w, y_w=y_w, y=y, S=np.tril(S) + np.tril(S, -1).T, C_new=C_new,
               h_sigma=int(h_sigma), norm=float(norm), state=new)
    return out


class GpuBatchCMAESPlanner(GpuBatchSamplingPlanner):
    """CMA-ES (covariance matrix adaptation) for `num_envs` environments on ONE context, the search distribution on the device: where
    Predictive Sampling, Cross-Entropy and MPPI search with a diagonal distribution, this one learns the d x d covariance of the
    d = spline points x nu parameters -- actuators correlated across a gait, knots correlated in time -- and its own step size. A plan
    step is `generations` times: the host resample of every nominal (the mean), one `set_states`, one `rollout_cma_batched` (the
    candidates mean + sigma s A z are written on the device; candidate 0 is the mean), one `cma_update_batched` and ONE sync; the
    returned mean is the member's new policy and the next generation's nominal. Covariance, factor, paths and step size never leave
    the context. Member e plans exactly like GpuCMAESPlanner(seed = s + e), which is this class with one environment.

    The Cholesky form with positive weights and Hansen's default parameters (`cma_parameters`; lam = num_trajectory_ - 1, the mean is
    not ranked). Coordinates are normalised by the half control range, so `sigma0` is a fraction of it; None: the model's
    `sampling_exploration`. sigma stays within [sigma_min, sigma_max]. The state starts at sigma0, C = I and zero paths in `allocate`,
    `reset`, and whenever the number of spline points changes; it is NOT shifted in time between plan steps (Cross-Entropy's variance
    is not either). d is at most capi.CMA_MAX_PARAMS = 128 (the A1 with up to 10 spline points); the Humanoid's 336 are refused.
    Every return is needed, so there is no `pruning` here. A member whose mu best returns hold a NaN (`valid` 0) keeps its policy and
    its distribution. `best_trajectory(env)` is the rollout of the member's LOWEST-RETURN candidate (`winner`), not of the new mean,
    which was never rolled out. Per member after a plan: `sigma`, `best_return`, `nominal_return`, `improvement`, `restarted`, `valid`,
    `winner`."""
    pivot_floor = 1.0e-12     # a pivot of the factorisation must exceed this share of its diagonal entry, else C restarts at I

    def __init__(self, num_envs, device=0, precision=64, seed=0, sigma0=None, sigma_min=1.0e-6, sigma_max=2.0, generations=1,
                 backend_factory=None):
        super().__init__(num_envs, device, precision, seed, backend_factory)
        del self.pruning
        self.sigma0, self.sigma_min, self.sigma_max, self.generations = sigma0, float(sigma_min), float(sigma_max), int(generations)
        self._state_for = None    # (context, d) the context's CMA state was set for
        self._defaults = None     # ((d, n), cma_parameters(d, n - 1))
        for p in self.envs:
            p.sigma, p.restarted, p.valid = None, 0, 1

    def _reset_own(self):
        super()._reset_own()
        self._state_for = None

    def allocate(self):
        super().allocate()
        self._state_for = None

    def _sigma0(self):
        s = self.envs[0].noise_exploration[0] if self.sigma0 is None else self.sigma0
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        return np.full(self.num_envs, s[0]) if s.size == 1 else s

    def _enqueue(self, horizon, prune):
        n = self.num_trajectory_
        plans = [p.policy.plan for p in self.envs]
        d = plans[0].size() * self.model.nu
        if d > capi.CMA_MAX_PARAMS:
            raise ValueError(f"{type(self).__name__}: {d} parameters ({plans[0].size()} spline points x {self.model.nu} actuators); the dense "
                             f"covariance is kept for at most {capi.CMA_MAX_PARAMS}")
        self._push_states()
        if self._state_for is None or self._state_for[0] is not self.ctx or self._state_for[1] != d:
            self.ctx.cma_set_state_batched(self.num_envs, d, self._sigma0())
            self._state_for = (self.ctx, d)
        self._pruned = False
        self.ctx.rollout_cma_batched(n, horizon, plans[0].interpolation(), np.stack([pl.times() for pl in plans]),
                                     np.stack([pl.values() for pl in plans]), seed=self.seed, iteration=self.iteration, num_envs=self.num_envs)
        self._last = "plan"
        self._n = n

    def cma_params(self, d):
        """the update's constants for d parameters and the current candidate count (Hansen's defaults, computed once per shape)"""
        key = (d, self.num_trajectory_)
        if self._defaults is None or self._defaults[0] != key:
            self._defaults = (key, cma_parameters(d, self.num_trajectory_ - 1))
        return dict(self._defaults[1], sigma_min=self.sigma_min, sigma_max=self.sigma_max, pivot_floor=self.pivot_floor)

    def optimize_policy(self, horizon, pool=None):
        if self.generations < 1:
            raise ValueError(f"{type(self).__name__}: generations = {self.generations}; at least one")
        for _ in range(self.generations):
            t0 = self._launch(horizon)
            out = self.ctx.cma_update_batched(self.num_envs, self.cma_params(self._state_for[1]))
            # (a member that is not valid: its resampled nominal)
            values = [out["mean"][e] if out["valid"][e] else p.policy.plan.values() for e, p in enumerate(self.envs)]
            self._finish(t0, [([out["index"][e]], [out["best_return"][e]], 0, values[e]) for e in range(self.num_envs)])
            for e, p in enumerate(self.envs):
                p.best_return, p.nominal_return = float(out["best_return"][e]), float(out["nominal_return"][e])
                p.improvement = float(out["improvement"][e])
                p.sigma, p.restarted, p.valid = float(out["sigma"][e]), int(out["restarted"][e]), int(out["valid"][e])


class GpuCMAESPlanner:
    """CMA-ES for one robot: GpuBatchCMAESPlanner with ONE environment -- the same code, so a fleet's member e IS this planner with
    seed s + e. The candidate count must be a multiple of 64, the mean included. `best_trajectory()` is the lowest-return candidate's
    rollout."""
    winner, improvement, best_return, nominal_return = (_member_attr(k) for k in ("winner", "improvement", "best_return", "nominal_return"))
    sigma, restarted, valid = (_member_attr(k) for k in ("sigma", "restarted", "valid"))
    policy, previous_policy, noise_exploration = (_member_attr(k) for k in ("policy", "previous_policy", "noise_exploration"))
    iteration, ctx, model, task, num_trajectory_ = (_fleet_attr(k) for k in ("iteration", "ctx", "model", "task", "num_trajectory_"))
    sigma0, sigma_min, sigma_max, generations = (_fleet_attr(k) for k in ("sigma0", "sigma_min", "sigma_max", "generations"))

    def __init__(self, device=0, precision=64, seed=0, sigma0=None, sigma_min=1.0e-6, sigma_max=2.0, generations=1, backend_factory=None):
        self.fleet = GpuBatchCMAESPlanner(1, device, precision, seed, sigma0, sigma_min, sigma_max, generations, backend_factory)
        self.seed = seed

    def initialize(self, model, task: Task):
        self.fleet.initialize(model, task)

    def allocate(self):
        self.fleet.allocate()

    def reset(self, horizon, initial_repeated_action=None):
        self.fleet.reset(horizon, initial_repeated_action)

    def set_state(self, state: State):
        self.fleet.set_states([state])

    def optimize_policy(self, horizon, pool=None):
        self.fleet.optimize_policy(horizon, pool)

    def action_from_policy(self, action, state, time, use_previous=False):
        return self.fleet.action_from_policy(0, action, state, time, use_previous)

    def best_trajectory(self):
        return self.fleet.best_trajectory(0)

    def num_parameters(self):
        return self.fleet.num_parameters()


class GpuCrossEntropyPlanner(_ContextOwner):
    """mjpc::CrossEntropyPlanner (mjpc/planners/cross_entropy/planner.{h,cc}) with the candidate
    fan-out, the sort and the elite statistics on the GPU. Differences forced by SURVEY F4/F5 as for
    the sampling planner; the extra nominal rollout (planner.cc:435) rides along as one more candidate."""

    def __init__(self, device=0, precision=64, seed=0, group=None, backend_factory=None):
        self.device, self.precision, self.seed = device, precision, seed
        self.group = group
        self._backend_factory = backend_factory
        self.mtx_ = threading.RLock()
        self.iteration = 0
        self.improvement = 0.0
        self.noise_compute_time = self.rollouts_compute_time = self.policy_update_compute_time = 0.0
        self.trajectory_order = []
        self.interpolation_ = ZERO  # member default kZeroSpline, planner.h:141-142 (CE never reads sampling_representation)
        # optimize_policy reads nothing of a launch but its n_elite best candidates, their splines and the nominal rollout -- what a pruned launch
        # at rank n_elite + 1 keeps exact (set_prune_rank: the nominal completes and may sit among the first n_elite + 1). pruning: the plan
        # launch parks the candidates that the previous plan's worst elite return x (1 + park_slack) condemns and retires those above the
        # K-th completed return. Off by default, and off on a planner with a group (world > 1).
        self.pruning = False
        self.park_slack = DEFAULT_PARK_SLACK   # "cross_entropy_park_slack" in the model; <= -1: no hints
        self.prune_stats = self.park_stats = None   # of the last plan (capi.Context.prune_stats / park_stats); None unless it was pruned
        self.park_hint_used = None                  # the hint the last plan's launch ran on (+inf: none), None unless it was pruned
        self.pruned_launch_repeated = False         # the last plan's pruned launch was refused (MJPCX_ESTATE) and repeated unpruned
        self._hint = None                           # (previous worst elite return, task signature), or None -- no hint for the next plan

    # ---- Initialize, planner.cc:41-74
    def initialize(self, model, task: Task):
        self.model, self.task = model, task
        self.park_slack = float(model.get_number("cross_entropy_park_slack", DEFAULT_PARK_SLACK))
        self._hint = None
        self.std_initial_ = model.get_number("sampling_exploration", 0.1)
        self.std_min_ = model.get_number("std_min", 0.01)
        self.explore_fraction_ = model.get_number("explore_fraction", 0.0)
        self.num_trajectory_ = int(model.get_number("sampling_trajectories", 10))
        self.n_elite_ = int(model.get_number("n_elite", max(self.num_trajectory_ // 10, 2)))

    # ---- Allocate, planner.cc:77-119
    def allocate(self):
        m = self.model
        self.state = np.zeros(m.nq + m.nv + m.na)
        self.mocap = np.zeros(7 * m.nmocap)
        self.userdata = np.zeros(m.nuserdata)
        self.time = 0.0
        self.policy, self.resampled_policy, self.previous_policy = SamplingPolicy(), SamplingPolicy(), SamplingPolicy()
        for p in (self.policy, self.resampled_policy, self.previous_policy):
            p.allocate(m, self.task, K_MAX_TRAJECTORY_HORIZON)
        self.variance = np.zeros(m.nu * K_MAX_TRAJECTORY_HORIZON)
        self.times_scratch = np.zeros(K_MAX_TRAJECTORY_HORIZON)
        self.parameters_scratch = np.zeros(m.nu * K_MAX_TRAJECTORY_HORIZON)
        self._nominal = None
        self.ctx = self._create_context()

    # ---- Reset, planner.cc:122-160
    def reset(self, horizon, initial_repeated_action=None):
        self.state[:] = 0
        self.mocap[:] = 0
        self.userdata[:] = 0
        self.time = 0.0
        for p in (self.policy, self.resampled_policy, self.previous_policy):
            p.reset(horizon, initial_repeated_action)
        self.variance[:] = self.std_initial_ ** 2
        self.improvement = 0.0
        self._nominal = None
        self._hint = None

    def set_state(self, state: State):
        self.state, self.mocap, self.userdata, self.time = state.copy_to()

    def _rollouts(self, n_local, horizon, plan, ns, prune, rank):
        """the plan launch; prune: at rank `rank`, parked on the hint (the switches are sticky and the context may be shared: on for this
        launch alone). Returns whether the launch was asked to prune"""
        pruned = bool(prune) and cost_is_non_negative(self.task)
        self.park_hint_used = _park_hint(self._hint, self.task, self.park_slack) if pruned else None
        if pruned:
            self.ctx.set_pruning(False)
            self.ctx.set_prune_rank(rank)
            self.ctx.set_pruning(True)
            self.ctx.set_park_hint(self.park_hint_used)
        try:
            self.ctx.rollout_noise(n_local, horizon, plan.interpolation(), plan.times(), plan.values(), ns)
        finally:
            if pruned:
                self.ctx.set_pruning(False)
                self.ctx.set_park_hint(np.inf)
                self.ctx.set_prune_rank(1)
        return pruned

    # ---- ResamplePolicy, planner.cc:322-348
    def resample_policy(self, horizon):
        P = self.resampled_policy.num_spline_points
        nu = self.model.nu
        nominal_time = self.time
        time_shift = max((horizon - 1) * self._timestep() / (P - 1), 1.0e-5)
        for t in range(P):
            self.times_scratch[t] = nominal_time
            self.resampled_policy.action(self.parameters_scratch[t * nu:(t + 1) * nu], None, nominal_time)
            nominal_time += time_shift
        interp = self.policy.plan.interpolation()
        self.resampled_policy.plan.clear()
        for t in range(P):
            self.resampled_policy.plan.add_node(self.times_scratch[t], self.parameters_scratch[t * nu:(t + 1) * nu])
        self.resampled_policy.plan.set_interpolation(interp)

    # ---- OptimizePolicy, planner.cc:168-291
    def optimize_policy(self, horizon, pool=None):
        self.resampled_policy.plan.set_interpolation(self.interpolation_)
        num_trajectory = self.num_trajectory_
        self.n_elite_ = min(self.n_elite_, num_trajectory)
        n_elite = self.n_elite_
        with self.mtx_:
            self.resampled_policy.copy_from(self.policy, self.policy.num_spline_points)
        self.resample_policy(horizon)
        t0 = _time.perf_counter()
        P, nu = self.resampled_policy.num_spline_points, self.model.nu
        np_ = P * nu
        # ---- Rollouts, planner.cc:388-443: N noised candidates + the nominal as global candidate N
        rank, world = (self.group.rank, self.group.world) if self.group else (0, 1)
        if world > num_trajectory:
            raise ValueError("more ranks than candidates: every rank needs at least one rollout")
        q, r = divmod(num_trajectory, world)   # contiguous ranges, the first (N % world) ranks take one more
        n_local = q + (1 if rank < r else 0)
        offset = rank * q + min(rank, r)
        if rank == world - 1:
            n_local = num_trajectory - offset + 1          # the last rank also rolls out the nominal
        explore_count = int(np.sum(np.arange(num_trajectory) < num_trajectory * self.explore_fraction_))
        ns = capi.make_noise_spec(seed=self.seed, iteration=self.iteration, mode=capi.NOISE_CROSS_ENTROPY,
                                  candidate_offset=offset, nominal_candidate=num_trajectory, explore_count=explore_count,
                                  std0=self.std_initial_, std1=self.std_min_, param_variance=self.variance[:np_])
        plan = self.resampled_policy.plan
        sync_task(self.ctx, self.task)
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        pruned = self._rollouts(n_local, horizon, plan, ns, self.pruning and world == 1, n_elite + 1)
        self._offset, self._n_local = offset, n_local
        self.prune_stats = self.park_stats = None
        self.pruned_launch_repeated = False
        if pruned:
            self.prune_stats, self.park_stats = self.ctx.prune_stats(), self.ctx.park_stats()
        # ---- full sort in the reference (planner.cc:206-211); only the elites matter downstream
        k = min(n_elite + 1, n_local)
        try:
            idx, ret = self.ctx.topk(k)
        except capi.MjpcxError as err:
            if not pruned or err.code != MJPCX_ESTATE:
                raise
            # the pruned launch's ranking is not proven (a negative step cost): the same candidates again, all to the horizon
            self.pruned_launch_repeated = True
            self._rollouts(n_local, horizon, plan, ns, False, 1)
            idx, ret = self.ctx.topk(k)
        idx = idx.astype(np.int64) + offset
        if world > 1:
            idx, ret = self.group.merge_topk(idx, ret, n_elite + 1)
        keep = idx != num_trajectory                      # the nominal rollout is not a candidate
        idx, ret = idx[keep][:n_elite], ret[keep][:n_elite]
        self.trajectory_order = [int(i) for i in idx]
        self.rollouts_compute_time = (_time.perf_counter() - t0) * 1e6
        # ---- elite mean / variance, planner.cc:216-270
        t0 = _time.perf_counter()
        mine = np.array([i - offset for i in self.trajectory_order if offset <= i < offset + n_local and i != num_trajectory],
                        dtype=np.int32)
        s, sret = self.ctx.elite_moments(mine)
        if world > 1:
            tot = self.group.sum_array(np.concatenate([s.reshape(-1), [sret]]))
            s, sret = tot[:-1].reshape(P, nu), tot[-1]
        mean = s / n_elite
        avg_return = sret / n_elite
        sq, _ = self.ctx.elite_moments(mine, mean)
        if world > 1:
            sq = self.group.sum_array(sq.reshape(-1)).reshape(P, nu)
        self.variance[:] = 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            self.variance[:np_] = (sq / (n_elite - 1)).reshape(-1)   # n_elite == 1 -> inf/nan, as the reference
        self.parameters_scratch[:np_] = mean.reshape(-1)
        with self.mtx_:
            self.previous_policy.copy_from(self.policy)
            self.policy.plan.clear()
            self.policy.plan.set_interpolation(self.interpolation_)
            for t in range(P):
                self.policy.plan.add_node(self.times_scratch[t], mean[t])
        self.improvement = max(avg_return - float(ret[0]), 0.0)
        # the next plan's hint: this plan's worst elite return, unless its resume launch shows that the estimate it ran on was stale
        worst = float(ret[n_elite - 1]) if len(ret) >= n_elite else np.nan
        stale = pruned and float(self.park_stats["resumed"]) > K_PARK_MAX_RESUME_SHARE * max(n_local, 1)
        self._hint = (worst, task_signature(self.task)) if pruned and np.isfinite(worst) and worst >= 0 and not stale else None
        self._nominal = None
        self.iteration += 1
        self.policy_update_compute_time = (_time.perf_counter() - t0) * 1e6

    # ---- NominalTrajectory, planner.cc:294-308
    def nominal_trajectory(self, horizon, pool=None):
        plan = self.resampled_policy.plan
        sync_task(self.ctx, self.task)
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        self.ctx.rollout_splines(horizon, plan.interpolation(), plan.times(), plan.values()[None])
        self._nominal = self.ctx.fetch_trajectory(0)
        self._n_local = 0
        return self._nominal

    def action_from_policy(self, action, state, time, use_previous=False):
        with self.mtx_:
            return (self.previous_policy if use_previous else self.policy).action(action, state, time)

    # ---- BestTrajectory, planner.cc:446-448: the NOMINAL trajectory
    def best_trajectory(self):
        if self._nominal is None and self.ctx is not None and getattr(self, "_n_local", 0) > 0:
            local = self.num_trajectory_ - self._offset
            if 0 <= local < self._n_local:
                self._nominal = self.ctx.fetch_trajectory(local)
        return self._nominal

    def num_parameters(self):
        return self.policy.num_spline_points * self.model.nu


class GpuBatchCrossEntropyPlanner(_Fleet):
    """Cross-Entropy for `num_envs` environments (robots) on ONE context: every plan step is one `set_states`, one
    `rollout_noise_batched_ce` over all E x (n + 1) candidates with a variance row per environment, one `ce_update_batched`
    (selection of the elites, their mean, variance and mean return, on the device) and one sync -- instead of E plan steps of
    four host round trips each. The environments share the model, the task (unless `set_tasks` gives each its own) and n_elite_,
    std_initial_, std_min_, explore_fraction_; each has its own state, clock, mocap pose, policy and variance. Environment e with seed s behaves exactly
    like a GpuCrossEntropyPlanner with seed s + e: the per-environment logic (ResamplePolicy, policy copy, ActionFromPolicy) IS
    that planner's, one member per environment. The nominal rollout rides along as each environment's last candidate, so
    num_trajectory_ + 1 must be a positive multiple of 64."""

    def __init__(self, num_envs, device=0, precision=64, seed=0, backend_factory=None):
        super().__init__(num_envs, device, precision, backend_factory)
        self.seed = seed
        self.iteration = 0
        self.rollouts_compute_time = self.policy_update_compute_time = 0.0
        # the members never roll out themselves: they are handed the shared context instead of creating their own
        self.envs = [GpuCrossEntropyPlanner(device, precision, seed + e, backend_factory=lambda task: self.ctx) for e in range(self.num_envs)]
        # pruning: the plan launch runs at rank n_elite + 1 with a bound per robot (set_prune_rank + set_pruning_batched): it parks, per robot,
        # the candidates that the robot's previous worst elite return x (1 + park_slack) condemns and retires those above the robot's K-th
        # completed return. ce_update_batched reads the n_elite best without the nominal: what such a launch keeps exact. Off by default.
        self.pruning = False
        self.park_slack = DEFAULT_PARK_SLACK   # "cross_entropy_park_slack" in the model; <= -1: no hints
        self.prune_stats = self.park_stats = None   # of the last plan, per robot (capi.Context.prune_stats_batched); None unless it was pruned
        self.park_hints_used = None                 # the hints the last plan's launch ran on (E; +inf: none), None unless it was pruned
        self.pruned_launch_repeated = False         # the last plan's pruned launch was refused (MJPCX_ESTATE) and repeated unpruned
        self._hint = [None] * self.num_envs         # per robot: (previous worst elite return, task signature), or None

    def initialize(self, model, task: Task):
        super().initialize(model, task)
        self.park_slack = float(model.get_number("cross_entropy_park_slack", DEFAULT_PARK_SLACK))
        self._hint = [None] * self.num_envs

    num_trajectory_ = _fleet_setting("num_trajectory_")
    n_elite_ = _fleet_setting("n_elite_")
    std_initial_ = _fleet_setting("std_initial_")
    std_min_ = _fleet_setting("std_min_")
    explore_fraction_ = _fleet_setting("explore_fraction_")
    _n_advice = ("with the nominal rollout every environment launches num_trajectory_ + 1 candidates: set sampling_trajectories / "
                 "num_trajectory_ to 63, 127, ..., 2047, ...")

    def _reset_own(self):
        self._last = None
        self._hint = [None] * self.num_envs

    def _enqueue(self, n, horizon, ns, prune, rank):
        """the plan launch, with the members' resampled policies and variances as they stand: optimize_policy repeats it unpruned, same
        seed and iteration, when the context refuses the pruned one's ranking. Returns whether the launch was asked to prune"""
        plans = [p.resampled_policy.plan for p in self.envs]
        np_ = self.envs[0].resampled_policy.num_spline_points * self.model.nu
        # (a cost that can be negative in any robot's task row: no pruning for the launch -- partial returns would be no lower bounds there)
        pruned = bool(prune) and all(cost_is_non_negative(p.task) for p in self.envs)
        self.park_hints_used = np.array([_park_hint(h, p.task, self.park_slack) for h, p in zip(self._hint, self.envs)]) if pruned else None
        if pruned:
            self.ctx.set_prune_rank(rank)
            self.ctx.set_pruning_batched(True, self.num_envs, None, self.park_hints_used)
        try:
            self.ctx.rollout_noise_batched_ce(n, horizon, plans[0].interpolation(), np.stack([pl.times() for pl in plans]),
                                              np.stack([pl.values() for pl in plans]), np.stack([p.variance[:np_] for p in self.envs]),
                                              ns, num_envs=self.num_envs)
        finally:
            if pruned:   # (the switches are sticky: on for this launch alone)
                self.ctx.set_pruning_batched(False)
                self.ctx.set_prune_rank(1)
        return pruned

    # ---- OptimizePolicy, cross_entropy/planner.cc:168-291, for every environment
    def optimize_policy(self, horizon, pool=None):
        num_trajectory = int(self.num_trajectory_)
        n = num_trajectory + 1                               # the nominal rollout is local candidate num_trajectory
        self._check_n(n)
        self.n_elite_ = min(self.n_elite_, num_trajectory)
        n_elite = self.n_elite_
        for p in self.envs:
            p.resampled_policy.plan.set_interpolation(p.interpolation_)
            with p.mtx_:
                p.resampled_policy.copy_from(p.policy, p.policy.num_spline_points)
            p.resample_policy(horizon)
        t0 = _time.perf_counter()
        first = self.envs[0]
        P, nu = first.resampled_policy.num_spline_points, self.model.nu
        np_ = P * nu
        explore_count = int(np.sum(np.arange(num_trajectory) < num_trajectory * self.explore_fraction_))
        ns = capi.make_noise_spec(seed=self.seed, iteration=self.iteration, mode=capi.NOISE_CROSS_ENTROPY, candidate_offset=0,
                                  nominal_candidate=num_trajectory, explore_count=explore_count, std0=self.std_initial_,
                                  std1=self.std_min_)
        self._push_states()
        pruned = self._enqueue(n, horizon, ns, self.pruning, n_elite + 1)
        self.prune_stats = self.park_stats = None
        self.pruned_launch_repeated = False
        if pruned:
            st = self.ctx.prune_stats_batched(self.num_envs)
            self.prune_stats = {k: st[k] for k in ("retired", "retire_step_sum", "negative_cost", "wavefronts_ended_early", "final_bound")}
            self.park_stats = {k: st[k] for k in ("parked", "settled_retired", "resumed")}
        try:
            idx, ret, mean, var, avg = self.ctx.ce_update_batched(self.num_envs, n_elite, num_trajectory)
        except capi.MjpcxError as err:
            if not pruned or err.code != MJPCX_ESTATE:
                raise
            # some robot's pruned ranking is not proven (a negative step cost): the same candidates again, all to the horizon
            self.pruned_launch_repeated = True
            self._enqueue(n, horizon, ns, False, 1)
            idx, ret, mean, var, avg = self.ctx.ce_update_batched(self.num_envs, n_elite, num_trajectory)
        self._last = "plan"
        self._n = n
        self.rollouts_compute_time = (_time.perf_counter() - t0) * 1e6
        self.iteration += 1
        # ---- the elites' mean becomes the policy, their variance the next step's noise (planner.cc:216-290)
        t0 = _time.perf_counter()
        for e, p in enumerate(self.envs):
            p._offset, p._n_local = 0, n
            p.trajectory_order = [int(i) for i in idx[e]]
            p.variance[:] = 0.0
            p.variance[:np_] = np.asarray(var[e]).reshape(-1)
            m = np.asarray(mean[e]).reshape(P, nu)
            p.parameters_scratch[:np_] = m.reshape(-1)
            with p.mtx_:
                p.previous_policy.copy_from(p.policy)
                p.policy.plan.clear()
                p.policy.plan.set_interpolation(p.interpolation_)
                for t in range(P):
                    p.policy.plan.add_node(p.times_scratch[t], m[t])
            p.improvement = max(float(avg[e]) - float(ret[e][0]), 0.0)
            p._nominal = None
            p.iteration = self.iteration
            # the next plan's hint: the robot's worst elite return, unless its resume launch shows that the estimate it ran on was stale
            worst = float(ret[e][n_elite - 1])
            stale = pruned and float(self.park_stats["resumed"][e]) > K_PARK_MAX_RESUME_SHARE * max(n, 1)
            self._hint[e] = (worst, task_signature(p.task)) if pruned and np.isfinite(worst) and worst >= 0 and not stale else None
        self.policy_update_compute_time = (_time.perf_counter() - t0) * 1e6

    def nominal_trajectory(self, horizon, pool=None):
        plans = [p.resampled_policy.plan for p in self.envs]
        if any(pl.size() != plans[0].size() for pl in plans):
            raise ValueError("the environments' policies have different numbers of spline nodes")
        out = self._nominal_launch(horizon, plans[0].interpolation(), np.stack([pl.times() for pl in plans]), [pl.values() for pl in plans])
        for p, tr in zip(self.envs, out):
            p._nominal = tr
            p._n_local = 0
        return out

    # ---- BestTrajectory, planner.cc:446-448: the NOMINAL rollout, the environment's last candidate
    def best_trajectory(self, env):
        p = self.envs[env]
        if p._nominal is None:
            p._nominal = self._fetch_planned(env, self._n - 1)
        return p._nominal


# ====================================================================================== iLQG
def log_scale(max_value, min_value, steps):
    """LogScale, mjpc/utilities.cc:819-826 (ascending from min_value to max_value)."""
    step = (np.log(max_value) - np.log(min_value)) / max(steps - 1, 1)
    return np.exp(np.log(min_value) + np.arange(steps) * step)


def find_interval(xs, value, length):
    """FindInterval, mjpc/utilities.h:124-144."""
    up = int(np.searchsorted(np.asarray(xs[:length]), value, side="right"))
    lo = up - 1
    if lo < 0:
        return 0, 0
    if lo > length - 1:
        return length - 1, length - 1
    return lo, min(up, length - 1)


def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def state_diff(model, s1, s2, h=1.0):
    """StateDiff, mjpc/utilities.cc:543-553: (s2 - s1) / h in the tangent space (mj_differentiatePos + velocities)."""
    nq, nv = model.nq, model.nv
    if nq == nv:
        return (np.asarray(s2, float) - np.asarray(s1, float)) / h
    a = model.arrays
    dx = np.zeros(2 * nv)
    for j in range(model.njnt):
        qa, da, t = int(a["jnt_qposadr"][j]), int(a["jnt_dofadr"][j]), int(a["jnt_type"][j])
        if t == 0:  # free
            dx[da:da + 3] = (s2[qa:qa + 3] - s1[qa:qa + 3]) / h
            qa, da = qa + 3, da + 3
        if t in (0, 1):  # free / ball: mju_subQuat
            qb, qa_ = np.asarray(s1[qa:qa + 4], float), np.asarray(s2[qa:qa + 4], float)
            qd = _quat_mul(np.array([qb[0], -qb[1], -qb[2], -qb[3]]), qa_)
            ax = qd[1:].copy()
            sn = np.linalg.norm(ax)
            if sn > 1e-15:
                ax /= sn
            speed = 2 * np.arctan2(sn, qd[0])
            if speed > np.pi:
                speed -= 2 * np.pi
            dx[da:da + 3] = ax * speed / h
        else:
            dx[da] = (s2[qa] - s1[qa]) / h
    dx[nv:] = (np.asarray(s2[nq:], float) - np.asarray(s1[nq:], float)) / h
    return dx


def normalize_state_quaternions(model, x):
    """mj_normalizeQuat on an interpolated state (ilqg/policy.cc:118-125)."""
    a = model.arrays
    for j in range(model.njnt):
        t = int(a["jnt_type"][j])
        if t in (0, 1):
            qa = int(a["jnt_qposadr"][j]) + (3 if t == 0 else 0)
            n = np.linalg.norm(x[qa:qa + 4])
            x[qa:qa + 4] = [1, 0, 0, 0] if n < 1e-15 else x[qa:qa + 4] / n
    return x


def model_derivatives(ctx, tr, T, derivative_skip, fd_tolerance, fd_mode):
    """ModelDerivatives::Compute incl. skip + interpolation, model_derivatives.cc:45-165 (the gradient-based planners' shared
    step; the caller zeroes A, B, D at the last step, which has no transition)"""
    evaluate = derivative_steps(T, derivative_skip)
    A, B, C, D = ctx.transition_fd(tr.times[evaluate], tr.states[evaluate], tr.actions[evaluate], fd_tolerance, int(fd_mode))
    if len(evaluate) == T:
        return A, B, C, D
    full = [np.zeros((T,) + x.shape[1:]) for x in (A, B, C, D)]
    ev = np.array(evaluate)
    for t in range(T):
        k = int(np.searchsorted(ev, t, side="right")) - 1
        e0 = k
        e1 = min(k + 1, len(ev) - 1)
        tt = 0.0 if (ev[e0] == t or e0 == e1) else (t - ev[e0]) / (ev[e1] - ev[e0])
        for f, x in zip(full, (A, B, C, D)):
            f[t] = x[e0] * (1.0 - tt) + x[e1] * tt
    return full


class ILQGSettings:
    """iLQGSettings, mjpc/planners/ilqg/settings.h."""
    min_linesearch_step = 1.0e-3
    fd_tolerance = 1.0e-6
    fd_mode = 0
    min_regularization = 1.0e-6
    max_regularization = 1.0e6
    regularization_type = 0
    max_regularization_iterations = 5
    action_limits = 1
    nominal_feedback_scaling = 1
    verbose = 0


class ILQGPolicy:
    """iLQGPolicy, mjpc/planners/ilqg/policy.{h,cc}: a nominal trajectory + time-varying linear feedback."""

    def __init__(self, model, task, horizon_cap=K_MAX_TRAJECTORY_HORIZON):
        self.model = model
        nu, ds, ndx = model.nu, model.nq + model.nv + model.na, 2 * model.nv + model.na
        self.trajectory = capi.Trajectory(ds, nu, task.num_residual, task.num_trace, horizon_cap)
        self.feedback_gain = np.zeros((horizon_cap, nu, ndx))
        self.action_improvement = np.zeros((horizon_cap, nu))
        self.feedback_scaling = 1.0
        self.representation = int(model.get_number("ilqg_representation", 1))

    def reset(self, horizon, initial_repeated_action=None):
        tr = self.trajectory
        for a in (tr.states, tr.times, tr.residual, tr.costs, tr.trace):
            a[...] = 0
        tr.actions[...] = 0 if initial_repeated_action is None else np.asarray(initial_repeated_action)
        tr.total_return, tr.failure = 0.0, False
        self.feedback_gain[:horizon] = 0
        self.action_improvement[:horizon] = 0
        self.feedback_scaling = 1.0

    def copy_from(self, other, horizon):
        import copy
        self.trajectory = copy.deepcopy(other.trajectory)
        self.feedback_gain[:horizon] = other.feedback_gain[:horizon]
        self.action_improvement[:horizon] = other.action_improvement[:horizon]

    @staticmethod
    def _slope(g, xs, ys, length):
        """FiniteDifferenceSlope (utilities.cc:362-395) at grid point g"""
        if g == length - 1:
            return (ys[g] - ys[g - 1]) / (xs[g] - xs[g - 1]) if length > 2 else np.zeros_like(ys[g])
        if g == 0:
            return (ys[1] - ys[0]) / (xs[1] - xs[0])
        return 0.5 * (ys[g + 1] - ys[g]) / (xs[g + 1] - xs[g]) + 0.5 * (ys[g] - ys[g - 1]) / (xs[g] - xs[g - 1])

    @classmethod
    def _interp(cls, x, xs, ys, length, zero, representation=1):
        b0, b1 = find_interval(xs, x, length)
        if zero or b0 == b1:
            return ys[b0].copy()
        span = xs[b1] - xs[b0]
        t = (x - xs[b0]) / span
        if representation != 2:
            return ys[b0] * (1.0 - t) + ys[b1] * t
        c0, c1 = 2.0 * t ** 3 - 3.0 * t * t + 1.0, (t ** 3 - 2.0 * t * t + t) * span
        c2, c3 = -2.0 * t ** 3 + 3 * t * t, (t ** 3 - t * t) * span
        return c0 * ys[b0] + c1 * cls._slope(b0, xs, ys, length) + c2 * ys[b1] + c3 * cls._slope(b1, xs, ys, length)

    def action(self, action, state, time):
        """policy.cc:82-161 (zero-order / linear / cubic representations)."""
        tr, H = self.trajectory, self.trajectory.horizon
        b0, b1 = find_interval(tr.times, time, H)
        zero = b0 == b1 or self.representation == 0
        rep = self.representation
        action[:] = self._interp(time, tr.times, tr.actions, H - 1, zero, rep)
        if state is not None:
            xi = self._interp(time, tr.times, tr.states, H, zero, rep)
            if self.model.nq != self.model.nv:
                xi = normalize_state_quaternions(self.model, xi)
            K = self._interp(time, tr.times, self.feedback_gain, H - 1, zero, rep)
            action += self.feedback_scaling * (K @ state_diff(self.model, xi, np.asarray(state, float)))
        return clamp(action, self.model.actuator_ctrlrange)


class GpuILQGPlanner(_ContextOwner):
    """mjpc::iLQGPlanner (mjpc/planners/ilqg/planner.{h,cc}) with every data-parallel piece on the GPU:
    feedback / line-search rollouts (mjpcx_rollout_feedback), finite-difference model derivatives
    (mjpcx_transition_fd), cost derivatives (mjpcx_cost_derivatives) and the Riccati sweep on the matrix
    cores (mjpcx_backward_pass). Host side: the regularisation schedule, BestRollout, policy bookkeeping."""

    def __init__(self, device=0, precision=64, backend_factory=None):
        self.device, self.precision = device, precision
        self._backend_factory = backend_factory
        self.settings = ILQGSettings()
        self.mtx_ = threading.RLock()
        self.first_candidate = 0    # this planner's first candidate in the context's rollout (a member of GpuBatchILQGPlanner: env * n)

    def initialize(self, model, task: Task):
        self.model, self.task = model, task
        self.dim_state = model.nq + model.nv + model.na
        self.dim_state_derivative = 2 * model.nv + model.na
        self.dim_action = model.nu
        self.num_rollouts_gui_ = int(model.get_number("ilqg_num_rollouts", 10))
        self.settings.regularization_type = int(model.get_number("ilqg_regularization_type", self.settings.regularization_type))
        self.num_trajectory_ = self.num_rollouts_gui_

    def allocate(self):
        m = self.model
        self.state = np.zeros(self.dim_state)
        self.mocap = np.zeros(7 * m.nmocap)
        self.userdata = np.zeros(m.nuserdata)
        self.time = 0.0
        self.policy = ILQGPolicy(m, self.task)
        self.previous_policy = ILQGPolicy(m, self.task)
        self.candidate0 = ILQGPolicy(m, self.task)          # candidate_policy[0]
        self.differentiable_ = _agent_differentiable(m)
        self.ctx = self._create_context(self.differentiable_)

    def reset(self, horizon, initial_repeated_action=None):
        self.state[:] = 0; self.mocap[:] = 0; self.userdata[:] = 0
        self.time = 0.0
        for p in (self.policy, self.previous_policy, self.candidate0):
            p.reset(horizon, initial_repeated_action)
        # iLQGBackwardPass::Reset, backward_pass.cc:50-62
        self.regularization, self.regularization_rate, self.regularization_factor = 1.0, 1.0, 2.0
        self.dV = np.zeros(2)
        self.action_step = self.feedback_scaling = self.improvement = self.expected = self.surprise = 0.0
        self.derivative_skip_ = int(self.model.get_number("derivative_skip", 0))
        self.winner = 0
        self.nominal_index = -1
        # the last iteration's trajectory[winner] / trajectory[0] returns, and whether it reached the policy update
        self.winner_return = self.linesearch0_return = 0.0
        self.iteration_completed = False
        self.timers = {}

    def set_state(self, state: State):
        self.state, self.mocap, self.userdata, self.time = state.copy_to()

    # ---- backward_pass.cc:327-356
    def scale_regularization(self, factor, reg_min, reg_max):
        if factor > 1:
            self.regularization_rate = max(self.regularization_rate * factor, factor)
        else:
            self.regularization_rate = min(self.regularization_rate * factor, factor)
        self.regularization = min(max(self.regularization * self.regularization_rate, reg_min), reg_max)

    def update_regularization(self, reg_min, reg_max, z, s):
        bad = lambda v: not np.isfinite(v) or abs(v) > 1e10
        f = self.regularization_factor
        if bad(z) or bad(s):
            self.scale_regularization(f * f, reg_min, reg_max)
        elif z > 0.5 or s > 0.3:
            self.scale_regularization(1.0 / f, reg_min, reg_max)
        elif z < 0.1 or s < 0.06:
            self.scale_regularization(f, reg_min, reg_max)

    def _linesearch_steps(self):
        n = self.num_trajectory_
        steps = np.zeros(n)
        steps[:n - 1] = log_scale(1.0, self.settings.min_linesearch_step, n - 1)
        steps[n - 1] = 0.0
        return steps

    @staticmethod
    def best_rollout(returns, failure):
        """iLQGPlanner::BestRollout, planner.cc:727-740 (scan from the last index, strict <)."""
        best, best_return = -1, 0.0
        for j in range(len(returns) - 1, -1, -1):
            if failure[j]:
                continue
            if best == -1 or returns[j] < best_return:
                best, best_return = j, returns[j]
        return best

    # ---- OptimizePolicy, planner.cc:156-164
    def optimize_policy(self, horizon, pool=None):
        self.num_trajectory_ = self.num_rollouts_gui_       # the reference clamps to kMaxTrajectory = 128 (lifted)
        self.nominal_trajectory(horizon)
        self.iteration(horizon)

    # ---- NominalTrajectory, planner.cc:167-223 + FeedbackRollouts :695-724
    def nominal_trajectory(self, horizon, pool=None):
        if self.num_trajectory_ == 0:
            return
        t0 = _time.perf_counter()
        request = self._nominal_request(horizon)
        sync_task(self.ctx, self.task)
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        self.ctx.rollout_feedback(horizon, 1, self.policy.representation, self.settings.nominal_feedback_scaling, *request)
        ret, fail = self.ctx.returns()
        self._nominal_select(horizon, ret, fail)
        self.timers["nominal"] = (_time.perf_counter() - t0) * 1e6

    # The two rollout phases of a plan step, each split at its launch, so that GpuBatchILQGPlanner can put the launches of a whole fleet
    # into one batched call and run this planner's own code on either side: *_request gives the arrays of the feedback rollouts
    # (times, states, actions, gains, improvement, alpha), the other half takes this planner's returns of them.
    def _nominal_request(self, horizon):
        self.policy.trajectory.horizon = horizon
        tr = self.policy.trajectory
        return (tr.times[:horizon], tr.states[:horizon], tr.actions[:horizon], self.policy.feedback_gain[:horizon],
                self.policy.action_improvement[:horizon], self._linesearch_steps())

    def _nominal_select(self, horizon, ret, fail):
        steps = self._linesearch_steps()
        best = self.best_rollout(ret, fail)
        self.nominal_index = best                           # this planner's winning nominal rollout; -1: every one failed
        if best == -1:
            import copy
            self.candidate0.trajectory = copy.deepcopy(self.policy.trajectory)
            self.feedback_scaling = 0.0
        else:
            self._take_trajectory(self.candidate0, best, horizon)
            self.feedback_scaling = steps[best]
        self.candidate0.feedback_gain[:horizon] = self.policy.feedback_gain[:horizon]
        self.candidate0.action_improvement[:horizon] = self.policy.action_improvement[:horizon]
        self.candidate0.representation = self.policy.representation

    def _take_trajectory(self, policy, index, horizon):
        """candidate_policy[0].trajectory = trajectory[index] (buffers keep their allocated capacity)."""
        got = self.ctx.fetch_trajectory(self.first_candidate + index)
        tr = policy.trajectory
        for name in ("states", "actions", "times", "residual", "costs", "trace"):
            getattr(tr, name)[:horizon] = getattr(got, name)
        tr.horizon, tr.total_return, tr.failure = horizon, got.total_return, got.failure

    def _model_derivatives(self, tr, T):
        return model_derivatives(self.ctx, tr, T, self.derivative_skip_, self.settings.fd_tolerance, self.settings.fd_mode)

    # ---- Iteration, planner.cc:377-627
    def iteration(self, horizon, pool=None):
        request = self._iteration_before_rollouts(horizon)
        if request is None:
            return
        # ---- ActionRollouts, planner.cc:630-692: line search over the improvement step
        t0 = _time.perf_counter()
        sync_task(self.ctx, self.task)
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        self.ctx.rollout_feedback(horizon, 0, 0, 1, *request)
        ret, fail = self.ctx.returns()
        if self._iteration_after_rollouts(horizon, ret, fail):
            self.timers["rollouts"] = (_time.perf_counter() - t0) * 1e6

    def _iteration_before_rollouts(self, horizon):
        """derivatives and the backward pass on the context's current state; the line search's request, or None when the backward
        pass failed every retry (the iteration ends there)"""
        st = self.settings
        c0 = self.candidate0
        tr = c0.trajectory
        T = horizon
        self._previous_return = tr.total_return
        self.iteration_completed = False
        t0 = _time.perf_counter()
        A, B, C, D = self._model_derivatives(tr, T)
        # the last step has no transition (model_derivatives.cc:88-92 computes only C there)
        A[T - 1] = 0; B[T - 1] = 0; D[T - 1] = 0
        self.timers["model_derivative"] = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        cx, cu, cxx, cxu, cuu = self.ctx.cost_derivatives(tr.residual[:T], C, D)
        self.timers["cost_derivative"] = (_time.perf_counter() - t0) * 1e6
        # ---- backward pass with regularisation retries, planner.cc:429-520
        t0 = _time.perf_counter()
        ok, reg_iter = False, 0
        limits = np.asarray(self.model.actuator_ctrlrange, float).reshape(-1, 2)
        while reg_iter < st.max_regularization_iterations and not ok:
            out = self.ctx.backward_pass(self.regularization, st.regularization_type, st.action_limits, A, B, cx, cu, cxx,
                                         cxu, cuu, tr.actions[:T], limits)
            ok = out["ok"]
            if not ok and self.regularization <= st.max_regularization:
                self.scale_regularization(self.regularization_factor, st.min_regularization, st.max_regularization)
                reg_iter += 1
            elif not ok:
                break
        self.timers["backward_pass"] = (_time.perf_counter() - t0) * 1e6
        if not ok:
            return None
        self.dV = out["dV"]
        c0.feedback_gain[:T] = out["K"]
        c0.action_improvement[:T] = out["du"]
        return (tr.times[:T], tr.states[:T], tr.actions[:T], c0.feedback_gain[:T], c0.action_improvement[:T], self._linesearch_steps())

    def _iteration_after_rollouts(self, horizon, ret, fail):
        """selection, regularisation update and policy update from the line search's returns; False when every rollout failed"""
        st = self.settings
        c0 = self.candidate0
        tr = c0.trajectory
        T = horizon
        steps = self._linesearch_steps()
        previous_return = self._previous_return
        self.linesearch0_return = float(ret[0])
        best = self.best_rollout(ret, fail)
        if best == -1:
            return False
        self.winner = best
        self.winner_return = float(ret[best])
        # candidate_policy[winner]: the nominal trajectory with actions += step * improvement (NOT re-rolled)
        import copy
        winner_policy = ILQGPolicy.__new__(ILQGPolicy)
        winner_policy.__dict__ = dict(c0.__dict__)
        winner_policy.trajectory = copy.deepcopy(c0.trajectory)
        winner_policy.trajectory.actions[:T] = tr.actions[:T] + steps[best] * c0.action_improvement[:T]
        self._take_trajectory(c0, best, T)
        if best == 0:
            winner_policy.trajectory = copy.deepcopy(c0.trajectory)
        self.action_step = steps[best]
        self.expected = -1.0 * self.action_step * (self.dV[0] + self.action_step * self.dV[1]) + 1.0e-16
        self.improvement = previous_return - float(ret[best])
        self.surprise = min(max(0.0, self.improvement / self.expected), 2.0)
        self.update_regularization(st.min_regularization, st.max_regularization, self.surprise, self.action_step)
        with self.mtx_:
            self.previous_policy.copy_from(self.policy, T)
            self.previous_policy.feedback_scaling = self.policy.feedback_scaling
            self.policy.copy_from(winner_policy, T)
            self.policy.feedback_scaling = 1.0
        self.iteration_completed = True
        return True

    def action_from_policy(self, action, state, time, use_previous=False):
        with self.mtx_:
            return (self.previous_policy if use_previous else self.policy).action(action, state, time)

    def best_trajectory(self):
        with self.mtx_:
            return self.policy.trajectory

    def num_parameters(self):
        return self.dim_action * K_MAX_TRAJECTORY_HORIZON


class GpuBatchILQGPlanner(_Fleet):
    """iLQG for `num_envs` environments (robots) on ONE context. The two feedback-rollout phases of a plan step -- the nominal
    under iLQGPolicy::Action and the line search under the index policy, three quarters of an iteration and pure per-step latency --
    are one `rollout_feedback_batched` launch each for the whole fleet (any number of rollouts per environment: iLQG's ten). Between
    them the derivative chain and the backward pass with its regularisation retries run for the whole fleet in ONE call,
    `ilqg_step_batched`, on the nominal rollouts still on the device (`device_chain`: None = whenever the context has that call, False
    = never). Without it -- the oracle backends of the tests, or an environment whose nominal rollouts all failed, whose nominal is then
    the host's policy trajectory and no device rollout -- an environment runs the unchanged sequential chain on the shared context:
    plain `set_state` of that environment, model derivatives, cost derivatives, the backward pass with its retries. An environment
    whose backward pass fails every retry sits the line search out, exactly as GpuILQGPlanner.iteration returns early. The environments
    share the model, the task (unless `set_tasks` gives each its own; a member's sequential chain then runs on its own task) and the
    settings; each has its own state, clock, mocap pose, policy and regularisation. The
    per-environment logic (BestRollout, the regularisation schedule, the policy bookkeeping) IS GpuILQGPlanner's, one member per
    environment.
    timers: `derivatives_backward` is the whole middle either way. On the sequential path `model_derivative`, `cost_derivative` and
    `backward_pass` are the members' sums; with the device chain the stages are one call, whose total is under `model_derivative`, the
    other two are 0 (plus whatever a member that fell back to the sequential chain spent)."""

    def __init__(self, num_envs, device=0, precision=64, backend_factory=None):
        super().__init__(num_envs, device, precision, backend_factory)
        self.timers = {}
        self.device_chain = None    # None: ilqg_step_batched whenever the context has it; False: the sequential middle (the tests' comparison)
        self.used_device_chain = False   # which middle the last optimize_policy ran
        # the members never create a context of their own: they are handed the shared one
        self.envs = [GpuILQGPlanner(device, precision, backend_factory=lambda task: self.ctx) for _ in range(self.num_envs)]
        for p in self.envs:
            p.settings = self.envs[0].settings      # one ILQGSettings for the fleet

    derivative_chain = True
    num_rollouts_gui_ = _fleet_setting("num_rollouts_gui_")
    derivative_skip_ = _fleet_setting("derivative_skip_")
    settings = _fleet_setting("settings")

    def _reset_own(self):
        self.timers = {}

    def _rollout(self, horizon, mode, representation, use_state, requests):
        """one batched launch of every environment's request; each member's share of the returns"""
        n = len(requests[0][5])
        self._push_states()
        self.ctx.rollout_feedback_batched(horizon, mode, representation, use_state, *[np.stack([r[k] for r in requests]) for k in range(6)])
        ret, fail = self.ctx.returns()
        for e, p in enumerate(self.envs):
            p.first_candidate = e * n
        return [(ret[e * n:(e + 1) * n], fail[e * n:(e + 1) * n]) for e in range(self.num_envs)]

    def _prepare(self):
        n = int(self.num_rollouts_gui_)
        if n < 1:
            raise ValueError("GpuBatchILQGPlanner: ilqg_num_rollouts / num_rollouts_gui_ must be >= 1")
        if any(p.policy.representation != self.envs[0].policy.representation for p in self.envs):
            raise ValueError("the environments' policies have different representations")
        for p in self.envs:
            p.num_trajectory_ = n

    # ---- NominalTrajectory of every environment: one launch
    def nominal_trajectory(self, horizon, pool=None):
        self._prepare()
        t0 = _time.perf_counter()
        first = self.envs[0]
        shares = self._rollout(horizon, 1, first.policy.representation, first.settings.nominal_feedback_scaling,
                               [p._nominal_request(horizon) for p in self.envs])
        for p, (ret, fail) in zip(self.envs, shares):
            p._nominal_select(horizon, ret, fail)
        self.timers["nominal"] = (_time.perf_counter() - t0) * 1e6

    def _use_device_chain(self):
        st = self.settings
        if self.device_chain is not None and not self.device_chain:
            return False
        if not hasattr(self.ctx, "ilqg_step_batched"):
            if self.device_chain:
                raise ValueError("GpuBatchILQGPlanner: device_chain on a context without ilqg_step_batched")
            return False
        # what the call would refuse keeps the sequential middle: no retries at all (the iteration ends before the backward pass), members
        # with different factors, a regularisation, rate or factor that is not a positive finite number
        ok = lambda v: np.isfinite(v) and v > 0
        return (1 <= st.max_regularization_iterations <= 64 and len({p.regularization_factor for p in self.envs}) == 1 and
                all(ok(p.regularization) and ok(p.regularization_rate) and ok(p.regularization_factor) for p in self.envs) and
                np.isfinite(st.min_regularization) and np.isfinite(st.max_regularization) and st.min_regularization <= st.max_regularization)

    def _sequential_middle(self, p, horizon):
        if self._tasks is not None:     # the plain calls of this chain read the context's plain values: the member's own task. (The plain
            sync_task(self.ctx, p.task)  # residual state replaces the fleet's per-environment one; the next _push_states brings it back.)
        self.ctx.set_state(p.state, p.time, p.mocap, p.userdata)
        return p._iteration_before_rollouts(horizon)

    def _step_args(self, T):
        """what ilqg_step_batched takes after the candidates: the steps, the settings and every member's regularisation"""
        st = self.settings
        return (T, derivative_steps(T, self.derivative_skip_), st.fd_tolerance, int(st.fd_mode), st.regularization_type, st.action_limits,
                [p.regularization for p in self.envs], [p.regularization_rate for p in self.envs], self.envs[0].regularization_factor,
                st.min_regularization, st.max_regularization, st.max_regularization_iterations)

    def _device_middle(self, horizon):
        """GpuILQGPlanner._iteration_before_rollouts of every member from ONE ilqg_step_batched; the line search's requests"""
        t0 = _time.perf_counter()
        out = self.ctx.ilqg_step_batched([p.nominal_index for p in self.envs], *self._step_args(horizon))
        requests = self._scatter_step(out, horizon)
        call_us = (_time.perf_counter() - t0) * 1e6
        for e, p in enumerate(self.envs):
            if out["status"][e] < 0:
                requests[e] = self._sequential_middle(p, horizon)
        return requests, call_us

    def _scatter_step(self, out, T):
        """the results of one ilqg_step_batched[_from] into the members; per member the line search's request, None for one that took
        no part (status -1: untouched) or whose backward pass failed every retry (status 0)"""
        requests = []
        for e, p in enumerate(self.envs):
            status = int(out["status"][e])
            if status < 0:
                requests.append(None)               # its nominal is not on the device: the sequential chain, below
                continue
            c0 = p.candidate0
            tr = c0.trajectory
            p._previous_return = tr.total_return
            p.iteration_completed = False
            p.regularization, p.regularization_rate = float(out["mu"][e]), float(out["rate"][e])
            p.timers.update(model_derivative=0.0, cost_derivative=0.0, backward_pass=0.0)
            if status == 0:
                requests.append(None)
                continue
            p.dV = out["dV"][e].copy()
            c0.feedback_gain[:T] = out["K"][e]
            c0.action_improvement[:T] = out["du"][e]
            requests.append((tr.times[:T], tr.states[:T], tr.actions[:T], c0.feedback_gain[:T], c0.action_improvement[:T], p._linesearch_steps()))
        return requests

    # ---- OptimizePolicy, ilqg/planner.cc:156-164, for every environment
    def optimize_policy(self, horizon, pool=None):
        self.nominal_trajectory(horizon)
        # ---- derivatives and the backward pass: one call for the fleet, or one environment after the other on its plain state
        t0 = _time.perf_counter()
        self.used_device_chain = self._use_device_chain()
        if self.used_device_chain:
            requests, call_us = self._device_middle(horizon)
        else:
            requests, call_us = [self._sequential_middle(p, horizon) for p in self.envs], 0.0
        self.timers["derivatives_backward"] = (_time.perf_counter() - t0) * 1e6
        for key in ("model_derivative", "cost_derivative", "backward_pass"):
            self.timers[key] = sum(p.timers[key] for p in self.envs) + (call_us if key == "model_derivative" else 0.0)
        # ---- ActionRollouts of the environments that got that far: one launch. The others ride along on their nominal with zero
        # steps and are ignored.
        self.sat_out = [r is None for r in requests]
        if all(self.sat_out):
            return
        t0 = _time.perf_counter()
        for e, p in enumerate(self.envs):
            if requests[e] is None:
                tr, c0 = p.candidate0.trajectory, p.candidate0
                requests[e] = (tr.times[:horizon], tr.states[:horizon], tr.actions[:horizon], c0.feedback_gain[:horizon],
                               c0.action_improvement[:horizon], np.zeros(p.num_trajectory_))
        shares = self._rollout(horizon, 0, 0, 1, requests)
        for p, out, (ret, fail) in zip(self.envs, self.sat_out, shares):
            if not out:
                p._iteration_after_rollouts(horizon, ret, fail)
        self.timers["rollouts"] = (_time.perf_counter() - t0) * 1e6

    def best_trajectory(self, env):
        return self.envs[env].best_trajectory()

    winner = property(lambda self: [p.winner for p in self.envs])
    action_step = property(lambda self: [p.action_step for p in self.envs])
    feedback_scaling = property(lambda self: [p.feedback_scaling for p in self.envs])
    dV = property(lambda self: [p.dV for p in self.envs])
    improvement = property(lambda self: [p.improvement for p in self.envs])
    expected = property(lambda self: [p.expected for p in self.envs])
    surprise = property(lambda self: [p.surprise for p in self.envs])
    regularization = property(lambda self: [p.regularization for p in self.envs])


# ====================================================================================== Gradient
K_MAX_GRADIENT_SPLINE_POINTS = 25  # gradient/spline_mapping.h:27


class GradientSettings:
    """GradientPlannerSettings, mjpc/planners/gradient/settings.h."""
    max_rollout = 1
    min_linesearch_step = 1.0e-8
    fd_tolerance = 1.0e-5
    fd_mode = 0
    action_limits = 1


class GradientPolicy:
    """GradientPolicy, mjpc/planners/gradient/policy.{h,cc}: P spline points of nu parameters, sampled as the rollout kernels
    sample them (spline.TimeSpline semantics) and clamped. This equals the reference's Zero / Linear / CubicInterpolation except for a
    cubic on two points, where the reference's FiniteDifferenceSlope takes the second point's slope as 0."""

    def __init__(self, model, task, horizon_cap=K_MAX_TRAJECTORY_HORIZON):
        self.model = model
        nu = model.nu
        self.k = np.zeros((horizon_cap, nu))
        self.parameters = np.zeros((horizon_cap, nu))
        self.parameter_update = np.zeros((horizon_cap, nu))
        self.times = np.zeros(horizon_cap)
        self.num_parameters = nu * horizon_cap
        # the reference's default is kMaxTrajectoryHorizon, its mappings hold 25 points: clamped to [1, 25]
        P = int(model.get_number("gradient_spline_points", K_MAX_TRAJECTORY_HORIZON))
        self.num_spline_points = min(max(P, 1), K_MAX_GRADIENT_SPLINE_POINTS)
        self.representation = int(model.get_number("gradient_representation", LINEAR))

    def reset(self, horizon, initial_repeated_action=None):
        self.k[:horizon] = 0
        self.parameters[:horizon] = 0 if initial_repeated_action is None else np.asarray(initial_repeated_action, float)
        self.parameter_update[:horizon] = 0
        self.times[:horizon] = 0

    def copy_from(self, other, horizon=None):
        for name in ("k", "parameters", "parameter_update", "times"):
            getattr(self, name)[...] = getattr(other, name)
        self.num_spline_points, self.num_parameters, self.representation = (other.num_spline_points, other.num_parameters,
                                                                            other.representation)

    def sample(self, time):
        """the spline before the clamp: FindInterval, then TimeSpline::Sample's interpolation and node slopes (spline.cc:103-156,
        269-287); after Reset every node time is 0 and the last node holds, as in the reference"""
        P, xs, ys = self.num_spline_points, self.times, self.parameters
        b0, b1 = find_interval(xs, time, P)
        if b0 == b1 or self.representation == ZERO:
            return ys[b0].copy()
        span = xs[b1] - xs[b0]
        t = (time - xs[b0]) / span
        if self.representation == LINEAR:
            return ys[b0] * (1.0 - t) + ys[b1] * t

        def slope(i):
            if i == 0:
                return (ys[1] - ys[0]) / (xs[1] - xs[0])
            if i == P - 1:
                return (ys[i] - ys[i - 1]) / (xs[i] - xs[i - 1])
            return 0.5 * (ys[i + 1] - ys[i]) / (xs[i + 1] - xs[i]) + 0.5 * (ys[i] - ys[i - 1]) / (xs[i] - xs[i - 1])
        c0, c1 = 2.0 * t * t * t - 3.0 * t * t + 1.0, (t * t * t - 2.0 * t * t + t) * span
        c2, c3 = -2.0 * t * t * t + 3 * t * t, (t * t * t - t * t) * span
        return c0 * ys[b0] + c1 * slope(b0) + c2 * ys[b1] + c3 * slope(b1)

    def action(self, action, state, time):
        """policy.cc:81-103 with the device's spline semantics"""
        action[:] = self.sample(time)
        return clamp(action, self.model.actuator_ctrlrange)


class GpuGradientPlanner(_ContextOwner):
    """mjpc::GradientPlanner (mjpc/planners/gradient/planner.{h,cc}, max_rollout = 1) with its device work on the GPU: the
    nominal and line-search rollouts (mjpcx_rollout_splines), finite-difference model derivatives (mjpcx_transition_fd), cost
    derivatives (mjpcx_cost_derivatives), and the adjoint sweep with its spline-mapping projection (mjpcx_gradient_pass).
    Host side: ResamplePolicy, the line-search steps, the selection, policy bookkeeping. Failed rollouts never win; the
    128-candidate cap is lifted; gradient_spline_points is clamped to [1, 25]."""

    def __init__(self, device=0, precision=64, backend_factory=None):
        self.device, self.precision = device, precision
        self._backend_factory = backend_factory
        self.settings = GradientSettings()
        self.mtx_ = threading.RLock()

    def initialize(self, model, task: Task):
        self.model, self.task = model, task
        self.dim_state = model.nq + model.nv + model.na
        self.dim_state_derivative = 2 * model.nv + model.na
        self.dim_action = model.nu
        self.num_trajectory = int(model.get_number("gradient_num_trajectory", 32))

    def allocate(self):
        m = self.model
        self.state = np.zeros(self.dim_state)
        self.mocap = np.zeros(7 * m.nmocap)
        self.userdata = np.zeros(m.nuserdata)
        self.time = 0.0
        self.policy = GradientPolicy(m, self.task)
        self.previous_policy = GradientPolicy(m, self.task)
        self.candidate0 = GradientPolicy(m, self.task)      # candidate_policy[0]
        self.trajectory0 = None                             # trajectory[0]
        self.differentiable_ = _agent_differentiable(m)
        self.ctx = self._create_context(self.differentiable_)

    def reset(self, horizon, initial_repeated_action=None):
        self.state[:] = 0; self.mocap[:] = 0; self.userdata[:] = 0
        self.time = 0.0
        for p in (self.policy, self.previous_policy, self.candidate0):
            p.reset(horizon, initial_repeated_action)
        self.trajectory0 = None
        self.dV = np.zeros(2)
        self.action_step = self.expected = self.improvement = self.surprise = 0.0
        self.winner = -1
        self.derivative_skip_ = int(self.model.get_number("derivative_skip", 0))
        self.linesearch_steps = np.zeros(0)
        self.timers = {}

    def set_state(self, state: State):
        self.state, self.mocap, self.userdata, self.time = state.copy_to()

    # ---- ResamplePolicy, planner.cc:355-381
    def resample_policy(self, horizon):
        c0 = self.candidate0
        P, nu = c0.num_spline_points, self.model.nu
        time_shift = max((horizon - 1) * self._timestep() / (P - 1), 1.0e-5) if P > 1 else 0.0   # (the planning model's opt.timestep)
        params = np.zeros((P, nu))
        nominal_time = self.time
        for t in range(P):
            c0.action(params[t], None, nominal_time)
            nominal_time += time_shift
        c0.parameters[:P] = params
        c0.times[:P] = self.time + np.arange(P) * time_shift     # LinearRange

    # ---- NominalTrajectory, planner.cc:300-311
    def nominal_trajectory(self, horizon, pool=None):
        c0 = self.candidate0
        P = c0.num_spline_points
        sync_task(self.ctx, self.task)
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        self.ctx.rollout_splines(horizon, c0.representation, c0.times[:P], c0.parameters[:P])
        self.trajectory0 = self.ctx.fetch_trajectory(0)

    # ---- OptimizePolicy, planner.cc:159-327
    def optimize_policy(self, horizon, pool=None):
        N = self.num_trajectory                             # the reference clamps to kMaxTrajectory = 128 (lifted)
        if N < 1:
            return
        T = horizon
        c0 = self.candidate0
        t0 = _time.perf_counter()
        with self.mtx_:
            c0.copy_from(self.policy)
        self.resample_policy(horizon)
        self.nominal_trajectory(horizon)
        tr = self.trajectory0
        c_prev = tr.total_return
        self.timers["nominal"] = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        st = self.settings
        A, B, C, D = model_derivatives(self.ctx, tr, T, self.derivative_skip_, st.fd_tolerance, st.fd_mode)
        A[T - 1] = 0; B[T - 1] = 0; D[T - 1] = 0
        self.timers["model_derivative"] = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        cx, cu, _, _, _ = self.ctx.cost_derivatives(tr.residual[:T], C, D)
        self.timers["cost_derivative"] = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        P = c0.num_spline_points
        out = self.ctx.gradient_pass(A, B, cx, cu, c0.representation, c0.times[:P], tr.times[:T])
        self.dV = out["dV"]
        c0.k[:T] = out["k"]
        c0.parameter_update[:P] = out["gradient"]
        self.timers["gradient"] = (_time.perf_counter() - t0) * 1e6
        # ---- Rollouts, planner.cc:384-418: theta + s_i * parameter_update, one batch
        t0 = _time.perf_counter()
        steps = self._linesearch_steps(N)
        nodes = c0.parameters[:P][None] + steps[:, None, None] * c0.parameter_update[:P][None]
        self.ctx.set_state(self.state, self.time, self.mocap, self.userdata)
        self.ctx.rollout_splines(T, c0.representation, c0.times[:P], nodes)
        ret, fail = self.ctx.returns()
        self._select(c_prev, ret, fail, nodes, steps, self.ctx.fetch_trajectory)
        self.timers["rollouts"] = (_time.perf_counter() - t0) * 1e6

    def _linesearch_steps(self, N):
        steps = np.zeros(N)
        if N > 1:
            steps[:N - 1] = log_scale(1.0, self.settings.min_linesearch_step, N - 1)
        self.linesearch_steps = steps
        return steps

    def _select(self, c_prev, ret, fail, nodes, steps, fetch):
        """the winner among the line-search rollouts and the policy update (planner.cc:262-327). fetch(winner) returns the winner's
        trajectory; None (a batch planner) leaves trajectory0 to be fetched when it is asked for."""
        N, c0 = len(steps), self.candidate0
        P = c0.num_spline_points
        c_best = c_prev
        # strict < from the last candidate down, starting from the nominal's return; failed rollouts never win
        winner = N - 1
        for j in range(N - 1, -1, -1):
            if fail[j]:
                continue
            if ret[j] < c_best:
                c_best, winner = float(ret[j]), j
        if c_best < c_prev:
            c0.parameters[:P] = nodes[winner]
            self.trajectory0 = fetch(winner) if fetch is not None else None
        self.winner = winner
        self.action_step = float(steps[winner])
        self.expected = -self.action_step * self.dV[0] - 1.0e-16
        self.improvement = c_prev - c_best
        self.surprise = min(max(0.0, self.improvement / self.expected), 2.0)
        if c_best >= c_prev:
            self.winner = N - 1
        with self.mtx_:
            self.previous_policy.copy_from(self.policy)
            self.policy.parameters[:P] = c0.parameters[:P]
            self.policy.times[:P] = c0.times[:P]

    def action_from_policy(self, action, state, time, use_previous=False):
        with self.mtx_:
            return (self.previous_policy if use_previous else self.policy).action(action, state, time)

    def best_trajectory(self):
        return self.trajectory0

    def num_parameters(self):
        return self.policy.num_spline_points * self.model.nu


def derivative_steps(T, derivative_skip):
    """the steps ModelDerivatives::Compute evaluates for derivative_skip (model_derivatives.cc:45-106; model_derivatives above)"""
    s = derivative_skip + 1
    evaluate = [0] + list(range(s, T - s, s)) + [T - 2, T - 1]
    return sorted(set(e for e in evaluate if 0 <= e < T))


class GpuBatchGradientPlanner(_Fleet):
    """The Gradient planner for `num_envs` environments (robots) on ONE context: a plan step is one `set_states`, one
    `rollout_splines_batched` of the resampled policies (64 candidates per environment, candidate 0 the nominal), one
    `gradient_step_batched` -- model derivatives, cost derivatives and the adjoint sweep of every environment chained on the device,
    the first sync --, one `rollout_splines_batched` of theta + s_i * parameter_update for all environments and `returns()`, the
    second sync: two host round trips for the fleet instead of six per robot. The environments share the model, the task (unless `set_tasks` gives each its own)
    and the settings; each has its own state, clock, mocap pose and policy. The per-environment logic (ResamplePolicy, the line-search
    steps, the selection rule with its ties toward the higher index, the policy bookkeeping) IS GpuGradientPlanner's, one member
    per environment. gradient_num_trajectory must be a positive multiple of 64."""

    def __init__(self, num_envs, device=0, precision=64, backend_factory=None):
        super().__init__(num_envs, device, precision, backend_factory)
        self.timers = {}
        # the members never roll out themselves: they are handed the shared context instead of creating their own
        self.envs = [GpuGradientPlanner(device, precision, backend_factory=lambda task: self.ctx) for _ in range(self.num_envs)]
        for p in self.envs:
            p.settings = self.envs[0].settings      # one GradientSettings for the fleet

    derivative_chain = True
    num_trajectory = _fleet_setting("num_trajectory")
    derivative_skip_ = _fleet_setting("derivative_skip_")
    settings = _fleet_setting("settings")
    _n_advice = "set gradient_num_trajectory / num_trajectory accordingly"

    def _reset_own(self):
        self._last = None
        self.timers = {}

    def _nominal_splines(self):
        """candidate0 of every environment, as _nominal_launch takes them: (representation, node times, node values)"""
        c0s = [p.candidate0 for p in self.envs]
        P = c0s[0].num_spline_points
        if any(c.num_spline_points != P or c.representation != c0s[0].representation for c in c0s):
            raise ValueError("the environments' policies have different spline shapes")
        return c0s[0].representation, np.stack([c.times[:P] for c in c0s]), [c.parameters[:P] for c in c0s]

    # ---- OptimizePolicy, gradient/planner.cc:159-327, for every environment
    def optimize_policy(self, horizon, pool=None):
        N = int(self.num_trajectory)
        self._check_n(N)
        T, E = horizon, self.num_envs
        t0 = _time.perf_counter()
        for p in self.envs:
            with p.mtx_:
                p.candidate0.copy_from(p.policy)
            p.resample_policy(horizon)
        rep, times, values = self._nominal_splines()
        self._nominal_launch(horizon, rep, times, values, fetch=False)    # gradient_step_batched reads the nominals on the device
        self.timers["nominal"] = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        first = self.envs[0]
        st, c0 = first.settings, first.candidate0
        P, rep = c0.num_spline_points, c0.representation
        out = self.ctx.gradient_step_batched(E, 0, T, derivative_steps(T, first.derivative_skip_), st.fd_tolerance, int(st.fd_mode), rep, times)
        self.timers["derivatives"] = (_time.perf_counter() - t0) * 1e6
        # ---- Rollouts, planner.cc:384-418: theta + s_i * parameter_update of every environment, one batch
        t0 = _time.perf_counter()
        nodes = []
        for e, p in enumerate(self.envs):
            p.dV = np.array(out["dV"][e])
            p.candidate0.k[:T] = out["k"][e]
            p.candidate0.parameter_update[:P] = out["gradient"][e]
            steps = p._linesearch_steps(N)
            nodes.append(p.candidate0.parameters[:P][None] + steps[:, None, None] * p.candidate0.parameter_update[:P][None])
        nodes = np.stack(nodes)
        self.ctx.rollout_splines_batched(T, rep, times, nodes, num_envs=E, n_per_env=N)
        ret, fail = self.ctx.returns()
        self._last, self._n = "plan", N
        for e, p in enumerate(self.envs):
            p.trajectory0 = None          # the winner's (or, without one, the zero step's = the nominal's) rollout: best_trajectory fetches it
            p._select(float(out["nominal_return"][e]), ret[e * N:(e + 1) * N], fail[e * N:(e + 1) * N], nodes[e], p.linesearch_steps, None)
        self.timers["rollouts"] = (_time.perf_counter() - t0) * 1e6

    def nominal_trajectory(self, horizon, pool=None):
        out = self._nominal_launch(horizon, *self._nominal_splines())
        for p, tr in zip(self.envs, out):
            p.trajectory0 = tr
        return out

    def best_trajectory(self, env):
        p = self.envs[env]
        if p.trajectory0 is None:
            p.trajectory0 = self._fetch_planned(env, p.winner)
        return p.trajectory0

    winner = property(lambda self: [p.winner for p in self.envs])
    dV = property(lambda self: [p.dV for p in self.envs])
    action_step = property(lambda self: [p.action_step for p in self.envs])
    improvement = property(lambda self: [p.improvement for p in self.envs])
    expected = property(lambda self: [p.expected for p in self.envs])
    surprise = property(lambda self: [p.surprise for p in self.envs])


# ====================================================================================== iLQS
SPLINE_FIT_NONE, SPLINE_FIT_OK, SPLINE_FIT_UNREACHED, SPLINE_FIT_NOT_POSITIVE_DEFINITE = -1, 0, 1, 2
SPLINE_FIT_UNREACHED_TOLERANCE = 1.0e-9   # SplineFit::kUnreachedTolerance


def fit_spline(interpolation, node_times, step_times, actions, ctrlrange=None):
    """mjpc::SplineFit (host/mjpc/planners/gpu_ilqs/spline_fit.h) in numpy: spline nodes fitted to `actions` at `step_times` by least
    squares, M built by sampling a TimeSpline of unit node vectors. An unreached node (column norm <= 1e-9 of the largest) takes
    the action at the nearest step time; the others solve the reduced normal equations. Returns (values P x nu, status, unreached)."""
    nt, st = np.asarray(node_times, float), np.asarray(step_times, float)
    a = np.asarray(actions, float).reshape(len(st), -1)
    P, nu = len(nt), a.shape[1]
    basis = TimeSpline(P, interpolation)
    for k in range(P):
        basis.add_node(nt[k], np.eye(P)[k])
    M = np.array([basis.sample(t) for t in st])
    norm = np.sqrt((M * M).sum(axis=0))
    reached = norm > SPLINE_FIT_UNREACHED_TOLERANCE * norm.max()
    unreached = int(P - reached.sum())
    x = np.zeros((P, nu))
    for k in np.flatnonzero(~reached):
        x[k] = a[int(np.argmin(np.abs(st - nt[k])))]
    R = M[:, reached]
    try:
        L = np.linalg.cholesky(R.T @ R)
    except np.linalg.LinAlgError:
        return np.zeros((P, nu)), SPLINE_FIT_NOT_POSITIVE_DEFINITE, unreached
    rhs = R.T @ (a - M[:, ~reached] @ x[~reached])
    x[reached] = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    if ctrlrange is not None:
        for k in range(P):
            clamp(x[k], ctrlrange)
    return x, (SPLINE_FIT_UNREACHED if unreached else SPLINE_FIT_OK), unreached


class GpuILQSPlanner:
    """mjpc::iLQSPlanner (mjpc/planners/ilqs/planner.{h,cc}) over the sampling and iLQG mirrors, each with its own context, both on
    the differentiable model unless agent_differentiable = 0. Deviations (host/mjpc/planners/gpu_ilqs/planner.h): the fit goes
    into the sampling winner's plan at the node times its update uses; unreached nodes are defined; an iLQG iteration that
    stopped early never activates iLQG; no cap on the spline points."""
    SAMPLING, ILQG = 0, 1

    def __init__(self, device=0, precision=64, seed=0, backend_factory=None):
        self.sampling = GpuSamplingPlanner(device, precision, seed, backend_factory=backend_factory)
        self.ilqg = GpuILQGPlanner(device, precision, backend_factory=backend_factory)

    def initialize(self, model, task: Task):
        self.model, self.task = model, task
        self.sampling.initialize(model, task)
        self.ilqg.initialize(model, task)

    def allocate(self):
        # the iLQG mirror reads agent_differentiable (default 1) itself; the sampling half is told the same
        self.sampling.differentiable = _agent_differentiable(self.model)
        self.sampling.allocate()
        self.ilqg.allocate()

    def reset(self, horizon, initial_repeated_action=None):
        self.sampling.reset(horizon, initial_repeated_action)
        self.ilqg.reset(horizon, initial_repeated_action)
        self._reset_own()

    def _reset_own(self):
        self.active_policy = self.previous_active_policy = self.SAMPLING
        self.ilqg_ran = False
        self.fit_status, self.fit_unreached = SPLINE_FIT_NONE, 0
        self.last_fit = None
        self.timers = {}

    def set_state(self, state: State):
        self.sampling.set_state(state)
        self.ilqg.set_state(state)

    def convert_policy(self, horizon):
        """iLQG's nominal actions -> the sampling spline, at the node times the sampling update lays out"""
        s = self.sampling
        P, nu = s.policy.num_spline_points, self.model.nu
        time_horizon = (horizon - 1) * s._timestep()
        if not s.sliding_plan_ and s.interpolation_ == ZERO:
            shift = max(time_horizon / P, 1.0e-5)
        else:
            shift = max(time_horizon / (P - 1), 1.0e-5) if P > 1 else float("inf")
        node_times, t = np.zeros(P), s.time
        for k in range(P):
            node_times[k] = t
            t += shift
        tr = self.ilqg.candidate0.trajectory
        step_times, actions = tr.times[:horizon - 1].copy(), tr.actions[:horizon - 1].copy()
        values, self.fit_status, self.fit_unreached = fit_spline(s.interpolation_, node_times, step_times, actions,
                                                                 self.model.actuator_ctrlrange)
        self.last_fit = dict(node_times=node_times, values=values, step_times=step_times, actions=actions)
        if self.fit_status == SPLINE_FIT_NOT_POSITIVE_DEFINITE:
            return
        plan = TimeSpline(nu, s.interpolation_)
        for k in range(P):
            plan.add_node(node_times[k], values[k])
        if s.sliding_plan_:
            with s.mtx_:
                s.policy.plan = plan
        else:
            s.winner_policy.plan = plan
            s.winner_policy.num_spline_points = P

    def _handoff(self, horizon):
        """ilqg.candidate_policy[0].trajectory = sampling.trajectory[0] (buffers keep their capacity)"""
        self._take_handoff(self.sampling.ctx.fetch_trajectory(0), horizon)
        # its nominal_trajectory did not run, so its context has not seen this plan's state (the derivatives read its mocap)
        g = self.ilqg
        g.ctx.set_state(g.state, g.time, g.mocap, g.userdata)

    def _take_handoff(self, got, horizon):
        tr = self.ilqg.candidate0.trajectory
        for name in ("states", "actions", "times", "residual", "costs", "trace"):
            getattr(tr, name)[:horizon] = getattr(got, name)[:horizon]
        tr.horizon, tr.total_return, tr.failure = horizon, got.total_return, got.failure

    # ---- OptimizePolicy, planner.cc:87-214
    def optimize_policy(self, horizon, pool=None):
        s, g = self.sampling, self.ilqg
        previous = self.previous_active_policy = self.active_policy
        g.num_trajectory_ = g.num_rollouts_gui_
        self.ilqg_ran = False
        self.fit_status, self.fit_unreached = SPLINE_FIT_NONE, 0
        self.timers = {}
        if previous == self.ILQG:
            t0 = _time.perf_counter()
            g.nominal_trajectory(horizon)
            self.timers["nominal"] = (_time.perf_counter() - t0) * 1e6
            t0 = _time.perf_counter()
            self.convert_policy(horizon)
            self.timers["fit"] = (_time.perf_counter() - t0) * 1e6
        t0 = _time.perf_counter()
        s.optimize_policy(horizon)
        self.timers["sampling"] = (_time.perf_counter() - t0) * 1e6
        reference = s.nominal_return if previous == self.SAMPLING else g.candidate0.trajectory.total_return
        if s.winner > 0 and s.best_return < reference:
            self.active_policy = self.SAMPLING
            return
        if previous == self.SAMPLING:
            self._handoff(horizon)
        t0 = _time.perf_counter()
        g.iteration(horizon)
        self.timers["iteration"] = (_time.perf_counter() - t0) * 1e6
        self.ilqg_ran = True
        reference = s.best_return if previous == self.SAMPLING else g.linesearch0_return
        if g.iteration_completed and g.winner_return < reference:
            self.active_policy = self.ILQG

    def nominal_trajectory(self, horizon, pool=None):
        if self.active_policy == self.SAMPLING:
            return self.sampling.nominal_trajectory(horizon)
        return self.ilqg.nominal_trajectory(horizon)

    # ---- ActionFromPolicy, planner.cc:228-253
    def action_from_policy(self, action, state, time, use_previous=False):
        if use_previous:
            if self.previous_active_policy == self.SAMPLING:
                return self.sampling.action_from_policy(action, state, time, True)
            # iLQG was previously active: if the last plan stopped after sampling, iLQG's current policy is the previous one
            return self.ilqg.action_from_policy(action, state, time, self.active_policy == self.ILQG)
        if self.active_policy == self.SAMPLING:
            return self.sampling.action_from_policy(action, state, time, False)
        return self.ilqg.action_from_policy(action, state, time, False)

    def best_trajectory(self):
        return self.sampling.best_trajectory() if self.active_policy == self.SAMPLING else self.ilqg.best_trajectory()

    def num_parameters(self):
        return self.sampling.num_parameters() + self.ilqg.num_parameters()


class _ILQSMember(GpuILQSPlanner):
    """GpuILQSPlanner over two members of fleet planners instead of two planners of its own: convert_policy, action_from_policy and the
    per-member state are its; the plan step is GpuBatchILQSPlanner's"""

    def __init__(self, sampling, ilqg):
        self.sampling, self.ilqg = sampling, ilqg


class GpuBatchILQSPlanner:
    """iLQS for `num_envs` environments (robots): a GpuBatchSamplingPlanner and a GpuBatchILQGPlanner, one context each, both on the
    differentiable model unless agent_differentiable = 0. Member e plans exactly like GpuILQSPlanner(seed = seed + e); the member
    logic (convert_policy, the comparisons of ilqs/planner.cc:87-214, ActionFromPolicy) IS that planner's. In one plan step the fleet
    is mixed -- some members' active policy is sampling, others' iLQG -- and the step is, whatever E:
      1. the nominal rollouts of the members whose active policy is iLQG (P): one `rollout_feedback_batched` on the iLQG context, the
         others riding on the first P member's request and ignored; then each P member's spline fit, on the host;
      2. sampling for all: one `rollout_noise_batched` + `best_batched` on the sampling context;
      3. per member the comparison; C = the members that go on to iLQG;
      4. the hand-off: a C member outside P takes candidate 0 of its share of the sampling rollout into candidate0.trajectory (the
         host needs it for the line search and the policy bookkeeping); `set_states` on the iLQG context;
      5. ONE `ilqg_step_batched_from`: hand-off members name the sampling context's candidate 0, P members their own best nominal
         rollout, members outside C -1. The nominals never pass through the host. (`device_chain = False`, a fleet
         GpuBatchILQGPlanner._use_device_chain turns away, or a P member whose nominal rollouts all failed: the sequential chain.);
      6. ONE line-search `rollout_feedback_batched`; members outside C and members whose backward pass failed ride along with zero steps.
    At most four syncs and the hand-off fetches. `backend_factory(task, half)`, half in ("sampling", "ilqg"), gives test backends.
    timers: nominal, fit, sampling, handoff, derivatives_backward, rollouts (us). last_step: (from_source, candidate, status) of the
    plan step's ilqg_step_batched_from, None when there was none."""
    SAMPLING, ILQG = GpuILQSPlanner.SAMPLING, GpuILQSPlanner.ILQG

    def __init__(self, num_envs, device=0, precision=64, seed=0, backend_factory=None):
        if int(num_envs) < 1:
            raise ValueError("GpuBatchILQSPlanner needs at least one environment")
        self.num_envs, self.device, self.precision, self.seed = int(num_envs), device, precision, seed
        half = lambda name: (lambda task: backend_factory(task, name)) if backend_factory is not None else None
        self.sampling = GpuBatchSamplingPlanner(num_envs, device, precision, seed, backend_factory=half("sampling"))
        self.ilqg = GpuBatchILQGPlanner(num_envs, device, precision, backend_factory=half("ilqg"))
        self.envs = [_ILQSMember(s, g) for s, g in zip(self.sampling.envs, self.ilqg.envs)]
        self.model = self.task = None
        self.device_chain = None    # None: ilqg_step_batched_from whenever the iLQG context has it; False: the sequential middle
        self.used_device_chain = False
        self.last_step = None
        self.timers = {}

    def initialize(self, model, task: Task):
        self.model, self.task = model, task
        self.sampling.initialize(model, task)
        self.ilqg.initialize(model, task)
        for m in self.envs:
            m.model, m.task = model, task

    def set_tasks(self, tasks):
        """one Task per environment, for both halves (_Fleet.set_tasks)"""
        self.sampling.set_tasks(tasks)
        self.ilqg.set_tasks(tasks)
        for e, m in enumerate(self.envs):
            m.task = self.task if tasks is None else self.sampling.envs[e].task

    def set_models(self, models):
        """not for a planner with a derivative chain: the batched derivative calls use the context's one model"""
        raise NotImplementedError(_Fleet._MODELS_FOLLOW_UP)

    def allocate(self):
        # the iLQG half reads agent_differentiable (default 1) itself; the sampling half is told the same
        self.sampling.differentiable = _agent_differentiable(self.model)
        self.sampling.allocate()
        self.ilqg.allocate()

    def reset(self, horizon, initial_repeated_action=None):
        self.sampling.reset(horizon, initial_repeated_action)
        self.ilqg.reset(horizon, initial_repeated_action)
        for m in self.envs:
            m._reset_own()
        self.last_step = None
        self.timers = {}

    def set_states(self, states):
        """one State per environment (Planner::SetState for each)"""
        self.sampling.set_states(states)
        self.ilqg.set_states(states)

    def _use_device_chain(self):
        g = self.ilqg
        if self.device_chain is not None and not self.device_chain:
            return False
        if not hasattr(g.ctx, "ilqg_step_batched_from"):
            if self.device_chain:
                raise ValueError("GpuBatchILQSPlanner: device_chain on a context without ilqg_step_batched_from")
            return False
        return g._use_device_chain()

    # ---- OptimizePolicy, ilqs/planner.cc:87-214, for every environment
    def optimize_policy(self, horizon, pool=None):
        s, g, E = self.sampling, self.ilqg, self.num_envs
        s._check_n(s.num_trajectory_)
        g._prepare()
        self.timers = dict.fromkeys(("nominal", "fit", "sampling", "handoff", "derivatives_backward", "rollouts"), 0.0)
        self.last_step = None
        for m in self.envs:
            m.previous_active_policy = m.active_policy
            m.ilqg_ran = False
            m.fit_status, m.fit_unreached = SPLINE_FIT_NONE, 0
            m.timers = {}
        P = [e for e, m in enumerate(self.envs) if m.previous_active_policy == self.ILQG]
        in_P = set(P)
        # ---- 1. iLQG's nominal for the members it was active for, and their policy conversion
        if P:
            t0 = _time.perf_counter()
            first = g.envs[P[0]]
            requests = {e: g.envs[e]._nominal_request(horizon) for e in P}
            shares = g._rollout(horizon, 1, first.policy.representation, first.settings.nominal_feedback_scaling,
                                [requests.get(e, requests[P[0]]) for e in range(E)])
            for e in P:
                g.envs[e]._nominal_select(horizon, *shares[e])
            self.timers["nominal"] = (_time.perf_counter() - t0) * 1e6
            t0 = _time.perf_counter()
            for e in P:
                self.envs[e].convert_policy(horizon)
            self.timers["fit"] = (_time.perf_counter() - t0) * 1e6
        # ---- 2. sampling, every member
        t0 = _time.perf_counter()
        s.optimize_policy(horizon)
        self.timers["sampling"] = (_time.perf_counter() - t0) * 1e6
        # ---- 3. who goes on to iLQG
        C = []
        for e, m in enumerate(self.envs):
            sp, gp = s.envs[e], g.envs[e]
            reference = sp.nominal_return if e not in in_P else gp.candidate0.trajectory.total_return
            if sp.winner > 0 and sp.best_return < reference:
                m.active_policy = self.SAMPLING
            else:
                C.append(e)
        if not C:
            return
        # ---- 4. ilqg.candidate_policy[0].trajectory = sampling.trajectory[0], the host's copy; the iLQG context sees this plan's states
        t0 = _time.perf_counter()
        n = s.num_trajectory_
        for e in C:
            if e not in in_P:
                self.envs[e]._take_handoff(s.ctx.fetch_trajectory(e * n), horizon)
        g._push_states()
        self.timers["handoff"] = (_time.perf_counter() - t0) * 1e6
        # ---- 5. derivatives and the backward pass: one call for the fleet, each nominal gathered from the context that holds it
        t0 = _time.perf_counter()
        requests = [None] * E
        self.used_device_chain = self._use_device_chain()
        candidate, from_source = [-1] * E, [0] * E
        for e in C:
            if e not in in_P:
                candidate[e], from_source[e] = 0, 1
            else:
                candidate[e] = g.envs[e].nominal_index      # -1: every nominal rollout failed, the nominal is the host's policy trajectory
        if self.used_device_chain and max(candidate) >= 0:
            out = g.ctx.ilqg_step_batched_from(s.ctx, from_source, candidate, *g._step_args(horizon))
            requests = g._scatter_step(out, horizon)
            self.last_step = (list(from_source), list(candidate), [int(x) for x in out["status"]])
        else:
            candidate = [-1] * E
        for e in C:
            if candidate[e] < 0:
                requests[e] = g._sequential_middle(g.envs[e], horizon)
        self.timers["derivatives_backward"] = (_time.perf_counter() - t0) * 1e6
        # ---- 6. the line search of the members that got that far: one launch; the others ride along with zero steps and are ignored
        self.sat_out = [r is None for r in requests]
        if not all(self.sat_out):
            t0 = _time.perf_counter()
            lead = next(r for r in requests if r is not None)
            zero = lead[:5] + (np.zeros(len(lead[5])),)
            shares = g._rollout(horizon, 0, 0, 1, [zero if r is None else r for r in requests])
            for e in range(E):
                if not self.sat_out[e]:
                    g.envs[e]._iteration_after_rollouts(horizon, *shares[e])
            self.timers["rollouts"] = (_time.perf_counter() - t0) * 1e6
        for e in C:
            m, sp, gp = self.envs[e], s.envs[e], g.envs[e]
            m.ilqg_ran = True
            reference = sp.best_return if e not in in_P else gp.linesearch0_return
            if gp.iteration_completed and gp.winner_return < reference:
                m.active_policy = self.ILQG

    def action_from_policy(self, env, action, state, time, use_previous=False):
        return self.envs[env].action_from_policy(action, state, time, use_previous)

    def best_trajectory(self, env):
        if self.envs[env].active_policy == self.SAMPLING:
            return self.sampling.best_trajectory(env)
        return self.ilqg.best_trajectory(env)

    def num_parameters(self):
        return self.sampling.num_parameters() + self.ilqg.num_parameters()

    active_policy = property(lambda self: [m.active_policy for m in self.envs])
    previous_active_policy = property(lambda self: [m.previous_active_policy for m in self.envs])
    ilqg_ran = property(lambda self: [m.ilqg_ran for m in self.envs])
    fit_status = property(lambda self: [m.fit_status for m in self.envs])
    fit_unreached = property(lambda self: [m.fit_unreached for m in self.envs])
    last_fit = property(lambda self: [m.last_fit for m in self.envs])
