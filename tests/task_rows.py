"""Test helper: E unlike sets of task parameters for one task -- weights, norm parameters, residual parameters and risk -- as the rows
mjpcx_set_task_params_batched takes and as E Task objects for the planners' set_tasks. Never used by the product."""
import copy

import numpy as np

RISKS = (0.0, 0.5, -0.5)          # risk-neutral, risk-averse, risk-seeking
LISTS = ("dim_norm_residual", "num_norm_parameter", "norm", "weight", "weight_names", "norm_parameter", "parameters", "trace_site",
         "residual_int", "residual_real")


def unlike_rows(task, E, seed=5, risks=RISKS):
    """dict of weight E x num_term, norm_parameter E x (sum of num_norm_parameter), parameters E x num_parameter, risk E: every
    weight scaled by 0.5 .. 2, every norm parameter by 0.7 .. 1.5 (they stay positive), every residual parameter that is not a
    selection scaled by 0.8 .. 1.2 and moved by 0.01 .. 0.1, risks cycling through `risks`"""
    rng = np.random.default_rng(seed)
    weight = np.array(task.weight, float)[None] * rng.uniform(0.5, 2.0, (E, len(task.weight)))
    norm_parameter = np.array(task.norm_parameter, float).reshape(1, -1) * rng.uniform(0.7, 1.5, (E, len(task.norm_parameter)))
    names = [k for k in task.model.numeric if k.startswith("residual_")]
    parameters = np.tile(np.array(task.parameters, float).reshape(1, -1), (E, 1))
    for j, name in enumerate(names):
        if not name.startswith("residual_select_"):
            parameters[:, j] = parameters[:, j] * rng.uniform(0.8, 1.2, E) + rng.uniform(0.01, 0.1, E)
    return dict(weight=weight, norm_parameter=norm_parameter, parameters=parameters, risk=np.array([risks[e % len(risks)] for e in range(E)], float))


def copy_task(task):
    """a Task that shares the model and nothing that a planner or a transition writes"""
    t = copy.copy(task)
    for k in LISTS:
        setattr(t, k, list(getattr(task, k)))
    return t


def task_of_row(task, rows, e):
    t = copy_task(task)
    t.weight, t.norm_parameter = [float(x) for x in rows["weight"][e]], [float(x) for x in rows["norm_parameter"][e]]
    t.parameters, t.risk = [float(x) for x in rows["parameters"][e]], float(rows["risk"][e])
    return t


def unlike_tasks(task, E, seed=5, risks=RISKS):
    """E Tasks with the rows of unlike_rows. QuadrupedFlat: the environments are also given different gaits (stand, walk, trot, ...) and
    modes (Quadruped, Biped, ...) through transition(), so their frozen residual state differs, before the rows are applied; the
    selections the residual state was frozen from are kept."""
    bases = []
    for e in range(E):
        t = copy_task(task)
        if task.name == "QuadrupedFlat":
            t.parameters[t.ids["gait"]] = float(e % 3)
            t.transition(0.0, mode=e % 2)
        bases.append(t)
    out = []
    for e, t in enumerate(bases):
        rows = unlike_rows(t, E, seed, risks)
        out.append(task_of_row(t, rows, e))
        if task.name == "QuadrupedFlat":
            out[-1]._freeze()
    return out


def rows_of(tasks):
    """the rows of set_task_params_batched from E Tasks"""
    arr = lambda k: np.array([getattr(t, k) for t in tasks], float).reshape(len(tasks), -1)
    return dict(weight=arr("weight"), norm_parameter=arr("norm_parameter"), parameters=arr("parameters"), risk=np.array([float(t.risk) for t in tasks]))
