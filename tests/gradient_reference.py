"""CPU restatement of the Gradient planner's first-order math (test infrastructure only):
   spline_mapping      mjpc/planners/gradient/spline_mapping.cc:25-205  (Zero / Linear / CubicSplineMapping::Compute)
   gradient_sweep      mjpc/planners/gradient/gradient.cc:43-108         (Gradient::GradientStep + Compute)
   gradient_pass       both, with parameter_update = M^T k as gradient/planner.cc:247-257 forms it
and an oracle-backed context that adds gradient_pass to tests/oracle_backend.py's OracleContext."""
import numpy as np

from mujoco_mpc_amd.planners import find_interval
from oracle_backend import OracleContext


def cubic_coefficients(x, xs, length):
    """CubicCoefficients, utilities.cc:337-359"""
    b0, b1 = find_interval(xs, x, length)
    if b0 == b1:
        return np.array([1.0, 0.0, 0.0, 0.0])
    span = xs[b1] - xs[b0]
    t = (x - xs[b0]) / span
    return np.array([2.0 * t * t * t - 3.0 * t * t + 1.0, (t * t * t - 2.0 * t * t + t) * span, -2.0 * t * t * t + 3 * t * t,
                     (t * t * t - t * t) * span])


def spline_mapping(representation, input_times, output_times, dim=1):
    """M (dim * num_output x dim * num_input): the Jacobian of the output-time actions w.r.t. the spline parameters, as the
    reference's SplineMapping::Compute builds it"""
    xs = np.asarray(input_times, float)
    P, To = len(xs), len(output_times)
    M = np.zeros((dim * To, dim * P))
    if representation in (0, 1):
        for i, x in enumerate(output_times):
            b0, b1 = find_interval(xs, x, P)
            for j in range(dim):
                if representation == 0 or b0 == b1:
                    M[dim * i + j, dim * b0 + j] = 1.0
                else:
                    a = (x - xs[b0]) / (xs[b1] - xs[b0])
                    M[dim * i + j, dim * b0 + j] = 1.0 - a
                    M[dim * i + j, dim * b1 + j] = a
        return M
    # cubic: point_slope_mapping [I; D] (2 dim P x dim P), then the output mapping (dim To x 2 dim P), then their product
    S = np.zeros((2 * dim * P, dim * P))
    for i in range(P):
        for j in range(dim):
            S[dim * i + j, dim * i + j] = 1.0
    for i in range(P):
        dt1 = 1.0 / (xs[i] - xs[i - 1]) if i > 0 else 0.0
        dt2 = 1.0 / (xs[i + 1] - xs[i]) if i < P - 1 else 0.0
        if 0 < i < P - 1:
            dt1 *= 0.5
            dt2 *= 0.5
        for j in range(dim):
            r = dim * P + dim * i + j
            if i - 1 >= 0:
                S[r, dim * (i - 1) + j] = -dt1
            S[r, dim * i + j] = dt1 - dt2
            if i + 1 <= P - 1:
                S[r, dim * (i + 1) + j] = dt2
    O = np.zeros((dim * To, 2 * dim * P))
    for i, x in enumerate(output_times):
        b0, b1 = find_interval(xs, x, P)
        c = cubic_coefficients(x, xs, P)
        for j in range(dim):
            O[dim * i + j, dim * b0 + j] = c[0]
            O[dim * i + j, dim * P + dim * b0 + j] = c[1]
            if b0 != b1:
                O[dim * i + j, dim * b1 + j] = c[2]
                O[dim * i + j, dim * P + dim * b1 + j] = c[3]
    return O @ S


def gradient_sweep(A, B, cx, cu):
    """Gradient::Compute: Vx (T x n), k (T x m), dV[2]"""
    T, n = cx.shape
    m = cu.shape[1]
    Vx, k, dV = np.zeros((T, n)), np.zeros((T, m)), np.zeros(2)
    Vx[T - 1] = cx[T - 1]
    for t in range(T - 1, 0, -1):
        Qx = A[t - 1].T @ Vx[t] + cx[t - 1]
        Qu = B[t - 1].T @ Vx[t] + cu[t - 1]
        k[t - 1] = -Qu
        Vx[t - 1] = Qx
        dV[0] += k[t - 1] @ Qu
    k[T - 1] = k[T - 2]
    return Vx, k, dV


def gradient_pass(A, B, cx, cu, representation, node_times, step_times):
    """what mjpcx_gradient_pass returns: the sweep and parameter_update = M^T k (P x m), M over the first T - 1 step times"""
    A, B, cx, cu = (np.asarray(x, float) for x in (A, B, cx, cu))
    T, m = cu.shape
    Vx, k, dV = gradient_sweep(A, B, cx, cu)
    M = spline_mapping(representation, node_times, np.asarray(step_times, float)[:T - 1], dim=m)
    g = M.T @ k[:T - 1].reshape(-1)
    return dict(Vx=Vx, k=k, dV=dV, gradient=g.reshape(len(node_times), m), kernel_ms=0.0)


class OracleGradientContext(OracleContext):
    """OracleContext (CPU oracle rollouts and derivatives) with the gradient pass restated above"""

    def gradient_pass(self, A, B, cx, cu, representation, node_times, step_times):
        return gradient_pass(A, B, cx, cu, representation, node_times, step_times)
