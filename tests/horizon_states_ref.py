"""Yardsticks of the predicted-horizon-states tests (tests/test_horizon_states_abi.py, tests/test_gpu_horizon_states.py).  None of them is the kernel:
  rollout            the recurrence of include/a1mpc.h (a1mpc_horizon_states_batch) restated in numpy.longdouble, vectorised over the QPs, with the sum of the absolute
                     values of every accumulated term beside each state (the scale of the states bar: cancellation does not enter)
  reference_states   A_qp x0 + B_qp u on the reference's own A_qp / B_qp (S/ConvexMpc.cpp compiled verbatim, oracle/_ref), with |A_qp||x0| + |B_qp||u| and its P, g
  cost_gap           the cost identity cost[0](u) + cost[1](u) - cost[0](0) = 1/2 u'Pu + g'u as a ratio to the sum of the absolute values of its terms
BAR = 1e-12 is the bar tests/test_gpu_pipeline_and_instrumentation.py::test_gpu_formed_dense_qp_equals_reference_ConvexMpc holds the GPU's P to against the same library."""
import numpy as np

LD = np.longdouble
BAR = 1e-12


def _inv3(M):
    """inverse of (n, 3, 3) by cofactors, in M's dtype (numpy.linalg has no longdouble)"""
    a, b, c, d, e, f, g, h, i = (M[:, r, k] for r in range(3) for k in range(3))
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * c00 + b * c01 + c * c02
    out = np.empty_like(M)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = c00 / det, (c * h - b * i) / det, (b * f - c * e) / det
    out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = c01 / det, (a * i - c * g) / det, (c * d - a * f) / det
    out[:, 2, 0], out[:, 2, 1], out[:, 2, 2] = c02 / det, (b * g - a * h) / det, (a * e - b * d) / det
    return out


def _skew(r):
    """(..., 3) -> (..., 3, 3), S/utils/Utils.cpp skew"""
    S = np.zeros(r.shape + (3,), r.dtype)
    S[..., 0, 1], S[..., 0, 2] = -r[..., 2], r[..., 1]
    S[..., 1, 0], S[..., 1, 2] = r[..., 2], -r[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -r[..., 1], r[..., 0]
    return S


def rollout(params, h, x0, R, foot, foot_stride=0, u=None, yaw=None, steps=None):
    """-> (X, S), each (n, steps, 13) longdouble: X[:, t] = x_(t+1) of x_(t+1) = A_d x_t + B_d,t u_t from x_0 = x0 (A_d = I + dt A_c, B_d,t = dt B_c,t, S/ConvexMpc.cpp:110-151),
    S[:, t] = the same recurrence on absolute values (|A_d| S_t + |B_d,t||u_t| from S_0 = |x0|).  cos / sin of the yaw are the model's inputs and taken in double, as the
    reference takes them (:112-113); everything after them is longdouble."""
    x0 = np.asarray(x0, np.float64); n = x0.shape[0]; steps = h if steps is None else steps
    dt = LD(params["dt"]); bv = dt / LD(params["mass"])
    yaw = x0[:, 2] if yaw is None else np.asarray(yaw, np.float64)
    c, s = np.cos(yaw).astype(LD), np.sin(yaw).astype(LD)
    T = np.zeros((n, 3, 3), LD)
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 2, 2] = c, s, -s, c, 1
    Rm = np.asarray(R, np.float64).reshape(n, 3, 3).astype(LD)
    Ib = np.asarray(params["inertia"], np.float64).reshape(3, 3).astype(LD)
    Ii = _inv3(np.einsum("nij,jk,nlk->nil", Rm, Ib, Rm))
    feet = np.asarray(foot, np.float64).reshape(n, h if foot_stride else 1, 4, 3).astype(LD)
    U = np.zeros((n, h, 4, 3), LD) if u is None else np.asarray(u, np.float64).reshape(n, h, 4, 3).astype(LD)
    x = x0.astype(LD); sx = np.abs(x)
    X = np.zeros((n, steps, 13), LD); S = np.zeros((n, steps, 13), LD)
    for t in range(steps):
        Bw = dt * np.einsum("nij,nljk->nlik", Ii, _skew(feet[:, t if foot_stride else 0]))     # (n, leg, 3, 3)
        f = U[:, t]
        xn = x.copy(); sn = sx.copy()
        xn[:, 0:3] += dt * np.einsum("nij,nj->ni", T, x[:, 6:9]); sn[:, 0:3] += dt * np.einsum("nij,nj->ni", np.abs(T), sx[:, 6:9])
        xn[:, 3:6] += dt * x[:, 9:12]; sn[:, 3:6] += dt * sx[:, 9:12]
        xn[:, 6:9] += np.einsum("nlik,nlk->ni", Bw, f); sn[:, 6:9] += np.einsum("nlik,nlk->ni", np.abs(Bw), np.abs(f))
        xn[:, 9:12] += bv * f.sum(1); sn[:, 9:12] += bv * np.abs(f).sum(1)
        xn[:, 11] += dt * x[:, 12]; sn[:, 11] += dt * sx[:, 12]
        x, sx = xn, sn
        X[:, t], S[:, t] = x, sx
    return X, S


def reference_states(REF, params, h, x0, xref, R, foot, foot_stride, contact, u=None, yaw=None):
    """-> dict(X, S (n, h, 13) longdouble, P (n, 12h, 12h), g (n, 12h)): X = A_qp x0 + B_qp u, S = |A_qp||x0| + |B_qp||u| on the A_qp / B_qp the reference's ConvexMpc
    fills (REF.convex_mpc_form(..., want_AB=True)); the two products are taken in longdouble so that the yardstick's own rounding stays out of the comparison"""
    n = len(x0); p = params
    X = np.zeros((n, h, 13), LD); S = np.zeros((n, h, 13), LD); P = np.zeros((n, 12 * h, 12 * h)); g = np.zeros((n, 12 * h))
    for b in range(n):
        eul = np.array(x0[b][:3]); eul[2] = x0[b][2] if yaw is None else yaw[b]
        r = REF.convex_mpc_form(h, p["q"], p["r"], eul, p["mass"], p["inertia"], R[b], foot[b], contact[b], x0[b], xref[b], p["dt"], foot_stride=foot_stride, want_AB=True)
        A, B = r["A_qp"].astype(LD), r["B_qp"].astype(LD)
        ub = np.zeros(12 * h, LD) if u is None else np.asarray(u[b], np.float64).astype(LD)
        xb = np.asarray(x0[b], np.float64).astype(LD)
        X[b] = (A @ xb + B @ ub).reshape(h, 13); S[b] = (np.abs(A) @ np.abs(xb) + np.abs(B) @ np.abs(ub)).reshape(h, 13)
        P[b], g[b] = r["P"], r["g"]
    return dict(X=X, S=S, P=P, g=g)


def states_ratio(x_pred, X, S):
    """max over the 12 dynamic components of |x_pred - X| / S (the bar is BAR); S > 0 on every component the tests look at"""
    d = np.abs(np.asarray(x_pred).astype(LD) - X)[..., :12]
    return float((d / S[..., :12]).max())


def cost_gap(cost_u, cost_0, P, g, u):
    """per QP: |cost[0](u) + cost[1](u) - cost[0](0) - (1/2 u'Pu + g'u)| / (cost[0](u) + cost[0](0) + cost[1](u) + 1/2 |u|'|P||u| + |g|'|u|), products in longdouble"""
    cu, c0 = np.asarray(cost_u).astype(LD), np.asarray(cost_0).astype(LD)
    uu = np.asarray(u, np.float64).astype(LD); Pl = np.asarray(P).astype(LD); gl = np.asarray(g).astype(LD)
    quad = LD(0.5) * np.einsum("ni,nij,nj->n", uu, Pl, uu) + np.einsum("ni,ni->n", gl, uu)
    scale = cu[:, 0] + c0[:, 0] + cu[:, 1] + LD(0.5) * np.einsum("ni,nij,nj->n", np.abs(uu), np.abs(Pl), np.abs(uu)) + np.einsum("ni,ni->n", np.abs(gl), np.abs(uu))
    return np.abs(cu[:, 0] + cu[:, 1] - c0[:, 0] - quad) / scale


def costs(params, h, X, xref, u=None):
    """(n, 2) longdouble: [sum q_k (x_(t+1),k - x_ref_t,k)^2, sum r_j u_(t,j)^2] of a trajectory X (n, h, 13) -- the definition in include/a1mpc.h"""
    n = X.shape[0]
    q = np.asarray(params["q"], np.float64)[:12].astype(LD); r = np.asarray(params["r"], np.float64).astype(LD)
    e = X[..., :12] - np.asarray(xref, np.float64).reshape(n, h, 13)[..., :12].astype(LD)
    out = np.zeros((n, 2), LD)
    out[:, 0] = (q * e * e).sum((1, 2))
    if u is not None:
        uu = np.asarray(u, np.float64).reshape(n, h, 12).astype(LD)
        out[:, 1] = (r * uu * uu).sum((1, 2))
    return out
