"""The stability measures of a device walk (include/cmpc.h, "physical limits") as a function of their 44 inputs per (row, problem), restated in numpy
float64 with no float32 cast anywhere, on tests/walk_limits_ref.py's hull / signed_distance -- the support region as a HULL, so that it shares nothing
with the product's minimum over candidate directions -- and its finite differences.  Not product code: the tests hold the library's derivative
(include/cmpc.h, "the measures, differentiated") to it.  Input order: com[3], dcom[3], q[2][3], omega[2][3], corner[2][4][3], comRef_xy[2]."""
import ctypes as C

import numpy as np

import cmpc_amd as cm
from tests import walk_limits_ref as wl

N_IN = 44
COM, DCOM, Q, OMEGA, CORNER, REF = slice(0, 3), slice(3, 6), slice(6, 12), slice(12, 18), slice(18, 42), slice(42, 44)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def exp_so3(w):
    """Rodrigues: the rotation matrix Exp(w) of a rotation vector"""
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * K @ K


def inputs(N, X, P, state_out, corners, b):
    """-> (u[44] float64 with omega = 0, ctx): the independent inputs of problem b of one tape row, and what stays fixed (the stage-1 rotations as float64
    matrices, the support set, whether the state is finite)"""
    L = cm.Layout(N)
    corners = np.broadcast_to(np.asarray(corners, np.float64), (X.shape[0], 2, 4, 3))
    u = np.zeros(N_IN)
    s = state_out[b].astype(np.float64)
    u[COM], u[DCOM] = s[:3], s[3:6]
    for c in range(2):
        u[6 + 3 * c:9 + 3 * c] = X[b, L.pos[c] + 3:L.pos[c] + 6].astype(np.float64)
    u[CORNER] = corners[b].reshape(-1)
    u[REF] = P[b, L.p_comref + 3:L.p_comref + 5].astype(np.float64)
    ctx = dict(R=[P[b, L.p_R[c] + 9:L.p_R[c] + 18].astype(np.float64).reshape(3, 3, order="F") for c in range(2)],
               on=[bool(P[b, L.p_gam[c] + 1] > 0.5) for c in range(2)], finite=bool(np.isfinite(state_out[b]).all()))
    return u, ctx


def measures(u, ctx, gravity):
    """the four measures at inputs u[44]: height, reach, margin (signed distance to the hull), track; NaN as the forward reports them"""
    out = np.full(4, np.nan)
    if not ctx["finite"]:
        return out
    com, dcom, q, om, cn, ref = u[COM], u[DCOM], u[Q].reshape(2, 3), u[OMEGA].reshape(2, 3), u[CORNER].reshape(2, 4, 3), u[REF]
    out[3] = np.hypot(com[0] - ref[0], com[1] - ref[1])
    feet = [c for c in range(2) if ctx["on"][c]]
    if not feet:
        return out
    height = com[2] - np.mean([q[c][2] for c in feet])
    out[0] = height
    out[1] = max(np.linalg.norm(com - q[c]) for c in feet)
    xi = com[:2] + dcom[:2] * np.sqrt(max(height, 0.0) / gravity)
    pts = []
    for c in feet:
        R = ctx["R"][c] @ exp_so3(om[c])
        pts += [(q[c] + R @ cn[c, j])[:2] for j in range(4)]
    out[2] = wl.signed_distance(pts, xi)
    return out


def differences(u, ctx, gravity, h):
    """-> (forward, backward, central) finite differences [4, 44] of measures() at step h"""
    f0 = measures(u, ctx, gravity)
    fwd, bwd, cen = np.zeros((4, N_IN)), np.zeros((4, N_IN)), np.zeros((4, N_IN))
    for i in range(N_IN):
        up, dn = u.copy(), u.copy()
        up[i] += h
        dn[i] -= h
        fp, fm = measures(up, ctx, gravity), measures(dn, ctx, gravity)
        fwd[:, i], bwd[:, i], cen[:, i] = (fp - f0) / h, (f0 - fm) / h, (fp - fm) / (2 * h)
    return fwd, bwd, cen


def tape_of(N, ticks):
    """random or crafted ticks (tests/walk_limits_ref.py) stacked like rows of a walk tape: X[rows, B, n_x], P[rows, B, n_p], states[rows + 1, B, 9]
    (row r + 1 = tick r's state_out; row 0 is not read by the measures)"""
    X = np.ascontiguousarray(np.stack([t["X"] for t in ticks]), np.float32)
    P = np.ascontiguousarray(np.stack([t["P"] for t in ticks]), np.float32)
    S = np.ascontiguousarray(np.stack([np.zeros_like(ticks[0]["state_out"])] + [t["state_out"] for t in ticks]), np.float32)
    return X, P, S


def host_jacobian(lib, N, X, P, S, corners, gravity):
    """cmpc_walk_measures_jacobian -> [rows, B, 4, 44]"""
    rows, B = X.shape[:2]
    c = np.ascontiguousarray(corners, np.float32)
    J = np.full((rows, B, 4, N_IN), 99.0)
    assert lib.cmpc_walk_measures_jacobian(N, B, rows, _ptr(X), _ptr(P), _ptr(S), _ptr(c), 24 if c.ndim == 4 else 0, gravity, _ptr(J)) == 0
    return J


def host_vjp(lib, N, X, P, S, end_tick, corners, gravity, gM, gS, gX, tick0=0):
    """cmpc_walk_measures_vjp on copies of the seeds -> (gS', gX', direct[rows, B, 32])"""
    rows, B = X.shape[:2]
    c = np.ascontiguousarray(corners, np.float32)
    gS, gX, direct = gS.copy(), gX.copy(), np.full((rows, B, 32), 99.0)
    assert lib.cmpc_walk_measures_vjp(N, B, tick0, rows, _ptr(X), _ptr(P), _ptr(S), _ptr(end_tick), _ptr(c), 24 if c.ndim == 4 else 0, gravity,
                                      _ptr(np.ascontiguousarray(gM)), _ptr(gS), _ptr(gX), _ptr(direct)) == 0
    return gS, gX, direct


def host_jvp(lib, N, X, P, S, end_tick, corners, gravity, dS, dX, dP=None, dModel=None, tick0=0):
    """cmpc_walk_measures_jvp -> dM[rows, B, k, 4]"""
    rows, B = X.shape[:2]
    k = dS.shape[2]
    c = np.ascontiguousarray(corners, np.float32)
    dM = np.full((rows, B, k, 4), 99.0)
    assert lib.cmpc_walk_measures_jvp(N, B, tick0, rows, k, _ptr(X), _ptr(P), _ptr(S), _ptr(end_tick), _ptr(c), 24 if c.ndim == 4 else 0, gravity,
                                      _ptr(dS), _ptr(dX), _ptr(dP), _ptr(dModel), _ptr(dM)) == 0
    return dM


def vjp_from_jacobian(N, J, gM):
    """the contraction of the dense Jacobian with the cotangents: (d states[rows, B, 5], d foot positions [rows, B, 6], direct[rows, B, 32])"""
    g = np.einsum("rbm,rbmi->rbi", gM, J)
    direct = np.concatenate([g[..., REF], g[..., OMEGA], g[..., CORNER]], -1)
    return g[..., :5], g[..., Q], direct


def random_seeds(rng, N, rows, B):
    """seeds of the reverse walk and cotangents of the measures"""
    L = cm.Layout(N)
    return (rng.standard_normal((rows, B, 4)), rng.standard_normal((rows + 1, B, 9)), rng.standard_normal((rows, B, L.nx)).astype(np.float32))


def random_dirs(rng, N, rows, B, k):
    L = cm.Layout(N)
    return (rng.standard_normal((rows + 1, B, k, 9)), rng.standard_normal((rows, B, k, L.nx)).astype(np.float32),
            rng.standard_normal((rows, B, k, L.np)).astype(np.float32), rng.standard_normal((B, k, 34)))


def random_end_tick(rng, B, rows, tick0=0):
    """end ticks that include -1 (never), tick0 (no row counts) and tick0 + rows (every row counts)"""
    e = rng.integers(-1, tick0 + rows + 1, B).astype(np.int32)
    e[:3] = [-1, tick0, tick0 + rows]
    return e


def poison_behind(X, P, S, end_tick, tick0=0):
    """NaN in the tape rows at or past each problem's end (the rows the measures must not read) -> copies"""
    X, P, S = X.copy(), P.copy(), S.copy()
    for b, e in enumerate(end_tick):
        if e >= 0:
            r = max(int(e) - tick0, 0)
            X[r:, b], P[r:, b], S[r + 1:, b] = np.nan, np.nan, np.nan
    return X, P, S
