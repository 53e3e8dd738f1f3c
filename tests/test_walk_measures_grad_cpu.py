"""The derivative of a device walk's stability measures on the CPU (include/cmpc.h, "the measures, differentiated"): the host forms
cmpc_walk_measures_jacobian / _vjp / _vjp_fold / _jvp (no GPU, no solve) against central differences of an independent float64 restatement
(tests/walk_measures_grad_ref.py: the support region as a hull), crafted cases by their analytic values, the adjoint identity, the contractions of the
dense Jacobian, the endings, the fold, the symbols and the refusals.

Bounds.  FD: worst |J - FD| / (1 + |J|) measured on these seeds 1.92e-7 at h = 1e-5 (the curvature of track and reach at that step) and 1.92e-9 at
h = 1e-6 (profiles/r18_walk_measures_grad.txt); the bound is ten times the worse, 1.92e-6, under the 1e-5 a wrong sign or vertex would need.
Contractions: 1e-12 relative -- both sides are sums in double of the same partials in another order.  The ABI rounds the six foot-position terms of
dGradX to float32, so where those enter a comparison they get half a float32 ulp each on top (2^-24 relative), and nothing else does."""
import ctypes as C
import os

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_limits_ref as wl
from tests import walk_measures_grad_ref as mg
from tests import walk_record_ref as wr
from tests.walk_measures_grad_ref import _ptr

N, G = 10, 9.80665
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BOUND = 1.92e-6
KINK = 1e-4
REL = 1e-12
HALF_ULP32 = 2.0 ** -24
L = cm.Layout(N)
FEET = np.array([L.pos[c] + 3 + i for c in range(2) for i in range(3)])


def random_tape(B, per_problem_corners=False):
    ticks, _ = wl.random_ticks(N, B, seed=B, n=2)
    X, P, S = mg.tape_of(N, ticks)
    corners = wl.CORNERS
    if per_problem_corners:
        rng = np.random.default_rng(B + 7)
        corners = (np.broadcast_to(wl.CORNERS, (B, 2, 4, 3)) + rng.uniform(-0.01, 0.01, (B, 2, 4, 3))).astype(np.float32)
    return X, P, S, corners


@pytest.mark.parametrize("B", [70, 300])
def test_jacobian_against_finite_differences(B):
    """all 44 inputs, omega through R Exp(omega); a (problem, row) whose own one-sided differences at h = 1e-6 disagree by more than 1e-4 is a kink (or
    curvature the step cannot resolve) and is left out: at most 5 % of the rows with a finite state (measured: 2 of 114 and 13 of 500)"""
    lib = cm._capi.lib()
    X, P, S, corners = random_tape(B)
    J = mg.host_jacobian(lib, N, X, P, S, corners, G)
    assert np.isfinite(J).all()
    rows = left = 0
    worst = {1e-5: 0.0, 1e-6: 0.0}
    for r in range(2):
        for b in range(B):
            u, ctx = mg.inputs(N, X[r], P[r], S[r + 1], corners, b)
            alive = np.isfinite(mg.measures(u, ctx, G))
            assert (J[r, b][~alive] == 0).all(), (r, b)       # a measure the forward reports as NaN has a zero row
            assert (J[r, b][:, 5] == 0).all()                 # dcom_z
            if not ctx["finite"]:
                continue
            assert alive[3] and alive[:3].all() == any(ctx["on"])
            rows += 1
            fwd, bwd, cen = mg.differences(u, ctx, G, 1e-6)
            if (np.abs(fwd - bwd)[alive] > KINK).any():
                left += 1
                continue
            steps = {1e-6: cen}
            if B == 70:
                steps[1e-5] = mg.differences(u, ctx, G, 1e-5)[2]
            for h, fd in steps.items():
                err = (np.abs(J[r, b] - fd) / (1 + np.abs(J[r, b])))[alive].max()
                worst[h] = max(worst[h], err)
                assert err <= FD_BOUND, (r, b, h, err)
    print(f"B={B}: {rows} rows with a finite state, {left} left out, worst {worst}")
    assert rows > 0.8 * 2 * B and left <= 0.05 * rows, (rows, left)


# ---- crafted single cases: two soles of 16 cm x 6 cm at (0, +-0.08, 0), yaw 0, each by its analytic value ----
CASES = ("edge", "vertex", "single", "empty", "sunk", "coincident", "nonfinite")


def crafted():
    """one tape row of the 7 problems of CASES -> (X, P, S, support)"""
    rng = np.random.default_rng(3)
    B = len(CASES)
    support = ["LR", "LR", "L", "", "LR", "L", "LR"]
    t = wl.stand(rng, N, wr._tick(rng, N, B, [0] * B, rng.integers(-2, N + 1, (B, 2))), support, np.zeros((B, 2)))
    for b in range(B):
        for c in range(2):
            t["X"][b, L.pos[c] + 3:L.pos[c] + 6] = [0.0, 0.08 if c == 0 else -0.08, 0.0]
        t["state_out"][b] = [0.0, 0.0, 0.7, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        t["P"][b, L.p_comref + 3:L.p_comref + 6] = [0.3, 0.4, 0.7]
    s = t["state_out"]
    s[0, :2], s[0, 3:5] = [0.04, 0.0625], [0.0, 0.125]        # edge: xi inside, nearest the left foot's outer side y = 0.11
    s[1, :2] = [0.2, 0.2]                                     # vertex: xi outside, nearest the corner (0.08, 0.11) at distance 0.15
    s[2, :2], s[2, 3:5] = [0.04, 0.0625], [0.0, 0.125]        # single: the edge case on the left foot alone, the right foot's position NaN
    t["X"][2, L.pos[1] + 3:L.pos[1] + 6] = np.nan
    s[4, :3], s[4, 3:5] = [0.04, 0.0625, -0.25], [0.5, 0.5]   # sunk: height < 0, tau = 0, xi = com_xy
    s[5, :3] = [0.0, 0.08, 0.0]                               # coincident: the CoM in the supporting foot, the reference in the CoM
    t["P"][5, L.p_comref + 3:L.p_comref + 6] = s[5, :3]
    s[6, 4] = np.nan                                          # nonfinite
    X, P, S = mg.tape_of(N, [t])
    return X, P, S, support


def test_crafted_cases_by_their_analytic_values():
    lib = cm._capi.lib()
    X, P, S, _ = crafted()
    J = mg.host_jacobian(lib, N, X, P, S, wl.CORNERS, G)[0]
    i = {k: j for j, k in enumerate(CASES)}
    assert np.isfinite(J).all()
    q = lambda c, a: 6 + 3 * c + a
    om = lambda c, a: 12 + 3 * c + a
    cn = lambda c, j, a: 18 + 12 * c + 3 * j + a
    cx, cy, qy = (np.float64(np.float32(v)) for v in (0.08, 0.03, 0.08))    # the corners and the feet's |y| as the library reads them
    com = S[1].astype(np.float64)

    def track(b):      # (com_xy - ref_xy) / |.| on com_xy, its negative on ref_xy
        d = com[b, :2] - P[0, b, L.p_comref + 3:L.p_comref + 5].astype(np.float64)
        d = d / np.linalg.norm(d)
        return {0: d[0], 1: d[1], 42: -d[0], 43: -d[1]}

    def expect(b, rows):
        want = np.zeros((4, 44))
        for m, entries in rows.items():
            for k, v in entries.items():
                want[m, k] = v
        np.testing.assert_allclose(J[b], want, rtol=0, atol=1e-12, err_msg=CASES[b])
        return want

    # edge: margin = 0.11 - xi_y; xi_x = 0.04 splits the side's two corners 3 : 1, and turns with the foot about its centre
    for name, feet in (("edge", (0, 1)), ("single", (0,))):
        b = i[name]
        tau = np.sqrt(com[b, 2] / G)
        dtau = 1.0 / (2 * G * tau)
        dcy = com[b, 4]
        w0 = (com[b, 0] + cx) / (2 * cx)
        reach_foot = 0 if name == "single" else 1      # the right foot is the farther one
        d = com[b, :3] - np.array([0.0, qy if reach_foot == 0 else -qy, 0.0])
        u = d / np.linalg.norm(d)
        want = expect(b, {0: {2: 1.0, **{q(c, 2): -1.0 / len(feet) for c in feet}},
                          1: {0: u[0], 1: u[1], 2: u[2], q(reach_foot, 0): -u[0], q(reach_foot, 1): -u[1], q(reach_foot, 2): -u[2]},
                          2: {1: -1.0, 4: -tau, 2: -dcy * dtau, **{q(c, 2): dcy * dtau / len(feet) for c in feet}, q(0, 1): 1.0,
                              cn(0, 0, 1): w0, cn(0, 3, 1): 1 - w0, om(0, 2): w0 * cx - (1 - w0) * cx},
                          3: track(b)})
        if name == "single":      # the foot outside the support set receives exactly zero, whatever its position holds
            assert (J[b][:, 9:12] == 0).all() and (J[b][:, 15:18] == 0).all() and (J[b][:, 30:42] == 0).all() and want[2, q(1, 2)] == 0
    # vertex: margin = -|xi - v|, v = (0.08, 0.11) the left foot's corner 0; the unit vector (0.8, 0.6) -- in float32 corners to rounding
    b = i["vertex"]
    v = np.array([cx, qy + cy])
    n = (com[b, :2] - v) / np.linalg.norm(com[b, :2] - v)
    tau = np.sqrt(com[b, 2] / G)
    d = com[b, :3] - np.array([0.0, -qy, 0.0])      # the right foot is the farther one
    u = d / np.linalg.norm(d)
    expect(b, {0: {2: 1.0, q(0, 2): -0.5, q(1, 2): -0.5},
               1: {0: u[0], 1: u[1], 2: u[2], q(1, 0): -u[0], q(1, 1): -u[1], q(1, 2): -u[2]},
               2: {0: -n[0], 1: -n[1], 3: -n[0] * tau, 4: -n[1] * tau, q(0, 0): n[0], q(0, 1): n[1], cn(0, 0, 0): n[0], cn(0, 0, 1): n[1],
                   om(0, 2): n[1] * cx - n[0] * cy},
               3: track(b)})
    assert abs(n[0] - 0.8) < 1e-6 and abs(n[1] - 0.6) < 1e-6
    # empty support: rows 0..2 zero, track alive
    b = i["empty"]
    expect(b, {3: track(b)})
    # sunk (height <= 0): tau = 0, so the margin sees neither dcom nor, through tau, the heights
    b = i["sunk"]
    # (xi = (0.04, 0.0625) is nearest the front side x = 0.08)
    assert (J[b, 2, [2, 3, 4, q(0, 2), q(1, 2)]] == 0).all() and J[b, 2, 0] == -1.0 and J[b, 2, 1] == 0 and J[b, 0, 2] == 1.0
    # coincident (track == 0 and r == 0): zeros, not NaN
    b = i["coincident"]
    assert (J[b, 1] == 0).all() and (J[b, 3] == 0).all() and J[b, 0, 2] == 1.0 and J[b, 0, q(0, 2)] == -1.0
    # a state that is not finite: all zero
    assert (J[i["nonfinite"]] == 0).all()


def _dense_direction(dS, dX, dP, dModel):
    """the 44-vector of every (row, problem, column) from the JVP's direction arrays"""
    rows, B, k = dX.shape[:3]
    v = np.zeros((rows, B, k, 44))
    v[..., :5] = dS[1:, :, :, :5]
    v[..., mg.Q] = dX[..., FEET].astype(np.float64)
    v[..., mg.CORNER] = dModel[None, :, :, 10:34]
    v[..., mg.REF] = dP[..., L.p_comref + 3:L.p_comref + 5].astype(np.float64)
    return v


@pytest.mark.parametrize("per_problem", [False, True])
def test_vjp_and_jvp_against_the_dense_jacobian_and_each_other(per_problem):
    lib = cm._capi.lib()
    B, k = 70, 3
    X, P, S, corners = random_tape(B, per_problem)
    rng = np.random.default_rng(11)
    J = mg.host_jacobian(lib, N, X, P, S, corners, G)
    gM, _, _ = mg.random_seeds(rng, N, 2, B)
    zS, zX = np.zeros((3, B, 9)), np.zeros((2, B, L.nx), np.float32)
    gS, gX, direct = mg.host_vjp(lib, N, X, P, S, None, corners, G, gM, zS, zX)
    wS, wq, wdirect = mg.vjp_from_jacobian(N, J, gM)
    # (relative to the size of the TERMS: an entry of J -- the omega of a foot, say -- may be a sum of terms of order one that cancel)
    mag = np.einsum("rbm,rbmi->rbi", np.abs(gM), np.abs(J)) + np.abs(gM).sum(-1)[..., None]
    np.testing.assert_array_less(np.abs(gS[1:, :, :5] - wS), REL * mag[..., :5] + 1e-300)
    np.testing.assert_array_less(np.abs(direct - wdirect), REL * np.concatenate([mag[..., mg.REF], mag[..., mg.OMEGA], mag[..., mg.CORNER]], -1) + 1e-300)
    # (the foot positions leave the ABI as float32: the double sum rounded once)
    np.testing.assert_array_less(np.abs(gX[..., FEET].astype(np.float64) - wq), (REL + HALF_ULP32) * mag[..., mg.Q] + 1e-300)
    assert (gS[0] == 0).all() and (gS[..., 5:] == 0).all() and (np.delete(gX, FEET, -1) == 0).all()
    # the JVP against J v
    dS, dX, dP, dModel = mg.random_dirs(rng, N, 2, B, k)
    dM = mg.host_jvp(lib, N, X, P, S, None, corners, G, dS, dX, dP, dModel)
    v = _dense_direction(dS, dX, dP, dModel)
    want = np.einsum("rbmi,rbki->rbkm", J, v)
    np.testing.assert_array_less(np.abs(dM - want), REL * np.einsum("rbmi,rbki->rbkm", np.abs(J), np.abs(v)) + 1e-300)
    # without the optional directions: their entries read as zero
    dM0 = mg.host_jvp(lib, N, X, P, S, None, corners, G, dS, dX)
    v0 = _dense_direction(dS, dX, np.zeros_like(dP), np.zeros_like(dModel))
    np.testing.assert_array_less(np.abs(dM0 - np.einsum("rbmi,rbki->rbkm", J, v0)), REL * np.einsum("rbmi,rbki->rbkm", np.abs(J), np.abs(v0)) + 1e-300)
    # the adjoint identity per problem and column: <w, JVP v> = <VJP w, v>
    lhs = np.einsum("rbm,rbkm->bk", gM, dM)
    parts = [np.einsum("rbi,rbki->bk", gS[1:, :, :5], dS[1:, :, :, :5]), np.einsum("rbi,rbki->bk", direct[..., :2], v[..., mg.REF]),
             np.einsum("rbi,rbki->bk", direct[..., 8:], v[..., mg.CORNER])]
    foot = np.einsum("rbi,rbki->bk", gX[..., FEET].astype(np.float64), v[..., mg.Q])
    scale = np.einsum("rbm,rbmi,rbki->bk", np.abs(gM), np.abs(J), np.abs(v))
    foot_scale = np.einsum("rbi,rbki->bk", mag[..., mg.Q], np.abs(v[..., mg.Q]))
    assert (np.abs(lhs - (sum(parts) + foot)) <= REL * scale + HALF_ULP32 * foot_scale).all()
    # ... and with no direction on the foot positions, so that nothing float32 enters: plain 1e-12
    dX0 = dX.copy()
    dX0[..., FEET] = 0
    dM1 = mg.host_jvp(lib, N, X, P, S, None, corners, G, dS, dX0, dP, dModel)
    lhs1 = np.einsum("rbm,rbkm->bk", gM, dM1)
    assert (np.abs(lhs1 - sum(parts)) <= REL * scale).all() and (np.abs(lhs1) > 0.01).mean() > 0.7


def test_endings_select_zero_and_read_nothing():
    """random end ticks that include never, tick0 and tick0 + rows; NaN in the tape rows and in the seeds at or past each problem's end"""
    lib = cm._capi.lib()
    B, k, tick0 = 70, 2, 3
    X, P, S, corners = random_tape(B, True)
    rng = np.random.default_rng(12)
    e = mg.random_end_tick(rng, B, 2, tick0)
    counted = np.array([[(e[b] < 0) or (tick0 + r < e[b]) for b in range(B)] for r in range(2)])      # row e itself is excluded
    assert counted[:, 0].all() and not counted[:, 1].any() and counted[:, 2].all() and len(set(counted.sum(0))) == 3
    gM, gS0, gX0 = mg.random_seeds(rng, N, 2, B)
    free = mg.host_vjp(lib, N, X, P, S, None, corners, G, gM, gS0, gX0, tick0)
    Xn, Pn, Sn = mg.poison_behind(X, P, S, e, tick0)
    gMn, gSn, gXn = gM.copy(), gS0.copy(), gX0.copy()
    gMn[~counted], gXn[~counted] = np.nan, np.nan
    gSn[1:][~counted] = np.nan
    gS, gX, direct = mg.host_vjp(lib, N, Xn, Pn, Sn, e, corners, G, gMn, gSn, gXn, tick0)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)
    assert (direct[~counted] == 0).all()
    np.testing.assert_array_equal(bits(gS[1:][~counted]), bits(gSn[1:][~counted]))      # the += entries of a row that does not count: unwritten
    np.testing.assert_array_equal(bits(gX[~counted]), bits(gXn[~counted]))
    for got, want in zip((gS[1:][counted], gX[counted], direct[counted]), (free[0][1:][counted], free[1][counted], free[2][counted])):
        np.testing.assert_array_equal(bits(got), bits(want))                              # a row that counts: the call without endings, to the bit
    np.testing.assert_array_equal(bits(gS[0]), bits(gSn[0]))
    np.testing.assert_array_equal(bits(gS[..., 5:]), bits(gSn[..., 5:]))                   # states 5..8 and everything of x but the feet: untouched
    np.testing.assert_array_equal(bits(np.delete(gX, FEET, -1)), bits(np.delete(gXn, FEET, -1)))
    assert np.abs(gS[1:][counted][:, :5] - gS0[1:][counted][:, :5]).max() > 0
    # the JVP: zero rows behind the end, whatever the directions and the tape hold there
    dS, dX, dP, dModel = mg.random_dirs(rng, N, 2, B, k)
    freeM = mg.host_jvp(lib, N, X, P, S, None, corners, G, dS, dX, dP, dModel, tick0)
    dSn, dXn, dPn = dS.copy(), dX.copy(), dP.copy()
    dSn[1:][~counted], dXn[~counted], dPn[~counted] = np.nan, np.nan, np.nan
    dM = mg.host_jvp(lib, N, Xn, Pn, Sn, e, corners, G, dSn, dXn, dPn, dModel, tick0)
    assert (dM[~counted] == 0).all()
    np.testing.assert_array_equal(bits(dM[counted]), bits(freeM[counted]))


def test_fold():
    lib = cm._capi.lib()
    rows, B = 5, 9
    rng = np.random.default_rng(13)
    direct = rng.standard_normal((rows, B, 32))
    direct[2] = 0.0
    gP0, gM0 = rng.standard_normal((rows, B, L.np)).astype(np.float32), rng.standard_normal((B, 34))
    gP0[2, :, L.p_comref + 3] = -0.0      # a zero term is not added: the entry keeps its bits
    gP, gM = gP0.copy(), gM0.copy()
    assert lib.cmpc_walk_measures_vjp_fold(N, B, rows, _ptr(direct), _ptr(gP), _ptr(gM)) == 0
    want = gP0.copy()
    want[..., L.p_comref + 3:L.p_comref + 5] += direct[..., :2].astype(np.float32)
    want[2] = gP0[2]
    np.testing.assert_array_equal(gP.view(np.uint32), want.view(np.uint32))
    assert (gP != gP0).sum() == 2 * (rows - 1) * B                                     # two words of grad_P per row and problem
    wm = gM0.copy()
    for b in range(B):
        for wd in range(24):
            s = 0.0
            for r in range(rows):                                                      # ascending rows, in float64
                s = s + direct[r, b, 8 + wd]
            wm[b, 10 + wd] = wm[b, 10 + wd] + s
    np.testing.assert_array_equal(gM.view(np.uint64), wm.view(np.uint64))
    # either output may be NULL
    gP2, gM2 = gP0.copy(), gM0.copy()
    assert lib.cmpc_walk_measures_vjp_fold(N, B, rows, _ptr(direct), _ptr(gP2), None) == 0
    assert lib.cmpc_walk_measures_vjp_fold(N, B, rows, _ptr(direct), None, _ptr(gM2)) == 0
    np.testing.assert_array_equal(gP2.view(np.uint32), gP.view(np.uint32))
    np.testing.assert_array_equal(gM2.view(np.uint64), gM.view(np.uint64))


def test_symbols_and_refusals():
    lib = cm._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    for name in ("cmpc_walk_measures_vjp_device", "cmpc_walk_measures_vjp_fold_device", "cmpc_walk_measures_jvp_device", "cmpc_walk_measures_vjp",
                 "cmpc_walk_measures_vjp_fold", "cmpc_walk_measures_jvp", "cmpc_walk_measures_jacobian"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and "int " + name + "(" in hdr, name
    assert "#define CMPC_WALK_MEASURE_INPUTS 44" in hdr and "#define CMPC_WALK_MEASURE_DIRECT 32" in hdr
    assert cm._capi.WALK_MEASURE_INPUTS == 44 and cm._capi.WALK_MEASURE_DIRECT == 32
    assert C.sizeof(cm._capi.CmpcWalkMeasureGrads) == 32 and C.sizeof(cm._capi.CmpcWalkMeasureDirs) == 40
    assert "derivatives\n * of the measures" not in hdr and "derivatives of the measures. */" not in hdr
    B = 4
    X, P, S, corners = random_tape(B)
    c = np.ascontiguousarray(corners, np.float32)
    rng = np.random.default_rng(14)
    gM, gS, gX = mg.random_seeds(rng, N, 2, B)
    direct, J, dM = np.zeros((2, B, 32)), np.zeros((2, B, 4, 44)), np.zeros((2, B, 1, 4))
    dS, dX, _, _ = mg.random_dirs(rng, N, 2, B, 1)

    def vjp(horizon=N, rows=2, x=X, corners_ptr=_ptr(c), gravity=G, seeds=_ptr(gM), out=_ptr(direct)):
        return lib.cmpc_walk_measures_vjp(horizon, B, 0, rows, _ptr(x), _ptr(P), _ptr(S), None, corners_ptr, 0, gravity, seeds, _ptr(gS), _ptr(gX), out)

    def jvp(horizon=N, rows=2, k=1, dirs=_ptr(dS), out=_ptr(dM)):
        return lib.cmpc_walk_measures_jvp(horizon, B, 0, rows, k, _ptr(X), _ptr(P), _ptr(S), None, _ptr(c), 0, G, dirs, _ptr(dX), None, None, out)
    assert vjp() == 0 and jvp() == 0
    assert vjp(horizon=1) != 0 and vjp(rows=0) != 0 and vjp(x=None) != 0 and vjp(corners_ptr=None) != 0 and vjp(gravity=0.0) != 0
    assert vjp(seeds=None) != 0 and vjp(out=None) != 0
    assert jvp(horizon=1) != 0 and jvp(rows=0) != 0 and jvp(k=0) != 0 and jvp(dirs=None) != 0 and jvp(out=None) != 0
    assert lib.cmpc_walk_measures_jacobian(1, B, 2, _ptr(X), _ptr(P), _ptr(S), _ptr(c), 0, G, _ptr(J)) != 0
    assert lib.cmpc_walk_measures_jacobian(N, B, 2, _ptr(X), _ptr(P), _ptr(S), _ptr(c), 0, G, None) != 0
    assert lib.cmpc_walk_measures_vjp_fold(N, B, 2, None, None, None) != 0 and lib.cmpc_walk_measures_vjp_fold(1, B, 2, _ptr(direct), None, None) != 0
    # the device forms refuse a NULL handle before anything else
    assert lib.cmpc_walk_measures_vjp_device(None, 0, 1, None, 0, None, None, None) != 0
    assert lib.cmpc_walk_measures_vjp_fold_device(None, 1, None, None, None, None) != 0
    assert lib.cmpc_walk_measures_jvp_device(None, 0, 1, None, 0, None, 1, None, None) != 0
