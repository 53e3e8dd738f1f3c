"""The planner's reference trajectories differentiated, on the CPU (include/cmpc.h: cmpc_reference_from_planner_vjp / _jvp, the host forms, which need no
handle and no GPU): the VJP against the float64 restatement of tests/reference_grad_ref.py under a derived bound, both clamps, both kinds of height, ended
problems and NaN in everything the rule excludes; segments against one call, to the bit; the JVP against the forward's expression, to the bit; the two
against each other; the argument errors and the Python surface.  N = 10, dt = 0.06."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cmpc_amd as cm
from oracle import plant_ref
from tests import reference_grad_ref as rg

N, DT, MASS, TICK0 = 10, 0.06, 56.0, 3
L = cm.Layout(N)
NAN = float("nan")
# never ended, ended before the rows (0, tick0), inside them, at their end and behind it
END = np.array([-1, 0, 3, 4, 5, 7, 8, 20, -1], np.int32)
B = len(END)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _refs(knots, in_dt, t_first, height, mass=MASS):
    return cm._capi.CmpcPlannerRefs(knots, in_dt, t_first, mass, height)


def _case(knots, in_dt, height, rows, seed=0):
    """t_first = 0.25: tick 3 runs at 0.18, so its first knots fall before the first planner knot (the low clamp); 7 knots end 0.12 s (in_dt 0.02) or
    0.3 s (0.05) behind t_first, inside every horizon of 0.6 s (the high clamp); 70 knots of 0.05 s outlast the last horizon"""
    rng = np.random.default_rng(1000 * knots + int(1000 * in_dt) + rows + seed)
    g = rng.normal(size=(rows, B, L.np)).astype(np.float32)
    start = rng.normal(size=(2, B, knots, 3))
    return rng, g, start, 0.25


def _poison(g, end, height, rows, tick0=TICK0):
    """NaN in every row the rule excludes, in every entry outside the reference rows and, with a fixed height, in the z entries of comRef"""
    g = g.copy()
    keep = np.zeros(L.np, bool)
    keep[L.p_comref:L.p_href + 3 * (N + 1)] = True
    g[:, :, ~keep] = np.nan
    if height == height:
        g[:, :, L.p_comref + 2:L.p_href:3] = np.nan
    for b in range(g.shape[1]):
        g[rg.admitted_rows(end, b, tick0, rows):, b] = np.nan
    return g


def _host_vjp(rows, pl, end, g, gc, gh, tick0=TICK0, batch=B):
    return cm._capi.lib().cmpc_reference_from_planner_vjp(N, DT, batch, tick0, rows, C.byref(pl) if pl is not None else None, _ptr(end), _ptr(g), _ptr(gc), _ptr(gh))


def _host_jvp(rows, k, pl, dc, dh, dp, tick0=TICK0, batch=B):
    return cm._capi.lib().cmpc_reference_from_planner_jvp(N, DT, batch, tick0, rows, k, C.byref(pl) if pl is not None else None, _ptr(dc), _ptr(dh), _ptr(dp))


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("height", [0.7, NAN], ids=["height", "free_z"])
@pytest.mark.parametrize("knots", [7, 70])
@pytest.mark.parametrize("in_dt", [0.02, 0.05])
def test_host_vjp_against_the_restatement(in_dt, knots, height, rows):
    """|got - want| <= 4 (m + 2) 2^-53 sum |w g| per entry, m the number of terms: the inputs are exact in double, a weight can differ from the
    restatement's by an ulp of its division (and for h of the division by the mass), and a sum of m terms adds m roundings -- derived, not measured"""
    rng, g, start, t_first = _case(knots, in_dt, height, rows)
    gp = _poison(g, END, height, rows)
    gc, gh = start[0].copy(), start[1].copy()
    assert _host_vjp(rows, _refs(knots, in_dt, t_first, height), END, gp, gc, gh) == 0
    assert np.isfinite(gc).all() and np.isfinite(gh).all()
    wc, wh, mc, mh, nc, nh = rg.vjp(L, DT, TICK0, rows, knots, in_dt, t_first, MASS, height, END, gp, start[0], start[1])
    for got, want, mag, m, name in ((gc, wc, mc, nc, "com"), (gh, wh, mh, nh, "h")):
        gap = np.abs(got - want)
        bound = 4 * (m + 2) * 2.0 ** -53 * mag
        print(f"{name}: worst gap / bound {np.max(gap / np.maximum(bound, 1e-300)):.3f}, entries with terms {(m > 1).sum()} of {m.size}")
        assert (gap <= bound).all(), name
    for b in range(B):      # a problem without an admitted row keeps its start value to the bit
        if rg.admitted_rows(END, b, TICK0, rows) == 0:
            assert (gc[b] == start[0][b]).all() and (gh[b] == start[1][b]).all()
    assert np.abs(gc - start[0]).max() > 0 and np.abs(gh - start[1]).max() > 0
    if height == height:
        assert (gc[..., 2] == start[0][..., 2]).all()
    else:
        assert np.abs(gc[..., 2] - start[0][..., 2]).max() > 0
    # both clamps are on the path: an MPC knot before the first planner knot, and (7 knots) one behind the last
    s = (rg.t_offset(TICK0, DT, t_first) + np.arange(N + 1) * DT) / in_dt
    assert s[0] < 0 and (knots == 70 or s[-1] > knots - 1)
    # one output alone
    only = start[0].copy()
    assert _host_vjp(rows, _refs(knots, in_dt, t_first, height), END, gp, only, None) == 0 and (only.view(np.int64) == gc.view(np.int64)).all()
    only = start[1].copy()
    assert _host_vjp(rows, _refs(knots, in_dt, t_first, height), END, gp, None, only) == 0 and (only.view(np.int64) == gh.view(np.int64)).all()


@pytest.mark.parametrize("height", [0.7, NAN], ids=["height", "free_z"])
def test_segments_compose_to_the_bit(height):
    """rows 0 .. 2 then 3 .. 4 into the same buffers equal one call over 0 .. 4; the start value is added to, not overwritten"""
    knots, in_dt, rows = 70, 0.05, 5
    rng, g, start, t_first = _case(knots, in_dt, height, rows, seed=7)
    gp = _poison(g, END, height, rows)
    pl = _refs(knots, in_dt, t_first, height)
    one = [start[0].copy(), start[1].copy()]
    assert _host_vjp(rows, pl, END, gp, one[0], one[1]) == 0
    two = [start[0].copy(), start[1].copy()]
    assert _host_vjp(3, pl, END, gp, two[0], two[1]) == 0
    assert _host_vjp(2, pl, END, np.ascontiguousarray(gp[3:]), two[0], two[1], tick0=TICK0 + 3) == 0
    for a, b in zip(one, two):
        assert (a.view(np.int64) == b.view(np.int64)).all()
    zero = [np.zeros_like(start[0]), np.zeros_like(start[1])]
    assert _host_vjp(rows, pl, END, gp, zero[0], zero[1]) == 0
    for q in range(2):      # the start value is in the sum: got - (sum from zero) is the start value up to the sum's own rounding
        np.testing.assert_allclose(one[q] - zero[q], start[q], rtol=0, atol=1e-12)
        assert np.abs(one[q] - zero[q]).max() > 0.1


@pytest.mark.parametrize("height", [0.7, NAN], ids=["height", "free_z"])
@pytest.mark.parametrize("knots,in_dt", [(7, 0.02), (70, 0.05)])
def test_host_jvp_is_the_forward_expression(knots, in_dt, height):
    """float32-valued directions: every written entry is, to the bit, the forward's expression on the direction -- (float)((1 - w) d0 + w d1), for h divided
    by the mass, in double (oracle/plant_ref.resample_references on the column, rounded to float32; the handle-bound forward itself,
    cmpc_set_reference_from_planner, is compared in tests/test_gpu_reference_grad.py) -- except the z row of comRef under a fixed height: +0.0f.  Every
    entry outside the 6 (N + 1) reference rows keeps its NaN sentinel."""
    rows, k, t_first = 3, 2, 0.25
    rng = np.random.default_rng(knots)
    dc = rng.normal(size=(B, k, knots, 3)).astype(np.float32).astype(np.float64)
    dh = rng.normal(size=(B, k, knots, 3)).astype(np.float32).astype(np.float64)
    dp = np.full((rows, B, k, L.np), np.nan, np.float32)
    assert _host_jvp(rows, k, _refs(knots, in_dt, t_first, height), dc, dh, dp) == 0
    inside = np.zeros(L.np, bool)
    inside[L.p_comref:L.p_href + 3 * (N + 1)] = True
    assert np.isnan(dp[..., ~inside]).all() and np.isfinite(dp[..., inside]).all()
    for r in range(rows):
        for b in range(B):
            for j in range(k):
                cr, hr = plant_ref.resample_references(dc[b, j], dh[b, j], in_dt, rg.t_offset(TICK0 + r, DT, t_first), N, DT, MASS, NAN)
                got_c, got_h = rg.reference_rows(L, dp[r, b, j])
                want_c = cr.astype(np.float32)
                if height == height:
                    want_c[:, 2] = 0.0
                assert (got_c.view(np.int32) == want_c.view(np.int32)).all() and (got_h.view(np.int32) == hr.astype(np.float32).view(np.int32)).all()
    # one direction alone: the other's rows are written as +0.0f
    dp1 = np.full_like(dp, np.nan)
    assert _host_jvp(rows, k, _refs(knots, in_dt, t_first, height), dc, None, dp1) == 0
    n3 = 3 * (N + 1)
    assert (dp1[..., L.p_comref:L.p_comref + n3].view(np.int32) == dp[..., L.p_comref:L.p_comref + n3].view(np.int32)).all()
    assert (dp1[..., L.p_href:L.p_href + n3].view(np.int32) == 0).all() and np.isnan(dp1[..., ~inside]).all()


@pytest.mark.parametrize("height", [0.7, NAN], ids=["height", "free_z"])
def test_host_forms_are_adjoint(height):
    """<g, J d> against <J^T g, d> per problem, nobody ended: the gap is at most 2^-23 sum |g . Jd|, the float32 rounding of the JVP's output (the VJP's
    own double rounding is nine orders below it)"""
    knots, in_dt, rows, t_first = 70, 0.05, 5, 0.25
    rng = np.random.default_rng(5)
    g = rng.normal(size=(rows, B, L.np)).astype(np.float32)
    dc, dh = rng.normal(size=(B, 1, knots, 3)), rng.normal(size=(B, 1, knots, 3))
    pl = _refs(knots, in_dt, t_first, height)
    dp = np.zeros((rows, B, 1, L.np), np.float32)
    assert _host_jvp(rows, 1, pl, dc, dh, dp) == 0
    gc, gh = np.zeros((B, knots, 3)), np.zeros((B, knots, 3))
    assert _host_vjp(rows, pl, None, g, gc, gh) == 0
    for b in range(B):
        prod = g[:, b].astype(np.float64) * dp[:, b, 0].astype(np.float64)
        lhs, rhs = prod.sum(), (gc[b] * dc[b, 0]).sum() + (gh[b] * dh[b, 0]).sum()
        bound = 2.0 ** -23 * np.abs(prod).sum()
        print(f"problem {b}: <g, J d> {lhs:.12e}  <J^T g, d> {rhs:.12e}  gap {abs(lhs - rhs):.2e}  bound {bound:.2e}")
        assert lhs != 0.0 and abs(lhs - rhs) <= bound


def test_argument_errors():
    knots, rows, k = 7, 2, 2
    g = np.zeros((rows, B, L.np), np.float32)
    gc, gh = np.zeros((B, knots, 3)), np.zeros((B, knots, 3))
    dc, dh, dp = np.zeros((B, k, knots, 3)), np.zeros((B, k, knots, 3)), np.zeros((rows, B, k, L.np), np.float32)
    good = lambda **kw: _refs(**{**dict(knots=knots, in_dt=0.02, t_first=0.0, height=0.7), **kw})
    assert _host_vjp(rows, good(), None, g, gc, gh) == 0 and _host_jvp(rows, k, good(), dc, dh, dp) == 0
    bad = [good(knots=1), good(in_dt=0.0), good(in_dt=-0.02), good(in_dt=NAN), good(in_dt=float("inf")), good(mass=0.0), good(mass=NAN),
           good(mass=float("inf")), None]
    for pl in bad:
        assert _host_vjp(rows, pl, None, g, gc, gh) == -1
        assert _host_jvp(rows, k, pl, dc, dh, dp) == -1
    assert _host_vjp(0, good(), None, g, gc, gh) == -1 and _host_vjp(rows, good(), None, g, gc, gh, tick0=-1) == -1
    assert _host_vjp(rows, good(), None, None, gc, gh) == -1 and _host_vjp(rows, good(), None, g, None, None) == -1
    assert _host_jvp(0, k, good(), dc, dh, dp) == -1 and _host_jvp(rows, k, good(), dc, dh, dp, tick0=-1) == -1 and _host_jvp(rows, 0, good(), dc, dh, dp) == -1
    assert _host_jvp(rows, k, good(), dc, dh, None) == -1 and _host_jvp(rows, k, good(), None, None, dp) == -1
    # the device forms refuse a NULL handle before anything touches a GPU
    lib = cm._capi.lib()
    pl = good()
    assert lib.cmpc_reference_from_planner_vjp_device(None, 0, rows, C.byref(pl), None, _ptr(g), _ptr(gc), _ptr(gh), None) == -1
    assert lib.cmpc_reference_from_planner_jvp_device(None, 0, rows, k, C.byref(pl), _ptr(dc), _ptr(dh), _ptr(dp), None) == -1


def test_exports_struct_size_and_python_surface():
    lib = cm._capi.lib()
    for name in ("cmpc_reference_from_planner_vjp", "cmpc_reference_from_planner_vjp_device", "cmpc_reference_from_planner_jvp",
                 "cmpc_reference_from_planner_jvp_device"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(cm._capi.CmpcPlannerRefs) == 8 + 4 * 8      # (LP64: the int padded to 8, four doubles)
    ro = cm.rollout.WalkingRollout
    for name in ("set_references", "backward_device_refs", "forward_sensitivity_device_refs"):
        assert hasattr(ro, name), name
    for name in ("reference_from_planner_vjp_device", "reference_from_planner_jvp_device"):
        assert hasattr(cm.BatchSolver, name), name
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.set_references)[:7] == ["self", "com", "h", "in_dt", "t_first", "robot_mass", "com_height"]
    assert par(ro.backward_device_refs) == ["self", "w", "grad_states", "grad_X", "rot"]
    assert par(ro.forward_sensitivity_device_refs)[:4] == ["self", "w", "dir_ref_com", "dir_ref_h"]
    # the pinned signatures are unchanged
    assert par(ro.backward_device) == ["self", "w", "grad_states", "grad_X"] == par(ro.backward_device_rot)
    assert par(ro.forward_sensitivity_device) == ["self", "w", "dir_state0", "dir_list0", "dir_list_rot0", "dir_plan", "dir_plan_rot", "dir_push", "dir_models",
                                                  "dir_wrench", "solutions"]
    assert par(ro.forward_sensitivity)[2:] == par(ro.forward_sensitivity_device)[2:]
    assert par(ro.walk_device) == ["self", "ticks", "com0", "dcom0", "h0", "push", "push_ticks", "replan", "trace", "stop", "skip_ended"]
    assert par(cm.rollout_differentiable)[-2:] == ["ref_com", "ref_h"] and par(cm.rollout_differentiable)[:10] == [
        "rollout", "ticks", "state0", "push", "models", "push_ticks", "plan_yaw", "device_walk", "replan", "plan_rot"]
    with pytest.raises(NotImplementedError):      # only on the device walk, and refused before anything touches a GPU
        cm.rollout_differentiable(None, 1, None, ref_com=object())
    assert "backward_device_refs" in ro.backward.__doc__ and "CoM references are not differentiated" not in ro.backward.__doc__
