"""The physical limits of a device walk on the CPU: the host form cmpc_rollout_record_limits (no GPU, no solve) against its numpy restatement
(tests/walk_limits_ref.py: the support region as a hull, the chain of tests/walk_record_ref.py in front) on ticks made by hand at N = 10, B = 12 --
double and single support, no support, point feet (a segment, a point), a capture point inside the region, outside nearest an edge and outside nearest a
vertex, a non-finite state, a solver status in front of violated limits, several limits violated at once; with and without the limits bit, with
every limit off, and with no limits at all (cmpc_rollout_record to the bit); the refusals and the symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_limits_ref as wl
from tests import walk_record_ref as wr
from tests.test_walk_record_cpu import _ptr, box, host_record, host_record_arrays

N, B, G = 10, 12, 9.80665
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = dict(height_min=0.6, height_max=0.8, reach_max=0.78, margin_min=-0.15, track_max=0.12)
NAMES = ("double", "single", "none", "segment", "point", "inside", "edge", "vertex", "nonfinite", "status", "several", "plain")


def crafted():
    """two ticks of the 12 problems of NAMES, the per-problem corners [B, 2, 4, 3] (zero for the point feet), and the outcome they start from"""
    rng = np.random.default_rng(5)
    support = ["LR", "L", "", "LR", "R", "LR", "LR", "LR", "LR", "LR", "LR", "R"]
    yaw = rng.uniform(-0.5, 0.5, (B, 2))
    yaw[5:8] = 0.0
    corners = np.broadcast_to(wl.CORNERS, (B, 2, 4, 3)).copy()
    corners[3] = 0.0        # point feet in double support: a segment
    corners[4, 1] = 0.0     # the supporting foot's corners all zero: a point
    ticks = []
    for i in range(2):
        t = wl.stand(rng, N, wr._tick(rng, N, B, [0] * B, rng.integers(-2, N + 1, (B, 2))), support, yaw)
        s = t["state_out"]
        s[5, :2], s[5, 3:5] = [0.0, 0.0], [0.0, 0.0]          # the capture point at the middle of the two feet
        s[6, :2], s[6, 3:5] = [0.0, 0.0], [1.2, 0.0]          # ... thrown forward: in front of the toes' edge
        s[7, :2], s[7, 3:5] = [0.0, 0.0], [1.2, 1.6]          # ... and forward-left: beyond the left foot's front corner
        s[8, 7] = np.inf                                      # code 5: every measure NaN, no limit code with bit 2 off
        t["info"][9, 5] = 2                                   # solver status 2 (code 3) on a robot that has sunk
        s[9, 2] = 0.3
        s[10, :3] = [0.4, 0.0, 0.95]                          # too high, too far from its feet and from its reference at once: code 6 wins
        ticks.append(t)
    ticks[1]["state_out"][0, 2] = 0.45                        # tick 1: the double-support robot sinks (6), the single-support one drifts off (7),
    ticks[1]["state_out"][1, 0] = 0.5                         # ... whose reference goes with it so that track stays inside
    ticks[1]["P"][1, cm.Layout(N).p_comref + 3] = 0.5
    ticks[1]["P"][11, cm.Layout(N).p_comref + 3:cm.Layout(N).p_comref + 5] += 0.3     # the plain one loses its reference (9)
    return ticks, corners, wr.new_outcome(rng.uniform(-1, 1, (B, 9)).astype(np.float32))


def limits_struct(lim, measures=None, extremes=None):
    """the cmpc_walk_limits of a dict like wl.OFF and two host arrays (or None)"""
    return cm._capi.CmpcWalkLimits(lim["height_min"], lim["height_max"], lim["reach_max"], lim["margin_min"], lim["track_max"],
                                   _ptr(measures) if measures is not None else None, 0 if measures is None else measures.shape[0],
                                   _ptr(extremes) if extremes is not None else None)


def host_record_limits(lib, N, ticks, arrays, box_upper, box_lower, lim, corners, gravity=G, tick0=11):
    """cmpc_rollout_record_limits tick by tick; arrays gains measures [T, B, 4] (filled with 99 first) and extremes [B, 5] (at their start)"""
    Bt = ticks[0]["X"].shape[0]
    arrays["measures"] = np.full((len(ticks), Bt, 4), 99, np.float32)
    arrays["extremes"] = wl.new_extremes(Bt)
    c = np.ascontiguousarray(corners, np.float32)
    stride = 24 if c.ndim == 4 else 0
    ls = limits_struct(lim, arrays["measures"], arrays["extremes"])
    for i, t in enumerate(ticks):
        rc = lib.cmpc_rollout_record_limits(N, Bt, tick0 + i, i, _ptr(t["X"]), _ptr(t["P"]), _ptr(t["info"]), _ptr(t["ok"]), _ptr(t["land"]),
                                            _ptr(t["state_out"]), _ptr(t["zmp"]), _ptr(box_upper), _ptr(box_lower), C.byref(arrays["_c"]), C.byref(ls),
                                            _ptr(c), stride, gravity)
        assert rc == 0


def assert_limits_match(got, rows, ext):
    """the measures rows within 1e-6 of the restatement's (NaN where it has NaN), the extremes exactly those of the library's own measures"""
    want = np.stack([r["measures"] for r in rows])
    np.testing.assert_array_equal(np.isnan(got["measures"]), np.isnan(want))
    np.testing.assert_allclose(got["measures"][~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=1e-6)
    if ext is not None:
        np.testing.assert_array_equal(np.isinf(got["extremes"]), np.isinf(ext))
        np.testing.assert_allclose(got["extremes"][~np.isinf(ext)], ext[~np.isinf(ext)], rtol=0, atol=1e-6)
        good = np.stack([~np.isnan(r["com"][:, 0]) for r in rows])     # (the com row of a tick that is not a good one is NaN)
        m = np.where(good[:, :, None], got["measures"], np.nan)
        with np.errstate(all="ignore"):
            own = np.stack([np.fmin.reduce(m[:, :, 0]), np.fmax.reduce(m[:, :, 0]), np.fmax.reduce(m[:, :, 1]), np.fmin.reduce(m[:, :, 2]),
                            np.fmax.reduce(m[:, :, 3])], 1)
        fin = ~np.isnan(own)
        np.testing.assert_array_equal(got["extremes"][fin], own[fin].astype(np.float32))


def test_thresholds_stand_clear_of_every_measure():
    """every limit of the crafted case lies at least 1e-4 from every measured value, so that 1e-6 of float64 agreement decides no code"""
    ticks, corners, _ = crafted()
    for t in ticks:
        m = wl.measures(N, t["X"], t["P"], t["state_out"], corners, G)
        for col, keys in ((0, ("height_min", "height_max")), (1, ("reach_max",)), (2, ("margin_min",)), (3, ("track_max",))):
            v = m[:, col][np.isfinite(m[:, col])]
            for k in keys:
                assert np.abs(v - LIMITS[k]).min() >= 1e-4, (k, v)


def test_crafted_geometry_is_what_it_says():
    ticks, corners, _ = crafted()
    t = ticks[0]
    m = wl.measures(N, t["X"], t["P"], t["state_out"], corners, G)
    i = {k: j for j, k in enumerate(NAMES)}
    assert np.isnan(m[i["none"], :3]).all() and np.isfinite(m[i["none"], 3])
    assert np.isnan(m[i["nonfinite"]]).all()
    assert m[i["inside"], 2] > 0.02 and m[i["edge"], 2] < -0.05 and m[i["vertex"], 2] < -0.05
    assert m[i["segment"], 2] <= 0 and m[i["point"], 2] < 0
    L = cm.Layout(N)
    for name in ("edge", "vertex"):
        b = i[name]
        com, dcom = t["state_out"][b, :3].astype(np.float64), t["state_out"][b, 3:5].astype(np.float64)
        xi = com[:2] + dcom * np.sqrt(m[b, 0] / G)
        pts = np.array([t["X"][b, L.pos[c] + 3:L.pos[c] + 5].astype(np.float64) + corners[b, c, j, :2] for c in range(2) for j in range(4)])     # (yaw 0)
        nearest_vertex = np.linalg.norm(pts - xi, axis=1).min()
        assert (abs(-m[b, 2] - nearest_vertex) < 1e-9) == (name == "vertex"), name


@pytest.mark.parametrize("stop_mask", [15, 7, 11, 9, 8])
def test_host_form_matches_the_restatement(stop_mask):
    lib = cm._capi.lib()
    up, lo = box(cm.config.ergocub_gazebo_v1(N, 0.06))
    ticks, corners, outcome = crafted()
    rows, stats, final, ext = wl.reference(N, ticks, outcome, stop_mask, up, lo, LIMITS, corners, G)
    a = host_record_arrays(2, B, outcome, stop_mask)
    host_record_limits(lib, N, ticks, a, up, lo, LIMITS, corners)
    wr.assert_matches(a, rows, stats, final)
    assert_limits_match(a, rows, ext)
    # the crafted ticks do what they were made for
    code = np.stack([r["code"] for r in rows])
    i = {k: j for j, k in enumerate(NAMES)}
    limits, solver, nonfinite = bool(stop_mask & 8), bool(stop_mask & 2), bool(stop_mask & 4)
    assert code[0, i["several"]] == 6 and code[0, i["edge"]] == 8 and code[0, i["vertex"]] == 8 and code[0, i["status"]] == 3 and code[0, i["nonfinite"]] == 5
    assert code[0, i["none"]] == 0 and code[0, i["inside"]] == 0
    assert code[1, i["double"]] == 6 and code[1, i["single"]] == 7 and code[1, i["plain"]] == 9
    assert code[1, i["several"]] == (-1 if limits else 6) and code[1, i["status"]] == (-1 if solver else 3) and code[1, i["nonfinite"]] == (-1 if nonfinite else 5)
    assert stats[0, 5] == 3 and stats[1, 5] == (3 if limits else 6) and (stats[:, 1].sum() > 0) == (limits or solver or nonfinite)
    for name, tick in (("several", 11), ("edge", 11), ("double", 12), ("single", 12), ("plain", 12)):
        assert final["end_tick"][i[name]] == (tick if limits else -1), name
        # the value that fired can be read from the trace, on the ending tick too
        assert np.isfinite(a["measures"][tick - 11, i[name]]).all()
    assert np.isnan(a["measures"][0, i["status"]]).all() == solver     # a tick that codes 1..5 end holds NaN
    if limits:
        assert np.isnan(a["measures"][1, i["several"]]).all() and np.isinf(a["extremes"][i["several"]]).all()     # ended at its first tick: no good tick


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_form_matches_the_restatement_on_random_ticks(seed):
    """random codes 0..5, random support sets and yaws, problems ended earlier, with every limit off (no threshold to stand clear of) and all bits set"""
    lib = cm._capi.lib()
    up, lo = box(cm.config.ergocub_gazebo_v1(N, 0.06))
    ticks, outcome = wl.random_ticks(N, B, seed, n=3)
    rows, stats, final, ext = wl.reference(N, ticks, outcome, 15, up, lo, wl.OFF, wl.CORNERS, G)
    a = host_record_arrays(3, B, outcome, 15)
    host_record_limits(lib, N, ticks, a, up, lo, wl.OFF, wl.CORNERS)
    wr.assert_matches(a, rows, stats, final)
    assert_limits_match(a, rows, ext)


def test_every_limit_off_records_measures_and_ends_nobody():
    lib = cm._capi.lib()
    up, lo = box(cm.config.ergocub_gazebo_v1(N, 0.06))
    ticks, corners, outcome = crafted()
    rows, stats, final, ext = wl.reference(N, ticks, outcome, 15, up, lo, wl.OFF, corners, G)
    a = host_record_arrays(2, B, outcome, 15)
    host_record_limits(lib, N, ticks, a, up, lo, wl.OFF, corners)
    wr.assert_matches(a, rows, stats, final)
    assert_limits_match(a, rows, ext)
    assert (stats[:, 5] == 0).all() and not (np.stack([r["code"] for r in rows]) >= 6).any()
    plain = host_record_arrays(2, B, outcome, 15)
    host_record(lib, N, ticks, plain, up, lo)
    for k in plain:
        if k != "_c":
            np.testing.assert_array_equal(a[k].view(np.uint8), plain[k].view(np.uint8), err_msg=k)     # what the record wrote before is untouched


def test_limits_null_is_the_record_to_the_bit():
    lib = cm._capi.lib()
    up, lo = box(cm.config.ergocub_gazebo_v1(N, 0.06))
    for variant in ("codes", "ended", "feet"):
        ticks, outcome = wr.crafted_ticks(N, variant)
        a, b = host_record_arrays(2, 5, outcome, 7), host_record_arrays(2, 5, outcome, 7)
        host_record(lib, N, ticks, a, up, lo)
        for i, t in enumerate(ticks):
            assert lib.cmpc_rollout_record_limits(N, 5, 11 + i, i, _ptr(t["X"]), _ptr(t["P"]), _ptr(t["info"]), _ptr(t["ok"]), _ptr(t["land"]),
                                                  _ptr(t["state_out"]), _ptr(t["zmp"]), _ptr(up), _ptr(lo), C.byref(b["_c"]), None, None, 0, 0.0) == 0
        for k in a:
            if k != "_c":
                np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


def test_refusals_and_symbols():
    lib = cm._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    for name in ("cmpc_set_walk_limits", "cmpc_walk_extremes_init_device", "cmpc_rollout_record_limits"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and "int " + name + "(" in hdr, name
    assert "#define CMPC_WALK_MEASURES 4" in hdr and "#define CMPC_WALK_EXTREMES 5" in hdr
    assert cm._capi.STOP_BITS["limits"] == 8 and cm._capi.WALK_MEASURES == 4 and cm._capi.WALK_EXTREMES == 5
    assert C.sizeof(cm._capi.CmpcWalkLimits) == 64
    up, lo = box(cm.config.ergocub_gazebo_v1(N, 0.06))
    ticks, corners, outcome = crafted()
    t = ticks[0]
    a = host_record_arrays(2, B, outcome, 15)
    ms, c = np.zeros((1, B, 4), np.float32), np.ascontiguousarray(corners)

    def call(lim, row=0, corners_ptr=_ptr(c), gravity=G, horizon=N):
        return lib.cmpc_rollout_record_limits(horizon, B, 0, row, _ptr(t["X"]), _ptr(t["P"]), _ptr(t["info"]), _ptr(t["ok"]), _ptr(t["land"]),
                                              _ptr(t["state_out"]), _ptr(t["zmp"]), _ptr(up), _ptr(lo), C.byref(a["_c"]), C.byref(lim), corners_ptr, 24, gravity)
    assert call(limits_struct(dict(LIMITS, height_min=0.9, height_max=0.8))) != 0           # height_min above height_max
    bad = limits_struct(LIMITS, ms)
    bad.rows = 0
    assert call(bad) != 0                                                                    # a measures trace without rows
    assert call(limits_struct(LIMITS, ms), row=1) != 0                                       # a record row past the measures trace
    assert call(limits_struct(LIMITS), corners_ptr=None) != 0 and call(limits_struct(LIMITS), gravity=0.0) != 0
    assert call(limits_struct(dict(LIMITS, height_min=np.nan, height_max=0.1), ms)) == 0     # NaN beside a number: that limit alone is off
    assert lib.cmpc_set_walk_limits(None, None) != 0 and lib.cmpc_walk_extremes_init_device(None, None, None) != 0     # a NULL handle
