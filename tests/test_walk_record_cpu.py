"""The record rule of a device walk on the CPU: the host form cmpc_rollout_record (no GPU, no solve) against its numpy restatement
(tests/walk_record_ref.py) on ticks made by hand at N = 10, B = 5 -- landing knots -2, -1, 0, 3 and N on the feet; one problem per tick code 0..5 with
overlapping conditions (the first match wins); a problem that ended earlier; every combination of the stop bits; two consecutive ticks, so that the
final state, the iteration words and the least box slack accumulate."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_record_ref as wr

N = 10


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_record_arrays(rows, B, outcome, stop_mask, trace=True):
    """numpy arrays laid out like BatchSolver.walk_record's, the outcome copied in, and the cmpc_walk_record that points at them"""
    a = {k: v.copy() for k, v in outcome.items()}
    a["stats"] = np.full((rows, 6), -7, np.int32)     # (the call writes the whole row)
    if trace:
        for k, tail in wr.TRACE.items():
            a[k] = np.full((rows, B) + tail, 99, wr.TRACE_DTYPE[k])
    p = lambda k: _ptr(a[k]) if k in a else None
    a["_c"] = cm._capi.CmpcWalkRecord(rows, stop_mask, p("com"), p("zmp"), p("land"), p("landing_offset"), p("iterations"), p("code"), p("end_tick"),
                                      p("end_code"), p("iterations_sum"), p("iterations_max"), p("final_state"), p("box_slack_min"), p("stats"))
    return a


def host_record(lib, N, ticks, arrays, box_upper, box_lower, tick0=11, ok=True):
    for i, t in enumerate(ticks):
        rc = lib.cmpc_rollout_record(N, t["X"].shape[0], tick0 + i, i, _ptr(t["X"]), _ptr(t["P"]), _ptr(t["info"]), _ptr(t["ok"]) if ok else None,
                                     _ptr(t["land"]), _ptr(t["state_out"]), _ptr(t["zmp"]), _ptr(box_upper), _ptr(box_lower), C.byref(arrays["_c"]))
        assert rc == 0


def box(cfg):
    return (np.ascontiguousarray([c.bounding_box_upper_limit for c in cfg.contacts], np.float32),
            np.ascontiguousarray([c.bounding_box_lower_limit for c in cfg.contacts], np.float32))


@pytest.mark.parametrize("stop_mask", range(8))
@pytest.mark.parametrize("variant", ["feet", "codes", "ended"])
def test_host_record_matches_the_restatement(variant, stop_mask):
    lib = cm._capi.lib()
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    up, lo = box(cfg)
    ticks, outcome = wr.crafted_ticks(N, variant)
    rows, stats, final = wr.reference(N, ticks, outcome, stop_mask, up, lo)
    a = host_record_arrays(2, 5, outcome, stop_mask)
    host_record(lib, N, ticks, a, up, lo)
    wr.assert_matches(a, rows, stats, final)
    # the crafted ticks do what they were made for
    codes = np.stack([r["code"] for r in rows])
    if variant == "feet":
        assert (codes == 0).all() and np.isfinite(final["box_slack_min"]).all()
        assert sorted(set(np.stack([t["land"] for t in ticks]).ravel().tolist())) == [-2, -1, 0, 3, N]
        assert (final["iterations_sum"] == ticks[0]["info"][:, 0] + ticks[1]["info"][:, 0]).all()
    else:
        want = [0, 1, 2, 3, -1 if variant == "ended" else 4]
        assert codes[0].tolist() == want
        solver, nonfinite = bool(stop_mask & 2), bool(stop_mask & 4)
        assert codes[1].tolist() == [5, -1, -1 if solver else 1, -1 if solver else 2, -1 if (variant == "ended" or solver) else 0]
        assert final["end_tick"][0] == (12 if nonfinite else -1) and final["end_tick"][1] == 11      # (bit 0 is honoured whether set or not)
        assert final["end_tick"][4] == (7 if variant == "ended" else 11 if solver else -1)


def test_host_record_optional_pointers_and_bad_arguments():
    lib = cm._capi.lib()
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    up, lo = box(cfg)
    ticks, outcome = wr.crafted_ticks(N, "codes")
    for t in ticks:
        t["ok"][:] = 1      # (ok == NULL means every merge good)
    rows, stats, final = wr.reference(N, ticks, outcome, 7, up, lo)
    a = host_record_arrays(2, 5, outcome, 7, trace=False)     # no trace: the outcome and the statistics alone
    host_record(lib, N, ticks, a, up, lo, ok=False)
    np.testing.assert_array_equal(a["stats"], stats)
    for k in ("end_tick", "end_code", "iterations_sum", "iterations_max"):
        np.testing.assert_array_equal(a[k], final[k])
    t = ticks[0]
    args = lambda row: (N, 5, 0, row, _ptr(t["X"]), _ptr(t["P"]), _ptr(t["info"]), None, _ptr(t["land"]), _ptr(t["state_out"]), _ptr(t["zmp"]), _ptr(up),
                        _ptr(lo), C.byref(a["_c"]))
    assert lib.cmpc_rollout_record(*args(2)) != 0 and lib.cmpc_rollout_record(*args(-1)) != 0      # a row outside the record
    a["_c"].dEndTick = None
    assert lib.cmpc_rollout_record(*args(0)) != 0                                                   # the outcome arrays are required
