"""GPU: the physical limits of a device walk (include/cmpc.h, cmpc_set_walk_limits; WalkingRollout.set_limits).  The record kernel with limits against
the host form, bit for bit; a taped walk under graded hidden pushes whose measures the numpy restatement (tests/walk_limits_ref.py, the support region
as a hull) reproduces from the tape, and whose endings under limits chosen between the problems' peaks are the restatement's prediction; the reverse
walk's gates on those endings; a refill walk whose trials end by reach_max, each held to a mismatch walk of its own; the HBM-factor solver."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_limits_ref as wl
from tests import walk_record_ref as wr
from tests import walk_refill_ref as rf
from tests.test_gpu_walk_record import OUTCOME, _host, _solver_with_box
from tests.test_walk_limits_cpu import LIMITS, crafted, host_record_limits
from tests.test_walk_record_cpu import box, host_record_arrays

pytestmark = pytest.mark.gpu

N, DT, G = 10, 0.06, cm.config.GRAVITY
STOP = ("merge", "solver", "nonfinite", "limits")


def _bits(x, y, msg=""):
    np.testing.assert_array_equal(rf.bits(x), rf.bits(y), err_msg=msg)


def _cfg_corners(cfg):
    return np.asarray([c.corners for c in cfg.contacts], np.float32)


def _device_record_limits(s, ticks, outcome, stop_mask, lim, tick0=11):
    """cmpc_rollout_record_device tick by tick under cmpc_set_walk_limits, the outcome copied in first -> the record, measures and extremes on the host"""
    import torch
    names = [k for k, b in cm._capi.STOP_BITS.items() if stop_mask & b]
    rec = s.walk_record(len(ticks), stop=names)
    for k in OUTCOME:
        rec[k].copy_(torch.from_numpy(outcome[k]))
    rec["stats"].fill_(-7)     # (the call clears its row)
    B = ticks[0]["X"].shape[0]
    measures = torch.full((len(ticks), B, 4), 99.0, dtype=torch.float32, device="cuda")
    extremes = s.walk_extremes_init_device()
    s.set_walk_limits(height=(lim["height_min"], lim["height_max"]), reach_max=lim["reach_max"], margin_min=lim["margin_min"], track_max=lim["track_max"],
                      measures=measures, extremes=extremes)
    try:
        for i, t in enumerate(ticks):
            d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            s.rollout_record_device(tick0 + i, i, d["X"], d["P"], d["info"], d["ok"], d["land"], d["state_out"], d["zmp"], rec)
    finally:
        s.set_walk_limits(off=True)
    torch.cuda.synchronize()
    out = _host(rec)
    out.update(measures=measures.cpu().numpy(), extremes=extremes.cpu().numpy())
    return out


@pytest.mark.parametrize("case", [("crafted", 15), ("crafted", 7), ("models", 15), (70, 15), (70, 3), (300, 15), (300, 12)])
def test_record_kernel_with_limits_is_the_host_form(case):
    """the crafted ticks of the CPU test on the handle's corners and on per-problem models (the corner stride of the model records), random ticks at
    B = 70 (a partial second wave) and B = 300 (a second workgroup), masks with and without bit 3: every output bit-equal, dStats word 5 included"""
    kind, stop_mask = case
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    up, lo = box(cfg)
    if isinstance(kind, str):
        ticks, _, outcome = crafted()
    else:
        ticks, outcome = wl.random_ticks(N, kind, seed=kind)
    B = ticks[0]["X"].shape[0]
    s = _solver_with_box(cfg, B)
    corners = _cfg_corners(cfg)
    if kind == "models":
        from tests.test_gpu_walk_refill_long import _slot_models
        rows = _slot_models(B)
        s.set_models(rows)
        corners = rows[:, 10:].astype(np.float32).reshape(B, 2, 4, 3)
    h = host_record_arrays(len(ticks), B, outcome, stop_mask)
    host_record_limits(cm._capi.lib(), N, ticks, h, up, lo, LIMITS, corners, gravity=G)
    got = _device_record_limits(s, ticks, outcome, stop_mask, LIMITS)
    for k in list(wr.TRACE) + list(OUTCOME) + ["stats", "measures", "extremes"]:
        _bits(got[k], h[k], k)
    code = h["code"]
    assert ((code >= 6) & (code <= 9)).sum() >= 3 and h["stats"][:, 5].sum() == ((code >= 6) & (code <= 9)).sum()
    assert (h["stats"][:, 1].sum() > 0) and np.isfinite(h["measures"]).any() and np.isnan(h["measures"]).any()
    if not isinstance(kind, str):
        assert {6, 7, 8, 9} <= set(code.ravel().tolist()) or kind == 70, sorted(set(code.ravel().tolist()))


def test_limits_off_is_the_record_kernel_of_before_and_bad_settings_are_refused():
    """with no limits set the record is what it was (dStats word 5 stays 0); height_min above height_max and a measures trace with too few rows for
    the record's row are refused"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    up, lo = box(cfg)
    ticks, _, outcome = crafted()
    B = ticks[0]["X"].shape[0]
    s = _solver_with_box(cfg, B)
    from tests.test_gpu_walk_record import _device_record
    from tests.test_walk_record_cpu import host_record
    h = host_record_arrays(2, B, outcome, 7)
    host_record(cm._capi.lib(), N, ticks, h, up, lo)
    got = _device_record(s, ticks, outcome, 7)
    for k in list(wr.TRACE) + list(OUTCOME) + ["stats"]:
        _bits(got[k], h[k], k)
    assert (got["stats"][:, 5] == 0).all()
    with pytest.raises(RuntimeError, match="height_min"):
        s.set_walk_limits(height=(0.9, 0.8))
    short = torch.zeros((1, B, 4), dtype=torch.float32, device="cuda")
    s.set_walk_limits(measures=short)
    try:
        rec = s.walk_record(2)
        d = {k: torch.from_numpy(v).cuda() for k, v in ticks[0].items()}
        with pytest.raises(RuntimeError, match="measures"):
            s.rollout_record_device(0, 1, d["X"], d["P"], d["info"], d["ok"], d["land"], d["state_out"], d["zmp"], rec)
    finally:
        s.set_walk_limits(off=True)
    torch.cuda.synchronize()


# ---- walks under graded hidden pushes: forces the MPC is never told about, one pattern per problem, from nothing up ----
PUSHES = [(1, 0.0, 0, 16), (1, 0.4, 0, 16), (1, 0.9, 0, 16), (1, 1.6, 0, 16), (2, -1.5, 0, 16), (2, -3.0, 0, 16), (0, -1.2, 0, 16), (0, 3.0, 2, 5)]     # (axis, m/s^2, ticks)
PEAKS = dict(height_min=(0, np.nanmin), height_max=(0, np.nanmax), reach_max=(1, np.nanmax), margin_min=(2, np.nanmin), track_max=(3, np.nanmax))


def _hidden(T, table):
    h = np.zeros((T, len(table), 6), np.float32)
    for b, (axis, mag, t0, t1) in enumerate(table):
        h[t0:t1, b, axis] = mag
    return h


def _stand(B, seed=11):
    rng = np.random.default_rng(seed)
    com0 = (np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.005, 0.005, (B, 3))).astype(np.float32)
    return com0, np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32)


def _np(w):
    return {k: v.cpu().numpy() for k, v in w.items() if hasattr(v, "cpu")}


def _between(values, i):
    """the midpoint between the i-th and the (i + 1)-th of the sorted per-problem peaks, which must lie more than 1e-4 apart"""
    v = np.sort(np.asarray(values, np.float64))
    assert v[i + 1] - v[i] > 1e-4, v
    return float(0.5 * (v[i] + v[i + 1]))


def _restated(cfg, w, ticks):
    """the restatement applied to the tape's per-tick X, P and states -> measures [ticks, B, 4] float64"""
    tp = w["tape"]
    X, P, S = tp["X"].cpu().numpy(), tp["P"].cpu().numpy(), tp["states"].cpu().numpy()
    return np.stack([wl.measures(cfg.N, X[t], P[t], S[t + 1], _cfg_corners(cfg), G) for t in range(ticks)])


def _free_and_limited(n, B, ticks, table, ranks, **opts):
    """one roll-out, the pushes of `table`: the taped walk with every limit NaN (the measures alone), the limits picked between its problems' peaks
    (ranks: {limit: index into the sorted peaks}), the restatement's prediction, and the taped walks under those limits without and with skip_ended"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(n, DT)
    ro = cm.rollout.WalkingRollout(cfg, B, **opts)
    start, mm = _stand(B), dict(hidden_wrench=_hidden(ticks, table))
    ro.set_limits()
    free = ro.walk_device_taped(ticks, *start, mismatch=mm)
    torch.cuda.synchronize()
    f = _np(free)
    ref = _restated(cfg, free, ticks)
    lim = dict(wl.OFF)
    for k, i in ranks.items():
        col, peak = PEAKS[k]
        lim[k] = _between(peak(ref[:, :, col], axis=0), i)
    ro.set_limits(height=(lim["height_min"], lim["height_max"]), reach_max=lim["reach_max"], margin_min=lim["margin_min"], track_max=lim["track_max"])
    walks = {}
    for skip in (False, True):
        walks[skip] = ro.walk_device_taped(ticks, *start, mismatch=mm, stop=STOP, skip_ended=skip)
    torch.cuda.synchronize()
    ro.clear_limits()
    plain = ro.walk_device_taped(ticks, *start, mismatch=mm)
    torch.cuda.synchronize()
    return dict(cfg=cfg, ro=ro, B=B, ticks=ticks, free=free, f=f, ref=ref, lim=lim, walks=walks, plain=plain,
                predicted=wl.predict_endings(ref.astype(np.float32), f["code"], lim))


def _check_against_the_restatement(c, codes):
    f, ref, lim, B, ticks = c["f"], c["ref"], c["lim"], c["B"], c["ticks"]
    # the walk without limits: nobody ends, no code 6..9, measures on every tick, and the restatement reproduces them from the tape
    assert (f["end_tick"] == -1).all() and (f["code"] == 0).all() and (f["stats"][:, 5] == 0).all() and f["measures"].shape == (ticks, B, 4)
    assert np.isfinite(f["measures"]).all() and np.isfinite(ref).all()
    np.testing.assert_allclose(f["measures"], ref, rtol=0, atol=1e-6)
    ext = np.stack([f["measures"][..., 0].min(0), f["measures"][..., 0].max(0), f["measures"][..., 1].max(0), f["measures"][..., 2].min(0),
                    f["measures"][..., 3].max(0)], 1)
    _bits(f["extremes"], ext, "extremes")
    # setting no limits at all changes no other key, and returns neither measures nor extremes
    p = _np(c["plain"])
    assert set(p) == set(f) - {"measures", "extremes"}
    for k in p:
        _bits(np.delete(p[k], 6, -1) if k == "info" else p[k], np.delete(f[k], 6, -1) if k == "info" else f[k], k)
    # the thresholds stand clear of every value the restatement and the device could disagree on
    for k, (col, _) in PEAKS.items():
        if not np.isnan(lim[k]):
            assert np.abs(ref[..., col] - lim[k]).min() > 1e-5, k
    end_tick, end_code = c["predicted"]
    assert set(end_code[end_tick >= 0].tolist()) == set(codes) and (end_tick == -1).any(), (end_tick, end_code)
    for skip, w in c["walks"].items():
        g = _np(w)
        np.testing.assert_array_equal(g["end_tick"], end_tick)
        np.testing.assert_array_equal(g["end_code"], end_code)
        on = end_tick == -1
        for k in f:      # problems that do not end: every key of the walk without limits, to the bit (info word 6 is the clock)
            if k in ("stats", "extremes"):
                continue
            a, b = (g[k][:, on], f[k][:, on]) if g[k].shape[:2] == (ticks, B) else (g[k][on], f[k][on])
            if k == "info":
                a, b = np.delete(a, 6, -1), np.delete(b, 6, -1)
            _bits(a, b, f"{k}, skip_ended={skip}")
        _bits(g["extremes"][on], f["extremes"][on], "extremes of the walkers")
        for b in np.flatnonzero(~on):
            e = end_tick[b]
            _bits(g["measures"][:e + 1, b], f["measures"][:e + 1, b], f"problem {b}: measures up to and on its ending tick")
            assert np.isnan(g["measures"][e + 1:, b]).all() and (g["code"][e + 1:, b] == -1).all() and g["code"][e, b] == end_code[b]
            assert wl.limit_code(g["measures"][e, b], lim) == end_code[b]      # the value that fired, read from the trace
            _bits(g["final_state"][b], c["free"]["tape"]["states"][e, b].cpu().numpy(), f"problem {b}: final_state, the state after its last good tick")
        np.testing.assert_array_equal(g["stats"][:, 5], np.array([(end_tick == t).sum() for t in range(ticks)]))
    # skip_ended: an ended problem's rows stay what its ending tick left (the tape rows behind it repeat the ending tick's)
    g, tp = _np(c["walks"][True]), c["walks"][True]["tape"]
    for b in np.flatnonzero(end_tick >= 0):
        e = end_tick[b]
        _bits(g["state"][b], c["free"]["tape"]["states"][e + 1, b].cpu().numpy(), f"problem {b}: the state its ending tick left")
        _bits(g["X"][b], c["free"]["tape"]["X"][e, b].cpu().numpy(), f"problem {b}: X of its ending tick")
        _bits(g["P"][b], c["free"]["tape"]["P"][e, b].cpu().numpy(), f"problem {b}: P of its ending tick")


@pytest.fixture(scope="module")
def graded():
    # the ranks are where the graded pushes leave room: the deepest sink ends by height, the third-largest reach, the third-deepest margin and the
    # third-largest track lie above problems that no other limit has ended by then
    return _free_and_limited(N, 8, 16, PUSHES, dict(height_min=0, height_max=6, reach_max=5, margin_min=2, track_max=4))


def test_taped_walk_under_graded_pushes(graded):
    """B = 8, 16 ticks: the measures against the restatement within 1e-6; limits between adjacent peaks; end ticks and codes as the restatement
    predicts, one problem at least per code 6..9 and walkers left; the problems that walk on bit-equal in every key; skip_ended the same"""
    _check_against_the_restatement(graded, (6, 7, 8, 9))


def test_gates_inherit_the_physical_endings(graded):
    """backward_device on the walk under limits equals backward_device on the taped walk without limits with end_tick replaced by the limits walk's;
    without skip_ended the two tapes are identical"""
    import torch
    c = graded
    ro, ticks, B = c["ro"], c["ticks"], c["B"]
    w, free = c["walks"][False], c["free"]
    for k, v in free["tape"].items():
        if hasattr(v, "cpu"):
            a, b = w["tape"][k].cpu().numpy(), v.cpu().numpy()
            _bits(np.delete(a, 6, -1) if k == "info" else a, np.delete(b, 6, -1) if k == "info" else b, "tape " + k)
    rng = np.random.default_rng(3)
    gS = torch.from_numpy(rng.normal(size=(ticks + 1, B, 9))).cuda()
    gX = torch.from_numpy((1e-2 * rng.normal(size=(ticks, B, ro.L.nx))).astype(np.float32)).cuda()
    got = ro.backward_device(w, gS, gX)
    swapped = dict(free)
    swapped["end_tick"] = w["end_tick"]
    want = ro.backward_device(swapped, gS, gX)
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k in got:
        _bits(got[k].cpu().numpy(), want[k].cpu().numpy(), k)
    end = w["end_tick"].cpu().numpy()
    status = got["status"].cpu().numpy()
    for b in np.flatnonzero(end >= 0):      # the gate: rows from the ending tick on are not walked (status 6), and their wrench rows are zero
        assert (status[end[b]:, b] == 6).all() and (got["wrench"][end[b]:, b] == 0).all()
    assert (end >= 0).sum() >= 4 and (status[:, end == -1] != 6).all()


def test_hbm_factor_solver():
    """N = 13, B = 6, factors="hbm", 12 ticks: the same checks, limits on the height, the reach and the margin"""
    c = _free_and_limited(13, 6, 12, [(a, m, t0, min(t1, 12)) for a, m, t0, t1 in PUSHES[:6]], dict(height_min=0, reach_max=3, margin_min=1), factors="hbm")
    _check_against_the_restatement(c, (6, 7, 8))


def test_refill_walk_ends_trials_by_reach():
    """B = 4, Q = 10, trials of 8 ticks under hidden lateral pushes graded by trial, reach_max between two trials' peaks: each trial's end tick, end
    code and measures rows are those of a walk_device_mismatch of its own in the same slot under the same limits; a freed slot takes the next trial on
    the following tick; extremes on a refill walk are refused"""
    import torch
    B, Q, TT, T = 4, 10, 8, 24
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0 = _stand(Q, seed=12)
    hidden = np.zeros((TT, Q, 6), np.float32)
    hidden[:, :, 1] = 0.3 * ((np.arange(Q) * 7) % Q)[None, :]      # 0 .. 2.7 m/s^2 sideways, shuffled over the queue
    mm = dict(hidden_wrench=hidden)
    ro = cm.rollout.WalkingRollout(cfg, B)
    ro.set_limits()
    free = ro.walk_device_refill_trials(T, TT, com0, dcom0, h0, mismatch=mm)
    torch.cuda.synchronize()
    assert "extremes" not in free and free["measures"].shape == (T, B, 4)
    ft = _np(free["trials"])
    assert (ft["end_tick"] == -1).all() and (ft["ticks"] == TT).all()
    peaks = np.array([free["trials"]["trace"](q)["measures"][:, 1].max().item() for q in range(Q)])
    reach_max = _between(peaks, Q // 2 - 1)
    ro.set_limits(reach_max=reach_max)
    w = ro.walk_device_refill_trials(T, TT, com0, dcom0, h0, mismatch=mm, stop=STOP)
    torch.cuda.synchronize()
    g, t = _np(w), _np(w["trials"])
    ended = t["end_tick"] >= 0
    assert ended.sum() >= 2 and (~ended).sum() >= 2 and (t["end_code"][ended] == 7).all() and (t["start"] >= 0).all()
    length = np.where(ended, t["end_tick"] + 1, TT)
    np.testing.assert_array_equal(t["ticks"], length)
    by_slot = [[q for q in np.argsort(t["start"], kind="stable") if t["slot"][q] == b] for b in range(B)]
    for b in range(B):      # a freed slot takes the next trial on the following tick
        assert by_slot[b] and t["start"][by_slot[b][0]] == 0
        for q1, q2 in zip(by_slot[b], by_slot[b][1:]):
            assert t["start"][q2] == t["start"][q1] + length[q1], (b, q1, q2)
    ref_ro = cm.rollout.WalkingRollout(cfg, B)
    ref_ro.set_limits(reach_max=reach_max)
    for j in range(max(len(s) for s in by_slot)):
        trials = np.array([s[j] if j < len(s) else s[0] for s in by_slot])
        ref = _np(ref_ro.walk_device_mismatch(TT, com0[trials], dcom0[trials], h0[trials], dict(hidden_wrench=np.ascontiguousarray(hidden[:, trials])),
                                              stop=STOP, skip_ended=True))
        for b in range(B):
            if j >= len(by_slot[b]):
                continue
            q = by_slot[b][j]
            s0, rows = int(t["start"][q]), int(length[q])
            assert t["end_tick"][q] == ref["end_tick"][b] and t["end_code"][q] == ref["end_code"][b], (q, b)
            _bits(g["measures"][s0:s0 + rows, b], ref["measures"][:rows, b], f"trial {q} (slot {b}, start {s0}) measures")
            _bits(g["code"][s0:s0 + rows, b], ref["code"][:rows, b], f"trial {q} code")
            _bits(g["com"][s0:s0 + rows, b], ref["com"][:rows, b], f"trial {q} com")
            if ended[q]:
                assert g["measures"][s0 + rows - 1, b, 1] > reach_max      # the value that fired
    # extremes on a refill walk: refused by the library
    s = ro.solver
    ro.clear_limits()
    s.set_walk_limits(extremes=s.walk_extremes_init_device())
    try:
        with pytest.raises(RuntimeError, match="dExtremes"):
            ro.walk_device_refill_trials(T, TT, com0, dcom0, h0, mismatch=mm)
    finally:
        s.set_walk_limits(off=True)
    torch.cuda.synchronize()
