"""The wrench sensor of a sensed walk without a GPU (include/cmpc.h, "sensed pushes"): the host forms of the built library -- the functions the kernels
run -- against the independent float64 restatement tests/wrench_sensor_ref.py, the limiting sensors, the transpose and the tangent, the ctypes mirror
against the header, and the refusals that need no device."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import cmpc_amd as cm
from tests import wrench_sensor_ref as ref

ws = cm.wrench_sensor
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmpc.h")
N, B, TICKS, TICK_FIRST, TH, TN, BAND = 10, 8, 6, 1, 4, 3, 0.5
# The rule is linear on a branch, so a central difference has no truncation error: the gap is rounding, eps_machine * |f| / step ~ 1e-16 / 1e-4 = 1e-12
# relative to entries of order one (tests/test_mismatch_cpu.py states the same for the plant).  1e-8 leaves four decades.
FD = 1e-8


def fixture(threshold=True):
    """hidden[4, B, 6], noise[3, B, 6]: problems 0-2 below the dead-band (n2 = 0.1875 < 0.25), problem 3 exactly on it (n2 == 0.25: passes; with
    threshold=False moved to 0.75, away from the kink), problems 4-6 with force norms in [1, 2], problem 7 all zero.  The noise is small beside the
    margins of problems 0-2 and 4-7 and zero on problem 3, so that its threshold case stays exact."""
    rng = np.random.default_rng(20)
    hidden = np.zeros((TH, B, 6), np.float32)
    hidden[:, 0:3, :3] = 0.25
    hidden[:, 3, 0] = 0.5 if threshold else 0.75
    for b in (4, 5, 6):
        d = rng.normal(size=(TH, 3))
        hidden[:, b, :3] = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.0, 2.0, (TH, 1))).astype(np.float32)
    hidden[:, :7, 3:] = rng.normal(0, 0.3, (TH, 7, 3)).astype(np.float32)
    noise = rng.normal(0, 0.01, (TN, B, 6)).astype(np.float32)
    noise[:, 3] = 0
    return hidden, noise


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


CASES = list(itertools.product((0, 2), (1, 3, N), (False, True), (0, 3)))


@pytest.mark.parametrize("delay,hold,with_noise,tick0", CASES)
def test_host_form_is_the_restatement(delay, hold, with_noise, tick0):
    """every dPass equal; wrench and plant rows bit-equal after the restatement's own float32 roundings; rows outside the schedules read zeros by
    selection; and both branches occur in every row whose reading has a source row -- a condition of the fixture, checked here"""
    hidden, noise = fixture()
    noise = noise if with_noise else None
    rows = TICKS - tick0
    wr, pl, ps = ws.sense(N, hidden, TICK_FIRST, tick0, rows, delay, hold, BAND, noise)
    wr_r, pl_r, ps_r = ref.sense(N, hidden, noise, TICK_FIRST, delay, hold, BAND, tick0, rows, as_float32=True)
    np.testing.assert_array_equal(ps, ps_r)
    np.testing.assert_array_equal(bits(wr), bits(wr_r))
    np.testing.assert_array_equal(bits(pl), bits(pl_r))
    for r in range(rows):
        t = tick0 + r
        if 0 <= t - delay - TICK_FIRST < TH:
            assert ps[r].min() == 0 and ps[r].max() == 1, (t, ps[r])
            assert ps[r, 3] == 1      # (the threshold case: n2 == deadband^2 passes)
        elif noise is None:
            assert not ps[r].any() and not bits(wr[r]).any()      # (no source row and no noise: a reading of +0, zeroed)
        if not 0 <= t - TICK_FIRST < TH:      # (no true row: the plant feels minus what the MPC was told, or +0)
            np.testing.assert_array_equal(bits(pl[r]), bits(np.where(ps[r][:, None] == 1, -wr[r, :, 0], np.float32(0)).astype(np.float32) + np.float32(0)))
    assert not bits(wr[:, :, hold:]).any()      # (the knots beyond hold_knots are +0)


def test_outside_the_schedules_nothing_is_read():
    """NaN planted around the schedules, inside one allocation: ticks before tick_first + delay and past the schedule read zeros by selection"""
    hidden, noise = fixture()
    pad = lambda a: np.concatenate([np.full((2,) + a.shape[1:], np.nan, np.float32), a, np.full((2,) + a.shape[1:], np.nan, np.float32)])
    hp, npad = pad(hidden), pad(noise)
    for delay in (0, 2):
        want = ws.sense(N, hidden, TICK_FIRST, 0, TICKS, delay, 3, BAND, noise)
        got = ws.sense(N, hp[2:2 + TH], TICK_FIRST, 0, TICKS, delay, 3, BAND, npad[2:2 + TN])
        for a, b in zip(want, got):
            assert np.isfinite(b).all()
            np.testing.assert_array_equal(bits(a) if a.dtype != np.int32 else a, bits(b) if b.dtype != np.int32 else b)


def test_limiting_sensors():
    """deadband = inf is the blind sensor: wrench rows all +0 and plant == true, bit for bit.  deadband = 0, delay = 0, no noise is the perfect sensor:
    plant all +0 and the wrench knots < hold_knots equal the hidden row"""
    hidden, noise = fixture()
    true = np.zeros((TICKS, B, 6), np.float32)
    true[TICK_FIRST:TICK_FIRST + TH] = hidden
    wr, pl, ps = ws.sense(N, hidden, TICK_FIRST, 0, TICKS, 1, 3, np.inf, noise)
    assert not ps.any() and not bits(wr).any()
    np.testing.assert_array_equal(bits(pl), bits(true))
    wr, pl, ps = ws.sense(N, hidden, TICK_FIRST, 0, TICKS, 0, 3, 0.0, None)
    assert ps.all() and not bits(pl).any()
    np.testing.assert_array_equal(bits(wr[:, :, :3]), bits(np.broadcast_to(true[:, :, None, :], (TICKS, B, 3, 6)).copy()))
    assert not bits(wr[:, :, 3:]).any()


def _dyadic(rng, shape, scale=1.0):
    """values on a grid of 2^-8 inside (-2, 2) * scale: float32 holds them and their few-term sums exactly, so the float32 rounding of the tangent's
    wrench rows and of the transpose's float32 input changes nothing"""
    return rng.integers(-512, 513, shape).astype(np.float64) / 256.0 * scale


@pytest.mark.parametrize("delay,hold,with_noise,tick0", [(0, 1, False, 0), (2, 3, True, 0), (1, N, True, 3), (2, 3, False, 3)])
def test_vjp_and_jvp_are_the_restated_jacobian(delay, hold, with_noise, tick0):
    """the host VJP is J^T g and the host JVP is J d of the restated Jacobian, and <g, J d> == <J^T g, d>, to 1e-14 relative (sums of a few terms in two
    orders); on exactly representable seeds"""
    hidden, noise = fixture()
    noise = noise if with_noise else None
    rows = TICKS - tick0
    rng = np.random.default_rng(5)
    gw, gp = _dyadic(rng, (rows, B, N, 6)), _dyadic(rng, (rows, B, 6))
    dh, dn = _dyadic(rng, (TH, B, 6)), (_dyadic(rng, (TN, B, 6)) if with_noise else None)
    gt, gn = ws.sense_vjp(N, hidden, TICK_FIRST, tick0, rows, gw, gp, delay, hold, BAND, noise)
    gt_r, gn_r = ref.vjp(N, hidden, noise, TICK_FIRST, delay, hold, BAND, tick0, rows, gw, gp)
    dw, dp = ws.sense_jvp(N, hidden, TICK_FIRST, tick0, rows, 1, dh[:, :, None], None if dn is None else dn[:, :, None], delay, hold, BAND, noise)
    dw_r, dp_r = ref.jvp(N, hidden, noise, TICK_FIRST, delay, hold, BAND, tick0, rows, dh, dn)
    close = lambda a, b: np.abs(a - b).max() <= 1e-14 * max(1.0, np.abs(b).max())
    assert close(gt, gt_r) and close(dw[:, :, 0].astype(np.float64), dw_r) and close(dp[:, :, 0], dp_r)
    assert (gn is None) == (noise is None) and (gn is None or close(gn, gn_r))
    lhs = float((gw * dw[:, :, 0]).sum() + (gp * dp[:, :, 0]).sum())
    rhs = float((gt * dh).sum() + (0.0 if gn is None else (gn * dn).sum()))
    assert abs(lhs - rhs) <= 1e-14 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    assert np.abs(gt).max() > 0 and np.abs(dw).max() > 0


@pytest.mark.parametrize("delay,hold,tick0", [(0, 3, 0), (2, N, 0), (1, 1, 3)])
def test_vjp_and_jvp_match_central_differences(delay, hold, tick0):
    """against central differences of the restated rule (float64), step 1e-4, on inputs whose force norm is at least 1e-2 from the threshold"""
    hidden, noise = fixture(threshold=False)
    rows, eps = TICKS - tick0, 1e-4
    for t in range(tick0, TICKS):      # (the condition on the inputs, checked)
        for b in range(B):
            f = ref.reading(hidden, noise, TICK_FIRST, delay, t, b)[:3]
            assert abs(np.linalg.norm(f) - BAND) >= 1e-2
    rng = np.random.default_rng(9)
    dh, dn = _dyadic(rng, (TH, B, 6)), _dyadic(rng, (TN, B, 6))
    h64, n64 = hidden.astype(np.float64), noise.astype(np.float64)
    f = lambda s: ref.sense(N, h64 + s * eps * dh, n64 + s * eps * dn, TICK_FIRST, delay, hold, BAND, tick0, rows)[:2]
    (w1, p1), (w0, p0) = f(1.0), f(-1.0)
    fd_w, fd_p = (w1 - w0) / (2 * eps), (p1 - p0) / (2 * eps)
    dw, dp = ws.sense_jvp(N, hidden, TICK_FIRST, tick0, rows, 1, dh[:, :, None], dn[:, :, None], delay, hold, BAND, noise)
    for name, got, want in (("wrench", dw[:, :, 0].astype(np.float64), fd_w), ("plant", dp[:, :, 0], fd_p)):
        gap = np.abs(got - want).max() / np.abs(want).max()
        print(f"sensor JVP delay={delay} hold={hold} tick0={tick0} {name}: relative gap to central differences {gap:.2e} (bound {FD:.0e})")
        assert gap <= FD, (name, gap)
    gw, gp = _dyadic(rng, (rows, B, N, 6)), _dyadic(rng, (rows, B, 6))
    gt, gn = ws.sense_vjp(N, hidden, TICK_FIRST, tick0, rows, gw, gp, delay, hold, BAND, noise)
    lhs, rhs = float((gw * fd_w).sum() + (gp * fd_p).sum()), float((gt * dh).sum() + (gn * dn).sum())
    print(f"sensor VJP delay={delay} hold={hold} tick0={tick0}: <g, FD> {lhs:.12e}  <J^T g, d> {rhs:.12e}")
    assert abs(lhs - rhs) <= FD * max(abs(lhs), abs(rhs))


def test_jvp_columns_are_single_column_calls():
    hidden, noise = fixture()
    rng = np.random.default_rng(3)
    dh, dn = rng.normal(size=(TH, B, 3, 6)), rng.normal(size=(TN, B, 3, 6))
    dw, dp = ws.sense_jvp(N, hidden, TICK_FIRST, 0, TICKS, 3, dh, dn, 1, 3, BAND, noise)
    for j in range(3):
        dw1, dp1 = ws.sense_jvp(N, hidden, TICK_FIRST, 0, TICKS, 1, dh[:, :, j:j + 1], dn[:, :, j:j + 1], 1, 3, BAND, noise)
        np.testing.assert_array_equal(bits(dw[:, :, j]), bits(dw1[:, :, 0]))
        np.testing.assert_array_equal(bits(dp[:, :, j]), bits(dp1[:, :, 0]))


def test_struct_mirror_exports_and_surface():
    """the ctypes mirror has the header's field order and the size the header comment states; the symbols are declared, exported and built; the Python
    names exist and the pinned signatures are as tests/test_mismatch_cpu.py asserts them"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct cmpc_wrench_sensor \{(.*?)\} cmpc_wrench_sensor;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in cm._capi.CmpcWrenchSensor._fields_] == ["delay_ticks", "hold_knots", "deadband", "dSensorNoise", "noise_ticks"]
    size = int(re.search(r"sizeof\(cmpc_wrench_sensor\) == (\d+)", text).group(1))
    assert C.sizeof(cm._capi.CmpcWrenchSensor) == size == 32
    lib = cm._capi.lib()
    for name in ("cmpc_wrench_sense", "cmpc_wrench_sense_device", "cmpc_wrench_sense_vjp", "cmpc_wrench_sense_vjp_device", "cmpc_wrench_sense_jvp",
                 "cmpc_wrench_sense_jvp_device", "cmpc_rollout_walk_sensed_device"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and name in text, name
    ro = cm.rollout.WalkingRollout
    for name in ("wrench_sensor", "walk_device_sensed", "walk_resume_device_sensed", "backward_device_sensed", "forward_sensitivity_device_sensed"):
        assert hasattr(ro, name), name
    for name in ("_wrench_sensor", "_wrench_sense_device", "_rollout_walk_sensed_device", "_wrench_sense_vjp_device", "_wrench_sense_jvp_device"):
        assert hasattr(cm.BatchSolver, name), name
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.wrench_sensor) == ["self", "delay", "hold_knots", "deadband", "noise"]
    assert [inspect.signature(ro.wrench_sensor).parameters[k].default for k in ("delay", "hold_knots", "deadband", "noise")] == [0, 1, 0.7, None]
    assert par(ro.walk_device_sensed)[:8] == ["self", "ticks", "com0", "dcom0", "h0", "mismatch", "sensor", "tape"]
    assert par(ro.walk_resume_device_sensed)[:5] == ["self", "snapshot", "ticks", "mismatch", "sensor"]
    assert par(ro.backward_device_sensed) == ["self", "w", "grad_states", "grad_X"]
    assert par(ro.forward_sensitivity_device_sensed)[:5] == ["self", "w", "k", "dir_hidden_wrench", "dir_sensor_noise"]
    # the pinned signatures, as tests/test_mismatch_cpu.py asserts them
    assert par(ro.walk_device_mismatch)[:6] == ["self", "ticks", "com0", "dcom0", "h0", "mismatch"]
    assert par(ro.walk_resume_device_mismatch)[:4] == ["self", "snapshot", "ticks", "mismatch"]
    for k in ("hidden_wrench", "state_noise", "force_gain"):
        assert inspect.signature(cm.rollout_differentiable).parameters[k].default is None
    assert par(ro.walk_device)[-1] == "skip_ended" and par(ro.backward_device) == ["self", "w", "grad_states", "grad_X"]


def _walk_sensed_refusal(io=None, hidden=True, plant=True, **sensor):
    """cmpc_rollout_walk_sensed_device without a handle: -> (return code, error text).  The checks of the sensor come before the handle is looked at."""
    lib = cm._capi.lib()
    h = np.zeros((TH, B, 6), np.float32)
    nz = np.zeros((TN, B, 6), np.float32)
    pw = np.zeros((TICKS, B, 6), np.float32)
    m = cm._capi.CmpcPlantMismatch(TICK_FIRST, h.ctypes.data if hidden else None, TH if hidden else 0, None, 0, None)
    kw = dict(delay_ticks=0, hold_knots=1, deadband=0.7, noise=None, noise_ticks=0)
    kw.update(sensor)
    s = cm._capi.CmpcWrenchSensor(kw["delay_ticks"], kw["hold_knots"], kw["deadband"], nz.ctypes.data if kw["noise"] else None, kw["noise_ticks"])
    io = io or cm._capi.CmpcWalkIO()
    out = C.c_int(-1)
    rc = lib.cmpc_rollout_walk_sensed_device(None, 4, 0, TICKS, 1, C.byref(io), None, 0, 0, C.byref(out), None, 0, C.byref(m), C.byref(s),
                                             pw.ctypes.data if plant else None, None)
    return rc, lib.cmpc_last_error(None).decode()


def test_refusals_that_need_no_device():
    """every CMPC_ERR_ARG case of cmpc_rollout_walk_sensed_device and of the sense forms, each by its own reason, before anything touches a GPU"""
    ERR_ARG = -1
    assert "CMPC_ERR_ARG = -1" in open(HEADER).read()
    io = cm._capi.CmpcWalkIO()
    io.dWrenchTicks, io.wrench_ticks = 8, 1
    assert _walk_sensed_refusal(io)[0] == ERR_ARG and "not summed" in _walk_sensed_refusal(io)[1]
    io = cm._capi.CmpcWalkIO()
    io.tick.dWrench = 8
    assert _walk_sensed_refusal(io)[0] == ERR_ARG and "not summed" in _walk_sensed_refusal(io)[1]
    for kw, why in ((dict(hidden=False), "needs m->dHiddenWrench and dPlantWrench"), (dict(plant=False), "needs m->dHiddenWrench and dPlantWrench"),
                    (dict(hold_knots=0), "hold_knots"), (dict(delay_ticks=-1), "delay_ticks"), (dict(deadband=-0.1), "deadband"),
                    (dict(deadband=float("nan")), "deadband"), (dict(noise=True, noise_ticks=0), "sensor noise"),
                    (dict(noise_ticks=-1), "sensor noise")):
        rc, text = _walk_sensed_refusal(**kw)
        assert rc == ERR_ARG and why in text, (kw, rc, text)
    # the upper end of hold_knots needs the horizon: the host form has it (one check function behind every entry)
    hidden, noise = fixture()
    for kw, why in ((dict(hold_knots=N + 1), "hold_knots"), (dict(hold_knots=0), "hold_knots"), (dict(delay=-1), "delay_ticks"),
                    (dict(deadband=-1.0), "deadband"), (dict(deadband=float("nan")), "deadband")):
        with pytest.raises(ValueError, match=why):
            ws.sense(N, hidden, TICK_FIRST, 0, TICKS, **kw)
    with pytest.raises(ValueError, match="hidden-wrench schedule"):
        ws.sense(N, hidden[:0], TICK_FIRST, 0, TICKS)
    with pytest.raises(ValueError, match="hold_knots"):
        ws.sense_vjp(N, hidden, TICK_FIRST, 0, TICKS, np.zeros((TICKS, B, N, 6)), np.zeros((TICKS, B, 6)), hold_knots=N + 1)
    with pytest.raises(ValueError, match="hold_knots"):
        ws.sense_jvp(N, hidden, TICK_FIRST, 0, TICKS, 1, np.zeros((TH, B, 1, 6)), hold_knots=N + 1)
    # push= with a sensor, on the walk and on the resumed walk
    ro = cm.rollout.WalkingRollout
    with pytest.raises(ValueError, match="push="):
        ro.walk_device_sensed(None, TICKS, None, None, None, dict(hidden_wrench=hidden), object(), push=np.zeros((B, 3)))
    with pytest.raises(ValueError, match="push="):
        ro.walk_resume_device_sensed(None, None, TICKS, dict(hidden_wrench=hidden), object(), push=np.zeros((B, 3)))
