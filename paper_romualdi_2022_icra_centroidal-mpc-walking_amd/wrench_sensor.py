"""The host forms of the wrench sensor (include/cmpc.h, cmpc_wrench_sensor; DESIGN.md 7f, "Sensed pushes"): cmpc_wrench_sense, cmpc_wrench_sense_vjp and
cmpc_wrench_sense_jvp on numpy arrays, with no handle and no GPU -- the functions the kernels run, statement for statement.  A leaf module: it imports
_capi alone.  The walk under a sensor is WalkingRollout.walk_device_sensed()."""
import ctypes as C

import numpy as np

from . import _capi


def _structs(hidden, tick_first, delay, hold_knots, deadband, noise):
    """(cmpc_plant_mismatch, cmpc_wrench_sensor, the arrays they point at) from host arrays: hidden[Th, B, 6], noise[Tn, B, 6] or None, float32"""
    hidden = np.ascontiguousarray(hidden, np.float32)
    assert hidden.ndim == 3 and hidden.shape[2] == 6, "hidden: expected [Th, B, 6]"
    m = _capi.CmpcPlantMismatch(int(tick_first), hidden.ctypes.data if hidden.size else None, int(hidden.shape[0]), None, 0, None)
    if noise is not None:
        noise = np.ascontiguousarray(noise, np.float32)
        assert noise.ndim == 3 and noise.shape[1:] == hidden.shape[1:], "noise: expected [Tn, B, 6]"
    s = _capi.CmpcWrenchSensor(int(delay), int(hold_knots), float(deadband), None if noise is None else noise.ctypes.data,
                               0 if noise is None else int(noise.shape[0]))
    return m, s, (hidden, noise)


def _check(rc, name):
    if rc != 0:
        raise ValueError(f"{name} failed ({rc}): {_capi.lib().cmpc_last_error(None).decode()}")


def sense(horizon, hidden, tick_first, tick0, rows, delay=0, hold_knots=1, deadband=0.7, noise=None, wrench_rows=True):
    """cmpc_wrench_sense: rows tick0 .. tick0 + rows - 1 of the rule -> (wrench_rows[rows, B, N, 6] float32 or None, plant_wrench[rows, B, 6] float32,
    pass[rows, B] int32).  ValueError where the C ABI refuses the arguments."""
    m, s, keep = _structs(hidden, tick_first, delay, hold_knots, deadband, noise)
    B = keep[0].shape[1]
    wr = np.empty((max(rows, 0), B, horizon, 6), np.float32) if wrench_rows else None
    pl = np.empty((max(rows, 0), B, 6), np.float32)
    ps = np.empty((max(rows, 0), B), np.int32)
    _check(_capi.lib().cmpc_wrench_sense(int(horizon), B, int(tick0), int(rows), C.byref(m), C.byref(s), None if wr is None else wr.ctypes.data, pl.ctypes.data,
                                         ps.ctypes.data), "cmpc_wrench_sense")
    return wr, pl, ps


def sense_vjp(horizon, hidden, tick_first, tick0, rows, grad_wrench, grad_hidden, delay=0, hold_knots=1, deadband=0.7, noise=None):
    """cmpc_wrench_sense_vjp: grad_wrench[rows, B, N, 6] float32 and grad_hidden[rows, B, 6] float64 (taken on the plant rows) -> (hidden_wrench[Th, B, 6],
    sensor_noise[Tn, B, 6] or None), float64"""
    m, s, keep = _structs(hidden, tick_first, delay, hold_knots, deadband, noise)
    B = keep[0].shape[1]
    gw = np.ascontiguousarray(grad_wrench, np.float32)
    gh = np.ascontiguousarray(grad_hidden, np.float64)
    assert gw.shape == (rows, B, horizon, 6) and gh.shape == (rows, B, 6)
    gt = np.empty(keep[0].shape, np.float64)
    gn = None if keep[1] is None else np.empty(keep[1].shape, np.float64)
    _check(_capi.lib().cmpc_wrench_sense_vjp(int(horizon), B, int(tick0), int(rows), C.byref(m), C.byref(s), gw.ctypes.data, gh.ctypes.data, gt.ctypes.data,
                                             None if gn is None else gn.ctypes.data), "cmpc_wrench_sense_vjp")
    return gt, gn


def sense_jvp(horizon, hidden, tick_first, tick0, rows, k, dir_hidden, dir_noise=None, delay=0, hold_knots=1, deadband=0.7, noise=None):
    """cmpc_wrench_sense_jvp: dir_hidden[Th, B, k, 6] and dir_noise[Tn, B, k, 6] (or None) float64 -> (dir_wrench[rows, B, k, N, 6] float32,
    dir_plant_wrench[rows, B, k, 6] float64)"""
    m, s, keep = _structs(hidden, tick_first, delay, hold_knots, deadband, noise)
    B = keep[0].shape[1]
    dh = np.ascontiguousarray(dir_hidden, np.float64)
    assert dh.shape == (keep[0].shape[0], B, k, 6)
    dn = None
    if keep[1] is not None and dir_noise is not None:
        dn = np.ascontiguousarray(dir_noise, np.float64)
        assert dn.shape == (keep[1].shape[0], B, k, 6)
    dw = np.empty((rows, B, k, horizon, 6), np.float32)
    dp = np.empty((rows, B, k, 6), np.float64)
    _check(_capi.lib().cmpc_wrench_sense_jvp(int(horizon), B, int(tick0), int(rows), int(k), C.byref(m), C.byref(s), dh.ctypes.data,
                                             None if dn is None else dn.ctypes.data, dw.ctypes.data, dp.ctypes.data), "cmpc_wrench_sense_jvp")
    return dw, dp
