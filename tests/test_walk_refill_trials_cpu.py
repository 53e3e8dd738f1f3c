"""Per-trial models and a per-trial plant mismatch on the refill walk, without a GPU (include/cmpc.h, cmpc_walk_refill_trials;
WalkingRollout.walk_device_refill_trials): the new symbol and struct, the layouts that must not have moved, every refusal that comes before anything
touches a GPU -- the old entry point's, in its order, and the three new ones -- and the Python surface's refusals."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_refill_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmpc_rollout_walk_refill_trials_device"
B, Q, TT = 5, 7, 3


def test_symbol_struct_and_pinned_layouts():
    lib = cm._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    assert NAME in cm._capi.EXPORTS and hasattr(lib, NAME) and "int " + NAME + "(" in hdr
    # the mirror: the header's field order, and the size its comment states
    body = re.search(r"typedef struct cmpc_walk_refill_trials \{(.*?)\} cmpc_walk_refill_trials;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in cm._capi.CmpcWalkRefillTrials._fields_]
    assert names == ["dModels", "dModelOk", "dHiddenWrench", "hidden_ticks", "dStateNoise", "noise_ticks", "dForceGain"]
    assert C.sizeof(cm._capi.CmpcWalkRefillTrials) == 56
    t = cm._capi.CmpcWalkRefillTrials
    assert [getattr(t, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48]
    # the two structs the feature sits between keep their sizes
    assert C.sizeof(cm._capi.CmpcWalkRefill) == 8 + 8 * 5 + 8 + 8 * 9 + 16
    assert C.sizeof(cm._capi.CmpcPlantMismatch) == 48
    # the Python surface: the new method, the solver's two pieces, and the pinned signature and refusal of walk_device_refill
    ro = cm.rollout.WalkingRollout
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.walk_device_refill_trials) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "models", "mismatch", "kwargs"]
    assert par(cm.BatchSolver.walk_refill_trials) == ["self", "models", "hidden_wrench", "state_noise", "force_gain", "device"]
    assert par(cm.BatchSolver.rollout_walk_refill_device)[-1] == "trials"
    assert par(ro.walk_device_refill) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "push", "push_ticks", "wrench_trials", "trace", "stop",
                                          "replan", "mismatch", "taped", "every"]
    assert "Out of scope" in ro.walk_device_refill.__doc__ and "walk_device_refill_trials" in ro.walk_device_refill.__doc__


def test_refusals_need_no_gpu():
    lib = cm._capi.lib()
    lib.cmpc_last_error.restype = C.c_char_p
    a = rf.arrays(B, Q, rows=2, seed=9)
    rec, f = rf.structs(a, TT)
    assert lib.cmpc_rollout_refill_init(B, C.byref(f)) == 0
    why = lambda: lib.cmpc_last_error(None).decode()
    spare = a["state0"].ctypes.data      # (any non-NULL address: nothing is read before the refusal)

    def walk(m, io, trials, rec=rec, f=f):
        out = C.c_int(0)
        return getattr(lib, NAME)(None, m, 0, 1, C.byref(io) if io is not None else None, C.byref(rec) if rec is not None else None,
                                  C.byref(f) if f is not None else None, C.byref(trials) if trials is not None else None, 0, 0, C.byref(out), None)

    # ---- the old entry point's refusals in its order, with the per-trial struct absent, empty, and -- for the two that come first -- bad
    bad = cm._capi.CmpcWalkRefillTrials(None, None, None, -1, None, 0, None)
    for trials in (None, cm._capi.CmpcWalkRefillTrials()):
        io = cm._capi.CmpcWalkIO()
        assert walk(17, io, trials) == -1 and "max_contacts must be 1 .. 16" in why()
        assert walk(0, io, trials) == -1 and "max_contacts must be 1 .. 16" in why()
        assert walk(16, io, trials) == -1 and "null handle" in why()
        io.dWrenchTicks, io.wrench_ticks = spare, 1
        assert walk(4, io, trials) == -1 and "dWrenchTicks is not taken" in why()
        assert walk(4, None, trials) == -1 and "null argument" in why()
        assert walk(4, cm._capi.CmpcWalkIO(), trials, rec=None) == -1 and "null argument" in why()
        assert walk(4, cm._capi.CmpcWalkIO(), trials, f=None) == -1 and "null argument" in why()
    io = cm._capi.CmpcWalkIO()
    assert walk(17, io, bad) == -1 and "max_contacts must be 1 .. 16" in why()
    io.dWrenchTicks, io.wrench_ticks = spare, 1
    assert walk(4, io, bad) == -1 and "dWrenchTicks is not taken" in why()
    # ---- the new refusals: a negative count, a schedule with no rows, dModelOk without dModels -- each named, none needing a handle
    io = cm._capi.CmpcWalkIO()
    T = cm._capi.CmpcWalkRefillTrials
    for trials in (T(None, None, None, -1, None, 0, None), T(None, None, None, 0, None, -3, None), T(None, None, spare, -1, spare, 2, None)):
        assert walk(4, io, trials) == -1 and "negative count" in why()
    for trials in (T(None, None, spare, 0, None, 0, None), T(None, None, None, 0, spare, 0, None), T(spare, None, spare, 2, spare, 0, spare)):
        assert walk(4, io, trials) == -1 and "schedule with no rows" in why()
    assert walk(4, io, T(None, spare, None, 0, None, 0, None)) == -1 and "dModelOk without dModels" in why()
    assert walk(4, io, T(None, spare, spare, 2, spare, 2, spare)) == -1 and "dModelOk without dModels" in why()
    # ... and what passes them reaches the handle check, counts without schedules included
    for trials in (T(spare, spare, spare, 2, spare, 3, spare), T(spare, None, None, 4, None, 5, None)):
        assert walk(4, io, trials) == -1 and "null handle" in why()


def test_python_refusals_before_anything_touches_a_gpu():
    ro = types.SimpleNamespace(M=5, force_sample_time=False)
    walk = cm.rollout.WalkingRollout.walk_device_refill_trials
    z = np.zeros((3, 3))
    with pytest.raises(ValueError, match="tick_first"):
        walk(ro, 4, 2, z, z, z, mismatch=dict(force_gain=np.ones(3), tick_first=3))
    for fst in (False, True):
        with pytest.raises(NotImplementedError):
            walk(types.SimpleNamespace(M=17, force_sample_time=fst), 4, 2, z, z, z, models=np.zeros((3, 34)))
    for kw in (dict(replan={2: None}), dict(taped=True), dict(every=4), dict(no_such_argument=1), dict(mismatch=dict(gain=np.ones(3)))):
        with pytest.raises(TypeError):
            walk(ro, 4, 2, z, z, z, **kw)
    with pytest.raises(ValueError, match="not both"):
        walk(ro, 4, 2, z, z, z, push=z, wrench_trials=np.zeros((1, 3, 10, 6)))
    # walk_device_refill itself still refuses a mismatch
    with pytest.raises(NotImplementedError):
        cm.rollout.WalkingRollout.walk_device_refill(ro, 4, 2, z, z, z, mismatch=dict(force_gain=np.ones(3)))
