"""Ended problems out of the launches (include/cmpc.h, cmpc_set_ended_device), the part that needs no GPU: the symbol is declared, exported and mirrored,
a NULL handle is a bad argument, and WalkingRollout.walk_device has the switch, off by default."""
import ctypes as C
import inspect
import os
import re

import cmpc_amd as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmpc_set_ended_device"


def _declaration():
    header = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    m = re.search(r"^int " + NAME + r"\(([^)]*)\);", header, re.M)
    assert m, NAME + " is not declared in include/cmpc.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_the_library_exports_the_setter():
    assert NAME in cm._capi.EXPORTS
    assert hasattr(C.CDLL(cm._capi.LIB_PATH), NAME)


def test_a_null_handle_is_a_bad_argument():
    lib = cm._capi.lib()
    words = (C.c_int * 4)(-1, 0, -1, 2)
    assert lib.cmpc_set_ended_device(None, None) == -1          # CMPC_ERR_ARG
    assert lib.cmpc_set_ended_device(None, C.cast(words, C.c_void_p)) == -1
    assert b"cmpc_set_ended_device" in lib.cmpc_last_error(None)


def test_the_ctypes_prototype_is_the_headers():
    args = _declaration()
    assert args == ["cmpc_handle h", "const int* dEndTick"], args
    fn = cm._capi.lib().cmpc_set_ended_device
    # the handle is an opaque pointer and the mask a device pointer: both cross the FFI as void*; the result is the status int (ctypes' default)
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p] and len(fn.argtypes) == len(args)
    assert fn.restype is C.c_int


def test_walk_device_has_the_switch_off_by_default():
    p = inspect.signature(cm.rollout.WalkingRollout.walk_device).parameters
    assert "skip_ended" in p and p["skip_ended"].default is False
    assert list(p)[-1] == "skip_ended"         # (behind the existing arguments: positional callers are untouched)
    doc = cm.rollout.WalkingRollout.walk_device.__doc__
    for word in ("skip_ended", "state", "X", "P", "info", "lists"):
        assert word in doc, word
    assert hasattr(cm.BatchSolver, "set_ended_device")
