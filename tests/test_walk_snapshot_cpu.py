"""The walk snapshot without a GPU: the host copy cmpc_rollout_snapshot against numpy fancy indexing (every bit, NaN payloads and -0.0 included), its
argument checks and the device form's that need no GPU, the struct's size and the size formula, the Python surface, and the segment schedule of a
checkpointed walk (a pure function)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_snapshot_ref as ws

N, M, B, SB = 10, 5, 70, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _index_cases(rng, batch=B, src_batch=SB):
    mixed = rng.integers(0, src_batch, batch).astype(np.int32)
    mixed[[3, batch - 1]] = -1
    mixed[[0, 17]] = src_batch
    return {"permutation": rng.permutation(batch).astype(np.int32), "all_equal": np.full((batch,), 4, np.int32), "out_of_range": mixed}


def _host(src, dst, index, ok, batch=B, src_batch=SB, max_contacts=M, horizon=N, without_src=(), without_dst=()):
    lib = cm._capi.lib()
    s, d = ws.struct(src, 7, 1, without_src), ws.struct(dst, 0, 0, without_dst)
    return lib.cmpc_rollout_snapshot(horizon, batch, src_batch, max_contacts, C.byref(s), C.byref(d), None if index is None else index.ctypes.data_as(C.c_void_p),
                                     None if ok is None else ok.ctypes.data_as(C.c_void_p))


@pytest.mark.parametrize("case", ["identity", "permutation", "all_equal", "out_of_range"])
def test_host_snapshot_is_fancy_indexing(case):
    rng = np.random.default_rng(11)
    sb = B if case in ("identity", "permutation") else SB
    src = ws.arrays(N, M, sb, rng)
    dst = ws.arrays(N, M, B, fill=0xA5)
    index = None if case == "identity" else _index_cases(rng, B, sb)[case]
    want, want_ok = ws.expected(src, dst, index, sb)
    ok = np.full((B,), -9, np.int32)
    assert _host(src, dst, index, ok, src_batch=sb) == 0
    assert (ok == want_ok).all()
    assert (want_ok == 0).sum() == (4 if case == "out_of_range" else 0)
    for k in want:
        assert (ws.bits(dst[k]) == ws.bits(want[k])).all(), k
    if case == "out_of_range":      # a bad index leaves the whole problem as it was
        for k in dst:
            assert (dst[k][want_ok == 0].view(np.uint8) == 0xA5).all(), k


@pytest.mark.parametrize("side", ["src", "dst"])
def test_optional_arrays_are_skipped(side):
    rng = np.random.default_rng(12)
    src, dst = ws.arrays(N, M, SB, rng), ws.arrays(N, M, B, fill=0x5A)
    index = _index_cases(rng)["out_of_range"]
    want, want_ok = ws.expected(src, dst, index, SB, without=ws.OPTIONAL)
    assert _host(src, dst, index, None, **{"without_" + side: ws.OPTIONAL}) == 0      # (and without ok)
    for k in want:
        assert (ws.bits(dst[k]) == ws.bits(want[k])).all(), k
    for k in ws.OPTIONAL:
        assert (dst[k].view(np.uint8) == 0x5A).all(), k


def test_argument_checks_need_no_gpu():
    lib = cm._capi.lib()
    rng = np.random.default_rng(13)
    src, dst = ws.arrays(N, M, B, rng), ws.arrays(N, M, B, fill=0)
    assert _host(src, dst, None, None, src_batch=B) == 0
    assert _host(src, dst, None, None, src_batch=B, max_contacts=0) == -1
    assert _host(src, dst, None, None, src_batch=SB) == -1                      # identity with src_batch != batch
    assert _host(src, dst, None, None, src_batch=B, horizon=0) == -1 and _host(src, dst, None, None, batch=0, src_batch=0) == -1
    for k, _, _ in ws.FIELDS:                                                  # a NULL required pointer, on either side
        want = 0 if k in ws.OPTIONAL else -1
        assert _host(src, dst, None, None, src_batch=B, without_src=(k,)) == want, k
        assert _host(src, dst, None, None, src_batch=B, without_dst=(k,)) == want, k
    alias = dict(dst)                                                           # a destination array that is also a source array
    alias["dLand"] = src["dLand"]
    assert _host(src, alias, None, None, src_batch=B) == -1
    alias = dict(dst)
    alias["dListT"] = src["dListTB"]
    assert _host(src, alias, None, None, src_batch=B) == -1
    s, d = ws.struct(src), ws.struct(dst)
    assert lib.cmpc_rollout_snapshot(N, B, B, M, None, C.byref(d), None, None) == -1 and lib.cmpc_rollout_snapshot(N, B, B, M, C.byref(s), None, None, None) == -1
    # the device form refuses a NULL handle before anything touches a GPU
    assert lib.cmpc_rollout_snapshot_device(None, M, B, C.byref(s), C.byref(d), None, None, None) == -1


def test_struct_size_and_size_formula():
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    body = re.search(r"typedef struct cmpc_walk_snapshot \{(.*?)\} cmpc_walk_snapshot;", hdr, re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    ints = [d for d in decls if d.startswith("int ") and "*" not in d]
    ptrs = [d for d in decls if "*" in d]
    assert len(ints) == 2 and len(ptrs) == 20 and len(ints) + len(ptrs) == len(decls)
    assert [d.split("*")[1].strip() for d in ptrs] == [k for k, _, _ in ws.FIELDS]
    assert C.sizeof(cm._capi.CmpcWalkSnapshot) == 4 * len(ints) + C.sizeof(C.c_void_p) * len(ptrs)
    lib = cm._capi.lib()
    L = cm.Layout(20)
    assert lib.cmpc_walk_snapshot_bytes(20, 6) == 4 * (2 * L.nx + L.np) + 176 * 6 + 160
    a = ws.arrays(20, 6, 1, fill=0)
    assert lib.cmpc_walk_snapshot_bytes(20, 6) == sum(v.nbytes for v in a.values())          # the formula is the arrays' bytes
    assert lib.cmpc_walk_snapshot_bytes(0, 6) == 0 and lib.cmpc_walk_snapshot_bytes(20, 0) == 0
    assert "4 (2 n_x + n_p) + 176 M + 160" in hdr


def test_exports_and_python_surface():
    lib = cm._capi.lib()
    for name in ("cmpc_rollout_snapshot", "cmpc_rollout_snapshot_device", "cmpc_walk_snapshot_bytes"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name), name
    ro = cm.rollout.WalkingRollout
    for name in ("walk_device_checkpointed", "walk_resume_device", "backward_device_checkpointed"):
        assert hasattr(ro, name), name
    for name in ("walk_snapshot", "rollout_snapshot_device"):
        assert hasattr(cm.BatchSolver, name), name
    assert hasattr(cm, "rollout_differentiable_checkpointed")
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(cm.BatchSolver.walk_snapshot)[:3] == ["self", "tick", "lists_in"]
    assert par(cm.BatchSolver.rollout_snapshot_device) == ["self", "src", "dst", "index", "ok", "src_batch"]
    assert par(ro.walk_device_checkpointed) == ["self", "ticks", "com0", "dcom0", "h0", "every", "kwargs"]
    assert par(ro.walk_resume_device) == ["self", "snapshot", "ticks", "index", "push", "push_ticks", "replan", "trace", "stop", "skip_ended", "taped", "every"]
    assert par(ro.backward_device_checkpointed) == ["self", "w", "grad_states", "grad_X", "rot"]
    assert par(cm.rollout_differentiable_checkpointed) == ["rollout", "ticks", "state0", "every", "push", "models", "push_ticks", "replan"]
    # the pinned signatures are unchanged
    assert par(ro.backward_device_refs) == ["self", "w", "grad_states", "grad_X", "rot"]
    assert par(ro.backward_device) == ["self", "w", "grad_states", "grad_X"] == par(ro.backward_device_rot)
    assert par(ro.forward_sensitivity_device) == ["self", "w", "dir_state0", "dir_list0", "dir_list_rot0", "dir_plan", "dir_plan_rot", "dir_push", "dir_models",
                                                  "dir_wrench", "solutions"]
    assert par(ro.walk_device) == ["self", "ticks", "com0", "dcom0", "h0", "push", "push_ticks", "replan", "trace", "stop", "skip_ended"]
    assert par(ro.walk_device_taped) == ["self", "ticks", "com0", "dcom0", "h0", "kwargs"]
    assert par(cm.rollout_differentiable)[-2:] == ["ref_com", "ref_h"] and par(cm.rollout_differentiable)[:10] == [
        "rollout", "ticks", "state0", "push", "models", "push_ticks", "plan_yaw", "device_walk", "replan", "plan_rot"]
    for doc in (ro.backward_device_checkpointed.__doc__, ro.walk_resume_device.__doc__):
        assert "Out of scope" in doc
    assert "same batch size and factor storage" in ro.walk_resume_device.__doc__


def test_segment_schedule():
    sched = cm.rollout.walk_schedule
    calls, snaps = sched(16, 5, {7: None})
    assert calls == [(0, 5), (5, 7), (7, 10), (10, 15), (15, 16)] and snaps == [5, 10, 15]
    assert sched(16, 16) == ([(0, 16)], []) and sched(16, 40, ()) == ([(0, 16)], []) and sched(16, None) == ([(0, 16)], [])
    assert sched(16, 8) == ([(0, 8), (8, 16)], [8])
    assert sched(16, 5, {0: None, 10: None, 16: None, 99: None}) == ([(0, 5), (5, 10), (10, 15), (15, 16)], [5, 10, 15])      # replans on a boundary or outside
    # a resumed walk: the multiples of `every` are tick numbers of the whole walk, and none sits at the resume tick itself
    assert sched(6, 5, {7: None, 12: None}, tick0=10) == ([(10, 12), (12, 15), (15, 16)], [15])
    assert sched(1, 1) == ([(0, 1)], []) and sched(3, 1) == ([(0, 1), (1, 2), (2, 3)], [1, 2])
    with pytest.raises(AssertionError):
        sched(4, 0)
