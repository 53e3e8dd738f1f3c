"""Trials of a refill walk that start from a snapshot, without a GPU (include/cmpc.h, cmpc_walk_refill_snapshot;
WalkingRollout.walk_device_refill_from_snapshot): the new symbols, the struct and the Python surface with the pinned signatures unchanged; every refusal
that comes before anything touches a GPU -- the old entry point's, in its order, and the new ones, each named; the host form of the restore step against
a numpy restatement (tests/walk_refill_snapshot_ref.py) for both values of the pool's lists_in against both live parities, over poisoned destinations;
and the host form once more from a stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_refill_ref as rf
from tests import walk_refill_snapshot_ref as rs
from tests import walk_snapshot_ref as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK, RESTORE = "cmpc_rollout_walk_refill_snapshot_device", "cmpc_rollout_refill_restore"
N, M, B, S = 10, 5, 5, 3


def test_symbols_struct_and_python_surface():
    lib = cm._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    for name in (WALK, RESTORE):
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and "int " + name + "(" in hdr, name
    # the mirror: the header's field order and offsets, and the size its comment states
    body = re.search(r"typedef struct cmpc_walk_refill_snapshot \{(.*?)\} cmpc_walk_refill_snapshot;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    t = cm._capi.CmpcWalkRefillSnapshot
    assert names == [f[0] for f in t._fields_] == ["pool", "pool_batch", "dTrialSnapshot", "dTrialSnapshotOk"]
    assert [getattr(t, n).offset for n in names] == [0, 8, 16, 24] and C.sizeof(t) == 32 and "sizeof == 32" in hdr
    # the structs the feature sits between keep their sizes
    assert C.sizeof(cm._capi.CmpcWalkRefillTrials) == 56 and C.sizeof(cm._capi.CmpcWalkRefill) == 8 + 8 * 5 + 8 + 8 * 9 + 16
    assert C.sizeof(cm._capi.CmpcWalkSnapshot) == 8 + 20 * 8 and C.sizeof(cm._capi.CmpcWalkRecord) == 8 + 13 * 8
    # the Python surface
    ro = cm.rollout.WalkingRollout
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.walk_device_refill_from_snapshot) == ["self", "snapshot", "ticks", "trial_ticks", "snapshot_of", "models", "mismatch", "kwargs"]
    assert par(cm.BatchSolver.walk_refill_snapshot) == ["self", "snapshot", "snapshot_of", "device"]
    assert par(cm.BatchSolver.rollout_walk_refill_snapshot_device)[:3] == ["self", "tick0", "ticks"]
    assert "snapshot" in par(cm.BatchSolver.rollout_walk_refill_snapshot_device) and "trials" in par(cm.BatchSolver.rollout_walk_refill_snapshot_device)
    # the pinned signatures are unchanged
    assert par(cm.BatchSolver.rollout_walk_refill_device)[-1] == "trials"
    assert par(ro.walk_device_refill_trials) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "models", "mismatch", "kwargs"]
    assert par(ro.walk_device_refill) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "push", "push_ticks", "wrench_trials", "trace", "stop",
                                          "replan", "mismatch", "taped", "every"]
    assert par(ro.walk_resume_device) == ["self", "snapshot", "ticks", "index", "push", "push_ticks", "replan", "trace", "stop", "skip_ended", "taped", "every"]
    assert par(ro.walk_resume_device_mismatch) == ["self", "snapshot", "ticks", "mismatch", "kwargs"]
    # the docstrings point at the new method and keep the pinned words
    for doc in (ro.walk_resume_device.__doc__, ro.walk_device_refill.__doc__):
        assert "Out of scope" in doc and "walk_device_refill" in doc and "walk_device_refill_from_snapshot" in doc
    assert "same batch size and factor storage" in ro.walk_resume_device.__doc__


def _walk_c(lib, m, io, rec, f, trials, frm):
    out = C.c_int(0)
    ref = lambda x: C.byref(x) if x is not None else None
    return getattr(lib, WALK)(None, m, 0, 1, ref(io), ref(rec), ref(f), ref(trials), ref(frm), 0, 0, C.byref(out), None)


def test_refusals_need_no_gpu():
    lib = cm._capi.lib()
    lib.cmpc_last_error.restype = C.c_char_p
    why = lambda: lib.cmpc_last_error(None).decode()
    a = rf.arrays(B, 7, rows=2, seed=9)
    rec, f = rf.structs(a, 3)
    assert lib.cmpc_rollout_refill_init(B, C.byref(f)) == 0
    spare = a["state0"].ctypes.data      # (any non-NULL address: nothing is read before the refusal)
    rng = np.random.default_rng(21)
    pool = ws.arrays(N, M, S, rng)
    idx, ok = np.zeros(7, np.int32), np.zeros(7, np.int32)
    good_pool = ws.struct(pool, 8, 1)
    good = rs.from_struct(good_pool, S, idx, ok)
    T = cm._capi.CmpcWalkRefillTrials

    # ---- the old entry point's refusals, in its order, with `from` absent and with a good one
    for frm in (None, good):
        io = cm._capi.CmpcWalkIO()
        assert _walk_c(lib, 17, io, rec, f, None, frm) == -1 and "max_contacts must be 1 .. 16" in why()
        assert _walk_c(lib, 0, io, rec, f, None, frm) == -1 and "max_contacts must be 1 .. 16" in why()
        assert _walk_c(lib, 16, io, rec, f, None, frm) == -1 and "null handle" in why()
        assert _walk_c(lib, 4, None, rec, f, None, frm) == -1 and "null argument" in why()
        assert _walk_c(lib, 4, io, None, f, None, frm) == -1 and "null argument" in why()
        assert _walk_c(lib, 4, io, rec, None, None, frm) == -1 and "null argument" in why()
        assert _walk_c(lib, 4, io, rec, f, T(None, None, None, -1, None, 0, None), frm) == -1 and "negative count" in why()
        assert _walk_c(lib, 4, io, rec, f, T(None, None, spare, 0, None, 0, None), frm) == -1 and "schedule with no rows" in why()
        assert _walk_c(lib, 4, io, rec, f, T(None, spare, None, 0, None, 0, None), frm) == -1 and "dModelOk without dModels" in why()
        io.dWrenchTicks, io.wrench_ticks = spare, 1
        assert _walk_c(lib, 4, io, rec, f, None, frm) == -1 and "dWrenchTicks is not taken" in why()
    # ... and they come ahead of the new ones: a bad `from` behind a bad max_contacts names max_contacts
    io = cm._capi.CmpcWalkIO()
    assert _walk_c(lib, 17, io, rec, f, None, rs.from_struct(None, S, idx, ok)) == -1 and "max_contacts must be 1 .. 16" in why()

    # ---- the new refusals, each named, none needing a handle
    def new(frm, words, f=f, io=io):
        assert _walk_c(lib, 4, io, rec, f, None, frm) == -1 and WALK in why() and words in why(), (words, why())

    new(rs.from_struct(None, S, idx, ok), "pool is NULL")
    for tick in (0, -3):
        p = ws.struct(pool, tick, 1)
        new(rs.from_struct(p, S, idx, ok), "pool->tick must be at least 1")
    for pb in (0, -1):
        new(rs.from_struct(good_pool, pb, idx, ok), "pool_batch must be at least 1")
    for k, _, _ in ws.FIELDS:
        p = ws.struct(pool, 8, 0, without=(k,))
        frm = rs.from_struct(p, S, idx, ok)
        if k in ws.OPTIONAL:
            assert _walk_c(lib, 4, io, rec, f, None, frm) == -1 and "null handle" in why(), k
        else:
            new(frm, "a required pool array is NULL")
    for li in (-1, 2):
        p = ws.struct(pool, 8, li)
        new(rs.from_struct(p, S, idx, ok), "pool->lists_in must be 0 or 1")
    new(rs.from_struct(good_pool, S, None, ok), "dTrialSnapshot is NULL")
    _, f0 = rf.structs(a, 3, trials=0)      # (an empty queue needs no indices: on to the handle check)
    assert _walk_c(lib, 4, io, rec, f0, None, rs.from_struct(good_pool, S, None, None)) == -1 and "null handle" in why()
    # a pool array that is also a live array: a list buffer of the walk, the record's end ticks, the state buffer
    io2 = cm._capi.CmpcWalkIO()
    io2.dListTB = pool["dListT"].ctypes.data
    new(good, "a pool array is also a live array", io=io2)
    io2 = cm._capi.CmpcWalkIO()
    io2.tick.dStateOut = pool["dState"].ctypes.data
    new(good, "a pool array is also a live array", io=io2)
    p = ws.struct(pool, 8, 1)
    p.dEndTick = a["end_tick"].ctypes.data
    new(rs.from_struct(p, S, idx, ok), "a pool array is also a live array")
    # what passes them all reaches the handle check (dTrialSnapshotOk is optional)
    assert _walk_c(lib, 4, io, rec, f, None, rs.from_struct(good_pool, S, idx, None)) == -1 and "null handle" in why()


def test_python_refusals_before_anything_touches_a_gpu():
    ro = types.SimpleNamespace(M=5, force_sample_time=False)
    walk = cm.rollout.WalkingRollout.walk_device_refill_from_snapshot
    snap = dict(tick=8, lists_in=1, max_contacts=5, batch=4)
    of = np.zeros(3, np.int32)
    with pytest.raises(ValueError, match="tick_first"):
        walk(ro, snap, 4, 2, of, mismatch=dict(force_gain=np.ones(3), tick_first=8))
    for kw in (dict(replan={2: None}), dict(taped=True), dict(every=4), dict(index=of), dict(skip_ended=True), dict(no_such_argument=1),
               dict(mismatch=dict(gain=np.ones(3)))):
        with pytest.raises(TypeError):
            walk(ro, snap, 4, 2, of, **kw)
    with pytest.raises(ValueError, match="not both"):
        walk(ro, snap, 4, 2, of, push=np.zeros((3, 3)), wrench_trials=np.zeros((1, 3, 10, 6)))
    with pytest.raises(NotImplementedError):
        walk(types.SimpleNamespace(M=17, force_sample_time=False), snap, 4, 2, of)
    with pytest.raises(ValueError, match="tick 1 or later"):
        walk(ro, dict(snap, tick=0), 4, 2, of)
    # a checkpoint whose walk's wrench schedule reaches the snapshot's tick is not continued (a schedule from tick 0, and one that starts at the tick)
    sched = types.SimpleNamespace(shape=(9, 4, 10, 6))
    with pytest.raises(NotImplementedError, match="wrench schedule"):
        walk(ro, dict(snap, wrench=(sched, 0)), 4, 2, of)
    with pytest.raises(NotImplementedError, match="wrench schedule"):
        walk(ro, dict(snap, wrench=(types.SimpleNamespace(shape=(1, 4, 10, 6)), 8)), 4, 2, of)


def _case(pool_lists_in, live_prev, seed):
    """B = 5 slots at tick 4 over a pool of 3 rows: slot 0 spawned from row 2, slot 1 walking since tick 2 (its index is good: untouched all the same), slot 2
    spawned with index -1, slot 3 spawned with index pool_batch, slot 4 spawned from row 2 again -- a repeat -- whose row had ended in the pool.  Trial 5 is
    never started, and an empty slot whose start tick is this tick is covered by the second call below."""
    rng = np.random.default_rng(seed)
    pool = ws.arrays(N, M, S, rng)
    pool["dEndTick"][:], pool["dEndCode"][:] = [-1, -1, 3], [0, 0, 5]
    live = ws.arrays(N, M, B, fill=rs.POISON)
    start = np.array([4, 2, 4, 4, 4], np.int32)
    trial = np.array([1, 0, 2, 3, 4], np.int32)
    of = np.array([1, 2, -1, S, 2, 0], np.int32)
    ok = np.full(6, -7, np.int32)
    return pool, live, start, trial, of, ok


@pytest.mark.parametrize("pool_lists_in", [0, 1])
@pytest.mark.parametrize("live_prev", [0, 1])
def test_host_restore_against_the_numpy_restatement(pool_lists_in, live_prev):
    lib = cm._capi.lib()
    pool, live, start, trial, of, ok = _case(pool_lists_in, live_prev, 30 + 2 * pool_lists_in + live_prev)
    want, want_ok = rs.expected(pool, pool_lists_in, 8, live, live_prev, 4, start, trial, of, ok)
    p, l = ws.struct(pool, 8, pool_lists_in), ws.struct(live, 0, live_prev)
    f, frm = rs.refill_struct(start, trial, 6), rs.from_struct(p, S, of, ok)
    before = {k: v.copy() for k, v in pool.items()}
    assert lib.cmpc_rollout_refill_restore(N, B, M, 4, C.byref(l), C.byref(f), C.byref(frm)) == 0
    assert ok.tolist() == want_ok.tolist() == [-7, 1, 0, 0, 1, -7]
    for k in want:
        assert (ws.bits(live[k]) == ws.bits(want[k])).all(), k
    for k in pool:
        assert (ws.bits(pool[k]) == ws.bits(before[k])).all(), k
    # ---- written down from the contract, independently of the restatement
    poison32 = np.uint32(0xA5A5A5A5).view(np.int32)
    for k in live:
        assert (live[k][1:2].view(np.uint8) == rs.POISON).all(), k                    # the walking slot: bit-untouched
        for b in (2, 3):                                                               # a bad index: nothing copied, ended at spawn with the pool's tick
            if k not in ("dEndTick", "dEndCode"):
                assert (live[k][b:b + 1].view(np.uint8) == rs.POISON).all(), (k, b)
        for b in (0, 4):                                                               # the repeated row: no word left unwritten
            assert (ws.bits(live[k][b:b + 1]) == ws.bits(live[k][0:1])).all(), (k, b)
    assert live["dEndTick"].tolist() == [3, poison32, 8, 8, 3] and live["dEndCode"].tolist() == [5, poison32, 0, 0, 5]    # (the ended row's outcome came along)
    for k in ("dState", "dP", "dX", "dX0", "dInfo", "dZmp", "dOk", "dLand", "dFinalState", "dBoxSlackMin", "dIterationsSum", "dIterationsMax"):
        assert (ws.bits(live[k][0:1]) == ws.bits(pool[k][2:3])).all(), k
    # the list sets: the pool's set lists_in is in the live set this tick reads as previous, its other set in the other live set
    sets = (rs.SET_A, rs.SET_B)
    for here, there in ((live_prev, pool_lists_in), (1 - live_prev, 1 - pool_lists_in)):
        for kl, kp in zip(sets[here], sets[there]):
            assert (ws.bits(live[kl][0]) == ws.bits(pool[kp][2])).all(), (kl, kp)
    assert not (ws.bits(pool["dListT"][2]) == ws.bits(pool["dListTB"][2])).all()         # (the two sets differ: a wrong pairing would show)

    # ---- another tick: nobody's start tick matches, then an empty slot whose start tick does -- nothing moves, with and without the flags
    after = {k: v.copy() for k, v in live.items()}
    trial[3] = -1
    for tick, flags in ((5, ok), (4, None)):
        start2 = start.copy()
        if tick == 4:
            start2[[0, 2, 4]] = 1
        f2, frm2 = rs.refill_struct(start2, trial, 6), rs.from_struct(p, S, of, flags)
        ok_before = ok.copy()
        assert lib.cmpc_rollout_refill_restore(N, B, M, tick, C.byref(l), C.byref(f2), C.byref(frm2)) == 0
        assert (ok == ok_before).all()
        for k in live:
            assert (ws.bits(live[k]) == ws.bits(after[k])).all(), (k, tick)


def test_host_restore_skips_optional_arrays_and_refuses():
    lib = cm._capi.lib()
    pool, live, start, trial, of, ok = _case(0, 1, 40)
    for side in ("pool", "live"):
        live = ws.arrays(N, M, B, fill=rs.POISON)
        ok[:] = -7
        want, want_ok = rs.expected(pool, 0, 8, live, 1, 4, start, trial, of, ok, without=ws.OPTIONAL)
        p = ws.struct(pool, 8, 0, without=ws.OPTIONAL if side == "pool" else ())
        l = ws.struct(live, 0, 1, without=ws.OPTIONAL if side == "live" else ())
        f, frm = rs.refill_struct(start, trial, 6), rs.from_struct(p, S, of, ok)
        assert lib.cmpc_rollout_refill_restore(N, B, M, 4, C.byref(l), C.byref(f), C.byref(frm)) == 0
        for k in want:
            assert (ws.bits(live[k]) == ws.bits(want[k])).all(), (side, k)
        for k in ws.OPTIONAL:
            assert (live[k].view(np.uint8) == rs.POISON).all(), (side, k)
    # the refusals of the host form
    lib.cmpc_last_error.restype = C.c_char_p
    why = lambda: lib.cmpc_last_error(None).decode()
    p, l = ws.struct(pool, 8, 0), ws.struct(live, 0, 1)
    f, frm = rs.refill_struct(start, trial, 6), rs.from_struct(p, S, of, ok)
    call = lambda l=l, f=f, frm=frm, n=N, b=B, m=M, t=4: lib.cmpc_rollout_refill_restore(n, b, m, t, C.byref(l) if l is not None else None,
                                                                                       C.byref(f) if f is not None else None,
                                                                                       C.byref(frm) if frm is not None else None)
    assert call() == 0
    assert call(l=None) == -1 and call(f=None) == -1 and call(frm=None) == -1
    assert call(n=0) == -1 and call(b=0) == -1 and call(m=0) == -1 and call(t=-1) == -1
    assert call(l=ws.struct(live, 0, 2)) == -1
    assert call(frm=rs.from_struct(ws.struct(pool, 0, 0), S, of, ok)) == -1 and "pool->tick" in why()
    assert call(frm=rs.from_struct(p, S, None, ok)) == -1 and "dTrialSnapshot is NULL" in why()
    assert call(l=ws.struct(live, 0, 1, without=("dLand",))) == -1
    alias = dict(live)
    alias["dListTB"] = pool["dListT"]
    assert call(l=ws.struct(alias, 0, 1)) == -1 and "also a live array" in why()
    assert call(f=rs.refill_struct(start, trial, 0), frm=rs.from_struct(p, S, None, None)) == 0        # (an empty queue: nothing to do)


def test_host_form_under_sanitizers(tmp_path):
    """the host form's loop (csrc/cmpc_contacts.h, what cmpc_rollout_refill_restore runs) from a stand-alone program with its own main, built with
    -fsanitize=address,undefined: no report, and the rows written down by hand (pool word e of array i holds 1000 (i + 1) + e; rows of 1, 9 and 70 words)"""
    import __graft_entry__ as ge
    # the clang++ beside the hipcc that built the library (its sanitizer runtimes are linked statically); no compiler is a failure, not a skip
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(ge.HIPCC) or ge.HIPCC)))
    cxx = next((p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(p)), None)
    assert cxx is not None, f"no clang++ under {rocm}"
    exe = str(tmp_path / "refill_restore_host_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", ge.CSRC, os.path.join(ROOT, "tests", "refill_restore_host_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    poison = str(0xA5A5A5A5)
    row2 = "first 1002 2018 3140 last 1002 2026 3209"
    untouched = f"first {poison} {poison} {poison} last {poison} {poison} {poison}"
    assert r.stdout.splitlines() == [
        "slot 0 end -1 code 9 " + row2,
        "slot 1 end -1 code 9 " + untouched,
        "slot 2 end 8 code 0 " + untouched,
        "slot 3 end -1 code 9 " + untouched,
        "slot 4 end -1 code 9 " + row2,
        "ok -7 1 0 -7 1 -7",
        "again 3140 3209",
    ]
