"""A footstep plan and reference trajectories per trial of a refill walk, without a GPU (include/cmpc.h, cmpc_walk_refill_plans;
WalkingRollout.walk_device_refill_plans): the new symbols, the struct and the Python surface with the pinned signatures unchanged; the host form of the
plan select against a numpy restatement (tests/walk_refill_plans_ref.py) over poisoned destinations; the host form of the fold, with an order check on
values whose float64 sum depends on the order; every refusal that needs no handle; the Python refusals, raised before a GPU is touched; and both
host forms once more from a stand-alone program built with the address and undefined-behaviour sanitizers."""
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
from tests import walk_refill_plans_ref as pr
from tests import walk_refill_ref as rf
from tests import walk_refill_snapshot_ref as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK, SELECT, FOLD, FOLD_DEV = ("cmpc_rollout_walk_refill_plans_device", "cmpc_rollout_refill_plans", "cmpc_rollout_plan_fold",
                                "cmpc_rollout_plan_fold_device")
M, B, PN, KNOTS = 5, 6, 3, 23      # (rows of 40, 70, 2 and 69 words: both paths of the device's row copy have a host counterpart here)


def _why(lib):
    lib.cmpc_last_error.restype = C.c_char_p
    return lambda: lib.cmpc_last_error(None).decode()


def test_symbols_struct_and_python_surface():
    lib = cm._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    for name in (WALK, SELECT, FOLD, FOLD_DEV):
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and "int " + name + "(" in hdr, name
    body = re.search(r"typedef struct cmpc_walk_refill_plans \{(.*?)\} cmpc_walk_refill_plans;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    t = cm._capi.CmpcWalkRefillPlans
    assert names == [f[0] for f in t._fields_] == ["pool_plans", "dPoolT", "dPoolPose", "dPoolN", "dPoolCom", "dPoolH", "dTrialPlan", "dTrialPlanOk",
                                                   "dPlanT", "dPlanPose", "dPlanN", "dPlanCom", "dPlanH"]
    assert [getattr(t, n).offset for n in names] == [0] + list(range(8, 104, 8)) and C.sizeof(t) == 104 and "sizeof == 104" in hdr
    # the structs the feature sits between keep their sizes
    assert C.sizeof(cm._capi.CmpcWalkRefillTrials) == 56 and C.sizeof(cm._capi.CmpcWalkRefillSnapshot) == 32 and C.sizeof(cm._capi.CmpcWalkTapeRegroup) == 32
    ro = cm.rollout.WalkingRollout
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.walk_device_refill_plans) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "plans", "plan_of", "references", "models", "mismatch",
                                                "taped", "kwargs"]
    assert par(cm.BatchSolver.walk_refill_plans)[:4] == ["self", "pool", "plan_of", "plan"]
    assert par(cm.BatchSolver.rollout_walk_refill_plans_device)[:3] == ["self", "tick0", "ticks"] and "plans" in par(cm.BatchSolver.rollout_walk_refill_plans_device)
    assert par(cm.BatchSolver.plan_fold_device) == ["self", "index", "per_trial", "pool_rows", "out"]
    # the pinned signatures are unchanged
    assert par(cm.BatchSolver.rollout_walk_refill_device)[-1] == "trials"
    assert par(ro.walk_device_refill_trials) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "models", "mismatch", "kwargs"]
    assert par(ro.walk_device_refill_taped) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "models", "mismatch", "kwargs"]
    assert par(ro.backward_device_refill) == ["self", "w", "grad_states", "grad_X", "rot", "refs", "replan"]
    assert "plan_pool" in ro.backward_device_refill.__doc__ and "ITS OWN plan row" in ro.backward_device_refill.__doc__


def _case(seed=3):
    """B = 6 slots at tick 4 over a pool of 3 plans, a queue of 8: slot 0 spawned with row 2, slot 1 walking since tick 2 (its index is good: untouched all
    the same), slot 2 spawned with index -1, slot 3 spawned with index Pn, slot 4 spawned with row 2 again -- a repeat --, slot 5 empty with a start tick
    that matches.  Trials 6 and 7 are never started."""
    rng = np.random.default_rng(seed)
    pool = pr.pool_arrays(PN, M, KNOTS, rng)
    live = pr.live_arrays(B, M, KNOTS)
    start = np.array([4, 2, 4, 4, 4, 4], np.int32)
    trial = np.array([1, 0, 2, 3, 4, -1], np.int32)
    of = np.array([1, 2, -1, PN, 2, 0, 1, 0], np.int32)
    ok = np.full(8, -7, np.int32)
    end_tick, end_code = np.full(B, -1, np.int32), np.full(B, 9, np.int32)
    return pool, live, start, trial, of, ok, end_tick, end_code


def _rec(end_tick, end_code):
    rec = cm._capi.CmpcWalkRecord()
    rec.rows, rec.dEndTick, rec.dEndCode = 1, end_tick.ctypes.data, end_code.ctypes.data
    return rec


@pytest.mark.parametrize("traj", [True, False])
def test_host_select_against_the_numpy_restatement(traj):
    lib = cm._capi.lib()
    pool, live, start, trial, of, ok, end_tick, end_code = _case()
    want, want_ok, want_end, want_code = pr.select(pool, live, 4, start, trial, of, ok, end_tick, end_code, traj=traj)
    before = {k: v.copy() for k, v in pool.items()}
    c, f, rec = pr.plans_struct(pool, live, of, ok, traj=traj), rs.refill_struct(start, trial, 8), _rec(end_tick, end_code)
    assert getattr(lib, SELECT)(B, M, 4, C.byref(f), C.byref(c), C.byref(rec), KNOTS) == 0, _why(lib)()
    assert ok.tolist() == want_ok.tolist() == [-7, 1, 0, 0, 1, -7, -7, -7]
    assert end_tick.tolist() == want_end.tolist() == [-1, -1, 0, 0, -1, -1] and end_code.tolist() == want_code.tolist() == [9, 9, 0, 0, 9, 9]
    for k in want:
        assert (rf.bits(live[k]) == rf.bits(want[k])).all(), k
    for k in pool:
        assert (rf.bits(pool[k]) == rf.bits(before[k])).all(), k
    # ---- written down from the contract, independently of the restatement: memory outside the spawned slots' rows keeps the fill pattern
    for k in live:
        copied = k in pr.LISTS or traj
        for b in range(-1, B + 1):
            row = live[k][1 + b:2 + b]
            if b in (0, 4) and copied:
                assert (rf.bits(row[0]) == rf.bits(pool[k][2])).all(), (k, b)
            else:
                assert (row.view(np.uint8) == pr.POISON).all(), (k, b)
    # ---- another tick: nobody's start tick matches -- nothing moves, with and without the flags
    after = {k: v.copy() for k, v in live.items()}
    for flags in (ok, None):
        c2 = pr.plans_struct(pool, live, of, flags, traj=traj)
        ok_before = ok.copy()
        assert getattr(lib, SELECT)(B, M, 5, C.byref(f), C.byref(c2), C.byref(rec), KNOTS) == 0
        assert (ok == ok_before).all() and end_tick.tolist() == want_end.tolist()
        for k in live:
            assert (rf.bits(live[k]) == rf.bits(after[k])).all(), k
    # an empty queue: nothing to do, and no index array is needed
    c3 = pr.plans_struct(pool, live, None, None, traj=traj)
    assert getattr(lib, SELECT)(B, M, 4, C.byref(rs.refill_struct(start, trial, 0)), C.byref(c3), C.byref(rec), KNOTS) == 0


def test_host_select_refuses():
    lib = cm._capi.lib()
    why = _why(lib)
    pool, live, start, trial, of, ok, end_tick, end_code = _case()
    f, rec = rs.refill_struct(start, trial, 8), _rec(end_tick, end_code)
    good = pr.plans_struct(pool, live, of, ok)
    call = lambda c=good, f=f, rec=rec, b=B, m=M, t=4, n=KNOTS: getattr(lib, SELECT)(b, m, t, C.byref(f) if f is not None else None,
                                                                                   C.byref(c) if c is not None else None,
                                                                                   C.byref(rec) if rec is not None else None, n)
    assert call() == 0
    assert call(c=None) == -1 and call(f=None) == -1 and call(rec=None) == -1
    assert call(b=0) == -1 and call(m=0) == -1 and call(t=-1) == -1 and call(n=0) == -1
    assert call(c=pr.plans_struct(pool, live, of, ok, traj=False), n=0) == 0       # (plan_knots is read with pool trajectories only)
    kept = (end_tick.copy(), ok.copy(), {k: v.copy() for k, v in live.items()})      # (a refused call writes nothing)
    assert call(c=pr.plans_struct(pool, live, of, ok, pool_plans=0)) == -1 and "pool_plans must be at least 1" in why()
    assert call(c=pr.plans_struct(pool, live, of, ok, without=("dPoolPose",))) == -1 and "a pool list array is NULL" in why()
    assert call(c=pr.plans_struct(pool, live, None, ok)) == -1 and "dTrialPlan is NULL" in why()
    assert call(c=pr.plans_struct(pool, live, of, ok, without=("dPoolH",))) == -1 and "both or neither" in why()
    assert call(c=pr.plans_struct(pool, live, of, ok, without=("dPlanN",))) == -1 and "a writable view is NULL" in why()
    assert call(c=pr.plans_struct(pool, live, of, ok, without=("dPlanCom",))) == -1 and "a writable view is NULL" in why()
    alias = pr.plans_struct(pool, live, of, ok)
    alias.dPlanT = pool["T"].ctypes.data
    assert call(c=alias) == -1 and "also a live array" in why()
    assert (end_tick == kept[0]).all() and (ok == kept[1]).all() and all((rf.bits(live[k]) == rf.bits(kept[2][k])).all() for k in live)


def test_host_fold_against_the_numpy_restatement():
    lib = cm._capi.lib()
    rng = np.random.default_rng(8)
    Q, words, rows = 11, 6 * M, 4
    per = rng.normal(size=(Q, 2, M, 3))
    index = np.array([0, 2, 0, 7, 2, -1, 0, 2, 0, 4, 2], np.int32)       # row 1 and row 3 are empty; 7, -1 and 4 lie outside the pool
    # an order check: 1e16, 1, -1e16, 1 in trials 0, 2, 6, 8 of row 0.  Ascending: ((1e16 + 1) - 1e16) + 1 = 1; any order that pairs the large values first gives 2
    per[[0, 2, 6, 8], 0, 0, 0] = [1e16, 1.0, -1e16, 1.0]
    assert (((0.0 + 1e16) + 1.0) - 1e16) + 1.0 == 1.0 and ((1e16 - 1e16) + 1.0) + 1.0 == 2.0
    per[3] = np.nan         # a trial whose index lies outside the pool
    per[9, 1] = np.inf      # another
    per[1, 0, 1, 2] = np.nan    # a member of row 2: its NaN reaches row 2's entry and nothing else
    per[4, 1, 0, 0] = -0.0
    out = np.full((rows, 2, M, 3), 123.0)
    assert getattr(lib, FOLD)(Q, words, index.ctypes.data, per.ctypes.data, rows, out.ctypes.data) == 0, _why(lib)()
    want = pr.fold(index, per, rows)
    assert (rf.bits(out) == rf.bits(want)).all()
    assert out[0, 0, 0, 0] == 1.0
    assert (rf.bits(out[[1, 3]]) == 0).all()                                  # an empty row is +0.0, written whole
    nan = np.isnan(out)
    assert nan.sum() == 1 and nan[2, 0, 1, 2] and np.isfinite(out[0]).all()
    # by hand, one entry: row 2 holds trials 1, 4, 7, 10, added in that order from +0.0
    e = (1, 2, 1)
    assert out[(2,) + e] == (((0.0 + per[(1,) + e]) + per[(4,) + e]) + per[(7,) + e]) + per[(10,) + e]
    # no trials at all: zeros, and no arrays needed
    out[:] = 5.0
    assert getattr(lib, FOLD)(0, words, None, None, rows, out.ctypes.data) == 0 and (rf.bits(out) == 0).all()
    # the refusals (the device form's that need no handle are the same, ahead of its handle check)
    why = _why(lib)
    for fn, tail in ((getattr(lib, FOLD), ()), (lambda *a: getattr(lib, FOLD_DEV)(None, *a), (None,))):
        call = lambda q=Q, w=words, i=index.ctypes.data, p=per.ctypes.data, r=rows, o=out.ctypes.data: fn(q, w, i, p, r, o, *tail)
        assert call(q=-1) == -1 and call(w=0) == -1 and call(r=0) == -1 and "pool_rows < 1" in why()
        assert call(o=None) == -1 and call(i=None) == -1 and call(p=None) == -1 and "a NULL array" in why()
        assert call(o=per.ctypes.data) == -1 and "dOut is also dPerTrial" in why()
        assert call(w=1 << 20, r=1 << 12) == -1 and "entries" in why()
    assert getattr(lib, FOLD_DEV)(None, Q, words, index.ctypes.data, per.ctypes.data, rows, out.ctypes.data, None) == -1 and "null handle" in why()


def _walk_c(lib, m, io, rec, f, trials, plans, tape=None):
    out = C.c_int(0)
    ref = lambda x: C.byref(x) if x is not None else None
    return getattr(lib, WALK)(None, m, 0, 1, ref(io), ref(rec), ref(f), ref(trials), ref(plans), 0, 0, C.byref(out), ref(tape), 0, None)


def _io(live, traj=True):
    """a cmpc_walk_io whose planner pointers are the views of pr.plans_struct(...)"""
    io = cm._capi.CmpcWalkIO()
    io.tick.dPlanT, io.tick.dPlanPose, io.tick.dPlanN = (live[k][1:].ctypes.data for k in pr.LISTS)
    if traj:
        io.tick.dPlanCom, io.tick.dPlanH, io.tick.plan_knots = live["Com"][1:].ctypes.data, live["H"][1:].ctypes.data, KNOTS
    return io


def test_walk_refusals_need_no_gpu():
    lib = cm._capi.lib()
    why = _why(lib)
    a = rf.arrays(B, 8, rows=2, seed=9)
    rec, f = rf.structs(a, 3)
    assert lib.cmpc_rollout_refill_init(B, C.byref(f)) == 0
    spare = a["state0"].ctypes.data
    pool, live, _, _, of, ok, _, _ = _case()
    good, io = pr.plans_struct(pool, live, of, ok), _io(live)
    T = cm._capi.CmpcWalkRefillTrials
    # ---- what the taped refill call refuses stays refused, in its order, with plans absent and with a good one
    for plans in (None, good):
        assert _walk_c(lib, 17, io, rec, f, None, plans) == -1 and "max_contacts must be 1 .. 16" in why()
        assert _walk_c(lib, 0, io, rec, f, None, plans) == -1 and "max_contacts must be 1 .. 16" in why()
        assert _walk_c(lib, M, None, rec, f, None, plans) == -1 and "null argument" in why()
        assert _walk_c(lib, M, io, None, f, None, plans) == -1 and "null argument" in why()
        assert _walk_c(lib, M, io, rec, None, None, plans) == -1 and "null argument" in why()
        assert _walk_c(lib, M, io, rec, f, T(None, None, None, -1, None, 0, None), plans) == -1 and "negative count" in why()
        assert _walk_c(lib, M, io, rec, f, T(None, None, spare, 0, None, 0, None), plans) == -1 and "schedule with no rows" in why()
        assert _walk_c(lib, M, io, rec, f, T(None, spare, None, 0, None, 0, None), plans) == -1 and "dModelOk without dModels" in why()
        assert _walk_c(lib, M, io, rec, f, None, plans, tape=cm._capi.CmpcWalkTape()) == -1 and "incomplete tape" in why()
        assert _walk_c(lib, M, io, rec, f, None, plans) == -1 and "null handle" in why()
        io2 = _io(live)
        io2.dWrenchTicks, io2.wrench_ticks = spare, 1
        assert _walk_c(lib, M, io2, rec, f, None, plans) == -1 and "dWrenchTicks is not taken" in why()
    # ... and they come ahead of the new ones
    bad = pr.plans_struct(pool, live, of, ok, pool_plans=0)
    assert _walk_c(lib, 17, io, rec, f, None, bad) == -1 and "max_contacts must be 1 .. 16" in why()
    assert _walk_c(lib, M, io, rec, f, None, bad, tape=cm._capi.CmpcWalkTape()) == -1 and "incomplete tape" in why()

    # ---- the new refusals, each named, none needing a handle
    def new(plans, words, f=f, io=io):
        assert _walk_c(lib, M, io, rec, f, None, plans) == -1 and WALK in why() and words in why(), (words, why())

    for n in (0, -2):
        new(pr.plans_struct(pool, live, of, ok, pool_plans=n), "pool_plans must be at least 1")
    for k in pr.LISTS:
        new(pr.plans_struct(pool, live, of, ok, without=("dPool" + k,)), "a pool list array is NULL")
    new(pr.plans_struct(pool, live, None, ok), "dTrialPlan is NULL")
    _, f0 = rf.structs(a, 3, trials=0)      # (an empty queue needs no indices: on to the handle check)
    assert _walk_c(lib, M, io, rec, f0, None, pr.plans_struct(pool, live, None, None)) == -1 and "null handle" in why()
    for k in pr.TRAJ:
        new(pr.plans_struct(pool, live, of, ok, without=("dPool" + k,)), "both or neither")
    new(good, "pool trajectories need io->tick.dPlanCom and dPlanH", io=_io(live, traj=False))
    for k in pr.LISTS + pr.TRAJ:
        new(pr.plans_struct(pool, live, of, ok, without=("dPlan" + k,)), "a writable view is not io's pointer")
        other = pr.plans_struct(pool, live, of, ok)
        setattr(other, "dPlan" + k, spare)
        new(other, "a writable view is not io's pointer")
    # without pool trajectories the trajectory views are not read
    assert _walk_c(lib, M, io, rec, f, None, pr.plans_struct(pool, live, of, ok, traj=False)) == -1 and "null handle" in why()
    # a pool array that is also a live array: a view, a list buffer of either set
    io3, alias = _io(live), pr.plans_struct(pool, live, of, ok)
    io3.tick.dPlanPose = alias.dPlanPose = pool["Pose"].ctypes.data
    new(alias, "a pool array is also a live array", io=io3)
    for field in ("dListTB", "tick.dListN"):
        io4 = _io(live)
        if field == "dListTB":
            io4.dListTB = pool["T"].ctypes.data
        else:
            io4.tick.dListN = pool["N"].ctypes.data
        new(good, "a pool array is also a live array", io=io4)
    # what passes them all reaches the handle check (dTrialPlanOk is optional)
    assert _walk_c(lib, M, io, rec, f, None, pr.plans_struct(pool, live, of, None)) == -1 and "null handle" in why()


def test_python_refusals_before_anything_touches_a_gpu():
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    ro = types.SimpleNamespace(M=8, cfg=cfg, force_sample_time=False)
    walk = cm.rollout.WalkingRollout.walk_device_refill_plans
    plans = [cm.rollout.walking_plan(cfg), cm.rollout.walking_plan(cfg, steps=4)]
    of = np.zeros(3, np.int32)
    z = np.zeros((3, 3), np.float32)
    for kw in (dict(replan={2: None}), dict(every=4), dict(snapshot=dict(tick=3))):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            walk(ro, 4, 2, z, z, z, plans, of, **kw)
    with pytest.raises(NotImplementedError, match="16 contacts"):
        walk(types.SimpleNamespace(M=17, cfg=cfg, force_sample_time=False), 4, 2, z, z, z, plans, of)
    with pytest.raises(ValueError, match="more than the roll-out's M - 1"):
        walk(types.SimpleNamespace(M=4, cfg=cfg, force_sample_time=False), 4, 2, z, z, z, plans, of)
    for kw in (dict(no_such_argument=1), dict(skip_ended=True), dict(mismatch=dict(gain=np.ones(3)))):
        with pytest.raises(TypeError):
            walk(ro, 4, 2, z, z, z, plans, of, **kw)
    with pytest.raises(ValueError, match="tick_first"):
        walk(ro, 4, 2, z, z, z, plans, of, mismatch=dict(force_gain=np.ones(3), tick_first=2))
    with pytest.raises(ValueError, match="not both"):
        walk(ro, 4, 2, z, z, z, plans, of, push=z, wrench_trials=np.zeros((1, 3, 10, 6)))
    with pytest.raises(ValueError, match="a row per plan"):
        walk(ro, 4, 2, z, z, z, plans, of, references=dict(com=np.zeros((3, 9, 3)), h=np.zeros((3, 9, 3)), in_dt=0.06))
    with pytest.raises(ValueError, match="references = dict"):
        walk(ro, 4, 2, z, z, z, plans, of, references=dict(com=np.zeros((2, 9, 3)), h=np.zeros((2, 9, 3))))
    with pytest.raises(ValueError, match="references go with plans"):
        walk(ro, 4, 2, z, z, z, None, of, references=dict(com=np.zeros((2, 9, 3)), h=np.zeros((2, 9, 3)), in_dt=0.06))
    # the pool is padded the way the roll-out pads its own plan: zero times, the identity pose, the counts kept
    t, pose, n = cm.rollout.WalkingRollout.plan_pool(ro, plans)
    assert t.shape == (2, 2, 8, 2) and pose.shape == (2, 2, 8, 7) and n.tolist() == [[4, 4], [3, 3]]
    assert (t[1, :, 3:] == 0).all() and (pose[1, :, 3:] == np.array([0, 0, 0, 1, 0, 0, 0], np.float32)).all()
    t2, pose2, n2 = cm.rollout.WalkingRollout.plan_pool(ro, (t[:, :, :4], pose[:, :, :4], n))       # packed arrays, shorter than M
    assert (rf.bits(t2) == rf.bits(t)).all() and (rf.bits(pose2) == rf.bits(pose)).all() and (n2 == n).all()
    with pytest.raises(ValueError, match="more than the roll-out's M - 1"):
        cm.rollout.WalkingRollout.plan_pool(ro, (t, pose, np.full((2, 2), 8, np.int32)))


def test_host_forms_under_sanitizers(tmp_path):
    """the host forms' loops (csrc/cmpc_contacts.h, what cmpc_rollout_refill_plans and cmpc_rollout_plan_fold run) from a stand-alone program with its own
    main, built with -fsanitize=address,undefined: no report, and the rows written down by hand (pool word e of array i holds 1000 (i + 1) + e; rows of 40,
    70, 2, 69 and 69 words; the fold's row 0 is ((1e16 + 1) - 1e16) + 1 = 1 in ascending order)"""
    import __graft_entry__ as ge
    # the clang++ beside the hipcc that built the library (its sanitizer runtimes are linked statically); no compiler is a failure, not a skip
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(ge.HIPCC) or ge.HIPCC)))
    cxx = next((p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(p)), None)
    assert cxx is not None, f"no clang++ under {rocm}"
    exe = str(tmp_path / "refill_plans_host_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", ge.CSRC, os.path.join(ROOT, "tests", "refill_plans_host_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    poison = " ".join([str(0xA5A5A5A5)] * 5)
    row2 = "first 1080 2140 3004 4138 5138 last 1119 2209 3005 4206 5206"
    untouched = f"first {poison} last {poison}"
    assert r.stdout.splitlines() == [
        "slot 0 end -1 code 9 " + row2,
        "slot 1 end -1 code 9 " + untouched,
        "slot 2 end 0 code 0 " + untouched,
        "slot 3 end -1 code 9 " + untouched,
        "slot 4 end -1 code 9 " + row2,
        "ok -7 1 0 -7 1 -7",
        "again 2140 2209",
        "fold 1.0 44.0 48.0 0.0 0.0 0.0 20.0 22.0 24.0",
    ]
