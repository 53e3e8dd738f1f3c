"""The refill walk taped and its tape regrouped by trial, without a GPU (include/cmpc.h, cmpc_rollout_walk_refill_taped_device and cmpc_walk_tape_regroup;
WalkingRollout.walk_device_refill_taped, refill_trial_walk, backward_device_refill): the new symbols, the struct and the Python surface with the pinned
signatures unchanged; the host form of the regroup against a numpy restatement (tests/walk_refill_tape_ref.py) on a synthetic slot-major tape of random
bits whose assignment table comes from the refill tests' model; every refusal that comes before anything touches a GPU; and the host form once more from a
stand-alone program built with the address and undefined-behaviour sanitizers."""
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
from tests import walk_refill_tape_ref as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPED, DEVICE, HOST = "cmpc_rollout_walk_refill_taped_device", "cmpc_rollout_tape_regroup_device", "cmpc_rollout_tape_regroup"
N, M, B, Q, TT, TICKS = 10, 5, 4, 10, 6, 9
# trial 1 ends at its local tick 0, trial 2 mid-way at 3; in a walk of 9 ticks trials 5 .. 8 are cut off by the walk's end and trial 9 never starts
END_LOCAL = [-1, 0, 3, -1, -1, -1, -1, -1, -1, -1]


def test_symbols_struct_and_python_surface():
    lib = cm._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    for name in (TAPED, DEVICE, HOST):
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and "int " + name + "(" in hdr, name
    body = re.search(r"typedef struct cmpc_walk_tape_regroup \{(.*?)\} cmpc_walk_tape_regroup;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    t = cm._capi.CmpcWalkTapeRegroup
    assert names == [f[0] for f in t._fields_] == ["tick_first", "dTrialIndex", "dEndOut", "dOkOut"]
    assert [getattr(t, n).offset for n in names] == [0, 8, 16, 24] and C.sizeof(t) == 32 and "sizeof(cmpc_walk_tape_regroup) == 32" in hdr
    # the structs the feature sits between keep their sizes
    assert C.sizeof(cm._capi.CmpcWalkTape) == 8 + 11 * 8 + 8 + 3 * 4 + 4 and C.sizeof(cm._capi.CmpcWalkRefillTrials) == 56
    assert C.sizeof(cm._capi.CmpcWalkRefill) == 8 + 8 * 5 + 8 + 8 * 9 + 16
    # the Python surface
    ro = cm.rollout.WalkingRollout
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.walk_device_refill_taped) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "models", "mismatch", "kwargs"]
    assert par(ro.refill_trial_walk) == ["self", "w", "trials"]
    assert par(ro.backward_device_refill)[:4] == ["self", "w", "grad_states", "grad_X"]
    assert par(cm.BatchSolver.tape_regroup_device)[:5] == ["self", "src_tape", "refill", "trial_index", "dst_tape"]
    assert {"tape", "tape_row0"} <= set(par(cm.BatchSolver.rollout_walk_refill_device))
    # the pinned signatures are unchanged
    assert par(cm.BatchSolver.rollout_walk_refill_device)[-1] == "trials"
    assert par(ro.walk_device_refill_trials) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "models", "mismatch", "kwargs"]
    assert par(ro.walk_device_refill) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "push", "push_ticks", "wrench_trials", "trace", "stop",
                                          "replan", "mismatch", "taped", "every"]
    assert par(ro.backward_device) == ["self", "w", "grad_states", "grad_X"]
    assert '["trials"]["slot"]' in ro.backward_device_refill.__doc__     # (the plan gradient is the slot's: the docstring says how to sum it)


def _table():
    m = rf.assignment_model(B, Q, TT, TICKS, END_LOCAL)
    return m["slot"].astype(np.int32), m["start"].astype(np.int32), m["ticks"].astype(np.int32), m["end_tick"].astype(np.int32)


# the calls of the host-form test: (tick_first, the columns' trial indices).  With tick_first = 1 the source is the tape from its row 1 on, so the trials
# that started at tick 0 need a row in front of the tape
CALLS = ((0, (1, 2, 5, 9)), (0, (2, 2, -1, Q)), (0, (0, 3, 6, 8)), (1, (0, 4, 5, 7)), (1, (8, 1, 9, 6)))


def test_host_form_against_the_numpy_restatement():
    lib = cm._capi.lib()
    slot, start, ticks, end = _table()
    # ---- every kind the rule names is in the table, asserted before anything is compared
    assert end[1] == 0 and ticks[1] == 1, "a trial ended at local tick 0"
    assert 0 < end[2] < TT - 1 and ticks[2] == end[2] + 1, "a trial ended mid-way"
    cut = [q for q in range(Q) if end[q] < 0 and 0 < ticks[q] < TT]
    assert cut and all(start[q] + ticks[q] == TICKS for q in cut), "a trial cut off by the walk's end"
    assert ticks[9] == 0 and slot[9] == -1 and start[9] == -1, "a trial never started"
    through = [q for q in range(Q) if end[q] < 0 and ticks[q] == TT]
    assert through, "a trial walked through"
    flat = [(tf, q) for tf, idx in CALLS for q in idx]
    assert any(len(set(idx)) < len(idx) for _, idx in CALLS), "a repeated index"
    assert any(q == -1 for _, q in flat) and any(q == Q for _, q in flat), "an index of -1 and of Q"
    kinds = {(tf, q): rt.kind(q, Q, B, TICKS - tf, TT, tf, slot, start, ticks) for tf, q in flat}
    outside = [(tf, q) for (tf, q), k in kinds.items() if k == "none" and 0 <= q < Q]
    assert outside and all(tf == 1 and start[q] == 0 for tf, q in outside), "a tick_first that puts a trial's rows outside the source tape"
    assert any(k == "started" for (tf, _), k in kinds.items() if tf == 1), "a trial inside the shifted tape"
    for q in (1, 2, 9, cut[0], through[0]):
        assert (0, q) in kinds, q

    rng = np.random.default_rng(71)
    tape = rt.arrays(N, M, TICKS, B, rng)
    state0 = np.frombuffer(rng.integers(0, 256, Q * 36, dtype=np.uint8).tobytes(), np.float32).reshape(Q, 9).copy()
    f = rt.refill_struct(TT, state0, slot, start, ticks, end)
    for tf, idx in CALLS:
        src = {k: np.ascontiguousarray(v[tf:]) for k, v in tape.items()}
        before = {k: v.copy() for k, v in src.items()}
        dst = rt.arrays(N, M, TT, B)
        index = np.array(idx, np.int32)
        end_out, ok_out = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
        want, want_end, want_ok = rt.expected(src, dst, TICKS - tf, TT, tf, idx, state0, slot, start, ticks, end)
        s, d, g = rt.struct(src, TICKS - tf), rt.struct(dst, TT), rt.regroup_struct(tf, index, end_out, ok_out)
        assert getattr(lib, HOST)(N, B, M, C.byref(s), C.byref(f), C.byref(g), C.byref(d)) == 0
        assert end_out.tolist() == want_end.tolist() and ok_out.tolist() == want_ok.tolist(), (tf, idx)
        for k in want:
            assert (rt.bits(dst[k]) == rt.bits(want[k])).all(), (tf, idx, k)
        for k in src:
            assert (rt.bits(src[k]) == rt.bits(before[k])).all(), k
        # ---- written down from the contract, independently of the restatement: the end tick and the flag of every kind, and the sentinel
        for j, q in enumerate(idx):
            what = kinds[(tf, q)]
            col = {k: np.ascontiguousarray(dst[k][:, j]) for k in dst}
            if what == "none":
                assert end_out[j] == 0 and ok_out[j] == 0
                assert all((v.view(np.uint8) == rt.SENTINEL).all() for v in col.values()), (tf, q)
            elif what == "never":
                assert end_out[j] == 0 and ok_out[j] == 1 and q == 9
                assert (rt.bits(col["dStates"][0]) == rt.bits(state0[q])).all() and (col["dStates"][1:].view(np.uint8) == rt.SENTINEL).all()
                assert all((v.view(np.uint8) == rt.SENTINEL).all() for k, v in col.items() if k != "dStates"), (tf, q)
            else:
                assert ok_out[j] == 1
                assert end_out[j] == (end[q] if end[q] >= 0 else ticks[q] if ticks[q] < TT else -1)
                assert (rt.bits(col["dStates"][0]) == rt.bits(state0[q])).all()
                assert not any((v.view(np.uint8) == rt.SENTINEL).all() for v in col.values()), (tf, q)      # (no array left out)
                n, t0 = int(ticks[q]), int(start[q]) - tf
                for k in ("dX", "dLamG", "dListT", "dOk"):
                    assert (rt.bits(col[k][n - 1]) == rt.bits(src[k][t0 + n - 1, slot[q]])).all(), k
                    assert all((rt.bits(col[k][r]) == rt.bits(col[k][n - 1])).all() for r in range(n, TT)), k      # the last recorded row repeats
                assert (rt.bits(col["dStates"][n]) == rt.bits(src["dStates"][t0 + n, slot[q]])).all()
                assert (col["dPlanT"][0].view(np.uint64) == 0).all() and (col["dPlanN"][0] == 0).all()
                if n > 1:
                    assert (rt.bits(col["dPlanT"][1]) == rt.bits(src["dPlanT"][t0 + 1, slot[q]])).all()
    # the pinned expectations of the kinds, by hand: trial 1 -> 0, trial 2 -> 3, the cut-off trials -> their ticks, trial 9 -> 0, a trial walked through -> -1
    assert [int(end[q]) if end[q] >= 0 else int(ticks[q]) if ticks[q] < TT else -1 for q in range(Q)] == [-1, 0, 3, -1, -1, 5, 3, 3, 2, 0]


def _good():
    slot, start, ticks, end = _table()
    src, dst = rt.arrays(N, M, TICKS, B), rt.arrays(N, M, TT, B)
    state0 = np.zeros((Q, 9), np.float32)
    index, end_out, ok_out = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    keep = (slot, start, ticks, end, src, dst, state0, index, end_out, ok_out)
    return keep, rt.struct(src, TICKS), rt.refill_struct(TT, state0, slot, start, ticks, end), rt.regroup_struct(0, index, end_out, ok_out), rt.struct(dst, TT)


def test_regroup_refusals_need_no_gpu():
    lib = cm._capi.lib()
    lib.cmpc_last_error.restype = C.c_char_p
    why = lambda: lib.cmpc_last_error(None).decode()
    keep, s, f, g, d = _good()
    slot, start, ticks, end, src, dst, state0, index, end_out, ok_out = keep
    ref = lambda x: C.byref(x) if x is not None else None

    def both(words, s=s, f=f, g=g, d=d, m=M):
        assert getattr(lib, HOST)(N, B, m, ref(s), ref(f), ref(g), ref(d)) == -1 and HOST in why() and words in why(), (words, why())
        assert getattr(lib, DEVICE)(None, m, ref(s), ref(f), ref(g), ref(d), None) == -1 and DEVICE in why() and words in why(), (words, why())

    assert getattr(lib, HOST)(N, B, M, ref(s), ref(f), ref(g), ref(d)) == 0
    assert getattr(lib, DEVICE)(None, M, ref(s), ref(f), ref(g), ref(d), None) == -1 and "null handle" in why()      # (what passes them all)
    for kw in (dict(s=None), dict(f=None), dict(g=None), dict(d=None)):
        both("null argument", **kw)
    both("dTrialIndex or dEndOut is NULL", g=rt.regroup_struct(0, None, end_out, ok_out))
    both("dTrialIndex or dEndOut is NULL", g=rt.regroup_struct(0, index, None, ok_out))
    for field in ("dState0", "dTrialSlot", "dTrialStart", "dTrialTicks", "dTrialEndTick"):
        both("a required array of the refill is NULL", f=rt.refill_struct(TT, state0, slot, start, ticks, end, without=(field,)))
    for k, _, _ in rt.FIELDS:
        both("incomplete tape", s=rt.struct(src, TICKS, without=(k,)))
        both("incomplete tape", d=rt.struct(dst, TT, without=(k,)))
    both("incomplete tape", s=rt.struct(src, 0))
    both("incomplete tape", d=rt.struct(dst, TT, step=0.0))
    both("trial_ticks rows", d=rt.struct(dst, TT - 1))
    both("trial_ticks rows", f=rt.refill_struct(TT + 1, state0, slot, start, ticks, end))
    both("negative count of trials", f=rt.refill_struct(TT, state0, slot, start, ticks, end, trials=-1))
    for k in ("dX", "dStates", "dListN"):
        alias = dict(dst)
        alias[k] = src[k]
        both("a destination array is also a source array", d=rt.struct(alias, TT))
    both("max_contacts must be at least 1", m=0)
    # the order: an incomplete tape behind a NULL index names the index; a bad max_contacts comes last
    both("dTrialIndex or dEndOut is NULL", g=rt.regroup_struct(0, None, end_out, ok_out), s=rt.struct(src, 0), m=0)
    both("incomplete tape", s=rt.struct(src, 0), m=0)
    # dOkOut is optional, and an empty queue needs none of the per-trial arrays
    assert getattr(lib, HOST)(N, B, M, ref(s), ref(f), ref(rt.regroup_struct(0, index, end_out, None)), ref(d)) == 0
    empty = rt.refill_struct(TT, state0, slot, start, ticks, end, trials=0, without=("dState0", "dTrialSlot", "dTrialStart", "dTrialTicks", "dTrialEndTick"))
    end_out[:] = -7
    assert getattr(lib, HOST)(N, B, M, ref(s), ref(empty), ref(g), ref(d)) == 0 and end_out.tolist() == [0] * B and ok_out.tolist() == [0] * B
    assert getattr(lib, HOST)(0, B, M, ref(s), ref(f), ref(g), ref(d)) == -1 and getattr(lib, HOST)(N, 0, M, ref(s), ref(f), ref(g), ref(d)) == -1


def test_taped_walk_refusals_need_no_gpu():
    lib = cm._capi.lib()
    lib.cmpc_last_error.restype = C.c_char_p
    why = lambda: lib.cmpc_last_error(None).decode()
    a = rf.arrays(B, 7, rows=2, seed=9)
    rec, f = rf.structs(a, 3)
    spare = a["state0"].ctypes.data      # (any non-NULL address: nothing is read before the refusal)
    arr = rt.arrays(N, M, 4, B)
    T = cm._capi.CmpcWalkRefillTrials
    ref = lambda x: C.byref(x) if x is not None else None

    def walk(m, io, rec, f, trials, tape, row0=0, ticks=1):
        out = C.c_int(0)
        return getattr(lib, TAPED)(None, m, 0, ticks, ref(io), ref(rec), ref(f), ref(trials), 0, 0, C.byref(out), ref(tape), row0, None)

    def io_of(step=0.01, substeps=6, fst=0):
        io = cm._capi.CmpcWalkIO()
        io.tick.plant_step, io.tick.plant_substeps, io.tick.force_sample_time = step, substeps, fst
        return io
    good = rt.struct(arr, 4)
    # ---- the trials call's refusals, in its order, without a tape, with a good one and ahead of a bad one
    for tape in (None, good, rt.struct(arr, 0)):
        io = io_of()
        assert walk(17, io, rec, f, None, tape) == -1 and "max_contacts must be 1 .. 16" in why()
        assert walk(4, None, rec, f, None, tape) == -1 and "null argument" in why()
        assert walk(4, io, None, f, None, tape) == -1 and "null argument" in why()
        assert walk(4, io, rec, None, None, tape) == -1 and "null argument" in why()
        assert walk(4, io, rec, f, T(None, None, None, -1, None, 0, None), tape) == -1 and "negative count" in why()
        assert walk(4, io, rec, f, T(None, None, spare, 0, None, 0, None), tape) == -1 and "schedule with no rows" in why()
        assert walk(4, io, rec, f, T(None, spare, None, 0, None, 0, None), tape) == -1 and "dModelOk without dModels" in why()
        io.dWrenchTicks, io.wrench_ticks = spare, 1
        assert walk(4, io, rec, f, None, tape) == -1 and "dWrenchTicks is not taken" in why()
    # ---- the tape's refusals, each named, none needing a handle
    def new(words, tape, io=None, **kw):
        assert walk(4, io_of() if io is None else io, rec, f, None, tape, **kw) == -1 and TAPED in why() and words in why(), (words, why())
    for k, _, _ in rt.FIELDS:
        new("incomplete tape", rt.struct(arr, 4, without=(k,)))
    new("incomplete tape", rt.struct(arr, 0))
    new("incomplete tape", rt.struct(arr, 4, substeps=0))
    new("too few rows", good, row0=-1)
    new("too few rows", good, row0=4)
    new("too few rows", good, row0=2, ticks=3)
    new("scalars do not agree", good, io=io_of(step=0.02))
    new("scalars do not agree", good, io=io_of(substeps=5))
    new("scalars do not agree", good, io=io_of(fst=1))
    # what passes them all reaches the handle check; so does the call without a tape, which is the trials call
    for tape, kw in ((good, {}), (good, dict(row0=1, ticks=3)), (rt.struct(arr, 4, force_sample_time=1), dict(io=io_of(fst=3))), (None, {})):
        io = kw.pop("io", io_of())
        assert walk(4, io, rec, f, None, tape, **kw) == -1 and "null handle" in why()


def test_python_refusals_before_anything_touches_a_gpu():
    ro = types.SimpleNamespace(M=5, force_sample_time=False)
    R = cm.rollout.WalkingRollout
    z = np.zeros((3, 3))
    # the taped walk refuses what walk_device_refill_trials refuses
    with pytest.raises(ValueError, match="tick_first"):
        R.walk_device_refill_taped(ro, 4, 2, z, z, z, mismatch=dict(force_gain=np.ones(3), tick_first=3))
    with pytest.raises(NotImplementedError):
        R.walk_device_refill_taped(types.SimpleNamespace(M=17, force_sample_time=False), 4, 2, z, z, z)
    for kw in (dict(replan={2: None}), dict(taped=True), dict(every=4), dict(no_such_argument=1), dict(mismatch=dict(gain=np.ones(3)))):
        with pytest.raises(TypeError):
            R.walk_device_refill_taped(ro, 4, 2, z, z, z, **kw)
    with pytest.raises(ValueError, match="not both"):
        R.walk_device_refill_taped(ro, 4, 2, z, z, z, push=z, wrench_trials=np.zeros((1, 3, 10, 6)))
    # walk_device_refill's taped=True still raises
    with pytest.raises(NotImplementedError, match="taped"):
        R.walk_device_refill(ro, 4, 2, z, z, z, taped=True)
    # the reverse: rot, reference gradients, replan; long lists; a dict of the snapshot refill, and one without a tape
    taped = dict(tape=dict(refill=dict(trials=3), trial_ticks=2, models=None, mismatch=None))
    gs = np.zeros((3, 3, 9))
    for kw in (dict(rot=True), dict(refs=True), dict(replan={1: None})):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            R.backward_device_refill(ro, taped, gs, **kw)
    for fn, args in ((R.backward_device_refill, (gs,)), (R.refill_trial_walk, ([0, 1],))):
        with pytest.raises(NotImplementedError, match="16 contacts"):
            fn(types.SimpleNamespace(M=17, force_sample_time=False), taped, *args)
        with pytest.raises(NotImplementedError, match="snapshot"):
            fn(ro, dict(taped, tick0=8), *args)
        with pytest.raises(NotImplementedError, match="walk_device_refill_taped"):
            fn(ro, dict(trials={}), *args)
        with pytest.raises(NotImplementedError, match="walk_device_refill_taped"):
            fn(ro, dict(tape=dict(rows=4)), *args)      # (walk_device_taped's dict: no refill behind it)


def test_host_form_under_sanitizers(tmp_path):
    """the host form's loop (csrc/cmpc_contacts.h, what cmpc_rollout_tape_regroup runs) from a stand-alone program with its own main, built with
    -fsanitize=address,undefined: no report, and the words written down by hand (source word e of array i holds 1000 (i + 1) + e, state word e
    90000 + e, dState0 word e 70000 + e; rows of 1, 2, 9 and 70 words; B = 3 columns, 5 source rows, 4 destination rows)"""
    import __graft_entry__ as ge
    # the clang++ beside the hipcc that built the library (its sanitizer runtimes are linked statically); no compiler is a failure, not a skip
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(ge.HIPCC) or ge.HIPCC)))
    cxx = next((p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(p)), None)
    assert cxx is not None, f"no clang++ under {rocm}"
    exe = str(tmp_path / "refill_tape_host_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", ge.CSRC, os.path.join(ROOT, "tests", "refill_tape_host_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    p = str(0xA5A5A5A5)
    untouched = f"first {p} last {p} {p} {p} plan0 {p} state"
    through = "first 1350 last 2049 4029 10049 plan0 0 state 70000 90161"
    ended0 = "first 1070 last 1139 4003 9139 plan0 0 state 70036 90044"
    assert r.stdout.splitlines() == [
        "group 0 column 0 end -1 ok 1 " + through,
        "group 0 column 1 end 2 ok 1 first 1630 last 1909 4025 9909 plan0 0 state 70009 90143",
        f"group 0 column 2 end 0 ok 1 {untouched} 70018 {p}",
        f"group 1 column 0 end 0 ok 0 {untouched} {p} {p}",
        "group 1 column 1 end 0 ok 1 " + ended0,
        "group 1 column 2 end 0 ok 1 " + ended0,
        f"group 2 column 0 end 0 ok -7 {untouched} {p} {p}",
        f"group 2 column 1 end 0 ok -7 {untouched} {p} {p}",
        "group 2 column 2 end -1 ok -7 " + through,
    ]
