"""The refill of a walk's slots from a queue of trials without a GPU (include/cmpc.h, cmpc_walk_refill): the new symbols and the pinned signatures, the
host form cmpc_rollout_refill on hand-made records -- assignment order, archive, the spawned slots' outcome, the edge cases Q < B and Q = 0 -- every
refusal that must come before anything touches a GPU, the host form once more from a stand-alone program built with the address and
undefined-behaviour sanitizers, and the host form tick by tick against an independent model of the assignment rule (tests/walk_refill_ref.py)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_refill_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmpc_rollout_refill_init", "cmpc_rollout_refill_init_device", "cmpc_rollout_refill", "cmpc_rollout_refill_device",
       "cmpc_rollout_walk_refill_device")
B, Q, TT = 5, 7, 3


def _init(a, trial_ticks=TT, batch=None):
    rec, f = rf.structs(a, trial_ticks)
    return cm._capi.lib().cmpc_rollout_refill_init(a["trial"].shape[0] if batch is None else batch, C.byref(f))


def _refill(a, tick_next, trial_ticks=TT, live=True, tick_first=0, batch=None, **kw):
    rec, f = rf.structs(a, trial_ticks, tick_first, **kw)
    return cm._capi.lib().cmpc_rollout_refill(a["trial"].shape[0] if batch is None else batch, tick_next, C.byref(rec), C.byref(f),
                                             a["state"].ctypes.data if live else None)


def test_symbols_and_python_surface():
    lib = cm._capi.lib()
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    for name in NEW:
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and name + "(" in hdr, name
    assert "typedef struct cmpc_walk_refill {" in hdr and "typedef struct cmpc_walk_refill_trace {" in hdr
    ints, ptrs = 3, 15     # cmpc_walk_refill: trials, trial_ticks, wrench_ticks | the arrays; then the trace struct (two ints and a pointer)
    assert C.sizeof(cm._capi.CmpcWalkRefillTrace) == 16
    assert C.sizeof(cm._capi.CmpcWalkRefill) == 8 + 8 * 5 + 8 + 8 * 9 + 16 and ints + ptrs == 18
    for name in ("walk_refill", "rollout_refill_device", "rollout_walk_refill_device"):
        assert hasattr(cm.BatchSolver, name), name
    ro = cm.rollout.WalkingRollout
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.walk_device_refill) == ["self", "ticks", "trial_ticks", "com0", "dcom0", "h0", "push", "push_ticks", "wrench_trials", "trace", "stop",
                                          "replan", "mismatch", "taped", "every"]
    # the pinned signatures are unchanged
    assert par(ro.walk_device) == ["self", "ticks", "com0", "dcom0", "h0", "push", "push_ticks", "replan", "trace", "stop", "skip_ended"]
    assert par(ro.walk_device_taped) == ["self", "ticks", "com0", "dcom0", "h0", "kwargs"]
    assert par(ro.walk_resume_device) == ["self", "snapshot", "ticks", "index", "push", "push_ticks", "replan", "trace", "stop", "skip_ended", "taped", "every"]
    assert par(ro.backward_device_checkpointed) == ["self", "w", "grad_states", "grad_X", "rot"]
    assert par(cm.BatchSolver.rollout_walk_device)[:5] == ["self", "tick0", "ticks", "cold_first", "plan"]
    for doc in (ro.backward_device_checkpointed.__doc__, ro.walk_resume_device.__doc__):
        assert "Out of scope" in doc and "walk_device_refill" in doc
    assert "same batch size and factor storage" in ro.walk_resume_device.__doc__
    assert "Out of scope" in ro.walk_device_refill.__doc__
    # the existing structs keep their layout
    assert C.sizeof(cm._capi.CmpcWalkRecord) == 8 + 13 * 8 and C.sizeof(cm._capi.CmpcWalkIO) == C.sizeof(cm._capi.CmpcTickIO) + 3 * 8 + 8 + 8 + 8


def test_assignment_order_and_archive():
    """B = 5, Q = 7, trial_ticks = 3: the first fill, a call with slots 1 and 3 ended and slot 4 at trial_ticks, a call with nothing free, the archive pass
    alone.  Expectations written down from the rule."""
    a = rf.arrays(B, Q, rows=4, seed=3)
    assert _init(a) == 0
    assert a["next"][0] == 0 and (a["trial"] == -1).all() and (a["start_tick"] == 0).all()
    assert (a["q_slot"] == -1).all() and (a["q_start"] == -1).all() and (a["q_ticks"] == 0).all() and (a["q_end_tick"] == -1).all()
    assert (rf.bits(a["q_final_state"]) == rf.bits(a["state0"])).all() and np.isposinf(a["q_box_slack_min"]).all()
    # ---- the first fill: slots 0..4 <- trials 0..4
    assert _refill(a, 0) == 0
    assert a["trial"].tolist() == [0, 1, 2, 3, 4] and a["start_tick"].tolist() == [0] * 5 and a["next"][0] == 5
    assert a["trial_of"][0].tolist() == [0, 1, 2, 3, 4] and (a["trial_of"][1:].view(np.uint8) == 0x5A).all()
    assert a["q_slot"].tolist() == [0, 1, 2, 3, 4, -1, -1] and a["q_start"].tolist() == [0, 0, 0, 0, 0, -1, -1]
    for b in range(5):      # the spawned slots' outcome is cmpc_rollout_outcome_init_device's rule; the live state is the queue's
        for k, v in rf.outcome_init_rule(a["state0"][b]).items():
            assert (rf.bits(a[k][b]) == rf.bits(v)).all(), (k, b)
        assert (rf.bits(a["state"][b]) == rf.bits(a["state0"][b])).all()
    # ---- hand-made: slots 0..3 as if spawned at tick 1, three ticks recorded; slots 1 and 3 ended at local tick 1; slot 4 (start 0) is at trial_ticks
    rng = np.random.default_rng(5)
    a["start_tick"][:4] = 1
    a["end_tick"][[1, 3]] = 1
    a["end_code"][[1, 3]] = 3
    a["iterations_sum"][:] = [11, 12, 13, 14, 15]
    a["iterations_max"][:] = [6, 7, 8, 9, 10]
    a["final_state"][:] = rng.normal(size=(5, 9)).astype(np.float32)
    a["final_state"].view(np.uint32)[2, 4] = 0xFFC00055      # (NaN payloads and -0.0 are archived as bits)
    a["final_state"][0, 0] = -0.0
    a["box_slack_min"][:] = [0.5, 0.25, np.inf, -0.125, 1.5]
    before = {k: v.copy() for k, v in a.items()}
    assert _refill(a, 3) == 0
    for q, b in enumerate(range(5)):     # the archive: trial q sat in slot q
        for _, k, _, _ in rf.REC:
            assert (rf.bits(a["q_" + k][q]) == rf.bits(before[k][b])).all(), (k, q)
    assert a["q_ticks"].tolist() == [2, 2, 2, 2, 3, 0, 0]
    assert a["trial"].tolist() == [0, 5, 2, 6, -1] and a["start_tick"].tolist() == [1, 3, 1, 3, 0] and a["next"][0] == 7
    assert a["q_slot"].tolist() == [0, 1, 2, 3, 4, 1, 3] and a["q_start"].tolist() == [0, 0, 0, 0, 0, 3, 3]
    assert a["trial_of"][3].tolist() == [0, 5, 2, 6, -1]
    assert a["end_tick"].tolist() == [-1, -1, -1, -1, 3]       # (slot 4: exhausted, out of every later launch through the ended mask)
    for b, q in ((1, 5), (3, 6)):
        for k, v in rf.outcome_init_rule(a["state0"][q]).items():
            assert (rf.bits(a[k][b]) == rf.bits(v)).all(), (k, b)
        assert (rf.bits(a["state"][b]) == rf.bits(a["state0"][q])).all()
    for b in (0, 2):        # the slots that walk on are untouched; slot 4 keeps everything but its trial and end tick
        for k in [k for _, k, _, _ in rf.REC] + ["state"]:
            assert (rf.bits(a[k][b]) == rf.bits(before[k][b])).all(), (k, b)
    for k in ("end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min", "state"):
        assert (rf.bits(a[k][4]) == rf.bits(before[k][4])).all(), k
    # ---- nothing free: only the archive moves
    a["iterations_sum"][0] += 7
    before = {k: v.copy() for k, v in a.items()}
    assert _refill(a, 3) == 0
    assert a["q_iterations_sum"][0] == 18
    for k in a:
        if k != "q_iterations_sum":
            assert (rf.bits(a[k]) == rf.bits(before[k])).all(), k
    # ---- the archive pass alone (dStateLive NULL): the tick counts move, nothing is handed out and no trace row is written
    a["end_tick"][0] = 2
    before = {k: v.copy() for k, v in a.items()}
    assert _refill(a, 4, live=False, tick_first=4) == 0
    assert a["q_ticks"].tolist() == [3, 2, 3, 2, 3, 1, 1] and a["q_end_tick"][0] == 2
    for k in a:
        if k not in ("q_ticks", "q_end_tick"):
            assert (rf.bits(a[k]) == rf.bits(before[k])).all(), k


def test_fewer_trials_than_slots_and_none():
    a = rf.arrays(5, 2, rows=1, seed=7)
    a["end_tick"][:] = -1        # (as cmpc_rollout_outcome_init_device leaves a record: the empty slots' words are set)
    assert _init(a) == 0 and _refill(a, 0) == 0
    assert a["trial"].tolist() == [0, 1, -1, -1, -1] and a["end_tick"].tolist() == [-1, -1, 0, 0, 0] and a["next"][0] == 2
    assert a["trial_of"][0].tolist() == [0, 1, -1, -1, -1] and a["q_slot"].tolist() == [0, 1]
    # a later call leaves the empty slots' word as it is
    assert _refill(a, 1, tick_first=1) == 0
    assert a["end_tick"].tolist() == [-1, -1, 0, 0, 0] and a["trial"].tolist() == [0, 1, -1, -1, -1] and a["q_ticks"].tolist() == [1, 1]
    # Q = 0: every slot is out at once, and the per-trial arrays are not needed
    a = rf.arrays(5, 0, rows=1, seed=8)
    a["end_tick"][:] = -1
    state = a["state"].copy()
    none = tuple(k for _, k, _, _ in rf.TRIAL) + ("state0",)
    rec, f = rf.structs(a, TT, tick_first=2, without=none)
    lib = cm._capi.lib()
    assert lib.cmpc_rollout_refill_init(5, C.byref(f)) == 0
    assert lib.cmpc_rollout_refill(5, 2, C.byref(rec), C.byref(f), a["state"].ctypes.data) == 0
    assert a["trial"].tolist() == [-1] * 5 and a["end_tick"].tolist() == [2] * 5 and a["next"][0] == 0 and a["trial_of"][0].tolist() == [-1] * 5
    assert (rf.bits(a["state"]) == rf.bits(state)).all()


def test_refusals_need_no_gpu():
    lib = cm._capi.lib()
    a = rf.arrays(B, Q, rows=2, seed=9)
    assert _init(a) == 0 and _refill(a, 0) == 0
    # the host form's argument checks
    assert _refill(a, -1) == -1 and _refill(a, 0, trial_ticks=0) == -1 and _refill(a, 0, batch=0) == -1 and _refill(a, 0, trials=-1) == -1
    for k in ("start_tick", "trial", "next", "state0", "q_end_tick", "q_slot", "q_ticks", "end_tick", "box_slack_min"):
        assert _refill(a, 0, without=(k,)) == -1, k
    rec, f = rf.structs(a, TT)
    assert lib.cmpc_rollout_refill(B, 0, None, C.byref(f), a["state"].ctypes.data) == -1 and lib.cmpc_rollout_refill(B, 0, C.byref(rec), None, None) == -1
    f.dWrenchTrials, f.wrench_ticks = a["state0"].ctypes.data, 0          # a schedule with no rows
    assert lib.cmpc_rollout_refill(B, 0, C.byref(rec), C.byref(f), a["state"].ctypes.data) == -1
    rec, f = rf.structs(a, TT)
    # the device forms refuse a NULL handle before anything touches a GPU
    assert lib.cmpc_rollout_refill_device(None, 0, C.byref(rec), C.byref(f), a["state"].ctypes.data, None) == -1
    assert lib.cmpc_rollout_refill_init_device(None, C.byref(f), None) == -1
    # the walk: what needs no handle is refused ahead of the handle check, so the message says which refusal it was
    lib.cmpc_last_error.restype = C.c_char_p
    io = cm._capi.CmpcWalkIO()
    out = C.c_int(0)
    walk_c = lambda m: lib.cmpc_rollout_walk_refill_device(None, m, 0, 1, C.byref(io), C.byref(rec), C.byref(f), 0, 0, C.byref(out), None)
    why = lambda: lib.cmpc_last_error(None).decode()
    assert walk_c(17) == -1 and "max_contacts must be 1 .. 16" in why()
    assert walk_c(0) == -1 and "max_contacts must be 1 .. 16" in why()
    assert walk_c(16) == -1 and "null handle" in why()
    io.dWrenchTicks, io.wrench_ticks = a["state0"].ctypes.data, 1
    assert walk_c(4) == -1 and "dWrenchTicks is not taken" in why()
    io = cm._capi.CmpcWalkIO()
    assert walk_c(4) == -1 and "null handle" in why()
    assert lib.cmpc_rollout_walk_refill_device(None, 4, 0, 1, None, C.byref(rec), C.byref(f), 0, 0, None, None) == -1 and "null argument" in why()
    # the Python surface: NotImplementedError for what is out of scope, before self is used for anything but its list length and flag
    ro = types.SimpleNamespace(M=5, force_sample_time=False)
    walk = cm.rollout.WalkingRollout.walk_device_refill
    z = np.zeros((3, 3))
    for kw in (dict(replan={2: None}), dict(mismatch=dict(force_gain=np.ones(3))), dict(taped=True), dict(every=4)):
        with pytest.raises(NotImplementedError):
            walk(ro, 4, 2, z, z, z, **kw)
    for fst in (False, True):          # lists longer than the front kernel's LDS stage, with force_sample_time or without
        with pytest.raises(NotImplementedError):
            walk(types.SimpleNamespace(M=17, force_sample_time=fst), 4, 2, z, z, z)
    with pytest.raises(TypeError):
        walk(ro, 4, 2, z, z, z, no_such_argument=1)
    with pytest.raises(ValueError):
        walk(ro, 4, 2, z, z, z, push=z, wrench_trials=np.zeros((1, 3, 10, 6)))


def test_host_form_under_sanitizers(tmp_path):
    """the host form's loops (csrc/cmpc_contacts.h, what cmpc_rollout_refill runs) from a stand-alone program with its own main, built with
    -fsanitize=address,undefined, over the B = 5 case: no report, and the assignment above"""
    import __graft_entry__ as ge
    # the clang++ beside the hipcc that built the library (its sanitizer runtimes are linked statically); no compiler is a failure, not a skip
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(ge.HIPCC) or ge.HIPCC)))
    cxx = next((p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(p)), None)
    assert cxx is not None, f"no clang++ under {rocm}"
    exe = str(tmp_path / "refill_host_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", ge.CSRC, os.path.join(ROOT, "tests", "refill_host_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[0] == "fill next 5 trial 0 1 2 3 4 start 0 0 0 0 0 end -1 -1 -1 -1 -1 slot 0 1 2 3 4 -1 -1 ticks 0 0 0 0 0 0 0"
    assert lines[1] == "refill next 7 trial 0 5 2 6 -1 start 1 3 1 3 0 end -1 -1 -1 -1 3 slot 0 1 2 3 4 1 3 ticks 2 2 2 2 3 0 0"
    assert lines[2] == lines[1].replace("refill", "nothing-free")
    assert lines[3] == "archive next 7 trial 0 5 2 6 -1 start 1 3 1 3 0 end -1 -1 -1 -1 3 slot 0 1 2 3 4 1 3 ticks 3 2 3 2 3 1 1"


# ---- the assignment rule: an independent model, held to the hand-made tables, and the host form held to the model ----
def test_assignment_model_reproduces_the_hand_made_tables():
    """tests/walk_refill_ref.py's model against the tables of tests/test_gpu_walk_refill.py that were written down by hand: the stormy queue (trials 1, 4, 2 and
    6 ending at local ticks 0, 0, 2 and 1), the calm one, test_queue_runs_dry's, and test_assignment_order_and_archive's B = 5 case"""
    end = [-1] * 10
    end[1], end[4], end[2], end[6] = 0, 0, 2, 1
    m = rf.assignment_model(4, 10, 4, 12, end)
    assert m["trial_of"].tolist() == rf.TRIAL_OF and m["slot"].tolist() == rf.SLOT and m["start"].tolist() == rf.START
    assert m["ticks"].tolist() == rf.TICKS and m["end_tick"].tolist() == rf.END
    assert rf.walk_length(4, 10, 4, end) == 9
    m = rf.assignment_model(4, 10, 4, 12, [-1] * 10)
    assert m["slot"].tolist() == rf.SLOT_CALM and m["start"].tolist() == rf.START_CALM and m["ticks"].tolist() == [4] * 10 and (m["end_tick"] == -1).all()
    # test_queue_runs_dry: Q = 5, B = 4, trial_ticks = 4, 10 ticks
    m = rf.assignment_model(4, 5, 4, 10, [-1] * 5)
    assert m["trial_of"].tolist() == [[0, 1, 2, 3]] * 4 + [[4, -1, -1, -1]] * 4 + [[-1] * 4] * 2
    assert m["slot"].tolist() == [0, 1, 2, 3, 0] and m["start"].tolist() == [0, 0, 0, 0, 4] and m["ticks"].tolist() == [4] * 5 and (m["end_tick"] == -1).all()
    # a walk cut short: trial 4 has walked 2 of its 4 ticks after 6, and an ending behind the cut is not seen
    m = rf.assignment_model(4, 5, 4, 6, [-1, -1, -1, -1, 3])
    assert m["ticks"].tolist() == [4, 4, 4, 4, 2] and m["end_tick"].tolist() == [-1] * 5
    # Q < B, Q = 0, and an ending at or past trial_ticks that never happens
    m = rf.assignment_model(5, 2, 3, 2, [-1, 7])
    assert m["trial_of"].tolist() == [[0, 1, -1, -1, -1]] * 2 and m["end_tick"].tolist() == [-1, -1]
    m = rf.assignment_model(3, 0, 3, 2, [])
    assert m["trial_of"].tolist() == [[-1] * 3] * 2 and m["slot"].shape == (0,)


def _random_cases():
    """(B, Q, trial_ticks, ticks, end_local, seed) of the property test: every B with every end probability and seven queue lengths 0 .. 4 B, seeds fixed"""
    cases, seed = [], 1000
    for B in (1, 2, 5, 63, 64, 65, 256, 257, 300):
        for p_end in (0.0, 0.25, 0.75):
            for Q in sorted({0, 1, max(B - 1, 0), B, B + 1, 2 * B + 3, 4 * B}) + [None]:
                seed += 1
                rng = np.random.default_rng(seed)
                if Q is None:
                    Q = int(rng.integers(0, 4 * B + 1))
                trial_ticks = int(rng.integers(1, 7))
                end = np.where(rng.random(Q) < p_end, rng.integers(0, trial_ticks, Q), -1)
                full = rf.walk_length(B, Q, trial_ticks, end)
                # mostly one tick past the end of the queue (the slots run dry); one walk in four is cut short
                ticks = full + 1 if seed % 4 else max(1, full // 2)
                cases.append((B, Q, trial_ticks, ticks, end, seed))
    return cases


def test_host_form_follows_the_assignment_model():
    """cmpc_rollout_refill tick by tick against the model, over random B, Q, trial_ticks and endings: the test writes a slot's end_tick / end_code at the tick
    the model ends its trial, as the record kernel would, and compares trial, start_tick, next and the trial_of row after every call, then q_slot,
    q_start, q_ticks and q_end_tick behind the archive-only call.  All exact."""
    cases = _random_cases()
    assert len(cases) >= 200 and {c[0] for c in cases} == {1, 2, 5, 63, 64, 65, 256, 257, 300}
    assert any(c[1] == 0 for c in cases) and any(c[1] == 4 * c[0] for c in cases) and {c[2] for c in cases} == {1, 2, 3, 4, 5, 6}
    ended = 0
    for B_, Q_, tt, ticks, end, seed in cases:
        why = f"B {B_} Q {Q_} trial_ticks {tt} ticks {ticks} seed {seed}"
        m = rf.assignment_model(B_, Q_, tt, ticks, end)
        a = rf.arrays(B_, Q_, rows=ticks, seed=seed)
        a["end_tick"][:] = -1        # (as cmpc_rollout_outcome_init_device leaves a record)
        without = tuple(k for _, k, _, _ in rf.TRIAL) + ("state0",) if Q_ == 0 else ()
        rec, f = rf.structs(a, tt, without=without)
        lib = cm._capi.lib()
        assert lib.cmpc_rollout_refill_init(B_, C.byref(f)) == 0, why
        for t in range(ticks):
            assert lib.cmpc_rollout_refill(B_, t, C.byref(rec), C.byref(f), a["state"].ctypes.data) == 0, why
            want = m["trial_of"][t]
            sits = want >= 0
            assert np.array_equal(a["trial"], want) and np.array_equal(a["trial_of"][t], want), (why, t)
            assert np.array_equal(a["start_tick"][sits], m["start"][want[sits]]), (why, t)
            assert a["next"][0] == np.count_nonzero((m["start"] >= 0) & (m["start"] <= t)), (why, t)
            assert (a["end_tick"][~sits] >= 0).all() and (a["end_tick"][sits] == -1).all(), (why, t)      # (an empty slot is out through the ended mask)
            fresh = np.flatnonzero(sits)[m["start"][want[sits]] == t]        # (a spawned slot's live state is its trial's)
            assert (rf.bits(a["state"][fresh]) == rf.bits(a["state0"][want[fresh]])).all(), (why, t)
            # the record behind tick t: the trials the model ends at this tick
            local = t - m["start"][want[sits]]
            ends = np.flatnonzero(sits)[(end[want[sits]] == local) & (local < tt)]
            a["end_tick"][ends] = end[want[ends]]
            a["end_code"][ends] = 3
            ended += len(ends)
        assert (a["trial_of"][ticks:].size == 0), why
        assert lib.cmpc_rollout_refill(B_, ticks, C.byref(rec), C.byref(f), None) == 0, why
        if Q_:
            for k, mk in (("q_slot", "slot"), ("q_start", "start"), ("q_ticks", "ticks"), ("q_end_tick", "end_tick")):
                assert np.array_equal(a[k], m[mk]), (why, k)
            assert np.array_equal(a["q_end_code"], np.where(m["end_tick"] >= 0, 3, 0)), why
    assert ended > 1000
