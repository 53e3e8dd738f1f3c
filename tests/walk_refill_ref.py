"""Helpers of the refill tests: the arrays of a cmpc_walk_record's outcome and of a cmpc_walk_refill as numpy arrays (or CUDA tensors), the two C structs
over them, the crafted B = 5, Q = 7 case both test files use, an independent model of the assignment rule (assignment_model: plain Python, nothing of the
library) and the hand-made tables of tests/test_gpu_walk_refill.py that the model is held to."""
import ctypes as C

import numpy as np

import cmpc_amd as cm

REC = (("dEndTick", "end_tick", np.int32, ()), ("dEndCode", "end_code", np.int32, ()), ("dIterationsSum", "iterations_sum", np.int32, ()),
       ("dIterationsMax", "iterations_max", np.int32, ()), ("dFinalState", "final_state", np.float32, (9,)), ("dBoxSlackMin", "box_slack_min", np.float32, ()))
PER_SLOT = (("dStartTick", "start_tick"), ("dTrial", "trial"))
TRIAL = (("dTrialEndTick", "q_end_tick", np.int32, ()), ("dTrialEndCode", "q_end_code", np.int32, ()), ("dTrialIterationsSum", "q_iterations_sum", np.int32, ()),
         ("dTrialIterationsMax", "q_iterations_max", np.int32, ()), ("dTrialFinalState", "q_final_state", np.float32, (9,)),
         ("dTrialBoxSlackMin", "q_box_slack_min", np.float32, ()), ("dTrialTicks", "q_ticks", np.int32, ()), ("dTrialSlot", "q_slot", np.int32, ()),
         ("dTrialStart", "q_start", np.int32, ()))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def arrays(B, Q, rows=0, seed=0, fill=0x5A):
    """every array the refill reads or writes: the slots' outcome and state (random, NaN payloads included), the queue's initial states (random), everything
    else filled with the byte `fill` so that a word left unwritten shows"""
    rng = np.random.default_rng(seed)
    a = {}
    for _, k, dt, tail in REC:
        a[k] = rng.integers(0, 50, (B,) + tail).astype(dt) if dt == np.int32 else rng.normal(size=(B,) + tail).astype(dt)
    a["state"] = rng.normal(size=(B, 9)).astype(np.float32)
    a["state0"] = rng.normal(size=(max(Q, 1), 9)).astype(np.float32)[:Q]
    if Q > 0:
        a["state0"].view(np.uint32)[0, 0] = 0x7FC00123      # (a NaN payload is copied as bits)
    for _, k in PER_SLOT:
        a[k] = np.frombuffer(bytes([fill]) * 4 * B, np.int32).copy()
    a["next"] = np.frombuffer(bytes([fill]) * 4, np.int32).copy()
    for _, k, dt, tail in TRIAL:
        a[k] = np.frombuffer(bytes([fill]) * 4 * Q * int(np.prod(tail + (1,))), dt).copy().reshape((Q,) + tail)
    if rows:
        a["trial_of"] = np.frombuffer(bytes([fill]) * 4 * rows * B, np.int32).copy().reshape(rows, B)
    return a


def _ptr(x):
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def structs(a, trial_ticks, tick_first=0, trials=None, without=()):
    """(cmpc_walk_record, cmpc_walk_refill) over the arrays of `a` (numpy: the host form; CUDA tensors: the device form); without: names left NULL"""
    get = lambda k: None if k in without else _ptr(a.get(k))
    rec = cm._capi.CmpcWalkRecord()
    rec.rows = 1
    for field, k, _, _ in REC:
        setattr(rec, field, get(k))
    f = cm._capi.CmpcWalkRefill()
    f.trials = int(a["state0"].shape[0]) if trials is None else trials
    f.trial_ticks = trial_ticks
    f.dNext, f.dState0 = get("next"), get("state0")
    for field, k in PER_SLOT:
        setattr(f, field, get(k))
    for field, k, _, _ in TRIAL:
        setattr(f, field, get(k))
    if a.get("trial_of") is not None and "trial_of" not in without:
        f.trace = cm._capi.CmpcWalkRefillTrace(int(a["trial_of"].shape[0]), tick_first, _ptr(a["trial_of"]))
    return rec, f


def outcome_init_rule(state0_row):
    """what cmpc_rollout_outcome_init_device gives a problem that starts from state0_row"""
    return dict(end_tick=np.int32(-1), end_code=np.int32(0), iterations_sum=np.int32(0), iterations_max=np.int32(0),
                final_state=np.asarray(state0_row, np.float32), box_slack_min=np.float32(np.inf))


def to_cuda(a):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in a.items()}


def to_host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---- the assignment rule (DESIGN.md 7f "The assignment rule"), written from the rule and not from the library's code: a slot is a time from which it is free
def assignment_model(B, Q, trial_ticks, ticks, end_local):
    """Who sits where in a refill walk of `ticks` ticks: B slots, Q trials of trial_ticks ticks each, trial q ending at its local tick end_local[q] (-1, or
    at or past trial_ticks: it never ends).  A slot is free at a tick if it is empty, if its trial ended at an earlier tick, or if its trial has walked
    trial_ticks ticks; the free slots, in ascending order, take the next trials; once the queue is empty a free slot is left empty.
    -> dict(trial_of[ticks, B], slot[Q], start[Q], ticks[Q], end_tick[Q]) int32: -1 in trial_of an empty slot, -1 in slot / start a trial never started,
    ticks the local ticks a trial has walked inside the walk, end_tick its ending local tick if that tick lies inside the walk, else -1."""
    end_local = [int(e) for e in end_local]
    assert len(end_local) == Q and B >= 1 and trial_ticks >= 1 and ticks >= 0
    length = [e + 1 if 0 <= e < trial_ticks else trial_ticks for e in end_local]      # (the ticks a trial holds its slot)
    trial_of = np.full((ticks, B), -1, np.int32)
    slot, start = np.full(Q, -1, np.int32), np.full(Q, -1, np.int32)
    free_from, sits = [0] * B, [-1] * B
    queue = iter(range(Q))
    for t in range(ticks):
        for b in range(B):
            if free_from[b] <= t:
                q = next(queue, None)
                sits[b] = -1 if q is None else q
                if q is not None:
                    slot[q], start[q], free_from[b] = b, t, t + length[q]
        trial_of[t] = sits
    walked = np.array([0 if start[q] < 0 else min(length[q], ticks - start[q]) for q in range(Q)], np.int32).reshape(Q)
    end_tick = np.array([end_local[q] if start[q] >= 0 and 0 <= end_local[q] < trial_ticks and start[q] + end_local[q] < ticks else -1 for q in range(Q)],
                        np.int32).reshape(Q)
    return dict(trial_of=trial_of, slot=slot, start=start, ticks=walked, end_tick=end_tick)


def walk_length(B, Q, trial_ticks, end_local):
    """the fewest ticks of a refill walk that records every trial to its end"""
    m = assignment_model(B, Q, trial_ticks, Q * trial_ticks + 1, end_local)
    return int((m["start"] + m["ticks"]).max()) if Q else 1


# ---- the hand-made tables of tests/test_gpu_walk_refill.py (B = 4, Q = 10, trial_ticks = 4, 12 ticks), worked out by hand from the assignment rule.  Trial 1
# ends at its local tick 0 (global 0), trial 4 (NaN state) at local 0 (global 1), trial 2 at local 2 (global 2), trial 6 at local 1 (global 4); a slot is free
# the tick after its trial ended, or once it has walked 4 ticks:
#   tick 0: slots 0..3 <- 0..3 | tick 1: slot 1 <- 4 | tick 2: slot 1 <- 5 | tick 3: slot 2 <- 6 | tick 4: slots 0, 3 (walked through) <- 7, 8 |
#   tick 5: slot 2 <- 9 | tick 6: slot 1 (trial 5 walked through) empty | tick 8: slots 0, 3 empty | tick 9: slot 2 empty
TRIAL_OF = [[0, 1, 2, 3], [0, 4, 2, 3], [0, 5, 2, 3], [0, 5, 6, 3], [7, 5, 6, 8], [7, 5, 9, 8], [7, -1, 9, 8], [7, -1, 9, 8], [-1, -1, 9, -1],
            [-1, -1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]]
SLOT = [0, 1, 2, 3, 1, 1, 2, 0, 3, 2]
START = [0, 0, 0, 0, 1, 2, 3, 4, 4, 5]
TICKS = [4, 1, 3, 4, 1, 4, 2, 4, 4, 4]
END = [-1, 0, 2, -1, 0, -1, 1, -1, -1, -1]
# the same queue with trials 1, 2, 4 and 6 harmless: nothing ends, the slots turn over every 4 ticks
SLOT_CALM = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
START_CALM = [0, 0, 0, 0, 4, 4, 4, 4, 8, 8]
