"""Helpers of the refill tests: the arrays of a cmpc_walk_record's outcome and of a cmpc_walk_refill as numpy arrays (or CUDA tensors), the two C structs
over them, and the crafted B = 5, Q = 7 case both test files use."""
import ctypes as C

import numpy as np

import cmpc_amd as cm

REC = (("dEndTick", "end_tick", np.int32, ()), ("dEndCode", "end_code", np.int32, ()), ("dIterationsSum", "iterations_sum", np.int32, ()),
       ("dIterationsMax", "iterations_max", np.int32, ()), ("dFinalState", "final_state", np.float32, (9,)), ("dBoxSlackMin", "box_slack_min", np.float32, ()))
SLOT = (("dStartTick", "start_tick"), ("dTrial", "trial"))
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
    for _, k in SLOT:
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
    for field, k in SLOT:
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
