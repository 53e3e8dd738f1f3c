"""Numpy restatement of the two steps a refill walk with plans per trial adds (include/cmpc.h, cmpc_walk_refill_plans), written from the header's contract
and not from the library's code: the plan select of one tick -- which slots are spawned, what each receives, what a bad index does -- and the fold of
per-trial gradients onto the pool's rows, in ascending trial order."""
import numpy as np

import cmpc_amd as cm

LISTS = ("T", "Pose", "N")
TRAJ = ("Com", "H")
POISON = 0xA5


def pool_arrays(Pn, M, knots, rng):
    """a pool of Pn plans in the layout of the planner's lists, random bits (NaN payloads included), and its trajectories"""
    p = dict(T=rng.normal(size=(Pn, 2, M, 2)), Pose=rng.normal(size=(Pn, 2, M, 7)).astype(np.float32), N=rng.integers(0, M + 1, (Pn, 2)).astype(np.int32),
             Com=rng.normal(size=(Pn, knots, 3)).astype(np.float32), H=rng.normal(size=(Pn, knots, 3)).astype(np.float32))
    p["T"].view(np.uint64)[0, 0, 0, 0] = 0x7FF8000000000123
    p["Pose"].view(np.uint32)[-1, 1, M - 1, 6] = 0x7FC00456
    return p


def live_arrays(B, M, knots, fill=POISON):
    """the slots' rows (and one slot more in front and behind, so that a write outside the batch shows), every byte `fill`"""
    shapes = dict(T=((B + 2, 2, M, 2), np.float64), Pose=((B + 2, 2, M, 7), np.float32), N=((B + 2, 2), np.int32), Com=((B + 2, knots, 3), np.float32),
                  H=((B + 2, knots, 3), np.float32))
    return {k: np.frombuffer(bytes([fill]) * (int(np.prod(s)) * np.dtype(dt).itemsize), dt).copy().reshape(s) for k, (s, dt) in shapes.items()}


def plans_struct(pool, live, plan_of, ok, pool_plans=None, traj=True, without=()):
    """the cmpc_walk_refill_plans over a pool and the slots' rows (live[k][1:-1] is the batch); without: fields left NULL"""
    c = cm._capi.CmpcWalkRefillPlans()
    c.pool_plans = int(pool["T"].shape[0]) if pool_plans is None else pool_plans
    for k in LISTS + (TRAJ if traj else ()):
        if "dPool" + k not in without:
            setattr(c, "dPool" + k, pool[k].ctypes.data)
        if "dPlan" + k not in without:
            setattr(c, "dPlan" + k, live[k][1:].ctypes.data)
    c.dTrialPlan = None if plan_of is None else plan_of.ctypes.data
    c.dTrialPlanOk = None if ok is None else ok.ctypes.data
    return c


def select(pool, live, tick, start_tick, trial, plan_of, ok, end_tick, end_code, traj=True):
    """(the slots' rows, dTrialPlanOk, dEndTick, dEndCode) after the select launch of `tick`.  A slot is spawned when start_tick[b] == tick and it holds a
    trial of the queue; a spawned slot whose trial's index lies in the pool receives the row (ok 1); one whose index lies outside receives nothing and is
    ended at spawn, local tick 0 with code 0 (ok 0); every other slot, and ok of every other trial, is left as it was."""
    B, Q, Pn = len(start_tick), len(plan_of), pool["T"].shape[0]
    out = {k: v.copy() for k, v in live.items()}
    ok, end_tick, end_code = ok.copy(), end_tick.copy(), end_code.copy()
    for b in range(B):
        q = int(trial[b])
        if int(start_tick[b]) != tick or q < 0 or q >= Q:
            continue
        p = int(plan_of[q])
        if p < 0 or p >= Pn:
            ok[q], end_tick[b], end_code[b] = 0, 0, 0
            continue
        ok[q] = 1
        for k in LISTS + (TRAJ if traj else ()):
            out[k][1 + b] = pool[k][p]
    return out, ok, end_tick, end_code


def fold(index, per_trial, pool_rows):
    """out[p] = the float64 sum of per_trial[q] over the trials with index[q] == p, from +0.0 and in ascending q: a member is added, a non-member is not
    touched (so its NaN stays where it is), an index outside the pool belongs to no row"""
    per_trial = np.asarray(per_trial, np.float64)
    out = np.zeros((pool_rows,) + per_trial.shape[1:], np.float64)
    for q in range(len(index)):
        p = int(index[q])
        if 0 <= p < pool_rows:
            out[p] = out[p] + per_trial[q]
    return out
