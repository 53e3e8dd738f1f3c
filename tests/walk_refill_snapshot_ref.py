"""Numpy restatement of the restore step of a refill walk whose trials start from a snapshot (include/cmpc.h, cmpc_walk_refill_snapshot), written from
the header's contract and not from the library's code: which slots are spawned at a tick, what each receives, and -- the part that is easy to get wrong --
which pool list set lands in which live set.  The arrays and the snapshot struct are tests/walk_snapshot_ref.py's."""
import ctypes as C

import numpy as np

import cmpc_amd as cm
from tests import walk_snapshot_ref as ws

SET_A = ("dListT", "dListPose", "dListN")
SET_B = ("dListTB", "dListPoseB", "dListNB")
POISON = 0xA5


def paired(pool_lists_in, live_prev):
    """{live field: pool field}: the pool's set pool_lists_in goes to the live set this tick reads as "previous" (live_prev), the pool's other set to the
    other live set; every other array goes to the array of its name"""
    m = {k: k for k, _, _ in ws.FIELDS}
    if pool_lists_in != live_prev:
        m.update(dict(zip(SET_A, SET_B)))
        m.update(dict(zip(SET_B, SET_A)))
    return m


def expected(pool, pool_lists_in, pool_tick, live, live_prev, tick, start_tick, trial, snapshot_of, ok, without=()):
    """(live arrays after the restore launch of `tick`, dTrialSnapshotOk after it).  A slot is spawned when start_tick[b] == tick and it holds a trial;
    a spawned slot whose trial's index lies in the pool receives the row (ok 1); one whose index lies outside receives nothing but dEndTick = pool_tick,
    dEndCode = 0 (ok 0); every other slot, and ok of every other trial, is left as it was.  without: fields NULL on either side (skipped)."""
    B, Q, pool_batch = len(start_tick), len(snapshot_of), pool["dState"].shape[0]
    out = {k: v.copy() for k, v in live.items()}
    ok = ok.copy()
    names = paired(pool_lists_in, live_prev)
    for b in range(B):
        q = int(trial[b])
        if int(start_tick[b]) != tick or q < 0 or q >= Q:
            continue
        s = int(snapshot_of[q])
        if s < 0 or s >= pool_batch:
            ok[q] = 0
            out["dEndTick"][b], out["dEndCode"][b] = pool_tick, 0
            continue
        ok[q] = 1
        for k in out:
            if k not in without and names[k] not in without:
                out[k][b] = pool[names[k]][s]
    return out, ok


def refill_struct(start_tick, trial, trials):
    """a cmpc_walk_refill with what the restore reads: trials, dStartTick, dTrial (trial_ticks 1; everything else NULL)"""
    f = cm._capi.CmpcWalkRefill()
    f.trials, f.trial_ticks = trials, 1
    f.dStartTick, f.dTrial = start_tick.ctypes.data, trial.ctypes.data
    return f


def from_struct(pool_struct, pool_batch, snapshot_of, ok):
    """the cmpc_walk_refill_snapshot over a pool struct (kept alive by the caller) and the two per-trial arrays (None: NULL)"""
    return cm._capi.CmpcWalkRefillSnapshot(C.addressof(pool_struct) if pool_struct is not None else None, pool_batch,
                                           None if snapshot_of is None else snapshot_of.ctypes.data, None if ok is None else ok.ctypes.data)
