"""Numpy restatement of the regroup of a refill walk's tape by trial (include/cmpc.h, cmpc_walk_tape_regroup) for the tests: the arrays of a tape as host
buffers, the C structs over them, and the rule written from the header with plain indexing -- nothing of the library."""
import ctypes as C

import numpy as np

import cmpc_amd as cm

# (struct field, per-problem shape as a function of (nx, np, ng, M), dtype) in the order of cmpc_walk_tape's pointer fields
FIELDS = (
    ("dX", lambda nx, n_p, ng, M: (nx,), np.float32), ("dP", lambda nx, n_p, ng, M: (n_p,), np.float32), ("dLamG", lambda nx, n_p, ng, M: (ng,), np.float32),
    ("dInfo", lambda nx, n_p, ng, M: (8,), np.float32), ("dStates", lambda nx, n_p, ng, M: (9,), np.float32), ("dOk", lambda nx, n_p, ng, M: (), np.int32),
    ("dLand", lambda nx, n_p, ng, M: (2,), np.int32), ("dPlanT", lambda nx, n_p, ng, M: (2, M, 2), np.float64),
    ("dListT", lambda nx, n_p, ng, M: (2, M, 2), np.float64), ("dPlanN", lambda nx, n_p, ng, M: (2,), np.int32), ("dListN", lambda nx, n_p, ng, M: (2,), np.int32),
)
PLAN = ("dPlanT", "dPlanN")
SENTINEL = 0xC3


def bits(a):
    """the array as unsigned words, so that NaN payloads and the sign of zero take part in a comparison"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def arrays(N, M, rows, batch, rng=None, fill=SENTINEL):
    """{field: array[rows (+ 1 for dStates), batch, ...]}: random BITS (so NaN patterns of every payload, infinities and -0.0 occur) with rng, or every
    byte `fill`"""
    L = cm.Layout(N)
    out = {}
    for k, shape, dt in FIELDS:
        shp = (rows + (1 if k == "dStates" else 0), batch) + shape(L.nx, L.np, L.ng, M)
        a = np.empty(shp, dt)
        flat = a.view(np.uint8).reshape(-1)
        if rng is None:
            flat[:] = fill
        else:
            flat[:] = rng.integers(0, 256, flat.size, dtype=np.uint8)
            if dt != np.int32:      # (a few quiet and signalling NaNs planted as well: random bits give one in 256 floats, fewer doubles)
                w = bits(a).reshape(-1)
                pick = rng.integers(0, w.size, max(4, w.size // 13))
                w[pick[0::2]] = 0x7FC00123 if a.itemsize == 4 else 0x7FF8000000000123
                w[pick[1::2]] = 0xFFA00001 if a.itemsize == 4 else 0xFFF4000000000001
        out[k] = a
    return out


def struct(arr, rows, step=0.01, substeps=6, force_sample_time=0, first=1, without=()):
    """the cmpc_walk_tape over the arrays; the fields named in `without` are NULL"""
    t = cm._capi.CmpcWalkTape()
    t.rows = rows
    for k, _, _ in FIELDS:
        setattr(t, k, None if k in without else arr[k].ctypes.data_as(C.c_void_p))
    t.plant_step, t.plant_substeps, t.force_sample_time, t.first_row_is_first_tick = step, substeps, force_sample_time, first
    return t


def regroup_struct(tick_first, index, end_out, ok_out):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return cm._capi.CmpcWalkTapeRegroup(tick_first, p(index), p(end_out), p(ok_out))


def refill_struct(trial_ticks, state0, slot, start, ticks, end_tick, trials=None, without=()):
    """a cmpc_walk_refill with what the regroup reads: the counts, dState0 and the four per-trial words"""
    f = cm._capi.CmpcWalkRefill()
    f.trials = int(state0.shape[0]) if trials is None else trials
    f.trial_ticks = trial_ticks
    for field, a in (("dState0", state0), ("dTrialSlot", slot), ("dTrialStart", start), ("dTrialTicks", ticks), ("dTrialEndTick", end_tick)):
        setattr(f, field, None if field in without else a.ctypes.data_as(C.c_void_p))
    return f


def kind(q, Q, B, src_rows, trial_ticks, tick_first, slot, start, ticks):
    """'none', 'never' or 'started' for the column whose index is q"""
    if not 0 <= q < Q:
        return "none"
    n = int(ticks[q])
    if n < 1:
        return "never"
    t0 = int(start[q]) - tick_first
    if not 0 <= slot[q] < B or t0 < 0 or t0 + min(n, trial_ticks) - 1 >= src_rows:
        return "none"
    return "started"


def expected(src, dst, src_rows, trial_ticks, tick_first, index, state0, slot, start, ticks, end_tick):
    """(arrays of dst after the regroup, end_out, ok_out): the rule of include/cmpc.h column by column"""
    B, Q = dst["dX"].shape[1], state0.shape[0]
    out = {k: v.copy() for k, v in dst.items()}
    end_out, ok_out = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for j, q in enumerate(index):
        what = kind(q, Q, B, src_rows, trial_ticks, tick_first, slot, start, ticks)
        if what == "none":
            continue
        ok_out[j] = 1
        out["dStates"][0, j] = state0[q]
        if what == "never":
            continue
        s, t0, n, e = int(slot[q]), int(start[q]) - tick_first, int(ticks[q]), int(end_tick[q])
        for r in range(trial_ticks):
            sr = t0 + min(r, n - 1)
            for k in out:
                if k == "dStates":
                    out[k][r + 1, j] = src[k][sr + 1, s]
                elif r == 0 and k in PLAN:
                    out[k][0, j] = 0
                else:
                    out[k][r, j] = src[k][sr, s]
        end_out[j] = e if e >= 0 else n if n < trial_ticks else -1
    return out, end_out, ok_out
