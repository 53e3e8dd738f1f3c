"""The record rule of a device walk (include/cmpc.h, "a walk of the whole batch on the device") restated in numpy, problem by problem, in float64:
what cmpc_rollout_record / cmpc_rollout_record_device must write for one tick.  Not product code: the tests hold the library to it."""
import numpy as np

import cmpc_amd as cm

STOP_MERGE, STOP_SOLVER, STOP_NONFINITE = 1, 2, 4


def new_outcome(state0):
    B = state0.shape[0]
    return dict(end_tick=np.full(B, -1, np.int32), end_code=np.zeros(B, np.int32), iterations_sum=np.zeros(B, np.int32),
                iterations_max=np.zeros(B, np.int32), final_state=state0.astype(np.float32).copy(), box_slack_min=np.full(B, np.inf, np.float32))


def tick_code(ended_before, ok, status, state_out):
    if ended_before:
        return -1
    if not ok:
        return 1
    if status != 0:
        return 1 + int(status)
    if not np.isfinite(state_out).all():
        return 5
    return 0


def record_tick(N, tick, stop_mask, X, P, info, ok, land, state_out, zmp, box_upper, box_lower, outcome):
    """-> (row, stats): row = dict(com[B,3], zmp[B,2], land[B,2], landing_offset[B,2,3], iterations[B], code[B]), stats[6]; `outcome` (new_outcome) is
    updated in place.  ok may be None (every merge good)."""
    L = cm.Layout(N)
    B = X.shape[0]
    row = dict(com=np.full((B, 3), np.nan, np.float32), zmp=np.full((B, 2), np.nan, np.float32), land=np.full((B, 2), -2, np.int32),
               landing_offset=np.full((B, 2, 3), np.nan), iterations=np.zeros(B, np.int32), code=np.zeros(B, np.int32))
    stats = np.zeros(6, np.int32)
    up, lo = np.asarray(box_upper, np.float32).astype(np.float64), np.asarray(box_lower, np.float32).astype(np.float64)
    for b in range(B):
        before = outcome["end_tick"][b] >= 0
        code = tick_code(before, True if ok is None else bool(ok[b]), info[b, 5], state_out[b])
        row["code"][b] = code
        ends = code == 1 or (2 <= code <= 4 and stop_mask & STOP_SOLVER) or (code == 5 and stop_mask & STOP_NONFINITE)
        if not before:
            stats[0] += 1
            stats[4] += 2 <= code <= 4
        if ends:
            stats[1] += 1
            outcome["end_tick"][b], outcome["end_code"][b] = tick, code
        if before or ends:
            continue
        it = int(info[b, 0])
        row["iterations"][b] = it
        row["com"][b], row["zmp"][b], row["land"][b] = state_out[b, :3], zmp[b], land[b]
        stats[2] += it
        stats[3] = max(stats[3], it)
        outcome["iterations_sum"][b] += it
        outcome["iterations_max"][b] = max(outcome["iterations_max"][b], it)
        outcome["final_state"][b] = state_out[b]
        row["landing_offset"][b] = 0.0
        for c in range(2):
            k = int(land[b, c])
            if 0 < k <= N:
                Rt = P[b, L.p_R[c] + 9 * (k - 1):L.p_R[c] + 9 * k].astype(np.float64).reshape(3, 3)     # vec(R) column-major: the rows of this are R^T's
                d = X[b, L.pos[c] + 3 * k:L.pos[c] + 3 * k + 3].astype(np.float64) - P[b, L.p_nom[c] + 3 * k:L.p_nom[c] + 3 * k + 3].astype(np.float64)
                off = np.array([(Rt[i, 0] * d[0] + Rt[i, 1] * d[1]) + Rt[i, 2] * d[2] for i in range(3)])
                row["landing_offset"][b, c] = off
                slack = np.float32(min((up[c] - off).min(), (off - lo[c]).min()))
                outcome["box_slack_min"][b] = min(outcome["box_slack_min"][b], slack)
    return row, stats


def stats_of_trace(code, iterations, ended_by):
    """the statistics rows [T, 6] from a trace: code[T, B], iterations[T, B], ended_by[T, B] bool (the problem ended at that tick)"""
    T = code.shape[0]
    st = np.zeros((T, 6), np.int32)
    st[:, 0] = (code != -1).sum(1)
    st[:, 1] = ended_by.sum(1)
    st[:, 2] = iterations.sum(1)
    st[:, 3] = iterations.max(1)
    st[:, 4] = ((code >= 2) & (code <= 4)).sum(1)
    return st


# ---- crafted ticks: what a tick could have left, made by hand (no solve) ----
LAND_VALUES = lambda N: [3, N, -2, -1, 0]     # a landing inside the horizon, at its end, an unsampled foot, a foot that never lifts, knot 0


def _tick(rng, N, B, cond, land):
    """one tick's leftovers for B problems; cond[b]: 0 clean, 1 merge failed, 2..4 solver status 1..3, 5 non-finite state.  Conditions overlap on purpose
    (a failed merge also carries a solver status and a non-finite state, a solver status also a non-finite state): the first match must win."""
    L = cm.Layout(N)
    X = rng.uniform(-0.1, 0.1, (B, L.nx)).astype(np.float32)
    P = rng.uniform(-1.0, 1.0, (B, L.np)).astype(np.float32)
    for c in range(2):      # nominal positions near the solution's, so that the offsets sit around the box
        P[:, L.p_nom[c]:L.p_nom[c] + 3 * (N + 1)] = X[:, L.pos[c]:L.pos[c] + 3 * (N + 1)] + rng.uniform(-0.03, 0.03, (B, 3 * (N + 1))).astype(np.float32)
    info = np.zeros((B, 8), np.float32)
    info[:, 0] = rng.integers(3, 30, B)
    state_out = rng.uniform(-1, 1, (B, 9)).astype(np.float32)
    zmp = rng.uniform(-0.05, 0.05, (B, 2)).astype(np.float32)
    ok = np.ones(B, np.int32)
    cond = np.asarray(cond)
    ok[cond == 1] = 0
    info[cond == 1, 5] = 2
    for s in (1, 2, 3):
        info[cond == 1 + s, 5] = s
    state_out[(cond >= 1) & (cond <= 2), 4] = np.nan
    state_out[cond == 5, 7] = np.inf
    return dict(X=X, P=P, info=info, ok=ok, land=np.ascontiguousarray(land, np.int32), state_out=state_out, zmp=zmp)


def crafted_ticks(N, variant):
    """two consecutive ticks of B = 5 problems and the outcome they start from.  variant "feet": every tick clean, the feet's landing knots run through
    LAND_VALUES; "codes": tick 0 has one problem per code 0..4, tick 1 brings code 5 on the problem that was clean; "ended": the same with problem 4
    ended earlier (tick 7 of some earlier call, code 3)."""
    rng = np.random.default_rng(3)
    v = LAND_VALUES(N)
    lands = [[(v[b], v[(b + 1) % 5]) for b in range(5)], [(v[(b + 2) % 5], v[(b + 3) % 5]) for b in range(5)]]
    conds = [[0] * 5, [0] * 5] if variant == "feet" else [[0, 1, 2, 3, 4], [5, 0, 1, 2, 0]]
    ticks = [_tick(rng, N, 5, conds[i], lands[i]) for i in range(2)]
    state0 = rng.uniform(-1, 1, (5, 9)).astype(np.float32)
    out = new_outcome(state0)
    if variant == "ended":
        out["end_tick"][4], out["end_code"][4], out["iterations_sum"][4], out["iterations_max"][4] = 7, 3, 40, 9
    return ticks, out


def random_ticks(N, B, seed, n=2):
    """n consecutive ticks of B problems with random conditions, landing knots in -2..N, and one problem in eight ended earlier"""
    rng = np.random.default_rng(seed)
    ticks = [_tick(rng, N, B, rng.choice(6, B, p=[0.7, 0.06, 0.06, 0.06, 0.06, 0.06]), rng.integers(-2, N + 1, (B, 2))) for _ in range(n)]
    out = new_outcome(rng.uniform(-1, 1, (B, 9)).astype(np.float32))
    early = rng.random(B) < 0.125
    out["end_tick"][early], out["end_code"][early] = 2, 1
    return ticks, out


def reference(N, ticks, outcome, stop_mask, box_upper, box_lower, tick0=11):
    """the restatement over consecutive ticks (numbers tick0, tick0 + 1, ..): (rows, stats[T, 6], final outcome); `outcome` is not modified"""
    out = {k: a.copy() for k, a in outcome.items()}
    rows, stats = [], []
    for i, t in enumerate(ticks):
        r, st = record_tick(N, tick0 + i, stop_mask, t["X"], t["P"], t["info"], t["ok"], t["land"], t["state_out"], t["zmp"], box_upper, box_lower, out)
        rows.append(r); stats.append(st)
    return rows, np.stack(stats), out


TRACE = dict(com=(3,), zmp=(2,), land=(2,), landing_offset=(2, 3), iterations=(), code=())
TRACE_DTYPE = dict(com=np.float32, zmp=np.float32, land=np.int32, landing_offset=np.float64, iterations=np.int32, code=np.int32)


def assert_matches(got, rows, stats, outcome):
    """got: dict of numpy arrays named like walk_record's (trace [T, B, ..], outcome, stats) against the restatement.  Ints and float copies bit-equal
    (NaN rows as NaN), landing_offset to 1e-12 absolute, box_slack_min to 1e-7."""
    for i, r in enumerate(rows):
        for k in ("land", "iterations", "code"):
            np.testing.assert_array_equal(got[k][i], r[k], err_msg=f"{k}, row {i}")
        for k in ("com", "zmp"):
            assert got[k][i].dtype == np.float32
            nan = np.isnan(r[k])
            np.testing.assert_array_equal(np.isnan(got[k][i]), nan, err_msg=f"{k}, row {i}")
            np.testing.assert_array_equal(got[k][i][~nan].view(np.uint32), r[k][~nan].view(np.uint32), err_msg=f"{k}, row {i}")
        nan = np.isnan(r["landing_offset"])
        np.testing.assert_array_equal(np.isnan(got["landing_offset"][i]), nan)
        np.testing.assert_allclose(got["landing_offset"][i][~nan], r["landing_offset"][~nan], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got["stats"][:len(rows)], stats)
    for k in ("end_tick", "end_code", "iterations_sum", "iterations_max"):
        np.testing.assert_array_equal(got[k], outcome[k], err_msg=k)
    np.testing.assert_array_equal(got["final_state"].view(np.uint32), outcome["final_state"].view(np.uint32))
    inf = np.isinf(outcome["box_slack_min"])
    np.testing.assert_array_equal(got["box_slack_min"][inf], outcome["box_slack_min"][inf])
    np.testing.assert_allclose(got["box_slack_min"][~inf], outcome["box_slack_min"][~inf], rtol=0, atol=1e-7)
