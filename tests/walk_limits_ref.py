"""The physical limits of a device walk (include/cmpc.h, "physical limits") restated in numpy float64: the four measures of a tick with the support
region as a HULL -- a monotone chain and point-to-segment distances, not the product's minimum over candidate directions -- the codes 6..9 behind
tests/walk_record_ref.py's chain, the measures row and the extremes.  Not product code: the tests hold the library to it."""
import numpy as np

import cmpc_amd as cm
from tests import walk_record_ref as wr

STOP_LIMITS = 8
OFF = dict(height_min=np.nan, height_max=np.nan, reach_max=np.nan, margin_min=np.nan, track_max=np.nan)


def hull(points):
    """the convex hull of points [n, 2], counter-clockwise, collinear points dropped (Andrew's monotone chain); 1 or 2 points for a point or a segment"""
    pts = sorted(set(map(tuple, np.asarray(points, np.float64).tolist())))
    if len(pts) <= 2:
        return np.array(pts)
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.array(lower[:-1] + upper[:-1])


def _to_segment(p, a, b):
    ab = b - a
    t = np.clip(np.dot(p - a, ab) / np.dot(ab, ab), 0.0, 1.0)
    return float(np.linalg.norm(p - (a + t * ab)))


def signed_distance(points, xi):
    """signed Euclidean distance of xi to the convex hull of points, positive inside"""
    h, xi = hull(points), np.asarray(xi, np.float64)
    if len(h) == 1:
        return -float(np.linalg.norm(xi - h[0]))
    if len(h) == 2:
        return -_to_segment(xi, h[0], h[1])
    edges = [(h[i], h[(i + 1) % len(h)]) for i in range(len(h))]
    d = min(_to_segment(xi, a, b) for a, b in edges)
    inside = all((b[0] - a[0]) * (xi[1] - a[1]) - (b[1] - a[1]) * (xi[0] - a[0]) >= 0 for a, b in edges)
    return d if inside else -d


def measures(N, X, P, state_out, corners, gravity):
    """-> [B, 4] float64: height, reach, margin, track at the time of state_out (stage 1 of the tick's problem).  corners [2, 4, 3] or [B, 2, 4, 3]."""
    L = cm.Layout(N)
    B = X.shape[0]
    X, P, S = X.astype(np.float64), P.astype(np.float64), state_out.astype(np.float64)
    corners = np.broadcast_to(np.asarray(corners, np.float32).astype(np.float64), (B, 2, 4, 3))
    out = np.full((B, 4), np.nan)
    for b in range(B):
        if not np.isfinite(state_out[b]).all():
            continue
        com, dcom = S[b, :3], S[b, 3:6]
        ref = P[b, L.p_comref + 3:L.p_comref + 6]
        out[b, 3] = np.hypot(com[0] - ref[0], com[1] - ref[1])
        feet = [c for c in range(2) if P[b, L.p_gam[c] + 1] > 0.5]
        if not feet:
            continue
        q = {c: X[b, L.pos[c] + 3:L.pos[c] + 6] for c in feet}
        R = {c: P[b, L.p_R[c] + 9:L.p_R[c] + 18].reshape(3, 3, order="F") for c in feet}
        height = com[2] - np.mean([q[c][2] for c in feet])
        out[b, 0] = height
        out[b, 1] = max(np.linalg.norm(com - q[c]) for c in feet)
        xi = com[:2] + dcom[:2] * np.sqrt(max(height, 0.0) / gravity)
        pts = [(q[c] + R[c] @ corners[b, c, j])[:2] for c in feet for j in range(4)]
        out[b, 2] = signed_distance(pts, xi)
    return out


def limit_code(m, lim):
    """the code 6..9 of float32 measures m[4] under lim (a dict like OFF), or 0; a NaN on either side never fires"""
    m = np.asarray(m, np.float32).astype(np.float64)
    if m[0] < lim["height_min"] or m[0] > lim["height_max"]:
        return 6
    if m[1] > lim["reach_max"]:
        return 7
    if m[2] < lim["margin_min"]:
        return 8
    if m[3] > lim["track_max"]:
        return 9
    return 0


def new_extremes(B):
    e = np.empty((B, 5), np.float32)
    e[:] = [np.inf, -np.inf, -np.inf, np.inf, -np.inf]
    return e


def record_tick(N, tick, stop_mask, t, box_upper, box_lower, outcome, lim, corners, gravity, extremes=None):
    """tests/walk_record_ref.record_tick with the limits behind it -> (row, stats): row gains measures[B, 4] float32; outcome and extremes are updated
    in place.  A problem that a limit ends is shown to the old restatement as ended before the tick (its row is the NaN row either way) and its code,
    its ending and the two counts are put right afterwards."""
    B = t["X"].shape[0]
    m32 = measures(N, t["X"], t["P"], t["state_out"], corners, gravity).astype(np.float32)
    before = outcome["end_tick"] >= 0
    code = np.array([wr.tick_code(before[b], bool(t["ok"][b]), t["info"][b, 5], t["state_out"][b]) for b in range(B)])
    lcode = np.array([limit_code(m32[b], lim) if code[b] == 0 else 0 for b in range(B)])
    fell = (lcode > 0) & bool(stop_mask & STOP_LIMITS)
    outcome["end_tick"][fell] = tick
    row, stats = wr.record_tick(N, tick, stop_mask & 7, t["X"], t["P"], t["info"], t["ok"], t["land"], t["state_out"], t["zmp"], box_upper, box_lower, outcome)
    outcome["end_code"][fell] = lcode[fell]
    row["code"][lcode > 0] = lcode[lcode > 0]
    stats[0] += fell.sum()
    stats[1] += fell.sum()
    stats[5] = (lcode > 0).sum()
    ended_now = (outcome["end_tick"] >= 0) & ~before
    good = ~before & ~ended_now
    row["measures"] = np.where((good | fell)[:, None], m32, np.float32(np.nan)).astype(np.float32)
    if extremes is not None:
        for b in np.flatnonzero(good):
            e, m = extremes[b], m32[b]
            e[0] = m[0] if m[0] < e[0] else e[0]
            e[1] = m[0] if m[0] > e[1] else e[1]
            e[2] = m[1] if m[1] > e[2] else e[2]
            e[3] = m[2] if m[2] < e[3] else e[3]
            e[4] = m[3] if m[3] > e[4] else e[4]
    return row, stats


def reference(N, ticks, outcome, stop_mask, box_upper, box_lower, lim, corners, gravity, tick0=11):
    """the restatement over consecutive ticks: (rows, stats[T, 6], final outcome, extremes); `outcome` is not modified"""
    out = {k: a.copy() for k, a in outcome.items()}
    ext = new_extremes(ticks[0]["X"].shape[0])
    rows, stats = [], []
    for i, t in enumerate(ticks):
        r, st = record_tick(N, tick0 + i, stop_mask, t, box_upper, box_lower, out, lim, corners, gravity, ext)
        rows.append(r); stats.append(st)
    return rows, np.stack(stats), out, ext


def predict_endings(m32, code, lim):
    """a walk under lim with the limits bit set, from the float32 measures m32[T, B, 4] and the codes code[T, B] of the same walk without limits:
    (end_tick[B], end_code[B]) -- a problem ends at the first tick whose code is not 0 or whose measures break a limit"""
    T, B = code.shape
    end_tick, end_code = np.full(B, -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        for t in range(T):
            c = int(code[t, b]) if code[t, b] != 0 else limit_code(m32[t, b], lim)
            if c != 0:
                end_tick[b], end_code[b] = t, c
                break
    return end_tick, end_code


# ---- crafted ticks: two feet on the ground plane and a state placed against them ----
SUPPORTS = ("LR", "L", "R", "")
CORNERS = np.array([[[0.08, 0.03, 0], [0.08, -0.03, 0], [-0.08, -0.03, 0], [-0.08, 0.03, 0]]] * 2, np.float32)     # a sole of 16 cm x 6 cm per foot


def stand(rng, N, t, support, yaw=None):
    """gives the tick t (tests/walk_record_ref._tick) a stage 1 to measure: feet near (0, +-0.08, 0) under a yaw, support[b] in SUPPORTS as the Gamma
    of stage 1, a state near (0, 0, 0.7) with a velocity (entries that the tick made non-finite stay so) and a comRef near the CoM"""
    L = cm.Layout(N)
    B = t["X"].shape[0]
    yaw = rng.uniform(-0.5, 0.5, (B, 2)) if yaw is None else np.asarray(yaw, np.float64)
    for b in range(B):
        old = t["state_out"][b].copy()
        for c in range(2):
            t["X"][b, L.pos[c] + 3:L.pos[c] + 6] = [rng.uniform(-0.02, 0.02), (0.08 if c == 0 else -0.08) + rng.uniform(-0.01, 0.01), rng.uniform(-0.005, 0.005)]
            cy, sy = np.cos(yaw[b, c]), np.sin(yaw[b, c])
            Rm = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
            t["P"][b, L.p_R[c] + 9:L.p_R[c] + 18] = Rm.reshape(-1, order="F")
            t["P"][b, L.p_gam[c] + 1] = 1.0 if "LR"[c] in support[b] else 0.0
        t["state_out"][b] = np.concatenate([[rng.uniform(-0.03, 0.03), rng.uniform(-0.05, 0.05), 0.7 + rng.uniform(-0.02, 0.02)], rng.uniform(-0.3, 0.3, 3),
                                            rng.uniform(-0.1, 0.1, 3)])
        t["P"][b, L.p_comref + 3:L.p_comref + 6] = t["state_out"][b, :3] + rng.uniform(-0.05, 0.05, 3).astype(np.float32)
        t["state_out"][b][~np.isfinite(old)] = old[~np.isfinite(old)]
    return t


def random_ticks(N, B, seed, n=2):
    """tests/walk_record_ref.random_ticks (random codes 0..5, one problem in eight ended earlier) with a stage 1 of random support under every tick,
    and three problems in ten thrown up to 0.4 m off their feet along every axis"""
    ticks, out = wr.random_ticks(N, B, seed, n)
    rng = np.random.default_rng(seed + 1000)
    for t in ticks:
        stand(rng, N, t, rng.choice(SUPPORTS, B, p=[0.5, 0.2, 0.2, 0.1]))
        wild = rng.random(B) < 0.3
        t["state_out"][wild, :3] += rng.uniform(-0.4, 0.4, (int(wild.sum()), 3)).astype(np.float32)
    return ticks, out
