"""TEST INFRASTRUCTURE ONLY -- independent restatement, plain Python on exact integers, of forceSampleTime: the snap of a planner's contact lists
to the MPC grid that the reference makes on every tick before the merge (ContactPhaseList::forceSampleTime(m_dT),
src/centroidal-mpc-walking/src/CentroidalMPCBlock.cpp:586-592).

PARITY UNPINNED: the rule lives in BipedalLocomotionFramework, whose source is not in the reference tree.  This file restates the rule stated in
include/cmpc.h (cmpc_contacts_force_sample_time) and shares no code with the product's statement of it (csrc/cmpc_contacts.h):
    t_ns = llround(t 1e9), dt_ns = llround(dt 1e9)           (llround: to nearest, halves away from zero)
    on the grid (t_ns % dt_ns == 0): t unchanged, to the bit
    |t| >= 1e9 s: unchanged ("never")
    else q = floor((2 t_ns + dt_ns) / (2 dt_ns)), snapped t = float(q dt_ns) * 1e-9
    a contact fails when a time is not finite, or when its duration is positive and its snapped duration is zero."""
import math
from fractions import Fraction

import numpy as np

NEVER = 1e9


def llround(x: float) -> int:
    """C's llround on the exact value of the double x"""
    f = Fraction(x)
    r = math.floor(abs(f) + Fraction(1, 2))
    return r if f >= 0 else -r


def dt_in_ns(dt: float) -> int:
    return llround(dt * 1e9)


def snap_time(t: float, dt_ns: int):
    """-> (snapped time, finite)"""
    if not math.isfinite(t):
        return t, False
    if abs(t) >= NEVER:
        return t, True
    t_ns = llround(t * 1e9)
    if t_ns % dt_ns == 0:
        return t, True
    q = (2 * t_ns + dt_ns) // (2 * dt_ns)     # Python's // is floor division
    return float(q * dt_ns) * 1e-9, True


def snap_contact(a: float, d: float, dt_ns: int):
    """-> (snapped activation, snapped deactivation, ok)"""
    sa, fa = snap_time(a, dt_ns)
    sd, fd = snap_time(d, dt_ns)
    return sa, sd, fa and fd and not (d > a and sd == sa)


def snap_lists(dt: float, t, n):
    """t[B,2,M,2] float64, n[B,2] -> (snapped copy of t, ok[B] bool).  Entries beyond n are copied unchanged."""
    dt_ns = dt_in_ns(dt)
    t = np.asarray(t, np.float64)
    out = t.copy()
    ok = np.ones(t.shape[0], bool)
    for b in range(t.shape[0]):
        for c in range(2):
            for m in range(int(n[b][c])):
                sa, sd, good = snap_contact(float(t[b, c, m, 0]), float(t[b, c, m, 1]), dt_ns)
                out[b, c, m, 0], out[b, c, m, 1] = sa, sd
                ok[b] &= good
    return out, ok


def random_lists(rng, B, M, dt, n_min=0):
    """B problems of two feet with up to M contacts, times drawn to cover the rule's corners: exact grid points (k dt as a float, and k dt_ns / 1e9),
    ties (half-way between two grid points), negative times, random off-grid times, the 1e9 s sentinel, durations that collapse (shorter than dt
    inside one grid cell) and non-finite times.  -> (t[B,2,M,2], n[B,2] int32)."""
    dt_ns = dt_in_ns(dt)
    t = np.zeros((B, 2, M, 2))
    n = rng.integers(n_min, M + 1, (B, 2)).astype(np.int32)

    def draw():
        kind = rng.integers(9)
        k = int(rng.integers(-200, 200))
        if kind == 0:
            return k * dt                                     # on the grid (as a float product)
        if kind == 1:
            return (k * dt_ns) / 1e9                          # on the grid (from nanoseconds)
        if kind == 2:
            return (k * dt_ns + dt_ns // 2) / 1e9             # a tie when dt_ns is even
        if kind == 3:
            return (k * dt_ns + dt_ns // 2 + int(rng.choice([-1, 1]))) / 1e9   # one nanosecond either side of a tie
        if kind == 4:
            return float(rng.choice([NEVER, -NEVER, 2e9, 1e12]))
        return float(rng.uniform(-12.0, 12.0))

    for b in range(B):
        for c in range(2):
            for m in range(M):
                a = draw()
                kind = rng.integers(6)
                if kind == 0:
                    d = a                                     # zero duration (never a failure)
                elif kind == 1:
                    d = a + float(rng.uniform(0.0, 0.3)) * dt  # short: collapses unless it straddles a rounding boundary
                elif kind == 2:
                    d = NEVER
                elif kind == 3 and rng.random() < 0.3:
                    d = float(rng.choice([np.nan, np.inf, -np.inf]))
                else:
                    d = a + float(rng.uniform(0.0, 3.0))
                t[b, c, m] = (a, d)
    return t, n
