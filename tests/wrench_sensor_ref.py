"""The wrench sensor of a sensed walk (include/cmpc.h, cmpc_wrench_sensor) restated in plain numpy, float64, with no code shared with the library: the
rule, its Jacobian on the branch taken, its VJP and its JVP.  The rule is piecewise linear -- linear on each side of the dead-band -- so the Jacobian is a
matrix of 0, +1 and -1 and the derivative forms are products with it.

Schedules: hidden[Th, B, 6] and noise[Tn, B, 6] (or None), row r = tick - tick_first.  The float32 roundings the library makes are made here by the caller
(as_float32=True): ONE add for the reading, ONE subtract for the plant row."""
import numpy as np


def _row(sched, r, b):
    """row r of a schedule for problem b when it is inside, else None (a select: the outside is never read)"""
    return None if sched is None or r < 0 or r >= sched.shape[0] else sched[r, b]


def reading(hidden, noise, tick_first, delay, t, b, as_float32=False):
    """the sensor's reading of tick t: the hidden row of tick t - delay plus the noise row of tick t"""
    src = _row(hidden, t - delay - tick_first, b)
    nz = _row(noise, t - tick_first, b)
    dt = np.float32 if as_float32 else np.float64
    out = np.zeros(6, dt) if src is None else np.array(src, dt)
    if nz is not None:
        out = (out + np.array(nz, dt)).astype(dt)
    return out


def passes(read, deadband):
    """not (|force|^2 < deadband^2), both squares in float64: a force on the threshold passes and so does a NaN"""
    f = np.asarray(read[:3], np.float64)
    n2 = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]
    band2 = np.float64(deadband) * np.float64(deadband)
    return not (n2 < band2)


def sense(N, hidden, noise, tick_first, delay, hold, deadband, tick0, rows, as_float32=False):
    """-> wrench_rows[rows, B, N, 6], plant[rows, B, 6], pass[rows, B]"""
    B = hidden.shape[1]
    dt = np.float32 if as_float32 else np.float64
    wr = np.zeros((rows, B, N, 6), dt)
    pl = np.zeros((rows, B, 6), dt)
    ps = np.zeros((rows, B), np.int32)
    for r in range(rows):
        t = tick0 + r
        for b in range(B):
            read = reading(hidden, noise, tick_first, delay, t, b, as_float32)
            true = _row(hidden, t - tick_first, b)
            true = np.zeros(6, dt) if true is None else np.array(true, dt)
            if passes(read, deadband):
                ps[r, b] = 1
                wr[r, b, :hold] = read
                pl[r, b] = (true - read).astype(dt)
            else:
                pl[r, b] = true
    return wr, pl, ps


def jacobian(N, hidden, noise, tick_first, delay, hold, deadband, tick0, rows):
    """d(wrench_rows, plant) / d(hidden, noise) on the branch the inputs take: a dense matrix [rows B N 6 + rows B 6, Th B 6 + Tn B 6]"""
    Th, B = hidden.shape[:2]
    Tn = 0 if noise is None else noise.shape[0]
    n_w, n_p = rows * B * N * 6, rows * B * 6
    J = np.zeros((n_w + n_p, (Th + Tn) * B * 6))
    col_h = lambda r, b, c: (r * B + b) * 6 + c
    col_n = lambda r, b, c: Th * B * 6 + (r * B + b) * 6 + c
    row_w = lambda r, b, k, c: ((r * B + b) * N + k) * 6 + c
    row_p = lambda r, b, c: n_w + (r * B + b) * 6 + c
    for r in range(rows):
        t = tick0 + r
        for b in range(B):
            p = passes(reading(hidden, noise, tick_first, delay, t, b), deadband)
            rt, rs, rn = t - tick_first, t - delay - tick_first, t - tick_first
            for c in range(6):
                if 0 <= rt < Th:
                    J[row_p(r, b, c), col_h(rt, b, c)] += 1.0
                if not p:
                    continue
                if 0 <= rs < Th:
                    J[row_p(r, b, c), col_h(rs, b, c)] -= 1.0
                    for k in range(hold):
                        J[row_w(r, b, k, c), col_h(rs, b, c)] += 1.0
                if 0 <= rn < Tn:
                    J[row_p(r, b, c), col_n(rn, b, c)] -= 1.0
                    for k in range(hold):
                        J[row_w(r, b, k, c), col_n(rn, b, c)] += 1.0
    return J


def vjp(N, hidden, noise, tick_first, delay, hold, deadband, tick0, rows, grad_wrench, grad_plant):
    """J^T applied to (grad_wrench[rows, B, N, 6], grad_plant[rows, B, 6]) -> grad_hidden[Th, B, 6], grad_noise[Tn, B, 6] or None"""
    J = jacobian(N, hidden, noise, tick_first, delay, hold, deadband, tick0, rows)
    g = J.T @ np.concatenate([np.asarray(grad_wrench, np.float64).ravel(), np.asarray(grad_plant, np.float64).ravel()])
    nh = hidden.size
    return g[:nh].reshape(hidden.shape), (None if noise is None else g[nh:].reshape(noise.shape))


def jvp(N, hidden, noise, tick_first, delay, hold, deadband, tick0, rows, dir_hidden, dir_noise):
    """J applied to (dir_hidden[Th, B, 6], dir_noise[Tn, B, 6] or None) -> dir_wrench[rows, B, N, 6], dir_plant[rows, B, 6]"""
    J = jacobian(N, hidden, noise, tick_first, delay, hold, deadband, tick0, rows)
    d = [np.asarray(dir_hidden, np.float64).ravel()]
    if noise is not None:
        d.append(np.zeros(noise.size) if dir_noise is None else np.asarray(dir_noise, np.float64).ravel())
    out = J @ np.concatenate(d)
    B = hidden.shape[1]
    n_w = rows * B * N * 6
    return out[:n_w].reshape(rows, B, N, 6), out[n_w:].reshape(rows, B, 6)
