"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the reference rows' derivative in the planner's trajectories (include/cmpc.h,
cmpc_reference_from_planner_vjp / _jvp).  It shares nothing with the code under test: the map trajectories -> (comRef, hRef) of one tick is linear, so its
matrix is oracle/plant_ref.resample_references applied to unit trajectories at that tick's t_offset -- with com_height = NaN to see the z row, with a
number after subtracting the image of zero (the constant height).  The VJP is sum_r W_r^T g_r over the rows the ending rule admits."""
import numpy as np

from oracle import plant_ref


def t_offset(tick, dt, t_first):
    """where tick number `tick` reads the trajectories: now - t_first, now = tick * dt"""
    return tick * dt - t_first


def matrices(N, dt, knots, in_dt, toff, mass, com_height):
    """-> (Wc, Wh) [N + 1, 3, knots]: comRef_k[a] = sum_j Wc[k, a, j] c[j][a] (+ the constant height), hRef_k[a] = sum_j Wh[k, a, j] h[j][a]"""
    zero = np.zeros((knots, 3))
    c0, h0 = plant_ref.resample_references(zero, zero, in_dt, toff, N, dt, mass, com_height)
    Wc, Wh = np.zeros((N + 1, 3, knots)), np.zeros((N + 1, 3, knots))
    for j in range(knots):
        unit = zero.copy()
        unit[j] = 1.0
        c, h = plant_ref.resample_references(unit, unit, in_dt, toff, N, dt, mass, com_height)
        Wc[:, :, j], Wh[:, :, j] = c - c0, h - h0
    return Wc, Wh


def admitted_rows(end_tick, b, tick0, rows):
    """rows of problem b with tick0 + r < e (e < 0: never ended)"""
    e = -1 if end_tick is None else int(end_tick[b])
    return rows if e < 0 else int(min(max(e - tick0, 0), rows))


def reference_rows(L, g_row):
    """g_row [..., n_p] -> (gc, gh) [..., N + 1, 3]: its comRef / hRef entries"""
    n3 = 3 * (L.N + 1)
    shape = g_row.shape[:-1] + (L.N + 1, 3)
    return g_row[..., L.p_comref:L.p_comref + n3].reshape(shape), g_row[..., L.p_href:L.p_href + n3].reshape(shape)


def vjp(L, dt, tick0, rows, knots, in_dt, t_first, mass, com_height, end_tick, grad_p, start_com, start_h):
    """-> (grad_com, grad_h, mag_com, mag_h, terms_com, terms_h) [B, knots, 3]: the sums (start value included), the sums of the terms' magnitudes and
    the numbers of terms, for the test's bound.  Entries the rule excludes are never touched, so NaN there does not reach the result."""
    B = grad_p.shape[1]
    out = [start_com.astype(np.float64).copy(), start_h.astype(np.float64).copy()]
    mag = [np.abs(out[0]), np.abs(out[1])]
    cnt = [np.ones_like(out[0]), np.ones_like(out[1])]
    for r in range(rows):
        W = matrices(L.N, dt, knots, in_dt, t_offset(tick0 + r, dt, t_first), mass, com_height)
        for b in range(B):
            if r >= admitted_rows(end_tick, b, tick0, rows):
                continue
            g = reference_rows(L, grad_p[r, b].astype(np.float64))
            for q in range(2):
                for k in range(L.N + 1):
                    for a in range(3):
                        js = np.nonzero(W[q][k, a])[0]
                        for j in js:
                            term = W[q][k, a, j] * g[q][k, a]
                            out[q][b, j, a] += term
                            mag[q][b, j, a] += abs(term)
                            cnt[q][b, j, a] += 1
    return out[0], out[1], mag[0], mag[1], cnt[0], cnt[1]


def jvp(L, dt, tick, knots, in_dt, t_first, mass, com_height, dir_com, dir_h):
    """one column's directions [knots, 3] -> (d comRef, d hRef) [N + 1, 3] float64 of tick `tick`"""
    Wc, Wh = matrices(L.N, dt, knots, in_dt, t_offset(tick, dt, t_first), mass, com_height)
    return np.einsum("kaj,ja->ka", Wc, dir_com), np.einsum("kaj,ja->ka", Wh, dir_h)
