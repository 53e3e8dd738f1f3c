"""Float64 restatement of the plant-model mismatch (include/cmpc.h, "plant-model mismatch on the device walk"; DESIGN.md 7f, "Mismatch"), built on what
exists: the plant is oracle/plant_ref.plant_step on a copy of x with the knot-0 forces times the gain and a copy of p with the knot-0 wrench plus the hidden
one; its Jacobian is tests/rollout_adjoint_ref.plant_jacobian at those inputs with the chain rule
    d/d f_q = gain d/d(gain f_q),   d/d hidden = d/d (fExt_0 | tauExt_0),   d/d gain = sum_q d/d(gain f_q) f_q;
the tick VJP is rollout_adjoint_ref.tick_vjp with that plant, the com0 / dcom0 / h0 rows of the solve's gP split off as the gradient of the state noise.
Test infrastructure: no GPU.  tests/test_mismatch_cpu.py holds it to central differences; tests/test_gpu_mismatch.py holds the kernels to it."""
import numpy as np

import cmpc_amd as cm
from oracle import plant_ref
from tests import rollout_adjoint_ref as ra

# columns of the mismatched plant's Jacobian: rollout_adjoint_ref's 69 (the force columns now with respect to the MPC's forces) | hidden 6 | gain 1
C_HID, C_GAIN, NCOL = ra.NCOL, ra.NCOL + 6, ra.NCOL + 7


def applied_inputs(L, x, p, hidden=None, gain=1.0):
    """(x with the knot-0 corner forces times gain, p with the knot-0 wrench plus hidden), float64 copies"""
    x2, p2 = np.array(x, np.float64), np.array(p, np.float64)
    for c in range(2):
        for j in range(4):
            x2[L.f[c][j]:L.f[c][j] + 3] *= float(gain)
    if hidden is not None:
        h = np.asarray(hidden, np.float64)
        p2[L.p_fext:L.p_fext + 3] += h[0:3]
        p2[L.p_text:L.p_text + 3] += h[3:6]
    return x2, p2


def plant_step(L, corners, x, p, state, step, substeps, hidden=None, gain=1.0, **kw):
    """-> (new_state[9], zmp[2]) of the mismatched plant"""
    x2, p2 = applied_inputs(L, x, p, hidden, gain)
    return plant_ref.plant_step(L, np.asarray(corners, np.float64).reshape(2, 4, 3), x2, p2, np.asarray(state, np.float64), step, substeps, **kw)


def zmp_branches(L, corners, x, p, gain=1.0, threshold=0.001):
    """the two thresholds of the plant's ZMP as the APPLIED force decides them -> (foot_in (bool, bool): the foot's F_z > threshold, defined: the F_z of
    the feet that are in sum to more than threshold, margin: the smallest |F_z / threshold - 1| over the feet in contact and the sum, so that a caller can
    require float32 and float64 to agree on the side)"""
    x2, _ = applied_inputs(L, x, p, None, gain)
    fz = [sum(x2[L.f[c][j] + 2] for j in range(4)) if p[L.p_gam[c]] > 0.5 else None for c in range(2)]
    foot_in = tuple(bool(f is not None and f > threshold) for f in fz)
    ztot = sum(f for f, on in zip(fz, foot_in) if on)
    sides = [abs(f / threshold - 1.0) for f in fz if f is not None] + [abs(ztot / threshold - 1.0)]
    return foot_in, bool(ztot > threshold), min(sides)


def free_fall(state, f_ext, tau_ext, duration, gravity=ra.GRAVITY):
    """the plant with no contact force applied (gain = 0, or both feet in the air), closed form over `duration`: a = f_ext - g e_z,
    com' = com + T v + T^2/2 a, v' = v + T a, h' = h + T tau_ext (there is no force for the CoM to have a lever arm to)"""
    s = np.asarray(state, np.float64)
    a = np.asarray(f_ext, np.float64) - np.array([0.0, 0.0, gravity])
    T = float(duration)
    return np.concatenate([s[0:3] + T * s[3:6] + 0.5 * T * T * a, s[3:6] + T * a, s[6:9] + T * np.asarray(tau_ext, np.float64)])


def schedule_row(schedule, tick_first, tick):
    """row of tick number `tick` of a schedule [rows, B, .] whose row 0 is tick `tick_first`; None outside it (the term is then not applied)"""
    r = int(tick) - int(tick_first)
    return schedule[r] if schedule is not None and 0 <= r < len(schedule) else None


def walk_plant_gaps(L, corners_of, tape, mismatch, problems=None):
    """Every tick of a taped mismatched walk through the restated plant: plant_step(tape X[i], tape P[i], tape states[i] (the TRUE state), tick i's hidden
    row or None, the gain) against tape states[i + 1].  tape: host arrays X, P [T, B, .], states [T + 1, B, 9], step (float32), substeps; corners_of(b)
    -> [2][4][3] float64 of problem b; mismatch: host arrays.  -> (gap[T, B] largest absolute difference, gamma[T, B, 2] the contact flags of knot 0)"""
    T, B = tape["X"].shape[0], tape["X"].shape[1]
    problems = range(B) if problems is None else problems
    gain = mismatch.get("force_gain")
    gap, gamma = np.zeros((T, B)), np.zeros((T, B, 2), bool)
    step = float(np.float32(tape["step"]))
    for i in range(T):
        hid = schedule_row(mismatch.get("hidden_wrench"), mismatch.get("tick_first", 0), i)
        for b in problems:
            ref, _ = plant_step(L, corners_of(b), tape["X"][i, b], tape["P"][i, b], tape["states"][i, b], step, int(tape["substeps"]),
                                None if hid is None else hid[b], 1.0 if gain is None else float(gain[b]), gravity=float(np.float32(ra.GRAVITY)))
            gap[i, b] = np.abs(np.asarray(tape["states"][i + 1, b], np.float64) - ref).max()
            gamma[i, b] = [tape["P"][i, b, L.p_gam[c]] > 0.5 for c in range(2)]
    return gap, gamma


def plant_jacobian(L, corners, x, p, state, step, substeps, hidden=None, gain=1.0, gravity=ra.GRAVITY):
    """[9, 76] = d state' / d (state, pos_0, f_0 (the MPC's), fExt_0, tauExt_0, corners, hidden, gain)"""
    x2, p2 = applied_inputs(L, x, p, hidden, gain)
    J0 = ra.plant_jacobian(L, corners, x2, p2, state, step, substeps, gravity)
    J = np.zeros((9, NCOL))
    J[:, :ra.NCOL] = J0
    J[:, ra.C_F:ra.C_FEXT] = float(gain) * J0[:, ra.C_F:ra.C_FEXT]
    J[:, C_HID:C_HID + 6] = J0[:, ra.C_FEXT:ra.C_CORN]
    xi, _ = ra.plant_columns(L)
    f_raw = np.asarray(x, np.float64)[xi[6:]]           # the 24 knot-0 forces as the MPC gave them (the columns of a gated-off foot are zero in J0)
    J[:, C_GAIN] = J0[:, ra.C_F:ra.C_FEXT] @ f_raw
    return J


def plant_vjp(L, corners, x, p, state, step, substeps, g_out, hidden=None, gain=1.0, gravity=ra.GRAVITY):
    """-> (g_state[9], g_x[n_x], g_p[n_p], g_model[34], g_hidden[6], g_gain)"""
    J = plant_jacobian(L, corners, x, p, state, step, substeps, hidden, gain, gravity)
    xi, pi = ra.plant_columns(L)
    g = J.T @ np.asarray(g_out, np.float64)
    gx, gp, gm = np.zeros(L.nx), np.zeros(L.np), np.zeros(34)
    gx[xi] = g[ra.C_POS:ra.C_FEXT]
    gp[pi] = g[ra.C_FEXT:ra.C_CORN]
    gm[10:34] = g[ra.C_CORN:ra.NCOL]
    return g[0:9], gx, gp, gm, g[C_HID:C_HID + 6], float(g[C_GAIN])


def tick_vjp(cfg, tape, now, g_state_out, g_list_out=None, g_x=None, theta=None, gravity=ra.GRAVITY):
    """rollout_adjoint_ref.tick_vjp with the mismatched plant: tape as there (state: the TRUE state, P: what the solve saw) plus hidden[6] or None and gain
    (default 1).  -> its dict plus hidden[6], noise[9], gain; a flagged tick has zeros in all three."""
    L = cm.Layout(cfg.N)
    hidden, gain = tape.get("hidden"), float(tape.get("gain", 1.0))
    extra = {}

    def plant(L_, corners, x, p, state, step, substeps, g_out, gravity_=ra.GRAVITY):
        gs, gx, gp, gm, gh, gg = plant_vjp(L_, corners, x, p, state, step, substeps, g_out, hidden, gain, gravity_)
        extra.update(hidden=gh, gain=gg)
        return gs, gx, gp, gm
    saved = ra.plant_vjp
    ra.plant_vjp = plant
    try:
        r = ra.tick_vjp(cfg, tape, now, g_state_out, g_list_out, g_x, theta, gravity)
    finally:
        ra.plant_vjp = saved
    if r["status"] != 0:
        return dict(r, hidden=np.zeros(6), noise=np.zeros(9), gain=0.0)
    return dict(r, hidden=extra["hidden"], noise=r["p_sol"][L.p_com0:L.p_com0 + 9].copy(), gain=extra["gain"])


def reverse_sweep(cfg, tapes, nows, g_states, g_X=None, theta=None, push_knots=None):
    """rollout_adjoint_ref.reverse_sweep over mismatched ticks -> its dict plus hidden_wrench[T][6], state_noise[T][9], force_gain (summed last tick first)"""
    T = len(tapes)
    rows = dict(hidden_wrench=[None] * T, state_noise=[None] * T, force_gain=0.0)
    it = iter(reversed(range(T)))

    def tick(cfg_, tape, now, g, gl, gx, th):
        i = next(it)
        r = tick_vjp(cfg_, tape, now, g, gl, gx, th)
        rows["hidden_wrench"][i], rows["state_noise"][i] = r["hidden"], r["noise"]
        rows["force_gain"] += r["gain"]
        return r
    out = ra.reverse_sweep(cfg, tapes, nows, g_states, g_X, theta, push_knots, tick=tick)
    out.update(hidden_wrench=np.array(rows["hidden_wrench"]), state_noise=np.array(rows["state_noise"]), force_gain=rows["force_gain"])
    return out
