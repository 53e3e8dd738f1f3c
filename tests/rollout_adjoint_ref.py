"""Float64 restatement of the roll-out tick in reverse (include/cmpc.h: cmpc_plant_step_jvp_device / _vjp_device, cmpc_contacts_position_vjp_device,
cmpc_rollout_tick_vjp_device), one problem at a time, built on tests/sens_ref.Sens and tests/sens_model_ref.ModelSens for the solve and on
the oracle's ContactList queries (oracle/contacts_ref.py, integer nanoseconds as oracle/schedule_ref.py) for the index maps of the list path.

  * plant: the dense Jacobian of oracle/plant_ref.plant_step's map, d state' / d (state, pos_0, f_0, fExt_0, tauExt_0, corners), from the closed form of the
    Runge-Kutta sweep (the dynamics are affine and nilpotent with the forces held); JVP = J d, VJP = J^T g.
  * lists: the adjoint of adjust, sample and merge in the contacts' positions.
  * tick: plant VJP -> adjust -> solution VJP (p and model) -> state rows of gP -> sample + merge;  reverse_sweep chains ticks.

Test infrastructure: no GPU.  tests/test_rollout_adjoint_cpu.py holds it to finite differences and brute force; tests/test_gpu_rollout_adjoint.py holds the
device kernels to it."""
import numpy as np

import cmpc_amd as cm
from oracle import contacts_ref
from tests import sens_model_ref, snap_ref

NS = 1_000_000_000
GRAVITY = 9.80665


def _skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


# ---------------------------------------------------------------------------------------------------------------- plant
# columns of the dense plant Jacobian: state 9 | pos (c, i) 6 | forces (c, j, i) 24 | fExt_0 3 | tauExt_0 3 | corners (c, j, i) 24
C_STATE, C_POS, C_F, C_FEXT, C_TEXT, C_CORN, NCOL = 0, 9, 15, 39, 42, 45, 69


def plant_jacobian(L, corners, x, p, state, step, substeps, gravity=GRAVITY):
    """[9, 69] = d state' / d (state, pos_0, f_0, fExt_0, tauExt_0, corners) at (x, p, state); the forces of a foot with Gamma_c,0 <= 0.5 are gated off."""
    x, p, state = (np.asarray(a, np.float64) for a in (x, p, state))
    corners = np.asarray(corners, np.float64).reshape(2, 4, 3)
    T = float(substeps) * float(step)
    c0, v0 = state[0:3], state[3:6]
    R = [p[L.p_R[c]:L.p_R[c] + 9].reshape(3, 3, order="F") for c in range(2)]
    on = [p[L.p_gam[c]] > 0.5 for c in range(2)]
    f = np.array([[x[L.f[c][j]:L.f[c][j] + 3] if on[c] else np.zeros(3) for j in range(4)] for c in range(2)])
    cp = np.array([[x[L.pos[c]:L.pos[c] + 3] + R[c] @ corners[c][j] for j in range(4)] for c in range(2)])
    F = f.sum((0, 1))
    a = F + p[L.p_fext:L.p_fext + 3] - np.array([0.0, 0.0, gravity])
    Iint = T * c0 + 0.5 * T * T * v0 + T ** 3 / 6.0 * a
    I3, SF = np.eye(3), _skew(F)
    J = np.zeros((9, NCOL))
    J[0:3, 0:3] = I3; J[0:3, 3:6] = T * I3
    J[3:6, 3:6] = I3
    J[6:9, 6:9] = I3; J[6:9, 0:3] = T * SF; J[6:9, 3:6] = 0.5 * T * T * SF
    J[0:3, C_FEXT:C_FEXT + 3] = 0.5 * T * T * I3
    J[3:6, C_FEXT:C_FEXT + 3] = T * I3
    J[6:9, C_FEXT:C_FEXT + 3] = T ** 3 / 6.0 * SF
    J[6:9, C_TEXT:C_TEXT + 3] = T * I3
    for c in range(2):
        for j in range(4):
            q = 4 * c + j
            if on[c]:
                J[0:3, C_F + 3 * q:C_F + 3 * q + 3] = 0.5 * T * T * I3
                J[3:6, C_F + 3 * q:C_F + 3 * q + 3] = T * I3
                J[6:9, C_F + 3 * q:C_F + 3 * q + 3] = T * _skew(cp[c][j]) + T ** 3 / 6.0 * SF - _skew(Iint)
            J[6:9, C_POS + 3 * c:C_POS + 3 * c + 3] += -T * _skew(f[c][j])
            J[6:9, C_CORN + 3 * q:C_CORN + 3 * q + 3] = -T * _skew(f[c][j]) @ R[c]
    return J


def plant_columns(L):
    """(x indices of columns 9..39, p indices of columns 39..45): where the Jacobian's columns live in x and p"""
    xi = [L.pos[c] + i for c in range(2) for i in range(3)] + [L.f[c][j] + i for c in range(2) for j in range(4) for i in range(3)]
    pi = [L.p_fext + i for i in range(3)] + [L.p_text + i for i in range(3)]
    return np.array(xi), np.array(pi)


def plant_jvp(L, corners, x, p, state, step, substeps, d_state, d_x=None, d_p=None, d_model=None, gravity=GRAVITY):
    """d state' [9] along (d_state[9], d_x[n_x], d_p[n_p], d_model[34]); None = zero"""
    J = plant_jacobian(L, corners, x, p, state, step, substeps, gravity)
    xi, pi = plant_columns(L)
    d = np.zeros(NCOL)
    d[0:9] = d_state
    if d_x is not None:
        d[C_POS:C_FEXT] = np.asarray(d_x, np.float64)[xi]
    if d_p is not None:
        d[C_FEXT:C_CORN] = np.asarray(d_p, np.float64)[pi]
    if d_model is not None:
        d[C_CORN:] = np.asarray(d_model, np.float64)[10:34]
    return J @ d


def plant_vjp(L, corners, x, p, state, step, substeps, g_out, gravity=GRAVITY):
    """-> (g_state[9], g_x[n_x], g_p[n_p], g_model[34])"""
    J = plant_jacobian(L, corners, x, p, state, step, substeps, gravity)
    xi, pi = plant_columns(L)
    g = J.T @ np.asarray(g_out, np.float64)
    gx, gp, gm = np.zeros(L.nx), np.zeros(L.np), np.zeros(34)
    gx[xi] = g[C_POS:C_FEXT]
    gp[pi] = g[C_FEXT:C_CORN]
    gm[10:34] = g[C_CORN:]
    return g[0:9], gx, gp, gm


# ---------------------------------------------------------------------------------------------------------------- lists
def _ns(t):
    return int(round(float(t) * NS))


def _as_list(t, n):
    """t[M][2], n -> the oracle's contact list on integer nanoseconds, each contact carrying its index"""
    return [dict(activation=_ns(t[m][0]), deactivation=_ns(t[m][1]), idx=m) for m in range(int(n))]


def _active(lst, t_ns):
    c = contacts_ref.get_active_contact(lst, t_ns)
    return -1 if c is None else c["idx"]


def _next(lst, t_ns):
    i = contacts_ref.get_next_contact_index(lst, t_ns)
    return i if i < len(lst) else -1


def _owner(lst, t_ns):
    m = _active(lst, t_ns)
    if m >= 0:
        return m
    m = _next(lst, t_ns)
    return m if m >= 0 else len(lst) - 1


def list_position_vjp(L, dt, now, list_t, list_n, land, plan=None, prev=None, ok=True, g_out=None, g_p=None, force_sample_time=False, phase=3):
    """One problem.  list_t[2][M][2], list_n[2], land[2]; plan / prev = (t[2][M][2], n[2]) or None (prev None: first tick).
    -> dict(x=[n_x] what the adjust part adds to gX, prev=[2][M][3], plan=[2][M][3], status)."""
    N = L.N
    list_t = np.asarray(list_t, np.float64)
    M = list_t.shape[1]
    out = dict(x=np.zeros(L.nx), prev=np.zeros((2, M, 3)), plan=np.zeros((2, M, 3)), status=0 if ok else 5)
    if not ok:
        return out
    g_out = np.zeros((2, M, 3)) if g_out is None else np.asarray(g_out, np.float64)
    now_ns, dt_ns = _ns(now), _ns(dt)
    for c in range(2):
        n = int(list_n[c])
        sampled = 1 <= n <= M
        lst = _as_list(list_t[c], n) if sampled else []
        nx = -1
        if sampled and 0 <= int(land[c]) <= N:
            nx = _next(lst, now_ns)
        if (phase & 1) and nx >= 0:
            out["x"][L.pos[c] + 3 * int(land[c]):L.pos[c] + 3 * int(land[c]) + 3] += g_out[c][nx]
        if not (phase & 2):
            continue
        merge = prev is not None
        glist = np.zeros((M, 3))
        nlist = max(0, min(n, M))
        for m in range(nlist):
            if m != nx:
                glist[m] += g_out[c][m]
        if sampled and g_p is not None:
            gp = np.asarray(g_p, np.float64)
            for k in range(N):
                o = _owner(lst, now_ns + k * dt_ns)
                if k == 0:
                    glist[o] += gp[L.p_nom[c]:L.p_nom[c] + 3] + gp[L.p_cur[c]:L.p_cur[c] + 3]
                glist[o] += gp[L.p_nom[c] + 3 * (k + 1):L.p_nom[c] + 3 * (k + 1) + 3]
        if not merge:
            out["prev"][c] = glist
            continue
        pt = np.asarray(plan[0], np.float64)[c].copy()
        pn, mn = int(plan[1][c]), int(prev[1][c])
        if force_sample_time:
            grid = snap_ref.dt_in_ns(dt)
            for m in range(pn):
                pt[m][0], pt[m][1], _ = snap_ref.snap_contact(float(pt[m][0]), float(pt[m][1]), grid)
        ma = _active(_as_list(np.asarray(prev[0], np.float64)[c], mn), now_ns)
        first = _next(_as_list(pt, pn), now_ns)
        n0 = 1 if ma >= 0 else 0
        for m in range(nlist):
            if m < n0:
                out["prev"][c][ma] += glist[m]
            elif first >= 0 and first + m - n0 < M:
                out["plan"][c][first + m - n0] += glist[m]
    return out


# ---------------------------------------------------------------------------------------------------------------- tick
def tick_vjp(cfg, tape, now, g_state_out, g_list_out=None, g_x=None, theta=None, gravity=GRAVITY):
    """One tick of one problem in reverse.  tape: dict(X, P, lam_g, state, status (the solve's), ok, land, list_t, list_n, plan=(t, n), prev=(t, n) or None,
    step, substeps, force_sample_time).  -> dict(state[9], prev_list[2][M][3], plan[2][M][3], wrench[N][6], model[34], p[n_p], status, weak, ...).
    theta: the problem's model (default: cfg's)."""
    N = cfg.N
    L = cm.Layout(N)
    x, p, lam = (np.asarray(tape[k], np.float64) for k in ("X", "P", "lam_g"))
    M = np.asarray(tape["list_t"]).shape[1]
    zero = dict(state=np.zeros(9), prev_list=np.zeros((2, M, 3)), plan=np.zeros((2, M, 3)), wrench=np.zeros((N, 6)), model=np.zeros(34),
                p=np.zeros(L.np), weak=0)
    if not tape.get("ok", True):
        return dict(zero, status=5)
    if not (np.isfinite(x).all() and np.isfinite(p).all() and np.isfinite(lam).all() and np.isfinite(np.asarray(tape["state"], np.float64)).all()):
        return dict(zero, status=2)
    if int(tape.get("status", 0)) != 0:
        return dict(zero, status=4)
    th = sens_model_ref.theta_of(cfg) if theta is None else np.asarray(theta, np.float64)
    corners = th[10:34].astype(np.float32).astype(np.float64)     # (the record the kernels read is float32)
    gs, gx, gp_plant, gm_plant = plant_vjp(L, corners, x, p, tape["state"], tape["step"], tape["substeps"], g_state_out, gravity)
    if g_x is not None:
        gx = gx + np.asarray(g_x, np.float64)
    lst = dict(list_t=tape["list_t"], list_n=tape["list_n"], land=tape["land"], plan=tape.get("plan"), prev=tape.get("prev"),
               force_sample_time=bool(tape.get("force_sample_time")))
    gx = gx + list_position_vjp(L, cfg.sampling_time, now, g_out=g_list_out, phase=1, **lst)["x"]
    MS = sens_model_ref.ModelSens(cfg, x, p, lam, theta=th)
    gp_sol = MS.S.vjp(gx)
    gm = MS.vjp(gx) + gm_plant
    gp = gp_sol + gp_plant
    back = list_position_vjp(L, cfg.sampling_time, now, g_out=g_list_out, g_p=gp_sol, phase=2, **lst)
    wrench = np.concatenate([gp[L.p_fext:L.p_fext + 3 * N].reshape(N, 3), gp[L.p_text:L.p_text + 3 * N].reshape(N, 3)], 1)
    return dict(state=gs + gp[L.p_com0:L.p_com0 + 9], prev_list=back["prev"], plan=back["plan"], wrench=wrench, model=gm, p=gp, status=0, weak=MS.S.weak,
                gx=gx, p_sol=gp_sol, model_sol=gm - gm_plant)     # (the last three: what went into and came out of the bare solution VJP)


def reverse_sweep(cfg, tapes, nows, g_states, g_X=None, theta=None, push_knots=None, tick=tick_vjp):
    """The ticks of one problem in reverse: g_states[T+1][9] = dl / d state_i (state_0 .. state_T), g_X[T][n_x] or None.
    -> dict(state0, list0, push[3] (the wrench gradients summed over the push_knots[i] first knots of tick i), wrench[T][N][6], models[34], plan, status[T])."""
    T = len(tapes)
    M = np.asarray(tapes[0]["list_t"]).shape[1]
    g = np.asarray(g_states[T], np.float64).copy()
    gl = np.zeros((2, M, 3))
    out = dict(push=np.zeros(3), wrench=[None] * T, models=np.zeros(34), plan=np.zeros((2, M, 3)), status=[0] * T)
    for i in reversed(range(T)):
        r = tick(cfg, tapes[i], nows[i], g, gl, None if g_X is None else g_X[i], theta)
        g = r["state"] + np.asarray(g_states[i], np.float64)
        gl = r["prev_list"]
        out["wrench"][i], out["status"][i] = r["wrench"], r["status"]
        out["models"] += r["model"]
        out["plan"] += r["plan"]
        if push_knots is not None and push_knots[i] > 0:
            out["push"] += r["wrench"][:push_knots[i], :3].sum(0)
    out["state0"], out["list0"] = g, gl
    out["wrench"] = np.array(out["wrench"])
    return out


# ---------------------------------------------------------------------------------------------------------------- forward mode (for the dense per-tick Jacobians)
def list_position_jvp(L, dt, now, list_t, list_n, land, d_prev, prev=None):
    """The forward list path of one problem along a perturbation d_prev[2][M][3] of the previous tick's positions (first tick: of the list itself; the
    planner's positions are not perturbed).  -> (d_p[n_p]: nominalPos / currentPos rows, d_list[2][M][3]: the merged list before the adjustment, nx[2]: the
    entry the adjustment overwrites with x.pos[land], or -1)."""
    N = L.N
    list_t = np.asarray(list_t, np.float64)
    M = list_t.shape[1]
    now_ns, dt_ns = _ns(now), _ns(dt)
    d_p, d_list, nxs = np.zeros(L.np), np.zeros((2, M, 3)), [-1, -1]
    for c in range(2):
        n = int(list_n[c])
        if prev is None:
            d_list[c, :n] = d_prev[c, :n]
        else:
            ma = _active(_as_list(np.asarray(prev[0], np.float64)[c], int(prev[1][c])), now_ns)
            if ma >= 0:
                d_list[c, 0] = d_prev[c, ma]
        if not 1 <= n <= M:
            continue
        lst = _as_list(list_t[c], n)
        for k in range(N):
            o = _owner(lst, now_ns + k * dt_ns)
            if k == 0:
                d_p[L.p_nom[c]:L.p_nom[c] + 3] = d_list[c, o]
                d_p[L.p_cur[c]:L.p_cur[c] + 3] = d_list[c, o]
            d_p[L.p_nom[c] + 3 * (k + 1):L.p_nom[c] + 3 * (k + 1) + 3] = d_list[c, o]
        if 0 <= int(land[c]) <= N:
            nxs[c] = _next(lst, now_ns)
    return d_p, d_list, nxs


def tick_jvp(cfg, tape, now, d_state, d_prev_list, MS=None, theta=None, gravity=GRAVITY):
    """One tick of one problem forwards: (d state, d previous list positions) -> (d state', d list positions out), through merge -> sample -> setState ->
    solve (sens_ref's JVP) -> adjust -> plant.  MS: the tick's ModelSens (built when None)."""
    L = cm.Layout(cfg.N)
    x, p, lam = (np.asarray(tape[k], np.float64) for k in ("X", "P", "lam_g"))
    th = sens_model_ref.theta_of(cfg) if theta is None else np.asarray(theta, np.float64)
    if MS is None:
        MS = sens_model_ref.ModelSens(cfg, x, p, lam, theta=th)
    d_p, d_list, nxs = list_position_jvp(L, cfg.sampling_time, now, tape["list_t"], tape["list_n"], tape["land"], d_prev_list, tape.get("prev"))
    d_p[L.p_com0:L.p_com0 + 9] = d_state
    dx = MS.S.jvp(d_p)
    for c in range(2):
        if nxs[c] >= 0:
            k = int(tape["land"][c])
            d_list[c, nxs[c]] = dx[L.pos[c] + 3 * k:L.pos[c] + 3 * k + 3]
    corners = th[10:34].astype(np.float32).astype(np.float64)
    d_out = plant_jvp(L, corners, x, p, tape["state"], tape["step"], tape["substeps"], d_state, d_x=dx, gravity=gravity)
    return d_out, d_list
