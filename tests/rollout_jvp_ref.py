"""Float64 restatement of the roll-out tick FORWARDS in every input group (include/cmpc.h: cmpc_contacts_jvp_device, cmpc_plant_step_jvp_cols_device,
cmpc_rollout_tick_jvp_device; DESIGN.md 7d, "Forwards"), one problem and one direction column at a time, built on tests/rollout_adjoint_ref.py and
tests/rollout_rot_ref.py (imported, not changed): their index maps, plant Jacobians and solution sensitivities, applied forwards.

  * lists: list_jvp -- merge -> sample (phase bit 1) and the step adjustment (phase bit 2) along directions of the previous list's and the planner's
    positions and orientations; the transpose of rar.list_position_vjp plus rrr.list_orientation_vjp.
  * tick: tick_jvp -- list JVP -> the p direction assembled (list rows, state rows, wrench rows, the caller's extra p direction) -> the solution JVP in p,
    model and rotation directions (the same three linear maps rrr.tick_vjp_rot transposes) -> adjust -> plant JVP; the transpose of rrr.tick_vjp_rot.
  * forward_sweep chains ticks, first tick first; the transpose of rrr.reverse_sweep.

A foot that was not sampled (land = -2, an empty list, n > M) passes nothing on, in positions as in orientations (rrr.list_maps).

Test infrastructure: no GPU.  tests/test_rollout_jvp_cpu.py holds it to the restated adjoints and to finite differences of the oracle roll-out;
tests/test_gpu_rollout_jvp.py holds the device kernels to it."""
import numpy as np

import cmpc_amd as cm
from tests import rollout_adjoint_ref as rar
from tests import rollout_rot_ref as rrr
from tests import sens_model_ref
from tests import sens_rot_ref as srr

GRAVITY = rar.GRAVITY


def _z(a, shape):
    return np.zeros(shape) if a is None else np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------------------- lists
def list_jvp(L, dt, now, list_t, list_n, land, plan=None, prev=None, ok=True, d_prev=None, d_prev_rot=None, d_plan=None, d_plan_rot=None, d_x=None,
             force_sample_time=False, phase=3, d_list=None):
    """One problem, one column.  list_t[2][M][2], list_n[2], land[2]; plan / prev = (t[2][M][2], n[2]) or None (prev None: first tick, d_prev / d_prev_rot
    are the directions of the list itself and the planner's are not read).  d_*[2][M][3] (None = zero), d_x[n_x] the solution's direction (phase bit 2).
    phase 2 alone: d_list = the phase-1 result, copied and updated.
    -> dict(list[2][M][3], list_rot[2][M][3], p[n_p] (nominalPos / currentPos rows), rot[2][N][3], nx[2] (the overwritten entry or -1), status)."""
    N = L.N
    list_t = np.asarray(list_t, np.float64)
    M = list_t.shape[1]
    out = dict(list=np.zeros((2, M, 3)) if d_list is None or (phase & 1) else np.array(d_list, np.float64), list_rot=np.zeros((2, M, 3)), p=np.zeros(L.np),
               rot=np.zeros((2, N, 3)), nx=[-1, -1], status=0 if ok else 5)
    if not ok:
        out["list"][:] = 0.0
        return out
    maps = rrr.list_maps(L, dt, now, list_t, list_n, land, plan, prev, force_sample_time)
    pos_of = dict(prev=_z(d_prev, (2, M, 3)), plan=_z(d_plan, (2, M, 3)))
    rot_of = dict(prev=_z(d_prev_rot, (2, M, 3)), plan=_z(d_plan_rot, (2, M, 3)))
    for c in range(2):
        mp = maps[c]
        if not mp["sampled"]:
            continue
        if phase & 1:
            for m, s in enumerate(mp["src"]):
                if s is not None:
                    out["list"][c, m] = pos_of[s[0]][c][s[1]]
                    out["list_rot"][c, m] = rot_of[s[0]][c][s[1]]
            for k, o in enumerate(mp["owner"]):
                if k == 0:
                    out["p"][L.p_nom[c]:L.p_nom[c] + 3] = out["list"][c, o]
                    out["p"][L.p_cur[c]:L.p_cur[c] + 3] = out["list"][c, o]
                out["p"][L.p_nom[c] + 3 * (k + 1):L.p_nom[c] + 3 * (k + 1) + 3] = out["list"][c, o]
                out["rot"][c, k] = out["list_rot"][c, o]
        if 0 <= int(land[c]) <= N:
            out["nx"][c] = rar._next(rar._as_list(list_t[c], mp["n"]), rar._ns(now))
        if (phase & 2) and out["nx"][c] >= 0:
            k = int(land[c])
            out["list"][c, out["nx"][c]] = 0.0 if d_x is None else np.asarray(d_x, np.float64)[L.pos[c] + 3 * k:L.pos[c] + 3 * k + 3]
    return out


# ---------------------------------------------------------------------------------------------------------------- tick
def tick_jvp(cfg, tape, now, d_state=None, d_prev_list=None, d_prev_list_rot=None, d_plan=None, d_plan_rot=None, d_wrench=None, d_model=None, d_p=None,
             theta=None, RS=None, gravity=GRAVITY):
    """One tick of one problem forwards along one column of all eight input groups (None = zero): d_state[9], d_prev_list / d_prev_list_rot / d_plan /
    d_plan_rot[2][M][3], d_wrench[N][6], d_model[34], d_p[n_p] (added to the assembled p direction; its R and Gamma entries are read as zero).  tape as
    rar.tick_vjp's.  -> dict(state[9], list[2][M][3], list_rot[2][M][3], x[n_x], rot[2][N][3], p[n_p] (the assembled direction), status); a flagged tick
    gives zeros.  RS: the tick's RotSens (built when None)."""
    N = cfg.N
    L = cm.Layout(N)
    x, p, lam = (np.asarray(tape[k], np.float64) for k in ("X", "P", "lam_g"))
    M = np.asarray(tape["list_t"]).shape[1]
    zero = dict(state=np.zeros(9), list=np.zeros((2, M, 3)), list_rot=np.zeros((2, M, 3)), x=np.zeros(L.nx), rot=np.zeros((2, N, 3)), p=np.zeros(L.np))
    if not tape.get("ok", True):
        return dict(zero, status=5)
    if not (np.isfinite(x).all() and np.isfinite(p).all() and np.isfinite(lam).all() and np.isfinite(np.asarray(tape["state"], np.float64)).all()):
        return dict(zero, status=2)
    if int(tape.get("status", 0)) != 0:
        return dict(zero, status=4)
    th = sens_model_ref.theta_of(cfg) if theta is None else np.asarray(theta, np.float64)
    if RS is None:
        RS = srr.RotSens(cfg, x, p, lam, theta=th)
    lst = rrr._lists_of(tape)
    d_state = _z(d_state, 9)
    fw = list_jvp(L, cfg.sampling_time, now, d_prev=d_prev_list, d_prev_rot=d_prev_list_rot, d_plan=d_plan, d_plan_rot=d_plan_rot, phase=1, **lst)
    dp = fw["p"].copy()
    dp[L.p_com0:L.p_com0 + 9] = d_state
    if d_wrench is not None:
        w = np.asarray(d_wrench, np.float64)
        dp[L.p_fext:L.p_fext + 3 * N] = w[:, :3].ravel()
        dp[L.p_text:L.p_text + 3 * N] = w[:, 3:].ravel()
    if d_p is not None:
        dp = dp + np.asarray(d_p, np.float64)
    # the three linear maps rrr.tick_vjp_rot transposes, each through its own solve: Sens (p), ModelSens (theta), RotSens (omega)
    dx = RS.S.jvp(dp)
    if d_model is not None and np.any(d_model):
        dx = dx + RS.MS.jvp(np.asarray(d_model, np.float64))
    if fw["rot"].any():
        dx = dx + RS.jvp(fw["rot"])
    d_list = list_jvp(L, cfg.sampling_time, now, d_x=dx, phase=2, d_list=fw["list"], **lst)["list"]
    corners = th[10:34].astype(np.float32).astype(np.float64)     # (the record the kernels read is float32)
    d_out = rrr.plant_jvp(L, corners, x, p, tape["state"], tape["step"], tape["substeps"], d_state, d_x=dx, d_p=dp, d_model=d_model, d_rot0=fw["rot"][:, 0],
                          gravity=gravity)
    return dict(state=d_out, list=d_list, list_rot=fw["list_rot"], x=dx, rot=fw["rot"], p=dp, status=0)


def forward_sweep(cfg, tapes, nows, d_state0=None, d_list0=None, d_list_rot0=None, d_plan=None, d_plan_rot=None, d_push=None, d_model=None, d_wrench=None,
                  theta=None, push_knots=None, sens=None):
    """The ticks of one problem forwards along one column: d_state0[9], d_list0 / d_list_rot0[2][M][3] (the first tick's lists), d_plan / d_plan_rot
    (the planner's contacts, read by every merge), d_push[3] (enters the fExt rows of the push_knots[i] first knots of tick i), d_model[34],
    d_wrench[T][N][6]; sens: the ticks' RotSens, when the caller sweeps the same tapes more than once.  -> dict(states[T+1][9], list, list_rot (the final lists'), X[T][n_x], status[T])."""
    T, N = len(tapes), cfg.N
    ds, dl, dlr = _z(d_state0, 9), d_list0, d_list_rot0
    out = dict(states=[ds.copy()], X=[], status=[])
    for i in range(T):
        w = None if d_wrench is None else np.array(d_wrench[i], np.float64)
        if d_push is not None and push_knots is not None and push_knots[i] > 0:
            w = np.zeros((N, 6)) if w is None else w
            w[:push_knots[i], :3] += np.asarray(d_push, np.float64)
        r = tick_jvp(cfg, tapes[i], nows[i], ds, dl, dlr, d_plan, d_plan_rot, w, d_model, None, theta, None if sens is None else sens[i])
        ds, dl, dlr = r["state"], r["list"], r["list_rot"]
        out["states"].append(ds.copy())
        out["X"].append(r["x"])
        out["status"].append(r["status"])
    out["states"], out["X"] = np.array(out["states"]), np.array(out["X"])
    out["list"], out["list_rot"] = dl, dlr
    return out
