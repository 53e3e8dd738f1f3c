"""Float64 restatement of the plant-model mismatch FORWARDS (include/cmpc.h, "the mismatch FORWARDS"; DESIGN.md 7f, "Mismatch, forwards"), one problem and
one direction column at a time, built on what exists (imported, not changed):

  * plant_jvp -- tests/mismatch_ref.plant_jacobian (76 columns: the 69 of the plain plant, the force columns with respect to the MPC's forces, then the
    hidden wrench and the gain) applied to a direction, plus the rotation columns of tests/rollout_rot_ref taken at the applied forces;
  * tick_jvp -- tests/rollout_jvp_ref.tick_jvp with that plant, the noise direction added to the com0 / dcom0 / h0 rows of the p direction the SOLVE is
    given and to nothing else (it goes in as that function's extra p direction: the plant reads none of those rows);
  * forward_sweep chains ticks, first tick first; the transpose of tests/mismatch_ref.reverse_sweep.

The solve's p part is applied COLUMN BY COLUMN, dx = sum_j dp_j S.jvp(e_j) over the covered entries of p (ColumnSens): sens_ref.Sens.rhs forms its right-hand
side as a difference of two evaluations, at p + dp and at p, whose rounding is not linear in dp, while Sens.vjp contracts with rhs(e_j) entry by entry.  With
the same unit columns on both sides the restated JVP is the restated VJP's transpose to the rounding of the solves alone (on the landing tick of
tests/test_mismatch_jvp_cpu.py: 3.9e-13 of the larger side, against 1.0e-12 with rhs(dp) in one piece).

Test infrastructure: no GPU.  tests/test_mismatch_jvp_cpu.py holds it to mismatch_ref's adjoints and to central differences of mismatch_ref.plant_step;
tests/test_gpu_mismatch_jvp.py holds the device kernels to it."""
import numpy as np

import cmpc_amd as cm
from tests import mismatch_ref as mr
from tests import rollout_adjoint_ref as ra
from tests import rollout_jvp_ref as rjr
from tests import rollout_rot_ref as rrr
from tests import sens_model_ref, sens_ref
from tests import sens_rot_ref as srr

GRAVITY = ra.GRAVITY


class _ColumnP:
    """sens_ref.Sens with jvp applied column by column: d x / d p_j for every covered j from ONE multi-column solve, kept on the Sens object"""
    def __init__(self, S):
        self._S = S

    def __getattr__(self, name):
        return getattr(self._S, name)

    def jvp(self, dp):
        S = self._S
        if getattr(S, "_p_columns", None) is None:
            idx = np.nonzero(sens_ref.covered_mask(S.N))[0]
            unit = np.eye(S.L.np)
            Y = S._solve(-np.stack([S.rhs(unit[j]) for j in idx], 1))
            J = np.zeros((S.L.nx, idx.size))
            J[S.keep] = Y[:S.nk]
            if S.n is not None:
                J = J - np.outer(S.n, S.n @ J)
            S._p_columns = (idx, J)
        idx, J = S._p_columns
        return J @ np.asarray(dp, np.float64)[idx]


class ColumnSens:
    """a tick's sens_rot_ref.RotSens (built on first use when not given: a flagged tick never builds it) whose p part is _ColumnP"""
    def __init__(self, cfg, x, p, lam, theta, RS=None):
        self._args, self._RS = (cfg, x, p, lam, theta), RS

    def _rs(self):
        if self._RS is None:
            cfg, x, p, lam, theta = self._args
            self._RS = srr.RotSens(cfg, x, p, lam, theta=theta)
        return self._RS

    S = property(lambda self: _ColumnP(self._rs().S))
    MS = property(lambda self: self._rs().MS)

    def jvp(self, rot):
        return self._rs().jvp(rot)


def plant_direction(L, d_state=None, d_x=None, d_p=None, d_model=None, d_hidden=None, d_gain=0.0):
    """the 76 entries of a direction in the column order of mismatch_ref.plant_jacobian (None = zero)"""
    xi, pi = ra.plant_columns(L)
    d = np.zeros(mr.NCOL)
    if d_state is not None:
        d[0:9] = d_state
    if d_x is not None:
        d[ra.C_POS:ra.C_FEXT] = np.asarray(d_x, np.float64)[xi]
    if d_p is not None:
        d[ra.C_FEXT:ra.C_CORN] = np.asarray(d_p, np.float64)[pi]
    if d_model is not None:
        d[ra.C_CORN:ra.NCOL] = np.asarray(d_model, np.float64)[10:34]
    if d_hidden is not None:
        d[mr.C_HID:mr.C_HID + 6] = d_hidden
    d[mr.C_GAIN] = 0.0 if d_gain is None else float(d_gain)
    return d


def plant_jvp(L, corners, x, p, state, step, substeps, d_state=None, d_x=None, d_p=None, d_model=None, d_rot0=None, hidden=None, gain=1.0, d_hidden=None,
              d_gain=0.0, gravity=GRAVITY):
    """d state'[9] of the mismatched plant along (d_state[9], d_x[n_x], d_p[n_p], d_model[34], d_rot0[2][3], d_hidden[6], d_gain); None = zero"""
    J = mr.plant_jacobian(L, corners, x, p, state, step, substeps, hidden, gain, gravity)
    out = J @ plant_direction(L, d_state, d_x, d_p, d_model, d_hidden, d_gain)
    if d_rot0 is not None:     # (the contact points turn under the forces the plant APPLIES)
        x2, p2 = mr.applied_inputs(L, x, p, hidden, gain)
        out = out + rrr.plant_rot_columns(L, corners, x2, p2, state, step, substeps) @ np.asarray(d_rot0, np.float64).reshape(6)
    return out


def tick_jvp(cfg, tape, now, d_state=None, d_prev_list=None, d_prev_list_rot=None, d_plan=None, d_plan_rot=None, d_wrench=None, d_model=None, d_p=None,
             d_hidden=None, d_noise=None, d_gain=0.0, theta=None, RS=None, gravity=GRAVITY):
    """rollout_jvp_ref.tick_jvp with the mismatched plant: tape as mismatch_ref.tick_vjp's (state: the TRUE state, P: what the solve saw, hidden[6] or None,
    gain, default 1); the further directions d_hidden[6], d_noise[9], d_gain (None = zero).  -> its dict; a flagged tick gives zeros."""
    L = cm.Layout(cfg.N)
    hidden, gain = tape.get("hidden"), float(tape.get("gain", 1.0))
    th = sens_model_ref.theta_of(cfg) if theta is None else np.asarray(theta, np.float64)
    RS = ColumnSens(cfg, *(np.asarray(tape[k], np.float64) for k in ("X", "P", "lam_g")), th, RS)
    extra = d_p
    if d_noise is not None:     # the solve's com0 / dcom0 / h0 rows only: the plant is handed d_state alone and reads no such row of the p direction
        extra = np.zeros(L.np) if d_p is None else np.array(d_p, np.float64)
        extra[L.p_com0:L.p_com0 + 9] += np.asarray(d_noise, np.float64)

    def plant(L_, corners, x, p, state, step, substeps, ds, d_x=None, d_p=None, d_model=None, d_rot0=None, gravity=GRAVITY):
        return plant_jvp(L_, corners, x, p, state, step, substeps, ds, d_x, d_p, d_model, d_rot0, hidden, gain, d_hidden, d_gain, gravity)
    saved = rrr.plant_jvp
    rrr.plant_jvp = plant
    try:
        return rjr.tick_jvp(cfg, tape, now, d_state, d_prev_list, d_prev_list_rot, d_plan, d_plan_rot, d_wrench, d_model, extra, theta, RS, gravity)
    finally:
        rrr.plant_jvp = saved


def forward_sweep(cfg, tapes, nows, d_state0=None, d_list0=None, d_plan=None, d_model=None, d_wrench=None, d_hidden=None, d_noise=None, d_gain=0.0,
                  theta=None):
    """The mismatched ticks of one problem forwards along one column: rollout_jvp_ref.forward_sweep's position groups plus d_hidden[T][6], d_noise[T][9]
    (row i: tick i's) and d_gain.  -> dict(states[T+1][9], list (the final lists'), X[T][n_x], status[T])."""
    T = len(tapes)
    ds, dl = (np.zeros(9) if d_state0 is None else np.asarray(d_state0, np.float64)), d_list0
    out = dict(states=[ds.copy()], X=[], status=[])
    for i in range(T):
        r = tick_jvp(cfg, tapes[i], nows[i], ds, dl, None, d_plan, None, None if d_wrench is None else d_wrench[i], d_model, None,
                     None if d_hidden is None else d_hidden[i], None if d_noise is None else d_noise[i], d_gain, theta)
        ds, dl = r["state"], r["list"]
        out["states"].append(ds.copy())
        out["X"].append(r["x"])
        out["status"].append(r["status"])
    out["states"], out["X"], out["list"] = np.array(out["states"]), np.array(out["X"]), dl
    return out
