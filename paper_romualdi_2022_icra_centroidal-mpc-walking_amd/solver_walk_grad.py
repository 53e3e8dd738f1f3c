"""The derivative layer of BatchSolver: the methods that call the entries of csrc/cmpc_api_walk_grad.hip -- the roll-out tick and the device walk in
reverse and forwards, the column plant JVPs, the list path forwards, the three gates.  A base class without state: the handle, _launch, _opt, _dev and
_list_tape are BatchSolver's (solver.py)."""
from __future__ import annotations

import ctypes as C

from . import _args, _capi
from ._args import ptr


class WalkGradCalls:
    # ---- the roll-out tick in reverse (include/cmpc.h, "the roll-out tick in reverse") ----
    def _tick_tape(self, tape):
        """(cmpc_tick_tape, M, device) of the tape dict of one tick (rollout_tick_vjp_device), its tensors checked"""
        import torch
        L, B = self.layout, self.batch
        lt = tape["list_t"]
        M = lt.shape[2]
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        tt, tn = (B, 2, M, 2), (B, 2)
        ct = _capi.CmpcTickTape(self._opt(tape["X"], f32, (B, L.nx), "X"), self._opt(tape["P"], f32, (B, L.np), "P"), self._opt(tape["lam_g"], f32, (B, L.ng), "lam_g"),
                                self._opt(tape["state"], f32, (B, 9), "state"), self._opt(tape["info"], f32, (B, _capi.INFO), "info"),
                                self._opt(tape.get("ok"), i32, (B,), "ok"), self._opt(tape["land"], i32, tn, "land"),
                                self._opt(tape.get("plan_t"), f64, tt, "plan_t"), self._opt(tape.get("plan_n"), i32, tn, "plan_n"),
                                self._opt(tape.get("prev_t"), f64, tt, "prev_t"), self._opt(tape.get("prev_n"), i32, tn, "prev_n"),
                                self._opt(lt, f64, tt, "list_t"), self._opt(tape["list_n"], i32, tn, "list_n"),
                                float(tape["step"]), int(tape["substeps"]), 1 if tape.get("force_sample_time") else 0)
        return ct, M, lt.device

    def rollout_tick_vjp_device(self, now, tape, dGradStateOut, dGradListOut=None, dGradX=None, dGradPlan=None, dGradModel=None, wrench=True, grad_p=False,
                                dGradListRotOut=None, rot=False, dGradPlanRot=None, mismatch=False, hidden_wrench=None, force_gain=None, dGradGain=None):
        """cmpc_rollout_tick_vjp_device: one tick in reverse.  tape: dict(X, P, lam_g, state, info, ok (or None), land, plan_t, plan_n, prev_t, prev_n
        (both None on the first tick), list_t, list_n, step, substeps, force_sample_time) of CUDA tensors as the forward tick left them.
        dGradStateOut[B,9] float64, dGradListOut[B,2,M,3] float64 or None, dGradX[B,n_x] float32 or None; dGradPlan / dGradModel: float64 tensors added to
        in place, or None.  Returns dict(state[B,9], prev_list[B,2,M,3] float64, wrench[B,N,6] float32 or None, p[B,n_p] float32 or None,
        sens[B,CMPC_SENS] float32 with the tick's status in word 0).
        rot=True (cmpc_rollout_tick_vjp_rot_device): the contacts' orientations are carried along, in the body-frame tangent of their quaternions --
        dGradListRotOut[B,2,M,3] float64 or None, dGradPlanRot[B,2,M,3] float64 added to in place or None; the dict also holds prev_list_rot[B,2,M,3] and
        rot[B,2,N,3] float64 (the tick's per-stage dl/domega: the solve's, plus the plant's on stage 0), every other entry bit-equal to rot=False but
        sens, which is the rotation VJP's.
        mismatch=True (cmpc_rollout_tick_vjp_mismatch_device; with or without rot): the tick ran under hidden_wrench[B,6] / force_gain[B] float32 (its own
        rows; None: not applied) and tape["state"] is the TRUE state; the dict also holds hidden[B,6] float64 and noise[B,9] float32, and dGradGain[B]
        float64 (or None) is added to in place."""
        import torch
        L, B, N = self.layout, self.batch, self.cfg.N
        ct, M, dev = self._tick_tape(tape)
        g3 = (B, 2, M, 3)
        f32, f64 = torch.float32, torch.float64
        out = dict(state=torch.empty((B, 9), dtype=f64, device=dev), prev_list=torch.empty(g3, dtype=f64, device=dev),
                   wrench=torch.empty((B, N, 6), dtype=f32, device=dev) if wrench else None,
                   p=torch.empty((B, L.np), dtype=f32, device=dev) if grad_p else None, sens=torch.empty((B, _capi.SENS), dtype=f32, device=dev))
        args = (self._opt(dGradStateOut, f64, (B, 9), "dGradStateOut"), self._opt(dGradListOut, f64, g3, "dGradListOut"),
                self._opt(dGradX, f32, (B, L.nx), "dGradX"), out["state"].data_ptr(), out["prev_list"].data_ptr(),
                out["wrench"].data_ptr() if wrench else None, self._opt(dGradPlan, f64, g3, "dGradPlan"),
                self._opt(dGradModel, f64, (B, _capi.MODEL_DOUBLES), "dGradModel"), out["p"].data_ptr() if grad_p else None, out["sens"].data_ptr())
        margs = None
        if mismatch:
            out["hidden"] = torch.empty((B, 6), dtype=f64, device=dev)
            out["noise"] = torch.empty((B, 9), dtype=f32, device=dev)
            margs = (self._opt(hidden_wrench, f32, (B, 6), "hidden_wrench"), self._opt(force_gain, f32, (B,), "force_gain"), out["hidden"].data_ptr(),
                     out["noise"].data_ptr(), self._opt(dGradGain, f64, (B,), "dGradGain"))
        elif not (hidden_wrench is None and force_gain is None and dGradGain is None):
            raise AssertionError("mismatch arguments need mismatch=True")
        if not rot:
            if not (dGradListRotOut is None and dGradPlanRot is None):
                raise AssertionError("orientation gradients need rot=True")
            if mismatch:
                self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_mismatch_device(self._h, M, float(now), ct, *args, None, None, None, None, *margs, st))
            else:
                self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_device(self._h, M, float(now), ct, *args, st))
            return out
        out["prev_list_rot"] = torch.empty(g3, dtype=f64, device=dev)
        out["rot"] = torch.empty((B, 2, N, 3), dtype=f64, device=dev)
        rargs = (self._opt(dGradListRotOut, f64, g3, "dGradListRotOut"), out["prev_list_rot"].data_ptr(), self._opt(dGradPlanRot, f64, g3, "dGradPlanRot"),
                 out["rot"].data_ptr())
        if mismatch:
            self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_mismatch_device(self._h, M, float(now), ct, *args, *rargs, *margs, st))
        else:
            self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_rot_device(self._h, M, float(now), ct, *args, *rargs, st))
        return out

    # ---- the roll-out tick forwards, in k directions (include/cmpc.h, "the roll-out tick FORWARDS") ----
    def plant_step_jvp_cols_device(self, dX, dP, dState, dDirState, dDirX=None, dDirP=None, dDirModel=None, dDirRot0=None, step=0.01, substeps=6, out=None):
        """cmpc_plant_step_jvp_cols_device: plant_step_jvp_device with k columns per problem -- dDirState[B, k, 9] float64, dDirX[B, k, n_x] /
        dDirP[B, k, n_p] float32, dDirModel[B, k, 34] and dDirRot0[B, k, 2, 3] float64 (None: zero) -> d state'[B, k, 9] float64; column j is bit-equal to
        plant_step_jvp_device on column j."""
        import torch
        L, B = self.layout, self.batch
        if dDirState.dim() != 3:
            raise AssertionError("dDirState: expected [B, k, 9]")
        k = int(dDirState.shape[1])
        out = _args.out(out, torch.float64, (B, k, 9), "out", dX.device)
        args = (self._opt(dDirState, torch.float64, (B, k, 9), "dDirState"), self._opt(dDirX, torch.float32, (B, k, L.nx), "dDirX"),
                self._opt(dDirP, torch.float32, (B, k, L.np), "dDirP"), self._opt(dDirModel, torch.float64, (B, k, _capi.MODEL_DOUBLES), "dDirModel"),
                self._opt(dDirRot0, torch.float64, (B, k, 2, 3), "dDirRot0"), out.data_ptr())
        self._launch(dX.device, lambda st: self._lib.cmpc_plant_step_jvp_cols_device(self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step),
                                                                                     int(substeps), k, *args, st))
        return out

    def plant_step_jvp_mismatch_cols_device(self, dX, dP, dState, dDirState, dDirX=None, dDirP=None, dDirModel=None, dDirRot0=None, hidden_wrench=None,
                                            force_gain=None, dDirHidden=None, dDirGain=None, step=0.01, substeps=6, out=None):
        """cmpc_plant_step_jvp_mismatch_cols_device: plant_step_jvp_cols_device at the mismatched plant (hidden_wrench[B, 6], force_gain[B] float32 or
        None) with the directions dDirHidden[B, k, 6] and dDirGain[B, k] float64 (None: zero) -> d state'[B, k, 9] float64.  All four None: the call
        above, bit for bit; column j is bit-equal to a k = 1 call on column j."""
        import torch
        L, B = self.layout, self.batch
        if dDirState.dim() != 3:
            raise AssertionError("dDirState: expected [B, k, 9]")
        k = int(dDirState.shape[1])
        f32, f64 = torch.float32, torch.float64
        out = _args.out(out, f64, (B, k, 9), "out", dX.device)
        args = (self._opt(dDirState, f64, (B, k, 9), "dDirState"), self._opt(dDirX, f32, (B, k, L.nx), "dDirX"), self._opt(dDirP, f32, (B, k, L.np), "dDirP"),
                self._opt(dDirModel, f64, (B, k, _capi.MODEL_DOUBLES), "dDirModel"), self._opt(dDirRot0, f64, (B, k, 2, 3), "dDirRot0"),
                self._opt(hidden_wrench, f32, (B, 6), "hidden_wrench"), self._opt(force_gain, f32, (B,), "force_gain"),
                self._opt(dDirHidden, f64, (B, k, 6), "dDirHidden"), self._opt(dDirGain, f64, (B, k), "dDirGain"), out.data_ptr())
        self._launch(dX.device, lambda st: self._lib.cmpc_plant_step_jvp_mismatch_cols_device(
            self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step), int(substeps), k, *args, st))
        return out

    def contacts_jvp_device(self, now, list_t, list_n, land, k, plan=None, prev=None, ok=None, dDirPrevList=None, dDirPrevListRot=None, dDirPlan=None,
                            dDirPlanRot=None, dDirX=None, phase=3, force_sample_time=False, out=None, out_rot=None, dDirP=None, rot=True):
        """The list path of one tick forwards (cmpc_contacts_jvp_device), the transpose of contacts_position_vjp_device + contacts_orientation_vjp_device
        with their tape arguments: directions [B, k, 2, M, 3] float64 of the previous list's and the planner's positions and orientations (None: zero),
        dDirX[B, k, n_x] float32 (phase bit 2: the landing entry takes the solution's direction).  phase 1: merge + sample; 2: adjust (out / out_rot
        are then the phase-1 results, updated in place); 3: both.  -> dict(list, list_rot [B, k, 2, M, 3] float64, p[B, k, n_p] float32 (dDirP or a
        zero tensor: only the nominalPos / currentPos rows are written), rot[B, k, 2, N, 3] float64 (rot=False: None), status[B] int32)."""
        import torch
        L, B, M, dev = self.layout, self.batch, list_t.shape[2], list_t.device
        g3 = (B, k, 2, M, 3)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        tape = self._list_tape(M, list_t, list_n, land, plan, prev, ok)
        res = dict(list=out if out is not None else torch.zeros(g3, dtype=f64, device=dev),
                   list_rot=out_rot if out_rot is not None else torch.zeros(g3, dtype=f64, device=dev), p=None, rot=None,
                   status=torch.empty((B,), dtype=i32, device=dev))
        if phase & 1:
            res["p"] = dDirP if dDirP is not None else torch.zeros((B, k, L.np), dtype=f32, device=dev)
            res["rot"] = torch.empty((B, k, 2, L.N, 3), dtype=f64, device=dev) if rot else None
        args = (self._opt(dDirPrevList, f64, g3, "dDirPrevList"), self._opt(dDirPrevListRot, f64, g3, "dDirPrevListRot"),
                self._opt(dDirPlan, f64, g3, "dDirPlan"), self._opt(dDirPlanRot, f64, g3, "dDirPlanRot"), self._opt(dDirX, f32, (B, k, L.nx), "dDirX"),
                self._opt(res["list"], f64, g3, "out"), self._opt(res["list_rot"], f64, g3, "out_rot"), self._opt(res["p"], f32, (B, k, L.np), "dDirP"),
                self._opt(res["rot"], f64, (B, k, 2, L.N, 3), "rot"), res["status"].data_ptr())
        self._launch(dev, lambda st: self._lib.cmpc_contacts_jvp_device(
            self._h, M, float(now), int(phase), 1 if force_sample_time else 0, int(k), *tape, *args, st))
        return res

    def rollout_tick_jvp_device(self, now, tape, k, dDirState=None, dDirPrevList=None, dDirPrevListRot=None, dDirPlan=None, dDirPlanRot=None, dDirWrench=None,
                                dDirModel=None, dDirP=None, x=False, rot=False, p_full=False, out_state=None):
        """cmpc_rollout_tick_jvp_device: one tick forwards in k directions (arguments and the returned dict: _rollout_tick_jvp)."""
        return self._rollout_tick_jvp(now, tape, k, dDirState, dDirPrevList, dDirPrevListRot, dDirPlan, dDirPlanRot, dDirWrench, dDirModel, dDirP, x, rot,
                                      p_full, out_state, None)

    def rollout_tick_jvp_mismatch_device(self, now, tape, k, hidden_wrench=None, force_gain=None, dDirHidden=None, dDirNoise=None, dDirGain=None,
                                         dDirState=None, dDirPrevList=None, dDirPrevListRot=None, dDirPlan=None, dDirPlanRot=None, dDirWrench=None,
                                         dDirModel=None, dDirP=None, x=False, rot=False, p_full=False, out_state=None):
        """cmpc_rollout_tick_jvp_mismatch_device: rollout_tick_jvp_device on a tick that ran under a mismatch -- hidden_wrench[B, 6] / force_gain[B]
        float32 are the tick's own rows (None: not applied), dDirHidden[B, k, 6] / dDirGain[B, k] float64 and dDirNoise[B, k, 9] float32 the mismatch
        directions (None: zero).  The noise direction enters the solve only.  All five None: rollout_tick_jvp_device, bit for bit."""
        return self._rollout_tick_jvp(now, tape, k, dDirState, dDirPrevList, dDirPrevListRot, dDirPlan, dDirPlanRot, dDirWrench, dDirModel, dDirP, x, rot,
                                      p_full, out_state, (hidden_wrench, force_gain, dDirHidden, dDirNoise, dDirGain))

    def _rollout_tick_jvp(self, now, tape, k, dDirState, dDirPrevList, dDirPrevListRot, dDirPlan, dDirPlanRot, dDirWrench, dDirModel, dDirP, x, rot, p_full,
                          out_state, mm):
        """cmpc_rollout_tick_jvp_device: one tick forwards in k directions, on the tape of rollout_tick_vjp_device.  Directions (each None: zero), with the
        column axis behind the batch axis: dDirState[B,k,9], dDirPrevList / dDirPrevListRot / dDirPlan / dDirPlanRot[B,k,2,M,3], dDirModel[B,k,34] float64;
        dDirWrench[B,k,N,6], dDirP[B,k,n_p] float32.  Returns dict(state[B,k,9], list[B,k,2,M,3], list_rot[B,k,2,M,3] float64, x[B,k,n_x] float32 (x=True),
        rot[B,k,2,N,3] float64 (rot=True), p[B,k,n_p] float32 (p_full=True: the assembled p direction), sens[B,CMPC_SENS] float32 with the tick's status
        in word 0) -- the keys of rollout_tick_vjp_device's dict, each holding the direction of what that one holds the gradient of."""
        import torch
        from ._capi import CmpcTickDirs, CmpcTickDirsOut
        L, B, N = self.layout, self.batch, self.cfg.N
        ct, M, dev = self._tick_tape(tape)
        k = int(k)
        g3 = (B, k, 2, M, 3)
        f32, f64 = torch.float32, torch.float64
        din = CmpcTickDirs(self._opt(dDirState, f64, (B, k, 9), "dDirState"), self._opt(dDirPrevList, f64, g3, "dDirPrevList"),
                           self._opt(dDirPrevListRot, f64, g3, "dDirPrevListRot"), self._opt(dDirPlan, f64, g3, "dDirPlan"),
                           self._opt(dDirPlanRot, f64, g3, "dDirPlanRot"), self._opt(dDirWrench, f32, (B, k, N, 6), "dDirWrench"),
                           self._opt(dDirModel, f64, (B, k, _capi.MODEL_DOUBLES), "dDirModel"), self._opt(dDirP, f32, (B, k, L.np), "dDirP"))
        out = dict(state=out_state if out_state is not None else torch.empty((B, k, 9), dtype=f64, device=dev), list=torch.empty(g3, dtype=f64, device=dev),
                   list_rot=torch.empty(g3, dtype=f64, device=dev), x=torch.empty((B, k, L.nx), dtype=f32, device=dev) if x else None,
                   rot=torch.empty((B, k, 2, N, 3), dtype=f64, device=dev) if rot else None,
                   p=torch.empty((B, k, L.np), dtype=f32, device=dev) if p_full else None, sens=torch.empty((B, _capi.SENS), dtype=f32, device=dev))
        dout = CmpcTickDirsOut(self._opt(out["state"], f64, (B, k, 9), "out_state"), out["list"].data_ptr(), out["list_rot"].data_ptr(),
                               out["x"].data_ptr() if x else None, out["rot"].data_ptr() if rot else None, out["p"].data_ptr() if p_full else None)
        if mm is not None:   # (the mismatch entry; all of it None: the library makes the plain call)
            hw, fg, dh, dn, dg = mm
            md = None
            if dh is not None or dn is not None or dg is not None:
                md = C.byref(_capi.CmpcTickDirsMismatch(self._opt(dh, f64, (B, k, 6), "dDirHidden"), self._opt(dn, f32, (B, k, 9), "dDirNoise"),
                                                        self._opt(dg, f64, (B, k), "dDirGain")))
            ph, pg = self._opt(hw, f32, (B, 6), "hidden_wrench"), self._opt(fg, f32, (B,), "force_gain")
            self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_jvp_mismatch_device(self._h, M, float(now), ct, k, din, dout, out["sens"].data_ptr(),
                                                                                         ph, pg, md, st))
            return out
        self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_jvp_device(self._h, M, float(now), ct, k, din, dout, out["sens"].data_ptr(), st))
        return out

    def rollout_walk_vjp_device(self, tick0, ticks, tape, row0, end_tick, grad_states, carry_state, carry_list, status, grad_X=None, wrench=None, grad_p=None,
                                dGradPlan=None, dGradModel=None, carry_list_rot=None, dGradPlanRot=None, grad_rot=None, removed=None, mismatch=None,
                                grad_hidden=None, grad_noise=None, grad_gain=None):
        """cmpc_rollout_walk_vjp_device: rows row0 .. row0 + ticks - 1 of tape (walk_tape) in reverse in ONE call.  grad_states[rows + 1, B, 9] float64 and
        grad_X[rows, B, n_x] float32 (or None) are the seeds; carry_state[B, 9] / carry_list[B, 2, M, 3] float64 go in as the carry entering the last row
        and come back as the carry leaving the first; wrench[rows, B, N, 6] / grad_p[rows, B, n_p] float32 (or None) and status[rows, B] int32 are written
        row by row; dGradPlan[B, 2, M, 3] / dGradModel[B, 34] float64 are added to in place.  end_tick: int32 [B] (a walk record's) or None.
        carry_list_rot[B, 2, M, 3] float64 given: cmpc_rollout_walk_vjp_rot_device, the contacts' orientations carried along -- it is the third carry;
        dGradPlanRot[B, 2, M, 3] float64 (or None) is added to in place, grad_rot[rows, B, 2, N, 3] float64 and removed[rows, B] float32 (or None) are
        written row by row.  Without it the three other arguments must be None and the call is the one it always was.
        mismatch (plant_mismatch(...)) given: cmpc_rollout_walk_vjp_mismatch_device, with or without carry_list_rot -- the walk ran under it; grad_hidden
        [rows, B, 6] float64 and grad_noise[rows, B, 9] float32 are written row by row, grad_gain[B] float64 is added to in place (each may be None)."""
        import torch
        R = int(tape["rows"])
        whole = lambda t, dtype, tail, name, extra=0: self._opt(t, dtype, (R + extra,) + tail, name)
        self._rollout_walk_vjp(whole, int(tick0), int(ticks), tape, int(row0), end_tick, grad_states,
                               whole(grad_X, torch.float32, (self.batch, self.layout.nx), "grad_X"), carry_state, carry_list, status, wrench, grad_p, dGradPlan,
                               dGradModel, carry_list_rot, dGradPlanRot, grad_rot, removed, mismatch, grad_hidden, grad_noise, grad_gain)

    def rollout_walk_vjp_rows_device(self, tick0, ticks, tape, row0, end_tick, grad_states, carry_state, carry_list, status, grad_X=None, wrench=None,
                                     dGradPlan=None, dGradModel=None, carry_list_rot=None, dGradPlanRot=None, grad_rot=None, removed=None, grad_X_rows=None,
                                     mismatch=None, grad_hidden=None, grad_noise=None, grad_gain=None):
        """rollout_walk_vjp_device on a SEGMENT tape (a few rows, re-used) with WHOLE-WALK arrays: grad_states[T + 1, B, 9], grad_X / wrench / grad_rot
        [T, B, ..] and status / removed [T, B] are indexed by the tick number, the tape by row0 + i for tick tick0 + i.  Each array goes to the library
        as the leading-axis view that starts tick0 - row0 rows in, so that tape row and array row coincide; the call reads and writes rows tick0 ..
        tick0 + ticks - 1 of them (and no other), exactly as rollout_walk_vjp_device does on a whole-walk tape.  The carries and the += outputs as
        there.  grad_X_rows[rows, B, n_x] float32 (instead of grad_X): the solutions' seeds of this segment alone, indexed like the tape.
        mismatch (plant_mismatch(...)) given: cmpc_rollout_walk_vjp_mismatch_device -- the segment ran under it; grad_hidden[T, B, 6] float64 and
        grad_noise[T, B, 9] float32 are whole-walk arrays written at the segment's rows, grad_gain[B] float64 is added to in place (each may be None)."""
        import torch
        tick0, ticks, row0 = int(tick0), int(ticks), int(row0)
        shift = tick0 - row0
        if not (shift >= 0 and ticks >= 1 and 0 <= row0 and row0 + ticks <= int(tape["rows"])):
            raise AssertionError("the segment must lie inside its tape")

        def view(t, dtype, tail, name, extra=0):
            if t is None:
                return None
            msg = f"{name}: expected {dtype} [>= {tick0 + ticks + extra}, {tuple(tail)}]"
            p = ptr(t, dtype, (None,) + tuple(tail), name, msg=msg)
            if t.shape[0] < tick0 + ticks + extra:
                raise AssertionError(msg)
            return p + shift * t.stride(0) * t.element_size()
        if grad_X is not None and grad_X_rows is not None:
            raise AssertionError("grad_X or grad_X_rows, not both")
        tail = (self.batch, self.layout.nx)
        gx = view(grad_X, torch.float32, tail, "grad_X") if grad_X_rows is None else self._opt(grad_X_rows, torch.float32, (int(tape["rows"]),) + tail, "grad_X_rows")
        self._rollout_walk_vjp(view, tick0, ticks, tape, row0, end_tick, grad_states, gx, carry_state, carry_list, status, wrench, None, dGradPlan, dGradModel,
                               carry_list_rot, dGradPlanRot, grad_rot, removed, mismatch, grad_hidden, grad_noise, grad_gain)

    def _rollout_walk_vjp(self, arr, tick0, ticks, tape, row0, end_tick, grad_states, gx, carry_state, carry_list, status, wrench, grad_p, dGradPlan, dGradModel,
                          carry_list_rot, dGradPlanRot, grad_rot, removed, mismatch, grad_hidden, grad_noise, grad_gain):
        """The one body of rollout_walk_vjp_device and rollout_walk_vjp_rows_device.  arr(tensor, dtype, tail, name, extra=0): the pointer of an array
        with one row per tick [rows + extra, *tail] as the public method indexes it (None -> NULL); gx: the pointer of the solutions' seeds.  One
        dispatch over plain / rot / mismatch, each its own C symbol."""
        import torch
        L, B, N, M = self.layout, self.batch, self.cfg.N, int(tape["max_contacts"])
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        g3 = (B, 2, M, 3)
        g = _capi.CmpcWalkGrads(arr(grad_states, f64, (B, 9), "grad_states", 1), gx, self._opt(carry_state, f64, (B, 9), "carry_state"),
                                self._opt(carry_list, f64, g3, "carry_list"), arr(wrench, f32, (B, N, 6), "wrench"), arr(grad_p, f32, (B, L.np), "grad_p"),
                                self._opt(dGradPlan, f64, g3, "dGradPlan"), self._opt(dGradModel, f64, (B, _capi.MODEL_DOUBLES), "dGradModel"),
                                arr(status, i32, (B,), "status"))
        e = self._opt(end_tick, i32, (B,), "end_tick")
        if mismatch is None and not (grad_hidden is None and grad_noise is None and grad_gain is None):
            raise AssertionError("mismatch gradients need mismatch")
        if carry_list_rot is None and not (dGradPlanRot is None and grad_rot is None and removed is None):
            raise AssertionError("orientation gradients need carry_list_rot")
        head = (self._h, M, tick0, ticks, tape["_c"], row0, e, g)
        if carry_list_rot is None and mismatch is None:
            return self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_device(*head, st))
        r = None
        if carry_list_rot is not None:
            r = _capi.CmpcWalkGradsRot(self._opt(carry_list_rot, f64, g3, "carry_list_rot"), self._opt(dGradPlanRot, f64, g3, "dGradPlanRot"),
                                       arr(grad_rot, f64, (B, 2, N, 3), "grad_rot"), arr(removed, f32, (B,), "removed"))
        if mismatch is None:
            return self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_rot_device(*head, r, st))
        mg = _capi.CmpcWalkGradsMismatch(arr(grad_hidden, f64, (B, 6), "grad_hidden"), arr(grad_noise, f32, (B, 9), "grad_noise"),
                                         self._opt(grad_gain, f64, (B,), "grad_gain"))
        self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_mismatch_device(
            *head, C.byref(r) if r is not None else None, C.byref(mismatch["_c"]), C.byref(mg), st))

    # ---- the gates of the reverse and the forward walk (include/cmpc.h) ----
    def rollout_walk_vjp_gate_device(self, gate, device=None):
        """cmpc_rollout_walk_vjp_gate_device: one gate step of the reverse walk as one launch; gate: a _capi.CmpcWalkGate of device pointers."""
        self._launch(self._dev(device), lambda st: self._lib.cmpc_rollout_walk_vjp_gate_device(self._h, C.byref(gate), st))

    def rollout_walk_vjp_rot_gate_device(self, gate, device=None):
        """cmpc_rollout_walk_vjp_rot_gate_device: one gate step of the reverse walk with the orientation arrays as one launch; gate: a
        _capi.CmpcWalkGateRot of device pointers."""
        self._launch(self._dev(device), lambda st: self._lib.cmpc_rollout_walk_vjp_rot_gate_device(self._h, C.byref(gate), st))

    def rollout_walk_jvp_device(self, tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot=None, dir_plan=None,
                                dir_plan_rot=None, dir_wrench=None, dir_model=None, dir_p=None, dir_x=None, removed=None):
        """cmpc_rollout_walk_jvp_device: rows row0 .. row0 + ticks - 1 of tape (walk_tape) forwards in k directions in ONE call.  dir_states
        [rows + 1, B, k, 9] float64: row row0 is read, rows row0 + 1 .. row0 + ticks are written; carry_list / carry_list_rot[B, k, 2, M, 3] float64 go in as
        the list directions entering the first row and come back as those leaving the last (carry_list_rot and dir_plan_rot both None: no rotation chain);
        dir_plan / dir_plan_rot[B, k, 2, M, 3], dir_model[B, k, 34] float64, dir_wrench[rows, B, k, N, 6], dir_p[rows, B, k, n_p] float32 (None: zero);
        dir_x[rows, B, k, n_x] float32 (or None), status[rows, B] int32 and removed[rows, B] float32 (or None) are written row by row.  end_tick: int32
        [B] (a walk record's) or None."""
        self._rollout_walk_jvp(tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot, dir_plan, dir_plan_rot, dir_wrench,
                               dir_model, dir_p, dir_x, removed, None)

    def rollout_walk_jvp_mismatch_device(self, tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, mismatch=None, dir_hidden=None,
                                         dir_noise=None, dir_gain=None, carry_list_rot=None, dir_plan=None, dir_plan_rot=None, dir_wrench=None, dir_model=None,
                                         dir_p=None, dir_x=None, removed=None):
        """cmpc_rollout_walk_jvp_mismatch_device: rollout_walk_jvp_device on a walk that ran under `mismatch` (plant_mismatch(...); None: none was applied and
        only the directions are), with the directions of its three parts, rows as the tape's: dir_hidden[rows, B, k, 6] float64, dir_noise[rows, B, k, 9]
        float32, dir_gain[B, k] float64 (each may be None: zero).  All four None: the call above, bit for bit."""
        self._rollout_walk_jvp(tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot, dir_plan, dir_plan_rot, dir_wrench,
                               dir_model, dir_p, dir_x, removed, (mismatch, dir_hidden, dir_noise, dir_gain))

    def _rollout_walk_jvp(self, tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot, dir_plan, dir_plan_rot, dir_wrench,
                          dir_model, dir_p, dir_x, removed, mm):
        import torch
        L, B, N, M, R, k = self.layout, self.batch, self.cfg.N, int(tape["max_contacts"]), int(tape["rows"]), int(k)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        g3 = (B, k, 2, M, 3)
        d = _capi.CmpcWalkDirs(self._opt(dir_states, f64, (R + 1, B, k, 9), "dir_states"), self._opt(carry_list, f64, g3, "carry_list"),
                               self._opt(carry_list_rot, f64, g3, "carry_list_rot"), self._opt(dir_plan, f64, g3, "dir_plan"),
                               self._opt(dir_plan_rot, f64, g3, "dir_plan_rot"), self._opt(dir_wrench, f32, (R, B, k, N, 6), "dir_wrench"),
                               self._opt(dir_model, f64, (B, k, _capi.MODEL_DOUBLES), "dir_model"), self._opt(dir_p, f32, (R, B, k, L.np), "dir_p"),
                               self._opt(dir_x, f32, (R, B, k, L.nx), "dir_x"), self._opt(status, i32, (R, B), "status"),
                               self._opt(removed, f32, (R, B), "removed"))
        e = self._opt(end_tick, i32, (B,), "end_tick")
        if mm is None:
            self._launch(dir_states.device, lambda st: self._lib.cmpc_rollout_walk_jvp_device(self._h, M, int(tick0), int(ticks), tape["_c"], int(row0), e, k, d, st))
            return
        mismatch, dir_hidden, dir_noise, dir_gain = mm
        md = _capi.CmpcWalkDirsMismatch(self._opt(dir_hidden, f64, (R, B, k, 6), "dir_hidden"), self._opt(dir_noise, f32, (R, B, k, 9), "dir_noise"),
                                        self._opt(dir_gain, f64, (B, k), "dir_gain"))
        self._launch(dir_states.device, lambda st: self._lib.cmpc_rollout_walk_jvp_mismatch_device(
            self._h, M, int(tick0), int(ticks), tape["_c"], int(row0), e, k, d, C.byref(mismatch["_c"]) if mismatch is not None else None, C.byref(md), st))

    def rollout_walk_jvp_gate_device(self, gate, device=None):
        """cmpc_rollout_walk_jvp_gate_device: one gate step of the forward walk as one launch; gate: a _capi.CmpcWalkJvpGate of device pointers."""
        self._launch(self._dev(device), lambda st: self._lib.cmpc_rollout_walk_jvp_gate_device(self._h, C.byref(gate), st))


    # ---- sensed pushes: the sensor's transpose and tangent (include/cmpc.h, cmpc_wrench_sensor).  Private: the public names are WalkingRollout's ----
    def _wrench_sense_vjp_device(self, tick0, rows, mismatch, sensor, grad_wrench, grad_hidden):
        """cmpc_wrench_sense_vjp_device: the reverse walk's wrench[rows, B, N, 6] float32 and hidden_wrench[rows, B, 6] float64 (taken on the plant rows)
        -> (hidden_wrench[Th, B, 6], sensor_noise[Tn, B, 6] or None) float64, shaped as the schedules of mismatch and sensor, in one launch"""
        import torch
        B, N, f64 = self.batch, self.cfg.N, torch.float64
        gw = ptr(grad_wrench, torch.float32, (rows, B, N, 6), "grad_wrench", required=True)
        gh = ptr(grad_hidden, f64, (rows, B, 6), "grad_hidden", required=True)
        dev = grad_wrench.device
        gt = torch.empty(tuple(mismatch["hidden_wrench"].shape), dtype=f64, device=dev)
        gn = None if sensor["noise"] is None else torch.empty(tuple(sensor["noise"].shape), dtype=f64, device=dev)
        self._launch(dev, lambda st: self._lib.cmpc_wrench_sense_vjp_device(
            self._h, int(tick0), int(rows), C.byref(mismatch["_c"]), C.byref(sensor["_c"]), gw, gh, gt.data_ptr(), None if gn is None else gn.data_ptr(), st),
            "cmpc_wrench_sense_vjp_device")
        return gt, gn

    def _wrench_sense_jvp_device(self, tick0, rows, k, mismatch, sensor, dir_hidden, dir_noise=None):
        """cmpc_wrench_sense_jvp_device: dir_hidden[Th, B, k, 6] and dir_noise[Tn, B, k, 6] (or None) float64 -> (dir_wrench[rows, B, k, N, 6] float32,
        dir_plant_wrench[rows, B, k, 6] float64): what cmpc_walk_dirs.dDirWrench and cmpc_walk_dirs_mismatch.dDirHidden take, in one launch"""
        import torch
        B, N, f64, k = self.batch, self.cfg.N, torch.float64, int(k)
        dh = ptr(dir_hidden, f64, (int(mismatch["hidden_wrench"].shape[0]), B, k, 6), "dir_hidden", required=True)
        dn = None
        if sensor["noise"] is not None:
            dn = ptr(dir_noise, f64, (int(sensor["noise"].shape[0]), B, k, 6), "dir_noise")
        dev = dir_hidden.device
        dw = torch.empty((rows, B, k, N, 6), dtype=torch.float32, device=dev)
        dp = torch.empty((rows, B, k, 6), dtype=f64, device=dev)
        self._launch(dev, lambda st: self._lib.cmpc_wrench_sense_jvp_device(
            self._h, int(tick0), int(rows), k, C.byref(mismatch["_c"]), C.byref(sensor["_c"]), dh, dn, dw.data_ptr(), dp.data_ptr(), st),
            "cmpc_wrench_sense_jvp_device")
        return dw, dp
