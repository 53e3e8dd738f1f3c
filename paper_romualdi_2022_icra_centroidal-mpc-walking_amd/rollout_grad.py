"""The device derivatives of WalkingRollout (a base class without state): the device walk in reverse and in forward mode, each public method a thin
front of ONE driver (_backward_device, _backward_checkpointed, _forward_sensitivity_device).  The host-stepped ones are rollout.py's."""
from .rollout_common import bound, direction, need, seed, tensor


class WalkGrads:
    def backward_device(self, w, grad_states, grad_X=None):
        """The device walk in reverse (cmpc_rollout_walk_vjp_device): ONE call per replan segment, last segment first, no host read and no synchronisation.
        w = walk_device_taped(...); grad_states[ticks + 1, B, 9] and grad_X[ticks, B, n_x] (or None) as in backward(), CUDA tensors or numpy.
        -> the keys of backward() -- state0, list0, wrench, push, models, plan, status -- and end_tick (w's).  A problem that ended at tick e
        (w["end_tick"]) contributes the loss over its states 0 .. e and its solutions 0 .. e - 1 (include/cmpc.h: the seeds of its later rows are not read,
        not even when they are not finite); its rows e .. of wrench are zero and of status 6.  Where nothing ended every entry is bit-equal to
        run(tape=True) + backward().  The contacts' orientations too: backward_device_rot()."""
        return self._backward_device(w, grad_states, grad_X, False)

    def backward_device_rot(self, w, grad_states, grad_X=None):
        """backward_device() with the contacts' orientations carried along (cmpc_rollout_walk_vjp_rot_device; body-frame tangents, as backward(rot=True)):
        still ONE call per replan segment, no host read and no synchronisation.  The dict also holds list_rot0[B, 2, M, 3] (the first tick's lists),
        plan_rot[B, 2, M, 3] (the planner's contacts, accumulated in one buffer over the segments as plan is), rot[ticks, B, 2, N, 3] (each tick's
        per-stage dl/domega), float64, and removed[ticks, B] float32 (word 6 of each tick's dSens); every key backward_device() also has is bit-equal to
        it.  A problem that ended at tick e: its rows e .. of rot are zero and of removed 0, and nothing of its later rows reaches list_rot0 or plan_rot.
        Where nothing ended every entry is bit-equal to run(tape=True) + backward(rot=True).  (A method of its own and not an argument of
        backward_device: that signature is pinned.)"""
        return self._backward_device(w, grad_states, grad_X, True)

    def backward_device_refs(self, w, grad_states, grad_X=None, rot=False):
        """backward_device() (rot=True: backward_device_rot()) with the gradient of the planner's CoM and angular-momentum trajectories -- the ones
        set_references() installed, or the default straight line; w["tape"]["references"] says which timing: the reverse walk runs with its grad_p rows on,
        and ONE call of cmpc_reference_from_planner_vjp_device over all rows with w["end_tick"] carries their comRef / hRef entries through the transpose
        of every tick's resampling.  Still no host read and no synchronisation.  -> the other method's keys, bit-equal, plus ref_com, ref_h [B, n, 3]
        float64 and grad_P [ticks, B, n_p] float32 (each tick's full dl/dp; zero rows behind a problem's end).  A problem that ended at tick e contributes
        its solutions 0 .. e - 1: its later rows of grad_P are not read.  With a fixed CoM height (the default 0.7) ref_com[..., 2] is exactly zero.
        Times, robot_mass and com_height are not differentiated.  (A method of its own: the signatures of backward_device / _rot are pinned.)"""
        return self._backward_device(w, grad_states, grad_X, rot, refs=True)

    def backward_device_measures(self, w, grad_measures, grad_states=None, grad_X=None, refs=False):
        """backward_device() (refs=True: backward_device_refs()) of a loss that is also seeded on the walk's stability measures (include/cmpc.h, "the
        measures, differentiated"): grad_measures[ticks, B, 4] float64 (CUDA or numpy) is the cotangent of height, reach, margin, track of every tick, as
        w["measures"] holds them; grad_states / grad_X as in backward_device (None: zero).  Queued on the launch stream with no host read: ONE launch of
        cmpc_walk_measures_vjp_device adds the measures' share to copies of the two seeds, the reverse walk runs on them as it is, and one small launch
        (cmpc_walk_measures_vjp_fold_device) adds the comRef term to grad_P -- in front of the reference VJP, which carries it into ref_com -- and the
        corners' term to models[:, 10:34].  -> the other method's keys, plus measure_direct[ticks, B, 32] float64 (comRef_xy 2, omega [2][3], corner
        [2][4][3] per tick: what no seed carries) and measure_rot[ticks, B, 2, 3], its omega part as a view: the stage-1 rotations' body-frame tangent,
        returned and NOT chained into the lists' or the planner's orientations.  A problem that ended at tick e contributes the measures of its ticks
        0 .. e - 1: the row that fired and the rows behind it are not read, whatever they hold.  With grad_measures all zero every shared key is
        bit-equal to the other method's.  The corners are those the walk's record read (the solver's, or the installed models'); a mismatch tape works
        as it is.  Not for checkpointed walks or a regrouped refill tape."""
        torch, B, L, s, z = self.torch, self.B, self.L, self.solver, self._z
        tape, T = w["tape"], w["tape"]["rows"]
        gM = seed(grad_measures, self.dev, torch.float64, (T, B, 4), "grad_measures", lambda t: f"grad_measures of shape {tuple(t.shape)}: expected {(T, B, 4)}")
        gS0 = None if grad_states is None else seed(grad_states, self.dev, torch.float64, (T + 1, B, 9), "grad_states")
        gX0 = None if grad_X is None else seed(grad_X, self.dev, torch.float32, (T, B, L.nx), "grad_X")

        def seeds():    # (a stream block of its own, in front of the reverse walk's)
            gS = z((T + 1, B, 9)) if gS0 is None else gS0.clone()
            gX = z((T, B, L.nx), torch.float32) if gX0 is None else gX0.clone()
            direct = z((T, B, 32))
            s.walk_measures_vjp_device(0, T, tape, 0, w["end_tick"], gM, gS, gX, direct)
            return gS, gX, direct
        gS, gX, direct = self._on_launch_stream(seeds)
        fold = lambda out: s.walk_measures_vjp_fold_device(direct, out.get("grad_P"), out["models"])
        out = self._backward_device(w, gS, gX, False, refs=refs, fold=fold)
        out["measure_direct"] = direct
        out["measure_rot"] = direct[:, :, 2:8].unflatten(2, (2, 3))
        return out

    def _backward_device(self, w, grad_states, grad_X, rot, refs=False, fold=None):
        tape = w["tape"]
        T, M, s = tape["rows"], tape["max_contacts"], self.solver
        mm = tape.get("mismatch")    # (the tape of a mismatched walk: cmpc_rollout_walk_vjp_mismatch_device, and three more keys)
        gS, gX, out = self._reverse_outputs(w, T, M, grad_states, grad_X, rot, tape["references"]["knots"] if refs else None, mm is not None)
        starts = list(tape["segments"])

        def reverse():
            g, gl, glr = gS[T].clone(), self._z((self.B, 2, M, 3)), self._z((self.B, 2, M, 3)) if rot else None    # (the gate selects zero where a problem ended)
            for j in reversed(range(len(starts))):
                t0, t1 = starts[j], starts[j + 1] if j + 1 < len(starts) else T
                s.rollout_walk_vjp_device(t0, t1 - t0, tape, t0, w["end_tick"], gS, g, gl, out["status"], grad_X=gX, wrench=out["wrench"],
                                          grad_p=out.get("grad_P"), dGradPlan=out["plan"], dGradModel=out["models"], carry_list_rot=glr, dGradPlanRot=out.get("plan_rot"),
                                          grad_rot=out.get("rot"), removed=out.get("removed"), mismatch=mm, grad_hidden=out.get("hidden_wrench"),
                                          grad_noise=out.get("state_noise"), grad_gain=out.get("force_gain"))
            self._reverse_finish(out, T, tape["push_ticks"], g, gl, glr)
            if fold is not None:    # (backward_device_measures: what the measures send to grad_P and models directly, in front of the reference VJP)
                fold(out)
            if refs:    # (the replan segments share the trajectories: one launch over all rows)
                s.reference_from_planner_vjp_device(0, T, tape["references"], w["end_tick"], out["grad_P"], out["ref_com"], out["ref_h"])
            return out
        return self._on_launch_stream(reverse)

    def _reverse_outputs(self, w, T, M, grad_states, grad_X, rot, n_ref, mismatched):
        """the seeds of a reverse walk of T ticks as checked tensors and its zeroed outputs -> (gS, gX, out)"""
        torch, B, N, L, z = self.torch, self.B, self.cfg.N, self.L, self._z
        gS = seed(grad_states, self.dev, torch.float64, (T + 1, B, 9), "grad_states")
        gX = None if grad_X is None else seed(grad_X, self.dev, torch.float32, (T, B, L.nx), "grad_X")
        out = dict(push=z((B, 3)), wrench=z((T, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((T, B), torch.int32),
                   end_tick=w["end_tick"])
        if rot:
            out.update(plan_rot=z((B, 2, M, 3)), rot=z((T, B, 2, N, 3)), removed=z((T, B), torch.float32))
        if n_ref is not None:
            out.update(grad_P=z((T, B, L.np), torch.float32), ref_com=z((B, n_ref, 3)), ref_h=z((B, n_ref, 3)))
        if mismatched:
            out.update(hidden_wrench=z((T, B, 6)), state_noise=z((T, B, 9), torch.float32), force_gain=z((B,)))
        return gS, gX, out

    def _reverse_finish(self, out, T, push_ticks, g, gl, glr):
        """the push's gradient (backward()'s expression, tick by tick in its order) and the carries behind tick 0 into out"""
        for i in reversed(range(min(T, push_ticks))):
            out["push"] += out["wrench"][i][:, :max(push_ticks - i, 1), :3].to(self.torch.float64).sum(1)
        out["state0"], out["list0"] = g, gl
        if glr is not None:
            out["list_rot0"] = glr

    def _sensed_tape(self, who, w):
        """(w with the tape's mismatch replaced by the one the plant ran under -- hidden schedule plant_wrench from tick 0, the walk's gain --, the walk's
        mismatch, the sensor)"""
        tape = w.get("tape")
        if tape is None or tape.get("sensor") is None or "segments" not in tape:
            raise ValueError(f"{who}: w is not walk_device_sensed(..., tape=True) with a sensor")
        mm = tape["mismatch"]
        plant_mm = self.solver.plant_mismatch(hidden_wrench=tape["plant_wrench"], force_gain=mm["force_gain"], tick_first=0, device=self.dev)
        return dict(w, tape=dict(tape, mismatch=plant_mm)), mm, tape["sensor"]

    def backward_device_sensed(self, w, grad_states, grad_X=None):
        """backward_device(w, grad_states, grad_X) on w = walk_device_sensed(..., tape=True): the reverse walk runs on the tape with the plant's own
        schedule (plant_wrench) as its hidden wrench, then ONE launch of cmpc_wrench_sense_vjp_device carries the wrench rows' and the plant rows'
        gradients through the transpose of the sensor.  -> backward_device's keys on that tape, in which plant_wrench[ticks, B, 6] is what backward_device
        calls hidden_wrench; hidden_wrench[Th, B, 6] float64 is the TOTAL gradient with respect to the true pushes, shaped as the schedule; sensor_noise
        [Tn, B, 6] float64 (None without sensor noise).  A problem that ended at tick e: its rows from e on (shifted by the delay) are exactly zero.  No
        host read."""
        w2, mm, sn = self._sensed_tape("backward_device_sensed", w)
        out = self._backward_device(w2, grad_states, grad_X, False)
        out["plant_wrench"] = out["hidden_wrench"]
        T = w["tape"]["rows"]
        out["hidden_wrench"], out["sensor_noise"] = self._queued(
            lambda: self.solver._wrench_sense_vjp_device(0, T, mm, sn, out["wrench"], out["plant_wrench"]))
        return out

    def forward_sensitivity_device_sensed(self, w, k, dir_hidden_wrench=None, dir_sensor_noise=None, dir_state_noise=None, dir_force_gain=None,
                                          dir_ref_com=None, dir_ref_h=None, **dirs):
        """forward_sensitivity_device_mismatch on w = walk_device_sensed(..., tape=True), in k columns, with directions of the TRUE pushes and of the sensor
        noise: dir_hidden_wrench[Th, B, k, 6] and dir_sensor_noise[Tn, B, k, 6] float64 (CUDA or numpy; None: zero), shaped as the schedules.  ONE launch of
        cmpc_wrench_sense_jvp_device turns them into the wrench rows' and the plant rows' directions, which the forward walk takes as dir_wrench and
        dir_hidden_wrench; the other direction groups as in forward_sensitivity_device_mismatch (dir_wrench itself is refused: the MPC's wrench is the
        sensed one).  The transpose of backward_device_sensed(), input for output; no host read."""
        torch = self.torch
        if dirs.get("dir_wrench") is not None:
            raise ValueError("forward_sensitivity_device_sensed: dir_wrench is the sensor's output here; give dir_hidden_wrench / dir_sensor_noise")
        w2, mm, sn = self._sensed_tape("forward_sensitivity_device_sensed", w)
        T, k = w["tape"]["rows"], int(k)
        dh = self._z(tuple(mm["hidden_wrench"].shape[:2]) + (k, 6)) if dir_hidden_wrench is None else tensor(dir_hidden_wrench, self.dev, torch.float64)
        dn = None if dir_sensor_noise is None or sn["noise"] is None else tensor(dir_sensor_noise, self.dev, torch.float64)
        dw, dp = self._queued(lambda: self.solver._wrench_sense_jvp_device(0, T, k, mm, sn, dh, dn))
        return self.forward_sensitivity_device_mismatch(w2, dir_hidden_wrench=dp, dir_state_noise=dir_state_noise, dir_force_gain=dir_force_gain,
                                                        dir_ref_com=dir_ref_com, dir_ref_h=dir_ref_h, **dict(dirs, dir_wrench=dw))

    def backward_device_checkpointed(self, w, grad_states, grad_X=None, rot=False):
        """backward_device (rot=True: backward_device_rot) without a whole-walk tape.  w = walk_device_checkpointed(...).  For each segment between two
        checkpoints, last first: the segment's snapshot is restored into workspace buffers (segment 0: the start is set up again from w["inputs"]), the
        segment is run again through cmpc_rollout_walk_taped_device into ONE re-used tape of at most every + 1 rows, and reversed through the carries
        with cmpc_rollout_walk_vjp[_rot]_device and w["end_tick"].  A segment that does not start at tick 0 has no first tick: its tape says
        first_row_is_first_tick = 0, its row 0 is a stub that holds the snapshot's list times and counts, and it is taped and reversed from row 1.
        The walk is bit-reproducible and the reverse walk composes over segments to the bit, so every key equals the full-tape method's bit for bit, at
        the cost of one more forward walk (a forward tick is about a tenth of a reverse tick).
        grad_states[ticks + 1, B, 9] as in backward_device; grad_X: None, a [ticks, B, n_x] tensor, or a callable (t0, t1, tape_segment) -> [t1 - t0, B,
        n_x] float32 CUDA tensor that runs once per segment with views of that segment's tape rows (X, P, lam_g, info, ok, land, states[t1 - t0 + 1]),
        so that the dense seeds need not exist either.
        -> the keys of backward_device (rot=True: of backward_device_rot) plus "tape_rows_peak".  No host read once the workspaces exist (the first
        call allocates them and turns the multiplier output on).  Out of scope: the reference gradients (backward_device_refs: their one-launch sum has
        a fixed ascending order that per-segment calls in reverse would change), the forward-mode walk, and refilled walks (walk_device_refill has no
        tape and no gradient).  A walk that ran under a plant mismatch is refused here (NotImplementedError): backward_device_checkpointed_mismatch()."""
        return self._queued(lambda: self._backward_checkpointed(w, grad_states, grad_X, rot))

    def backward_device_checkpointed_mismatch(self, w, grad_states, grad_X=None, rot=False):
        """backward_device_checkpointed for w = walk_device_checkpointed(..., mismatch=...): the same loop, with each segment run again UNDER THE MISMATCH
        (w["inputs"]["mismatch"], kept alive there) and reversed with cmpc_rollout_walk_vjp_mismatch_device.  -> backward_device's keys on a mismatch
        tape -- hidden_wrench[ticks, B, 6] float64, state_noise[ticks, B, 9] float32 and force_gain[B] float64 besides the others -- plus
        "tape_rows_peak".  The segments are reversed last first, so force_gain accumulates tick by tick in the full walk's order: every key equals
        backward_device's on walk_device_taped(mismatch=...) bit for bit.  A walk without a mismatch gives backward_device_checkpointed's dict.  (A
        method of its own: backward_device_checkpointed's signature and its refusal of a mismatch are pinned.)"""
        return self._queued(lambda: self._backward_checkpointed(w, grad_states, grad_X, rot, mismatch=True))

    def _backward_checkpointed(self, w, grad_states, grad_X, rot, mismatch=False):
        B, L, M, s, dev = self.B, self.L, self.M, self.solver, self.dev
        inp, cps = w["inputs"], w["checkpoints"]
        mm = inp.get("mismatch")
        if inp.get("sensor") is not None:    # (the sensor's delay couples rows across segments: its fold must run once over the whole arrays)
            raise NotImplementedError("backward_device_checkpointed: the walk ran under a wrench sensor; its reverse is backward_device_sensed on a tape")
        if mm is not None and not mismatch:
            raise NotImplementedError("backward_device_checkpointed: the walk ran under a plant mismatch; its reverse in bounded memory is "
                                      "backward_device_checkpointed_mismatch")
        T, every = inp["ticks"], inp["every"]
        # (backward_device's keys, the mismatch's three too; a callable grad_X gives its rows segment by segment)
        gS, gX, out = self._reverse_outputs(w, T, M, grad_states, None if callable(grad_X) else grad_X, rot, None, mm is not None)
        rows = min(every, T) + 1
        key = (rows, inp["stop"])
        ws = getattr(self, "_checkpoint_ws", None)
        if ws is None or ws["key"] != key:    # (one set of live buffers, one record without a trace and one tape, re-used by every segment and every call)
            s.set_multiplier_output(True)
            rec = s.walk_record(rows, stop=inp["stop"], trace=False, device=dev)
            ws = dict(key=key, live=self._live_buffers(rec),
                      tape=s.walk_tape(rows, M, step=self.cfg.sampling_time / self.substeps, substeps=self.substeps,
                                       force_sample_time=self.force_sample_time, device=dev),
                      gx=self._z((rows, B, L.nx), self.torch.float32))
            self._checkpoint_ws = ws
        live, tp = ws["live"], ws["tape"]
        bounds = [0] + sorted(cps) + [T]
        g, gl, glr = gS[T].clone(), self._z((B, 2, M, 3)), self._z((B, 2, M, 3)) if rot else None    # (as _backward_device's)
        peak = 0
        for j in reversed(range(len(bounds) - 1)):
            c0, c1 = bounds[j], bounds[j + 1]
            r0 = 0 if c0 == 0 else 1
            if c0 == 0:
                self._live_reset(live, inp["state0"], inp["replan"].get(0, inp["plan"]))
            else:
                s.rollout_snapshot_device(cps[c0], live)
                prev = live["lists"][live["lists_in"]]
                tp["list_t"][0].copy_(prev[0])
                tp["list_n"][0].copy_(prev[2])
            tp["_c"].first_row_is_first_tick = 1 if c0 == 0 else 0
            self._walk_live(live, c0, c1, c0, inp["replan"], inp["plan"], inp["wrench"], inp["refs"], inp["skip_ended"], tape=tp, tape_shift=c0 - r0,
                            cold=c0 == 0, mismatch=mm, limits=inp.get("limits"))
            gx_rows = None
            if callable(grad_X):
                seg = {k: tp[k][r0:r0 + c1 - c0] for k in ("X", "P", "lam_g", "info", "ok", "land", "plan_t", "list_t", "plan_n", "list_n")}
                seg["states"] = tp["states"][r0:r0 + c1 - c0 + 1]
                ws["gx"][r0:r0 + c1 - c0].copy_(grad_X(c0, c1, seg))
                gx_rows = ws["gx"]
            s.rollout_walk_vjp_rows_device(c0, c1 - c0, tp, r0, w["end_tick"], gS, g, gl, out["status"], grad_X=gX, grad_X_rows=gx_rows, wrench=out["wrench"],
                                           dGradPlan=out["plan"], dGradModel=out["models"], carry_list_rot=glr, dGradPlanRot=out.get("plan_rot"),
                                           grad_rot=out.get("rot"), removed=out.get("removed"), mismatch=mm, grad_hidden=out.get("hidden_wrench"),
                                           grad_noise=out.get("state_noise"), grad_gain=out.get("force_gain"))
            peak = max(peak, r0 + c1 - c0)
        self._reverse_finish(out, T, inp["push_ticks"], g, gl, glr)
        out["tape_rows_peak"] = peak
        return out

    def forward_sensitivity_device(self, w, dir_state0=None, dir_list0=None, dir_list_rot0=None, dir_plan=None, dir_plan_rot=None, dir_push=None,
                                   dir_models=None, dir_wrench=None, solutions=False):
        """The device walk in forward mode (cmpc_rollout_walk_jvp_device): ONE call per replan segment, first segment first, no host read and no
        synchronisation -- the transpose of backward_device(), input for output, with the orientations carried along.  w = walk_device_taped(...); the
        directions and the returned dict as forward_sensitivity() (k columns right behind B; dir_plan / dir_plan_rot are read by every segment), plus
        end_tick (w's).  A problem that ended at tick e (w["end_tick"]) keeps the directions of its states 0 .. e and of its solutions 0 .. e - 1
        (include/cmpc.h): its rows e + 1 .. of states, e .. of X and its final list directions are exactly zero, its rows e .. of status 6 and of removed 0,
        whatever its later tape rows or its rows of the directions hold -- not even NaN leaks.  Where nothing ended every entry is bit-equal to
        run(tape=True) + forward_sensitivity().  Directions of the planner's reference trajectories too: forward_sensitivity_device_refs().  A tape that
        carries a plant mismatch is refused (NotImplementedError): forward_sensitivity_device_mismatch()."""
        return self._forward_sensitivity_device(w, None, None, dir_state0, dir_list0, dir_list_rot0, dir_plan, dir_plan_rot, dir_push, dir_models, dir_wrench,
                                                solutions)

    def forward_sensitivity_device_refs(self, w, dir_ref_com=None, dir_ref_h=None, **dirs):
        """forward_sensitivity_device(w, **dirs) with directions of the planner's CoM and angular-momentum trajectories as well: dir_ref_com / dir_ref_h
        [B, k, n, 3] float64 (CUDA tensors or numpy; None: zero), n = w["tape"]["references"]["knots"].  ONE call of
        cmpc_reference_from_planner_jvp_device fills the comRef / hRef entries of a zeroed dir_p[ticks, B, k, n_p], which the forward walk reads as every
        tick's extra p direction.  The same dict comes back; the transpose of backward_device_refs(), input for output; no host read.  (A method of its
        own: forward_sensitivity_device's signature is pinned.)"""
        args = bound(self.forward_sensitivity_device, w, **dirs)
        return self._forward_sensitivity_device(w, dir_ref_com, dir_ref_h, *args.args[1:], **args.kwargs)

    def forward_sensitivity_device_mismatch(self, w, dir_hidden_wrench=None, dir_state_noise=None, dir_force_gain=None, dir_ref_com=None, dir_ref_h=None,
                                            **dirs):
        """forward_sensitivity_device_refs(w, dir_ref_com, dir_ref_h, **dirs) on a walk that ran under a plant mismatch, w = walk_device_taped(...,
        mismatch=...), with directions of the mismatch as well (cmpc_rollout_walk_jvp_mismatch_device): dir_hidden_wrench[ticks, B, k, 6] float64,
        dir_state_noise[ticks, B, k, 9] float32, dir_force_gain[B, k] float64 (CUDA tensors or numpy; None: zero) -- row i is the direction of what tick
        i's plant felt (hidden wrench; applied also where the schedule had no row: the wrench there was zero) or what tick i's MPC measured (noise: it
        enters the solve only).  The plant's partials are the mismatched plant's.  The same dict comes back: the transpose of backward_device() on that
        tape, its keys hidden_wrench, state_noise and force_gain included, input for output; ONE call per replan segment, no host read.  On a tape
        without a mismatch and without the three directions every key is bit-equal to forward_sensitivity_device_refs.  (A method of its own:
        forward_sensitivity_device's signature and its refusal of a mismatch tape are pinned.)"""
        args = bound(self.forward_sensitivity_device, w, **dirs)
        return self._forward_sensitivity_device(w, dir_ref_com, dir_ref_h, *args.args[1:], **args.kwargs,
                                                mismatch_dirs=(dir_hidden_wrench, dir_state_noise, dir_force_gain))

    def forward_sensitivity_device_measures(self, w, **dirs):
        """forward_sensitivity_device(w, solutions=True, **dirs) followed by ONE launch of cmpc_walk_measures_jvp_device on what it returned: the dict
        gains measures[ticks, B, k, 4] float64, the directions of height, reach, margin, track of every tick -- through the states, the knot-1 foot
        positions of the solutions' directions and, with dir_models, the corners.  The transpose of backward_device_measures(), input for output; no
        host read.  Rows at or past a problem's end are zero.  The stage-1 rotations carry no direction (their term is not chained in reverse
        either).  (A method of its own: forward_sensitivity_device's signature is pinned.)"""
        torch, B, s = self.torch, self.B, self.solver
        dirs = dict(dirs, solutions=True)
        r = self.forward_sensitivity_device(w, **dirs)
        tape = w["tape"]
        T, k = tape["rows"], int(r["states"].shape[2])
        dmod = dirs.get("dir_models")
        if dmod is not None:
            dmod = tensor(dmod, self.dev, torch.float64)

        def measures():
            r["measures"] = self._z((T, B, k, 4))
            s.walk_measures_jvp_device(0, T, tape, 0, w["end_tick"], k, r["states"], r["X"], r["measures"], dir_model=dmod)
            return r
        return self._on_launch_stream(measures)

    def _forward_sensitivity_device(self, w, dir_ref_com, dir_ref_h, dir_state0, dir_list0, dir_list_rot0, dir_plan, dir_plan_rot, dir_push, dir_models,
                                    dir_wrench, solutions, mismatch_dirs=None):
        torch, B, N, L = self.torch, self.B, self.cfg.N, self.L
        tape = w["tape"]
        if tape.get("mismatch") is not None and mismatch_dirs is None:    # (the plain tick JVP takes its partials at the MPC's forces and wrench: on this tape it would be silently wrong)
            raise NotImplementedError("forward_sensitivity_device: the tape carries a plant mismatch; its forward mode is forward_sensitivity_device_mismatch")
        T, M, s = tape["rows"], tape["max_contacts"], self.solver
        as_dir = lambda a, dtype, tail, lead=(): direction(a, self.dev, B, dtype, tail, lead)
        f32, f64, z = torch.float32, torch.float64, self._z
        ds, dl, dlr = as_dir(dir_state0, f64, (9,)), as_dir(dir_list0, f64, (2, M, 3)), as_dir(dir_list_rot0, f64, (2, M, 3))
        dpl, dplr = as_dir(dir_plan, f64, (2, M, 3)), as_dir(dir_plan_rot, f64, (2, M, 3))
        dpush, dmod, dwr = as_dir(dir_push, f32, (3,)), as_dir(dir_models, f64, (34,)), as_dir(dir_wrench, f32, (N, 6), lead=(T,))
        drc = drh = None
        if dir_ref_com is not None or dir_ref_h is not None:
            n_ref = tape["references"]["knots"]
            drc, drh = as_dir(dir_ref_com, f64, (n_ref, 3)), as_dir(dir_ref_h, f64, (n_ref, 3))
        dmh = dmn = dmg = None
        if mismatch_dirs is not None:
            dmh, dmn = as_dir(mismatch_dirs[0], f64, (6,), lead=(T,)), as_dir(mismatch_dirs[1], f32, (9,), lead=(T,))
            dmg = as_dir(mismatch_dirs[2], f64, ())
        ks = {int(a.shape[1]) for a in (ds, dl, dlr, dpl, dplr, dpush, dmod, drc, drh, dmg) if a is not None} | {
            int(a.shape[2]) for a in (dwr, dmh, dmn) if a is not None}
        need(len(ks) == 1, "forward_sensitivity_device: no direction, or directions of different k")
        k = ks.pop()
        rot = dlr is not None or dplr is not None
        out = dict(states=z((T + 1, B, k, 9)), status=z((T, B), torch.int32), removed=z((T, B), f32), end_tick=w["end_tick"])
        if solutions:
            out["X"] = z((T, B, k, L.nx), f32)
        starts = list(tape["segments"])

        def forward(dwr):
            if ds is not None:
                out["states"][0] = ds
            push_ticks = min(T, tape["push_ticks"]) if dpush is not None else 0
            if push_ticks > 0:      # (forward_sensitivity()'s expression, tick by tick)
                dwr = z((T, B, k, N, 6), f32) if dwr is None else dwr.clone()
                for i in range(push_ticks):
                    dwr[i][:, :, :max(tape["push_ticks"] - i, 1), :3] += dpush[:, :, None, :]
            cl = z((B, k, 2, M, 3)) if dl is None else dl.clone()
            clr = None if not rot else z((B, k, 2, M, 3)) if dlr is None else dlr.clone()
            dp = None
            if drc is not None or drh is not None:    # (the replan segments share the trajectories: one launch over all rows)
                dp = z((T, B, k, L.np), f32)
                s.reference_from_planner_jvp_device(0, T, k, tape["references"], dp, drc, drh)
            # (a tape without a mismatch and no direction of one: the plain entry, call for call)
            walk, mm = s.rollout_walk_jvp_device, {}
            if mismatch_dirs is not None and not (tape.get("mismatch") is None and dmh is None and dmn is None and dmg is None):
                walk, mm = s.rollout_walk_jvp_mismatch_device, dict(mismatch=tape.get("mismatch"), dir_hidden=dmh, dir_noise=dmn, dir_gain=dmg)
            for j, t0 in enumerate(starts):
                t1 = starts[j + 1] if j + 1 < len(starts) else T
                walk(t0, t1 - t0, tape, t0, w["end_tick"], k, out["states"], cl, out["status"], carry_list_rot=clr, dir_plan=dpl, dir_plan_rot=dplr,
                     dir_wrench=dwr, dir_model=dmod, dir_p=dp, dir_x=out.get("X"), removed=out["removed"], **mm)
            out["list"] = cl
            out["list_rot"] = clr if rot else z((B, k, 2, M, 3))
            return out
        return self._on_launch_stream(lambda: forward(dwr))
