"""The roll-out layer of BatchSolver: the methods that call the entries of csrc/cmpc_api_rollout.hip -- tick, record, measures, tape, walks, refill,
snapshot, plan fold, regroup -- each builder of a C struct (walk_record, walk_tape, walk_snapshot, walk_refill*, plant_mismatch) next to the call that
consumes it.  A base class without state: the handle, _launch, _opt, _dev and _box_arrays are BatchSolver's (solver.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args, _capi
from ._args import _upload, opt_ptr, ptr


class RolloutCalls:
    # ---- plant-model mismatch (include/cmpc.h, "plant-model mismatch on the device walk"; DESIGN.md 7f, "Mismatch") ----
    def plant_mismatch(self, hidden_wrench=None, state_noise=None, force_gain=None, tick_first=0, device=None):
        """A cmpc_plant_mismatch as a dict: hidden_wrench[Th, B, 6], state_noise[Tn, B, 9], force_gain[B] float32 (numpy or CUDA tensors, any subset; a
        schedule of zero rows counts as absent), tick_first the tick number of row 0 of the two schedules.  The dict keeps the device tensors alive and holds
        "_c", the C struct that points at them."""
        import torch
        B = self.batch
        dev = self._dev(device)
        hold = []

        def up(a, tail, name):
            if a is None:
                return None
            if not isinstance(a, torch.Tensor):    # (uploaded without the host waiting for the copy; the host array is kept with the dict)
                hold.append(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
                a = hold[-1].to(dev, non_blocking=True)
            t = a
            t = t.detach().to(dev, torch.float32).contiguous()
            if tuple(t.shape[-len(tail):]) != tuple(tail) or t.dim() != len(tail) + (0 if name == "force_gain" else 1):
                raise AssertionError(f"{name}: expected [.., {tail}]")
            return t if t.numel() > 0 else None
        m = dict(hidden_wrench=up(hidden_wrench, (B, 6), "hidden_wrench"), state_noise=up(state_noise, (B, 9), "state_noise"),
                 force_gain=up(force_gain, (B,), "force_gain"), tick_first=int(tick_first))
        rows = lambda t: 0 if t is None else int(t.shape[0])
        m["_host"] = hold
        m["_c"] = _capi.CmpcPlantMismatch(int(tick_first), opt_ptr(m["hidden_wrench"]), rows(m["hidden_wrench"]), opt_ptr(m["state_noise"]),
                                          rows(m["state_noise"]), opt_ptr(m["force_gain"]))
        return m

    def _tick_io(self, plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                 force_sample_time):
        """the cmpc_tick_io of one tick (include/cmpc.h) from torch CUDA tensors; the box limits are the configuration's"""
        from ._capi import CmpcTickIO
        up, lo = self._box_arrays()
        io = CmpcTickIO(*map(opt_ptr, plan[:3]), *(map(opt_ptr, prev) if prev is not None else (None, None, None)), *map(opt_ptr, lists[:3]), opt_ptr(ok),
                        opt_ptr(land), up.ctypes.data, lo.ctypes.data, *map(opt_ptr, (dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp)),
                        float(step), int(substeps), float(zmp_half_x), float(zmp_half_y))
        if planner is not None:   # (dComIn, dHIn, in_dt, t_offset, robot_mass, com_height): the tick writes the reference rows itself
            pc, ph, pdt, poff, mass, height = planner
            io.dPlanCom, io.dPlanH, io.plan_knots, io.plan_dt, io.plan_t_offset = pc.data_ptr(), ph.data_ptr(), int(pc.shape[1]), float(pdt), float(poff)
            io.robot_mass, io.com_height = float(mass), float("nan") if height is None else float(height)
        io.force_sample_time = 1 if force_sample_time else 0
        return io

    def rollout_tick_device(self, now, plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, warm,
                            step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False):
        """cmpc_rollout_tick_device: merge -> sample -> setState -> shift -> solve -> step adjustment -> plant as ONE call (include/cmpc.h); plan / prev /
        lists = (t, pose, n) CUDA tensors, prev None on the first tick (lists is then taken as filled by the caller); dWrench may be None.
        force_sample_time: the planner's lists (the caller's lists on the first tick, in place) are snapped to the MPC grid first (forceSampleTime,
        CentroidalMPCBlock.cpp:586-592); ok is then written on the first tick too."""
        io = self._tick_io(plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                           force_sample_time)
        self._launch(dP.device, lambda st: self._lib.cmpc_rollout_tick_device(self._h, lists[0].shape[2], float(now), 1 if warm else 0, io, st))

    def rollout_tick_mismatch_device(self, tick, mismatch, now, plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, warm,
                                     step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False):
        """cmpc_rollout_tick_mismatch_device: rollout_tick_device with the tick number `tick` selecting the rows of mismatch (plant_mismatch(...), or None:
        rollout_tick_device bit for bit).  dState / dStateOut hold the TRUE state; the measured one goes into dP."""
        io = self._tick_io(plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                           force_sample_time)
        mc = C.byref(mismatch["_c"]) if mismatch is not None else None
        self._launch(dP.device, lambda st: self._lib.cmpc_rollout_tick_mismatch_device(self._h, lists[0].shape[2], float(now), 1 if warm else 0, io, int(tick),
                                                                                       mc, st))

    # ---- the walk on the device (include/cmpc.h, "a walk of the whole batch on the device") ----
    def walk_record(self, rows, stop=("merge", "solver", "nonfinite"), trace=True, device=None):
        """The arrays of a cmpc_walk_record as a dict of CUDA tensors (trace arrays only with trace=True) plus "_c", the C struct that points at them.
        stop: which tick codes end a problem, names of _capi.STOP_BITS ("merge" is always honoured).  The outcome is NOT set up: outcome_init_device."""
        import torch
        B = self.batch
        dev = self._dev(device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        r = dict(end_tick=z((B,), torch.int32), end_code=z((B,), torch.int32), iterations_sum=z((B,), torch.int32), iterations_max=z((B,), torch.int32),
                 final_state=z((B, 9), torch.float32), box_slack_min=z((B,), torch.float32), stats=z((rows, 6), torch.int32))
        if trace:
            r.update(com=z((rows, B, 3), torch.float32), zmp=z((rows, B, 2), torch.float32), land=z((rows, B, 2), torch.int32),
                     landing_offset=z((rows, B, 2, 3), torch.float64), iterations=z((rows, B), torch.int32), code=z((rows, B), torch.int32))
        mask = 0
        for name in stop:
            mask |= _capi.STOP_BITS[name]
        r["_c"] = _capi.CmpcWalkRecord(int(rows), mask, *(opt_ptr(r.get(k)) for k in (
            "com", "zmp", "land", "landing_offset", "iterations", "code", "end_tick", "end_code", "iterations_sum", "iterations_max", "final_state",
            "box_slack_min", "stats")))
        return r

    def walk_extremes_init_device(self, extremes=None, device=None):
        """cmpc_walk_extremes_init_device: extremes [B, 5] float32 (made when None) at its start -- +inf in the minima (height min, margin min), -inf in
        the maxima (height max, reach max, track max)."""
        import torch
        extremes = _args.out(extremes, torch.float32, (self.batch, _capi.WALK_EXTREMES), "extremes", self._dev(device))
        self._launch(extremes.device, lambda st: self._lib.cmpc_walk_extremes_init_device(self._h, extremes.data_ptr(), st))
        return extremes

    def outcome_init_device(self, dState0, rec):
        """cmpc_rollout_outcome_init_device: the outcome arrays of rec (walk_record) at their start, final_state = dState0[B, 9]."""
        import torch
        p0 = ptr(dState0, torch.float32, (self.batch, 9), "dState0", True)
        self._launch(dState0.device, lambda st: self._lib.cmpc_rollout_outcome_init_device(self._h, p0, rec["_c"], st))

    def rollout_record_device(self, tick, row, dX, dP, dInfo, ok, land, dStateOut, dZmp, rec):
        """cmpc_rollout_record_device: the record of one tick into row `row` of rec (walk_record) from what the tick left; ok / dZmp may be None."""
        self._launch(dX.device, lambda st: self._lib.cmpc_rollout_record_device(
            self._h, int(tick), int(row), dX.data_ptr(), dP.data_ptr(), dInfo.data_ptr(), opt_ptr(ok), land.data_ptr(), dStateOut.data_ptr(), opt_ptr(dZmp),
            rec["_c"], st))

    def cold_start_device(self, dP, dX0=None):
        """cmpc_cold_start_device: the cold start (CoM at com0, feet at nominal, f_z = g / 8 per corner) of dP[B, np] into dX0[B, nx]."""
        import torch
        L = self.layout
        pp = ptr(dP, torch.float32, (self.batch, L.np), "dP", True)
        dX0 = _args.out(dX0, torch.float32, (self.batch, L.nx), "dX0", dP.device)
        self._launch(dP.device, lambda st: self._lib.cmpc_cold_start_device(self._h, pp, dX0.data_ptr(), st))
        return dX0

    def walk_tape(self, rows, max_contacts, step=0.01, substeps=6, force_sample_time=False, first_row_is_first_tick=True, device=None):
        """The arrays of a cmpc_walk_tape (include/cmpc.h) as a dict of CUDA tensors stacked over `rows` ticks -- X, P, lam_g, info, states[rows + 1], ok,
        land, plan_t, list_t, plan_n, list_n -- plus the host scalars (step, substeps, force_sample_time) and "_c", the C struct that points at them."""
        import torch
        B, L, M = self.batch, self.layout, int(max_contacts)
        dev = self._dev(device)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        t = dict(X=z((rows, B, L.nx), f32), P=z((rows, B, L.np), f32), lam_g=z((rows, B, L.ng), f32), info=z((rows, B, _capi.INFO), f32),
                 states=z((rows + 1, B, 9), f32), ok=z((rows, B), i32), land=z((rows, B, 2), i32), plan_t=z((rows, B, 2, M, 2), f64),
                 list_t=z((rows, B, 2, M, 2), f64), plan_n=z((rows, B, 2), i32), list_n=z((rows, B, 2), i32))
        t["_c"] = _capi.CmpcWalkTape(int(rows), *(t[k].data_ptr() for k in ("X", "P", "lam_g", "info", "states", "ok", "land", "plan_t", "list_t", "plan_n",
                                                                            "list_n")), float(step), int(substeps), 1 if force_sample_time else 0,
                                     1 if first_row_is_first_tick else 0)
        t.update(rows=int(rows), max_contacts=M, step=float(step), substeps=int(substeps), force_sample_time=bool(force_sample_time))
        return t

    def rollout_tape_device(self, row, tape, dX, dP, dInfo, ok, land, dStateIn, dStateOut, plan, lists, parts=3):
        """cmpc_rollout_tape_device: row `row` of tape (walk_tape) from what a tick left.  parts 1: dStateIn -> states[row], BEFORE a tick that runs in place;
        2: everything else behind the tick (the multiplier output must be on); 3: both, behind a tick that did not run in place.  ok may be None (a first
        tick without force_sample_time), plan = (t, pose, n) or None on a first tick; lists = (t, pose, n) of the tick."""
        dev = (dStateIn if dStateIn is not None else dX).device
        tn = lambda three: (opt_ptr(three[0]), opt_ptr(three[2])) if three is not None else (None, None)
        self._launch(dev, lambda st: self._lib.cmpc_rollout_tape_device(
            self._h, int(tape["max_contacts"]), int(row), int(parts), *map(opt_ptr, (dX, dP, dInfo, ok, land, dStateIn, dStateOut)), *tn(plan), *tn(lists),
            tape["_c"], st))

    # ---- the state of a walk between two ticks (include/cmpc.h, cmpc_walk_snapshot) ----
    def walk_snapshot(self, tick, lists_in, max_contacts, batch=None, device=None, tensors=None):
        """The arrays of a cmpc_walk_snapshot (include/cmpc.h) as a dict of CUDA tensors -- state[B, 9], P, X, X0, info, zmp, ok[B], land[B, 2], lists = the
        two list sets [(t, pose, n), (t, pose, n)], and the outcome end_tick, end_code, iterations_sum, iterations_max, final_state, box_slack_min --
        plus tick, lists_in, max_contacts, batch and "_c", the C struct that points at them.  Zero-filled; batch: the snapshot's own (default: the
        handle's).  tensors: a dict with some of these keys -- those tensors are taken as they are and not allocated (a walk's live buffers described as
        a snapshot); X0, info or zmp given as None there are left out of the struct (NULL: skipped by the copy)."""
        import torch
        B, L, M = int(self.batch if batch is None else batch), self.layout, int(max_contacts)
        dev = self._dev(device)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        shapes = dict(state=((B, 9), f32), P=((B, L.np), f32), X=((B, L.nx), f32), X0=((B, L.nx), f32), info=((B, _capi.INFO), f32), zmp=((B, 2), f32),
                      ok=((B,), i32), land=((B, 2), i32), end_tick=((B,), i32), end_code=((B,), i32), iterations_sum=((B,), i32),
                      iterations_max=((B,), i32), final_state=((B, 9), f32), box_slack_min=((B,), f32))
        lshapes = (((B, 2, M, 2), f64), ((B, 2, M, 7), f32), ((B, 2), i32))
        given = dict(tensors or {})

        s = {}
        for k, (shape, dt) in shapes.items():
            if k in given:
                s[k] = given[k]
                ptr(s[k], dt, shape, f"walk_snapshot: {k}")
                if s[k] is None and k not in ("X0", "info", "zmp"):
                    raise AssertionError(f"walk_snapshot: {k} is required")
            else:
                s[k] = torch.zeros(shape, dtype=dt, device=dev)
        if "lists" in given:
            s["lists"] = [tuple(st[:3]) for st in given["lists"]]
            for st in s["lists"]:
                for a, (sh, dt) in zip(st, lshapes):
                    ptr(a, dt, sh, "walk_snapshot: lists", True)
            if len(s["lists"]) != 2:
                raise AssertionError("walk_snapshot: lists: expected two sets (t, pose, n)")
        else:
            s["lists"] = [tuple(torch.zeros(sh, dtype=dt, device=dev) for sh, dt in lshapes) for _ in range(2)]
        s["_c"] = _capi.CmpcWalkSnapshot(int(tick), int(lists_in), *(opt_ptr(s[k]) for k in ("state", "P", "X", "X0", "info", "zmp", "ok", "land")),
                                         *(a.data_ptr() for st in s["lists"] for a in st),
                                         *(opt_ptr(s[k]) for k in ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")))
        s.update(tick=int(tick), lists_in=int(lists_in), max_contacts=M, batch=B)
        return s

    def walk_snapshot_mark(self, snap, tick, lists_in):
        """the host words of a snapshot dict (walk_snapshot) and of its C struct"""
        snap["tick"] = snap["_c"].tick = int(tick)
        snap["lists_in"] = snap["_c"].lists_in = int(lists_in)

    def rollout_snapshot_device(self, src, dst, index=None, ok=None, src_batch=None):
        """cmpc_rollout_snapshot_device: ONE launch on torch's current stream, no host read: problem b of dst (walk_snapshot; the handle's batch) receives
        the bit copy of problem index[b] of src (index: int32 [B] CUDA tensor; None: problem b, and src must then hold the handle's batch).  An index
        outside [0, src_batch) leaves that problem of dst unwritten and gives ok[b] = 0 (ok: int32 [B], written when given).  src_batch: default
        src["batch"].  dst's host words tick and lists_in become src's.  Save and restore are the same call with the arguments swapped; repeated
        indices branch one problem into many."""
        import torch
        B = self.batch
        sb = int(src["batch"] if src_batch is None else src_batch)
        if not (src["max_contacts"] == dst["max_contacts"] and dst["batch"] == B and sb <= src["batch"]):
            raise AssertionError("rollout_snapshot_device: snapshots of other sizes")
        i = self._opt(index, torch.int32, (B,), "index")
        o = self._opt(ok, torch.int32, (B,), "ok")
        self._launch(dst["state"].device, lambda st: self._lib.cmpc_rollout_snapshot_device(
            self._h, int(src["max_contacts"]), sb, C.byref(src["_c"]), C.byref(dst["_c"]), i, o, st))
        self.walk_snapshot_mark(dst, src["tick"], src["lists_in"])
        return dst

    def walk_measures_vjp_device(self, tick0, ticks, tape, row0, end_tick, grad_measures, grad_states, grad_X, direct):
        """cmpc_walk_measures_vjp_device: the cotangents grad_measures[rows, B, 4] float64 of the stability measures of rows row0 .. row0 + ticks - 1 of
        tape (walk_tape) in ONE launch -> grad_states[rows + 1, B, 9] float64 and grad_X[rows, B, n_x] float32 ADDED TO (the reverse walk's seeds), and
        direct[rows, B, 32] float64 written (comRef_xy 2, omega [2][3], corner [2][4][3]).  The corners are the handle's or the installed models'.
        end_tick: int32 [B] (a walk record's) or None -- rows at or past a problem's end select zero and are not read."""
        import torch
        L, B, R = self.layout, self.batch, int(tape["rows"])
        f32, f64 = torch.float32, torch.float64
        g = _capi.CmpcWalkMeasureGrads(self._opt(grad_measures, f64, (R, B, _capi.WALK_MEASURES), "grad_measures"),
                                       self._opt(grad_states, f64, (R + 1, B, 9), "grad_states"), self._opt(grad_X, f32, (R, B, L.nx), "grad_X"),
                                       self._opt(direct, f64, (R, B, _capi.WALK_MEASURE_DIRECT), "direct"))
        e = self._opt(end_tick, torch.int32, (B,), "end_tick")
        self._launch(grad_measures.device,
                     lambda st: self._lib.cmpc_walk_measures_vjp_device(self._h, int(tick0), int(ticks), tape["_c"], int(row0), e, C.byref(g), st))

    def walk_measures_vjp_fold_device(self, direct, grad_p=None, grad_model=None):
        """cmpc_walk_measures_vjp_fold_device: behind the reverse walk, direct[rows, B, 32]'s comRef pair ADDED TO grad_p[rows, B, n_p] float32 (the
        reverse walk's grad_p) and its corner words summed over the rows into grad_model[B, 34] float64 (entries 10..33); either may be None."""
        import torch
        L, B, R = self.layout, self.batch, int(direct.shape[0])
        d = self._opt(direct, torch.float64, (R, B, _capi.WALK_MEASURE_DIRECT), "direct")
        gp = self._opt(grad_p, torch.float32, (R, B, L.np), "grad_p")
        gm = self._opt(grad_model, torch.float64, (B, _capi.MODEL_DOUBLES), "grad_model")
        self._launch(direct.device, lambda st: self._lib.cmpc_walk_measures_vjp_fold_device(self._h, R, d, gp, gm, st))

    def walk_measures_jvp_device(self, tick0, ticks, tape, row0, end_tick, k, dir_states, dir_x, dir_measures, dir_p=None, dir_model=None):
        """cmpc_walk_measures_jvp_device: the transpose of walk_measures_vjp_device in k columns, in rollout_walk_jvp_device's layouts: dir_states
        [rows + 1, B, k, 9] float64, dir_x[rows, B, k, n_x] float32, dir_p[rows, B, k, n_p] float32 or None (its knot-1 comRef xy only), dir_model
        [B, k, 34] float64 or None (its corners only) -> dir_measures[rows, B, k, 4] float64, written; rows at or past a problem's end are zero."""
        import torch
        L, B, R, k = self.layout, self.batch, int(tape["rows"]), int(k)
        f32, f64 = torch.float32, torch.float64
        d = _capi.CmpcWalkMeasureDirs(self._opt(dir_states, f64, (R + 1, B, k, 9), "dir_states"), self._opt(dir_x, f32, (R, B, k, L.nx), "dir_x"),
                                      self._opt(dir_p, f32, (R, B, k, L.np), "dir_p"), self._opt(dir_model, f64, (B, k, _capi.MODEL_DOUBLES), "dir_model"),
                                      self._opt(dir_measures, f64, (R, B, k, _capi.WALK_MEASURES), "dir_measures"))
        e = self._opt(end_tick, torch.int32, (B,), "end_tick")
        self._launch(dir_states.device,
                     lambda st: self._lib.cmpc_walk_measures_jvp_device(self._h, int(tick0), int(ticks), tape["_c"], int(row0), e, k, C.byref(d), st))

    def _walk_io(self, plan, lists, lists_b, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                 force_sample_time):
        """the cmpc_walk_io of a walk that runs in place on dState (include/cmpc.h): _tick_io's tick without previous lists, the second list set and the
        time of the planner trajectories' first knot"""
        io = _capi.CmpcWalkIO()
        io.tick = self._tick_io(plan, None, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dState, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                                force_sample_time)
        io.dListTB, io.dListPoseB, io.dListNB = (a.data_ptr() for a in lists_b)
        io.plan_t_first = float(planner[3]) if planner is not None else 0.0
        return io

    def rollout_walk_device(self, tick0, ticks, cold_first, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, row0=0,
                            wrench_ticks=None, dWrench=None, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False,
                            tape=None, tape_row0=None, mismatch=None):
        """cmpc_rollout_walk_device: `ticks` ticks from tick number tick0 queued in one call, each followed by its record (rec: walk_record, or None), in
        place on dState.  lists / lists_b: the two sets of list buffers (t, pose, n), lists_in the one that holds the previous tick's lists (the first
        tick's own with cold_first); returns the set that holds the last tick's.  wrench_ticks[T, B, N, 6]: tick i < T of the call writes row i.
        planner = (dComIn, dHIn, in_dt, t_first, robot_mass, com_height), t_first the time of the trajectories' first knot.
        tape (walk_tape): cmpc_rollout_walk_taped_device -- tick i of the call also writes row tape_row0 + i (default: row0 + i) of the tape; the
        multiplier output must be on.
        mismatch (plant_mismatch(...)): cmpc_rollout_walk_mismatch_device, taped or not -- tick tick0 + i runs under row tick0 + i - tick_first of its schedules."""
        io = self._walk_io(plan, lists, lists_b, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                           force_sample_time)
        if wrench_ticks is not None:
            import torch
            io.dWrenchTicks = ptr(wrench_ticks, torch.float32, (None, self.batch, self.cfg.N, 6), "wrench_ticks")
            io.wrench_ticks = int(wrench_ticks.shape[0])
        out = C.c_int(-1)
        if mismatch is not None:
            self._launch(dP.device, lambda st: self._lib.cmpc_rollout_walk_mismatch_device(
                self._h, lists[0].shape[2], int(tick0), int(ticks), 1 if cold_first else 0, C.byref(io), rec["_c"] if rec is not None else None, int(row0),
                int(lists_in), C.byref(out), tape["_c"] if tape is not None else None, int(row0 if tape_row0 is None else tape_row0) if tape is not None else 0,
                C.byref(mismatch["_c"]), st))
            return out.value
        if tape is not None:
            self._launch(dP.device, lambda st: self._lib.cmpc_rollout_walk_taped_device(
                self._h, lists[0].shape[2], int(tick0), int(ticks), 1 if cold_first else 0, C.byref(io), rec["_c"] if rec is not None else None, int(row0),
                int(lists_in), C.byref(out), tape["_c"], int(row0 if tape_row0 is None else tape_row0), st))
            return out.value
        self._launch(dP.device, lambda st: self._lib.cmpc_rollout_walk_device(
            self._h, lists[0].shape[2], int(tick0), int(ticks), 1 if cold_first else 0, C.byref(io), rec["_c"] if rec is not None else None, int(row0),
            int(lists_in), C.byref(out), st))
        return out.value

    # ---- sensed pushes (include/cmpc.h, cmpc_wrench_sensor; DESIGN.md 7f, "Sensed pushes").  Private: the public names are WalkingRollout's ----
    def _wrench_sensor(self, delay=0, hold_knots=1, deadband=0.7, noise=None, device=None):
        """A cmpc_wrench_sensor as a dict: noise[Tn, B, 6] float32 (numpy or a CUDA tensor; zero rows count as absent) is added to the reading of tick
        tick_first + r of the walk's mismatch.  The dict keeps the device tensor alive and holds "_c", the C struct that points at it."""
        import torch
        hold = []
        t = None
        if noise is not None:
            t = _upload(noise, self._dev(device), torch.float32, hold).contiguous()
            if t.dim() != 3 or tuple(t.shape[1:]) != (self.batch, 6):
                raise AssertionError(f"noise: expected [.., {(self.batch, 6)}]")
            t = t if t.numel() > 0 else None
        return dict(delay=int(delay), hold_knots=int(hold_knots), deadband=float(deadband), noise=t, _host=hold,
                    _c=_capi.CmpcWrenchSensor(int(delay), int(hold_knots), float(deadband), opt_ptr(t), 0 if t is None else int(t.shape[0])))

    def _wrench_sense_device(self, tick0, rows, mismatch, sensor, wrench_rows=True, passed=True):
        """cmpc_wrench_sense_device: rows tick0 .. tick0 + rows - 1 of the sensor's rule in one launch -> (wrench_rows[rows, B, N, 6] or None,
        plant_wrench[rows, B, 6] float32, pass[rows, B] int32 or None)"""
        import torch
        B, N, dev = self.batch, self.cfg.N, mismatch["hidden_wrench"].device
        wr = torch.empty((rows, B, N, 6), dtype=torch.float32, device=dev) if wrench_rows else None
        pl = torch.empty((rows, B, 6), dtype=torch.float32, device=dev)
        ps = torch.empty((rows, B), dtype=torch.int32, device=dev) if passed else None
        self._launch(dev, lambda st: self._lib.cmpc_wrench_sense_device(self._h, int(tick0), int(rows), C.byref(mismatch["_c"]), C.byref(sensor["_c"]),
                                                                        opt_ptr(wr), pl.data_ptr(), opt_ptr(ps), st), "cmpc_wrench_sense_device")
        return wr, pl, ps

    def _rollout_walk_sensed_device(self, sensor, plant_wrench, tick0, ticks, cold_first, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo,
                                    dZmp, rec, row0=0, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False,
                                    tape=None, tape_row0=None, mismatch=None):
        """cmpc_rollout_walk_sensed_device: rollout_walk_device(mismatch=...) with a sense launch in front of each tick (sensor: _wrench_sensor(...)); tick i
        of the call writes row i of plant_wrench[ticks.., B, 6] float32.  No wrench_ticks and no dWrench: the MPC's wrench is the sensed one."""
        import torch
        io = self._walk_io(plan, lists, lists_b, ok, land, dState, None, dP, dX0, dX, dInfo, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                           force_sample_time)
        out = C.c_int(-1)
        pw = ptr(plant_wrench, torch.float32, (None, self.batch, 6), "plant_wrench", required=True)
        if plant_wrench.shape[0] < ticks:
            raise AssertionError("plant_wrench: fewer rows than ticks")
        self._launch(dP.device, lambda st: self._lib.cmpc_rollout_walk_sensed_device(
            self._h, lists[0].shape[2], int(tick0), int(ticks), 1 if cold_first else 0, C.byref(io), rec["_c"] if rec is not None else None, int(row0),
            int(lists_in), C.byref(out), tape["_c"] if tape is not None else None, int(row0 if tape_row0 is None else tape_row0) if tape is not None else 0,
            C.byref(mismatch["_c"]) if mismatch is not None else None, C.byref(sensor["_c"]), pw, st), "cmpc_rollout_walk_sensed_device")
        return out.value

    # ---- refill: a queue of trials behind the slots of a walk (include/cmpc.h, cmpc_walk_refill) ----
    def _need_refill(self):
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_device")

    def walk_refill(self, state0, trial_ticks, wrench_trials=None, trace_rows=0, trace_tick_first=0, device=None, init=True):
        """The arrays of a cmpc_walk_refill as a dict of CUDA tensors plus "_c", the C struct that points at them: state0 [Q, 9] float32 (the queue, kept),
        wrench_trials [R, Q, N, 6] float32 or None, the slots' start_tick / trial [B], next [1], the per-trial outcome end_tick, end_code, iterations_sum,
        iterations_max, final_state, box_slack_min, ticks, slot, start [Q, ..], and trial_of [trace_rows, B] (trace_rows > 0; row r is tick trace_tick_first
        + r).  init: cmpc_rollout_refill_init_device is queued (every slot empty, no trial started)."""
        import torch
        self._need_refill()
        B = self.batch
        dev = self._dev(device)
        ptr(state0, torch.float32, (None, 9), "state0", True, "state0 [Q, 9] float32")
        Q = int(state0.shape[0])
        z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)
        r = dict(state0=state0, wrench_trials=wrench_trials, start_tick=z((B,)), trial=z((B,)), next=z((1,)), end_tick=z((Q,)), end_code=z((Q,)),
                 iterations_sum=z((Q,)), iterations_max=z((Q,)), final_state=z((Q, 9), torch.float32), box_slack_min=z((Q,), torch.float32), ticks=z((Q,)),
                 slot=z((Q,)), start=z((Q,)), trials=Q, trial_ticks=int(trial_ticks))
        if trace_rows > 0:
            r["trial_of"] = z((int(trace_rows), B))
        c = _capi.CmpcWalkRefill()
        c.trials, c.trial_ticks = Q, int(trial_ticks)
        c.dStartTick, c.dTrial, c.dNext, c.dState0 = r["start_tick"].data_ptr(), r["trial"].data_ptr(), r["next"].data_ptr(), state0.data_ptr()
        if wrench_trials is not None:
            c.dWrenchTrials = ptr(wrench_trials, torch.float32, (None, Q, self.cfg.N, 6), "wrench_trials", msg="wrench_trials [R, Q, N, 6] float32")
            c.wrench_ticks = int(wrench_trials.shape[0])
        for field, key in (("dTrialEndTick", "end_tick"), ("dTrialEndCode", "end_code"), ("dTrialIterationsSum", "iterations_sum"),
                           ("dTrialIterationsMax", "iterations_max"), ("dTrialFinalState", "final_state"), ("dTrialBoxSlackMin", "box_slack_min"),
                           ("dTrialTicks", "ticks"), ("dTrialSlot", "slot"), ("dTrialStart", "start")):
            setattr(c, field, r[key].data_ptr())
        if trace_rows > 0:
            c.trace = _capi.CmpcWalkRefillTrace(int(trace_rows), int(trace_tick_first), r["trial_of"].data_ptr())
        r["_c"] = c
        if init:
            self._launch(dev, lambda st: self._lib.cmpc_rollout_refill_init_device(self._h, C.byref(c), st))
        return r

    def rollout_refill_device(self, tick_next, rec, refill, dStateLive):
        """cmpc_rollout_refill_device: the refill in front of tick tick_next as ONE launch -- archive the occupied slots' outcome (rec: walk_record) into
        their trials' rows, then free slots take the queue's next trials in ascending slot order (refill: walk_refill).  dStateLive [B, 9] float32, the walk's
        state buffer; None: the archive pass only."""
        self._need_refill()
        import torch
        live = ptr(dStateLive, torch.float32, (self.batch, 9), "dStateLive")
        dev = refill["start_tick"].device
        self._launch(dev, lambda st: self._lib.cmpc_rollout_refill_device(self._h, int(tick_next), C.byref(rec["_c"]), C.byref(refill["_c"]), live, st))

    def walk_refill_trials(self, models=None, hidden_wrench=None, state_noise=None, force_gain=None, device=None):
        """A cmpc_walk_refill_trials as a dict: the per-TRIAL data of a refill walk over a queue of Q trials -- models [Q, 34] float64 (cmpc_model's order,
        config.model_array's rows), hidden_wrench [Th, Q, 6], state_noise [Tn, Q, 9], force_gain [Q] float32 (numpy or CUDA tensors, any subset; a schedule
        of zero rows counts as absent; the schedules' rows are the trial's LOCAL ticks).  With models the dict holds model_ok [Q] int32, -1 until the trial's
        first tick writes 1 or 0.  The dict keeps the device tensors alive and holds "_c", the C struct that points at them."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_trials_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_trials_device")
        dev = self._dev(device)
        hold = []

        def up(a, dtype, tail, name):
            if a is None:
                return None
            t = _upload(a, dev, dtype, hold).contiguous()    # (the host array is kept with the dict)
            if t.dim() != len(tail) or any(w is not None and int(t.shape[i]) != w for i, w in enumerate(tail)):
                raise AssertionError(f"{name}: expected {list(tail)}")
            return t if t.numel() > 0 else None
        r = dict(models=up(models, torch.float64, (None, _capi.MODEL_DOUBLES), "models"), hidden_wrench=up(hidden_wrench, torch.float32, (None, None, 6), "hidden_wrench"),
                 state_noise=up(state_noise, torch.float32, (None, None, 9), "state_noise"), force_gain=up(force_gain, torch.float32, (None,), "force_gain"))
        counts = {int(t.shape[0 if k in ("models", "force_gain") else 1]) for k, t in r.items() if t is not None}
        if len(counts) > 1:
            raise AssertionError(f"walk_refill_trials: the arrays disagree on the number of trials {sorted(counts)}")
        r["trials"] = counts.pop() if counts else None
        r["model_ok"] = torch.full((r["trials"],), -1, dtype=torch.int32, device=dev) if r["models"] is not None else None
        rows = lambda t: 0 if t is None else int(t.shape[0])
        r["_host"] = hold
        r["_c"] = _capi.CmpcWalkRefillTrials(opt_ptr(r["models"]), opt_ptr(r["model_ok"]), opt_ptr(r["hidden_wrench"]), rows(r["hidden_wrench"]),
                                             opt_ptr(r["state_noise"]), rows(r["state_noise"]), opt_ptr(r["force_gain"]))
        return r

    def rollout_walk_refill_device(self, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0=0,
                                   step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False, tape=None, tape_row0=0,
                                   trials=None):
        """cmpc_rollout_walk_refill_device: `ticks` ticks of a refill walk from tick number tick0 in one call -- per tick the refill launch, the tick's three
        launches and the record -- in place on dState; the other arguments as rollout_walk_device's (no cold_first, wrench_ticks or mismatch: a slot's
        first tick runs inside the merge launches, and the wrench schedule is refill's per-trial one).  Returns the set that holds the last tick's lists.
        trials (walk_refill_trials(...)): cmpc_rollout_walk_refill_trials_device -- per-trial models and a per-trial plant mismatch; with models the handle
        is left on its per-problem table, which then holds each slot's last trial's model (set_models[_device] afterwards to go on with one's own).
        tape (walk_tape(...)): cmpc_rollout_walk_refill_taped_device -- tick i of the call also writes row tape_row0 + i of the tape, SLOT-major (seven
        launches a tick; the multiplier output must be on); tape_regroup_device gathers a trial's rows out of it.  (tape and tape_row0 stand in front of
        trials: that the parameter list ends with trials is pinned.)"""
        return self._rollout_walk_refill("taped" if tape is not None else "trials" if trials is not None else "", tick0, ticks, plan, lists, lists_b, lists_in, ok,
                                         land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0, step, substeps, zmp_half_x, zmp_half_y, planner,
                                         force_sample_time, tape=tape, tape_row0=tape_row0, trials=trials)

    def _rollout_walk_refill(self, entry, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0=0,
                             step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False, tape=None, tape_row0=0,
                             trials=None, snapshot=None, plans=None):
        """The one call behind rollout_walk_refill_device, _snapshot_device and _plans_device: the cmpc_walk_io, the queue-length checks, and the C entry
        point cmpc_rollout_walk_refill_<entry>_device -- entry "plans", "snapshot", "taped", "trials" or "" (the plain one).  Each takes, of the
        optional structs trials, snapshot, plans and tape, the ones its argument list has (include/cmpc.h), NULL where None."""
        name = f"cmpc_rollout_walk_refill_{entry}{'_' if entry else ''}device"
        if not hasattr(self._lib, name):
            raise RuntimeError(f"this build of libcmpc_hip has no {name}")
        io = self._walk_io(plan, lists, lists_b, ok, land, dState, None, dP, dX0, dX, dInfo, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner, force_sample_time)
        for given, what in ((trials, "trials: the per-trial arrays"), (snapshot, "snapshot_of"), (plans, "plan_of")):
            if given is not None and given["trials"] not in (None, refill["trials"]):    # (None: trials without an array)
                raise AssertionError(f"{what} must have the queue's length")
        if snapshot is not None and snapshot["pool"]["max_contacts"] != lists[0].shape[2]:
            raise AssertionError("the pool's lists must have the walk's length")
        if snapshot is not None and snapshot["pool"]["_c"].tick != snapshot["tick"]:
            raise AssertionError("the pool was marked with another tick since walk_refill_snapshot")
        ref = lambda d: C.byref(d["_c"]) if d is not None else None
        out = C.c_int(-1)
        structs = {"": (), "trials": (ref(trials),), "taped": (ref(trials),), "snapshot": (ref(trials), ref(snapshot)), "plans": (ref(trials), ref(plans))}[entry]
        taped = (ref(tape), int(tape_row0)) if entry in ("taped", "plans") else ()
        self._launch(dP.device, lambda st: getattr(self._lib, name)(
            self._h, lists[0].shape[2], int(tick0), int(ticks), C.byref(io), ref(rec), ref(refill), *structs, int(row0), int(lists_in), C.byref(out), *taped, st))
        return out.value

    def walk_refill_snapshot(self, snapshot, snapshot_of, device=None):
        """A cmpc_walk_refill_snapshot as a dict: the pool -- snapshot, a walk_snapshot dict filled by rollout_snapshot_device (its tick >= 1 and lists_in
        as marked; any batch size) -- and snapshot_of [Q] int32 (numpy or CUDA), the pool row each trial of the queue starts from.  The dict holds
        snapshot_of on the device, snapshot_ok [Q] int32 (-1 until the trial's spawn writes 1 or 0), trials = Q, tick = the pool's, the pool itself (kept
        alive) and "_c", the C struct that points at them."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_snapshot_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_snapshot_device")
        dev = self._dev(device)
        hold = []
        idx = _upload(snapshot_of, dev, torch.int32, hold).contiguous()    # (the host array is kept with the dict)
        if idx.dim() != 1:
            raise AssertionError("snapshot_of: expected [Q]")
        Q = int(idx.shape[0])
        ok = torch.full((Q,), -1, dtype=torch.int32, device=dev)
        c = _capi.CmpcWalkRefillSnapshot(C.addressof(snapshot["_c"]), int(snapshot["batch"]), idx.data_ptr() if Q else None, ok.data_ptr() if Q else None)
        return dict(pool=snapshot, snapshot_of=idx, snapshot_ok=ok, trials=Q, tick=int(snapshot["tick"]), _host=hold, _c=c)

    def rollout_walk_refill_snapshot_device(self, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, snapshot,
                                            row0=0, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False,
                                            trials=None):
        """cmpc_rollout_walk_refill_snapshot_device: rollout_walk_refill_device with trials that start from a pool of saved problems (snapshot:
        walk_refill_snapshot(...); None: cmpc_rollout_walk_refill_trials_device through the new entry point).  Six launches per tick: the restore goes
        between the refill and the front kernel, and a slot spawned at tick s runs tick t at the pool's tick + (t - s).  (A method of its own: the parameter
        list of rollout_walk_refill_device is pinned.)"""
        return self._rollout_walk_refill("snapshot", tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0,
                                         step, substeps, zmp_half_x, zmp_half_y, planner, force_sample_time, trials=trials, snapshot=snapshot)

    def walk_refill_plans(self, pool, plan_of, plan, pool_refs=None, planner=None, device=None):
        """A cmpc_walk_refill_plans as a dict: pool = (t [Pn, 2, M, 2] float64, pose [Pn, 2, M, 7] float32, n [Pn, 2] int32), the pool of footstep plans
        in the layout of the planner's lists; plan_of [Q] int32 (numpy or CUDA), the pool row of each trial of the queue; plan = (t, pose, n) [B, ..], the
        slots' planner rows the walk is given -- WRITTEN by the walk: pass clones; pool_refs = (com, h) [Pn, n, 3] float32 or None, the planner
        trajectories of each plan, with planner = the (com, h, ...) tuple the walk is given (com / h [B, n, 3], written too).  The dict holds plan_of on the
        device, plan_ok [Q] int32 (-1 until the trial's spawn writes 1 or 0), trials = Q, pool_plans = Pn, the tensors (kept alive) and "_c"."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_plans_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_plans_device")
        dev = self._dev(device)
        hold = []
        up = lambda a, dtype: _upload(a, dev, dtype, hold).contiguous()    # (the host arrays are kept with the dict)
        pt, pp, pn = up(pool[0], torch.float64), up(pool[1], torch.float32), up(pool[2], torch.int32)
        Pn, M = int(pt.shape[0]), int(plan[0].shape[2])
        if not (Pn >= 1 and tuple(pt.shape) == (Pn, 2, M, 2) and tuple(pp.shape) == (Pn, 2, M, 7) and tuple(pn.shape) == (Pn, 2)):
            raise AssertionError(f"pool: (t [Pn, 2, {M}, 2], pose [Pn, 2, {M}, 7], n [Pn, 2])")
        for a, dt, shape in zip(plan, (torch.float64, torch.float32, torch.int32), ((2, M, 2), (2, M, 7), (2,))):
            ptr(a, dt, (self.batch,) + shape, "plan", True, "plan: the slots' (t, pose, n) on the device")
        idx = up(plan_of, torch.int32)
        if idx.dim() != 1:
            raise AssertionError("plan_of: expected [Q]")
        Q = int(idx.shape[0])
        ok = torch.full((Q,), -1, dtype=torch.int32, device=dev)
        c = _capi.CmpcWalkRefillPlans()
        c.pool_plans = Pn
        c.dPoolT, c.dPoolPose, c.dPoolN = pt.data_ptr(), pp.data_ptr(), pn.data_ptr()
        c.dTrialPlan, c.dTrialPlanOk = (idx.data_ptr(), ok.data_ptr()) if Q else (None, None)
        c.dPlanT, c.dPlanPose, c.dPlanN = (a.data_ptr() for a in plan)
        refs = None
        if pool_refs is not None:
            if planner is None:
                raise AssertionError("pool_refs need the walk's planner tuple (the slots' trajectories)")
            n = int(planner[0].shape[1])
            refs = (up(pool_refs[0], torch.float32), up(pool_refs[1], torch.float32))
            if not all(tuple(a.shape) == (Pn, n, 3) for a in refs):
                raise AssertionError(f"pool_refs: com and h [Pn, {n}, 3] (the knots of the slots' trajectories)")
            c.dPoolCom, c.dPoolH = refs[0].data_ptr(), refs[1].data_ptr()
            c.dPlanCom, c.dPlanH = (ptr(a, torch.float32, (self.batch, n, 3), name, True) for a, name in zip(planner[:2], ("planner com", "planner h")))
        return dict(pool=(pt, pp, pn), pool_refs=refs, plan_of=idx, plan_ok=ok, trials=Q, pool_plans=Pn, plan=plan, planner=planner, _host=hold, _c=c)

    def rollout_walk_refill_plans_device(self, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, plans,
                                         row0=0, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False,
                                         tape=None, tape_row0=0, trials=None):
        """cmpc_rollout_walk_refill_plans_device: rollout_walk_refill_device with a footstep plan (and planner trajectories) per TRIAL (plans:
        walk_refill_plans(...) over the same `plan` and `planner` tensors, which the walk WRITES; None: the taped / trials call through the new entry
        point).  One launch more per tick, the plan select, behind the refill: six, eight when taped.  (A method of its own: the parameter list of
        rollout_walk_refill_device is pinned.)"""
        return self._rollout_walk_refill("plans", tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0,
                                         step, substeps, zmp_half_x, zmp_half_y, planner, force_sample_time, tape=tape, tape_row0=tape_row0, trials=trials,
                                         plans=plans)

    def plan_fold_device(self, index, per_trial, pool_rows, out=None):
        """cmpc_rollout_plan_fold_device: out[p] = the sum of per_trial[q] over the trials with index[q] == p, in ascending q, without atomics (the bits do
        not depend on scheduling).  index [Q] int32, per_trial [Q, ..] float64 CUDA tensors -> out [pool_rows, ..] float64, written whole (zero for a row
        no trial has); an index outside the pool contributes nowhere."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_plan_fold_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_plan_fold_device")
        Q = int(per_trial.shape[0])
        tail = tuple(per_trial.shape[1:])
        words = int(np.prod(tail)) if tail else 1
        pt = ptr(per_trial, torch.float64, (Q,) + tail, "per_trial", True, "per_trial [Q, ..] float64")
        pi = ptr(index, torch.int32, (Q,), "index", True, "index [Q] int32")
        out = _args.out(out, torch.float64, (int(pool_rows),) + tail, "out", per_trial.device)
        self._launch(per_trial.device, lambda st: self._lib.cmpc_rollout_plan_fold_device(
            self._h, Q, words, pi if Q else None, pt if Q else None, int(pool_rows), out.data_ptr(), st))
        return out

    def tape_regroup_device(self, src_tape, refill, trial_index, dst_tape=None, tick_first=0):
        """cmpc_rollout_tape_regroup_device: ONE launch on torch's current stream, no host read -- column j of dst_tape (walk_tape of refill["trial_ticks"]
        rows with first_row_is_first_tick; None: allocated here with src_tape's scalars) receives the rows of trial trial_index[j] out of the slot-major
        src_tape of a taped refill walk (rollout_walk_refill_device(tape=...), whose row 0 holds tick tick_first), by the rule at cmpc_walk_tape_regroup in
        include/cmpc.h.  trial_index: int32 [B] CUDA tensor; an entry outside the queue: no trial.  refill: the walk's walk_refill dict, its archive pass
        (rollout_refill_device(ticks, rec, refill, None)) queued behind the last tick.
        -> (dst_tape, end_tick [B] int32 -- what the reverse and the forward walks take as end_tick -- and ok [B] int32, 0 where the column has no trial)."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_tape_regroup_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_tape_regroup_device")
        B, M = self.batch, int(src_tape["max_contacts"])
        dev = src_tape["X"].device
        pi = ptr(trial_index, torch.int32, (B,), "trial_index", True, "trial_index [B] int32")
        if dst_tape is None:
            dst_tape = self.walk_tape(int(refill["trial_ticks"]), M, step=src_tape["step"], substeps=src_tape["substeps"],
                                      force_sample_time=src_tape["force_sample_time"], first_row_is_first_tick=True, device=dev)
        if not (dst_tape["max_contacts"] == M and dst_tape["rows"] == int(refill["trial_ticks"])):
            raise AssertionError("dst_tape: trial_ticks rows of the same list length")
        end = torch.zeros((B,), dtype=torch.int32, device=dev)
        ok = torch.zeros((B,), dtype=torch.int32, device=dev)
        g = _capi.CmpcWalkTapeRegroup(int(tick_first), pi, end.data_ptr(), ok.data_ptr())
        self._launch(dev, lambda st: self._lib.cmpc_rollout_tape_regroup_device(self._h, M, C.byref(src_tape["_c"]), C.byref(refill["_c"]), C.byref(g),
                                                                                C.byref(dst_tape["_c"]), st))
        return dst_tape, end, ok

