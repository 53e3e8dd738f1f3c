"""The device walks of WalkingRollout (a base class without state): walk_device and its mismatched, taped, checkpointed, sensed and resumed forms --
methods with pinned signatures in front of ONE driver each (_walk, _walk_resume) -- and what the drivers share (_walk_live, the live buffers)."""
from ._args import _upload
from .rollout_common import bound, need, refuse_push_with_sensor, walk_schedule


class DeviceWalks:
    def walk_device(self, ticks, com0, dcom0, h0, push=None, push_ticks=0, replan=None, trace=True, stop=("merge", "solver", "nonfinite"),
                    skip_ended=False):
        """The walk of run() queued on the device (cmpc_rollout_walk_device, include/cmpc.h): no host read and no synchronisation inside, the first tick
        started cold by a kernel, and every tick followed by the record kernel -- a problem whose merge fails (or, per `stop`, whose solve does not converge
        or whose state is not finite) ENDS on its own and the others walk on, where run() aborts the whole batch.
        skip_ended=False (the default): an ended problem stays in the launches, unobserved -- it holds its CU in every later solve, and its rows of state,
        X, P, info and lists are whatever the ticks behind its end made of them (final_state alone keeps the state after its last good tick).
        skip_ended=True: the record's end_tick is the handle's mask (cmpc_set_ended_device) around the queued segments, cleared again before the call
        returns (a later run() on this object is untouched): an ended problem is left out of every launch behind its ending tick, and its rows of state, X,
        P, info and of both list sets stay exactly what the ending tick left -- state is that tick's plant step from its (discarded) solve, one step past
        final_state (the list sets alternate from tick to tick, so an ended problem's rows of the returned `lists` are its ending tick's or the tick before's,
        as the parity of the remaining ticks has it).  The walking problems are bit-identical either way; still one call per segment, no host read, no synchronisation.
        com0 / dcom0 / h0 [B, 3] and push [B, 3]: numpy or CUDA tensors; replan {tick: (t, pose, n)} splits the walk into one call per
        segment (self.plan is left as it was); force_sample_time and models as in run(); not with retry="launch".
        -> dict of CUDA tensors, valid once the solver's launch stream has run (torch's current stream is made to wait for it): with trace=True the trace
        com[ticks, B, 3], zmp[ticks, B, 2], land[ticks, B, 2], landing_offset[ticks, B, 2, 3] (float64), iterations[ticks, B], code[ticks, B]; the outcome
        end_tick[B] (-1: walked to the end), end_code[B], iterations_sum[B], iterations_max[B], final_state[B, 9], box_slack_min[B]; stats[ticks, 6];
        lists (t, pose, n) of the last tick; X, P, info of the last tick; state[B, 9], the batch's state buffer after the last tick (ended problems
        included, unlike final_state).  The same walk with a device tape for backward_device(): walk_device_taped()."""
        return self._queued(lambda: self._walk(False, None, None, ticks, com0, dcom0, h0, push, push_ticks, replan, trace, stop, skip_ended))

    def walk_device_mismatch(self, ticks, com0, dcom0, h0, mismatch, **kwargs):
        """walk_device(ticks, com0, dcom0, h0, **kwargs) with a plant that is NOT the model (cmpc_rollout_walk_mismatch_device, include/cmpc.h):
        mismatch = dict(hidden_wrench=[Th, B, 6], state_noise=[Tn, B, 9], force_gain=[B], tick_first=0), any subset, numpy or CUDA float32 --
        hidden_wrench[r] is a mass-normalised force | torque the plant feels at tick tick_first + r and the MPC is never told about (push= is the wrench it
        IS told about), state_noise[r] is added to the state the MPC measures at that tick (the plant keeps the true one), force_gain scales every corner
        force the plant applies (a mass error: m_nominal / m_true).  Outside a schedule's rows the term is not applied.  Per problem; no launch more per
        tick, no host read.  The same with a tape: walk_device_taped(mismatch=...); checkpointed: walk_device_checkpointed(mismatch=...); from a snapshot:
        walk_resume_device_mismatch().  mismatch=None, or one with nothing set: walk_device, bit for bit.  (A method of its own and not an argument of
        walk_device: that signature is pinned.)"""
        args = bound(self.walk_device, ticks, com0, dcom0, h0, **kwargs)
        return self._queued(lambda: self._walk(False, None, None, *args.args, **args.kwargs, mismatch=mismatch))

    def walk_device_taped(self, ticks, com0, dcom0, h0, **kwargs):
        """walk_device(ticks, com0, dcom0, h0, **kwargs) through cmpc_rollout_walk_taped_device: every tick also writes its row of a device tape -- what
        backward_device() needs; about 12 KB per problem and tick at N = 20 -- and the dict gains "tape": the stacked tensors X, P, lam_g, info
        [ticks, B, ..], states[ticks + 1, B, 9] (row i the state tick i started from), ok, land, plan_t, list_t, plan_n, list_n, and dt, substeps,
        force_sample_time, push_ticks, segments (the first tick of each call), references (knots, dt, t_first, robot_mass, com_height of the planner's CoM /
        angular-momentum trajectories: set_references', else the straight line's).  The multiplier output is turned on first, as run(tape=True) does (x and info
        are bit-identical with it on): every other returned array is bit-identical to walk_device's.  Still no host read; works with replan and skip_ended
        (an ended problem's later rows then hold its ending tick's data).  (A method of its own and not an argument of walk_device: that signature is pinned.)
        mismatch= (walk_device_mismatch's argument): the walk runs under it, the tape keeps it alive in tape["mismatch"], and backward_device[_rot, _refs]
        then differentiate the mismatched plant and return three more keys."""
        mismatch = kwargs.pop("mismatch", None)
        args = bound(self.walk_device, ticks, com0, dcom0, h0, **kwargs)
        return self._queued(lambda: self._walk(True, None, None, *args.args, **args.kwargs, mismatch=mismatch))

    def walk_device_checkpointed(self, ticks, com0, dcom0, h0, every, **kwargs):
        """walk_device(ticks, com0, dcom0, h0, **kwargs) cut into calls at the multiples of `every` and at the replan ticks (walk_schedule), with ONE
        snapshot launch (cmpc_rollout_snapshot_device, include/cmpc.h) in front of each tick k * every, k >= 1.  -> walk_device's dict, bit-equal in
        every key, plus "checkpoints" {tick: snapshot} (BatchSolver.walk_snapshot: everything that tick reads of the ticks before it, about 13 KB per
        problem at N = 20) and "inputs", the small things a re-run needs, by reference: state0, the wrench schedule and push_ticks, the plans of replan
        and the plan in force at tick 0, the references, stop, skip_ended, ticks, every.  Like walk_device: no host read and no synchronisation.
        Continue or fork from a checkpoint: walk_resume_device().  The gradient without a whole-walk tape: backward_device_checkpointed()."""
        mismatch = kwargs.pop("mismatch", None)    # (walk_device_mismatch's argument; kept in "inputs" for backward_device_checkpointed_mismatch)
        args = bound(self.walk_device, ticks, com0, dcom0, h0, **kwargs)
        return self._queued(lambda: self._walk(False, int(every), None, *args.args, **args.kwargs, mismatch=mismatch))

    # ---- sensed pushes (include/cmpc.h, cmpc_wrench_sensor; DESIGN.md 7f, "Sensed pushes") ----
    def wrench_sensor(self, delay=0, hold_knots=1, deadband=0.7, noise=None):
        """A wrench sensor for walk_device_sensed, as a dict with the C struct and its tensors: the reading of tick t is the hidden wrench of tick t - delay
        plus noise[t - tick_first] ([Tn, B, 6] float32, numpy or CUDA; None: none), zeroed as a whole when its force is shorter than deadband (the
        reference's 0.7; 0: off; inf: a blind sensor), and handed to the MPC on knots 0 .. hold_knots - 1 of fExt / tauExt."""
        return self.solver._wrench_sensor(delay, hold_knots, deadband, noise, device=self.dev)

    def walk_device_sensed(self, ticks, com0, dcom0, h0, mismatch, sensor, tape=False, every=None, **kwargs):
        """walk_device_mismatch(ticks, com0, dcom0, h0, mismatch, **kwargs) with a wrench sensor between mismatch["hidden_wrench"] and the MPC
        (cmpc_rollout_walk_sensed_device): sensor = wrench_sensor(...).  ONE small launch in front of each tick turns the hidden schedule into the wrench
        rows the MPC sees (delayed, noisy, dead-banded, held for hold_knots knots) and the remainder only the plant feels; no host read.  The dict gains
        plant_wrench[ticks, B, 6] float32, that remainder.  tape=True: walk_device_taped's tape, which keeps mismatch, sensor and plant_wrench for
        backward_device_sensed() / forward_sensitivity_device_sensed().  every= (without a tape): walk_device_checkpointed's snapshots in front of the
        multiples of `every`, to resume from with walk_resume_device_sensed(); the checkpointed REVERSE of a sensed walk is refused (the delay couples
        rows across segments).  push= raises ValueError (the MPC's wrench is the sensed one).  sensor=None: walk_device_mismatch (tape=True:
        walk_device_taped(mismatch=...); every: walk_device_checkpointed(mismatch=...)), bit for bit, and no sensor key."""
        refuse_push_with_sensor(sensor, kwargs.get("push"))
        if tape and every is not None:
            raise ValueError("walk_device_sensed: tape=True or every=, not both")
        args = bound(self.walk_device, ticks, com0, dcom0, h0, **kwargs)
        return self._queued(lambda: self._walk(bool(tape), None if every is None else int(every), None, *args.args, **args.kwargs, mismatch=mismatch,
                                               sensor=sensor))

    def walk_resume_device_sensed(self, snapshot, ticks, mismatch, sensor, **kwargs):
        """walk_resume_device_mismatch(snapshot, ticks, mismatch, **kwargs) with a wrench sensor (walk_device_sensed's): one pilot walk, one snapshot,
        index = zeros, and B hidden pushes, each sensed.  Tick numbers are those of the whole walk, so a delay reaches across the cut: ticks 0 .. c - 1
        and a resume at c under the same mismatch and sensor equal the unbroken walk bit for bit.  The dict gains plant_wrench[ticks, B, 6] (row 0 = the
        resume tick).  push= raises ValueError, and so does a snapshot that carries a wrench schedule of its own."""
        refuse_push_with_sensor(sensor, kwargs.get("push"))
        args = bound(self.walk_resume_device, snapshot, ticks, **kwargs)
        return self._queued(lambda: self._walk_resume(*args.args, **args.kwargs, mismatch=mismatch, sensor=sensor))

    # ---- snapshots: resume and branch (include/cmpc.h, cmpc_walk_snapshot; DESIGN.md 7f, "Snapshots"); the reverse walk in bounded memory: rollout_grad.py ----
    def walk_resume_device(self, snapshot, ticks, index=None, push=None, push_ticks=0, replan=None, trace=True, stop=("merge", "solver", "nonfinite"),
                           skip_ended=False, taped=False, every=None):
        """Continues, or forks, a walk from a snapshot (a value of walk_device_checkpointed's "checkpoints", or any BatchSolver.walk_snapshot filled by
        rollout_snapshot_device): the snapshot is restored into fresh live buffers -- problem b of this roll-out receives problem index[b] of the
        snapshot (index: int32 [B], CUDA tensor or numpy; None: problem b) -- and ticks snapshot["tick"] .. snapshot["tick"] + ticks - 1 are walked warm
        (cold_first = 0), with no host read and no synchronisation.  -> walk_device's dict: the trace rows are those ticks only (row 0 = the resume
        tick), the outcome CONTINUES from the snapshot's (end_tick is a tick number of the whole walk), plus index_ok[B] (0: that index lay outside the
        snapshot's batch; the problem received nothing, its buffers keep their zero fill and it counts as ended from the start, end_tick 0 and end_code
        0), tick0, and "checkpoints" when `every` is given (snapshots in front of the multiples of `every` behind the resume tick).
        push[B, 3]: replaces the wrench schedule from the resume tick on; its rule is run()'s counted from that tick (the push on the first
        max(push_ticks - i, 1) knots of resume tick + i < push_ticks, zeros once behind).  Without it a checkpoint of walk_device_checkpointed goes on
        with its walk's schedule (gathered by index); any other snapshot leaves the wrench rows of P as they are.  replan {tick: plan}, tick numbers of
        the whole walk: the latest entry at or before a tick is the plan in force (none: self.plan) -- pass the source walk's replan to continue it.  The
        references are this roll-out's (set_references, else the straight line), long enough for the resumed ticks.
        index lets B problems fork from a snapshot of another batch size, many from one (splitting: the same robot under B different pushes).
        taped=True: "tape" as walk_device_taped's, of ticks + 1 rows: row 0 is a stub that holds the snapshot's list times and counts (the previous
        lists of the first resumed tick), row 1 + i is resume tick + i, first_row_is_first_tick = 0 (reverse it from row 1).
        Bit-equality with the unbroken walk is promised between handles of the same batch size and factor storage: the solver picks its kernel variant
        from them (the round-3 note on stragglers), and another variant rounds differently.  A queue of trials that each start from a
        snapshot, walked through the slots with ended robots replaced: walk_device_refill_from_snapshot().  Out of scope here: refilling the ended
        problems of THIS call -- a queue of trials behind the slots of a walk is walk_device_refill(), and from snapshots the method just named."""
        return self._queued(lambda: self._walk_resume(snapshot, ticks, index, push, push_ticks, replan, trace, stop, skip_ended, taped, every))

    def walk_resume_device_mismatch(self, snapshot, ticks, mismatch, **kwargs):
        """walk_resume_device(snapshot, ticks, **kwargs) under a plant mismatch (walk_device_mismatch's argument; tick_first is a tick number of the whole
        walk, so a push from the resume tick on has tick_first = snapshot["tick"]).  The headline use: one pilot walk, one snapshot, index = zeros, and B
        different hidden pushes -- the same mid-gait robot pushed B ways, none of which the MPC is told about.  Problem b is bit-equal to the unbroken walk
        of a batch whose problem b carries that mismatch.  taped=True: the tape keeps the mismatch in tape["mismatch"].  (A method of its own: the
        signature of walk_resume_device is pinned.)"""
        args = bound(self.walk_resume_device, snapshot, ticks, **kwargs)
        return self._queued(lambda: self._walk_resume(*args.args, **args.kwargs, mismatch=mismatch))

    def _walk(self, tape, every, states, ticks, com0, dcom0, h0, push, push_ticks, replan, trace, stop, skip_ended, mismatch=None, sensor=None):
        """walk_device and its mismatched, taped (tape) and checkpointed (every) forms: the start state in live buffers, the ticks queued by _walk_live.
        every None: walk_device's dict (with "tape": walk_device_taped's); else "checkpoints" and "inputs" besides.  states: _walk_live's."""
        torch, dev, s, up = self.torch, self.dev, self.solver, self._up
        mm = self._walk_mismatch = self._mismatch_of(mismatch)    # (kept until the next call: the queued launches read its tensors)
        sn = self._walk_sensor = self._sensor_of(sensor, mm, push)
        plant = torch.zeros((ticks, self.B, 6), dtype=torch.float32, device=dev) if sn is not None else None
        self._walk_inputs = []
        state0 = torch.cat([up(com0), up(dcom0), up(h0)], 1).contiguous()
        wrench = (self._push_schedule(up(push), push_ticks, self.B), 0) if push is not None else None
        # the planner's references as in run(): set_references', else a straight line at the plan's mean speed, a knot every dt from time zero
        refs = self._planner_refs(ticks)
        rec = s.walk_record(ticks, stop=stop, trace=trace, device=dev)
        tp = self._walk_tape(ticks) if tape else None
        plans = {int(t): p for t, p in dict(replan or {}).items() if 0 <= int(t) < ticks}
        # (the walk runs in place on its state: on state0 itself, or on a copy where "inputs" keeps state0 for a re-run)
        live = self._live_buffers(rec, state0 if every is None else state0.clone(), plans.get(0, self.plan))
        if states is not None:
            states[0].copy_(state0)
        cps = self._walk_live(live, 0, ticks, 0, plans, self.plan, wrench, refs, skip_ended, every=every, tape=tp, cold=True, states=states, mismatch=mm,
                              limits=self.limits, limits_out=rec, sensor=sn, plant=plant)
        if sn is not None:
            rec["plant_wrench"] = plant
        if every is not None:
            for c in cps.values():
                c["wrench"] = wrench
            rec.update(checkpoints=cps, inputs=dict(
                state0=state0, wrench=wrench, push_ticks=push_ticks if push is not None else 0, replan=plans, plan=self.plan, refs=refs, stop=tuple(stop),
                skip_ended=bool(skip_ended), ticks=int(ticks), every=every, mismatch=mm, limits=self.limits, **(dict(sensor=sn) if sn is not None else {})))
        return self._walk_finish(rec, live, tp, refs, push_ticks if push is not None else 0, mm, segments=[a for a, _ in walk_schedule(ticks, every, plans)[0]],
                                 **(dict(sensor=sn, plant_wrench=plant) if sn is not None else {}))

    def _walk_resume(self, snapshot, ticks, index, push, push_ticks, replan, trace, stop, skip_ended, taped, every, mismatch=None, sensor=None):
        torch, dev, s, B = self.torch, self.dev, self.solver, self.B
        mm = self._walk_mismatch = self._mismatch_of(mismatch)
        sn = self._walk_sensor = self._sensor_of(sensor, mm, push)
        plant = torch.zeros((ticks, B, 6), dtype=torch.float32, device=dev) if sn is not None else None
        self._walk_inputs = []
        t0 = int(snapshot["tick"])
        rec = s.walk_record(ticks, stop=stop, trace=trace, device=dev)
        live = self._live_buffers(rec)
        idx = None if index is None else self._up(index, torch.int32).contiguous()
        index_ok = torch.empty((B,), dtype=torch.int32, device=dev)
        s.rollout_snapshot_device(snapshot, live, idx, index_ok)
        wrench = None
        if push is not None:
            wrench = (self._push_schedule(self._up(push).contiguous(), push_ticks, B), t0)
        elif snapshot.get("wrench") is not None and t0 - snapshot["wrench"][1] < snapshot["wrench"][0].shape[0]:
            wt, first = snapshot["wrench"]
            if idx is not None:
                wt = wt.index_select(1, idx.clamp(0, int(snapshot["batch"]) - 1).to(torch.int64)).contiguous()
            wrench = (wt, first)
        if sn is not None and wrench is not None:
            raise ValueError("walk_resume_device_sensed: the snapshot carries a wrench schedule the MPC is told about; a known push and a sensed one are not summed")
        refs = self._planner_refs(t0 + ticks)
        plans = {int(t): p for t, p in dict(replan or {}).items() if 0 <= int(t) < t0 + ticks}
        tp = None
        if taped:
            tp = self._walk_tape(ticks + 1, first_row_is_first_tick=False)
            prev = live["lists"][live["lists_in"]]
            tp["list_t"][0].copy_(prev[0])
            tp["list_n"][0].copy_(prev[2])
        cps = self._walk_live(live, t0, t0 + ticks, t0, plans, self.plan, wrench, refs, skip_ended, every=every, tape=tp, tape_shift=t0 - 1, mismatch=mm,
                              limits=self.limits, limits_out=rec, sensor=sn, plant=plant)
        if every is not None:
            rec["checkpoints"] = cps
        rec.update(index_ok=index_ok, tick0=t0)
        if sn is not None:
            rec["plant_wrench"] = plant
            return self._walk_finish(rec, live, tp, mismatch=mm, tick0=t0, row0=1, sensor=sn, plant_wrench=plant)
        return self._walk_finish(rec, live, tp, mismatch=mm, tick0=t0, row0=1)    # (no push_ticks and no references on a resumed walk's tape)

    def _walk_live(self, live, t0, t1, row_shift, plans, base_plan, wrench, refs, skip_ended, every=None, tape=None, tape_shift=0, cold=False, states=None,
                   mismatch=None, limits=None, limits_out=None, sensor=None, plant=None):
        """Queues ticks t0 .. t1 - 1 on the live buffers (a snapshot dict whose "rec" is the walk record): one call of the C ABI per entry of
        walk_schedule, a snapshot launch in front of each tick k * every.  Record row = tick - row_shift, tape row = tick - tape_shift.  plans {tick:
        plan}: the latest entry at or before a tick is the plan in force (none: base_plan).  wrench = (wrench_ticks[T, B, N, 6], the tick of its row 0) or
        None.  states[.., B, 9]: the walk is cut at every tick and row tick + 1 - row_shift receives the state that tick left.  limits: set_limits'
        dict, on the handle around the calls; limits_out (a dict, or None: the codes alone) receives measures (with a trace in rec) and extremes.
        sensor (BatchSolver._wrench_sensor, with a mismatch that has a hidden schedule and no wrench): every call is cmpc_rollout_walk_sensed_device, and
        row tick - t0 of plant[t1 - t0, B, 6] receives what only the plant felt.
        -> {tick: snapshot}"""
        s, dt, rec = self.solver, self.cfg.sampling_time, live["rec"]
        calls, snaps = walk_schedule(t1 - t0, every, plans, t0)
        if states is not None:
            calls = [(t, t + 1) for t in range(t0, t1)]
        plan_at = lambda t: plans[max(k for k in plans if k <= t)] if any(k <= t for k in plans) else base_plan
        cur, out, sets = live["lists_in"], {}, live["lists"]
        if skip_ended:    # (the queued launches keep the pointer; the tensor outlives them in the walk's dict)
            s.set_ended_device(live["end_tick"])
        try:
            if limits_out is not None:
                limits_out.update(self._limits_on(limits, int(rec["stats"].shape[0]), "code" in rec))
            elif limits is not None:
                s.set_walk_limits(**limits)
            for a, b in calls:
                if a in snaps:
                    s.walk_snapshot_mark(live, a, cur)
                    out[a] = s.rollout_snapshot_device(live, s.walk_snapshot(a, cur, self.M, device=self.dev))
                wr = wrench[0][a - wrench[1]:] if wrench is not None and a - wrench[1] < wrench[0].shape[0] else None
                need(sensor is None or wr is None, "a known push and a sensed one are not summed")
                walk, more = (s.rollout_walk_device, dict(wrench_ticks=wr)) if sensor is None else (
                    lambda *args, **kw: s._rollout_walk_sensed_device(sensor, plant[a - t0:], *args, **kw), {})
                cur = walk(a, b - a, cold and a == t0, plan_at(a), sets[0], sets[1], cur, live["ok"], live["land"], live["state"], live["P"], live["X0"],
                           live["X"], live["info"], live["zmp"], rec, row0=a - row_shift, step=dt / self.substeps, substeps=self.substeps, planner=refs,
                           force_sample_time=self.force_sample_time, tape=tape, tape_row0=a - tape_shift, mismatch=mismatch, **more)
                if states is not None:
                    states[b - row_shift].copy_(live["state"])
        finally:
            self._limits_off(limits)
            if skip_ended:
                s.set_ended_device(None)
        s.walk_snapshot_mark(live, t1, cur)
        return out

    def _mismatch_of(self, mismatch):
        """mismatch (None, a dict of hidden_wrench / state_noise / force_gain / tick_first, or a BatchSolver.plant_mismatch dict) -> the solver's dict, or None
        when nothing is set (zero-length schedules count as absent): the walk is then the plain one, call for call"""
        if mismatch is None:
            return None
        m = mismatch if "_c" in mismatch else self.solver.plant_mismatch(device=self.dev, **mismatch)
        return None if all(m[k] is None for k in ("hidden_wrench", "state_noise", "force_gain")) else m

    @staticmethod
    def _sensor_of(sensor, mm, push):
        """the sensor of a walk (None: none), checked against the walk's other inputs before anything is queued"""
        if sensor is None:
            return None
        refuse_push_with_sensor(sensor, push)
        if mm is None or mm["hidden_wrench"] is None:
            raise ValueError("a sensor needs mismatch['hidden_wrench'], the schedule it reads")
        return sensor

    def _up(self, a, dtype=None):
        """a walk's input on the device (float32 unless dtype is given); the host array of a queued copy is kept in _walk_inputs until the next walk"""
        return _upload(a, self.dev, dtype or self.torch.float32, self._walk_inputs)

    def _walk_tape(self, rows, **kw):
        """a device tape of `rows` rows for a walk of this roll-out, the multiplier output on before anything is queued, as run(tape=True) does"""
        self.solver.set_multiplier_output(True)
        return self.solver.walk_tape(rows, self.M, step=self.cfg.sampling_time / self.substeps, substeps=self.substeps,
                                     force_sample_time=self.force_sample_time, device=self.dev, **kw)

    def _walk_finish(self, rec, live, tape=None, refs=None, push_ticks=0, mismatch=None, **entries):
        """The end every device walk shares: rec gives up its C struct and receives the live buffers of the last tick -- lists, X, P, info, state -- and
        the tape with its host entries: dt, `entries`, push_ticks and the references' timing (with refs), mismatch (when there is one)."""
        del rec["_c"]
        if tape is not None:
            tape.update(dt=self.cfg.sampling_time, **entries)
            if refs is not None:
                tape.update(push_ticks=push_ticks, references=dict(knots=int(refs[0].shape[1]), dt=refs[2], t_first=refs[3], robot_mass=refs[4], com_height=refs[5]))
            if mismatch is not None:
                tape["mismatch"] = mismatch
            rec["tape"] = tape
        rec.update(lists=live["lists"][live["lists_in"]], X=live["X"], P=live["P"], info=live["info"], state=live["state"])
        return rec

    def _live_buffers(self, rec, state0=None, plan0=None):
        """The live buffers of a walk described as a snapshot (BatchSolver.walk_snapshot); the outcome arrays are rec's.  Without state0: zero-filled, for
        a restore or _live_reset.  With state0 [B, 9] (taken as it is: the walk runs in place on it) and plan0: allocated as walk_device has them in
        front of tick 0 -- zeros, ok = 1, a copy of the plan in list set 0 -- and the outcome queued at its start: no fill a fresh walk does not need."""
        torch = self.torch
        given = {k: rec[k] for k in ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")}
        if state0 is not None:
            given.update(state=state0, ok=torch.ones((self.B,), dtype=torch.int32, device=self.dev),
                         lists=[tuple(a.clone() for a in plan0), tuple(torch.zeros_like(a) for a in plan0)])
        live = self.solver.walk_snapshot(0, 0, self.M, device=self.dev, tensors=given)
        live["rec"] = rec
        if state0 is not None:
            self.solver.outcome_init_device(state0, rec)
        return live

    def _live_reset(self, live, state0, plan0):
        """buffers that are used again (the checkpointed reverse's workspace) put back to what walk_device has in front of tick 0: zeros, ok = 1, the plan in
        list set 0, the outcome at its start"""
        for k in ("P", "X", "X0", "info", "zmp", "land"):
            live[k].zero_()
        live["ok"].fill_(1)
        live["state"].copy_(state0)
        for d, a in zip(live["lists"][0], plan0):
            d.copy_(a)
        for d in live["lists"][1]:
            d.zero_()
        self.solver.outcome_init_device(live["state"], live["rec"])
        self.solver.walk_snapshot_mark(live, 0, 0)

    def _push_schedule(self, dpush, push_ticks, columns):
        """run()'s schedule as rows of wrench_ticks: the push on the first max(push_ticks - i, 1) knots of row i < push_ticks, zeros once in row push_ticks;
        columns: B for a walk, the queue's Q for the trials of a refill walk (rows = the trial's local ticks)"""
        wt = self.torch.zeros((push_ticks + 1, columns, self.cfg.N, 6), dtype=self.torch.float32, device=self.dev)
        for i in range(push_ticks):
            wt[i, :, :max(push_ticks - i, 1), :3] = dpush[:, None, :]
        return wt
