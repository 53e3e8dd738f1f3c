"""The refill walks of WalkingRollout (a base class without state), the plan pools, the tape regrouped by trial and every trial's gradient.  The
refusals come before self is used for anything but M (their tests hand them a bare namespace): hence RefillWalks._walk_refill_trials(self, ...)."""
import numpy as np

from .contacts import pack_lists
from .rollout_common import need, plan_speed, refuse_long_lists, refuse_push_and_wrench_trials, seed

_SNAP_STAGE = " (a slot's first tick uses the front kernel's LDS stage; with force_sample_time the snap runs there too)"
_TRIAL_KWARGS = dict(push=None, push_ticks=0, wrench_trials=None, trace=True, stop=("merge", "solver", "nonfinite"))
_TICKS = "ticks >= 1 and trial_ticks >= 1"


def _trial_arguments(who, M, mismatch, kwargs, rows, why=" of a refill walk"):
    """the per-trial arguments of a refill walk, checked in one order -> (mismatch without its tick_first, kwargs over _TRIAL_KWARGS' defaults)"""
    mismatch = dict(mismatch or {})
    if int(mismatch.pop("tick_first", 0)) != 0:
        raise ValueError(f"{who}: the schedules' rows are {rows}, so tick_first must be 0")
    for k in [k for k in kwargs if k not in _TRIAL_KWARGS] + [k for k in mismatch if k not in ("hidden_wrench", "state_noise", "force_gain")]:
        raise TypeError(f"{who}: unexpected argument {k!r}")
    refuse_long_lists(who, M, why)
    args = dict(_TRIAL_KWARGS, **kwargs)
    refuse_push_and_wrench_trials(who, args["push"], args["wrench_trials"])
    return mismatch, args


class RefillWalks:
    def walk_device_refill(self, ticks, trial_ticks, com0, dcom0, h0, push=None, push_ticks=0, wrench_trials=None, trace=True,
                           stop=("merge", "solver", "nonfinite"), replan=None, mismatch=None, taped=False, every=None):
        """A queue of Q trials walked through the B slots of this roll-out in ONE walk of `ticks` ticks (cmpc_rollout_walk_refill_device, include/cmpc.h;
        DESIGN.md 7f "Refill"): every trial is a walk of trial_ticks ticks from its own initial state, and a slot takes the queue's next trial the tick after
        its robot ended (per `stop`) or finished, in ascending slot order.  No host read and no synchronisation inside; five launches per tick.
        com0 / dcom0 / h0 [Q, 3], numpy or CUDA; push [Q, 3] with run()'s schedule rule in the trial's LOCAL ticks (the push on the first max(push_ticks - i,
        1) knots of local tick i < push_ticks, zeros once at local tick push_ticks), or wrench_trials [R, Q, N, 6] float32 taken as it is (local tick r < R of
        trial q writes row [r, q]; later ticks leave the wrench rows alone); not both.  The references are the SLOT's (set_references, else the straight
        line) sized for trial_ticks and read at the trial's local time; the models are the slot's.  A trial runs at its local time and its first tick is a
        cold first tick inside the merge launches, so its bits are those of walk_device(trial_ticks, ...) on a roll-out of the same batch size and factor
        storage that holds it in the same slot.
        -> walk_device's slot-major dict (end_tick and the other outcome arrays are those of the slots' LAST trials, tick numbers local; a slot the queue
        left empty has end_tick >= 0), plus trial_of [ticks, B] int32 (the trial in each slot at each tick, -1: none) and trials: the per-trial outcome
        end_tick (-1 while walking or walked through), end_code, iterations_sum, iterations_max, final_state, box_slack_min, ticks (local ticks recorded),
        slot, start [Q, ..] (-1: never started), and trials["trace"](q) -> trial q's trace rows com, zmp, land, landing_offset, iterations, code
        [trial_ticks, ..] gathered out of the slot-major trace by one index_select each on the device, with valid [trial_ticks] bool (rows at or past
        trials["ticks"][q] are not the trial's).
        Per-trial models and a per-trial plant mismatch (hidden pushes, noise, a force gain): walk_device_refill_trials(), a method of its own because this
        signature is pinned; here the models are the slot's and mismatch= is refused.  Trials that start from a snapshot of a walk in progress instead of
        standing at tick 0 (warm from their first tick): walk_device_refill_from_snapshot().  A footstep plan and reference trajectories per trial
        instead of the slot's: walk_device_refill_plans().
        A tape behind every tick and every trial's gradient: walk_device_refill_taped() and backward_device_refill().
        Out of scope: gradients and forward mode through a refill walk of THIS method, and -- NotImplementedError, raised before anything touches a GPU -- replan,
        mismatch= (see above), taped=True, every (snapshots and checkpoints), and lists longer than 16 contacts."""
        for name, value in (("replan", replan), ("mismatch", mismatch), ("taped", taped or None), ("every", every)):
            if value is not None:
                raise NotImplementedError(f"walk_device_refill: {name} is out of scope of a refill walk")
        refuse_long_lists("walk_device_refill", self.M, _SNAP_STAGE)
        refuse_push_and_wrench_trials("walk_device_refill", push, wrench_trials)
        need(ticks >= 1 and trial_ticks >= 1, _TICKS)
        return self._queued(lambda: self._walk_refill(ticks, trial_ticks, com0, dcom0, h0, push, push_ticks, wrench_trials, trace, stop))

    def walk_device_refill_trials(self, ticks, trial_ticks, com0, dcom0, h0, models=None, mismatch=None, **kwargs):
        """walk_device_refill(ticks, trial_ticks, com0, dcom0, h0, **kwargs) with what a Monte-Carlo study randomises per TRIAL
        (cmpc_rollout_walk_refill_trials_device, include/cmpc.h; DESIGN.md 7f "Refill"): the robot and the disturbance.  kwargs: walk_device_refill's push,
        push_ticks, wrench_trials, trace and stop.
        models [Q, 34] float64, the rows of config.model_array (numpy or CUDA): trial q walks with model q -- the slot's record of the solver's per-problem
        table is rewritten on the device at the trial's first tick, bit-equal to what set_models_device would derive; a row that breaks the model rule ends
        its trial at local tick 0 with the solver's code (trials["model_ok"][q] = 0) and the slot goes to the next trial.
        mismatch = dict(hidden_wrench=[Th, Q, 6], state_noise=[Tn, Q, 9], force_gain=[Q]), any subset, float32: walk_device_mismatch's three parts with
        row = the trial's LOCAL tick and column = the trial; outside a schedule's rows the term is not applied.  A tick_first other than 0: ValueError.
        Still five launches per tick and no host read.  A trial's bits are those of walk_device_mismatch(trial_ticks, ..., tick_first=0) on a roll-out of
        the same batch size, factor storage and options that holds it in the same slot with models row `slot` = the trial's model and the schedules'
        column `slot` = the trial's rows.
        -> walk_device_refill's dict, plus trials["model_ok"] [Q] int32: 1 / 0 once the trial has started, -1 for a trial never started (and for every
        trial when models is None).  With models=None and nothing in mismatch: walk_device_refill, bit for bit.
        Afterwards the roll-out's own models are back (self.models through set_models_device, or none): a later walk_device on this object is bit-equal
        to one made before the call.  Out of scope, as for walk_device_refill: gradients, tapes, forward mode, snapshots, replan, lists longer than 16
        contacts (NotImplementedError).  The same walk with a tape behind every tick, for backward_device_refill(): walk_device_refill_taped()."""
        return RefillWalks._walk_refill_trials(self, "walk_device_refill_trials", False, ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs)

    def walk_device_refill_taped(self, ticks, trial_ticks, com0, dcom0, h0, models=None, mismatch=None, **kwargs):
        """walk_device_refill_trials(ticks, trial_ticks, com0, dcom0, h0, models, mismatch, **kwargs) through cmpc_rollout_walk_refill_taped_device
        (include/cmpc.h; DESIGN.md 7f "Refill, taped"): every tick also writes its row of a device tape, seven launches a tick, still no host read.  The
        multiplier output is turned on first, as walk_device_taped does (x and info are bit-identical with it on): every key walk_device_refill_trials
        returns is bit-equal to it.  The dict gains "tape": walk_device_taped's stacked tensors, `ticks` rows, SLOT-major -- column b of row t holds whatever
        trial sat in slot b at tick t -- plus what the reverse needs kept alive: refill (the queue's arrays), state0 [Q, 9], models [Q, 34] or None,
        mismatch (the per-trial schedules and gains), trial_ticks, dt, push_ticks.  backward_device() does not take this dict: refill_trial_walk() regroups
        up to B trials into a taped walk of their own, and backward_device_refill() does that for every trial of the queue.  (A method of its own:
        walk_device_refill's signature is pinned and its taped=True keeps raising.)  Out of scope: trials from a snapshot, replan, checkpoints, lists longer
        than 16 contacts (NotImplementedError)."""
        return RefillWalks._walk_refill_trials(self, "walk_device_refill_taped", True, ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs)

    def _walk_refill_trials(self, who, taped, ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs, plans=None):
        mismatch, args = _trial_arguments(who, self.M, mismatch, kwargs, "the trial's local ticks", _SNAP_STAGE)
        need(ticks >= 1 and trial_ticks >= 1, _TICKS)

        walk = lambda *a, **k: self._walk_refill(ticks, trial_ticks, com0, dcom0, h0, *a, tape=taped, plans=plans, **k)
        return self._queued(lambda: self._with_trial_data(models, mismatch, args, walk))

    def _with_trial_data(self, models, mismatch, args, walk):
        """walk(push, push_ticks, wrench_trials, trace, stop, trials=) under the per-trial data; behind it the own models are back and model_ok is set"""
        torch, s = self.torch, self.solver
        data = s.walk_refill_trials(models=models, device=self.dev, **mismatch)
        given = any(data[k] is not None for k in ("models", "hidden_wrench", "state_noise", "force_gain"))
        try:
            rec = walk(args["push"], args["push_ticks"], args["wrench_trials"], args["trace"], args["stop"], trials=data if given else None)
        finally:
            if data["models"] is not None:    # (the table holds each slot's last trial's model: back to the roll-out's own, in stream order)
                if self.models is not None:
                    s.set_models_device(self.models)
                else:
                    s.set_models(None)
        ok = data["model_ok"]
        Q = int(rec["trials"]["slot"].shape[0])
        rec["trials"]["model_ok"] = ok if ok is not None else torch.full((Q,), -1, dtype=torch.int32, device=self.dev)
        return rec

    # ---- a footstep plan and reference trajectories per trial (include/cmpc.h, cmpc_walk_refill_plans; DESIGN.md 7f, "Refill, plans per trial") ----
    _plan_speed = staticmethod(plan_speed)

    def plan_pool(self, plans):
        """A pool of footstep plans packed for walk_device_refill_plans: plans = a list of plan dicts as walking_plan returns them, or packed arrays
        (t [Pn, 2, m, 2], pose [Pn, 2, m, 7], n [Pn, 2]) with m <= M; -> numpy (t [Pn, 2, M, 2] float64, pose [Pn, 2, M, 7] float32, n [Pn, 2] int32),
        padded to the roll-out's M the way the roll-out pads its own plan (zero times, the identity pose), so a pool row built from the roll-out's plan
        has the bits of self.plan.  A plan with more than M - 1 contacts on a foot (the merged list holds the current contact besides the planner's
        future ones) is a ValueError.  No GPU is touched.  Packed CUDA tensors of the roll-out's M are returned as they are, without a host read: their
        counts are the caller's to keep at or below M - 1."""
        M = self.M
        if isinstance(plans, (list, tuple)) and len(plans) > 0 and isinstance(plans[0], dict):
            t, pose, n = pack_lists(self.cfg, list(plans))
        elif all(getattr(a, "is_cuda", False) for a in plans):    # (packed on the device already: taken as they are, no host read -- the counts are the caller's)
            if len(plans) != 3 or tuple(plans[0].shape[1:]) != (2, M, 2) or tuple(plans[1].shape[1:]) != (2, M, 7) or tuple(plans[2].shape[1:]) != (2,):
                raise ValueError(f"plans: device arrays must be padded to the roll-out's M = {M} already")
            return tuple(plans)
        else:
            host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
            t, pose, n = (host(a) for a in plans)
        t, pose, n = np.asarray(t, np.float64), np.asarray(pose, np.float32), np.asarray(n, np.int32)
        Pn, m = int(t.shape[0]), int(t.shape[2])
        if Pn < 1 or t.shape != (Pn, 2, m, 2) or pose.shape != (Pn, 2, m, 7) or n.shape != (Pn, 2):
            raise ValueError("plans: plan dicts, or (t [Pn, 2, m, 2], pose [Pn, 2, m, 7], n [Pn, 2]) with Pn >= 1")
        if int(n.max()) > M - 1:
            raise ValueError(f"plans: a plan with {int(n.max())} contacts on a foot, more than the roll-out's M - 1 = {M - 1}")
        k = min(m, M)
        tt = np.zeros((Pn, 2, M, 2)); pp = np.zeros((Pn, 2, M, 7), np.float32); pp[..., 3] = 1.0
        tt[:, :, :k] = t[:, :, :k]; pp[:, :, :k] = pose[:, :, :k]
        return tt, pp, np.ascontiguousarray(n)

    def plan_references(self, plans, trial_ticks):
        """The straight-line references of a pool of plan dicts, one row per plan at that plan's own mean speed, sized for trials of trial_ticks ticks: the
        very expression of _planner_refs, so row p has the bits of the default references of a roll-out constructed with plans[p].
        -> dict(com=[Pn, n, 3], h=[Pn, n, 3] float32 on the device, in_dt, t_first, robot_mass, com_height), walk_device_refill_plans' references=."""
        torch, N, dt, dev = self.torch, self.cfg.N, self.cfg.sampling_time, self.dev
        n_plan = trial_ticks + N + 2
        com = torch.zeros((len(plans), n_plan, 3), dtype=torch.float32, device=dev)
        for p, plan in enumerate(plans):
            com[p, :, 0] = (plan_speed(plan) * dt * torch.arange(n_plan, dtype=torch.float64, device=dev)).to(torch.float32)
        return dict(com=com, h=torch.zeros_like(com), in_dt=dt, t_first=0.0, robot_mass=1.0, com_height=0.7)

    def walk_device_refill_plans(self, ticks, trial_ticks, com0, dcom0, h0, plans, plan_of, references=None, models=None, mismatch=None, taped=False,
                                 **kwargs):
        """walk_device_refill_trials(ticks, trial_ticks, com0, dcom0, h0, models, mismatch, **kwargs) -- walk_device_refill_taped with taped=True -- with a
        FOOTSTEP PLAN AND REFERENCE TRAJECTORIES PER TRIAL (cmpc_rollout_walk_refill_plans_device, include/cmpc.h; DESIGN.md 7f "Refill, plans per
        trial"): which slot a trial lands in depends on who fell before it, so the slot's plan is nothing a study can choose; here trial q walks pool row
        plan_of[q].  One launch more per tick (the plan select, behind the refill: six, eight when taped), still no host read.
        plans: a list of plan dicts as walking_plan returns them, or packed arrays (plan_pool's argument), padded to the roll-out's M; a plan with more
        than M - 1 contacts is a ValueError.  plan_of [Q] int (numpy or CUDA); repeats are the normal case.  references: None keeps the SLOT's references
        as walk_device_refill does; else dict(com=[Pn, n, 3], h=[Pn, n, 3], in_dt, t_first, robot_mass, com_height) with set_references' meaning, row p
        going with plan p (plan_references() builds the straight lines at each plan's own mean speed).  kwargs: walk_device_refill_trials' push,
        push_ticks, wrench_trials, trace and stop; anything else is a TypeError.  plans=None: walk_device_refill_trials / walk_device_refill_taped.
        A trial's bits are those of walk_device_mismatch(trial_ticks, ..., tick_first=0) on a roll-out of the same batch size, factor storage and options
        that holds it in the same slot with that slot's plan (and references) the trial's pool row, models row `slot` the trial's model and the
        schedules' column `slot` the trial's rows.
        -> walk_device_refill_trials' dict (the taped one with taped=True) plus trials["plan"] [Q] int32 = plan_of and trials["plan_ok"] [Q] int32: 1 / 0
        once the trial has started (0: its index lay outside the pool -- nothing was copied, the trial is ended at spawn with end_tick 0 and end_code 0,
        and the slot goes to the next trial), -1 for a trial never started.  With taped=True the tape keeps plan_of and pool_plans, and
        backward_device_refill() returns plan_pool.  The slots' planner rows passed to the walk are clones: self.plan, self.references and the
        roll-out's models are what they were afterwards.
        Out of scope -- NotImplementedError, raised before anything touches a GPU: replan, every (snapshots and checkpoints), a snapshot (per-trial plans
        for trials from a snapshot would be a replan of a walk in progress), lists longer than 16 contacts."""
        who = "walk_device_refill_plans"
        for name in ("replan", "every", "snapshot"):
            if kwargs.get(name) is not None:
                raise NotImplementedError(f"{who}: {name} is out of scope of a refill walk with plans per trial")
            kwargs.pop(name, None)
        refuse_long_lists(who, self.M, " (a slot's first tick uses the front kernel's LDS stage)")
        if plans is None:
            if references is not None:
                raise ValueError(f"{who}: references go with plans")
            return RefillWalks._walk_refill_trials(self, who, bool(taped), ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs)
        pool = RefillWalks.plan_pool(self, plans)
        Pn = int(pool[0].shape[0])
        if references is not None:
            unknown = set(references) - {"com", "h", "in_dt", "t_first", "robot_mass", "com_height"}
            if unknown or "com" not in references or "h" not in references or "in_dt" not in references:
                raise ValueError(f"{who}: references = dict(com, h, in_dt, t_first=0.0, robot_mass=1.0, com_height=0.7)")
            if tuple(references["com"].shape) != tuple(references["h"].shape) or len(references["com"].shape) != 3 or \
                    int(references["com"].shape[0]) != Pn or int(references["com"].shape[1]) < 2 or int(references["com"].shape[2]) != 3:
                raise ValueError(f"{who}: references com and h of one shape [{Pn}, n >= 2, 3], a row per plan")
        given = dict(pool=pool, plan_of=plan_of, references=references)
        return RefillWalks._walk_refill_trials(self, who, bool(taped), ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs, plans=given)

    def walk_device_refill_from_snapshot(self, snapshot, ticks, trial_ticks, snapshot_of, models=None, mismatch=None, **kwargs):
        """A queue of Q = len(snapshot_of) trials that each START FROM A SNAPSHOT of a walk in progress, walked through the B slots of this roll-out in ONE
        walk of `ticks` ticks (cmpc_rollout_walk_refill_snapshot_device, include/cmpc.h; DESIGN.md 7f "Trials from a snapshot"): trial q is a fork of
        problem snapshot_of[q] of `snapshot` (a value of walk_device_checkpointed's "checkpoints", or any BatchSolver.walk_snapshot filled by
        rollout_snapshot_device, of any batch size; repeated rows are the normal case) and walks trial_ticks RESUMED ticks, t_s = snapshot["tick"] ..
        t_s + trial_ticks - 1, warm from its first one: there is no cold first tick.  A slot takes the queue's next trial the tick after its robot ended or
        finished, as in walk_device_refill; six launches per tick (the restore of the spawned slots goes between the refill and the front kernel), no host
        read, no synchronisation.  What walk_resume_device_mismatch(skip_ended=True) does for B robots per call, for a queue.
        models [Q, 34] and mismatch = dict(hidden_wrench=[Th, Q, 6], state_noise=[Tn, Q, 9], force_gain=[Q]): walk_device_refill_trials' per-trial data;
        their rows are the ticks SINCE SPAWN (row 0 is tick t_s of the trial), so a mismatch tick_first other than 0 is a ValueError.  kwargs:
        walk_device_refill_trials' push, push_ticks, wrench_trials (rows: ticks since spawn; without them the wrench rows of P stay what the snapshot
        holds), trace and stop; anything else is a TypeError.  A snapshot["wrench"] schedule that reaches t_s is not continued: NotImplementedError.  The
        references are the SLOT's, sized for t_s + trial_ticks and read at the whole-walk time.
        A trial's bits are those of walk_resume_device_mismatch(snapshot, trial_ticks, mismatch with tick_first = t_s, index = its row, skip_ended=True) on a
        roll-out of the same batch size, factor storage and options that holds it in the same slot, with models row `slot` the trial's model.
        -> walk_device_refill_trials' dict, with tick numbers of the whole walk in every end_tick, plus tick0 = t_s and trials["snapshot_ok"] [Q] int32:
        1 / 0 once the trial was spawned (0: its index lay outside the snapshot's batch -- nothing was copied, the trial is ended at spawn with end_tick
        t_s and end_code 0 and the slot goes to the next trial), -1 for a trial never started.  A trial whose snapshot row had already ended is ended at
        spawn too, with that row's outcome.  trials["ticks"] counts the resumed ticks the record saw of the trial: 0 for a trial ended at spawn (the
        C ABI's dTrialTicks holds 1 for it, the tick its slot was held).  Afterwards the roll-out's own models are back, as after
        walk_device_refill_trials.  Out of scope, as there: gradients, tapes, forward mode, replan, lists longer than 16 contacts (NotImplementedError)."""
        who = "walk_device_refill_from_snapshot"
        mismatch, args = _trial_arguments(who, self.M, mismatch, kwargs, "the ticks since the trial's spawn")
        t_s = int(snapshot["tick"])
        if t_s < 1:
            raise ValueError("walk_device_refill_from_snapshot: the snapshot must be of tick 1 or later (trials from tick 0: walk_device_refill_trials)")
        if snapshot.get("wrench") is not None and t_s - snapshot["wrench"][1] < snapshot["wrench"][0].shape[0]:
            raise NotImplementedError("walk_device_refill_from_snapshot: the snapshot's wrench schedule reaches its tick and is not continued by a refill "
                                      "walk (pass the rows as wrench_trials)")
        Q = len(snapshot_of)
        need(ticks >= 1 and trial_ticks >= 1, _TICKS)
        need(int(snapshot["max_contacts"]) == self.M, f"{who}: snapshot: expected max_contacts = {self.M}")

        def walk(*a, **k):
            pool = self.solver.walk_refill_snapshot(snapshot, snapshot_of, device=self.dev)
            z3 = self._z((Q, 3), self.torch.float32)    # (dState0: the restore overwrites what the refill launch copies from it)
            rec = self._walk_refill(ticks, trial_ticks, z3, z3, z3, *a, pool=pool, **k)
            rec["trials"]["snapshot_ok"] = pool["snapshot_ok"]
            return rec

        def spawned():
            rec = self._with_trial_data(models, mismatch, args, walk)
            t = rec["trials"]
            # a trial ended at spawn -- a bad index (code 0), or a row that had ended before the snapshot (end tick < t_s) -- was never seen walking by the record
            at_spawn = (t["end_tick"] >= 0) & ((t["end_tick"] < t_s) | (t["end_code"] == 0))
            t["ticks"].masked_fill_(at_spawn, 0)
            rec["tick0"] = t_s
            return rec
        return self._queued(spawned)

    def _walk_refill(self, ticks, trial_ticks, com0, dcom0, h0, push, push_ticks, wrench_trials, trace, stop, trials=None, pool=None, tape=False, plans=None):
        torch, B = self.torch, self.B
        need(not (tape and pool is not None), "trials that start from a snapshot are not taped")
        need(not (plans is not None and pool is not None), "trials that start from a snapshot keep their snapshot's lists")
        dt, dev, s = self.cfg.sampling_time, self.dev, self.solver
        self._walk_inputs, up = [], self._up
        z = lambda shape: self._z(shape, torch.float32)
        state0 = torch.cat([up(com0), up(dcom0), up(h0)], 1).contiguous()
        Q = int(state0.shape[0])
        if push is not None:    # (the schedule rule in the trial's local ticks)
            wrench_trials = self._push_schedule(up(push), push_ticks, Q)
        elif wrench_trials is not None:
            wrench_trials = up(wrench_trials).contiguous()
        refs = self._planner_refs(trial_ticks if pool is None else pool["tick"] + trial_ticks)
        plan_live, select = self.plan, None
        if plans is not None:    # (the select launch writes the slots' planner rows: clones, so that self.plan and self.references stay what they are)
            plan_live = tuple(a.clone() for a in self.plan)
            pool_refs, r = None, plans["references"]
            if r is not None:
                pool_refs = (r["com"], r["h"])
                n_ref = int(r["com"].shape[1])
                height = r.get("com_height", 0.7)
                refs = (z((B, n_ref, 3)), z((B, n_ref, 3)), float(r["in_dt"]), float(r.get("t_first", 0.0)), float(r.get("robot_mass", 1.0)),
                        float("nan") if height is None else float(height))
            select = s.walk_refill_plans(plans["pool"], plans["plan_of"], plan_live, pool_refs, planner=refs, device=dev)
            need(select["trials"] == Q, "plan_of must have the queue's length")
        rec = s.walk_record(ticks, stop=stop, trace=trace, device=dev)
        tp = self._walk_tape(ticks) if tape else None
        # the slots start empty; the set a slot's first tick writes at tick 0 is set 0, the one walk_device's first tick keeps the caller's lists in
        live = self._live_buffers(rec, z((B, 9)), self.plan)
        fill = s.walk_refill(state0, trial_ticks, wrench_trials, trace_rows=ticks, device=dev)
        sets = live["lists"]
        try:
            rec.update(self._limits_on(self.limits, ticks, trace, extremes=False))    # (a slot holds several trials: no extremes)
            # (ONE call: the public method of the struct that is given -- plans per trial: the select launch fills a spawned slot's planner rows in front
            #  of its first tick; trials from a snapshot: the restore launch fills a spawned slot's rows of both sets -- or the plain, trials or taped walk)
            walk, struct = ((s.rollout_walk_refill_plans_device, (select,)) if select is not None else
                            (s.rollout_walk_refill_snapshot_device, (pool,)) if pool is not None else (s.rollout_walk_refill_device, ()))
            cur = walk(0, ticks, plan_live, sets[0], sets[1], 1, live["ok"], live["land"], live["state"], live["P"], live["X0"], live["X"], live["info"],
                       live["zmp"], rec, fill, *struct, row0=0, step=dt / self.substeps, substeps=self.substeps, planner=refs,
                       force_sample_time=self.force_sample_time, trials=trials, **(dict(tape=tp, tape_row0=0) if tp is not None else {}))
        finally:
            self._limits_off(self.limits)
        s.walk_snapshot_mark(live, ticks, cur)
        s.rollout_refill_device(ticks, rec, fill, None)    # (the last tick's record ran behind its refill: one archive pass more)
        if tp is not None:    # (slot-major: refill_trial_walk regroups it by trial; the refill's arrays and the per-trial data stay alive with it)
            tp.update(trial_ticks=int(trial_ticks), refill=fill, state0=state0, models=None if trials is None else trials["models"],
                      mismatch=None if trials is None else {k: trials[k] for k in ("hidden_wrench", "state_noise", "force_gain")})
            if select is not None:
                tp.update(plan_of=select["plan_of"], pool_plans=select["pool_plans"])
        self._walk_finish(rec, live, tp, refs, push_ticks if push is not None else 0)
        trials = {k: fill[k] for k in ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min", "ticks", "slot", "start")}
        if trace:
            ar = torch.arange(trial_ticks, device=dev)

            def trial_trace(q):
                rows = (trials["start"][q].clamp(min=0) + ar).clamp(max=ticks - 1)
                idx = rows * B + trials["slot"][q].clamp(min=0)
                out = {k: rec[k].reshape((ticks * B,) + tuple(rec[k].shape[2:])).index_select(0, idx)
                       for k in ("com", "zmp", "land", "landing_offset", "iterations", "code", "measures") if k in rec}
                out["valid"] = ar < trials["ticks"][q]
                return out
            trials["trace"] = trial_trace
        if select is not None:
            trials.update(plan=select["plan_of"], plan_ok=select["plan_ok"])
        self._walk_refill_keep = (fill, refs, wrench_trials, trials, pool, select)    # (the queued launches read these)
        rec.update(trial_of=fill["trial_of"], trials=trials)
        return rec

    # ---- the refill walk's tape regrouped by trial (include/cmpc.h, cmpc_walk_tape_regroup; DESIGN.md 7f, "Refill, taped") ----
    def _refill_tape_of(self, who, w):
        """the slot-major tape of w = walk_device_refill_taped(...), or NotImplementedError -- raised before anything touches a GPU"""
        if "tick0" in w:
            raise NotImplementedError(f"{who}: trials that start from a snapshot are not taped (walk_device_refill_from_snapshot's dict)")
        tape = w.get("tape")
        if tape is None or "refill" not in tape:
            raise NotImplementedError(f"{who}: needs the dict of walk_device_refill_taped (a refill walk without a tape has nothing to regroup)")
        refuse_long_lists(who, self.M)
        return tape

    def refill_trial_walk(self, w, trials):
        """Up to B trials of w = walk_device_refill_taped(...) as a taped walk of their own: ONE launch (cmpc_rollout_tape_regroup_device) gathers trial
        trials[j]'s rows out of the slot-major tape into column j of a tape of trial_ticks rows -- row r the trial's local tick r, row 0 a cold first tick,
        rows past the trial's last recorded one repeating it.  trials: up to B trial numbers (a list, numpy or an int32 CUDA tensor; repeats allowed);
        fewer are padded with -1, a column without a trial.  No host read.
        -> a dict in the form of walk_device_taped's: tape (rows = trial_ticks, segments [0], push_ticks, dt, references, and -- when the walk ran under
        a per-trial mismatch -- mismatch: the trials' columns as a plant_mismatch with tick_first = 0), end_tick [B] int32 (the trial's own end tick; n for
        a trial the walk's end cut off after n ticks; 0 for a trial never started and for a pad column; -1 walked through), ok [B] int32 (0: a pad
        column) and trials [B] int32.  backward_device(view, ...) and forward_sensitivity_device_mismatch(view, ...) run on it as they are -- with the
        solver's models set to the trials' rows first when the walk had per-trial models, which backward_device_refill() does."""
        src = RefillWalks._refill_tape_of(self, "refill_trial_walk", w)    # (the refusals come before self is used for anything but its list length)
        torch, B, s = self.torch, self.B, self.solver
        if isinstance(trials, torch.Tensor):
            idx = trials.to(self.dev, torch.int32).reshape(-1)
        else:
            idx = torch.from_numpy(np.ascontiguousarray(np.asarray(trials, np.int64).reshape(-1), np.int32)).to(self.dev)
        need(idx.numel() <= B, f"refill_trial_walk: at most {B} trials per view")
        if idx.numel() < B:
            idx = torch.cat([idx, torch.full((B - idx.numel(),), -1, dtype=torch.int32, device=self.dev)])
        idx = idx.contiguous()

        def regroup():
            dst, end, ok = s.tape_regroup_device(src, src["refill"], idx)
            dst.update(dt=src["dt"], push_ticks=src["push_ticks"], segments=[0], references=src["references"])
            mm = src["mismatch"]
            if mm is not None and any(v is not None for v in mm.values()):
                Q = int(src["refill"]["trials"])
                col = idx.clamp(0, max(Q - 1, 0)).to(torch.int64)    # (a pad column takes some trial's rows: its end tick is 0, so nothing of them is read)
                pick = lambda t, dim: None if t is None else t.index_select(dim, col).contiguous()
                dst["mismatch"] = s.plant_mismatch(hidden_wrench=pick(mm["hidden_wrench"], 1), state_noise=pick(mm["state_noise"], 1),
                                                   force_gain=pick(mm["force_gain"], 0), tick_first=0, device=self.dev)
            return dict(tape=dst, end_tick=end, ok=ok, trials=idx)
        return self._queued(regroup)

    def backward_device_refill(self, w, grad_states, grad_X=None, rot=False, refs=False, replan=None):
        """Every trial's gradient of w = walk_device_refill_taped(...): the queue's trials in ascending order, B at a time, each group regrouped
        (refill_trial_walk) and run through backward_device()'s reverse walk; no host read and no synchronisation.
        grad_states [trial_ticks + 1, Q, 9] and grad_X [trial_ticks, Q, n_x] (or None): backward_device's seeds with the queue's Q for B, rows the trial's
        LOCAL ticks.  A trial that ended at local tick e, or that the walk's end cut off after e ticks, contributes its states 0 .. e and its solutions
        0 .. e - 1; the seeds of its later rows are not read, not even when they are not finite.  A trial never started returns state0 = grad_states[0]
        and zeros elsewhere.
        -> state0 [Q, 9], list0 [Q, 2, M, 3], wrench [trial_ticks, Q, N, 6], push [Q, 3], models [Q, 34], plan [Q, 2, M, 3], status [trial_ticks, Q],
        end_tick [Q] (the effective one: refill_trial_walk's), in backward_device's dtypes; under a per-trial mismatch also hidden_wrench
        [trial_ticks, Q, 6], state_noise [trial_ticks, Q, 9] and force_gain [Q].  Pad columns are dropped.  A trial's `plan` is the gradient with respect
        to the planner lists of the SLOT it walked in: sum it by w["trials"]["slot"] for the gradient of a slot's lists.
        On the tape of walk_device_refill_plans(taped=True) a trial's `plan` is the gradient with respect to ITS OWN plan row (the tape holds the trial's
        planner times and counts), and the dict gains plan_pool [Pn, 2, M, 3]: the sum of plan + list0 (the first tick's lists are the plan's) over the
        trials of each pool row, in ascending trial order and without atomics (cmpc_rollout_plan_fold_device); a row no trial named is zero, and a trial
        whose index lay outside the pool contributes nowhere.  With no plans on the tape the keys and their bits are what they were.
        With per-trial models the group's rows go through set_models_device first and the roll-out's own models are back afterwards, as after
        walk_device_refill_trials.  Every trial's keys are bit-equal to backward_device on a walk_device_taped of its own that holds it in any column
        with its model and its mismatch columns: the reverse kernels do not depend on the batch position.
        Out of scope -- NotImplementedError, raised before anything touches a GPU: rot=True and refs=True (the orientation and reference chains read
        per-slot data that a view does not regroup), replan, lists longer than 16 contacts, and a w of walk_device_refill_from_snapshot."""
        for name, value in (("rot", rot or None), ("refs", refs or None), ("replan", replan)):
            if value is not None:
                raise NotImplementedError(f"backward_device_refill: {name} is out of scope of a taped refill walk")
        src = RefillWalks._refill_tape_of(self, "backward_device_refill", w)
        torch, B, s, L = self.torch, self.B, self.solver, self.L
        TT, Q = int(src["trial_ticks"]), int(src["refill"]["trials"])
        gS = seed(grad_states, self.dev, torch.float64, (TT + 1, Q, 9), "grad_states")
        gX = None if grad_X is None else seed(grad_X, self.dev, torch.float32, (TT, Q, L.nx), "grad_X")
        batch_dim = dict(wrench=1, status=1, hidden_wrench=1, state_noise=1)    # (every other key has the batch in front)
        parts = []

        def pad(t):    # [rows, n, ..] -> [rows, B, ..] with zero seeds in the pad columns
            n = int(t.shape[1])
            return t if n == B else torch.cat([t, torch.zeros((t.shape[0], B - n) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)], 1).contiguous()
        try:
            for q0 in range(0, Q, B):
                q1 = min(q0 + B, Q)
                view = self.refill_trial_walk(w, list(range(q0, q1)))
                if src["models"] is not None:
                    rows = view["trials"].clamp(0, Q - 1).to(torch.int64)
                    self._queued(lambda: s.set_models_device(src["models"].index_select(0, rows).contiguous()))
                out = self._backward_device(view, pad(gS[:, q0:q1]), None if gX is None else pad(gX[:, q0:q1]), False)
                parts.append({k: v.narrow(batch_dim.get(k, 0), 0, q1 - q0) for k, v in out.items()})
        finally:
            if src["models"] is not None:    # (back to the roll-out's own, in stream order)
                if self.models is not None:
                    self._queued(lambda: s.set_models_device(self.models))
                else:
                    s.set_models(None)
        if not parts:
            raise ValueError("backward_device_refill: the queue is empty")
        out = {k: torch.cat([p[k] for p in parts], batch_dim.get(k, 0)) for k in parts[0]}
        if src.get("plan_of") is not None:    # (the pool's gradient: the fold over the trials that share a row, in ascending trial order)
            out["plan_pool"] = self._queued(lambda: s.plan_fold_device(src["plan_of"], (out["plan"] + out["list0"]).contiguous(), int(src["pool_plans"])))
        return out
