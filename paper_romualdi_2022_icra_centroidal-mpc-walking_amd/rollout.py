"""Receding-horizon walking roll-out of a whole batch, resident in HBM: every tick is what the reference's two blocks do
between them -- merge the planner's footsteps with the MPC-adjusted current contact (updateContactPhaseList,
CentroidalMPCBlock.cpp:594-607), sample the list into the MPC's parameters (setContactPhaseList :609), feed the measured
state (setState :407), warm-start from the shifted previous solution (is_warm_start_enabled), solve (advance :615), write
the optimised landing position back into the list (getOutput :626) and integrate the centroidal dynamics under the
first-knot forces until the next tick (WholeBodyQPBlock.cpp:1083-1150) -- as seven launches on one stream through the
C ABI (include/cmpc.h); torch only owns the buffers.  SURVEY 8f-1 .. 8f-4 chained."""
from __future__ import annotations

import inspect

import numpy as np

from .config import GRAVITY

from .contacts import PlannedContact, pack_lists
from .layout import Layout
from .solver import BatchSolver, _model_array, _upload

FOOT_Y = 0.08


def walking_plan(cfg, steps=6, step_length=0.1, swing=0.48, double_support=0.12, first_lift=0.36):
    """A periodic straight walk (absolute times from zero): the left foot lifts first at `first_lift`."""
    names = [c.contact_name for c in cfg.contacts]
    feet = {0: [PlannedContact(0.0, 0.0, (0.0, FOOT_Y, 0.0))], 1: [PlannedContact(0.0, 0.0, (0.0, -FOOT_Y, 0.0))]}
    t, side = first_lift, 0
    for s in range(steps):
        other = feet[1 - side][-1]
        feet[side][-1].deactivation_time = t
        x = other.position[0] + step_length * (0.5 if s == 0 else 1.0)
        feet[side].append(PlannedContact(t + swing, 0.0, (x, FOOT_Y if side == 0 else -FOOT_Y, 0.0)))
        t += swing + double_support
        side = 1 - side
    for lst in feet.values():
        lst[-1].deactivation_time = 1e9
    return {names[0]: feet[0], names[1]: feet[1]}


def walk_schedule(ticks, every, replan=(), tick0=0):
    """The calls of a checkpointed walk of ticks tick0 .. tick0 + ticks - 1 -- a pure function.  The walk is cut at the multiples of `every` (tick numbers,
    not counted from tick0) and at the replan ticks that lie strictly inside it.  -> (calls, snapshots): calls = [(t0, t1), ...], half-open and in order;
    snapshots = the ticks k * every, k >= 1, strictly inside the walk: each is the first tick of a call, and the snapshot is taken in front of it.
    every None, or at or beyond the walk's end: no snapshot."""
    tick0, end = int(tick0), int(tick0) + int(ticks)
    assert ticks >= 1 and tick0 >= 0 and (every is None or int(every) >= 1), "walk_schedule: ticks >= 1, tick0 >= 0, every >= 1"
    snaps = [] if every is None else [t for t in range(int(every), end, int(every)) if t > tick0]
    cuts = sorted({tick0, end} | set(snaps) | {int(t) for t in replan if tick0 < int(t) < end})
    return list(zip(cuts[:-1], cuts[1:])), snaps


class WalkingRollout:
    """warm_budget / retry: what a warm-started problem that does not converge costs its tick (include/cmpc.h, cmpc_set_warm_policy).
    warm_budget = iterations of the warm-started pass (0: the full budget; 14 = the library's default); retry = "kernel": such a problem starts again from the cold
    start inside the same launch (one workgroup holds its CU for two budgets); "launch": it comes back unconverged and the tick's few
    stragglers are solved again from the cold start in a small launch of their own (a CU each); None: they stay unconverged -- which is all
    the reference can do: its advance() returns false and the tick is aborted (CentroidalMPCBlock.cpp:615-619).
    force_sample_time: every tick snaps the planner's lists to the MPC grid before the merge (forceSampleTime, CentroidalMPCBlock.cpp:586-592; the rule of
    include/cmpc.h), on both tick paths and after a replan; a list that fails to snap aborts the tick like a failed merge (rec["merge_ok"]).
    models: per-problem models (include/cmpc.h, cmpc_set_models) -- B configurations, a [B, 34] array (config.model_array), or a [B, 34] float64 CUDA
    tensor (set on the device: a row that breaks the model rule gives its problem status 3 every tick, self.models_ok[b] = 0).  The horizon, sampling
    time, contacts' bounding boxes and solver options stay cfg's.  retry="launch" solves the stragglers with their own models."""

    def __init__(self, cfg, batch, plan=None, device=0, substeps=6, com_speed=None, warm_budget=14, retry="kernel", retry_batch=256, native_tick=True,
                 force_sample_time=False, models=None, **solver_opts):
        import torch
        self.torch = torch
        self.cfg, self.B = cfg, batch
        self.L = Layout(cfg.N)
        self.dev = torch.device("cuda", device)
        self.solver = BatchSolver(cfg, batch, device=device, **solver_opts)
        assert retry in ("kernel", "launch", None)
        self.retry, self.retry_batch = retry, min(retry_batch, batch)
        # native_tick: a warm-started tick is ONE call of the C ABI (cmpc_rollout_tick_device: the same seven entry points chained inside the library, bit-identical
        # results) instead of seven; ticks that need the host between the steps (cold starts, retry="launch", the dump hook) take the step-by-step path
        self.native_tick = native_tick and retry != "launch"
        self.force_sample_time = bool(force_sample_time)
        self.solver.set_warm_policy(warm_budget, restart_in_kernel=(retry == "kernel"))
        self.solver2 = BatchSolver(cfg, self.retry_batch, device=device, **solver_opts) if retry == "launch" else None
        self.models, self.models_ok = None, None
        if models is not None:
            if isinstance(models, torch.Tensor) and models.is_cuda:
                self.models = models.to(self.dev, torch.float64).contiguous()
                self.models_ok = self.solver.set_models_device(self.models)
            else:
                self.solver.set_models(models)
                self.models = torch.from_numpy(_model_array(models, batch)).to(self.dev)
        plan = plan or walking_plan(cfg)
        t, pose, n = pack_lists(cfg, [plan])
        M = t.shape[2] + 1     # the merged list holds at most the current contact + the planner's future contacts
        tt = np.zeros((1, 2, M, 2)); pp = np.zeros((1, 2, M, 7), np.float32); pp[..., 3] = 1.0
        tt[:, :, :M - 1] = t; pp[:, :, :M - 1] = pose
        rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (batch,) + a.shape[1:]))).to(self.dev)
        self.plan = (rep(tt), rep(pp), rep(n))
        self.M = M
        self.substeps = substeps
        # mean walking speed of the plan, for the CoM reference
        if com_speed is None:
            last = max(c.position[0] for lst in plan.values() for c in lst)
            t_last = max(c.activation_time for lst in plan.values() for c in lst)
            com_speed = last / t_last if t_last > 0 else 0.0
        self.com_speed = com_speed
        self.references, self._ref_override = None, None
        self.limits = None

    def set_limits(self, height=(None, None), reach_max=None, margin_min=None, track_max=None):
        """The physical limits of the device walks (cmpc_set_walk_limits, include/cmpc.h): height = (lo, hi) on the CoM height above the supporting feet,
        reach_max on the CoM's distance from a supporting foot, margin_min on the capture point's signed distance to the support region (positive
        inside), track_max on the horizontal distance of the CoM from its reference; None (or NaN): that limit is off.  Sticky on the object: every
        device walk method (walk_device and its taped, mismatch, checkpointed and resumed forms, the refill walks) sets it on the handle around its
        queued segments and clears it again, as skip_ended does, records the tick codes 6..9, accepts "limits" in stop= (a robot beyond a limit ENDS),
        and returns measures[ticks, B, 4] (height, reach, margin, track per tick; with trace=True) and extremes[B, 5] (height min, height max, reach
        max, margin min, track max over each problem's good ticks; not from a refill walk, whose slots hold several trials: use measures and
        trial_of).  set_limits() with nothing given traces the measures and ends nobody.  clear_limits() restores the default, and with it every
        result's keys and bits.  run() is untouched."""
        lo, hi = height if height is not None else (None, None)
        self.limits = dict(height=(lo, hi), reach_max=reach_max, margin_min=margin_min, track_max=track_max)

    def clear_limits(self):
        """No physical limits (the default): the device walks record codes 0..5 only and return neither measures nor extremes."""
        self.limits = None

    def _limits_on(self, limits, rows, trace, extremes=True):
        """the handle's limits for the segments about to be queued -> the tensors the walk returns with them ({} without limits); _limits_off() behind them"""
        if limits is None:
            return {}
        torch, s = self.torch, self.solver
        out = {}
        if trace:
            out["measures"] = torch.zeros((rows, self.B, 4), dtype=torch.float32, device=self.dev)
        if extremes:
            out["extremes"] = s.walk_extremes_init_device(device=self.dev)
        s.set_walk_limits(measures=out.get("measures"), extremes=out.get("extremes"), **limits)
        return out

    def _limits_off(self, limits):
        if limits is not None:    # (the queued launches keep the struct they were queued with; the tensors go back to the caller and outlive them)
            self.solver.set_walk_limits(off=True)

    def set_references(self, com, h=None, in_dt=None, t_first=0.0, robot_mass=1.0, com_height=0.7):
        """The planner's CoM and angular-momentum trajectories (what the reference's MANN planner emits besides the footsteps), resampled into the comRef /
        hRef rows of p by every tick (cmpc_write_reference_from_planner_device; CentroidalMPCBlock.cpp:525-577): com / h [B, n, 3], numpy or CUDA tensors,
        kept as float32 CUDA tensors; a knot every in_dt seconds, knot 0 at time t_first; h is divided by robot_mass; the CoM height is replaced by
        com_height unless that is None or NaN.  Once set, run() (both tick paths) and walk_device[_taped]() pass these instead of the straight line at
        com_speed.  set_references(None) restores that default, and with it every result's bits.  Their gradient: backward_device_refs()."""
        torch = self.torch
        if com is None:
            self.references = None
            return
        assert h is not None and in_dt is not None and float(in_dt) > 0 and float(robot_mass) > 0, "set_references(com, h, in_dt, ...)"
        as32 = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32))).to(self.dev, torch.float32).contiguous()
        com, h = as32(com), as32(h)
        assert com.dim() == 3 and com.shape[0] == self.B and com.shape[1] >= 2 and com.shape[2] == 3 and h.shape == com.shape, \
            f"set_references: com and h of shape [{self.B}, n >= 2, 3]"
        self.references = dict(com=com, h=h, in_dt=float(in_dt), t_first=float(t_first), robot_mass=float(robot_mass),
                               com_height=float("nan") if com_height is None else float(com_height))

    def _planner_refs(self, ticks):
        """(com, h, in_dt, t_first, robot_mass, com_height) of a walk of `ticks` ticks: what set_references installed, else a straight line at the plan's mean
        speed and zero angular momentum, a knot every dt from time zero to the end of the last tick's horizon, the CoM height forced to 0.7 as the
        reference does (CentroidalMPCBlock.cpp:534).  _ref_override = (com, h) (rollout_differentiable's ref_com / ref_h; either None) replaces the
        trajectories for one call and keeps the timing, mass and height."""
        torch, B, N, dt, dev = self.torch, self.B, self.cfg.N, self.cfg.sampling_time, self.dev
        ov = self._ref_override or (None, None)
        if self.references is not None:
            r = self.references
            com, h, rest = r["com"], r["h"], (r["in_dt"], r["t_first"], r["robot_mass"], r["com_height"])
        else:
            n_plan = ticks + N + 2 if ov[0] is None and ov[1] is None else int((ov[0] if ov[0] is not None else ov[1]).shape[1])
            com = torch.zeros((B, n_plan, 3), dtype=torch.float32, device=dev)
            com[:, :, 0] = (self.com_speed * dt * torch.arange(n_plan, dtype=torch.float64, device=dev)).to(torch.float32)[None, :]
            h, rest = torch.zeros_like(com), (dt, 0.0, 1.0, 0.7)
        if ov[0] is not None:
            com = ov[0]
        if ov[1] is not None:
            h = ov[1]
        assert com.shape == h.shape and tuple(com.shape) == (B, com.shape[1], 3) and com.shape[1] >= 2, "reference trajectories: com and h of one shape [B, n, 3]"
        return (com, h) + rest

    def run(self, *args, **kwargs):
        """The roll-out (see _run for the arguments), with the solver's launch stream as torch's current stream: every device call of a tick -- the library's
        kernels and the torch ops between them -- is then queued on ONE non-default stream, in order, without the event dependencies a call from the default
        stream needs (BatchSolver._stream_pair: two per call, ~24 us of idle GPU each time)."""
        if kwargs.pop("mismatch", None) is not None:
            raise NotImplementedError("run(): a plant mismatch is taken by the device walk only (walk_device_mismatch, walk_device_taped(mismatch=...))")
        torch = self.torch
        ls = self.solver.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        try:
            with torch.cuda.stream(ls):
                return self._run(*args, **kwargs)
        finally:
            cur.wait_stream(ls)

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
        if self.M > 16:
            raise NotImplementedError("walk_device_refill: lists longer than 16 contacts are out of scope (a slot's first tick uses the front kernel's LDS "
                                      "stage; with force_sample_time the snap runs there too)")
        if push is not None and wrench_trials is not None:
            raise ValueError("walk_device_refill: push or wrench_trials, not both")
        assert ticks >= 1 and trial_ticks >= 1
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
        return WalkingRollout._walk_refill_trials(self, "walk_device_refill_trials", False, ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs)

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
        return WalkingRollout._walk_refill_trials(self, "walk_device_refill_taped", True, ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs)

    def _walk_refill_trials(self, who, taped, ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs, plans=None):
        mismatch = dict(mismatch or {})
        if int(mismatch.pop("tick_first", 0)) != 0:
            raise ValueError(f"{who}: the schedules' rows are the trial's local ticks, so tick_first must be 0")
        for given, known in ((kwargs, ("push", "push_ticks", "wrench_trials", "trace", "stop")), (mismatch, ("hidden_wrench", "state_noise", "force_gain"))):
            for k in given:
                if k not in known:
                    raise TypeError(f"{who}: unexpected argument {k!r}")
        if self.M > 16:
            raise NotImplementedError(f"{who}: lists longer than 16 contacts are out of scope (a slot's first tick uses the front kernel's "
                                      "LDS stage; with force_sample_time the snap runs there too)")
        args = dict(push=None, push_ticks=0, wrench_trials=None, trace=True, stop=("merge", "solver", "nonfinite"))
        args.update(kwargs)
        if args["push"] is not None and args["wrench_trials"] is not None:
            raise ValueError(f"{who}: push or wrench_trials, not both")
        assert ticks >= 1 and trial_ticks >= 1

        def walk():
            torch, s = self.torch, self.solver
            data = s.walk_refill_trials(models=models, device=self.dev, **mismatch)
            given = any(data[k] is not None for k in ("models", "hidden_wrench", "state_noise", "force_gain"))
            try:
                rec = self._walk_refill(ticks, trial_ticks, com0, dcom0, h0, args["push"], args["push_ticks"], args["wrench_trials"], args["trace"],
                                        args["stop"], trials=data if given else None, tape=taped, plans=plans)
            finally:
                if data["models"] is not None:    # (the table holds each slot's last trial's model: back to the roll-out's own, in stream order)
                    if self.models is not None:
                        s.set_models_device(self.models)
                    else:
                        s.set_models(None)
            Q = int(rec["trials"]["slot"].shape[0])
            ok = data["model_ok"]
            rec["trials"]["model_ok"] = ok if ok is not None else torch.full((Q,), -1, dtype=torch.int32, device=self.dev)
            return rec
        return self._queued(walk)

    # ---- a footstep plan and reference trajectories per trial (include/cmpc.h, cmpc_walk_refill_plans; DESIGN.md 7f, "Refill, plans per trial") ----
    @staticmethod
    def _plan_speed(plan):
        """the mean walking speed of a plan: the expression of __init__ (com_speed=None)"""
        last = max(c.position[0] for lst in plan.values() for c in lst)
        t_last = max(c.activation_time for lst in plan.values() for c in lst)
        return last / t_last if t_last > 0 else 0.0

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
            com[p, :, 0] = (WalkingRollout._plan_speed(plan) * dt * torch.arange(n_plan, dtype=torch.float64, device=dev)).to(torch.float32)
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
        if self.M > 16:
            raise NotImplementedError(f"{who}: lists longer than 16 contacts are out of scope (a slot's first tick uses the front kernel's LDS stage)")
        if plans is None:
            if references is not None:
                raise ValueError(f"{who}: references go with plans")
            return WalkingRollout._walk_refill_trials(self, who, bool(taped), ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs)
        pool = WalkingRollout.plan_pool(self, plans)
        Pn = int(pool[0].shape[0])
        if references is not None:
            unknown = set(references) - {"com", "h", "in_dt", "t_first", "robot_mass", "com_height"}
            if unknown or "com" not in references or "h" not in references or "in_dt" not in references:
                raise ValueError(f"{who}: references = dict(com, h, in_dt, t_first=0.0, robot_mass=1.0, com_height=0.7)")
            if tuple(references["com"].shape) != tuple(references["h"].shape) or len(references["com"].shape) != 3 or \
                    int(references["com"].shape[0]) != Pn or int(references["com"].shape[1]) < 2 or int(references["com"].shape[2]) != 3:
                raise ValueError(f"{who}: references com and h of one shape [{Pn}, n >= 2, 3], a row per plan")
        given = dict(pool=pool, plan_of=plan_of, references=references)
        return WalkingRollout._walk_refill_trials(self, who, bool(taped), ticks, trial_ticks, com0, dcom0, h0, models, mismatch, kwargs, plans=given)

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
        mismatch = dict(mismatch or {})
        if int(mismatch.pop("tick_first", 0)) != 0:
            raise ValueError("walk_device_refill_from_snapshot: the schedules' rows are the ticks since the trial's spawn, so tick_first must be 0")
        for given, known in ((kwargs, ("push", "push_ticks", "wrench_trials", "trace", "stop")), (mismatch, ("hidden_wrench", "state_noise", "force_gain"))):
            for k in given:
                if k not in known:
                    raise TypeError(f"walk_device_refill_from_snapshot: unexpected argument {k!r}")
        if self.M > 16:
            raise NotImplementedError("walk_device_refill_from_snapshot: lists longer than 16 contacts are out of scope of a refill walk")
        args = dict(push=None, push_ticks=0, wrench_trials=None, trace=True, stop=("merge", "solver", "nonfinite"))
        args.update(kwargs)
        if args["push"] is not None and args["wrench_trials"] is not None:
            raise ValueError("walk_device_refill_from_snapshot: push or wrench_trials, not both")
        t_s = int(snapshot["tick"])
        if t_s < 1:
            raise ValueError("walk_device_refill_from_snapshot: the snapshot must be of tick 1 or later (trials from tick 0: walk_device_refill_trials)")
        if snapshot.get("wrench") is not None and t_s - snapshot["wrench"][1] < snapshot["wrench"][0].shape[0]:
            raise NotImplementedError("walk_device_refill_from_snapshot: the snapshot's wrench schedule reaches its tick and is not continued by a refill "
                                      "walk (pass the rows as wrench_trials)")
        Q = len(snapshot_of)
        assert ticks >= 1 and trial_ticks >= 1 and int(snapshot["max_contacts"]) == self.M

        def walk():
            torch, s = self.torch, self.solver
            data = s.walk_refill_trials(models=models, device=self.dev, **mismatch)
            given = any(data[k] is not None for k in ("models", "hidden_wrench", "state_noise", "force_gain"))
            pool = s.walk_refill_snapshot(snapshot, snapshot_of, device=self.dev)
            z3 = torch.zeros((Q, 3), dtype=torch.float32, device=self.dev)    # (dState0: the restore overwrites what the refill launch copies from it)
            try:
                rec = self._walk_refill(ticks, trial_ticks, z3, z3, z3, args["push"], args["push_ticks"], args["wrench_trials"], args["trace"],
                                        args["stop"], trials=data if given else None, pool=pool)
            finally:
                if data["models"] is not None:    # (the table holds each slot's last trial's model: back to the roll-out's own, in stream order)
                    if self.models is not None:
                        s.set_models_device(self.models)
                    else:
                        s.set_models(None)
            t = rec["trials"]
            ok = data["model_ok"]
            t["model_ok"] = ok if ok is not None else torch.full((Q,), -1, dtype=torch.int32, device=self.dev)
            t["snapshot_ok"] = pool["snapshot_ok"]
            # a trial ended at spawn -- a bad index (code 0), or a row that had ended before the snapshot (end tick < t_s) -- was never seen walking by the record
            at_spawn = (t["end_tick"] >= 0) & ((t["end_tick"] < t_s) | (t["end_code"] == 0))
            t["ticks"].masked_fill_(at_spawn, 0)
            rec["tick0"] = t_s
            return rec
        return self._queued(walk)

    def _walk_refill(self, ticks, trial_ticks, com0, dcom0, h0, push, push_ticks, wrench_trials, trace, stop, trials=None, pool=None, tape=False, plans=None):
        torch, B = self.torch, self.B
        assert not (tape and pool is not None), "trials that start from a snapshot are not taped"
        assert not (plans is not None and pool is not None), "trials that start from a snapshot keep their snapshot's lists"
        dt, dev, s = self.cfg.sampling_time, self.dev, self.solver
        self._walk_inputs, up = [], self._up
        z = lambda shape: torch.zeros(shape, dtype=torch.float32, device=dev)
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
            assert select["trials"] == Q, "plan_of must have the queue's length"
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

    def _mismatch_of(self, mismatch):
        """mismatch (None, a dict of hidden_wrench / state_noise / force_gain / tick_first, or a BatchSolver.plant_mismatch dict) -> the solver's dict, or None
        when nothing is set (zero-length schedules count as absent): the walk is then the plain one, call for call"""
        if mismatch is None:
            return None
        m = mismatch if "_c" in mismatch else self.solver.plant_mismatch(device=self.dev, **mismatch)
        return None if all(m[k] is None for k in ("hidden_wrench", "state_noise", "force_gain")) else m

    def walk_device_mismatch(self, ticks, com0, dcom0, h0, mismatch, **kwargs):
        """walk_device(ticks, com0, dcom0, h0, **kwargs) with a plant that is NOT the model (cmpc_rollout_walk_mismatch_device, include/cmpc.h):
        mismatch = dict(hidden_wrench=[Th, B, 6], state_noise=[Tn, B, 9], force_gain=[B], tick_first=0), any subset, numpy or CUDA float32 --
        hidden_wrench[r] is a mass-normalised force | torque the plant feels at tick tick_first + r and the MPC is never told about (push= is the wrench it
        IS told about), state_noise[r] is added to the state the MPC measures at that tick (the plant keeps the true one), force_gain scales every corner
        force the plant applies (a mass error: m_nominal / m_true).  Outside a schedule's rows the term is not applied.  Per problem; no launch more per
        tick, no host read.  The same with a tape: walk_device_taped(mismatch=...); checkpointed: walk_device_checkpointed(mismatch=...); from a snapshot:
        walk_resume_device_mismatch().  mismatch=None, or one with nothing set: walk_device, bit for bit.  (A method of its own and not an argument of
        walk_device: that signature is pinned.)"""
        args = inspect.signature(self.walk_device).bind(ticks, com0, dcom0, h0, **kwargs)
        args.apply_defaults()
        return self._queued(lambda: self._walk(False, None, None, *args.args, **args.kwargs, mismatch=mismatch))

    # ---- sensed pushes (include/cmpc.h, cmpc_wrench_sensor; DESIGN.md 7f, "Sensed pushes") ----
    def wrench_sensor(self, delay=0, hold_knots=1, deadband=0.7, noise=None):
        """A wrench sensor for walk_device_sensed, as a dict with the C struct and its tensors: the reading of tick t is the hidden wrench of tick t - delay
        plus noise[t - tick_first] ([Tn, B, 6] float32, numpy or CUDA; None: none), zeroed as a whole when its force is shorter than deadband (the
        reference's 0.7; 0: off; inf: a blind sensor), and handed to the MPC on knots 0 .. hold_knots - 1 of fExt / tauExt."""
        return self.solver._wrench_sensor(delay, hold_knots, deadband, noise, device=self.dev)

    @staticmethod
    def _sensor_of(sensor, mm, push):
        """the sensor of a walk (None: none), checked against the walk's other inputs before anything is queued"""
        if sensor is None:
            return None
        if push is not None:
            raise ValueError("push= with a sensor: a known push and a sensed one are not summed (hidden_wrench is what the sensor reads)")
        if mm is None or mm["hidden_wrench"] is None:
            raise ValueError("a sensor needs mismatch['hidden_wrench'], the schedule it reads")
        return sensor

    def walk_device_sensed(self, ticks, com0, dcom0, h0, mismatch, sensor, tape=False, every=None, **kwargs):
        """walk_device_mismatch(ticks, com0, dcom0, h0, mismatch, **kwargs) with a wrench sensor between mismatch["hidden_wrench"] and the MPC
        (cmpc_rollout_walk_sensed_device): sensor = wrench_sensor(...).  ONE small launch in front of each tick turns the hidden schedule into the wrench
        rows the MPC sees (delayed, noisy, dead-banded, held for hold_knots knots) and the remainder only the plant feels; no host read.  The dict gains
        plant_wrench[ticks, B, 6] float32, that remainder.  tape=True: walk_device_taped's tape, which keeps mismatch, sensor and plant_wrench for
        backward_device_sensed() / forward_sensitivity_device_sensed().  every= (without a tape): walk_device_checkpointed's snapshots in front of the
        multiples of `every`, to resume from with walk_resume_device_sensed(); the checkpointed REVERSE of a sensed walk is refused (the delay couples
        rows across segments).  push= raises ValueError (the MPC's wrench is the sensed one).  sensor=None: walk_device_mismatch (tape=True:
        walk_device_taped(mismatch=...); every: walk_device_checkpointed(mismatch=...)), bit for bit, and no sensor key."""
        if sensor is not None and kwargs.get("push") is not None:
            raise ValueError("push= with a sensor: a known push and a sensed one are not summed (hidden_wrench is what the sensor reads)")
        if tape and every is not None:
            raise ValueError("walk_device_sensed: tape=True or every=, not both")
        args = inspect.signature(self.walk_device).bind(ticks, com0, dcom0, h0, **kwargs)
        args.apply_defaults()
        return self._queued(lambda: self._walk(bool(tape), None if every is None else int(every), None, *args.args, **args.kwargs, mismatch=mismatch,
                                               sensor=sensor))

    def walk_resume_device_sensed(self, snapshot, ticks, mismatch, sensor, **kwargs):
        """walk_resume_device_mismatch(snapshot, ticks, mismatch, **kwargs) with a wrench sensor (walk_device_sensed's): one pilot walk, one snapshot,
        index = zeros, and B hidden pushes, each sensed.  Tick numbers are those of the whole walk, so a delay reaches across the cut: ticks 0 .. c - 1
        and a resume at c under the same mismatch and sensor equal the unbroken walk bit for bit.  The dict gains plant_wrench[ticks, B, 6] (row 0 = the
        resume tick).  push= raises ValueError, and so does a snapshot that carries a wrench schedule of its own."""
        if sensor is not None and kwargs.get("push") is not None:
            raise ValueError("push= with a sensor: a known push and a sensed one are not summed (hidden_wrench is what the sensor reads)")
        args = inspect.signature(self.walk_resume_device).bind(snapshot, ticks, **kwargs)
        args.apply_defaults()
        return self._queued(lambda: self._walk_resume(*args.args, **args.kwargs, mismatch=mismatch, sensor=sensor))

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
        as_t = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.dev, torch.float64).contiguous()
        dh = torch.zeros(tuple(mm["hidden_wrench"].shape[:2]) + (k, 6), dtype=torch.float64, device=self.dev) if dir_hidden_wrench is None \
            else as_t(dir_hidden_wrench)
        dn = None if dir_sensor_noise is None or sn["noise"] is None else as_t(dir_sensor_noise)
        dw, dp = self._queued(lambda: self.solver._wrench_sense_jvp_device(0, T, k, mm, sn, dh, dn))
        return self.forward_sensitivity_device_mismatch(w2, dir_hidden_wrench=dp, dir_state_noise=dir_state_noise, dir_force_gain=dir_force_gain,
                                                        dir_ref_com=dir_ref_com, dir_ref_h=dir_ref_h, **dict(dirs, dir_wrench=dw))

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
        args = inspect.signature(self.walk_device).bind(ticks, com0, dcom0, h0, **kwargs)
        args.apply_defaults()
        return self._queued(lambda: self._walk(True, None, None, *args.args, **args.kwargs, mismatch=mismatch))

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

    def _tick_by_steps(self, i, now, mpc_prev, warm, dump, dP, dX0, dX, dInfo, state, wrench, dpush, push_ticks, planner):
        """one tick as seven calls of the C ABI with the host between them (cold starts, retry="launch", the dump hook; native_tick=False)"""
        torch, L, cfg, B, N = self.torch, self.L, self.cfg, self.B, self.cfg.N
        dt, dev, s = cfg.sampling_time, self.dev, self.solver
        if mpc_prev is None:
            lists = tuple(a.clone() for a in self.plan)
            if self.force_sample_time:     # (the snapped list is what the reference passes on: contactPhaseList = mannContactPhaseList)
                _, ok = s.contacts_force_sample_time_device(lists[0], lists[2], out=lists[0])
            else:
                ok = torch.ones((B,), dtype=torch.int32, device=dev)
        elif self.force_sample_time:
            plan_t, ok_snap = s.contacts_force_sample_time_device(self.plan[0], self.plan[2])
            lists, ok = s.contacts_merge_device(now, (plan_t, self.plan[1], self.plan[2]), mpc_prev)
            ok = ok & ok_snap
        else:
            # (whether every merge succeeded is read by the host at the END of the tick, with the status words: a read here would drain the stream in the
            #  middle of the tick and leave the GPU idle while the host queues the six launches in front of the solve -- 0.17 ms of a 0.83 ms tick at
            #  B <= 256, tools/gpu_rollout_tick_overhead.py.  Until then a failed problem is harmless: its merged list is empty, the sampling kernel leaves
            #  its blocks of dP as they were and writes land = -2, the adjustment kernel skips it -- include/cmpc.h)
            lists, ok = s.contacts_merge_device(now, self.plan, mpc_prev)
        land = s.contacts_sample_device(now, lists, dP)
        s.write_reference_from_planner_device(planner[0], planner[1], planner[2], planner[3], planner[4], planner[5], dP)
        if dpush is not None and i <= push_ticks:      # (the wrench rows of dP change while the push lasts and once more when it ends; zero from the start otherwise)
            wrench.zero_()
            if i < push_ticks:
                wrench[:, :max(push_ticks - i, 1), :3] = dpush[:, None, :]
            s.write_state_device(state, dP, wrench)
        else:
            s.write_state_device(state, dP, None)
        shifted = not (mpc_prev is None or not warm)
        if not shifted:
            # cold start: CoM at com0, feet at nominal, f_z = g/8 per corner
            dX0.zero_()
            dX0[:, L.com:L.com + 3 * (N + 1)] = state[:, 0:3].repeat(1, N + 1)
            for c in range(2):
                dX0[:, L.pos[c]:L.pos[c] + 3 * (N + 1)] = dP[:, L.p_nom[c]:L.p_nom[c] + 3 * (N + 1)]
                for j in range(4):
                    dX0[:, L.f[c][j] + 2:L.f[c][j] + 3 * N:3] = GRAVITY / 8.0   # (the library's cold start: cmpc_config.gravity / 8, which this package always sets to GRAVITY)
        else:
            s.shift_solution_device(dX, dX0)
        if dump is not None and i == dump[0]:   # developer hook: (tick, path) -> the tick's P and X0
            np.savez(dump[1], P=dP.cpu().numpy(), X0=dX0.cpu().numpy())
        s.solve_device(dP, dX0, dX, dInfo, warm=shifted)
        nretry = 0
        if self.retry == "launch" and shifted:
            bad = (dInfo[:, 5] != 0).nonzero().flatten()        # (one scalar comes to the host: the count)
            nretry = int(bad.numel())
            for lo in range(0, nretry, self.retry_batch):
                chunk = bad[lo:lo + self.retry_batch]
                idx = torch.cat([chunk, chunk[:1].expand(self.retry_batch - chunk.numel())]) if chunk.numel() < self.retry_batch else chunk
                P2 = dP.index_select(0, idx)
                X02 = torch.zeros((self.retry_batch, L.nx), dtype=torch.float32, device=dev)       # the cold start of SURVEY 8d
                X02[:, L.com:L.com + 3 * (N + 1)] = P2[:, L.p_com0:L.p_com0 + 3].repeat(1, N + 1)
                for c in range(2):
                    X02[:, L.pos[c]:L.pos[c] + 3 * (N + 1)] = P2[:, L.p_nom[c]:L.p_nom[c] + 3 * (N + 1)]
                    for j in range(4):
                        X02[:, L.f[c][j] + 2:L.f[c][j] + 3 * N:3] = GRAVITY / 8.0
                if self.models is not None:     # (the retry handle's table: the stragglers' own models, row for row)
                    self.solver2.set_models_device(self.models.index_select(0, idx))
                X2, I2 = self.solver2.solve_device(P2, X02)
                I2[:, 0] += dInfo.index_select(0, idx)[:, 0]     # iterations of both attempts
                I2[:, 3] += 10000.0                              # safeguard word: solved again from the cold start
                dX.index_copy_(0, chunk, X2[:chunk.numel()])
                dInfo.index_copy_(0, chunk, I2[:chunk.numel()])
        s.contacts_adjust_device(now, dX, land, lists)
        state, zmp = s.plant_step_device(dX, dP, state, step=dt / self.substeps, substeps=self.substeps)
        return ok, lists, land, nretry, state, zmp

    def _run(self, ticks, com0, dcom0, h0, push=None, push_ticks=0, warm=True, dump=None, replan=None, slow=None, record="full", timing=True, tape=False):
        """com0/dcom0/h0 [B,3] numpy; push [B,3] (mass-normalised force held for the first `push_ticks` ticks);
        replan {tick: (t, pose, n)}: the planner's lists from that tick on (the reference's generator re-plans while walking);
        slow (threshold, list): developer hook -- (tick, problem, P row, X0 row, info row) of every solve with more iterations;
        record "full": per-tick CoM, ZMP, landing offsets (host loops over the batch); "light": iteration statistics and the tick's
        wall-clock latency only (what bench.py times).  timing=False: without the library's event pair around every solve (cmpc_set_timing: an event record
        is a barrier packet on the stream, ~10 us of a tick each); rec["solve_ms"] is then NaN.
        tape=True: rec["tape"] keeps what backward() needs, per tick, in device tensors: X, P, lam_g (the multiplier output is turned on: x and info
        are bit-identical with it on, so a taped roll-out is bit-identical to an untaped one), the state that went in, info, ok, land and the times and
        counts of the planner's, the previous tick's and the merged lists -- about 12 KB per problem and tick at N = 20 (x, p and lam_g are a thousand
        floats each).  The state and the previous tick's list times are copied BEFORE the tick: the roll-out aliases dState / dStateOut and alternates two
        list buffers.  rec["tape"]["state"] is the final state.  Not with retry="launch" (the stragglers' multipliers live on the retry handle).
        Returns a dict of per-tick numpy records."""
        torch, L, cfg, B, N = self.torch, self.L, self.cfg, self.B, self.cfg.N
        dt = cfg.sampling_time
        dev = self.dev
        s = self.solver
        dP = torch.zeros((B, L.np), dtype=torch.float32, device=dev)
        dX0 = torch.zeros((B, L.nx), dtype=torch.float32, device=dev)
        dX = torch.zeros_like(dX0)
        dInfo = torch.zeros((B, 8), dtype=torch.float32, device=dev)
        state = torch.from_numpy(np.concatenate([com0, dcom0, h0], 1).astype(np.float32)).to(dev)
        wrench = torch.zeros((B, N, 6), dtype=torch.float32, device=dev)
        dpush = torch.from_numpy(np.asarray(push, np.float32)).to(dev) if push is not None else None
        # references (CentroidalMPCBlock.cpp:525-577 resamples the planner's trajectories at the MPC knots): the planner here is a straight line at the plan's mean
        # speed and zero angular momentum, a knot every dt from time zero to the end of the last tick's horizon -- resampled on the device every tick
        # (cmpc_write_reference_from_planner_device; inside cmpc_rollout_tick_device for the warm ticks), CoM height forced to 0.7 as the reference does (:534)
        # -- or the trajectories of set_references(), read at now - t_first as the device walk reads them
        refs = self._planner_refs(ticks)
        planner = lambda now: (refs[0], refs[1], refs[2], now - refs[3], refs[4], refs[5])
        import time
        rec = dict(iterations_mean=[], iterations_max=[], converged=[], merge_ok=[], com=[], land=[], landing_offset=[], solve_ms=[], zmp=[],
                   tick_ms=[], retried=[], unconverged=[])
        mpc_prev, tick_bufs = None, None
        s.set_timing(timing)
        if tape:
            assert self.retry != "launch", "tape=True needs retry='kernel' or None"
            s.set_multiplier_output(True)
            rec["tape"] = dict(ticks=[], dt=dt, substeps=self.substeps, force_sample_time=self.force_sample_time, push_ticks=push_ticks if push is not None else 0)
        box_up = np.array([c.bounding_box_upper_limit for c in cfg.contacts])
        box_lo = np.array([c.bounding_box_lower_limit for c in cfg.contacts])
        for i in range(ticks):
            now = i * dt
            torch.cuda.synchronize()
            t_tick = time.perf_counter()
            if replan and i in replan:
                self.plan = replan[i]
            if tape:    # (before the tick: it overwrites the state in place, and the list buffer of two ticks ago)
                tk = dict(now=now, state=state.clone(), plan_t=self.plan[0], plan_n=self.plan[2],
                          prev_t=mpc_prev[0].clone() if mpc_prev is not None else None, prev_n=mpc_prev[2].clone() if mpc_prev is not None else None,
                          push_knots=max(push_ticks - i, 1) if (dpush is not None and i < push_ticks) else 0)
            if self.native_tick and warm and mpc_prev is not None and not (dump is not None and i == dump[0]):
                if tick_bufs is None:
                    tick_bufs = ([tuple(torch.zeros_like(a) for a in self.plan) for _ in range(2)], torch.empty((B, 2), dtype=torch.int32, device=dev),
                                 torch.empty((B, 2), dtype=torch.float32, device=dev))
                lists = tick_bufs[0][i & 1] if mpc_prev[0] is not tick_bufs[0][i & 1][0] else tick_bufs[0][1 - (i & 1)]
                ok = torch.empty((B,), dtype=torch.int32, device=dev)
                land, zmp = tick_bufs[1], tick_bufs[2]
                wr = None
                if dpush is not None and i <= push_ticks:
                    wrench.zero_()
                    if i < push_ticks:
                        wrench[:, :max(push_ticks - i, 1), :3] = dpush[:, None, :]
                    wr = wrench
                s.rollout_tick_device(now, self.plan, mpc_prev, lists, ok, land, state, wr, dP, dX0, dX, dInfo, state, zmp, True,
                                      step=dt / self.substeps, substeps=self.substeps, planner=planner(now), force_sample_time=self.force_sample_time)
                mpc_prev = lists
                nretry = 0
            else:
                ok, lists, land, nretry, state, zmp = self._tick_by_steps(i, now, mpc_prev, warm, dump, dP, dX0, dX, dInfo, state, wrench, dpush, push_ticks, planner(now))
                mpc_prev = lists
            if tape:
                tk.update(X=dX.clone(), P=dP.clone(), lam_g=s.multipliers_device(dX, dP), info=dInfo.clone(), ok=ok.clone(), land=land.clone(),
                          list_t=lists[0].clone(), list_n=lists[2].clone(), step=dt / self.substeps, substeps=self.substeps,
                          force_sample_time=self.force_sample_time)
                rec["tape"]["ticks"].append(tk)
                rec["tape"]["state"] = state.clone()
                rec["tape"]["lists"] = tuple(a.clone() for a in lists)
            torch.cuda.synchronize()
            tick_ms = (time.perf_counter() - t_tick) * 1e3
            if not bool(ok.cpu().numpy().all()):
                # the reference aborts the tick when updateContactPhaseList returns false (CentroidalMPCBlock.cpp:603-607): so does the roll-out -- what
                # the tick computed is discarded (every per-tick list gets its entry, so that the records stay aligned; bench.py fails the roll-out
                # when it sees 'aborted_tick')
                rec["merge_ok"].append(False)
                rec["aborted_tick"] = i
                rec["tick_ms"].append(float("nan")); rec["retried"].append(0); rec["unconverged"].append(B)
                rec["iterations_mean"].append(float("nan")); rec["iterations_max"].append(0); rec["converged"].append(False)
                rec["solve_ms"].append(float("nan"))
                break
            rec["tick_ms"].append(tick_ms)
            rec["retried"].append(nretry)
            info = dInfo.cpu().numpy()
            rec["unconverged"].append(int((info[:, 5] != 0).sum()))
            if slow is not None:
                for b in np.where(info[:, 0] > slow[0])[0]:
                    slow[1].append((i, int(b), dP[b].cpu().numpy(), dX0[b].cpu().numpy(), info[b].copy()))
            rec["iterations_mean"].append(float(info[:, 0].mean()))
            rec["iterations_max"].append(int(info[:, 0].max()))
            rec["converged"].append(bool((info[:, 5] == 0).all()))
            rec.setdefault("failed_info", []).append(info[info[:, 5] != 0])
            rec["merge_ok"].append(True)
            rec["solve_ms"].append(s.last_solve_ms() if timing else float("nan"))
            if record != "full":
                continue
            rec["com"].append(state[:, 0:3].cpu().numpy())
            rec["zmp"].append(zmp.cpu().numpy())
            ln = land.cpu().numpy()
            rec["land"].append(ln)
            # landing position against the nominal one of the same knot, in the foot frame (the bounding box the NLP imposes)
            Xh, Ph = dX.cpu().numpy(), dP.cpu().numpy()
            off = np.zeros((B, 2, 3))
            for c in range(2):
                for b in range(B):
                    k = ln[b, c]
                    if 0 < k <= N:
                        R = Ph[b, L.p_R[c] + 9 * (k - 1):L.p_R[c] + 9 * k].reshape(3, 3).T   # vec(R) column-major
                        d = Xh[b, L.pos[c] + 3 * k:L.pos[c] + 3 * k + 3] - Ph[b, L.p_nom[c] + 3 * k:L.p_nom[c] + 3 * k + 3]
                        off[b, c] = R.T @ d
            rec["landing_offset"].append(off)
        s.set_timing(True)
        rec["box_upper"], rec["box_lower"] = box_up, box_lo
        return rec

    def backward(self, tape, grad_states, grad_X=None, rot=False):
        """The taped roll-out in reverse (cmpc_rollout_tick_vjp_device, one call per tick, last tick first).  tape = run(..., tape=True)["tape"];
        grad_states[ticks + 1, B, 9] = dl / d state_i of the states BEFORE tick i (i = 0 .. ticks - 1) and of the final state (i = ticks), a CUDA tensor or
        numpy; grad_X[ticks, B, n_x] float32 or None = dl / d x_i, a loss on the ticks' solutions.
        -> dict(state0[B, 9], list0[B, 2, M, 3] (the positions of the first tick's lists), push[B, 3] (the sum of the wrench gradients over the ticks and
        knots the push was written to), wrench[ticks, B, N, 6], models[B, 34], plan[B, 2, M, 3] (the planner's contact positions), status[ticks, B] int32:
        0, or why that tick of that problem passed no gradient on -- include/cmpc.h), float64 but wrench (float32).  The solution map is taken as
        independent of the warm start; contact times are not differentiated, and the planner's CoM and angular-momentum references only on the device walk:
        backward_device_refs().
        rot=True (cmpc_rollout_tick_vjp_rot_device per tick): the contacts' orientations too, in the body-frame tangent of their quaternions
        (q <- q (x) exp(omega / 2)): the dict also holds list_rot0[B, 2, M, 3] (the first tick's lists), plan_rot[B, 2, M, 3] (the planner's contacts) and
        rot[ticks, B, 2, N, 3] (each tick's per-stage dl/domega), float64; every other entry is bit-equal to rot=False.  A double-support tick under load
        has no orientation derivative (include/cmpc.h, "rotation directions"): out["removed"][ticks, B] is word 6 of each tick's dSens."""
        torch, B, N, L = self.torch, self.B, self.cfg.N, self.L
        ticks = tape["ticks"]
        T = len(ticks)
        as64 = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.dev, torch.float64).contiguous()
        gS = as64(grad_states)
        assert tuple(gS.shape) == (T + 1, B, 9)
        gX = None
        if grad_X is not None:
            gX = (grad_X if isinstance(grad_X, torch.Tensor) else torch.from_numpy(np.asarray(grad_X))).to(self.dev, torch.float32).contiguous()
            assert tuple(gX.shape) == (T, B, L.nx)
        M = ticks[0]["list_t"].shape[2]
        out = dict(push=torch.zeros((B, 3), dtype=torch.float64, device=self.dev), wrench=torch.zeros((T, B, N, 6), dtype=torch.float32, device=self.dev),
                   models=torch.zeros((B, 34), dtype=torch.float64, device=self.dev), plan=torch.zeros((B, 2, M, 3), dtype=torch.float64, device=self.dev),
                   status=torch.zeros((T, B), dtype=torch.int32, device=self.dev))
        if rot:
            out.update(plan_rot=torch.zeros((B, 2, M, 3), dtype=torch.float64, device=self.dev), rot=torch.zeros((T, B, 2, N, 3), dtype=torch.float64, device=self.dev),
                       removed=torch.zeros((T, B), dtype=torch.float32, device=self.dev))
        ls = self.solver.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        with torch.cuda.stream(ls):
            g, gl, glr = gS[T].clone(), None, None
            for i in reversed(range(T)):
                tk = ticks[i]
                if rot:
                    r = self.solver.rollout_tick_vjp_device(tk["now"], tk, g, gl, None if gX is None else gX[i], dGradPlan=out["plan"], dGradModel=out["models"],
                                                            dGradListRotOut=glr, rot=True, dGradPlanRot=out["plan_rot"])
                    glr = r["prev_list_rot"]
                    out["rot"][i] = r["rot"]
                    out["removed"][i] = r["sens"][:, 6]
                else:
                    r = self.solver.rollout_tick_vjp_device(tk["now"], tk, g, gl, None if gX is None else gX[i], dGradPlan=out["plan"], dGradModel=out["models"])
                g = r["state"] + gS[i]
                gl = r["prev_list"]
                out["wrench"][i] = r["wrench"]
                out["status"][i] = r["sens"][:, 0].to(torch.int32)
                if tk["push_knots"] > 0:
                    out["push"] += r["wrench"][:, :tk["push_knots"], :3].to(torch.float64).sum(1)
            out["state0"], out["list0"] = g, gl
            if rot:
                out["list_rot0"] = glr
        cur.wait_stream(ls)
        return out

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
        torch, B, L, s = self.torch, self.B, self.L, self.solver
        tape = w["tape"]
        T = tape["rows"]
        as_t = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.dev, dt).contiguous()
        gM = as_t(grad_measures, torch.float64)
        assert tuple(gM.shape) == (T, B, 4), f"grad_measures of shape {tuple(gM.shape)}: expected {(T, B, 4)}"
        gS0 = None if grad_states is None else as_t(grad_states, torch.float64)
        gX0 = None if grad_X is None else as_t(grad_X, torch.float32)
        assert gS0 is None or tuple(gS0.shape) == (T + 1, B, 9)
        assert gX0 is None or tuple(gX0.shape) == (T, B, L.nx)
        ls = s.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        with torch.cuda.stream(ls):
            gS = torch.zeros((T + 1, B, 9), dtype=torch.float64, device=self.dev) if gS0 is None else gS0.clone()
            gX = torch.zeros((T, B, L.nx), dtype=torch.float32, device=self.dev) if gX0 is None else gX0.clone()
            direct = torch.zeros((T, B, 32), dtype=torch.float64, device=self.dev)
            s.walk_measures_vjp_device(0, T, tape, 0, w["end_tick"], gM, gS, gX, direct)
        cur.wait_stream(ls)
        fold = lambda out: s.walk_measures_vjp_fold_device(direct, out.get("grad_P"), out["models"])
        out = self._backward_device(w, gS, gX, False, refs=refs, fold=fold)
        out["measure_direct"] = direct
        out["measure_rot"] = direct[:, :, 2:8].unflatten(2, (2, 3))
        return out

    def _backward_device(self, w, grad_states, grad_X, rot, refs=False, fold=None):
        torch, B, N, L = self.torch, self.B, self.cfg.N, self.L
        tape = w["tape"]
        T, M, s = tape["rows"], tape["max_contacts"], self.solver
        as_t = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.dev, dt).contiguous()
        gS = as_t(grad_states, torch.float64)
        assert tuple(gS.shape) == (T + 1, B, 9)
        gX = None
        if grad_X is not None:
            gX = as_t(grad_X, torch.float32)
            assert tuple(gX.shape) == (T, B, L.nx)
        z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=self.dev)
        out = dict(push=z((B, 3)), wrench=z((T, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((T, B), torch.int32),
                   end_tick=w["end_tick"])
        if rot:
            out.update(plan_rot=z((B, 2, M, 3)), rot=z((T, B, 2, N, 3)), removed=z((T, B), torch.float32))
        if refs:
            n_ref = tape["references"]["knots"]
            out.update(grad_P=z((T, B, L.np), torch.float32), ref_com=z((B, n_ref, 3)), ref_h=z((B, n_ref, 3)))
        mm = tape.get("mismatch")
        if mm is not None:    # (the tape of a mismatched walk: cmpc_rollout_walk_vjp_mismatch_device, and three more keys)
            out.update(hidden_wrench=z((T, B, 6)), state_noise=z((T, B, 9), torch.float32), force_gain=z((B,)))
        starts = list(tape["segments"])
        ls = s.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        with torch.cuda.stream(ls):
            g, gl = gS[T].clone(), z((B, 2, M, 3))    # (the gate in front of the last tick selects zero where the problem has ended)
            glr = z((B, 2, M, 3)) if rot else None
            for j in reversed(range(len(starts))):
                t0, t1 = starts[j], starts[j + 1] if j + 1 < len(starts) else T
                s.rollout_walk_vjp_device(t0, t1 - t0, tape, t0, w["end_tick"], gS, g, gl, out["status"], grad_X=gX, wrench=out["wrench"],
                                          grad_p=out.get("grad_P"), dGradPlan=out["plan"], dGradModel=out["models"], carry_list_rot=glr, dGradPlanRot=out.get("plan_rot"),
                                          grad_rot=out.get("rot"), removed=out.get("removed"), mismatch=mm, grad_hidden=out.get("hidden_wrench"),
                                          grad_noise=out.get("state_noise"), grad_gain=out.get("force_gain"))
            for i in reversed(range(min(T, tape["push_ticks"]))):    # (backward()'s expression, tick by tick in its order)
                out["push"] += out["wrench"][i][:, :max(tape["push_ticks"] - i, 1), :3].to(torch.float64).sum(1)
            out["state0"], out["list0"] = g, gl
            if rot:
                out["list_rot0"] = glr
            if fold is not None:    # (backward_device_measures: what the measures send to grad_P and models directly, in front of the reference VJP)
                fold(out)
            if refs:    # (the replan segments share the trajectories: one launch over all rows)
                s.reference_from_planner_vjp_device(0, T, tape["references"], w["end_tick"], out["grad_P"], out["ref_com"], out["ref_h"])
        cur.wait_stream(ls)
        return out

    # ---- the refill walk's tape regrouped by trial (include/cmpc.h, cmpc_walk_tape_regroup; DESIGN.md 7f, "Refill, taped") ----
    def _refill_tape_of(self, who, w):
        """the slot-major tape of w = walk_device_refill_taped(...), or NotImplementedError -- raised before anything touches a GPU"""
        if "tick0" in w:
            raise NotImplementedError(f"{who}: trials that start from a snapshot are not taped (walk_device_refill_from_snapshot's dict)")
        tape = w.get("tape")
        if tape is None or "refill" not in tape:
            raise NotImplementedError(f"{who}: needs the dict of walk_device_refill_taped (a refill walk without a tape has nothing to regroup)")
        if self.M > 16:
            raise NotImplementedError(f"{who}: lists longer than 16 contacts are out of scope of a refill walk")
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
        src = WalkingRollout._refill_tape_of(self, "refill_trial_walk", w)    # (the refusals come before self is used for anything but its list length)
        torch, B, s = self.torch, self.B, self.solver
        if isinstance(trials, torch.Tensor):
            idx = trials.to(self.dev, torch.int32).reshape(-1)
        else:
            idx = torch.from_numpy(np.ascontiguousarray(np.asarray(trials, np.int64).reshape(-1), np.int32)).to(self.dev)
        assert idx.numel() <= B, f"refill_trial_walk: at most {B} trials per view"
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
        src = WalkingRollout._refill_tape_of(self, "backward_device_refill", w)
        torch, B, s, L = self.torch, self.B, self.solver, self.L
        TT, Q = int(src["trial_ticks"]), int(src["refill"]["trials"])
        as_t = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.dev, dt).contiguous()
        gS = as_t(grad_states, torch.float64)
        assert tuple(gS.shape) == (TT + 1, Q, 9)
        gX = None
        if grad_X is not None:
            gX = as_t(grad_X, torch.float32)
            assert tuple(gX.shape) == (TT, Q, L.nx)
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

    # ---- snapshots: resume, branch, and the reverse walk in bounded memory (include/cmpc.h, cmpc_walk_snapshot; DESIGN.md 7f, "Snapshots") ----
    def _queued(self, fn):
        """fn() with the solver's launch stream as torch's current stream, as walk_device queues its ticks"""
        torch = self.torch
        assert self.retry != "launch", "the device walk needs retry='kernel' or None"
        ls = self.solver.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        try:
            with torch.cuda.stream(ls):
                return fn()
        finally:
            cur.wait_stream(ls)

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
                if sensor is not None:
                    assert wr is None, "a known push and a sensed one are not summed"
                    cur = s._rollout_walk_sensed_device(sensor, plant[a - t0:], a, b - a, cold and a == t0, plan_at(a), sets[0], sets[1], cur, live["ok"],
                                                        live["land"], live["state"], live["P"], live["X0"], live["X"], live["info"], live["zmp"], rec,
                                                        row0=a - row_shift, step=dt / self.substeps, substeps=self.substeps, planner=refs,
                                                        force_sample_time=self.force_sample_time, tape=tape, tape_row0=a - tape_shift, mismatch=mismatch)
                    if states is not None:
                        states[b - row_shift].copy_(live["state"])
                    continue
                cur = s.rollout_walk_device(a, b - a, cold and a == t0, plan_at(a), sets[0], sets[1], cur, live["ok"], live["land"], live["state"], live["P"],
                                            live["X0"], live["X"], live["info"], live["zmp"], rec, row0=a - row_shift, wrench_ticks=wr,
                                            step=dt / self.substeps, substeps=self.substeps, planner=refs, force_sample_time=self.force_sample_time,
                                            tape=tape, tape_row0=a - tape_shift, mismatch=mismatch)
                if states is not None:
                    states[b - row_shift].copy_(live["state"])
        finally:
            self._limits_off(limits)
            if skip_ended:
                s.set_ended_device(None)
        s.walk_snapshot_mark(live, t1, cur)
        return out

    def walk_device_checkpointed(self, ticks, com0, dcom0, h0, every, **kwargs):
        """walk_device(ticks, com0, dcom0, h0, **kwargs) cut into calls at the multiples of `every` and at the replan ticks (walk_schedule), with ONE
        snapshot launch (cmpc_rollout_snapshot_device, include/cmpc.h) in front of each tick k * every, k >= 1.  -> walk_device's dict, bit-equal in
        every key, plus "checkpoints" {tick: snapshot} (BatchSolver.walk_snapshot: everything that tick reads of the ticks before it, about 13 KB per
        problem at N = 20) and "inputs", the small things a re-run needs, by reference: state0, the wrench schedule and push_ticks, the plans of replan
        and the plan in force at tick 0, the references, stop, skip_ended, ticks, every.  Like walk_device: no host read and no synchronisation.
        Continue or fork from a checkpoint: walk_resume_device().  The gradient without a whole-walk tape: backward_device_checkpointed()."""
        mismatch = kwargs.pop("mismatch", None)    # (walk_device_mismatch's argument; kept in "inputs" for backward_device_checkpointed_mismatch)
        args = inspect.signature(self.walk_device).bind(ticks, com0, dcom0, h0, **kwargs)
        args.apply_defaults()
        return self._queued(lambda: self._walk(False, int(every), None, *args.args, **args.kwargs, mismatch=mismatch))

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
        args = inspect.signature(self.walk_resume_device).bind(snapshot, ticks, **kwargs)
        args.apply_defaults()
        return self._queued(lambda: self._walk_resume(*args.args, **args.kwargs, mismatch=mismatch))

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
        torch, B, N, L, M, s, dev = self.torch, self.B, self.cfg.N, self.L, self.M, self.solver, self.dev
        inp, cps = w["inputs"], w["checkpoints"]
        mm = inp.get("mismatch")
        if inp.get("sensor") is not None:    # (the sensor's delay couples rows across segments: its fold must run once over the whole arrays)
            raise NotImplementedError("backward_device_checkpointed: the walk ran under a wrench sensor; its reverse is backward_device_sensed on a tape")
        if mm is not None and not mismatch:
            raise NotImplementedError("backward_device_checkpointed: the walk ran under a plant mismatch; its reverse in bounded memory is "
                                      "backward_device_checkpointed_mismatch")
        T, every = inp["ticks"], inp["every"]
        as_t = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(dev, dt).contiguous()
        gS = as_t(grad_states, torch.float64)
        assert tuple(gS.shape) == (T + 1, B, 9)
        gX = None
        if grad_X is not None and not callable(grad_X):
            gX = as_t(grad_X, torch.float32)
            assert tuple(gX.shape) == (T, B, L.nx)
        z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
        out = dict(push=z((B, 3)), wrench=z((T, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((T, B), torch.int32),
                   end_tick=w["end_tick"])
        if rot:
            out.update(plan_rot=z((B, 2, M, 3)), rot=z((T, B, 2, N, 3)), removed=z((T, B), torch.float32))
        if mm is not None:    # (backward_device's three more keys on a mismatch tape)
            out.update(hidden_wrench=z((T, B, 6)), state_noise=z((T, B, 9), torch.float32), force_gain=z((B,)))
        rows = min(every, T) + 1
        key = (rows, inp["stop"])
        ws = getattr(self, "_checkpoint_ws", None)
        if ws is None or ws["key"] != key:    # (one set of live buffers, one record without a trace and one tape, re-used by every segment and every call)
            s.set_multiplier_output(True)
            rec = s.walk_record(rows, stop=inp["stop"], trace=False, device=dev)
            ws = dict(key=key, live=self._live_buffers(rec),
                      tape=s.walk_tape(rows, M, step=self.cfg.sampling_time / self.substeps, substeps=self.substeps,
                                       force_sample_time=self.force_sample_time, device=dev),
                      gx=torch.zeros((rows, B, L.nx), dtype=torch.float32, device=dev))
            self._checkpoint_ws = ws
        live, tp = ws["live"], ws["tape"]
        bounds = [0] + sorted(cps) + [T]
        g, gl = gS[T].clone(), z((B, 2, M, 3))    # (the gate in front of the last tick selects zero where the problem has ended)
        glr = z((B, 2, M, 3)) if rot else None
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
        for i in reversed(range(min(T, inp["push_ticks"]))):    # (backward()'s expression, tick by tick in its order)
            out["push"] += out["wrench"][i][:, :max(inp["push_ticks"] - i, 1), :3].to(torch.float64).sum(1)
        out["state0"], out["list0"] = g, gl
        if rot:
            out["list_rot0"] = glr
        out["tape_rows_peak"] = peak
        return out

    def forward_sensitivity(self, tape, dir_state0=None, dir_list0=None, dir_list_rot0=None, dir_plan=None, dir_plan_rot=None, dir_push=None, dir_models=None,
                            dir_wrench=None, solutions=False):
        """The taped roll-out in forward mode (cmpc_rollout_tick_jvp_device, one call per tick, first tick first): how the whole trajectory moves along k
        input directions at once -- the transpose of backward(rot=True), input for output.  Every direction carries a column axis k right after B (CUDA
        tensors or numpy; None: zero): dir_state0[B, k, 9]; dir_list0 / dir_list_rot0[B, k, 2, M, 3], the positions and orientations (body-frame tangent)
        of the first tick's lists; dir_plan / dir_plan_rot[B, k, 2, M, 3], the planner's contacts, read by every merge; dir_push[B, k, 3], which enters
        the wrench rows of the knots and ticks the push was written to (the transpose of backward's push sum); dir_models[B, k, 34];
        dir_wrench[ticks, B, k, N, 6] float32.
        -> dict(states[ticks + 1, B, k, 9] float64: the directions of the states before each tick and of the final state; list, list_rot[B, k, 2, M, 3]:
        the final lists' directions; X[ticks, B, k, n_x] float32 when solutions=True; status[ticks, B] int32: 0, or why that tick of that problem passed
        nothing on; removed[ticks, B]: word 6 of each tick's dSens -- include/cmpc.h)."""
        torch, B, N, L = self.torch, self.B, self.cfg.N, self.L
        ticks = tape["ticks"]
        T = len(ticks)
        M = ticks[0]["list_t"].shape[2]

        def as_dir(a, dtype, tail, lead=()):
            if a is None:
                return None
            a = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.dev, dtype).contiguous()
            assert a.dim() == len(lead) + 2 + len(tail) and tuple(a.shape[:len(lead) + 1]) == lead + (B,) and tuple(a.shape[len(lead) + 2:]) == tail, \
                f"direction of shape {tuple(a.shape)}: expected {lead + (B, 'k') + tail}"
            return a
        f32, f64 = torch.float32, torch.float64
        ds, dl, dlr = as_dir(dir_state0, f64, (9,)), as_dir(dir_list0, f64, (2, M, 3)), as_dir(dir_list_rot0, f64, (2, M, 3))
        dpl, dplr = as_dir(dir_plan, f64, (2, M, 3)), as_dir(dir_plan_rot, f64, (2, M, 3))
        dpush, dmod, dwr = as_dir(dir_push, f32, (3,)), as_dir(dir_models, f64, (34,)), as_dir(dir_wrench, f32, (N, 6), lead=(T,))
        ks = {int(a.shape[1]) for a in (ds, dl, dlr, dpl, dplr, dpush, dmod) if a is not None} | ({int(dwr.shape[2])} if dwr is not None else set())
        assert len(ks) == 1, "forward_sensitivity: no direction, or directions of different k"
        k = ks.pop()
        rot = dlr is not None or dplr is not None
        out = dict(states=torch.zeros((T + 1, B, k, 9), dtype=f64, device=self.dev), status=torch.zeros((T, B), dtype=torch.int32, device=self.dev),
                   removed=torch.zeros((T, B), dtype=f32, device=self.dev))
        if solutions:
            out["X"] = torch.zeros((T, B, k, L.nx), dtype=f32, device=self.dev)
        ls = self.solver.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        with torch.cuda.stream(ls):
            if ds is not None:
                out["states"][0] = ds
            for i, tk in enumerate(ticks):
                w = None if dwr is None else dwr[i]
                if dpush is not None and tk["push_knots"] > 0:
                    w = torch.zeros((B, k, N, 6), dtype=f32, device=self.dev) if w is None else w.clone()
                    w[:, :, :tk["push_knots"], :3] += dpush[:, :, None, :]
                r = self.solver.rollout_tick_jvp_device(tk["now"], tk, k, dDirState=ds, dDirPrevList=dl, dDirPrevListRot=dlr, dDirPlan=dpl, dDirPlanRot=dplr,
                                                        dDirWrench=w, dDirModel=dmod, x=solutions, out_state=out["states"][i + 1])
                ds, dl = r["state"], r["list"]
                if rot:
                    dlr = r["list_rot"]
                if solutions:
                    out["X"][i] = r["x"]
                out["status"][i] = r["sens"][:, 0].to(torch.int32)
                out["removed"][i] = r["sens"][:, 6]
            out["list"] = dl
            out["list_rot"] = dlr if rot else torch.zeros((B, k, 2, M, 3), dtype=f64, device=self.dev)
        cur.wait_stream(ls)
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
        args = inspect.signature(self.forward_sensitivity_device).bind(w, **dirs)
        args.apply_defaults()
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
        args = inspect.signature(self.forward_sensitivity_device).bind(w, **dirs)
        args.apply_defaults()
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
            dmod = (dmod if isinstance(dmod, torch.Tensor) else torch.from_numpy(np.asarray(dmod))).to(self.dev, torch.float64).contiguous()
        ls = s.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        with torch.cuda.stream(ls):
            r["measures"] = torch.zeros((T, B, k, 4), dtype=torch.float64, device=self.dev)
            s.walk_measures_jvp_device(0, T, tape, 0, w["end_tick"], k, r["states"], r["X"], r["measures"], dir_model=dmod)
        cur.wait_stream(ls)
        return r

    def _forward_sensitivity_device(self, w, dir_ref_com, dir_ref_h, dir_state0, dir_list0, dir_list_rot0, dir_plan, dir_plan_rot, dir_push, dir_models,
                                    dir_wrench, solutions, mismatch_dirs=None):
        torch, B, N, L = self.torch, self.B, self.cfg.N, self.L
        tape = w["tape"]
        if tape.get("mismatch") is not None and mismatch_dirs is None:    # (the plain tick JVP takes its partials at the MPC's forces and wrench: on this tape it would be silently wrong)
            raise NotImplementedError("forward_sensitivity_device: the tape carries a plant mismatch; its forward mode is forward_sensitivity_device_mismatch")
        T, M, s = tape["rows"], tape["max_contacts"], self.solver

        def as_dir(a, dtype, tail, lead=()):
            if a is None:
                return None
            a = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(self.dev, dtype).contiguous()
            assert a.dim() == len(lead) + 2 + len(tail) and tuple(a.shape[:len(lead) + 1]) == lead + (B,) and tuple(a.shape[len(lead) + 2:]) == tail, \
                f"direction of shape {tuple(a.shape)}: expected {lead + (B, 'k') + tail}"
            return a
        f32, f64 = torch.float32, torch.float64
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
        assert len(ks) == 1, "forward_sensitivity_device: no direction, or directions of different k"
        k = ks.pop()
        rot = dlr is not None or dplr is not None
        z = lambda shape, dt=f64: torch.zeros(shape, dtype=dt, device=self.dev)
        out = dict(states=z((T + 1, B, k, 9)), status=z((T, B), torch.int32), removed=z((T, B), f32), end_tick=w["end_tick"])
        if solutions:
            out["X"] = z((T, B, k, L.nx), f32)
        starts = list(tape["segments"])
        ls = s.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        with torch.cuda.stream(ls):
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
        cur.wait_stream(ls)
        return out


def yaw_plan_poses(pose, plan_yaw):
    """pose[B, 2, M, 7] float32 (x y z, quaternion w x y z) with every contact yawed about its own z axis by plan_yaw[B, 2, M] float64:
    q <- q (x) (cos(psi / 2), 0, 0, sin(psi / 2)), formed in float64; an entry with psi == 0 keeps its bits."""
    import torch
    q = pose[..., 3:7].to(torch.float64)
    w, x, y, z = q.unbind(-1)
    c, s = torch.cos(0.5 * plan_yaw), torch.sin(0.5 * plan_yaw)
    qr = torch.stack([w * c - z * s, x * c + y * s, y * c - x * s, z * c + w * s], -1).to(torch.float32)
    out = pose.clone()
    out[..., 3:7] = torch.where((plan_yaw == 0)[..., None], pose[..., 3:7], qr)
    return out


def so3_right_jacobian(omega):
    """omega[..., 3] -> Jr[..., 3, 3], the right Jacobian of SO(3): Exp(omega + d) = Exp(omega) Exp(Jr(omega) d) to first order.  Formed in float64 as
    I + a W + b W^2 with W = [omega]x, a = -(1 - cos t) / t^2, b = (t - sin t) / t^3, t = |omega|, both by their series where t < 1e-2 (there the closed
    forms cancel; the series' first dropped term is below 1e-20).  W and W^2 have a zero column along omega's own axis, so the z column at
    omega = (0, 0, psi) is exactly e_z."""
    import torch
    om = omega.to(torch.float64)
    x, y, z = om.unbind(-1)
    t2 = x * x + y * y + z * z
    small = t2 < 1e-4
    t2s = torch.where(small, torch.ones_like(t2), t2)       # (the closed forms are not evaluated near zero)
    t = torch.sqrt(t2s)
    a = torch.where(small, -(0.5 - t2 / 24.0 + t2 * t2 / 720.0 - t2 * t2 * t2 / 40320.0), -(1.0 - torch.cos(t)) / t2s)
    b = torch.where(small, 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0 - t2 * t2 * t2 / 362880.0, (t - torch.sin(t)) / (t2s * t))
    o = torch.zeros_like(x)
    W = torch.stack([torch.stack([o, -z, y], -1), torch.stack([z, o, -x], -1), torch.stack([-y, x, o], -1)], -2)
    W2 = (W[..., :, None, :] * W.transpose(-1, -2)[..., None, :, :]).sum(-1)     # W2[i, j] = sum_k W[i, k] W[k, j], k in order
    return torch.eye(3, dtype=torch.float64, device=om.device) + a[..., None, None] * W + b[..., None, None] * W2


def rot_plan_poses(pose, plan_rot):
    """pose[B, 2, M, 7] float32 (x y z, quaternion w x y z) with every contact rotated by the rotation vector plan_rot[B, 2, M, 3] float64 in its own
    frame: q <- q (x) Exp(omega), Exp(omega) = (cos(t / 2), sin(t / 2) omega / t), formed in float64 (sin(t / 2) / t by its series where t < 1e-2).  An
    entry whose x and y components are exactly 0 is yaw_plan_poses' expression for that entry, to the bit (so a zero entry keeps its bits)."""
    import torch
    om = plan_rot.to(torch.float64)
    ox, oy, oz = om.unbind(-1)
    t2 = ox * ox + oy * oy + oz * oz
    small = t2 < 1e-4
    t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    k = torch.where(small, 0.5 - t2 / 48.0 + t2 * t2 / 3840.0 - t2 * t2 * t2 / 645120.0, torch.sin(0.5 * t) / t)
    rw = torch.where(small, 1.0 - t2 / 8.0 + t2 * t2 / 384.0 - t2 * t2 * t2 / 46080.0, torch.cos(0.5 * t))
    rx, ry, rz = k * ox, k * oy, k * oz
    w, x, y, z = pose[..., 3:7].to(torch.float64).unbind(-1)
    qr = torch.stack([w * rw - x * rx - y * ry - z * rz, w * rx + x * rw + y * rz - z * ry, w * ry - x * rz + y * rw + z * rx,
                      w * rz + x * ry - y * rx + z * rw], -1).to(torch.float32)
    out = yaw_plan_poses(pose, oz)
    out[..., 3:7] = torch.where(((ox == 0) & (oy == 0))[..., None], out[..., 3:7], qr)
    return out


def rollout_differentiable(rollout: WalkingRollout, ticks, state0, push=None, models=None, push_ticks=0, plan_yaw=None, device_walk=False, replan=None,
                           plan_rot=None, hidden_wrench=None, state_noise=None, force_gain=None, ref_com=None, ref_h=None):
    """The closed loop as a torch.autograd.Function, in the shape of solver.solve_differentiable: forward runs rollout.run(ticks, ..., tape=True) from
    state0[B, 9] (com, dcom, h; a CUDA tensor) under push[B, 3] (held for the first push_ticks ticks) and returns the states [ticks + 1, B, 9] float32
    (state0 first); backward is WalkingRollout.backward and returns state0.grad, push.grad and models.grad.  models: None, or a [B, 34] float64 CUDA
    tensor installed on the roll-out's solver (set_models_device) and left installed.  rollout.last_tape / rollout.last_backward hold the tape of the last
    forward and the dict of the last backward (its status words say which ticks passed no gradient on).
    plan_yaw: None, or a [B, 2, M] float64 CUDA tensor: entry (b, c, m) yaws the planner's contact m of foot c about its own z axis before the run
    (yaw_plan_poses, on a copy of rollout.plan's poses made for this call; rollout.plan is left as it was).  backward then runs with rot=True and
    plan_yaw.grad = the e_z component of plan_rot + list_rot0: the first tick's list is the planner's list entry for entry, and every later tick reads the
    planner's entries through the merge; rotations about one axis commute, so the body-frame tangent at the yawed quaternion is d psi e_z.
    device_walk=True: forward is rollout.walk_device_taped (replan: its argument; only here) and backward is WalkingRollout.backward_device -- no
    host read in either, and a problem may END (a failed merge, a solve that does not converge, a non-finite state) without taking the batch's gradient
    with it: nothing asserts that every tick ran.  For a problem that ended at tick e the returned states hold final_state in rows > e (row e is
    final_state already), and backward first folds the cotangents of those rows into row e, which is the derivative of the function as returned.
    rollout.last_walk is the walk's dict (end_tick says who ended and when).  Forward mode (torch.autograd.forward_ad over state0, push and models) is
    WalkingRollout.forward_sensitivity_device at k = 1, its dict in rollout.last_forward: the tangent of the rows > e of a problem that ended at tick e is
    the tangent of its row e -- a select, the transpose of backward's fold.  Not with plan_yaw (NotImplementedError): on the device path a yaw is
    plan_rot[..., 2].
    plan_rot: None, or a [B, 2, M, 3] float64 CUDA tensor, on both paths: entry (b, c, m) rotates the planner's contact m of foot c by the rotation
    vector omega in its own frame before the run, q <- q (x) Exp(omega) (rot_plan_poses, on a copy of rollout.plan's poses and of the poses of every
    plan in replan; an entry without x and y components is plan_yaw's rotation to the bit).  backward runs with rot=True (backward, or
    backward_device_rot with device_walk=True) and plan_rot.grad = Jr(omega)^T (plan_rot + list_rot0), Jr the right Jacobian of SO(3)
    (so3_right_jacobian): q (x) Exp(omega + d) = q (x) Exp(omega) (x) Exp(Jr(omega) d), and the library's gradients are in the body-frame tangent at
    the rotated quaternion.  Its z component at omega = (0, 0, psi) is plan_yaw.grad to the bit.  Forward mode passes Jr(omega) t as dir_plan_rot and
    dir_list_rot0.  Not together with plan_yaw (ValueError).
    ref_com / ref_h: None, or CUDA tensors [B, n, 3]: the planner's CoM / angular-momentum trajectories of this call, in place of the ones
    rollout.set_references installed (or of the default straight line); their timing, robot_mass and com_height are what it installed, or the default
    line's (a knot every dt from time zero, mass 1, height 0.7).  The walk reads them as float32.  Only with device_walk=True (NotImplementedError
    otherwise, before anything touches a GPU): backward is then WalkingRollout.backward_device_refs and returns ref_com.grad / ref_h.grad, forward mode
    takes their tangents through forward_sensitivity_device_refs.  The fold and select for the rows behind a problem's end are the same.
    hidden_wrench [Th, B, 6] / state_noise [Tn, B, 9] / force_gain [B]: None, or torch tensors: the plant mismatch of WalkingRollout.walk_device_mismatch
    with tick_first = 0 (a wrench the MPC is not told about, noise on the state it measures, a gain on the forces the plant applies).  Only with
    device_walk=True (NotImplementedError otherwise, before anything touches a GPU): backward returns their .grad from the keys hidden_wrench,
    state_noise and force_gain of backward_device (rows behind Th / Tn have no input to receive theirs).  Forward mode over a mismatched walk raises
    NotImplementedError here: call WalkingRollout.forward_sensitivity_device_mismatch on rollout.last_walk.  In bounded memory:
    rollout_differentiable_checkpointed_mismatch."""
    mismatched = hidden_wrench is not None or state_noise is not None or force_gain is not None
    if mismatched and not device_walk:
        raise NotImplementedError("rollout_differentiable: hidden_wrench / state_noise / force_gain need device_walk=True")
    if (ref_com is not None or ref_h is not None) and not device_walk:
        raise NotImplementedError("rollout_differentiable: ref_com / ref_h need device_walk=True")
    import torch

    if plan_rot is not None and plan_yaw is not None:
        raise ValueError("rollout_differentiable: plan_rot and plan_yaw are two parametrisations of the same rotation: give one")
    if device_walk:
        if plan_yaw is not None:
            raise NotImplementedError("rollout_differentiable(device_walk=True): plan_yaw is not taken on the device path; pass the yaw as plan_rot[..., 2]")
        return _rollout_differentiable_device(rollout, ticks, state0, push, models, push_ticks, replan, plan_rot, ref_com, ref_h,
                                              (hidden_wrench, state_noise, force_gain) if mismatched else None)
    if replan is not None:
        raise NotImplementedError("rollout_differentiable: replan needs device_walk=True")

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, state0, push, models, plan_yaw, plan_rot):
            if models is not None:
                rollout.models = models.detach().to(rollout.dev, torch.float64).contiguous()
                rollout.models_ok = rollout.solver.set_models_device(rollout.models)
            s0 = state0.detach().to(torch.float32).cpu().numpy()
            plan = rollout.plan
            if plan_yaw is not None:
                psi = plan_yaw.detach().to(rollout.dev, torch.float64)
                assert tuple(psi.shape) == tuple(plan[1].shape[:3]), f"plan_yaw: expected {tuple(plan[1].shape[:3])}"
                rollout.plan = (plan[0], yaw_plan_poses(plan[1], psi), plan[2])
            ctx.jr = None
            if plan_rot is not None:
                om = plan_rot.detach().to(rollout.dev, torch.float64)
                assert tuple(om.shape) == tuple(plan[1].shape[:3]) + (3,), f"plan_rot: expected {tuple(plan[1].shape[:3]) + (3,)}"
                rollout.plan = (plan[0], rot_plan_poses(plan[1], om), plan[2])
                ctx.jr = so3_right_jacobian(om)
            try:
                rec = rollout.run(ticks, s0[:, 0:3], s0[:, 3:6], s0[:, 6:9], push=None if push is None else push.detach().to(torch.float32).cpu().numpy(),
                                  push_ticks=push_ticks, record="light", tape=True)
            finally:
                rollout.plan = plan
            ctx.rot = plan_yaw is not None or plan_rot is not None
            tape = rec["tape"]
            assert len(tape["ticks"]) == ticks, f"the roll-out stopped at tick {rec.get('aborted_tick')}"
            rollout.last_tape = ctx.tape = tape
            ctx.dtypes = (state0.dtype, None if push is None else push.dtype)
            return torch.stack([tk["state"] for tk in tape["ticks"]] + [tape["state"]])

        @staticmethod
        def backward(ctx, gStates):
            r = rollout.backward(ctx.tape, gStates, rot=ctx.rot)
            rollout.last_backward = r
            return (r["state0"].to(ctx.dtypes[0]), None if ctx.dtypes[1] is None else r["push"].to(ctx.dtypes[1]),
                    r["models"] if ctx.needs_input_grad[2] else None,
                    (r["plan_rot"][..., 2] + r["list_rot0"][..., 2]) if ctx.rot and ctx.needs_input_grad[3] else None,
                    _jr_transposed(ctx.jr, r["plan_rot"] + r["list_rot0"]) if ctx.jr is not None and ctx.needs_input_grad[4] else None)

        @staticmethod
        def jvp(ctx, t_state0, t_push, t_models, t_yaw, t_rot):
            """torch.autograd.forward_ad: forward_sensitivity at k = 1 on the tape the forward left.  A yaw tangent is d psi e_z on the planner's
            orientations and on the first tick's list, the transpose of what backward returns for plan_yaw."""
            col = lambda t, dt: None if t is None else t.detach().to(rollout.dev, dt)[:, None].contiguous()
            yaw = None
            if t_yaw is not None:
                yaw = torch.zeros(tuple(t_yaw.shape[:1]) + (1,) + tuple(t_yaw.shape[1:]) + (3,), dtype=torch.float64, device=rollout.dev)
                yaw[..., 2] = t_yaw.detach().to(rollout.dev, torch.float64)[:, None]
            if t_rot is not None:
                yaw = _jr_applied(ctx.jr, t_rot.detach().to(rollout.dev, torch.float64))[:, None].contiguous()
            if all(t is None for t in (t_state0, t_push, t_models, t_yaw, t_rot)):
                return torch.zeros((len(ctx.tape["ticks"]) + 1, rollout.B, 9), dtype=torch.float32, device=rollout.dev)
            r = rollout.forward_sensitivity(ctx.tape, dir_state0=col(t_state0, torch.float64), dir_push=col(t_push, torch.float32),
                                            dir_models=col(t_models, torch.float64), dir_plan_rot=yaw, dir_list_rot0=yaw)
            rollout.last_forward = r
            return r["states"][:, :, 0].to(torch.float32)

    return _Fn.apply(state0, push, models, plan_yaw, plan_rot)


def _jr_transposed(jr, g):
    """Jr^T g per entry, the three products summed in index order"""
    return (jr * g[..., :, None]).sum(-2)


def _jr_applied(jr, t):
    """Jr t per entry, the three products summed in index order"""
    return (jr * t[..., None, :]).sum(-1)


def rollout_differentiable_checkpointed_mismatch(rollout: WalkingRollout, ticks, state0, every, hidden_wrench=None, state_noise=None, force_gain=None,
                                                 push=None, models=None, push_ticks=0, replan=None):
    """rollout_differentiable_checkpointed under a plant mismatch: hidden_wrench [Th, B, 6] / state_noise [Tn, B, 9] / force_gain [B] as
    rollout_differentiable's (tick_first = 0; each None or a torch tensor).  Forward is WalkingRollout.walk_device_checkpointed(mismatch=...) cut at every
    tick, backward is WalkingRollout.backward_device_checkpointed_mismatch: the returned states, and state0.grad, push.grad, models.grad,
    hidden_wrench.grad, state_noise.grad and force_gain.grad equal rollout_differentiable(device_walk=True, hidden_wrench=, state_noise=, force_gain=)'s to
    the bit, without a whole-walk tape.  Not here, as there: plan_rot, ref_com / ref_h and forward mode.  (A function of its own:
    rollout_differentiable_checkpointed's signature is pinned.)"""
    import torch

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, state0, push, models, hidden, noise, gain):
            det = lambda a: None if a is None else a.detach().to(rollout.dev, torch.float32).contiguous()
            mm = None
            if hidden is not None or noise is not None or gain is not None:
                mm = dict(hidden_wrench=det(hidden), state_noise=det(noise), force_gain=det(gain), tick_first=0)
            ctx.mm_meta = tuple(None if a is None else (a.dtype, int(a.shape[0])) for a in (hidden, noise, gain))
            assert all(a is None or 1 <= a.shape[0] <= ticks for a in (hidden, noise)), "hidden_wrench / state_noise: between 1 and `ticks` rows"
            if models is not None:
                rollout.models = models.detach().to(rollout.dev, torch.float64).contiguous()
                rollout.models_ok = rollout.solver.set_models_device(rollout.models)
            s0 = state0.detach().to(rollout.dev, torch.float32)
            states = torch.zeros((ticks + 1, rollout.B, 9), dtype=torch.float32, device=rollout.dev)
            w = rollout._queued(lambda: rollout._walk(
                False, int(every), states, ticks, s0[:, 0:3], s0[:, 3:6], s0[:, 6:9], None if push is None else push.detach().to(rollout.dev, torch.float32), push_ticks,
                replan, False, ("merge", "solver", "nonfinite"), False, mismatch=mm))
            rollout.last_walk = ctx.walk = w
            ctx.dtypes = (state0.dtype, None if push is None else push.dtype)
            e = w["end_tick"]
            row = torch.arange(ticks + 1, device=rollout.dev)[:, None]
            ctx.past = (e[None, :] >= 0) & (row > e[None, :])         # [ticks + 1, B]: rows behind a problem's end
            ctx.last = row == e[None, :]                                # the row its final state sits in
            return torch.where(ctx.past[..., None], w["final_state"][None], states)

        @staticmethod
        def backward(ctx, gStates):
            g = gStates.to(rollout.dev, torch.float64)
            folded = torch.where(ctx.past[..., None], g, torch.zeros_like(g)).sum(0)     # (zero for a problem that walked to the end)
            g = torch.where(ctx.last[..., None], g + folded[None], g).contiguous()
            r = rollout.backward_device_checkpointed_mismatch(ctx.walk, g)
            rollout.last_backward = r
            mg = lambda i, key, rows: (r[key][:ctx.mm_meta[i][1]] if rows else r[key]).to(ctx.mm_meta[i][0]) \
                if ctx.mm_meta[i] is not None and ctx.needs_input_grad[3 + i] else None
            return (r["state0"].to(ctx.dtypes[0]), None if ctx.dtypes[1] is None else r["push"].to(ctx.dtypes[1]),
                    r["models"] if ctx.needs_input_grad[2] else None,
                    # (a schedule shorter than the walk: the rows behind it have no input)
                    mg(0, "hidden_wrench", True), mg(1, "state_noise", True), mg(2, "force_gain", False))

    return _Fn.apply(state0, push, models, hidden_wrench, state_noise, force_gain)


def _rollout_differentiable_device(rollout, ticks, state0, push, models, push_ticks, replan, plan_rot=None, ref_com=None, ref_h=None, mismatch=None):
    """rollout_differentiable(device_walk=True); mismatch: None, or (hidden_wrench, state_noise, force_gain), each a tensor or None"""
    import torch
    hidden, noise, gain = mismatch if mismatch is not None else (None, None, None)

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, state0, push, models, plan_rot, ref_com, ref_h, hidden, noise, gain):
            mm = None
            if mismatch is not None:
                det = lambda a: None if a is None else a.detach().to(rollout.dev, torch.float32).contiguous()
                mm = dict(hidden_wrench=det(hidden), state_noise=det(noise), force_gain=det(gain), tick_first=0)
            ctx.mm_meta = tuple(None if a is None else (a.dtype, int(a.shape[0])) for a in (hidden, noise, gain))
            assert all(a is None or 1 <= a.shape[0] <= ticks for a in (hidden, noise)), "hidden_wrench / state_noise: between 1 and `ticks` rows"
            if models is not None:
                rollout.models = models.detach().to(rollout.dev, torch.float64).contiguous()
                rollout.models_ok = rollout.solver.set_models_device(rollout.models)
            s0 = state0.detach().to(rollout.dev, torch.float32)
            plan, plans = rollout.plan, replan
            ctx.jr = None
            ctx.refs = ref_com is not None or ref_h is not None
            ctx.ref_dtypes = (None if ref_com is None else ref_com.dtype, None if ref_h is None else ref_h.dtype)
            as32 = lambda a: None if a is None else a.detach().to(rollout.dev, torch.float32).contiguous()
            if ctx.refs:
                rollout._ref_override = (as32(ref_com), as32(ref_h))
            if plan_rot is not None:     # (the planner's contacts of every segment turn by the same vectors: the one plan_rot buffer sums over them)
                om = plan_rot.detach().to(rollout.dev, torch.float64)
                assert tuple(om.shape) == tuple(plan[1].shape[:3]) + (3,), f"plan_rot: expected {tuple(plan[1].shape[:3]) + (3,)}"
                rollout.plan = (plan[0], rot_plan_poses(plan[1], om), plan[2])
                plans = None if replan is None else {t: (p[0], rot_plan_poses(p[1], om), p[2]) for t, p in replan.items()}
                ctx.jr = so3_right_jacobian(om)
            try:
                w = rollout.walk_device_taped(ticks, s0[:, 0:3], s0[:, 3:6], s0[:, 6:9],
                                              push=None if push is None else push.detach().to(rollout.dev, torch.float32), push_ticks=push_ticks,
                                              replan=plans, trace=False, mismatch=mm)
            finally:
                rollout.plan = plan
                rollout._ref_override = None
            rollout.last_walk = ctx.walk = w
            ctx.dtypes = (state0.dtype, None if push is None else push.dtype)
            e = w["end_tick"]
            row = torch.arange(ticks + 1, device=rollout.dev)[:, None]
            ctx.past = (e[None, :] >= 0) & (row > e[None, :])         # [ticks + 1, B]: rows behind a problem's end
            ctx.last = row == e[None, :]                                # the row its final state sits in
            return torch.where(ctx.past[..., None], w["final_state"][None], w["tape"]["states"])

        @staticmethod
        def backward(ctx, gStates):
            g = gStates.to(rollout.dev, torch.float64)
            folded = torch.where(ctx.past[..., None], g, torch.zeros_like(g)).sum(0)     # (zero for a problem that walked to the end)
            g = torch.where(ctx.last[..., None], g + folded[None], g).contiguous()
            if ctx.refs:
                r = rollout.backward_device_refs(ctx.walk, g, rot=ctx.jr is not None)
            else:
                r = rollout.backward_device(ctx.walk, g) if ctx.jr is None else rollout.backward_device_rot(ctx.walk, g)
            rollout.last_backward = r
            return (r["state0"].to(ctx.dtypes[0]), None if ctx.dtypes[1] is None else r["push"].to(ctx.dtypes[1]),
                    r["models"] if ctx.needs_input_grad[2] else None,
                    _jr_transposed(ctx.jr, r["plan_rot"] + r["list_rot0"]) if ctx.jr is not None and ctx.needs_input_grad[3] else None,
                    r["ref_com"].to(ctx.ref_dtypes[0]) if ctx.ref_dtypes[0] is not None and ctx.needs_input_grad[4] else None,
                    r["ref_h"].to(ctx.ref_dtypes[1]) if ctx.ref_dtypes[1] is not None and ctx.needs_input_grad[5] else None,
                    # (a schedule shorter than the walk: the rows behind it have no input; a tape without a mismatch has none of the keys)
                    r["hidden_wrench"][:ctx.mm_meta[0][1]].to(ctx.mm_meta[0][0]) if ctx.mm_meta[0] is not None and ctx.needs_input_grad[6] else None,
                    r["state_noise"][:ctx.mm_meta[1][1]].to(ctx.mm_meta[1][0]) if ctx.mm_meta[1] is not None and ctx.needs_input_grad[7] else None,
                    r["force_gain"].to(ctx.mm_meta[2][0]) if ctx.mm_meta[2] is not None and ctx.needs_input_grad[8] else None)

        @staticmethod
        def jvp(ctx, t_state0, t_push, t_models, t_rot, t_ref_com, t_ref_h, t_hidden=None, t_noise=None, t_gain=None):
            if mismatch is not None:
                raise NotImplementedError("rollout_differentiable: forward mode under a plant mismatch is WalkingRollout.forward_sensitivity_device_mismatch "
                                          "on rollout.last_walk")
            """torch.autograd.forward_ad: forward_sensitivity_device at k = 1 on the tape the forward left.  The returned states hold final_state in the
            rows behind a problem's end, so those rows take the tangent of the row its final state sits in: the transpose of backward's fold."""
            col = lambda t, dt: None if t is None else t.detach().to(rollout.dev, dt)[:, None].contiguous()
            if all(t is None for t in (t_state0, t_push, t_models, t_rot, t_ref_com, t_ref_h)):
                return torch.zeros((ticks + 1, rollout.B, 9), dtype=torch.float32, device=rollout.dev)
            drot = None if t_rot is None else _jr_applied(ctx.jr, t_rot.detach().to(rollout.dev, torch.float64))[:, None].contiguous()
            dirs = dict(dir_state0=col(t_state0, torch.float64), dir_push=col(t_push, torch.float32), dir_models=col(t_models, torch.float64),
                        dir_plan_rot=drot, dir_list_rot0=drot)
            if t_ref_com is not None or t_ref_h is not None:
                r = rollout.forward_sensitivity_device_refs(ctx.walk, dir_ref_com=col(t_ref_com, torch.float64), dir_ref_h=col(t_ref_h, torch.float64), **dirs)
            else:
                r = rollout.forward_sensitivity_device(ctx.walk, **dirs)
            rollout.last_forward = r
            t = r["states"][:, :, 0]
            e = ctx.walk["end_tick"].to(torch.int64).clamp(min=0)
            at_end = t.gather(0, e[None, :, None].expand(1, rollout.B, 9))      # [1, B, 9]: each problem's row e (row 0 where it never ended: not selected)
            return torch.where(ctx.past[..., None], at_end, t).to(torch.float32)

    return _Fn.apply(state0, push, models, plan_rot, ref_com, ref_h, hidden, noise, gain)


def rollout_differentiable_measures(rollout: WalkingRollout, ticks, state0, push=None, models=None, push_ticks=0, replan=None, ref_com=None, ref_h=None,
                                    hidden_wrench=None, state_noise=None, force_gain=None):
    """rollout_differentiable(device_walk=True) that also returns the walk's stability measures, differentiably: -> (states [ticks + 1, B, 9],
    measures [ticks, B, 4]) float32 -- height, reach, margin, track of every tick (include/cmpc.h, "physical limits") as the walk's trace holds them: the
    row that ended a problem is included, its later rows are NaN, and so are the rows a code 1..5 ended.  The device walk only.  The measures trace is
    turned on for this walk under the roll-out's current limits -- none set: every limit off, nobody ends by one; limits set (set_limits): a robot beyond
    one ENDS, as with "limits" in stop= -- and the setting is restored afterwards.  backward is WalkingRollout.backward_device_measures with the
    states' fold of rollout_differentiable (refs with ref_com / ref_h): the cotangents of the measure rows at or past a problem's end are not read,
    so a loss may mask them or not.  Forward mode (torch.autograd.forward_ad over state0, push and models) is
    WalkingRollout.forward_sensitivity_device_measures at k = 1: the tangents of the measure rows at or past a problem's end are zero; under a plant
    mismatch, or with tangents on ref_com / ref_h, it raises NotImplementedError.  The other arguments, rollout.last_walk / last_backward /
    last_forward as in rollout_differentiable.  No plan_rot and no plan_yaw: the measures' own dependence on the stage-1 rotations is returned by
    backward_device_measures (measure_rot) and not chained into the planner's orientations."""
    import torch
    mismatch = (hidden_wrench, state_noise, force_gain) if any(a is not None for a in (hidden_wrench, state_noise, force_gain)) else None

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, state0, push, models, ref_com, ref_h, hidden, noise, gain):
            mm = None
            if mismatch is not None:
                det = lambda a: None if a is None else a.detach().to(rollout.dev, torch.float32).contiguous()
                mm = dict(hidden_wrench=det(hidden), state_noise=det(noise), force_gain=det(gain), tick_first=0)
            ctx.mm_meta = tuple(None if a is None else (a.dtype, int(a.shape[0])) for a in (hidden, noise, gain))
            assert all(a is None or 1 <= a.shape[0] <= ticks for a in (hidden, noise)), "hidden_wrench / state_noise: between 1 and `ticks` rows"
            if models is not None:
                rollout.models = models.detach().to(rollout.dev, torch.float64).contiguous()
                rollout.models_ok = rollout.solver.set_models_device(rollout.models)
            s0 = state0.detach().to(rollout.dev, torch.float32)
            ctx.refs = ref_com is not None or ref_h is not None
            ctx.ref_dtypes = (None if ref_com is None else ref_com.dtype, None if ref_h is None else ref_h.dtype)
            as32 = lambda a: None if a is None else a.detach().to(rollout.dev, torch.float32).contiguous()
            if ctx.refs:
                rollout._ref_override = (as32(ref_com), as32(ref_h))
            limits = rollout.limits
            stop = ("merge", "solver", "nonfinite") + (("limits",) if limits is not None else ())
            if limits is None:
                rollout.set_limits()
            try:
                w = rollout.walk_device_taped(ticks, s0[:, 0:3], s0[:, 3:6], s0[:, 6:9],
                                              push=None if push is None else push.detach().to(rollout.dev, torch.float32), push_ticks=push_ticks,
                                              replan=replan, trace=True, stop=stop, mismatch=mm)
            finally:
                rollout.limits = limits
                rollout._ref_override = None
            rollout.last_walk = ctx.walk = w
            ctx.dtypes = (state0.dtype, None if push is None else push.dtype)
            e = w["end_tick"]
            row = torch.arange(ticks + 1, device=rollout.dev)[:, None]
            ctx.past = (e[None, :] >= 0) & (row > e[None, :])         # [ticks + 1, B]: rows behind a problem's end
            ctx.last = row == e[None, :]                                # the row its final state sits in
            return torch.where(ctx.past[..., None], w["final_state"][None], w["tape"]["states"]), w["measures"].clone()

        @staticmethod
        def backward(ctx, gStates, gMeasures):
            g = gStates.to(rollout.dev, torch.float64)
            folded = torch.where(ctx.past[..., None], g, torch.zeros_like(g)).sum(0)     # (zero for a problem that walked to the end)
            g = torch.where(ctx.last[..., None], g + folded[None], g).contiguous()
            r = rollout.backward_device_measures(ctx.walk, gMeasures.to(rollout.dev, torch.float64).contiguous(), g, refs=ctx.refs)
            rollout.last_backward = r
            return (r["state0"].to(ctx.dtypes[0]), None if ctx.dtypes[1] is None else r["push"].to(ctx.dtypes[1]),
                    r["models"] if ctx.needs_input_grad[2] else None,
                    r["ref_com"].to(ctx.ref_dtypes[0]) if ctx.ref_dtypes[0] is not None and ctx.needs_input_grad[3] else None,
                    r["ref_h"].to(ctx.ref_dtypes[1]) if ctx.ref_dtypes[1] is not None and ctx.needs_input_grad[4] else None,
                    r["hidden_wrench"][:ctx.mm_meta[0][1]].to(ctx.mm_meta[0][0]) if ctx.mm_meta[0] is not None and ctx.needs_input_grad[5] else None,
                    r["state_noise"][:ctx.mm_meta[1][1]].to(ctx.mm_meta[1][0]) if ctx.mm_meta[1] is not None and ctx.needs_input_grad[6] else None,
                    r["force_gain"].to(ctx.mm_meta[2][0]) if ctx.mm_meta[2] is not None and ctx.needs_input_grad[7] else None)

        @staticmethod
        def jvp(ctx, t_state0, t_push, t_models, t_ref_com, t_ref_h, t_hidden=None, t_noise=None, t_gain=None):
            if mismatch is not None:
                raise NotImplementedError("rollout_differentiable_measures: forward mode under a plant mismatch is not implemented")
            if t_ref_com is not None or t_ref_h is not None:
                raise NotImplementedError("rollout_differentiable_measures: forward mode takes no tangent on ref_com / ref_h")
            zero = (torch.zeros((ticks + 1, rollout.B, 9), dtype=torch.float32, device=rollout.dev),
                    torch.zeros((ticks, rollout.B, 4), dtype=torch.float32, device=rollout.dev))
            if all(t is None for t in (t_state0, t_push, t_models)):
                return zero
            col = lambda t, dt: None if t is None else t.detach().to(rollout.dev, dt)[:, None].contiguous()
            r = rollout.forward_sensitivity_device_measures(ctx.walk, dir_state0=col(t_state0, torch.float64), dir_push=col(t_push, torch.float32),
                                                            dir_models=col(t_models, torch.float64))
            rollout.last_forward = r
            t = r["states"][:, :, 0]
            e = ctx.walk["end_tick"].to(torch.int64).clamp(min=0)
            at_end = t.gather(0, e[None, :, None].expand(1, rollout.B, 9))      # [1, B, 9]: each problem's row e (row 0 where it never ended: not selected)
            return torch.where(ctx.past[..., None], at_end, t).to(torch.float32), r["measures"][:, :, 0].to(torch.float32)

    return _Fn.apply(state0, push, models, ref_com, ref_h, hidden_wrench, state_noise, force_gain)


def rollout_differentiable_checkpointed(rollout: WalkingRollout, ticks, state0, every, push=None, models=None, push_ticks=0, replan=None):
    """rollout_differentiable(device_walk=True) in bounded memory: forward is WalkingRollout.walk_device_checkpointed (cut at every tick besides, so
    that the states [ticks + 1, B, 9] can be copied out: 36 bytes per problem and tick; still no host read), backward is
    WalkingRollout.backward_device_checkpointed -- no whole-walk tape exists at any time, only a snapshot every `every` ticks and one tape of
    every + 1 rows.  The returned states, and state0.grad, push.grad and models.grad, equal rollout_differentiable(device_walk=True)'s to the bit; the
    fold of the rows behind a problem's end is the same.  rollout.last_walk / rollout.last_backward as there.  Not here: plan_rot, ref_com / ref_h
    (backward_device_refs is out of scope of the checkpointed reverse walk) and forward mode.  Under a plant mismatch:
    rollout_differentiable_checkpointed_mismatch."""
    return rollout_differentiable_checkpointed_mismatch(rollout, ticks, state0, every, push=push, models=models, push_ticks=push_ticks, replan=replan)
