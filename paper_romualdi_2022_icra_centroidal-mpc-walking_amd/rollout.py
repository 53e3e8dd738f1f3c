"""Receding-horizon walking roll-out of a whole batch, resident in HBM: every tick is what the reference's two blocks do
between them -- merge the planner's footsteps with the MPC-adjusted current contact (updateContactPhaseList,
CentroidalMPCBlock.cpp:594-607), sample the list into the MPC's parameters (setContactPhaseList :609), feed the measured
state (setState :407), warm-start from the shifted previous solution (is_warm_start_enabled), solve (advance :615), write
the optimised landing position back into the list (getOutput :626) and integrate the centroidal dynamics under the
first-knot forces until the next tick (WholeBodyQPBlock.cpp:1083-1150) -- as seven launches on one stream through the
C ABI (include/cmpc.h); torch only owns the buffers.  SURVEY 8f-1 .. 8f-4 chained.  Here: the constructor and the HOST-STEPPED path; the device
walks, refill walks, device derivatives and autograd wrappers are rollout_walk / _refill / _grad / _autograd.py, re-exported here."""
from __future__ import annotations

import inspect  # noqa: F401  (every name this module had is still reached through it)

import numpy as np

from .config import GRAVITY

from .contacts import PlannedContact, pack_lists
from .layout import Layout
from .rollout_autograd import (_jr_applied, _jr_transposed, _rollout_differentiable_device, rollout_differentiable,  # noqa: F401
                               rollout_differentiable_checkpointed, rollout_differentiable_checkpointed_mismatch, rollout_differentiable_measures,
                               rot_plan_poses, so3_right_jacobian, yaw_plan_poses)
from .rollout_common import LaunchStream, direction, need, plan_speed, seed, tensor, walk_schedule  # noqa: F401
from .rollout_grad import WalkGrads
from .rollout_refill import RefillWalks
from .rollout_walk import DeviceWalks
from .solver import BatchSolver, _model_array, _upload  # noqa: F401

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


class WalkingRollout(LaunchStream, DeviceWalks, RefillWalks, WalkGrads):
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
        need(retry in ("kernel", "launch", None), 'retry: expected "kernel", "launch" or None')
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
        self.com_speed = plan_speed(plan) if com_speed is None else com_speed   # (the plan's mean walking speed, for the CoM reference)
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
        need(h is not None and in_dt is not None and float(in_dt) > 0 and float(robot_mass) > 0, "set_references(com, h, in_dt, ...)")
        com, h = tensor(com, self.dev, torch.float32, np.float32), tensor(h, self.dev, torch.float32, np.float32)
        need(com.dim() == 3 and com.shape[0] == self.B and com.shape[1] >= 2 and com.shape[2] == 3 and h.shape == com.shape, f"set_references: com and h of shape [{self.B}, n >= 2, 3]")
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
        need(com.shape == h.shape and tuple(com.shape) == (B, com.shape[1], 3) and com.shape[1] >= 2, "reference trajectories: com and h of one shape [B, n, 3]")
        return (com, h) + rest

    def run(self, *args, **kwargs):
        """The roll-out (see _run for the arguments), with the solver's launch stream as torch's current stream: every device call of a tick -- the library's
        kernels and the torch ops between them -- is then queued on ONE non-default stream, in order, without the event dependencies a call from the default
        stream needs (BatchSolver._stream_pair: two per call, ~24 us of idle GPU each time)."""
        if kwargs.pop("mismatch", None) is not None:
            raise NotImplementedError("run(): a plant mismatch is taken by the device walk only (walk_device_mismatch, walk_device_taped(mismatch=...))")
        return self._on_launch_stream(lambda: self._run(*args, **kwargs))

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
        dt, dev, s = cfg.sampling_time, self.dev, self.solver
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
            need(self.retry != "launch", "tape=True needs retry='kernel' or None")
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
        gS = seed(grad_states, self.dev, torch.float64, (T + 1, B, 9), "grad_states")
        gX = None if grad_X is None else seed(grad_X, self.dev, torch.float32, (T, B, L.nx), "grad_X")
        M, z = ticks[0]["list_t"].shape[2], self._z
        out = dict(push=z((B, 3)), wrench=z((T, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((T, B), torch.int32))
        if rot:
            out.update(plan_rot=z((B, 2, M, 3)), rot=z((T, B, 2, N, 3)), removed=z((T, B), torch.float32))

        def reverse():
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
            return out
        return self._on_launch_stream(reverse)

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
        as_dir = lambda a, dtype, tail, lead=(): direction(a, self.dev, B, dtype, tail, lead)
        f32, f64, z = torch.float32, torch.float64, self._z
        ds, dl, dlr = as_dir(dir_state0, f64, (9,)), as_dir(dir_list0, f64, (2, M, 3)), as_dir(dir_list_rot0, f64, (2, M, 3))
        dpl, dplr = as_dir(dir_plan, f64, (2, M, 3)), as_dir(dir_plan_rot, f64, (2, M, 3))
        dpush, dmod, dwr = as_dir(dir_push, f32, (3,)), as_dir(dir_models, f64, (34,)), as_dir(dir_wrench, f32, (N, 6), lead=(T,))
        ks = {int(a.shape[1]) for a in (ds, dl, dlr, dpl, dplr, dpush, dmod) if a is not None} | ({int(dwr.shape[2])} if dwr is not None else set())
        need(len(ks) == 1, "forward_sensitivity: no direction, or directions of different k")
        k = ks.pop()
        rot = dlr is not None or dplr is not None
        out = dict(states=z((T + 1, B, k, 9)), status=z((T, B), torch.int32), removed=z((T, B), f32))
        if solutions:
            out["X"] = z((T, B, k, L.nx), f32)

        def forward(ds, dl, dlr):
            if ds is not None:
                out["states"][0] = ds
            for i, tk in enumerate(ticks):
                w = None if dwr is None else dwr[i]
                if dpush is not None and tk["push_knots"] > 0:
                    w = z((B, k, N, 6), f32) if w is None else w.clone()
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
            out["list_rot"] = dlr if rot else z((B, k, 2, M, 3))
            return out
        return self._on_launch_stream(lambda: forward(ds, dl, dlr))
