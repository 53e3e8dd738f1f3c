"""The torch.autograd.Function wrappers of the roll-out and the rotation helpers they need, re-exported by rollout.py.  What the four Function
classes share is written once, as the module functions in front: models, mismatch, reference override, end masks, fold, select, the gradients' casts."""
from __future__ import annotations

from typing import TYPE_CHECKING

from .rollout_common import need, tensor

if TYPE_CHECKING:
    from .rollout import WalkingRollout


def _detached(rollout, a, dtype):
    return None if a is None else tensor(a.detach(), rollout.dev, dtype)


def _column(rollout, t, dtype):      # (a tangent [B, ..] as the k = 1 direction [B, 1, ..])
    return None if t is None else t.detach().to(rollout.dev, dtype)[:, None].contiguous()


def _plan_rotation(rollout, plan, plan_rot):
    import torch
    om = plan_rot.detach().to(rollout.dev, torch.float64)
    need(tuple(om.shape) == tuple(plan[1].shape[:3]) + (3,), f"plan_rot: expected {tuple(plan[1].shape[:3]) + (3,)}")
    return om


def _install_models(rollout, models):      # (left installed)
    if models is not None:
        import torch
        rollout.models = _detached(rollout, models, torch.float64)
        rollout.models_ok = rollout.solver.set_models_device(rollout.models)


def _mismatch_of(rollout, ctx, ticks, hidden, noise, gain):
    """-> walk_device_mismatch's dict of the detached parts with tick_first = 0, None when none is given; ctx.mm_meta = each part's (dtype, rows), or None"""
    import torch
    mm = None
    if hidden is not None or noise is not None or gain is not None:
        mm = dict(hidden_wrench=_detached(rollout, hidden, torch.float32), state_noise=_detached(rollout, noise, torch.float32),
                  force_gain=_detached(rollout, gain, torch.float32), tick_first=0)
    ctx.mm_meta = tuple(None if a is None else (a.dtype, int(a.shape[0])) for a in (hidden, noise, gain))
    need(all(a is None or 1 <= a.shape[0] <= ticks for a in (hidden, noise)), "hidden_wrench / state_noise: between 1 and `ticks` rows")
    return mm


def _override_references(rollout, ctx, ref_com, ref_h):      # (the caller's `finally` takes the override back)
    import torch
    ctx.refs = ref_com is not None or ref_h is not None
    ctx.ref_dtypes = (None if ref_com is None else ref_com.dtype, None if ref_h is None else ref_h.dtype)
    if ctx.refs:
        rollout._ref_override = (_detached(rollout, ref_com, torch.float32), _detached(rollout, ref_h, torch.float32))


def _walked(rollout, ctx, ticks, w, state0, push):      # (what every forward keeps of its walk: last_walk, the inputs' dtypes, the end masks)
    import torch
    rollout.last_walk = ctx.walk = w
    ctx.dtypes = (state0.dtype, None if push is None else push.dtype)
    e = w["end_tick"]
    row = torch.arange(ticks + 1, device=rollout.dev)[:, None]
    ctx.past = (e[None, :] >= 0) & (row > e[None, :])         # [ticks + 1, B]: rows behind a problem's end
    ctx.last = row == e[None, :]                                # the row its final state sits in


def _folded(rollout, ctx, gStates):
    """the states' cotangents with those of the rows behind a problem's end folded into the row its final state sits in"""
    import torch
    g = gStates.to(rollout.dev, torch.float64)
    folded = torch.where(ctx.past[..., None], g, torch.zeros_like(g)).sum(0)     # (zero for a problem that walked to the end)
    return torch.where(ctx.last[..., None], g + folded[None], g).contiguous()


def _selected(rollout, ctx, t):
    """the states' tangents t [ticks + 1, B, 9], the rows behind a problem's end taking that of the row its final state sits in: _folded's transpose"""
    import torch
    e = ctx.walk["end_tick"].to(torch.int64).clamp(min=0)
    at_end = t.gather(0, e[None, :, None].expand(1, rollout.B, 9))      # [1, B, 9]: each problem's row e (row 0 where it never ended: not selected)
    return torch.where(ctx.past[..., None], at_end, t).to(torch.float32)


def _input_grads(ctx, r):
    return (r["state0"].to(ctx.dtypes[0]), None if ctx.dtypes[1] is None else r["push"].to(ctx.dtypes[1]), r["models"] if ctx.needs_input_grad[2] else None)


def _ref_grads(ctx, r, first):      # (ref_com and ref_h are inputs first and first + 1 of the Function)
    return tuple(r[key].to(ctx.ref_dtypes[i]) if ctx.ref_dtypes[i] is not None and ctx.needs_input_grad[first + i] else None
                 for i, key in enumerate(("ref_com", "ref_h")))


def _mismatch_grads(ctx, r, first):
    """inputs first .. first + 2 of the Function: a schedule shorter than the walk has no input for the rows behind it; no mismatch, no keys"""
    meta = ctx.mm_meta
    return tuple(None if meta[i] is None or not ctx.needs_input_grad[first + i] else (r[k][:meta[i][1]] if i < 2 else r[k]).to(meta[i][0])
                 for i, k in enumerate(("hidden_wrench", "state_noise", "force_gain")))


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
            _install_models(rollout, models)
            s0 = state0.detach().to(torch.float32).cpu().numpy()
            plan = rollout.plan
            if plan_yaw is not None:
                psi = plan_yaw.detach().to(rollout.dev, torch.float64)
                need(tuple(psi.shape) == tuple(plan[1].shape[:3]), f"plan_yaw: expected {tuple(plan[1].shape[:3])}")
                rollout.plan = (plan[0], yaw_plan_poses(plan[1], psi), plan[2])
            ctx.jr = None
            if plan_rot is not None:
                om = _plan_rotation(rollout, plan, plan_rot)
                rollout.plan = (plan[0], rot_plan_poses(plan[1], om), plan[2])
                ctx.jr = so3_right_jacobian(om)
            try:
                rec = rollout.run(ticks, s0[:, 0:3], s0[:, 3:6], s0[:, 6:9], push=None if push is None else push.detach().to(torch.float32).cpu().numpy(),
                                  push_ticks=push_ticks, record="light", tape=True)
            finally:
                rollout.plan = plan
            ctx.rot = plan_yaw is not None or plan_rot is not None
            tape = rec["tape"]
            need(len(tape["ticks"]) == ticks, f"the roll-out stopped at tick {rec.get('aborted_tick')}")
            rollout.last_tape = ctx.tape = tape
            ctx.dtypes = (state0.dtype, None if push is None else push.dtype)
            return torch.stack([tk["state"] for tk in tape["ticks"]] + [tape["state"]])

        @staticmethod
        def backward(ctx, gStates):
            r = rollout.backward(ctx.tape, gStates, rot=ctx.rot)
            rollout.last_backward = r
            return _input_grads(ctx, r) + (
                (r["plan_rot"][..., 2] + r["list_rot0"][..., 2]) if ctx.rot and ctx.needs_input_grad[3] else None,
                _jr_transposed(ctx.jr, r["plan_rot"] + r["list_rot0"]) if ctx.jr is not None and ctx.needs_input_grad[4] else None)

        @staticmethod
        def jvp(ctx, t_state0, t_push, t_models, t_yaw, t_rot):
            """torch.autograd.forward_ad: forward_sensitivity at k = 1 on the tape the forward left.  A yaw tangent is d psi e_z on the planner's
            orientations and on the first tick's list, the transpose of what backward returns for plan_yaw."""
            col = lambda t, dt: _column(rollout, t, dt)
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
            mm = _mismatch_of(rollout, ctx, ticks, hidden, noise, gain)
            _install_models(rollout, models)
            s0 = state0.detach().to(rollout.dev, torch.float32)
            states = torch.zeros((ticks + 1, rollout.B, 9), dtype=torch.float32, device=rollout.dev)
            w = rollout._queued(lambda: rollout._walk(
                False, int(every), states, ticks, s0[:, 0:3], s0[:, 3:6], s0[:, 6:9], None if push is None else push.detach().to(rollout.dev, torch.float32), push_ticks,
                replan, False, ("merge", "solver", "nonfinite"), False, mismatch=mm))
            _walked(rollout, ctx, ticks, w, state0, push)
            return torch.where(ctx.past[..., None], w["final_state"][None], states)

        @staticmethod
        def backward(ctx, gStates):
            r = rollout.backward_device_checkpointed_mismatch(ctx.walk, _folded(rollout, ctx, gStates))
            rollout.last_backward = r
            return _input_grads(ctx, r) + _mismatch_grads(ctx, r, 3)

    return _Fn.apply(state0, push, models, hidden_wrench, state_noise, force_gain)


def _rollout_differentiable_device(rollout, ticks, state0, push, models, push_ticks, replan, plan_rot=None, ref_com=None, ref_h=None, mismatch=None):
    """rollout_differentiable(device_walk=True); mismatch: None, or (hidden_wrench, state_noise, force_gain), each a tensor or None"""
    import torch
    hidden, noise, gain = mismatch if mismatch is not None else (None, None, None)

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, state0, push, models, plan_rot, ref_com, ref_h, hidden, noise, gain):
            mm = _mismatch_of(rollout, ctx, ticks, hidden, noise, gain)
            _install_models(rollout, models)
            s0 = state0.detach().to(rollout.dev, torch.float32)
            plan, plans = rollout.plan, replan
            ctx.jr = None
            _override_references(rollout, ctx, ref_com, ref_h)
            if plan_rot is not None:     # (the planner's contacts of every segment turn by the same vectors: the one plan_rot buffer sums over them)
                om = _plan_rotation(rollout, plan, plan_rot)
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
            _walked(rollout, ctx, ticks, w, state0, push)
            return torch.where(ctx.past[..., None], w["final_state"][None], w["tape"]["states"])

        @staticmethod
        def backward(ctx, gStates):
            g = _folded(rollout, ctx, gStates)
            if ctx.refs:
                r = rollout.backward_device_refs(ctx.walk, g, rot=ctx.jr is not None)
            else:
                r = rollout.backward_device(ctx.walk, g) if ctx.jr is None else rollout.backward_device_rot(ctx.walk, g)
            rollout.last_backward = r
            return _input_grads(ctx, r) + (
                _jr_transposed(ctx.jr, r["plan_rot"] + r["list_rot0"]) if ctx.jr is not None and ctx.needs_input_grad[3] else None,
            ) + _ref_grads(ctx, r, 4) + _mismatch_grads(ctx, r, 6)

        @staticmethod
        def jvp(ctx, t_state0, t_push, t_models, t_rot, t_ref_com, t_ref_h, t_hidden=None, t_noise=None, t_gain=None):
            if mismatch is not None:
                raise NotImplementedError("rollout_differentiable: forward mode under a plant mismatch is WalkingRollout.forward_sensitivity_device_mismatch "
                                          "on rollout.last_walk")
            """torch.autograd.forward_ad: forward_sensitivity_device at k = 1 on the tape the forward left.  The returned states hold final_state in the
            rows behind a problem's end, so those rows take the tangent of the row its final state sits in: the transpose of backward's fold."""
            col = lambda t, dt: _column(rollout, t, dt)
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
            return _selected(rollout, ctx, r["states"][:, :, 0])

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
            mm = _mismatch_of(rollout, ctx, ticks, hidden, noise, gain)
            _install_models(rollout, models)
            s0 = state0.detach().to(rollout.dev, torch.float32)
            _override_references(rollout, ctx, ref_com, ref_h)
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
            _walked(rollout, ctx, ticks, w, state0, push)
            return torch.where(ctx.past[..., None], w["final_state"][None], w["tape"]["states"]), w["measures"].clone()

        @staticmethod
        def backward(ctx, gStates, gMeasures):
            g = _folded(rollout, ctx, gStates)
            r = rollout.backward_device_measures(ctx.walk, gMeasures.to(rollout.dev, torch.float64).contiguous(), g, refs=ctx.refs)
            rollout.last_backward = r
            return _input_grads(ctx, r) + _ref_grads(ctx, r, 3) + _mismatch_grads(ctx, r, 5)

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
            col = lambda t, dt: _column(rollout, t, dt)
            r = rollout.forward_sensitivity_device_measures(ctx.walk, dir_state0=col(t_state0, torch.float64), dir_push=col(t_push, torch.float32),
                                                            dir_models=col(t_models, torch.float64))
            rollout.last_forward = r
            return _selected(rollout, ctx, r["states"][:, :, 0]), r["measures"][:, :, 0].to(torch.float32)

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
