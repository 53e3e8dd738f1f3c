"""The reverse device walk with the contacts' orientations carried along (include/cmpc.h: cmpc_rollout_walk_vjp_rot_device and its gate;
WalkingRollout.backward_device_rot, rollout_differentiable(plan_rot=...)).  Comparisons of bits -- the gate kernel against the host form, the reverse walk
against run(tape=True) + backward(rot=True) and against backward_device, one call against two segments, an ended problem against the shorter walk it
amounts to, the autograd entry on the device path against the host path -- but for one adjoint identity against forward_sensitivity_device, held to
5 x ADJ (five chained ticks of tests/test_gpu_rollout_jvp.py's per-tick bound, which covers the rotation groups).
N = 10, dt = 0.06, the ergoCubGazeboV1 weights, the footsteps after each foot's first yawed U(-0.2, 0.2) rad per problem; the autograd tests run on the
landing scene of tests/test_gpu_rollout_rot_adjoint.py (N = 20, B = 8, 6 ticks)."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_tape_ref as wt
from tests.test_gpu_rollout_jvp import ADJ
from tests.test_gpu_walk_tape import _same_bits, _start

so3_right_jacobian, yaw_plan_poses = cm.rollout.so3_right_jacobian, cm.rollout.yaw_plan_poses

pytestmark = pytest.mark.gpu

N = 10
GRADS = ("state0", "list0", "wrench", "push", "models", "plan", "status")
ROT = ("list_rot0", "plan_rot", "rot", "removed")


def _cfg():
    return cm.config.ergocub_gazebo_v1(N, 0.06)


def _yawed(cfg, B, seed=21):
    """a roll-out whose planner's footsteps after each foot's first are yawed U(-0.2, 0.2) rad per problem"""
    import torch
    ro = cm.rollout.WalkingRollout(cfg, B)
    yaw = np.zeros((B, 2, ro.M))
    yaw[:, :, 1:] = np.random.default_rng(seed).uniform(-0.2, 0.2, (B, 2, ro.M - 1))
    ro.plan = (ro.plan[0], yaw_plan_poses(ro.plan[1], torch.from_numpy(yaw).to(ro.dev)), ro.plan[2])
    return ro


def _host(r, keys):
    return {k: r[k].cpu().numpy() for k in keys}


# ---- 1. the gate kernel against the host form ----
@pytest.mark.parametrize("B", [70, 300])
def test_gate_kernel_matches_the_host_form(B):
    """the three kinds of gate step with random end ticks and NaN in everything the tick left for an ended problem (and, in the first step of a call, in
    its carries): all five carries and rows, and the base's, against the host form to the bit.  B = 70 is a partial second wave, B = 300 a second
    workgroup"""
    import torch
    from tests.test_walk_tape_cpu import _ptr
    cfg = _cfg()
    s, L, M, T = cm.BatchSolver(cfg, B), cm.Layout(N), 4, 6
    lib = cm._capi.lib()
    rng = np.random.default_rng(B)
    e = rng.integers(-1, T + 1, B).astype(np.int32)
    assert (e == -1).any() and (e == 0).any() and (e == T).any()
    e_d = torch.from_numpy(e).cuda()
    for kind, t_post, gx in [("pre", T, True), ("pre", 3, False), ("both", 3, True), ("both", 1, False), ("post", 0, True)]:
        en_post = wt.ended(e, t_post)
        h = dict(seed=rng.normal(size=(B, 9)), t_state=rng.normal(size=(B, 9)), t_list=rng.normal(size=(B, 2, M, 3)), t_list_rot=rng.normal(size=(B, 2, M, 3)),
                 t_sens=rng.integers(0, 6, (B, 8)).astype(np.float32), carry_state=rng.normal(size=(B, 9)), carry_list=rng.normal(size=(B, 2, M, 3)),
                 carry_list_rot=rng.normal(size=(B, 2, M, 3)), wrench=rng.normal(size=(B, N, 6)).astype(np.float32),
                 gp=rng.normal(size=(B, L.np)).astype(np.float32), rot=rng.normal(size=(B, 2, N, 3)), status=np.full((B,), -9, np.int32),
                 removed=np.full((B,), -9.0, np.float32), ok_row=rng.integers(0, 2, B).astype(np.int32), gx_row=rng.normal(size=(B, L.nx)).astype(np.float32),
                 ok_out=np.full((B,), -9, np.int32), gx_out=np.full((B, L.nx), 7.0, np.float32))
        if kind != "pre":
            for k in ("t_state", "t_list", "t_list_rot", "t_sens", "wrench", "gp", "rot"):
                h[k][en_post] = np.nan
        else:
            for k in ("carry_state", "carry_list", "carry_list_rot"):
                h[k][wt.ended(e, t_post - 1)] = np.nan
        rot_in = h["rot"].copy()
        d = {k: torch.from_numpy(v).cuda() for k, v in h.items()}

        def gate(p, e_ptr):
            g = cm._capi.CmpcWalkGateRot()
            b = g.base
            b.batch, b.max_contacts, b.horizon, b.end_tick = B, M, N, e_ptr
            b.do_post, b.tick_post = int(kind != "pre"), t_post
            b.seed_state, b.tick_state, b.tick_list, b.tick_sens = p("seed"), p("t_state"), p("t_list"), p("t_sens")
            b.carry_state, b.carry_list, b.wrench_row, b.grad_p_row, b.status_row = p("carry_state"), p("carry_list"), p("wrench"), p("gp"), p("status")
            b.do_pre, b.tick_pre, b.first = int(kind != "post"), t_post - 1, int(kind == "pre")
            b.ok_row, b.ok_out = p("ok_row"), p("ok_out")
            if gx:
                b.grad_x_row, b.grad_x_out = p("gx_row"), p("gx_out")
            g.tick_list_rot, g.carry_list_rot, g.rot_row, g.removed_row = p("t_list_rot"), p("carry_list_rot"), p("rot"), p("removed")
            return g
        assert lib.cmpc_rollout_walk_vjp_rot_gate(C.byref(gate(lambda k: _ptr(h[k]), _ptr(e)))) == 0
        s.rollout_walk_vjp_rot_gate_device(gate(lambda k: d[k].data_ptr(), e_d.data_ptr()))
        torch.cuda.synchronize()
        outs = ("carry_state", "carry_list", "carry_list_rot", "wrench", "gp", "rot", "status", "removed", "ok_out", "gx_out")
        for k in outs:
            _same_bits(d[k], h[k], f"{kind}, tick {t_post}: {k}")
        for k in outs:
            assert np.isfinite(h[k]).all(), k
        if kind != "pre":
            assert (h["status"][en_post] == 6).all() and (h["removed"][en_post] == 0).all() and (h["rot"][en_post] == 0).all()
            assert (h["carry_list_rot"][en_post] == 0).all() and (h["carry_list"][en_post] == 0).all()
            _same_bits(h["rot"][~en_post], rot_in[~en_post], "a walking problem's row of dGradRot is the tick's")
            _same_bits(h["carry_list_rot"][~en_post], h["t_list_rot"][~en_post])
            np.testing.assert_array_equal(h["carry_state"][e == t_post], h["seed"][e == t_post])
        else:
            assert (h["carry_list_rot"][wt.ended(e, t_post - 1)] == 0).all() and (h["removed"] == -9.0).all()


# ---- 2, 3: one yawed walk of 16 ticks, shared by the tests below ----
@pytest.fixture(scope="module")
def walk16():
    import torch
    cfg = _cfg()
    B, ticks = 8, 16
    com0, dcom0, h0, push = _start(B)
    ro_run, ro = _yawed(cfg, B), _yawed(cfg, B)
    rec = ro_run.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False, tape=True)
    assert all(rec["merge_ok"]) and len(rec["tape"]["ticks"]) == ticks
    w = ro.walk_device_taped(ticks, com0, dcom0, h0, push=push, push_ticks=3)
    rng = np.random.default_rng(2)
    gS = torch.from_numpy(rng.normal(size=(ticks + 1, B, 9))).cuda()
    gX = torch.from_numpy((1e-2 * rng.normal(size=(ticks, B, ro.L.nx))).astype(np.float32)).cuda()
    ref = ro_run.backward(rec["tape"], gS, gX, rot=True)
    got = ro.backward_device_rot(w, gS, gX)
    plain = ro.backward_device(w, gS, gX)
    torch.cuda.synchronize()
    return dict(cfg=cfg, B=B, ticks=ticks, w=w, ro=ro, gS=gS, gX=gX, ref=ref, got=got, plain=plain)


def test_reverse_walk_with_orientations_is_backward_rot(walk16):
    """backward_device_rot against run(tape=True) + backward(rot=True), random seeds on the states and the solutions: every key to the bit; every key
    backward_device has is bit-equal to it on the same walk; the orientation outputs are not trivially zero"""
    ref, got, plain = walk16["ref"], walk16["got"], walk16["plain"]
    for k in GRADS + ROT:
        _same_bits(got[k], ref[k], k)
    for k in GRADS:
        _same_bits(got[k], plain[k], f"{k} against backward_device")
    assert set(got) == set(plain) | set(ROT)
    assert (got["status"].cpu().numpy() == 0).all() and (got["end_tick"].cpu().numpy() == -1).all()
    removed = got["removed"].cpu().numpy()
    print("\nremoved per tick (problem 0):", removed[:, 0].tolist(), " max |list_rot0|, |plan_rot|, |rot|:",
          [float(got[k].abs().max()) for k in ("list_rot0", "plan_rot", "rot")])
    for k in ("list_rot0", "plan_rot", "rot"):
        assert float(got[k].abs().max()) > 0, k
    assert (removed == 0).any(), "no tick kept its orientation derivative"


def test_segments_compose_through_three_carries(walk16):
    """rows 8 .. 15 and then 0 .. 7 through the three carry buffers against the one call over 0 .. 15 (backward_device_rot's): every bit"""
    import torch
    ro, w, gS, gX, got = walk16["ro"], walk16["w"], walk16["gS"], walk16["gX"], walk16["got"]
    B, T, M, dev = walk16["B"], walk16["ticks"], ro.M, ro.dev
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    out = dict(wrench=z((T, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((T, B), torch.int32), plan_rot=z((B, 2, M, 3)),
               rot=z((T, B, 2, N, 3)), removed=z((T, B), torch.float32))
    c, cl, clr = gS[T].clone(), z((B, 2, M, 3)), z((B, 2, M, 3))
    with torch.cuda.stream(ro.solver.launch_stream):
        for t0, n in ((8, 8), (0, 8)):
            ro.solver.rollout_walk_vjp_device(t0, n, w["tape"], t0, w["end_tick"], gS, c, cl, out["status"], grad_X=gX, wrench=out["wrench"],
                                              dGradPlan=out["plan"], dGradModel=out["models"], carry_list_rot=clr, dGradPlanRot=out["plan_rot"],
                                              grad_rot=out["rot"], removed=out["removed"])
    torch.cuda.synchronize()
    for a, k in ((c, "state0"), (cl, "list0"), (clr, "list_rot0")):
        _same_bits(a, got[k], k)
    for k in ("wrench", "models", "plan", "status", "plan_rot", "rot", "removed"):
        _same_bits(out[k], got[k], k)
    # r without its carry, r missing, rows outside the tape
    s, tp = ro.solver, w["tape"]
    g = cm._capi.CmpcWalkGrads(gS.data_ptr(), None, c.data_ptr(), cl.data_ptr(), None, None, None, None, out["status"].data_ptr())
    r = cm._capi.CmpcWalkGradsRot(clr.data_ptr(), None, None, None)
    call = lambda tick0, n, row0, rr: s._lib.cmpc_rollout_walk_vjp_rot_device(s._h, M, tick0, n, C.byref(tp["_c"]), row0, None, C.byref(g),
                                                                              None if rr is None else C.byref(rr), None)
    assert call(0, 1, 0, cm._capi.CmpcWalkGradsRot(None, None, None, None)) != 0 and "dCarryListRot" in s.last_error
    assert call(0, 1, 0, None) != 0
    assert call(0, T + 1, 0, r) != 0 and call(0, 1, T, r) != 0 and call(0, 0, 0, r) != 0 and call(0, 1, -1, r) != 0
    torch.cuda.synchronize()


# ---- 4, 5: an ended problem on the yawed plan ----
@pytest.fixture(scope="module", params=[False, True], ids=["stay", "skip_ended"])
def ended_walk(request):
    """the scene of test_an_ended_problem_keeps_its_gradient_and_the_others_theirs on the yawed plan: problem 3 ends at tick 2 (code 1) of 5 by the
    replan; the same batch without the replan; the 2-tick walk"""
    cfg = _cfg()
    B, T = 8, 5
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    push = np.zeros((B, 3)); push[:, 0] = np.linspace(-0.2, 0.2, B)
    ro, ro_b, ro_2 = _yawed(cfg, B), _yawed(cfg, B), _yawed(cfg, B)
    t = ro.plan[0].clone()
    t[3, 0] += 100.0
    kw = dict(push=push, push_ticks=2, skip_ended=request.param)
    w = ro.walk_device_taped(T, com0, z, z, replan={2: (t, ro.plan[1], ro.plan[2])}, **kw)
    base = ro_b.walk_device_taped(T, com0, z, z, **kw)
    two = ro_2.walk_device_taped(2, com0, z, z, **kw)
    assert w["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and int(w["end_code"][3]) == 1
    assert (base["end_tick"].cpu().numpy() == -1).all() and (two["end_tick"].cpu().numpy() == -1).all()
    return dict(cfg=cfg, B=B, T=T, ro=ro, w=w, ro_b=ro_b, base=base, ro_2=ro_2, two=two, com0=com0, kw=kw)


def test_an_ended_problem_keeps_its_orientation_gradient_and_the_others_theirs(ended_walk):
    """NaN seeds behind problem 3's end.  The seven others are bit-equal to the batch without the replan in every key; problem 3 equals the 2-tick walk
    reversed, in list_rot0 and plan_rot too; its rot rows 2 .. are exactly zero, its removed rows 2 .. 0, its status [0, 0, 6, 6, 6]; nothing anywhere is
    non-finite.  A problem whose com0 is NaN ends at tick 0: its orientation outputs are all zero and its state0 is its seed."""
    import torch
    v = ended_walk
    cfg, B, T, ro = v["cfg"], v["B"], v["T"], v["ro"]
    rng = np.random.default_rng(6)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    gS_nan, gX_nan = gS.copy(), gX.copy()
    gS_nan[3:, 3], gX_nan[2:, 3] = np.nan, np.nan
    got = ro.backward_device_rot(v["w"], gS_nan, gX_nan)
    ref = v["ro_b"].backward_device_rot(v["base"], gS, gX)
    short = v["ro_2"].backward_device_rot(v["two"], gS[:3], gX[:2])
    torch.cuda.synchronize()
    keys = GRADS + ROT
    got, ref, short = _host(got, keys), _host(ref, keys), _host(short, keys)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
    others = [0, 1, 2, 4, 5, 6, 7]
    for k in keys:
        ax = 1 if k in ("wrench", "status", "rot", "removed") else 0
        _same_bits(np.take(got[k], others, axis=ax), np.take(ref[k], others, axis=ax), k)
    assert (ref["status"] == 0).all()
    for k in ("state0", "list0", "push", "models", "plan", "list_rot0", "plan_rot"):
        _same_bits(got[k][3], short[k][3], f"problem 3: {k}")
    for k in ("wrench", "rot", "removed"):
        _same_bits(got[k][:2, 3], short[k][:, 3], f"problem 3: {k}")
        assert (got[k][2:, 3] == 0).all(), k
    assert got["status"][:, 3].tolist() == [0, 0, 6, 6, 6] and short["status"][:, 3].tolist() == [0, 0]
    # a problem that never had a finite state
    bad = v["com0"].copy()
    bad[5] = np.nan
    zz = np.zeros((B, 3))
    ro_n = _yawed(cfg, B)
    wn = ro_n.walk_device_taped(3, bad, zz, zz, **v["kw"])
    gn = _host(ro_n.backward_device_rot(wn, gS[:4], gX[:3]), keys)
    torch.cuda.synchronize()
    assert int(wn["end_tick"][5]) == 0 and (np.delete(wn["end_tick"].cpu().numpy(), 5) == -1).all()
    _same_bits(gn["state0"][5], gS[0, 5], "ended at tick 0: state0 is the seed on state 0")
    for k in ("list0", "push", "models", "plan", "list_rot0", "plan_rot"):
        assert (gn[k][5] == 0).all(), k
    for k in ("wrench", "rot", "removed"):
        assert (gn[k][:, 5] == 0).all(), k
    assert (gn["status"][:, 5] == 6).all() and (np.delete(gn["status"], 5, axis=1) == 0).all()
    for k in keys:
        assert np.isfinite(gn[k]).all(), k


def test_forward_and_reverse_are_adjoint_with_orientations_endings_included(ended_walk):
    """forward_sensitivity_device (state0, list0, list_rot0, plan, plan_rot, push, models; k = 2; solutions) against backward_device_rot with random
    grad_states / grad_X on the walk problem 3 ends in: per problem and column sum_i <gS_i, dS_i> + sum_i <gX_i, dX_i> over ALL rows equals the
    contraction of the seven input groups with their directions.  Relative gap <= 5 x ADJ (five chained ticks).  Problem 3 is included, both its sides
    non-zero; the orientation terms are non-zero for at least one problem."""
    import torch
    from tests.test_gpu_walk_jvp import _directions
    v = ended_walk
    cfg, B, T, ro, w = v["cfg"], v["B"], v["T"], v["ro"], v["w"]
    d = _directions(cfg, B, 2, ro.M, T, 12)
    del d["dir_wrench"]
    rng = np.random.default_rng(13)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    f = ro.forward_sensitivity_device(w, solutions=True, **d)
    r = ro.backward_device_rot(w, gS, gX)
    torch.cuda.synchronize()
    fs, fx = f["states"].cpu().numpy(), f["X"].cpu().numpy().astype(np.float64)
    pairs = (("state0", d["dir_state0"]), ("list0", d["dir_list0"]), ("list_rot0", d["dir_list_rot0"]), ("plan", d["dir_plan"]),
             ("plan_rot", d["dir_plan_rot"]), ("push", d["dir_push"].astype(np.float64)), ("models", d["dir_models"]))
    rh = {name: r[name].cpu().numpy() for name, _ in pairs}
    assert f["status"].cpu().numpy()[:, 3].tolist() == [0, 0, 6, 6, 6] and r["status"].cpu().numpy()[:, 3].tolist() == [0, 0, 6, 6, 6]
    worst, rot_terms = 0.0, 0
    for b in range(B):
        for j in range(2):
            lhs = float((gS[:, b] * fs[:, b, j]).sum() + (gX[:, b].astype(np.float64) * fx[:, b, j]).sum())
            terms = {name: float((rh[name][b] * dd[b, j]).sum()) for name, dd in pairs}
            rhs = sum(terms.values())
            gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)
            worst = max(worst, gap)
            rot_terms += int(terms["list_rot0"] + terms["plan_rot"] != 0.0)
            print(f"problem {b} column {j}: forward {lhs:.9e}  reverse {rhs:.9e}  gap {gap:.2e}  terms " + " ".join(f"{n} {t:.1e}" for n, t in terms.items()))
            if b == 3:
                assert lhs != 0.0 and rhs != 0.0
    print(f"forward walk against reverse walk with orientations over {T} ticks, worst gap over {B} problems x 2 columns: {worst:.2e} (bound {5 * ADJ:.1e})")
    assert worst <= 5 * ADJ and rot_terms > 0


# ---- 6. no host read ----
def test_nothing_is_read_back(walk16):
    """walk_device_taped(replan, skip_ended=True) + backward_device_rot under torch's sync debug mode, after a first call has allocated the workspaces"""
    import torch
    ro, B = walk16["ro"], walk16["B"]
    com0, dcom0, h0, push = _start(B)
    t = ro.plan[0].clone()
    gS = torch.ones((7, B, 9), dtype=torch.float64, device=ro.dev)
    gX = torch.zeros((6, B, ro.L.nx), dtype=torch.float32, device=ro.dev)
    kw = dict(push=push, push_ticks=2, replan={3: (t, ro.plan[1], ro.plan[2])}, skip_ended=True)
    ro.backward_device_rot(ro.walk_device_taped(6, com0, dcom0, h0, **kw), gS, gX)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device_taped(6, com0, dcom0, h0, **kw)
        r = ro.backward_device_rot(w, gS, gX)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert (w["end_tick"].cpu().numpy() == -1).all() and (r["status"].cpu().numpy() == 0).all() and w["tape"]["segments"] == [0, 3]
    assert np.isfinite(r["state0"].cpu().numpy()).all() and float(r["state0"].abs().max()) > 0 and np.isfinite(r["list_rot0"].cpu().numpy()).all()


# ---- 7. autograd, on the landing scene ----
@pytest.fixture(scope="module")
def landing():
    """rollout_differentiable on the landing scene (B = 8, 6 ticks, the landing footstep turned by omega): the gradients of one loss"""
    import torch
    from tests.test_gpu_rollout_rot_adjoint import _landing_scene
    B, T = 8, 6
    target = torch.tensor([0.05, 0.0, 0.7], device="cuda")

    def grads(omega=None, yaw=None, tangent=None, **kw):
        import torch.autograd.forward_ad as fwAD
        cfg, ro, s0, pushv, yaw0 = _landing_scene(B)
        state0 = torch.from_numpy(s0.astype(np.float32)).cuda().requires_grad_(tangent is None)
        push = torch.from_numpy(pushv.astype(np.float32)).cuda().requires_grad_(tangent is None)
        out = dict(ro=ro)
        if tangent is not None:
            with fwAD.dual_level():
                states = cm.rollout_differentiable(ro, T, state0, push=push, push_ticks=3, plan_rot=fwAD.make_dual(omega.clone(), tangent), **kw)
                primal, tan = fwAD.unpack_dual(states)
                assert tan is not None and tan.dtype == torch.float32 and tuple(tan.shape) == (T + 1, B, 9)
                out.update(states=primal.clone(), tangent=tan.clone())
            torch.cuda.synchronize()
            return out
        if omega is not None:
            omega = omega.clone().requires_grad_(True)
            kw["plan_rot"] = omega
        if yaw is not None:
            yaw = yaw.clone().requires_grad_(True)
            kw["plan_yaw"] = yaw
        states = cm.rollout_differentiable(ro, T, state0, push=push, push_ticks=3, **kw)
        assert tuple(states.shape) == (T + 1, B, 9)
        (((states[:, :, 0:3] - target) ** 2).sum() + (states[-1] ** 2).sum()).backward()
        torch.cuda.synchronize()
        out.update(states=states.detach(), state0=state0.grad, push=push.grad, plan_rot=None if omega is None else omega.grad,
                   plan_yaw=None if yaw is None else yaw.grad)
        return out
    _, ro, _, _, yaw0 = _landing_scene(B)
    yaw0 = torch.from_numpy(yaw0).cuda()
    omega = torch.zeros(tuple(yaw0.shape) + (3,), dtype=torch.float64, device="cuda")
    omega[..., 2] = yaw0
    return dict(B=B, T=T, grads=grads, omega=omega, yaw0=yaw0, plan=ro.plan, host=grads(omega), dev=grads(omega, device_walk=True))


def test_autograd_of_plan_rot_on_the_device_path_is_the_host_path(landing):
    """plan_rot = (0, 0, 0.2) on the landing footstep: device_walk=True against device_walk=False in the states, state0.grad, push.grad and plan_rot.grad,
    to the bit (nothing ended); the z component of plan_rot.grad is plan_yaw.grad of the existing host path to the bit"""
    a, b = landing["host"], landing["dev"]
    assert (b["ro"].last_walk["end_tick"].cpu().numpy() == -1).all()
    for k in ("states", "state0", "push", "plan_rot"):
        _same_bits(b[k], a[k], k)
    y = landing["grads"](yaw=landing["yaw0"])
    _same_bits(y["states"], a["states"], "states against plan_yaw's")
    _same_bits(a["plan_rot"][..., 2], y["plan_yaw"], "plan_rot.grad z against plan_yaw.grad")
    _same_bits(b["plan_rot"][..., 2], y["plan_yaw"], "plan_rot.grad z on the device path against plan_yaw.grad")
    assert float(y["plan_yaw"].abs().max()) > 0 and tuple(b["plan_rot"].shape) == tuple(landing["omega"].shape)


def test_autograd_of_plan_rot_with_an_ended_problem_and_a_tilt(landing):
    """problem 1 ended by a replan at tick 2: the others keep their bits, its own gradients are finite.  A tilt, omega = (0.05, 0, 0.2), runs: plan_rot.grad
    is finite and non-zero in x"""
    import torch
    b, plan = landing["dev"], landing["plan"]
    t = plan[0].clone()
    t[1, 1] += 100.0      # (the stance foot's times: its merge fails at the replan)
    c = landing["grads"](landing["omega"], device_walk=True, replan={2: (t, plan[1], plan[2])})
    assert c["ro"].last_walk["end_tick"].cpu().numpy().tolist() == [-1, 2, -1, -1, -1, -1, -1, -1]
    others = [0, 2, 3, 4, 5, 6, 7]
    for k in ("state0", "push", "plan_rot"):
        _same_bits(c[k][others], b[k][others], f"{k} of the others")
        assert bool(torch.isfinite(c[k]).all()), k
    assert float(c["state0"][1].abs().max()) > 0
    assert (c["ro"].last_backward["status"][:, 1].cpu().numpy() == [0, 0, 6, 6, 6, 6]).all()
    tilt = landing["omega"].clone()
    tilt[:, 0, 1, 0] = 0.05
    d = landing["grads"](tilt, device_walk=True)
    assert bool(torch.isfinite(d["plan_rot"]).all()) and float(d["plan_rot"][..., 0].abs().max()) > 0
    assert bool(torch.isfinite(d["states"]).all()) and (d["ro"].last_walk["end_tick"].cpu().numpy() == -1).all()


def test_forward_mode_of_plan_rot_is_forward_sensitivity_device(landing):
    """torch.autograd.forward_ad with a plan_rot tangent at a tilted omega: the tangent equals forward_sensitivity_device fed Jr(omega) t as dir_plan_rot and
    dir_list_rot0, to the bit"""
    import torch
    omega = landing["omega"].clone()
    omega[:, 0, 1, 0] = 0.05
    t = torch.from_numpy(np.random.default_rng(5).normal(size=tuple(omega.shape))).cuda()
    f = landing["grads"](omega, tangent=t, device_walk=True)
    ro = f["ro"]
    jt = (so3_right_jacobian(omega) * t[..., None, :]).sum(-1)[:, None].contiguous()
    col = ro.forward_sensitivity_device(ro.last_walk, dir_plan_rot=jt, dir_list_rot0=jt)
    torch.cuda.synchronize()
    assert (ro.last_walk["end_tick"].cpu().numpy() == -1).all()
    _same_bits(f["tangent"], col["states"][:, :, 0].to(torch.float32), "the tangent against forward_sensitivity_device's column")
    assert bool(f["tangent"][1:].any()) and not bool(f["tangent"][0].any()) and bool(torch.isfinite(f["tangent"]).all())
