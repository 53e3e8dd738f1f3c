"""The device walk taped and run in reverse (include/cmpc.h: cmpc_rollout_tape_device, cmpc_rollout_walk_taped_device, cmpc_rollout_walk_vjp_device and
its gate; WalkingRollout.walk_device_taped / backward_device, rollout_differentiable(device_walk=True)).  Everything here is a comparison of bits:
the tape kernel against torch clones, the gate kernel against the host form, the taped walk against the untaped one and against run(tape=True), the reverse
walk against run(tape=True) + backward(), one call against two segments, and an ended problem against the shorter walk it amounts to.
N = 10, dt = 0.06, the ergoCubGazeboV1 weights."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_tape_ref as wt
from tests.test_gpu_walk_record import _start

pytestmark = pytest.mark.gpu

N = 10
GRADS = ("state0", "list0", "wrench", "push", "models", "plan", "status")


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b, msg=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _cfg():
    return cm.config.ergocub_gazebo_v1(N, 0.06)


# ---- 1. the tape kernel against torch copies ----
@pytest.mark.parametrize("B", [70, 300])
def test_tape_kernel_makes_bit_copies(B):
    """two ticks through cmpc_rollout_tick_device (a cold first tick out of place, a warm merge tick in place), each followed by cmpc_rollout_tape_device,
    against clones taken tick by tick and multipliers_device; B = 70 is a partial second wave, B = 300 a second workgroup"""
    import torch
    cfg = _cfg()
    ro = cm.rollout.WalkingRollout(cfg, B)
    s, L, dev, dt = ro.solver, ro.L, ro.dev, cfg.sampling_time
    s.set_multiplier_output(True)
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    dP, dX0, dX, dInfo = z((B, L.np)), z((B, L.nx)), z((B, L.nx)), z((B, 8))
    com0, dcom0, h0, push = _start(B)
    state = torch.from_numpy(np.concatenate([com0, dcom0, h0], 1).astype(np.float32)).to(dev)
    state2 = torch.zeros_like(state)
    ok, land, zmp = torch.full((B,), 7, dtype=torch.int32, device=dev), z((B, 2), torch.int32), z((B, 2))
    sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
    n_plan = 2 + N + 2
    plan_com = z((B, n_plan, 3))
    plan_com[:, :, 0] = (ro.com_speed * dt * torch.arange(n_plan, dtype=torch.float64, device=dev)).to(torch.float32)[None, :]
    plan_h = torch.zeros_like(plan_com)
    kw = dict(step=dt / ro.substeps, substeps=ro.substeps)
    tape = s.walk_tape(2, ro.M, **kw)
    for k in ("X", "P", "lam_g", "info", "states", "plan_t", "list_t"):
        tape[k].fill_(-3.0)
    for k in ("ok", "land", "plan_n", "list_n"):
        tape[k].fill_(-3)
    want = []
    # tick 0: cold, out of place (state -> state2): both parts behind the tick
    s.contacts_sample_device(0.0, sets[0], dP)
    s.write_state_device(state, dP, None)
    s.cold_start_device(dP, dX0)
    s.rollout_tick_device(0.0, ro.plan, None, sets[0], ok, land, state, None, dP, dX0, dX, dInfo, state2, zmp, False, planner=(plan_com, plan_h, dt, 0.0, 1.0, 0.7), **kw)
    s.rollout_tape_device(0, tape, dX, dP, dInfo, None, land, state, state2, None, sets[0], parts=3)
    want.append(dict(X=dX.clone(), P=dP.clone(), lam_g=s.multipliers_device(dX, dP), info=dInfo.clone(), state_in=state.clone(), state_out=state2.clone(),
                     ok=torch.ones((B,), dtype=torch.int32, device=dev), land=land.clone(), list_t=sets[0][0].clone(), list_n=sets[0][2].clone()))
    # tick 1: warm, in place on state2: part 1 in front of it (it rewrites row 1 of the states with the same bits), part 2 behind it
    s.rollout_tape_device(1, tape, None, None, None, None, None, state2, None, None, None, parts=1)
    before = state2.clone()
    s.rollout_tick_device(dt, ro.plan, sets[0], sets[1], ok, land, state2, None, dP, dX0, dX, dInfo, state2, zmp, True, planner=(plan_com, plan_h, dt, dt, 1.0, 0.7), **kw)
    s.rollout_tape_device(1, tape, dX, dP, dInfo, ok, land, None, state2, ro.plan, sets[1], parts=2)
    want.append(dict(X=dX.clone(), P=dP.clone(), lam_g=s.multipliers_device(dX, dP), info=dInfo.clone(), state_in=before, state_out=state2.clone(),
                     ok=ok.clone(), land=land.clone(), list_t=sets[1][0].clone(), list_n=sets[1][2].clone(), plan_t=ro.plan[0].clone(), plan_n=ro.plan[2].clone()))
    torch.cuda.synchronize()
    for r, w in enumerate(want):
        for k in ("X", "P", "lam_g", "info", "ok", "land", "list_t", "list_n"):
            _same_bits(tape[k][r], w[k], f"row {r}: {k}")
        _same_bits(tape["states"][r], w["state_in"], f"row {r}: the state that went in")
        _same_bits(tape["states"][r + 1], w["state_out"], f"row {r}: the state it left")
    _same_bits(tape["plan_t"][1], want[1]["plan_t"])
    _same_bits(tape["plan_n"][1], want[1]["plan_n"])
    assert (tape["plan_t"][0] == -3.0).all() and (tape["plan_n"][0] == -3).all()      # a first tick has no planner row: left alone
    assert (want[1]["ok"] == 1).all() and (want[0]["info"][:, 0] > 0).all() and float(want[1]["lam_g"].abs().max()) > 0
    # the checks that need a handle: the multiplier output off, a row outside the tape, part 3 behind a tick that ran in place
    call = lambda s_, row, parts, sin: s_._lib.cmpc_rollout_tape_device(
        s_._h, ro.M, row, parts, dX.data_ptr(), dP.data_ptr(), dInfo.data_ptr(), None, land.data_ptr(), sin.data_ptr(), state2.data_ptr(), None, None,
        sets[1][0].data_ptr(), sets[1][2].data_ptr(), C.byref(tape["_c"]), None)
    assert call(s, 2, 3, state) != 0 and call(s, -1, 3, state) != 0 and call(s, 0, 0, state) != 0 and call(s, 0, 3, state2) != 0
    s2 = cm.BatchSolver(cfg, B)
    assert call(s2, 0, 3, state) != 0 and "multiplier" in s2.last_error
    torch.cuda.synchronize()


# ---- 2. the gate kernel against the host form ----
@pytest.mark.parametrize("B", [70, 300])
def test_gate_kernel_matches_the_host_form(B):
    """the three kinds of gate step -- PRE only (the first of a call), POST + PRE, POST only -- with random end ticks, random seeds and NaN in everything
    the tick left for an ended problem: every array the kernel writes against the host form, to the bit"""
    import torch
    from tests.test_walk_tape_cpu import _ptr
    cfg = _cfg()
    s, L, M = cm.BatchSolver(cfg, B), cm.Layout(N), 5
    lib = cm._capi.lib()
    rng = np.random.default_rng(B)
    T = 6
    e = rng.integers(-1, T + 1, B).astype(np.int32)
    assert (e == -1).any() and (e == 0).any() and (e == T).any()
    for kind, t_post, gx in [("pre", T, True), ("both", 3, True), ("both", 1, False), ("post", 0, True)]:
        en_post = wt.ended(e, t_post)
        h = dict(seed=rng.normal(size=(B, 9)), t_state=rng.normal(size=(B, 9)), t_list=rng.normal(size=(B, 2, M, 3)),
                 t_sens=rng.integers(0, 6, (B, 8)).astype(np.float32), carry_state=rng.normal(size=(B, 9)), carry_list=rng.normal(size=(B, 2, M, 3)),
                 wrench=rng.normal(size=(B, N, 6)).astype(np.float32), gp=rng.normal(size=(B, L.np)).astype(np.float32), status=np.full((B,), -9, np.int32),
                 ok_row=rng.integers(0, 2, B).astype(np.int32), gx_row=rng.normal(size=(B, L.nx)).astype(np.float32), ok_out=np.full((B,), -9, np.int32),
                 gx_out=np.full((B, L.nx), 7.0, np.float32))
        if kind != "pre":
            for k in ("t_state", "t_list", "t_sens", "wrench", "gp"):
                h[k][en_post] = np.nan
        else:
            h["carry_state"][wt.ended(e, t_post - 1)] = np.nan
        d = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
        e_d = torch.from_numpy(e).cuda()

        def gate(p, e_ptr):
            g = cm._capi.CmpcWalkGate()
            g.batch, g.max_contacts, g.horizon, g.end_tick = B, M, N, e_ptr
            g.do_post, g.tick_post = int(kind != "pre"), t_post
            g.seed_state, g.tick_state, g.tick_list, g.tick_sens = p("seed"), p("t_state"), p("t_list"), p("t_sens")
            g.carry_state, g.carry_list, g.wrench_row, g.grad_p_row, g.status_row = p("carry_state"), p("carry_list"), p("wrench"), p("gp"), p("status")
            g.do_pre, g.tick_pre, g.first = int(kind != "post"), t_post - 1, int(kind == "pre")
            g.ok_row, g.ok_out = p("ok_row"), p("ok_out")
            if gx:
                g.grad_x_row, g.grad_x_out = p("gx_row"), p("gx_out")
            return g
        assert lib.cmpc_rollout_walk_vjp_gate(C.byref(gate(lambda k: _ptr(h[k]), _ptr(e)))) == 0
        s.rollout_walk_vjp_gate_device(gate(lambda k: d[k].data_ptr(), e_d.data_ptr()))
        torch.cuda.synchronize()
        for k in ("carry_state", "carry_list", "wrench", "gp", "status", "ok_out", "gx_out"):
            _same_bits(d[k], h[k], f"{kind}, tick {t_post}: {k}")
        for k in ("carry_state", "carry_list", "wrench", "gp", "gx_out"):
            assert np.isfinite(h[k]).all(), k
        if kind != "pre":
            assert (h["status"][en_post] == 6).all() and (h["wrench"][en_post] == 0).all() and (h["carry_list"][en_post] == 0).all()
            np.testing.assert_array_equal(h["carry_state"][e == t_post], h["seed"][e == t_post])
        if kind != "post":
            assert (h["ok_out"][wt.ended(e, t_post - 1)] == 0).all()
            assert (h["gx_out"] == 7.0).all() if not gx else (h["gx_out"][wt.ended(e, t_post - 1)] == 0).all()


# ---- 3 .. 5, 7: one walk of 16 ticks, taped three ways, shared by the tests below ----
@pytest.fixture(scope="module")
def walk16():
    import torch
    cfg = _cfg()
    B, ticks = 8, 16
    com0, dcom0, h0, push = _start(B)
    ro_run = cm.rollout.WalkingRollout(cfg, B)
    rec = ro_run.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False, tape=True)
    assert all(rec["merge_ok"]) and len(rec["tape"]["ticks"]) == ticks
    ro = cm.rollout.WalkingRollout(cfg, B)
    plain = cm.rollout.WalkingRollout(cfg, B).walk_device(ticks, com0, dcom0, h0, push=push, push_ticks=3)
    w = ro.walk_device_taped(ticks, com0, dcom0, h0, push=push, push_ticks=3)
    rng = np.random.default_rng(2)
    gS = torch.from_numpy(rng.normal(size=(ticks + 1, B, 9))).cuda()
    gX = torch.from_numpy((1e-2 * rng.normal(size=(ticks, B, ro.L.nx))).astype(np.float32)).cuda()
    ref = ro_run.backward(rec["tape"], gS, gX)
    got = ro.backward_device(w, gS, gX)
    torch.cuda.synchronize()
    return dict(cfg=cfg, B=B, ticks=ticks, rec=rec, plain=plain, w=w, ro=ro, gS=gS, gX=gX, ref=ref, got=got)


def test_taped_walk_is_the_walk(walk16):
    """walk_device_taped() against walk_device() in every returned array, and every tape row against run(tape=True)'s (info word 6 is the clock)"""
    w, plain, tape, run_tape = walk16["w"], walk16["plain"], walk16["w"]["tape"], walk16["rec"]["tape"]
    assert set(w) - {"tape"} == set(plain)
    for k, v in plain.items():
        if k == "lists":
            for a, b in zip(w[k], v):
                _same_bits(a, b, k)
        elif k == "info":
            _same_bits(w[k][:, :6], v[:, :6], k)
            _same_bits(w[k][:, 7], v[:, 7], k)
        else:
            _same_bits(w[k], v, k)
    land = w["land"].cpu().numpy()
    assert land[4, 0, 0] == N and land[13, 0, 0] == 1 and (w["end_tick"].cpu().numpy() == -1).all()
    for i, tk in enumerate(run_tape["ticks"]):
        for k in ("X", "P", "lam_g", "land", "list_t", "list_n"):
            _same_bits(tape[k][i], tk[k], f"tick {i}: {k}")
        _same_bits(tape["states"][i], tk["state"], f"tick {i}: state")
        _same_bits(tape["info"][i][:, :6], tk["info"][:, :6], f"tick {i}: info")
        _same_bits(tape["info"][i][:, 7], tk["info"][:, 7], f"tick {i}: info")
        if i > 0:      # the previous tick's list of row i is row i - 1's; the planner's times are copied per row
            _same_bits(tape["list_t"][i - 1], tk["prev_t"], f"tick {i}: prev_t")
            _same_bits(tape["plan_t"][i], tk["plan_t"], f"tick {i}: plan_t")
    _same_bits(tape["states"][-1], run_tape["state"], "the final state")
    assert (tape["ok"].cpu().numpy() == 1).all()
    assert tape["dt"] == 0.06 and tape["substeps"] == walk16["ro"].substeps and tape["push_ticks"] == 3 and tape["force_sample_time"] is False


def test_reverse_walk_is_backward(walk16):
    """backward_device against run(tape=True) + backward() with random seeds on the states and on the solutions: every output to the bit"""
    ref, got = walk16["ref"], walk16["got"]
    for k in GRADS:
        _same_bits(got[k], ref[k], k)
    assert (got["status"].cpu().numpy() == 0).all()
    assert float(got["list0"].abs().max()) > 0 and float(got["plan"].abs().max()) > 0      # the step adjustment was on the path
    assert float(got["push"].abs().max()) > 0 and float(got["models"].abs().max()) > 0
    assert (got["end_tick"].cpu().numpy() == -1).all()


def test_segments_compose_on_the_device(walk16):
    """rows 8 .. 15 and then 0 .. 7 through the carry buffers against the one call over 0 .. 15 (backward_device's): every bit"""
    import torch
    ro, w, gS, gX, got = walk16["ro"], walk16["w"], walk16["gS"], walk16["gX"], walk16["got"]
    B, T, M, dev = walk16["B"], walk16["ticks"], ro.M, ro.dev
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    out = dict(wrench=z((T, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((T, B), torch.int32))
    c, cl = gS[T].clone(), z((B, 2, M, 3))
    with torch.cuda.stream(ro.solver.launch_stream):
        for t0, n in ((8, 8), (0, 8)):
            ro.solver.rollout_walk_vjp_device(t0, n, w["tape"], t0, w["end_tick"], gS, c, cl, out["status"], grad_X=gX, wrench=out["wrench"],
                                              dGradPlan=out["plan"], dGradModel=out["models"])
    torch.cuda.synchronize()
    _same_bits(c, got["state0"], "state0")
    _same_bits(cl, got["list0"], "list0")
    for k in ("wrench", "models", "plan", "status"):
        _same_bits(out[k], got[k], k)
    # rows outside the tape, and a tape whose row 0 is not a first tick
    s, tp = ro.solver, w["tape"]
    g = cm._capi.CmpcWalkGrads(gS.data_ptr(), None, c.data_ptr(), cl.data_ptr(), None, None, None, None, out["status"].data_ptr())
    call = lambda tick0, n, row0: s._lib.cmpc_rollout_walk_vjp_device(s._h, M, tick0, n, C.byref(tp["_c"]), row0, None, C.byref(g), None)
    assert call(0, T + 1, 0) != 0 and call(0, 1, T) != 0 and call(0, 0, 0) != 0 and call(0, 1, -1) != 0
    tp["_c"].first_row_is_first_tick = 0
    try:
        assert call(0, 1, 0) != 0
    finally:
        tp["_c"].first_row_is_first_tick = 1


def test_nothing_is_read_back(walk16):
    """walk_device_taped() and -- its workspaces allocated by the fixture's call -- backward_device under torch's sync debug mode"""
    import torch
    ro, B = walk16["ro"], walk16["B"]
    com0, dcom0, h0, push = _start(B)
    t = ro.plan[0].clone()
    gS = torch.ones((7, B, 9), dtype=torch.float64, device=ro.dev)
    gX = torch.zeros((6, B, ro.L.nx), dtype=torch.float32, device=ro.dev)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device_taped(6, com0, dcom0, h0, push=push, push_ticks=2, replan={3: (t, ro.plan[1], ro.plan[2])}, skip_ended=True)
        r = ro.backward_device(w, gS, gX)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert (w["end_tick"].cpu().numpy() == -1).all() and (r["status"].cpu().numpy() == 0).all() and w["tape"]["segments"] == [0, 3]
    assert np.isfinite(r["state0"].cpu().numpy()).all() and float(r["state0"].abs().max()) > 0


# ---- 6. an ended problem ----
@pytest.mark.parametrize("skip_ended", [False, True])
def test_an_ended_problem_keeps_its_gradient_and_the_others_theirs(skip_ended):
    """the replan of test_a_failed_merge_ends_one_problem_only: problem 3 ends at tick 2 (code 1) of 5.  The seven others are bit-equal to the batch without
    the replan; problem 3 equals a 2-tick taped walk reversed with grad_states[:3]; its seeds behind the end are NaN and nothing is.  A problem whose com0
    is NaN ends at tick 0: state0 is its seed on state 0, everything else zero, status 6 throughout."""
    import torch
    cfg = _cfg()
    B, T = 8, 5
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    push = np.zeros((B, 3)); push[:, 0] = np.linspace(-0.2, 0.2, B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    t[3, 0] += 100.0
    replan = {2: (t, ro.plan[1], ro.plan[2])}
    kw = dict(push=push, push_ticks=2, skip_ended=skip_ended)
    w = ro.walk_device_taped(T, com0, z, z, replan=replan, **kw)
    ro_b, ro_2 = cm.rollout.WalkingRollout(cfg, B), cm.rollout.WalkingRollout(cfg, B)
    base = ro_b.walk_device_taped(T, com0, z, z, **kw)
    two = ro_2.walk_device_taped(2, com0, z, z, **kw)
    rng = np.random.default_rng(6)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    gS_nan, gX_nan = gS.copy(), gX.copy()
    gS_nan[3:, 3], gX_nan[2:, 3] = np.nan, np.nan
    got = ro.backward_device(w, gS_nan, gX_nan)
    ref = ro_b.backward_device(base, gS, gX)
    short = ro_2.backward_device(two, gS[:3], gX[:2])
    torch.cuda.synchronize()
    assert w["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and int(w["end_code"][3]) == 1
    assert (base["end_tick"].cpu().numpy() == -1).all() and (two["end_tick"].cpu().numpy() == -1).all()
    h = lambda r: {k: r[k].cpu().numpy() for k in GRADS}
    got, ref, short = h(got), h(ref), h(short)
    for k in GRADS:
        assert np.isfinite(got[k]).all(), k
    others = [0, 1, 2, 4, 5, 6, 7]
    for k in GRADS:
        ax = 1 if k in ("wrench", "status") else 0
        _same_bits(np.take(got[k], others, axis=ax), np.take(ref[k], others, axis=ax), k)
    assert (ref["status"] == 0).all() and np.abs(ref["list0"]).max() > 0
    for k in ("state0", "list0", "push", "models", "plan"):
        _same_bits(got[k][3], short[k][3], f"problem 3: {k}")
    _same_bits(got["wrench"][:2, 3], short["wrench"][:, 3], "problem 3: wrench")
    assert got["status"][:, 3].tolist() == [0, 0, 6, 6, 6] and short["status"][:, 3].tolist() == [0, 0]
    assert (got["wrench"][2:, 3] == 0).all() and np.abs(got["wrench"][:2, 3]).max() > 0
    # a problem that never had a finite state
    bad = com0.copy()
    bad[5] = np.nan
    ro_n = cm.rollout.WalkingRollout(cfg, B)
    wn = ro_n.walk_device_taped(3, bad, z, z, **kw)
    gn = h(ro_n.backward_device(wn, gS[:4], gX[:3]))
    torch.cuda.synchronize()
    assert int(wn["end_tick"][5]) == 0 and (np.delete(wn["end_tick"].cpu().numpy(), 5) == -1).all()
    _same_bits(gn["state0"][5], gS[0, 5], "ended at tick 0: state0 is the seed on state 0")
    for k in ("list0", "push", "models", "plan"):
        assert (gn[k][5] == 0).all(), k
    assert (gn["wrench"][:, 5] == 0).all() and (gn["status"][:, 5] == 6).all()
    for k in GRADS:
        assert np.isfinite(gn[k]).all(), k
    assert (np.delete(gn["status"], 5, axis=1) == 0).all()


# ---- 8. autograd ----
def test_autograd_through_the_device_walk():
    """rollout_differentiable(device_walk=True) at B = 4, 6 ticks: state0.grad and push.grad equal the existing path's bit for bit when nothing ends; with
    one problem ended by the replan .backward() runs, the others' gradients are those bits again and the ended problem's state0.grad is finite"""
    import torch
    cfg = _cfg()
    B, T = 4, 6
    com0, dcom0, h0, pushv = _start(B, seed=3)
    s0 = np.concatenate([com0, dcom0, h0], 1).astype(np.float32)
    target = torch.tensor([0.05, 0.0, 0.7], device="cuda")

    def grads(**kw):
        ro = cm.rollout.WalkingRollout(cfg, B)
        state0 = torch.from_numpy(s0).cuda().requires_grad_(True)
        push = torch.from_numpy(pushv.astype(np.float32)).cuda().requires_grad_(True)
        states = cm.rollout_differentiable(ro, T, state0, push=push, push_ticks=3, **kw)
        assert tuple(states.shape) == (T + 1, B, 9)
        (((states[:, :, 0:3] - target) ** 2).sum() + (states[-1] ** 2).sum()).backward()
        torch.cuda.synchronize()
        return ro, states.detach(), state0.grad, push.grad
    _, st_a, gs_a, gp_a = grads()
    ro, st_b, gs_b, gp_b = grads(device_walk=True)
    _same_bits(st_b, st_a, "states")
    _same_bits(gs_b, gs_a, "state0.grad")
    _same_bits(gp_b, gp_a, "push.grad")
    assert float(gs_a.abs().max()) > 0 and float(gp_a.abs().max()) > 0 and (ro.last_walk["end_tick"].cpu().numpy() == -1).all()
    plan = cm.rollout.WalkingRollout(cfg, B).plan
    t = plan[0].clone()
    t[1, 0] += 100.0
    ro, st_c, gs_c, gp_c = grads(device_walk=True, replan={2: (t, plan[1], plan[2])})
    assert ro.last_walk["end_tick"].cpu().numpy().tolist() == [-1, 2, -1, -1]
    others = [0, 2, 3]
    _same_bits(gs_c[others], gs_a[others], "state0.grad of the others")
    _same_bits(gp_c[others], gp_a[others], "push.grad of the others")
    assert torch.isfinite(gs_c).all() and torch.isfinite(gp_c).all() and float(gs_c[1].abs().max()) > 0
    _same_bits(st_c[3:, 1], ro.last_walk["final_state"][1][None].expand(T - 2, 9), "rows behind the end hold final_state")
    _same_bits(st_c[:3, 1], st_a[:3, 1], "the ended problem's states up to its end")
    assert (ro.last_backward["status"][:, 1].cpu().numpy() == [0, 0, 6, 6, 6, 6]).all()
    with pytest.raises(NotImplementedError):
        cm.rollout_differentiable(ro, T, torch.from_numpy(s0).cuda(), plan_yaw=torch.zeros((B, 2, ro.M), dtype=torch.float64, device="cuda"), device_walk=True)
