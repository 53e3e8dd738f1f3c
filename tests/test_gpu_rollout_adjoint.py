"""GPU: the roll-out tick in reverse (include/cmpc.h: cmpc_plant_step_jvp_device / _vjp_device, cmpc_contacts_position_vjp_device,
cmpc_rollout_tick_vjp_device; WalkingRollout.run(tape=True) / backward, rollout_differentiable, BatchSolver.closed_loop_transition_device) against its
float64 restatement tests/rollout_adjoint_ref.py at the same float32 inputs.  Bounds (relative to the largest entry of the output group compared):
REF and ADJ are those of tests/test_gpu_sensitivity.py (kernels against sens_ref; adjoint identity on float32 device outputs); the glue around the solution
VJP is float64 on both sides, held to 1e-12, and its one float32 output to one rounding."""
import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import PlannedContact, pack_lists
from tests import rollout_adjoint_ref as rar
from tests.test_contacts_cpu import _random_walks

pytestmark = pytest.mark.gpu

REF = 5e-5
ADJ = 6e-4
F64 = 1e-12
ULP32 = 2.0 ** -23


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _plant_inputs(cfg, B, seed):
    """random float32 (X, P, state) with yawed feet, one foot of every third problem gated off, and a per-problem model table with moved corners"""
    rng = np.random.default_rng(seed)
    N = cfg.N
    L = cm.Layout(N)
    X = rng.normal(0, 0.3, (B, L.nx))
    P = np.zeros((B, L.np))
    for b in range(B):
        yaw = rng.uniform(-0.5, 0.5)
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
        for c in range(2):
            P[b, L.p_R[c]:L.p_R[c] + 9] = (Rz if c == 0 else Rz.T).reshape(-1, order="F")
            P[b, L.p_gam[c]] = 0.0 if (b % 3 == 2 and c == b % 2) else 1.0
            X[b, L.pos[c]:L.pos[c] + 3] = [0.05 * c, 0.08 * (1 - 2 * c), 0.0] + rng.normal(0, 0.01, 3)
            for j in range(4):
                X[b, L.f[c][j]:L.f[c][j] + 3] = [rng.normal(0, 0.2), rng.normal(0, 0.2), 9.80665 / 8 + rng.normal(0, 0.3)]
    P[:, L.p_fext:L.p_fext + 3] = rng.normal(0, 0.5, (B, 3))
    P[:, L.p_text:L.p_text + 3] = rng.normal(0, 0.1, (B, 3))
    state = np.concatenate([[0.0, 0.0, 0.7] + rng.normal(0, 0.02, (B, 3)), rng.normal(0, 0.1, (B, 3)), rng.normal(0, 0.05, (B, 3))], 1)
    models = np.tile(cm.config.model_row(cfg), (B, 1))
    models[:, 10:] += rng.normal(0, 0.005, (B, 24))
    return X.astype(np.float32), P.astype(np.float32), state.astype(np.float32), models


def test_plant_jvp_vjp_kernels_match_the_restatement():
    """Both sides compute in float64 from identical float32 inputs: double outputs <= 1e-12 relative, dGradX / dGradP (float32) to one rounding; the adjoint
    identity on device outputs <= ADJ; per-problem models; bit-identical across batch position and batch size."""
    _check_plant_kernels(cm.config.ergocub_gazebo_v1(20, 0.06))


def _check_plant_kernels(cfg):
    """the body of test_plant_jvp_vjp_kernels_match_the_restatement at cfg's horizon (tests/test_gpu_rollout_horizons.py runs it at others)"""
    import torch
    L = cm.Layout(cfg.N)
    B, step, nsub = 16, 0.01, 6
    X, P, state, models = _plant_inputs(cfg, B, 4)
    rng = np.random.default_rng(9)
    dS, dM, g = rng.normal(size=(B, 9)), rng.normal(size=(B, 34)), rng.normal(size=(B, 9))
    dX, dP = rng.normal(size=(B, L.nx)).astype(np.float32), rng.normal(size=(B, L.np)).astype(np.float32)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    worst = dict(jvp=0.0, g_state=0.0, g_model=0.0, g_x=0.0, g_p=0.0, adjoint=0.0)
    outs = {}
    for with_models in (False, True):
        s = cm.BatchSolver(cfg, B)
        if with_models:
            s.set_models(models)
        th = models if with_models else np.tile(cm.config.model_row(cfg), (B, 1))
        out = s.plant_step_jvp_device(cu(X), cu(P), cu(state), cu(dS), cu(dX), cu(dP), cu(dM), step=step, substeps=nsub)
        gS, gX, gP, gM = s.plant_step_vjp_device(cu(X), cu(P), cu(state), cu(g), step=step, substeps=nsub)
        torch.cuda.synchronize()
        out, gS, gX, gP, gM = (a.cpu().numpy() for a in (out, gS, gX, gP, gM))
        outs[with_models] = (out, gS, gX, gP, gM)
        for b in range(B):
            corners = th[b, 10:].astype(np.float32).astype(np.float64)      # (the record the kernels read is float32)
            args = (L, corners, X[b], P[b], state[b], float(np.float32(step)), nsub)
            grav = float(np.float32(rar.GRAVITY))                           # (... and so is the gravity the plant kernels are given)
            r_out = rar.plant_jvp(*args, dS[b], dX[b], dP[b], dM[b], gravity=grav)
            r_gs, r_gx, r_gp, r_gm = rar.plant_vjp(*args, g[b], gravity=grav)
            worst["jvp"] = max(worst["jvp"], _rel(out[b], r_out))
            worst["g_state"] = max(worst["g_state"], _rel(gS[b], r_gs))
            worst["g_model"] = max(worst["g_model"], _rel(gM[b], r_gm))
            for name, got, ref in (("g_x", gX[b], r_gx), ("g_p", gP[b], r_gp)):
                err = np.abs(got.astype(np.float64) - ref)
                tol = ULP32 * np.abs(ref) + F64 * np.abs(ref).max()
                worst[name] = max(worst[name], float((err / np.maximum(np.abs(ref), 1e-300))[ref != 0].max()))
                assert (err <= tol).all(), (name, b, float((err - tol).max()))
                assert np.count_nonzero(got) <= (30 if name == "g_x" else 6)
            lhs = g[b] @ out[b]
            rhs = gS[b] @ dS[b] + gX[b].astype(np.float64) @ dX[b] + gP[b].astype(np.float64) @ dP[b] + gM[b] @ dM[b]
            worst["adjoint"] = max(worst["adjoint"], abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    print(f"\nplant kernels N = {cfg.N} against the restatement: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"  (bounds: float64 groups {F64:.0e}, float32 groups one rounding {ULP32:.2e}, adjoint {ADJ:.0e})")
    assert worst["jvp"] <= F64 and worst["g_state"] <= F64 and worst["g_model"] <= F64 and worst["adjoint"] <= ADJ
    assert not np.array_equal(outs[False][0], outs[True][0])          # the model table is read
    # batch position and batch size: a batch of 5 holding problems 11, 3, 7, 0, 15
    idx = [11, 3, 7, 0, 15]
    s5 = cm.BatchSolver(cfg, 5)
    s5.set_models(models[idx])
    out5 = s5.plant_step_jvp_device(cu(X[idx]), cu(P[idx]), cu(state[idx]), cu(dS[idx]), cu(dX[idx]), cu(dP[idx]), cu(dM[idx]), step=step, substeps=nsub)
    v5 = s5.plant_step_vjp_device(cu(X[idx]), cu(P[idx]), cu(state[idx]), cu(g[idx]), step=step, substeps=nsub)
    torch.cuda.synchronize()
    for got, ref in zip((out5,) + tuple(v5), outs[True]):
        assert np.array_equal(got.cpu().numpy(), ref[idx])


def _list_case(cfg, B, M, seed, now, first_tick=False, snap=False):
    """random walks -> device lists through the forward kernels: (solver, plan, prev, lists, ok, land) on the device.  Times on the grid, or (snap) the
    walks' own off-grid times with forceSampleTime in front of the merge; the previous tick's list then carries the snapped times."""
    import torch
    dt = cfg.sampling_time
    walks = _random_walks(cfg, B, seed, t_end=3.0)
    for w in walks if not snap else []:
        for lst in w.values():
            for ct in lst:
                ct.activation_time = round(ct.activation_time / dt) * dt
                ct.deactivation_time = ct.deactivation_time if ct.deactivation_time >= 1e9 else round(ct.deactivation_time / dt) * dt
    plan = pack_lists(cfg, walks, max_contacts=M)
    prev = (plan[0].copy(), plan[1].copy(), plan[2].copy())
    if not first_tick:
        plan[0][5] += 50.0       # problem 5: the merge fails (a stance foot the planner does not know)
    s = cm.BatchSolver(cfg, B)
    dev = lambda t: tuple(torch.from_numpy(a).cuda() for a in t)
    dplan, dprev = dev(plan), dev(prev)
    if first_tick:
        lists, ok = tuple(a.clone() for a in dprev), None
    elif snap:
        snapped, ok_snap = s.contacts_force_sample_time_device(dplan[0], dplan[2])
        dprev = (s.contacts_force_sample_time_device(dprev[0], dprev[2])[0], dprev[1], dprev[2])
        lists, ok = s.contacts_merge_device(now, (snapped, dplan[1], dplan[2]), dprev)
        ok = ok & ok_snap
    else:
        lists, ok = s.contacts_merge_device(now, dplan, dprev)
    dPar = torch.zeros((B, cm.Layout(cfg.N).np), dtype=torch.float32, device="cuda")
    land = s.contacts_sample_device(now, lists, dPar)
    torch.cuda.synchronize()
    return s, dplan, dprev, lists, ok, land


@pytest.mark.parametrize("M,first_tick,now_k,snap", [(12, False, 9, False), (12, False, 22, False), (12, True, 0, False), (20, False, 14, False),
                                                     (12, False, 11, True)])
def test_list_adjoint_kernel_equals_the_restatement(M, first_tick, now_k, snap):
    """float64 sums of float32-exact inputs in a fixed order (the entry's own dGradListOut, then the sampling's terms stage by stage, k = 0 .. N-1, within
    stage 0 nominalPos_0, currentPos, nominalPos_1): equal to the restatement to 1e-12; the first tick, a failed merge (zero outputs, status 5) and
    max_contacts above 16 included, and off-grid planner times with force_sample_time."""
    _check_list_adjoint(cm.config.ergocub_gazebo_v1(20, 0.06), M, first_tick, now_k, snap)


def _check_list_adjoint(cfg, M, first_tick, now_k, snap):
    """the body of test_list_adjoint_kernel_equals_the_restatement at cfg's horizon and sampling time"""
    import torch
    L = cm.Layout(cfg.N)
    B = 24
    now = cfg.sampling_time * now_k
    s, dplan, dprev, lists, ok, land = _list_case(cfg, B, M, 17, now, first_tick, snap)
    rng = np.random.default_rng(3)
    gout = rng.normal(size=(B, 2, M, 3))
    gp = rng.normal(size=(B, L.np)).astype(np.float32)
    gx0 = rng.normal(size=(B, L.nx)).astype(np.float32)
    gplan0 = rng.normal(size=(B, 2, M, 3))
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dgx, dgplan = cu(gx0), cu(gplan0)
    gprev, status = s.contacts_position_vjp_device(now, lists[0], lists[2], land, plan=None if first_tick else (dplan[0], dplan[2]),
                                                   prev=None if first_tick else (dprev[0], dprev[2]), ok=ok, dGradListOut=cu(gout), dGradP=cu(gp),
                                                   dGradX=dgx, dGradPlan=dgplan, phase=3, force_sample_time=snap)
    # the two phases apart give the same as both at once
    dgx2, dgplan2 = cu(gx0), cu(gplan0)
    kw = dict(plan=None if first_tick else (dplan[0], dplan[2]), prev=None if first_tick else (dprev[0], dprev[2]), ok=ok, dGradListOut=cu(gout),
              force_sample_time=snap)
    s.contacts_position_vjp_device(now, lists[0], lists[2], land, dGradX=dgx2, phase=1, **kw)
    gprev2, _ = s.contacts_position_vjp_device(now, lists[0], lists[2], land, dGradP=cu(gp), dGradPlan=dgplan2, phase=2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dgx, dgx2) and torch.equal(dgplan, dgplan2) and torch.equal(gprev, gprev2)
    gprev, status, gx, gplan = gprev.cpu().numpy(), status.cpu().numpy(), dgx.cpu().numpy(), dgplan.cpu().numpy()
    lt, ln, ld = lists[0].cpu().numpy(), lists[2].cpu().numpy(), land.cpu().numpy()
    okh = np.ones(B, int) if ok is None else ok.cpu().numpy()
    pt, pn, vt, vn = (a.cpu().numpy() for a in (dplan[0], dplan[2], dprev[0], dprev[2]))
    worst, adjusted = 0.0, 0
    for b in range(B):
        r = rar.list_position_vjp(L, cfg.sampling_time, now, lt[b], ln[b], ld[b], plan=None if first_tick else (pt[b], pn[b]),
                                  prev=None if first_tick else (vt[b], vn[b]), ok=bool(okh[b]), g_out=gout[b], g_p=gp[b], force_sample_time=snap)
        assert status[b] == r["status"]
        for got, ref in ((gprev[b], r["prev"]), (gplan[b] - gplan0[b], r["plan"])):
            scale = max(np.abs(ref).max(), 1.0)
            worst = max(worst, float(np.abs(got - ref).max() / scale))
        assert np.array_equal(gx[b], (gx0[b].astype(np.float64) + r["x"]).astype(np.float32))     # one float32 sum per entry: exact
        adjusted += int(r["x"].any())
    print(f"\nlist adjoint kernel N={cfg.N} dt={cfg.sampling_time} M={M} first_tick={first_tick} now={now:.2f}: worst gap {worst:.2e} (bound {F64:.0e}), feet adjusted in {adjusted} problems")
    assert worst <= F64
    if not first_tick:
        assert status[5] == 5 and okh[5] == 0 and not gprev[5].any() and np.array_equal(gx[5], gx0[5]) and np.array_equal(gplan[5], gplan0[5])
        assert (np.delete(status, 5) == 0).all()
    assert adjusted > 0 or now_k == 0


# ---------------------------------------------------------------------------------------------------------------- ticks
def _walk(B, ticks, seed=5, tape=True, cfg=None, plan=None, push_newton=20.0, **kw):
    """the walk of tests/test_gpu_rollout.py (pushed for three ticks), taped; cfg / plan: another configuration and gait (tests/test_gpu_rollout_horizons.py),
    push_newton: the pushes are U(-push_newton, push_newton) N in x and y"""
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06) if cfg is None else cfg
    rng = np.random.default_rng(seed)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3))
    push[:, :2] = rng.uniform(-push_newton, push_newton, (B, 2)) / cm.synthetic.ROBOT_MASS
    ro = cm.rollout.WalkingRollout(cfg, B, plan=plan, **kw)
    rec = ro.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, tape=tape)
    return cfg, ro, rec


def _host_tape(tk, b):
    """problem b of one taped tick as the restatement's tape"""
    h = lambda k: tk[k][b].cpu().numpy()
    return dict(X=h("X"), P=h("P"), lam_g=h("lam_g"), state=h("state"), status=int(h("info")[5]), ok=bool(h("ok")), land=h("land"),
                list_t=h("list_t"), list_n=h("list_n"), plan=(h("plan_t"), h("plan_n")), prev=None if tk["prev_t"] is None else (h("prev_t"), h("prev_n")),
                step=float(np.float32(tk["step"])), substeps=tk["substeps"], force_sample_time=tk["force_sample_time"])


GROUPS = ("state", "prev_list", "wrench", "plan", "model", "p")


def test_tick_vjp_matches_the_restatement_on_taped_walking_ticks():
    """cmpc_rollout_tick_vjp_device on ticks 2 (before lift-off), 8 (swing), 14 (landing) and 18 (after) of the 24-tick walk against the restatement fed
    with the tape's own float32 (x, p, lam_g): every output group <= REF.  cmpc_solution_vjp_model_device alone is measured on the same ticks against
    sens_model_ref with the same input; the glue around it is exact float64, so the tick's gap on dl/dp and dl/dtheta stays within twice the bare VJP's."""
    import torch
    B = 8
    cfg, ro, rec = _walk(B, 24)
    assert all(rec["converged"]) and all(rec["merge_ok"])
    L = cm.Layout(cfg.N)
    ticks = rec["tape"]["ticks"]
    M = ticks[0]["list_t"].shape[2]
    rng = np.random.default_rng(21)
    worst = {k: 0.0 for k in GROUPS}
    bare = dict(p=0.0, model=0.0)
    s = ro.solver
    for i in (2, 8, 14, 18):
        tk = ticks[i]
        g_state, g_list = rng.normal(size=(B, 9)), rng.normal(size=(B, 2, M, 3)) * 0.1
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        gplan, gmodel = torch.zeros((B, 2, M, 3), dtype=torch.float64, device="cuda"), torch.zeros((B, 34), dtype=torch.float64, device="cuda")
        r = s.rollout_tick_vjp_device(tk["now"], tk, cu(g_state), cu(g_list), dGradPlan=gplan, dGradModel=gmodel, grad_p=True)
        # the bare solution VJP with the input the tick gave it: plant VJP, then the adjust part of the list VJP
        _, gx, _, _ = s.plant_step_vjp_device(tk["X"], tk["P"], tk["state"], cu(g_state), step=tk["step"], substeps=tk["substeps"])
        s.contacts_position_vjp_device(tk["now"], tk["list_t"], tk["list_n"], tk["land"], plan=(tk["plan_t"], tk["plan_n"]), prev=(tk["prev_t"], tk["prev_n"]),
                                       ok=tk["ok"], dGradListOut=cu(g_list), dGradX=gx, phase=1)
        bm, bp, _ = s.solution_vjp_model_device(tk["X"], tk["P"], tk["lam_g"], gx)
        torch.cuda.synchronize()
        assert (r["sens"][:, 0] == 0).all(), r["sens"][:, 0]
        got = dict(state=r["state"], prev_list=r["prev_list"], wrench=r["wrench"], plan=gplan, model=gmodel, p=r["p"])
        got = {k: v.cpu().numpy() for k, v in got.items()}
        bm, bp, gxh = bm.cpu().numpy(), bp.cpu().numpy(), gx.cpu().numpy()
        for b in (0, 5):
            ref = rar.tick_vjp(cfg, _host_tape(tk, b), tk["now"], g_state[b], g_list[b])
            assert ref["status"] == 0
            assert _rel(gxh[b], ref["gx"]) <= 1e-6                       # (float32 against float64 of the same exact glue)
            gaps = {k: _rel(got[k][b], ref[k]) for k in GROUPS}
            bgap = dict(p=_rel(bp[b], ref["p_sol"]), model=_rel(bm[b], ref["model_sol"]))
            print(f"tick {i} problem {b} land {tk['land'][b].tolist()} weak {ref['weak']}: tick " + " ".join(f"{k} {v:.1e}" for k, v in gaps.items()) +
                  "  bare VJP " + " ".join(f"{k} {v:.1e}" for k, v in bgap.items()))
            for k in GROUPS:
                worst[k] = max(worst[k], gaps[k])
            for k in bare:
                bare[k] = max(bare[k], bgap[k])
                assert gaps[k] <= 2 * bgap[k] + 1e-6, (i, b, k, gaps[k], bgap[k])      # (1e-6: the float32 sums of the solve's and the plant's parts)
    print("tick VJP against the restatement, worst: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {REF:.0e});  bare solution VJP: " +
          " ".join(f"{k} {v:.2e}" for k, v in bare.items()))
    assert max(worst.values()) <= REF, worst


def test_tick_vjp_flags_zero_outputs_and_leave_neighbours_alone():
    """One batch with four flagged problems: 1 stopped unconverged by the warm policy's iteration budget (an ordinary status-1 return, spliced in from a
    roll-out with warm_budget=3 and no retry) -> 4; 3 a NaN state -> 2; 4 a model row that breaks the model rule -> 3; 6 a failed merge -> 5.  Zero
    outputs, nothing added to the += outputs, and the neighbours bit-identical to the same batch with clean rows in those places."""
    import torch
    B = 8
    cfg, ro, rec = _walk(B, 4)
    _, ro_bad, rec_bad = _walk(B, 4, warm_budget=3, retry=None)
    # the first warm tick of the budget-3 roll-out with a status-1 problem: that problem's row goes into row 1 of the good roll-out's tape of the same tick
    found = [(i, int(j)) for i in (1, 2, 3) for j in (rec_bad["tape"]["ticks"][i]["info"][:, 5] == 1).nonzero().flatten().tolist()]
    assert found, "the budget of 3 iterations left no problem unconverged"
    i, j = found[0]
    tk, tb = dict(rec["tape"]["ticks"][i]), rec_bad["tape"]["ticks"][i]
    assert float(tb["info"][j, 5]) == 1.0 and (rec["tape"]["ticks"][i]["info"][:, 5] == 0).all()
    M = tk["list_t"].shape[2]
    clean = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in tk.items()}
    for k in ("X", "P", "lam_g", "state", "info", "land", "list_t", "list_n", "prev_t", "prev_n"):
        tk[k] = tk[k].clone()
        tk[k][1] = tb[k][j]
    tk["state"][3] = float("nan")
    tk["ok"] = tk["ok"].clone()
    tk["ok"][6] = 0
    theta = np.tile(cm.config.model_row(cfg), (B, 1))
    bad_theta = theta.copy()
    bad_theta[4, 0] = -1.0
    rng = np.random.default_rng(2)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g_state, g_list, g_x = cu(rng.normal(size=(B, 9))), cu(rng.normal(size=(B, 2, M, 3)) * 0.1), cu(rng.normal(size=(B, cm.Layout(cfg.N).nx)).astype(np.float32) * 0.01)
    plan0, model0 = rng.normal(size=(B, 2, M, 3)), rng.normal(size=(B, 34))
    res = []
    for tape, th in ((tk, bad_theta), (clean, theta)):
        ok_models = ro.solver.set_models_device(cu(th))
        gplan, gmodel = cu(plan0), cu(model0)
        r = ro.solver.rollout_tick_vjp_device(tape["now"], tape, g_state, g_list, g_x, dGradPlan=gplan, dGradModel=gmodel, grad_p=True)
        torch.cuda.synchronize()
        res.append({k: v.cpu().numpy() for k, v in dict(r, plan=gplan, model=gmodel, ok_models=ok_models).items()})
    a, c = res
    assert a["ok_models"][4] == 0 and c["ok_models"].all()
    flagged = {1: 4, 3: 2, 4: 3, 6: 5}
    assert (c["sens"][:, 0] == 0).all(), c["sens"][:, 0]
    for b in range(B):
        if b in flagged:
            assert a["sens"][b, 0] == flagged[b], (b, a["sens"][b])
            for k in ("state", "prev_list", "wrench", "p"):
                assert not a[k][b].any(), (b, k)
            assert np.array_equal(a["plan"][b], plan0[b]) and np.array_equal(a["model"][b], model0[b])
        else:
            assert a["sens"][b, 0] == 0
            for k in ("state", "prev_list", "wrench", "p", "plan", "model", "sens"):
                assert np.array_equal(a[k][b], c[k][b]), (b, k)
            assert a["state"][b].any() and a["p"][b].any()


def test_taped_rollout_is_bit_identical_to_the_untaped_one():
    """x and info are bit-identical with the multiplier output on: every tick's P, X0 and info (the `slow` hook: X0 of tick i+1 is the shifted X of tick i,
    P carries the sampled lists and the state), CoM, ZMP, landing knots and landing offsets (from X) agree to the last bit -- native tick and step-by-step."""
    B, ticks = 16, 8
    for native in (True, False):
        runs = []
        for tape in (False, True):
            cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
            rng = np.random.default_rng(5)
            com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
            dcom0, h0 = rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.02, 0.02, (B, 3))
            push = np.zeros((B, 3))
            push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
            ro = cm.rollout.WalkingRollout(cfg, B, native_tick=native)
            every = []
            rec = ro.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, slow=(-1, every), tape=tape)
            runs.append((rec, every))
        (ra, ea), (rb, eb) = runs
        assert all(ra["converged"]) and len(ea) == len(eb) == B * ticks
        for key in ("com", "zmp", "land", "landing_offset"):
            assert np.array_equal(np.stack(ra[key]), np.stack(rb[key]), equal_nan=True), (native, key)
        assert ra["iterations_max"] == rb["iterations_max"] and ra["iterations_mean"] == rb["iterations_mean"]
        for (i1, b1, P1, X01, I1), (i2, b2, P2, X02, I2) in zip(ea, eb):
            # (info word 6 is the solve's shader-clock count, a time: every other word is compared)
            assert (i1, b1) == (i2, b2) and np.array_equal(P1, P2) and np.array_equal(X01, X02) and np.array_equal(np.delete(I1, 6), np.delete(I2, 6)), (native, i1, b1)
        tape = rb["tape"]
        assert len(tape["ticks"]) == ticks and np.array_equal(tape["state"].cpu().numpy()[:, 0:3], ra["com"][-1])
        assert np.array_equal(tape["ticks"][3]["state"].cpu().numpy()[:, 0:3], ra["com"][2])       # the state that went INTO tick 3


def test_closed_loop_transition_matches_nine_reverse_sweeps_of_one_tick():
    """A_cl = d state' / d state of one tick, forward mode (the nine-column JVP through the plant JVP), against the rows the reverse path gives for unit
    dGradStateOut: <= ADJ of the largest entry."""
    import torch
    B = 8
    cfg, ro, rec = _walk(B, 8)
    s = ro.solver
    worst = 0.0
    for i in (1, 7):
        tk = rec["tape"]["ticks"][i]
        A, sens = s.closed_loop_transition_device(tk["X"], tk["P"], tk["lam_g"], tk["state"], step=tk["step"], substeps=tk["substeps"])
        rows = []
        for r in range(9):
            e = torch.zeros((B, 9), dtype=torch.float64, device="cuda")
            e[:, r] = 1.0
            out = s.rollout_tick_vjp_device(tk["now"], tk, e)
            assert (out["sens"][:, 0] == 0).all()
            rows.append(out["state"])
        At = torch.stack(rows, 1)
        torch.cuda.synchronize()
        assert (sens[:, 0] == 0).all()
        A, At = A.cpu().numpy(), At.cpu().numpy()
        for b in range(B):
            worst = max(worst, _rel(A[b], At[b]))
        assert np.abs(A - np.eye(9)).max() > 1e-2          # not the identity: the feedback is there
    print(f"\nclosed-loop transition, forward against reverse: worst gap {worst:.2e} (bound {ADJ:.0e})")
    assert worst <= ADJ


def test_backward_matches_the_restated_sweep_and_autograd_descends():
    """WalkingRollout.backward over 6 ticks of the walk against the restatement's reverse sweep on the same tape: <= 6 x REF per output group (a tick's
    error travels on through the same Jacobians as the gradient, so relative errors add up tick by tick).  rollout_differentiable: state0.grad, push.grad
    and models.grad equal backward's bit for bit, and one small gradient step on the CoM cost weights lowers sum |com_T - target|^2 on a batch standing
    under a push."""
    import torch
    B, T = 4, 6
    cfg, ro, rec = _walk(B, T, seed=7)
    assert all(rec["converged"])
    tape = rec["tape"]
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(4)
    gS = rng.normal(size=(T + 1, B, 9))
    out = ro.backward(tape, gS)
    torch.cuda.synchronize()
    assert (out["status"] == 0).all()
    got = {k: out[k].cpu().numpy() for k in ("state0", "list0", "push", "models", "plan", "wrench")}
    worst = {k: 0.0 for k in got}
    for b in (0, 2):
        tapes = [_host_tape(tk, b) for tk in tape["ticks"]]
        ref = rar.reverse_sweep(cfg, tapes, [tk["now"] for tk in tape["ticks"]], gS[:, b], push_knots=[tk["push_knots"] for tk in tape["ticks"]])
        assert ref["status"] == [0] * T
        for k in got:
            g = got[k][:, b] if k == "wrench" else got[k][b]
            worst[k] = max(worst[k], _rel(g, ref[k]))
    print("\nbackward over 6 ticks against the restated sweep: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {6 * REF:.0e})")
    assert max(worst.values()) <= 6 * REF, worst
    # autograd on a batch standing under a push
    B = 16
    names = [c.contact_name for c in cfg.contacts]
    stand = {names[0]: [PlannedContact(0.0, 1e9, (0.0, 0.08, 0.0))], names[1]: [PlannedContact(0.0, 1e9, (0.0, -0.08, 0.0))]}
    ro = cm.rollout.WalkingRollout(cfg, B, plan=stand, com_speed=0.0)
    rng = np.random.default_rng(12)
    s0 = np.concatenate([np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3)), rng.uniform(-0.05, 0.05, (B, 3)), np.zeros((B, 3))], 1)
    pushv = np.zeros((B, 3))
    pushv[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    theta = np.tile(cm.config.model_row(cfg), (B, 1))
    target = torch.tensor([0.0, 0.0, 0.7], device="cuda")

    def loss_of(models):
        state0 = torch.from_numpy(s0.astype(np.float32)).cuda().requires_grad_(True)
        push = torch.from_numpy(pushv.astype(np.float32)).cuda().requires_grad_(True)
        states = cm.rollout_differentiable(ro, 5, state0, push=push, models=models, push_ticks=3)
        return ((states[-1][:, 0:3] - target) ** 2).sum(), state0, push, states
    models = torch.from_numpy(theta).cuda().requires_grad_(True)
    loss, state0, push, states = loss_of(models)
    loss.backward()
    gS = torch.zeros((6, B, 9), dtype=torch.float64, device="cuda")
    gS[5, :, 0:3] = (2 * (states.detach()[-1][:, 0:3] - target)).to(torch.float64)
    ref = ro.backward(ro.last_tape, gS)
    torch.cuda.synchronize()
    assert (ro.last_backward["status"] == 0).all()
    assert torch.equal(state0.grad, ref["state0"].to(torch.float32)) and torch.equal(push.grad, ref["push"].to(torch.float32))
    assert torch.equal(models.grad, ref["models"])
    assert float(models.grad[:, 1:3].abs().max()) > 0
    step = models.grad[:, 1:3]
    alpha = 0.1 * float(theta[0, 1]) / float(step.abs().max())           # the largest change: a tenth of the weight
    m2 = models.detach().clone()
    m2[:, 1:3] -= alpha * step
    assert (m2[:, 1:3] > 0).all()
    loss2 = loss_of(m2)[0]
    print(f"loss {float(loss.detach()):.6e} -> {float(loss2.detach()):.6e}")
    assert float(loss2.detach()) < float(loss.detach())
