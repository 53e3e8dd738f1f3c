"""GPU: the roll-out tick in reverse with the contacts' orientations (include/cmpc.h: cmpc_plant_step_jvp_rot_device / _vjp_rot_device,
cmpc_contacts_orientation_vjp_device, cmpc_rollout_tick_vjp_rot_device; WalkingRollout.backward(rot=True), rollout_differentiable(plan_yaw=...)) against its
float64 restatement tests/rollout_rot_ref.py at the same float32 inputs.  Bounds: those of tests/test_gpu_rollout_adjoint.py, relative to the largest
entry of the output group compared -- F64 for float64 glue on both sides, REF for kernels against the restatement through a solve, ADJ for the adjoint
identity on float32 device outputs, 6 x REF for six chained ticks.  No other tolerance."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import rollout_adjoint_ref as rar
from tests import rollout_rot_ref as rrr
from tests.test_gpu_rollout_adjoint import ADJ, F64, GROUPS, REF, ULP32, _host_tape, _list_case, _plant_inputs, _rel

pytestmark = pytest.mark.gpu

EPS64 = 2.0 ** -52
ROT_GROUPS = ("prev_list_rot", "plan_rot", "rot")


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_plant_rot_kernels_match_the_restatement():
    """B = 16, N = 20, the inputs of the plant test (yawed feet, one foot of every third problem gated off, per-problem corners).  The JVP with dDirRot0
    and the VJP's dGradRot0 against the restatement <= F64; the adjoint identity with the rotation term <= ADJ; with the rotation pointer NULL every
    output is bit-equal to the existing entry points'; bit-identical in a batch of 5 holding problems 11, 3, 7, 0, 15; a gated-off foot has zero
    dGradRot0."""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    L = cm.Layout(cfg.N)
    B, step, nsub = 16, 0.01, 6
    X, P, state, models = _plant_inputs(cfg, B, 4)
    rng = np.random.default_rng(9)
    dS, dM, g = rng.normal(size=(B, 9)), rng.normal(size=(B, 34)), rng.normal(size=(B, 9))
    dX, dP = rng.normal(size=(B, L.nx)).astype(np.float32), rng.normal(size=(B, L.np)).astype(np.float32)
    dR = rng.normal(size=(B, 2, 3))
    s = cm.BatchSolver(cfg, B)
    s.set_models(models)
    kw = dict(step=step, substeps=nsub)
    out = s.plant_step_jvp_device(_cu(X), _cu(P), _cu(state), _cu(dS), _cu(dX), _cu(dP), _cu(dM), dDirRot0=_cu(dR), **kw)
    out_r = s.plant_step_jvp_device(_cu(X), _cu(P), _cu(state), _cu(np.zeros((B, 9))), dDirRot0=_cu(dR), **kw)      # the rotation direction alone
    out0 = s.plant_step_jvp_device(_cu(X), _cu(P), _cu(state), _cu(dS), _cu(dX), _cu(dP), _cu(dM), **kw)
    v = s.plant_step_vjp_device(_cu(X), _cu(P), _cu(state), _cu(g), grad_rot=True, **kw)
    v0 = s.plant_step_vjp_device(_cu(X), _cu(P), _cu(state), _cu(g), **kw)
    # the new entry points with the rotation pointer NULL, through the C ABI
    lib, null_out = cm._capi.lib(), torch.empty((B, 9), dtype=torch.float64, device="cuda")
    nS, nX = torch.empty((B, 9), dtype=torch.float64, device="cuda"), torch.empty((B, L.nx), dtype=torch.float32, device="cuda")
    nP, nM = torch.empty((B, L.np), dtype=torch.float32, device="cuda"), torch.empty((B, 34), dtype=torch.float64, device="cuda")
    dXc, dPc, dSt = _cu(X), _cu(P), _cu(state)
    a_dS, a_dX, a_dP, a_dM, a_g = _cu(dS), _cu(dX), _cu(dP), _cu(dM), _cu(g)
    s._launch(dXc.device, lambda st: lib.cmpc_plant_step_jvp_rot_device(s._h, dXc.data_ptr(), dPc.data_ptr(), dSt.data_ptr(), step, nsub, a_dS.data_ptr(),
                                                                        a_dX.data_ptr(), a_dP.data_ptr(), a_dM.data_ptr(), None, null_out.data_ptr(), st))
    s._launch(dXc.device, lambda st: lib.cmpc_plant_step_vjp_rot_device(s._h, dXc.data_ptr(), dPc.data_ptr(), dSt.data_ptr(), step, nsub, a_g.data_ptr(),
                                                                        nS.data_ptr(), nX.data_ptr(), nP.data_ptr(), nM.data_ptr(), None, st))
    torch.cuda.synchronize()
    assert torch.equal(null_out, out0)
    for got, ref in zip((nS, nX, nP, nM), v0):
        assert torch.equal(got, ref)
    for got, ref in zip(v[:4], v0):                      # asking for dGradRot0 changes no other output
        assert torch.equal(got, ref)
    out, out_r, out0, gR = (a.cpu().numpy() for a in (out, out_r, out0, v[4]))
    gS, gX, gP, gM = (a.cpu().numpy() for a in v[:4])
    worst = dict(jvp=0.0, jvp_rot=0.0, g_rot=0.0, adjoint=0.0, adjoint_rot=0.0)
    grav = float(np.float32(rar.GRAVITY))
    gated = 0
    for b in range(B):
        corners = models[b, 10:].astype(np.float32).astype(np.float64)
        args = (L, corners, X[b], P[b], state[b], float(np.float32(step)), nsub)
        worst["jvp"] = max(worst["jvp"], _rel(out[b], rrr.plant_jvp(*args, dS[b], dX[b], dP[b], dM[b], dR[b], gravity=grav)))
        r_rot = rrr.plant_jvp(*args, np.zeros(9), d_rot0=dR[b], gravity=grav)
        worst["jvp_rot"] = max(worst["jvp_rot"], _rel(out_r[b], r_rot))
        r_g = rrr.plant_vjp(*args, g[b], gravity=grav)[4]
        worst["g_rot"] = max(worst["g_rot"], _rel(gR[b], r_g))
        lhs = g[b] @ out[b]
        rhs = gS[b] @ dS[b] + gX[b].astype(np.float64) @ dX[b] + gP[b].astype(np.float64) @ dP[b] + gM[b] @ dM[b] + (gR[b] * dR[b]).sum()
        worst["adjoint"] = max(worst["adjoint"], abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        lhs, rhs = g[b] @ out_r[b], (gR[b] * dR[b]).sum()
        worst["adjoint_rot"] = max(worst["adjoint_rot"], abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        for c in range(2):
            if not P[b, L.p_gam[c]] > 0.5:
                gated += 1
                assert not gR[b, c].any() and gR[b, 1 - c].any()
            else:
                assert gR[b, c].any()
    print("\nplant rotation kernels against the restatement: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"  (bounds: float64 groups {F64:.0e}, adjoint {ADJ:.0e}); gated-off feet {gated}")
    assert worst["jvp"] <= F64 and worst["jvp_rot"] <= F64 and worst["g_rot"] <= F64 and worst["adjoint"] <= ADJ and worst["adjoint_rot"] <= ADJ
    assert gated >= 4 and not np.array_equal(out, out0)
    idx = [11, 3, 7, 0, 15]
    s5 = cm.BatchSolver(cfg, 5)
    s5.set_models(models[idx])
    out5 = s5.plant_step_jvp_device(_cu(X[idx]), _cu(P[idx]), _cu(state[idx]), _cu(dS[idx]), _cu(dX[idx]), _cu(dP[idx]), _cu(dM[idx]), dDirRot0=_cu(dR[idx]), **kw)
    v5 = s5.plant_step_vjp_device(_cu(X[idx]), _cu(P[idx]), _cu(state[idx]), _cu(g[idx]), grad_rot=True, **kw)
    torch.cuda.synchronize()
    for got, ref in zip((out5,) + tuple(v5), (out, gS, gX, gP, gM, gR)):
        assert np.array_equal(got.cpu().numpy(), ref[idx])


@pytest.mark.parametrize("M,first_tick,now_k,snap", [(12, False, 9, False), (12, False, 22, False), (12, True, 0, False), (20, False, 14, False),
                                                     (12, False, 11, True)])
def test_list_orientation_kernel_equals_the_restatement(M, first_tick, now_k, snap):
    """The cases of the position list test (B = 24; problem 5's merge fails).  float64 sums in a fixed order (the entry's own dGradListRotOut, then the
    stages it owns, k = 0 .. N-1): equal to list_orientation_vjp to F64.  The failed merge gives zeros, status 5, and leaves dGradPlanRot untouched.
    The landing entry's gradient DOES reach the output, where the position kernel cuts it.  With dGradListRotOut = None and a one-tick list the result
    is bit-equal to cmpc_contacts_rotation_vjp_device's."""
    _check_list_orientation(cm.config.ergocub_gazebo_v1(20, 0.06), M, first_tick, now_k, snap)


def _check_list_orientation(cfg, M, first_tick, now_k, snap):
    """the body of test_list_orientation_kernel_equals_the_restatement at cfg's horizon and sampling time"""
    import torch
    L, N = cm.Layout(cfg.N), cfg.N
    B = 24
    now = cfg.sampling_time * now_k
    s, dplan, dprev, lists, ok, land = _list_case(cfg, B, M, 17, now, first_tick, snap)
    rng = np.random.default_rng(3)
    gout, grot, gplan0 = rng.normal(size=(B, 2, M, 3)), rng.normal(size=(B, 2, N, 3)), rng.normal(size=(B, 2, M, 3))
    kw = dict(plan=None if first_tick else (dplan[0], dplan[2]), prev=None if first_tick else (dprev[0], dprev[2]), ok=ok, force_sample_time=snap)
    dgplan = _cu(gplan0)
    gprev, status = s.contacts_orientation_vjp_device(now, lists[0], lists[2], land, dGradListRotOut=_cu(gout), dGradRot=_cu(grot), dGradPlanRot=dgplan, **kw)
    # the position kernel on the same cotangent of the outgoing list alone: the landing entry is cut there
    dgplan_p, dgplan_o = _cu(gplan0), _cu(gplan0)
    ppos, _ = s.contacts_position_vjp_device(now, lists[0], lists[2], land, dGradListOut=_cu(gout), phase=2, dGradPlan=dgplan_p, **kw)
    pori, _ = s.contacts_orientation_vjp_device(now, lists[0], lists[2], land, dGradListRotOut=_cu(gout), dGradPlanRot=dgplan_o, **kw)
    torch.cuda.synchronize()
    gprev, status, gplan = gprev.cpu().numpy(), status.cpu().numpy(), dgplan.cpu().numpy()
    cut = (pori.cpu().numpy() - ppos.cpu().numpy()) + (dgplan_o.cpu().numpy() - dgplan_p.cpu().numpy())     # what the position kernel cut, per destination
    lt, ln, ld = lists[0].cpu().numpy(), lists[2].cpu().numpy(), land.cpu().numpy()
    okh = np.ones(B, int) if ok is None else ok.cpu().numpy()
    pt, pn, vt, vn = (a.cpu().numpy() for a in (dplan[0], dplan[2], dprev[0], dprev[2]))
    worst, landing = 0.0, 0
    for b in range(B):
        hk = dict(plan=None if first_tick else (pt[b], pn[b]), prev=None if first_tick else (vt[b], vn[b]), ok=bool(okh[b]), force_sample_time=snap)
        r = rrr.list_orientation_vjp(L, cfg.sampling_time, now, lt[b], ln[b], ld[b], g_out=gout[b], g_rot=grot[b], **hk)
        assert status[b] == r["status"]
        for got, ref in ((gprev[b], r["prev"]), (gplan[b] - gplan0[b], r["plan"])):
            worst = max(worst, float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0)))
        # a landing inside the horizon: what arrives from dGradListRotOut[nx] is all there in the orientation outputs and missing from the position ones
        for c in range(2):
            if okh[b] and 0 <= ld[b, c] <= N and 1 <= ln[b, c] <= M:
                nx = rar._next(rar._as_list(lt[b, c], ln[b, c]), rar._ns(now))
                if nx < 0:
                    continue
                landing += 1
                only = np.zeros((2, M, 3))
                only[c, nx] = gout[b, c, nx]
                ro = rrr.list_orientation_vjp(L, cfg.sampling_time, now, lt[b], ln[b], ld[b], g_out=only, **hk)
                assert ro["prev"].any() or ro["plan"].any()
                assert np.abs(cut[b, c]).max() > 0 and np.abs(cut[b, c] - (ro["prev"][c] + ro["plan"][c])).max() <= F64 * np.abs(gout).max(), (b, c)
    print(f"\nlist orientation kernel N={cfg.N} dt={cfg.sampling_time} M={M} first_tick={first_tick} now={now:.2f} snap={snap}: worst gap {worst:.2e} (bound {F64:.0e}), "
          f"feet with a landing entry passed through: {landing}")
    assert worst <= F64
    if not first_tick:
        assert status[5] == 5 and okh[5] == 0 and not gprev[5].any() and np.array_equal(gplan[5], gplan0[5])
        assert (np.delete(status, 5) == 0).all()
        assert landing > 0
    else:
        # one-tick list, no outgoing gradient: the owner sum of cmpc_contacts_rotation_vjp_device, bit for bit
        a, _ = s.contacts_orientation_vjp_device(now, lists[0], lists[2], land, dGradRot=_cu(grot))
        a2, _ = s.contacts_orientation_vjp_device(now, lists[0], lists[2], None, dGradRot=_cu(grot))
        ref = s.contacts_rotation_vjp_device(now, lists[0], lists[2], _cu(grot))
        torch.cuda.synchronize()
        assert torch.equal(a, ref) and torch.equal(a2, ref) and bool(ref.any())


# ---------------------------------------------------------------------------------------------------------------- ticks
def _yawed_walk(B, ticks, seed=5, yaw_seed=31, plan=None, yaw=None, **kw):
    """the pushed walk of tests/test_gpu_rollout_adjoint.py on a plan whose footsteps (every contact after a foot's first) are yawed per problem by
    U(-0.2, 0.2) rad (or by `yaw`[B, 2, M]), set on ro.plan's quaternions before the run; taped"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    rng = np.random.default_rng(seed)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3))
    push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    ro = cm.rollout.WalkingRollout(cfg, B, plan=plan, **kw)
    M = ro.plan[1].shape[2]
    if yaw is None:
        yaw = np.random.default_rng(yaw_seed).uniform(-0.2, 0.2, (B, 2, M))
        yaw[:, :, 0] = 0.0
    ro.plan = (ro.plan[0], cm.rollout.yaw_plan_poses(ro.plan[1], torch.from_numpy(yaw).cuda()), ro.plan[2])
    rec = ro.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, tape=True)
    return cfg, ro, rec, (com0, dcom0, h0, push)


def test_tick_vjp_rot_matches_the_restatement_on_taped_walking_ticks():
    """cmpc_rollout_tick_vjp_rot_device on ticks 2, 8, 14, 18 of a 24-tick walk over yawed footsteps (B = 8), problems 0 and 5: prev_list_rot, plan_rot and
    rot <= REF of tick_vjp_rot at the tape's own float32 (x, p, lam_g) -- all eight pairs, none excluded; every group the entry without orientations has
    is bit-equal to it on the same tape and inputs; rot on stage 0 minus the bare cmpc_solution_vjp_rot_device result is the plant's dGradRot0 to one
    float64 rounding, and rot beyond stage 0 is the bare result bit for bit."""
    import torch
    B = 8
    cfg, ro, rec, _ = _yawed_walk(B, 24)
    assert all(rec["converged"]) and all(rec["merge_ok"])
    N = cfg.N
    ticks = rec["tape"]["ticks"]
    M = ticks[0]["list_t"].shape[2]
    rng = np.random.default_rng(21)
    worst = {k: 0.0 for k in GROUPS + ROT_GROUPS}
    s = ro.solver
    for i in (2, 8, 14, 18):
        tk = ticks[i]
        g_state, g_list, g_lrot = rng.normal(size=(B, 9)), rng.normal(size=(B, 2, M, 3)) * 0.1, rng.normal(size=(B, 2, M, 3)) * 1e-3
        res = []
        for rot in (False, True):
            gplan, gmodel = torch.zeros((B, 2, M, 3), dtype=torch.float64, device="cuda"), torch.zeros((B, 34), dtype=torch.float64, device="cuda")
            gprot = torch.zeros((B, 2, M, 3), dtype=torch.float64, device="cuda")
            kw = dict(dGradListRotOut=_cu(g_lrot), rot=True, dGradPlanRot=gprot) if rot else {}
            r = s.rollout_tick_vjp_device(tk["now"], tk, _cu(g_state), _cu(g_list), dGradPlan=gplan, dGradModel=gmodel, grad_p=True, **kw)
            res.append(dict(r, plan=gplan, model=gmodel, plan_rot=gprot))
        old, new = res
        # the bare rotation VJP with the input the tick gave it, and the plant's own part
        _, gx, _, _, gR0 = s.plant_step_vjp_device(tk["X"], tk["P"], tk["state"], _cu(g_state), step=tk["step"], substeps=tk["substeps"], grad_rot=True)
        s.contacts_position_vjp_device(tk["now"], tk["list_t"], tk["list_n"], tk["land"], plan=(tk["plan_t"], tk["plan_n"]), prev=(tk["prev_t"], tk["prev_n"]),
                                       ok=tk["ok"], dGradListOut=_cu(g_list), dGradX=gx, phase=1)
        bare = s.solution_vjp_rot_device(tk["X"], tk["P"], tk["lam_g"], gx)[0]
        torch.cuda.synchronize()
        assert (new["sens"][:, 0] == 0).all() and (old["sens"][:, 0] == 0).all()
        for k in ("state", "prev_list", "wrench", "plan", "model", "p"):
            assert torch.equal(old[k], new[k]), (i, k)
        got = {k: new[k].cpu().numpy() for k in ROT_GROUPS + GROUPS}
        bare, gR0, sens = bare.cpu().numpy(), gR0.cpu().numpy(), new["sens"].cpu().numpy()
        assert np.array_equal(got["rot"][:, :, 1:], bare[:, :, 1:])
        d0 = got["rot"][:, :, 0] - bare[:, :, 0]
        assert (np.abs(d0 - gR0) <= 2 * EPS64 * np.maximum(np.abs(got["rot"][:, :, 0]), np.abs(bare[:, :, 0]))).all(), np.abs(d0 - gR0).max()
        assert gR0.any()
        print(f"\ntick {i}: dSens[5] (weakly active rows) {sens[:, 5].astype(int).tolist()}  dSens[6] (removed internal-force component) "
              + " ".join(f"{v:.1e}" for v in sens[:, 6]))
        for b in (0, 5):
            ref = rrr.tick_vjp_rot(cfg, _host_tape(tk, b), tk["now"], g_state[b], g_list[b], g_list_rot_out=g_lrot[b])
            assert ref["status"] == 0
            gaps = {k: _rel(got[k][b], ref[k]) for k in GROUPS + ROT_GROUPS}
            print(f"tick {i} problem {b} land {tk['land'][b].tolist()} weak {ref['weak']} removed {ref['removed']:.1e} |rot| {np.abs(ref['rot']).max():.2e} "
                  f"|rot0| {np.abs(ref['rot0']).max():.2e}: " + " ".join(f"{k} {v:.1e}" for k, v in gaps.items()))
            for k in gaps:
                worst[k] = max(worst[k], gaps[k])
    print("tick VJP with orientations against the restatement, worst: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {REF:.0e})")
    assert max(worst.values()) <= REF, worst


def test_tick_vjp_rot_flags_zero_outputs_and_leave_neighbours_alone():
    """The four-flag batch of tests/test_gpu_rollout_adjoint.py (1 not converged -> 4; 3 a NaN state -> 2; 4 a broken model row -> 3; 6 a failed merge
    -> 5) through the rotation entry: zeros in the rotation outputs too, nothing added to dGradPlanRot, neighbours bit-identical to the clean batch."""
    import torch
    B = 8
    cfg, ro, rec, _ = _yawed_walk(B, 4)
    _, ro_bad, rec_bad, _ = _yawed_walk(B, 4, warm_budget=3, retry=None)
    found = [(i, int(j)) for i in (1, 2, 3) for j in (rec_bad["tape"]["ticks"][i]["info"][:, 5] == 1).nonzero().flatten().tolist()]
    assert found, "the budget of 3 iterations left no problem unconverged"
    i, j = found[0]
    tk, tb = dict(rec["tape"]["ticks"][i]), rec_bad["tape"]["ticks"][i]
    assert float(tb["info"][j, 5]) == 1.0 and (rec["tape"]["ticks"][i]["info"][:, 5] == 0).all()
    M, N = tk["list_t"].shape[2], cfg.N
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
    g_state, g_list, g_x = _cu(rng.normal(size=(B, 9))), _cu(rng.normal(size=(B, 2, M, 3)) * 0.1), _cu(rng.normal(size=(B, cm.Layout(N).nx)).astype(np.float32) * 0.01)
    g_lrot = _cu(rng.normal(size=(B, 2, M, 3)))
    plan0, model0, prot0 = rng.normal(size=(B, 2, M, 3)), rng.normal(size=(B, 34)), rng.normal(size=(B, 2, M, 3))
    res = []
    for tape, th in ((tk, bad_theta), (clean, theta)):
        ok_models = ro.solver.set_models_device(_cu(th))
        gplan, gmodel, gprot = _cu(plan0), _cu(model0), _cu(prot0)
        r = ro.solver.rollout_tick_vjp_device(tape["now"], tape, g_state, g_list, g_x, dGradPlan=gplan, dGradModel=gmodel, grad_p=True, dGradListRotOut=g_lrot,
                                              rot=True, dGradPlanRot=gprot)
        torch.cuda.synchronize()
        res.append({k: v.cpu().numpy() for k, v in dict(r, plan=gplan, model=gmodel, plan_rot=gprot, ok_models=ok_models).items()})
    a, c = res
    assert a["ok_models"][4] == 0 and c["ok_models"].all()
    flagged = {1: 4, 3: 2, 4: 3, 6: 5}
    assert (c["sens"][:, 0] == 0).all(), c["sens"][:, 0]
    for b in range(B):
        if b in flagged:
            assert a["sens"][b, 0] == flagged[b], (b, a["sens"][b])
            for k in ("state", "prev_list", "wrench", "p", "prev_list_rot", "rot"):
                assert not a[k][b].any(), (b, k)
            assert np.array_equal(a["plan"][b], plan0[b]) and np.array_equal(a["model"][b], model0[b]) and np.array_equal(a["plan_rot"][b], prot0[b])
        else:
            assert a["sens"][b, 0] == 0
            for k in ("state", "prev_list", "wrench", "p", "plan", "model", "sens", "prev_list_rot", "rot", "plan_rot"):
                assert np.array_equal(a[k][b], c[k][b]), (b, k)
            assert a["rot"][b].any() and a["prev_list_rot"][b].any()


def _landing_scene(B):
    """A short-stepping walk whose left foot lifts at tick 1 and lands at tick 5, inside a 6-tick roll-out, its landing footstep yawed 0.2 rad, under a
    lateral push held for three ticks: the yaw acts through the swing stages' box rows (the push drives the landing position to the box) and, from the
    landing tick on, through the plant's lever arms."""
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    plan = cm.rollout.walking_plan(cfg, steps=6, step_length=0.1, swing=0.24, double_support=0.12, first_lift=0.06)
    ro = cm.rollout.WalkingRollout(cfg, B, plan=plan)
    M = ro.plan[1].shape[2]
    rng = np.random.default_rng(12)
    s0 = np.concatenate([np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3)), rng.uniform(-0.05, 0.05, (B, 3)), np.zeros((B, 3))], 1)
    pushv = np.zeros((B, 3))
    pushv[:, 1] = rng.uniform(25.0, 40.0, B) / cm.synthetic.ROBOT_MASS       # towards the swing (left) foot's side
    yaw0 = np.zeros((B, 2, M))
    yaw0[:, 0, 1] = 0.2
    return cfg, ro, s0, pushv, yaw0


def test_backward_rot_matches_the_restated_sweep_and_autograd_of_plan_yaw():
    """WalkingRollout.backward(rot=True) over 6 ticks of the yawed walk (B = 4) against the restated sweep on problems 0 and 2: <= 6 x REF per group, the
    rotation groups included; every other group bit-equal to rot=False.  rollout_differentiable: plan_yaw = zeros gives states bit-equal to plan_yaw =
    None; plan_yaw.grad is bit-equal to the e_z component of plan_rot + list_rot0 from backward; one gradient step of at most 0.02 rad on plan_yaw lowers
    the loss as a fresh roll-out measures it."""
    import torch
    B, T = 4, 6
    cfg, ro, rec, _ = _yawed_walk(B, T, seed=7)
    assert all(rec["converged"])
    tape = rec["tape"]
    rng = np.random.default_rng(4)
    gS = rng.normal(size=(T + 1, B, 9))
    out = ro.backward(tape, gS, rot=True)
    out0 = ro.backward(tape, gS)
    torch.cuda.synchronize()
    assert (out["status"] == 0).all()
    for k in out0:
        assert torch.equal(out[k], out0[k]), k
    names = ("state0", "list0", "push", "models", "plan", "wrench", "list_rot0", "plan_rot", "rot")
    got = {k: out[k].cpu().numpy() for k in names}
    worst = {k: 0.0 for k in names}
    for b in (0, 2):
        tapes = [_host_tape(tk, b) for tk in tape["ticks"]]
        ref = rrr.reverse_sweep(cfg, tapes, [tk["now"] for tk in tape["ticks"]], gS[:, b], push_knots=[tk["push_knots"] for tk in tape["ticks"]])
        assert ref["status"] == [0] * T
        for k in names:
            g = got[k][:, b] if k in ("wrench", "rot") else got[k][b]
            worst[k] = max(worst[k], _rel(g, ref[k]))
        print(f"\nproblem {b}: |list_rot0| {np.abs(ref['list_rot0']).max():.2e} |plan_rot| {np.abs(ref['plan_rot']).max():.2e} |rot| {np.abs(ref['rot']).max():.2e} "
              f"removed per tick " + " ".join(f"{v:.1e}" for v in ref["removed"]))
    print("backward(rot=True) over 6 ticks against the restated sweep: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {6 * REF:.0e})")
    assert max(worst.values()) <= 6 * REF, worst
    assert got["list_rot0"].any() and got["rot"].any()

    # autograd: a foot yawed 0.2 rad that lands inside the 6 ticks under a lateral push
    B = 8
    cfg, ro, s0, pushv, yaw0 = _landing_scene(B)

    def run(plan_yaw):
        state0 = torch.from_numpy(s0.astype(np.float32)).cuda()
        push = torch.from_numpy(pushv.astype(np.float32)).cuda()
        return cm.rollout_differentiable(ro, T, state0, push=push, push_ticks=3, plan_yaw=plan_yaw)

    def loss_of(states):
        return (states[-1][:, 1] ** 2 + states[-1][:, 4] ** 2 + states[-1][:, 6:9].pow(2).sum(1)).sum()
    plan_before = tuple(a.clone() for a in ro.plan)
    base = run(None)
    zero = run(torch.zeros((B, 2, yaw0.shape[2]), dtype=torch.float64, device="cuda"))
    assert torch.equal(base, zero)
    psi = torch.from_numpy(yaw0).cuda().requires_grad_(True)
    states = run(psi)
    assert all(torch.equal(a, b) for a, b in zip(ro.plan, plan_before))          # the roll-out's own plan is left as it was
    gam = cm.Layout(cfg.N).p_gam[0]
    assert float(ro.last_tape["ticks"][4]["P"][0, gam]) == 0.0 and float(ro.last_tape["ticks"][5]["P"][0, gam]) == 1.0      # the left foot swings, then lands
    loss = loss_of(states)
    loss.backward()
    gS = torch.zeros((T + 1, B, 9), dtype=torch.float64, device="cuda")
    fin = states.detach()[-1].to(torch.float64)
    gS[T, :, 1], gS[T, :, 4], gS[T, :, 6:9] = 2 * fin[:, 1], 2 * fin[:, 4], 2 * fin[:, 6:9]
    ref = ro.backward(ro.last_tape, gS.to(torch.float32).to(torch.float64), rot=True)
    torch.cuda.synchronize()
    assert (ro.last_backward["status"] == 0).all()
    assert psi.grad.dtype == torch.float64 and torch.equal(psi.grad, ref["plan_rot"][..., 2] + ref["list_rot0"][..., 2])
    assert float(psi.grad.abs().max()) > 0
    alpha = 0.02 / float(psi.grad.abs().max())
    psi2 = (psi.detach() - alpha * psi.grad)
    assert float((psi2 - psi.detach()).abs().max()) <= 0.02 * (1 + 1e-12)
    loss2 = loss_of(run(psi2))
    print(f"plan_yaw.grad (landing footstep) {psi.grad[:, 0, 1].tolist()}\nloss {float(loss.detach()):.9e} -> {float(loss2.detach()):.9e} "
          f"(yaw moved by at most 0.02 rad; removed {ro.last_backward['removed'].max(1).values.tolist()})")
    assert float(loss2.detach()) < float(loss.detach())
