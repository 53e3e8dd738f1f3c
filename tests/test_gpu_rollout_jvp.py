"""GPU: the roll-out tick forwards in k directions (include/cmpc.h: cmpc_plant_step_jvp_cols_device, cmpc_contacts_jvp_device,
cmpc_rollout_tick_jvp_device; WalkingRollout.forward_sensitivity, the jvp of rollout_differentiable) against its float64 restatement
tests/rollout_jvp_ref.py at the same float32 inputs, and against the device's own reverse mode on the same tape (the adjoint identity of a whole tick and
of a whole taped walk, over every input group at once).  Bounds: those of tests/test_gpu_rollout_adjoint.py, imported -- F64 for float64 glue on both
sides, REF for kernels against the restatement through a solve, ADJ for the adjoint identity on float32 device outputs (per problem, relative to the
larger side), 6 x ADJ for six chained ticks.  No other tolerance."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import rollout_jvp_ref as rjr
from tests import sens_rot_ref as srr
from tests.test_gpu_rollout_adjoint import ADJ, F64, REF, _host_tape, _list_case, _plant_inputs, _rel, _walk

pytestmark = pytest.mark.gpu

IN_GROUPS = ("state", "list", "list_rot", "plan", "plan_rot", "wrench", "model", "p")
OUT_GROUPS = ("state", "list", "list_rot", "x", "rot", "p")


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f32(a):
    """float64 values that float32 holds exactly"""
    return a.astype(np.float32).astype(np.float64)


def _gap(lhs, rhs):
    return abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)


def test_plant_columns_are_bit_equal_to_the_single_column_entry():
    """B = 16, N = 20, the inputs of the plant test, k = 3: every column of cmpc_plant_step_jvp_cols_device is bit-equal to plant_step_jvp_device on that
    column, with the rotation direction and without; a batch of 5 holding problems 11, 3, 7, 0, 15 is bit-identical."""
    _check_plant_columns(cm.config.ergocub_gazebo_v1(20, 0.06))


def _check_plant_columns(cfg):
    """the body of test_plant_columns_are_bit_equal_to_the_single_column_entry at cfg's horizon"""
    import torch
    L = cm.Layout(cfg.N)
    B, k, kw = 16, 3, dict(step=0.01, substeps=6)
    X, P, state, models = _plant_inputs(cfg, B, 4)
    rng = np.random.default_rng(9)
    dS, dM, dR = rng.normal(size=(B, k, 9)), rng.normal(size=(B, k, 34)), rng.normal(size=(B, k, 2, 3))
    dX, dP = rng.normal(size=(B, k, L.nx)).astype(np.float32), rng.normal(size=(B, k, L.np)).astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    s.set_models(models)
    base = (_cu(X), _cu(P), _cu(state))
    cols = s.plant_step_jvp_cols_device(*base, _cu(dS), _cu(dX), _cu(dP), _cu(dM), _cu(dR), **kw)
    cols0 = s.plant_step_jvp_cols_device(*base, _cu(dS), _cu(dX), _cu(dP), _cu(dM), **kw)
    bare = s.plant_step_jvp_cols_device(*base, _cu(dS), **kw)
    for j in range(k):
        one = s.plant_step_jvp_device(*base, _cu(dS[:, j]), _cu(dX[:, j]), _cu(dP[:, j]), _cu(dM[:, j]), dDirRot0=_cu(dR[:, j]), **kw)
        one0 = s.plant_step_jvp_device(*base, _cu(dS[:, j]), _cu(dX[:, j]), _cu(dP[:, j]), _cu(dM[:, j]), **kw)
        one_bare = s.plant_step_jvp_device(*base, _cu(dS[:, j]), **kw)
        torch.cuda.synchronize()
        assert torch.equal(cols[:, j], one) and torch.equal(cols0[:, j], one0) and torch.equal(bare[:, j], one_bare), j
        assert not torch.equal(one, one0) and bool(torch.isfinite(one).all())
    idx = [11, 3, 7, 0, 15]
    s5 = cm.BatchSolver(cfg, 5)
    s5.set_models(models[idx])
    cols5 = s5.plant_step_jvp_cols_device(_cu(X[idx]), _cu(P[idx]), _cu(state[idx]), _cu(dS[idx]), _cu(dX[idx]), _cu(dP[idx]), _cu(dM[idx]), _cu(dR[idx]), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(cols5.cpu().numpy(), cols.cpu().numpy()[idx])


@pytest.mark.parametrize("M,first_tick,now_k,snap", [(12, False, 9, False), (12, False, 22, False), (12, True, 0, False), (20, False, 14, False),
                                                     (12, False, 11, True)])
def test_list_jvp_kernel_equals_the_restatement_and_is_the_transpose_of_the_list_adjoints(M, first_tick, now_k, snap):
    """The five cases of the list adjoint tests (B = 24; problem 5's merge fails), k = 2, float32-exact random directions: every output equals
    rollout_jvp_ref.list_jvp to F64 (the kernel copies; the p rows are one rounding to float32 of an exact value); the two phases apart give the bits of both
    at once; the failed merge gives zeros and status 5; and <g, J d> = <J^T g, d> on the device against contacts_position_vjp_device (phase 3) plus
    contacts_orientation_vjp_device on the same tape, per problem and column, to F64."""
    _check_list_jvp(cm.config.ergocub_gazebo_v1(20, 0.06), M, first_tick, now_k, snap)


def _check_list_jvp(cfg, M, first_tick, now_k, snap):
    """the body of test_list_jvp_kernel_equals_the_restatement_and_is_the_transpose_of_the_list_adjoints at cfg's horizon and sampling time"""
    import torch
    L, N = cm.Layout(cfg.N), cfg.N
    B, k = 24, 2
    now = cfg.sampling_time * now_k
    s, dplan, dprev, lists, ok, land = _list_case(cfg, B, M, 17, now, first_tick, snap)
    rng = np.random.default_rng(3)
    d = {name: _f32(rng.normal(size=(B, k, 2, M, 3))) for name in ("prev", "prev_rot", "plan", "plan_rot")}
    dx = rng.normal(size=(B, k, L.nx)).astype(np.float32)
    tape = dict(plan=None if first_tick else (dplan[0], dplan[2]), prev=None if first_tick else (dprev[0], dprev[2]), ok=ok, force_sample_time=snap)
    dirs = dict(dDirPrevList=_cu(d["prev"]), dDirPrevListRot=_cu(d["prev_rot"]), dDirPlan=_cu(d["plan"]), dDirPlanRot=_cu(d["plan_rot"]))
    r = s.contacts_jvp_device(now, lists[0], lists[2], land, k, dDirX=_cu(dx), phase=3, **tape, **dirs)
    # the two phases apart
    r1 = s.contacts_jvp_device(now, lists[0], lists[2], land, k, phase=1, **tape, **dirs)
    r2 = s.contacts_jvp_device(now, lists[0], lists[2], land, k, dDirX=_cu(dx), phase=2, out=r1["list"].clone(), out_rot=r1["list_rot"].clone(), ok=ok,
                               force_sample_time=snap)
    # the adjoints on the same tape
    g_out, g_lrot, g_rot = _f32(rng.normal(size=(B, 2, M, 3))), _f32(rng.normal(size=(B, 2, M, 3))), _f32(rng.normal(size=(B, 2, N, 3)))
    g_p = rng.normal(size=(B, L.np)).astype(np.float32)
    gx = torch.zeros((B, L.nx), dtype=torch.float32, device="cuda")
    gplan, gplan_rot = (torch.zeros((B, 2, M, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    gprev, _ = s.contacts_position_vjp_device(now, lists[0], lists[2], land, dGradListOut=_cu(g_out), dGradP=_cu(g_p), dGradX=gx, dGradPlan=gplan, phase=3, **tape)
    gprev_rot, _ = s.contacts_orientation_vjp_device(now, lists[0], lists[2], land, dGradListRotOut=_cu(g_lrot), dGradRot=_cu(g_rot), dGradPlanRot=gplan_rot,
                                                     **tape)
    torch.cuda.synchronize()
    assert torch.equal(r["list"], r2["list"]) and torch.equal(r["list_rot"], r2["list_rot"]) and torch.equal(r["p"], r1["p"]) and torch.equal(r["rot"], r1["rot"])
    got = {name: r[name].cpu().numpy() for name in ("list", "list_rot", "p", "rot", "status")}
    gprev, gplan, gx, gprev_rot, gplan_rot = (a.cpu().numpy().astype(np.float64) for a in (gprev, gplan, gx, gprev_rot, gplan_rot))
    lt, ln, ld = lists[0].cpu().numpy(), lists[2].cpu().numpy(), land.cpu().numpy()
    okh = np.ones(B, int) if ok is None else ok.cpu().numpy()
    pt, pn, vt, vn = (a.cpu().numpy() for a in (dplan[0], dplan[2], dprev[0], dprev[2]))
    worst, worst_adj, landings = 0.0, 0.0, 0
    for b in range(B):
        hk = dict(plan=None if first_tick else (pt[b], pn[b]), prev=None if first_tick else (vt[b], vn[b]), ok=bool(okh[b]), force_sample_time=snap)
        for j in range(k):
            ref = rjr.list_jvp(L, cfg.sampling_time, now, lt[b], ln[b], ld[b], d_prev=d["prev"][b, j], d_prev_rot=d["prev_rot"][b, j], d_plan=d["plan"][b, j],
                               d_plan_rot=d["plan_rot"][b, j], d_x=dx[b, j], **hk)
            assert got["status"][b] == ref["status"]
            for name in ("list", "list_rot", "p", "rot"):
                want = ref[name].astype(np.float32) if name == "p" else ref[name]
                worst = max(worst, float(np.abs(got[name][b, j] - want).max() / max(np.abs(want).max(), 1.0)))
            landings += sum(1 for c in range(2) if ref["nx"][c] >= 0)
            lhs = ((g_out[b] * got["list"][b, j]).sum() + (g_lrot[b] * got["list_rot"][b, j]).sum() + g_p[b].astype(np.float64) @ got["p"][b, j] +
                   (g_rot[b] * got["rot"][b, j]).sum())
            rhs = ((gprev[b] * d["prev"][b, j]).sum() + (gplan[b] * d["plan"][b, j]).sum() + gx[b] @ dx[b, j].astype(np.float64) +
                   (gprev_rot[b] * d["prev_rot"][b, j]).sum() + (gplan_rot[b] * d["plan_rot"][b, j]).sum())
            if okh[b]:
                worst_adj = max(worst_adj, _gap(lhs, rhs))
            else:
                assert lhs == 0.0 and rhs == 0.0
    print(f"\nlist JVP kernel N={cfg.N} dt={cfg.sampling_time} M={M} first_tick={first_tick} now={now:.2f} snap={snap}: worst gap to the restatement {worst:.2e}, adjoint identity on the "
          f"device {worst_adj:.2e} (bound {F64:.0e} each), landing entries overwritten {landings}")
    assert worst <= F64 and worst_adj <= F64
    if not first_tick:
        assert got["status"][5] == 5 and okh[5] == 0 and not any(got[name][5].any() for name in ("list", "list_rot", "p", "rot"))
        assert (np.delete(got["status"], 5) == 0).all() and landings > 0


# ---------------------------------------------------------------------------------------------------------------- ticks
@pytest.fixture(scope="module")
def walk24():
    cfg, ro, rec = _walk(8, 24)
    assert all(rec["converged"]) and all(rec["merge_ok"])
    return cfg, ro, rec


def _tick_directions(rng, cfg, B, k, M):
    """k random columns of all eight input groups; float arrays the device takes as float32 are float32"""
    L, N = cm.Layout(cfg.N), cfg.N
    theta = cm.config.model_row(cfg)
    return dict(state=rng.normal(size=(B, k, 9)), list=rng.normal(size=(B, k, 2, M, 3)) * 0.1, list_rot=rng.normal(size=(B, k, 2, M, 3)) * 0.1,
                plan=rng.normal(size=(B, k, 2, M, 3)) * 0.1, plan_rot=rng.normal(size=(B, k, 2, M, 3)) * 0.1,
                wrench=rng.normal(size=(B, k, N, 6)).astype(np.float32), model=rng.normal(size=(B, k, 34)) * np.abs(theta).clip(1e-2) * 0.1,
                p=(rng.normal(size=(B, k, L.np)) * 0.1).astype(np.float32))


def _tick_jvp(s, tk, d, sel=slice(None), rows=slice(None), **kw):
    """rollout_tick_jvp_device on the columns `sel` of the directions d (problems `rows`)"""
    c = lambda a: _cu(a[rows][:, sel])
    k = d["state"][rows][:, sel].shape[1]
    return s.rollout_tick_jvp_device(tk["now"], tk, k, dDirState=c(d["state"]), dDirPrevList=c(d["list"]), dDirPrevListRot=c(d["list_rot"]),
                                     dDirPlan=c(d["plan"]), dDirPlanRot=c(d["plan_rot"]), dDirWrench=c(d["wrench"]), dDirModel=c(d["model"]), dDirP=c(d["p"]),
                                     x=True, rot=True, p_full=True, **kw)


def test_tick_jvp_matches_the_restatement_on_taped_walking_ticks(walk24):
    """cmpc_rollout_tick_jvp_device on ticks 2 (before lift-off), 8 (swing), 14 (landing) and 18 (after) of the 24-tick walk, B = 8, k = 3, every input
    group random, against rollout_jvp_ref.tick_jvp fed with the tape's own float32 (x, p, lam_g) on problems 0 and 5: every output group <= REF, relative
    to its largest entry.  dTickSens[:, 0] == 0 for all eight problems.  The bare cmpc_solution_jvp_rot_device fed with the assembled dDirPFull and
    dDirRot is printed alongside (its dx is the tick's, bit for bit: the tick calls it)."""
    import torch
    cfg, ro, rec = walk24
    B, k = 8, 3
    ticks = rec["tape"]["ticks"]
    M = ticks[0]["list_t"].shape[2]
    rng = np.random.default_rng(21)
    worst = {g: 0.0 for g in OUT_GROUPS}
    worst_bare = 0.0
    s = ro.solver
    for i in (2, 8, 14, 18):
        tk = ticks[i]
        d = _tick_directions(rng, cfg, B, k, M)
        r = _tick_jvp(s, tk, d)
        bare, bare_sens = s.solution_jvp_rot_device(tk["X"], tk["P"], tk["lam_g"], dDirP=r["p"], dDirModel=_cu(d["model"]), dDirRot=r["rot"])
        torch.cuda.synchronize()
        assert (r["sens"][:, 0] == 0).all(), r["sens"][:, 0]
        assert torch.equal(bare, r["x"]) and torch.equal(bare_sens[:, 1:], r["sens"][:, 1:])
        got = {g: r[g].cpu().numpy() for g in OUT_GROUPS}
        bare = bare.cpu().numpy()
        for b in (0, 5):
            tp = _host_tape(tk, b)
            RS = srr.RotSens(cfg, tp["X"], tp["P"], tp["lam_g"])
            for j in range(k):
                ref = rjr.tick_jvp(cfg, tp, tk["now"], d["state"][b, j], d["list"][b, j], d["list_rot"][b, j], d["plan"][b, j], d["plan_rot"][b, j],
                                   d["wrench"][b, j], d["model"][b, j], d["p"][b, j], RS=RS)
                assert ref["status"] == 0
                gaps = {g: _rel(got[g][b, j], ref[g]) for g in OUT_GROUPS}
                bgap = _rel(bare[b, j], ref["x"])
                print(f"tick {i} problem {b} column {j} land {tk['land'][b].tolist()} removed {float(r['sens'][b, 6]):.1e}: tick " +
                      " ".join(f"{g} {v:.1e}" for g, v in gaps.items()) + f"  bare solution JVP x {bgap:.1e}")
                worst_bare = max(worst_bare, bgap)
                for g in OUT_GROUPS:
                    worst[g] = max(worst[g], gaps[g])
    print("tick JVP against the restatement, worst: " + " ".join(f"{g} {v:.2e}" for g, v in worst.items()) + f" (bound {REF:.0e});  bare solution JVP: "
          f"x {worst_bare:.2e}")
    assert max(worst.values()) <= REF, worst


def test_tick_jvp_and_tick_vjp_are_adjoint_on_the_device(walk24):
    """<g, J d> = <J^T g, d> of a whole tick on the device: rollout_tick_jvp_device (k = 3) against rollout_tick_vjp_device(rot=True, grad_p=True,
    dGradX=...) on ticks 2, 8, 14, 18 of the walk, all eight input groups and all four cotangent groups (state', list, list orientations, x) random at once:
    <= ADJ relative to the larger side, per problem and column."""
    import torch
    cfg, ro, rec = walk24
    B, k = 8, 3
    L = cm.Layout(cfg.N)
    ticks = rec["tape"]["ticks"]
    M = ticks[0]["list_t"].shape[2]
    rng = np.random.default_rng(33)
    s = ro.solver
    worst = 0.0
    for i in (2, 8, 14, 18):
        tk = ticks[i]
        d = _tick_directions(rng, cfg, B, k, M)
        g = dict(state=rng.normal(size=(B, 9)), list=rng.normal(size=(B, 2, M, 3)) * 0.1, list_rot=rng.normal(size=(B, 2, M, 3)) * 0.1,
                 x=(rng.normal(size=(B, L.nx)) * 0.01).astype(np.float32))
        f = _tick_jvp(s, tk, d)
        acc = {name: torch.zeros(shape, dtype=torch.float64, device="cuda") for name, shape in (("plan", (B, 2, M, 3)), ("model", (B, 34)), ("plan_rot", (B, 2, M, 3)))}
        v = s.rollout_tick_vjp_device(tk["now"], tk, _cu(g["state"]), _cu(g["list"]), _cu(g["x"]), dGradPlan=acc["plan"], dGradModel=acc["model"], grad_p=True,
                                      dGradListRotOut=_cu(g["list_rot"]), rot=True, dGradPlanRot=acc["plan_rot"])
        torch.cuda.synchronize()
        assert (f["sens"][:, 0] == 0).all() and (v["sens"][:, 0] == 0).all()
        f = {name: f[name].cpu().numpy().astype(np.float64) for name in ("state", "list", "list_rot", "x")}
        v = {name: a.cpu().numpy().astype(np.float64) for name, a in dict(state=v["state"], list=v["prev_list"], list_rot=v["prev_list_rot"], plan=acc["plan"],
                                                                          plan_rot=acc["plan_rot"], wrench=v["wrench"], model=acc["model"], p=v["p"]).items()}
        for b in range(B):
            for j in range(k):
                lhs = sum((g[name][b].astype(np.float64) * f[name][b, j]).sum() for name in ("state", "list", "list_rot", "x"))
                terms = {name: float((v[name][b] * d[name][b, j].astype(np.float64)).sum()) for name in IN_GROUPS}
                rhs = sum(terms.values())
                gap = _gap(lhs, rhs)
                worst = max(worst, gap)
                if j == 0 and b in (0, 5):
                    print(f"tick {i} problem {b}: <g, J d> = {lhs:.9e}  <J^T g, d> = {rhs:.9e}  gap {gap:.2e}  terms " + " ".join(f"{n} {t:.1e}" for n, t in terms.items()))
    print(f"tick JVP against tick VJP on the device, worst gap over 4 ticks x 8 problems x 3 columns: {worst:.2e} (bound {ADJ:.0e})")
    assert worst <= ADJ


def test_tick_jvp_does_not_depend_on_k_or_the_batch_and_gives_the_closed_loop_transition(walk24):
    """Tick 8 (a merge tick) of the walk.  Columns computed at k = 1, at k = 3 and at k = 9 (which crosses a chunk of eight, and grows the workspace)
    are bit-equal; a permuted batch of 5 on its own handle is bit-equal; with nine unit state columns and every other direction NULL, dDirStateOut equals
    closed_loop_transition_device's A_cl bit for bit (no problem is flagged)."""
    import torch
    cfg, ro, rec = walk24
    B = 8
    tk = rec["tape"]["ticks"][8]
    assert tk["prev_t"] is not None
    M = tk["list_t"].shape[2]
    s = ro.solver
    d = _tick_directions(np.random.default_rng(8), cfg, B, 9, M)
    names = OUT_GROUPS + ("sens",)
    r3 = _tick_jvp(s, tk, d, slice(0, 3))
    r9 = _tick_jvp(s, tk, d)
    r1 = _tick_jvp(s, tk, d, slice(0, 1))
    r3b = _tick_jvp(s, tk, d, slice(0, 3))
    torch.cuda.synchronize()
    assert (r9["sens"][:, 0] == 0).all()
    for g in OUT_GROUPS:
        assert torch.equal(r9[g][:, :3], r3[g]) and torch.equal(r3[g][:, :1], r1[g]) and torch.equal(r3[g], r3b[g]), g
        assert bool(r9[g].any())
    # a permuted batch of 5 on a handle of its own
    idx = [6, 3, 7, 0, 5]
    s5 = cm.BatchSolver(cfg, 5)
    tk5 = {key: (v[idx].contiguous() if isinstance(v, torch.Tensor) else v) for key, v in tk.items()}
    r5 = _tick_jvp(s5, tk5, d, slice(0, 3), idx)
    torch.cuda.synchronize()
    for g in names:
        assert torch.equal(r5[g], r3[g][idx]), g
    # nine unit state columns alone: the closed-loop transition
    eye = torch.eye(9, dtype=torch.float64, device="cuda").expand(B, 9, 9).contiguous()
    rs = s.rollout_tick_jvp_device(tk["now"], tk, 9, dDirState=eye)
    A, sens = s.closed_loop_transition_device(tk["X"], tk["P"], tk["lam_g"], tk["state"], step=tk["step"], substeps=tk["substeps"])
    torch.cuda.synchronize()
    assert (rs["sens"][:, 0] == 0).all() and (sens[:, 0] == 0).all()
    assert torch.equal(rs["state"].transpose(1, 2), A)
    assert not rs["list_rot"].any()


def test_tick_jvp_flags_zero_outputs_and_leave_neighbours_alone():
    """The four-flag batch of test_tick_vjp_flags_zero_outputs_and_leave_neighbours_alone (1 not converged -> 4; 3 a NaN state -> 2; 4 a broken model row
    -> 3; 6 a failed merge -> 5), k = 2: the status words are those of the tick VJP on the same tape, the flagged problems have zeros in every output of
    every column, and the neighbours are bit-identical to the same batch with clean rows in those places."""
    import torch
    B, k = 8, 2
    cfg, ro, rec = _walk(B, 4)
    _, ro_bad, rec_bad = _walk(B, 4, warm_budget=3, retry=None)
    found = [(i, int(j)) for i in (1, 2, 3) for j in (rec_bad["tape"]["ticks"][i]["info"][:, 5] == 1).nonzero().flatten().tolist()]
    assert found, "the budget of 3 iterations left no problem unconverged"
    i, j = found[0]
    tk, tb = dict(rec["tape"]["ticks"][i]), rec_bad["tape"]["ticks"][i]
    assert float(tb["info"][j, 5]) == 1.0 and (rec["tape"]["ticks"][i]["info"][:, 5] == 0).all()
    M = tk["list_t"].shape[2]
    clean = {key: (v.clone() if isinstance(v, torch.Tensor) else v) for key, v in tk.items()}
    for key in ("X", "P", "lam_g", "state", "info", "land", "list_t", "list_n", "prev_t", "prev_n"):
        tk[key] = tk[key].clone()
        tk[key][1] = tb[key][j]
    tk["state"][3] = float("nan")
    tk["ok"] = tk["ok"].clone()
    tk["ok"][6] = 0
    theta = np.tile(cm.config.model_row(cfg), (B, 1))
    bad_theta = theta.copy()
    bad_theta[4, 0] = -1.0
    d = _tick_directions(np.random.default_rng(2), cfg, B, k, M)
    g_state = _cu(np.random.default_rng(3).normal(size=(B, 9)))
    res = []
    for tape, th in ((tk, bad_theta), (clean, theta)):
        ok_models = ro.solver.set_models_device(_cu(th))
        r = _tick_jvp(ro.solver, tape, d)
        v = ro.solver.rollout_tick_vjp_device(tape["now"], tape, g_state, rot=True)
        torch.cuda.synchronize()
        res.append({key: a.cpu().numpy() for key, a in dict(r, ok_models=ok_models, vjp_status=v["sens"][:, 0]).items()})
    a, c = res
    assert a["ok_models"][4] == 0 and c["ok_models"].all()
    flagged = {1: 4, 3: 2, 4: 3, 6: 5}
    assert (c["sens"][:, 0] == 0).all(), c["sens"][:, 0]
    assert np.array_equal(a["sens"][:, 0], a["vjp_status"]) and np.array_equal(c["sens"][:, 0], c["vjp_status"])
    for b in range(B):
        if b in flagged:
            assert a["sens"][b, 0] == flagged[b], (b, a["sens"][b])
            for g in OUT_GROUPS:
                assert not a[g][b].any(), (b, g)     # (any() is true for a NaN: zeros, not merely nothing finite)
        else:
            assert a["sens"][b, 0] == 0
            for g in OUT_GROUPS + ("sens",):
                assert np.array_equal(a[g][b], c[g][b]), (b, g)
            assert a["state"][b].any() and a["x"][b].any() and a["rot"][b].any()


def test_forward_sensitivity_is_the_transpose_of_backward_and_the_jvp_of_rollout_differentiable():
    """Six ticks of the walk (B = 8), forward_sensitivity at k = 2 with every direction group random against backward(rot=True) with random cotangents on
    every state and every solution: sum_i <gS_i, dS_i> + <gX_i, dX_i> equals the contraction of state0, list0, list_rot0, push, models, plan and plan_rot
    with their directions, <= 6 x ADJ per problem and column (six chained ticks).  torch.autograd.forward_ad through rollout_differentiable(..., models=,
    plan_yaw=) at k = 1: the tangent equals forward_sensitivity's column for the same directions bit for bit."""
    import torch
    import torch.autograd.forward_ad as fwAD
    B, T, k = 8, 6, 2
    cfg, ro, rec = _walk(B, T)
    assert all(rec["converged"]) and all(rec["merge_ok"])
    tape = rec["tape"]
    L = cm.Layout(cfg.N)
    M = tape["ticks"][0]["list_t"].shape[2]
    rng = np.random.default_rng(14)
    d = _tick_directions(rng, cfg, B, k, M)
    d_push = rng.normal(size=(B, k, 3)).astype(np.float32)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (rng.normal(size=(T, B, L.nx)) * 0.01).astype(np.float32)
    f = ro.forward_sensitivity(tape, dir_state0=d["state"], dir_list0=d["list"], dir_list_rot0=d["list_rot"], dir_plan=d["plan"], dir_plan_rot=d["plan_rot"],
                               dir_push=d_push, dir_models=d["model"], solutions=True)
    v = ro.backward(tape, gS, gX, rot=True)
    torch.cuda.synchronize()
    assert (f["status"] == 0).all() and (v["status"] == 0).all()
    assert tuple(f["states"].shape) == (T + 1, B, k, 9) and tuple(f["X"].shape) == (T, B, k, L.nx) and tuple(f["list"].shape) == (B, k, 2, M, 3)
    fs, fx = f["states"].cpu().numpy(), f["X"].cpu().numpy().astype(np.float64)
    assert np.array_equal(fs[0], d["state"]) and f["list"].any() and f["list_rot"].any()
    pairs = (("state0", d["state"]), ("list0", d["list"]), ("list_rot0", d["list_rot"]), ("push", d_push.astype(np.float64)), ("models", d["model"]),
             ("plan", d["plan"]), ("plan_rot", d["plan_rot"]))
    vh = {name: v[name].cpu().numpy() for name, _ in pairs}
    worst = 0.0
    for b in range(B):
        for j in range(k):
            lhs = (gS[:, b] * fs[:, b, j]).sum() + (gX[:, b].astype(np.float64) * fx[:, b, j]).sum()
            terms = {name: float((vh[name][b] * dd[b, j]).sum()) for name, dd in pairs}
            rhs = sum(terms.values())
            gap = _gap(lhs, rhs)
            worst = max(worst, gap)
            if j == 0 and b in (0, 5):
                print(f"\nproblem {b}: forward {lhs:.9e}  reverse {rhs:.9e}  gap {gap:.2e}  terms " + " ".join(f"{n} {t:.1e}" for n, t in terms.items()))
    print(f"forward sweep against reverse sweep over {T} ticks, worst gap over 8 problems x 2 columns: {worst:.2e} (bound {6 * ADJ:.1e})")
    assert worst <= 6 * ADJ
    # forward-mode autograd at k = 1
    theta = torch.from_numpy(np.tile(cm.config.model_row(cfg), (B, 1))).cuda()
    t_theta = _cu(d["model"][:, 0])
    psi, t_psi = torch.zeros((B, 2, M), dtype=torch.float64, device="cuda"), _cu(rng.normal(size=(B, 2, M)) * 0.1)
    c0 = rec["tape"]["ticks"][0]["state"]
    state0 = c0.clone()
    push = torch.zeros((B, 3), dtype=torch.float32, device="cuda")
    with fwAD.dual_level():
        states = cm.rollout_differentiable(ro, T, state0, push=push, models=fwAD.make_dual(theta, t_theta), push_ticks=3, plan_yaw=fwAD.make_dual(psi, t_psi))
        primal, tangent = fwAD.unpack_dual(states)
        assert tangent is not None and tangent.dtype == torch.float32 and tuple(tangent.shape) == (T + 1, B, 9)
        tangent = tangent.clone()
    yaw = torch.zeros((B, 1, 2, M, 3), dtype=torch.float64, device="cuda")
    yaw[:, 0, :, :, 2] = t_psi
    col = ro.forward_sensitivity(ro.last_tape, dir_models=t_theta[:, None].contiguous(), dir_plan_rot=yaw, dir_list_rot0=yaw)
    torch.cuda.synchronize()
    assert (col["status"] == 0).all()
    assert torch.equal(tangent, col["states"][:, :, 0].to(torch.float32)) and bool(tangent[1:].any()) and not bool(tangent[0].any())
