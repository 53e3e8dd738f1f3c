"""Per-problem models on the MI355X (include/cmpc.h, cmpc_set_models / cmpc_set_models_device): one batch mixing robots, frictions and foot
sizes solves every problem exactly as a handle created with that problem's model would, and holds it to the float64 oracle."""
import dataclasses
import os

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity

pytestmark = pytest.mark.gpu

ROBOTS = ["ergoCubGazeboV1", "ergoCubGazeboV1_1", "ergoCubSN000", "ergoCubSN001", "iCubGazeboV3"]
NO_CYCLES = [0, 1, 2, 3, 4, 5, 7]   # info columns without solve_cycles (a clock reading)


def _base():
    return cm.config.ergocub_gazebo_v1(20, 0.06)


def _robot_model_cfg(robot, golden_dir):
    """the base configuration (N = 20, dt = 0.06, its solver options and bounding boxes) with robot's model: friction, weights, corners"""
    r = cm.config.from_ini(open(os.path.join(golden_dir, "ini", f"{robot}.ini")).read())
    b = _base()
    contacts = [dataclasses.replace(cb, corners=list(cr.corners)) for cb, cr in zip(b.contacts, r.contacts)]
    return dataclasses.replace(b, static_friction_coefficient=r.static_friction_coefficient, com_weight=r.com_weight,
                               contact_position_weight=r.contact_position_weight, force_rate_of_change_weight=r.force_rate_of_change_weight,
                               angular_momentum_weight=r.angular_momentum_weight, contact_force_symmetry_weight=r.contact_force_symmetry_weight,
                               contacts=contacts)


def _solve(s, dP, dX0, warm=False):
    import torch
    dX, dI = s.solve_device(dP, dX0, warm=warm)
    torch.cuda.synchronize()
    return dX, dI


def _cold_and_warm(s, dP, dX0):
    """(X, info) of a cold solve and of a warm solve from its shifted solution"""
    import torch
    X1, I1 = _solve(s, dP, dX0)
    dX0w = torch.empty_like(dX0)
    s.shift_solution_device(X1, dX0w)
    X2, I2 = _solve(s, dP, dX0w, warm=True)
    return [(X1.cpu().numpy(), I1.cpu().numpy()), (X2.cpu().numpy(), I2.cpu().numpy())]


def _same(a, b, rows=None):
    (Xa, Ia), (Xb, Ib) = a, b
    if rows is not None:
        Xa, Ia, Xb, Ib = Xa[rows], Ia[rows], Xb[rows], Ib[rows]
    return np.array_equal(Xa.view(np.int32), Xb.view(np.int32)) and np.array_equal(Ia[:, NO_CYCLES].view(np.int32), Ib[:, NO_CYCLES].view(np.int32))


@pytest.mark.parametrize("B,factors", [(200, "lds"), (1280, "hbm")])
def test_mixed_robots_are_bit_identical_to_homogeneous_handles(B, factors, golden_dir):
    import torch
    cfgs = [_robot_model_cfg(r, golden_dir) for r in ROBOTS]
    _, P, X0 = cm.synthetic.walking_push(_base(), B, 150.0, 3, 7)
    dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
    table = cm.config.model_array([cfgs[b % 5] for b in range(B)])
    mixed = cm.BatchSolver(_base(), B, factors=factors)
    mixed.set_models(table)                                       # host form
    host = _cold_and_warm(mixed, dP, dX0)
    ok = mixed.set_models_device(torch.from_numpy(table).cuda())  # device form
    dev = _cold_and_warm(mixed, dP, dX0)
    assert (ok.cpu().numpy() == 1).all()
    mixed.close()
    for r, cfg in enumerate(cfgs):
        s = cm.BatchSolver(cfg, B, factors=factors)
        ref = _cold_and_warm(s, dP, dX0)
        s.close()
        rows = np.arange(r, B, 5)
        for k in range(2):
            assert _same(host[k], ref[k], rows), (ROBOTS[r], "host", "cold" if k == 0 else "warm")
            assert _same(dev[k], ref[k], rows), (ROBOTS[r], "device", "cold" if k == 0 else "warm")
    # the robots' models do differ: the same problems come out differently
    assert not np.array_equal(host[0][0][0], host[0][0][1])


def _randomised(B, seed):
    base = _base()
    rng = np.random.default_rng(seed)
    cfgs = []
    for b in range(B):
        s = rng.uniform(0.8, 1.2)
        contacts = [dataclasses.replace(c, corners=[tuple(s * v for v in cn) for cn in c.corners]) for c in base.contacts]
        cfgs.append(dataclasses.replace(base, static_friction_coefficient=float(rng.uniform(0.25, 1.0)), contacts=contacts))
    return cfgs


def _active_friction_rows(N, cfg, p, x, rel=1e-6):
    """friction rows of loaded corners (f_z above 1 % of g / 8) within rel x f_z of their face in the float64 optimum"""
    L = cm.Layout(N)
    n = 0
    for c in range(2):
        for k in range(N):
            if p[L.p_gam[c] + k] < 0.5:
                continue
            R = p[L.p_R[c] + 9 * k:L.p_R[c] + 9 * k + 9].reshape(3, 3, order="F")
            for j in range(4):
                f = R.T @ x[L.f[c][j] + 3 * k:L.f[c][j] + 3 * k + 3]
                if f[2] > 0.01 * 9.80665 / 8:
                    n += int(cfg.static_friction_coefficient * f[2] - max(abs(f[0]), abs(f[1])) < rel * f[2])
    return n


def test_randomised_friction_and_feet_match_the_oracle():
    import torch
    from oracle import oracle_lib as ol, problem_nlp
    B = 256
    cfgs = _randomised(B, 21)
    _, P, X0 = cm.synthetic.walking_push(_base(), B, 100.0, 3, 11)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(_base(), B)
    s.set_models(cfgs)
    dX, dI = _solve(s, torch.from_numpy(P32).cuda(), torch.from_numpy(X032).cuda())
    X, info = dX.cpu().numpy(), dI.cpu().numpy()
    parity.assert_no_sync_giveups(info)
    Xr = np.empty_like(X, dtype=np.float64)
    active, oracle_ok = 0, np.zeros(B, bool)
    for b in range(B):
        xr, ir = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfgs[b]), P32[b:b + 1].astype(np.float64), X032[b:b + 1].astype(np.float64),
                                    ol.ipm_opts(tol=1e-9, mu_min=1e-10))
        oracle_ok[b] = ir[0, 5] == 0
        Xr[b] = xr[0]
        active += oracle_ok[b] and _active_friction_rows(cfgs[b].N, cfgs[b], P32[b].astype(np.float64), xr[0]) > 0
    # (a randomised draw may hold a problem the float64 oracle itself does not solve: a handful at most, and the GPU must solve every other one)
    assert (~oracle_ok).sum() <= 3, np.nonzero(~oracle_ok)
    ok = np.nonzero(oracle_ok)[0]
    assert (info[ok, 5] == 0).all(), ok[info[ok, 5] != 0]
    worst = parity.worst_errors(20, P32[ok], X[ok], Xr[ok])
    print(f"\nrandomised models B={B}: problems with an active friction row {active}; " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    parity.assert_within(20, worst)
    assert active >= 3, active


def test_nlp_callbacks_follow_each_problems_model(golden_dir):
    import ctypes as C

    import torch
    from oracle import oracle_lib as ol, problem_nlp
    cfgs = [_robot_model_cfg(r, golden_dir) for r in ROBOTS] + _randomised(5, 4)
    B = len(cfgs)
    _, P, X0 = cm.synthetic.walking_push(_base(), B, 150.0, 3, 5)
    rng = np.random.default_rng(9)
    X = (X0 + 0.05 * rng.normal(size=X0.shape)).astype(np.float32)
    P32 = P.astype(np.float32)
    L = cm.Layout(20)
    LamG = rng.normal(size=(B, L.ng)).astype(np.float32)
    s = cm.BatchSolver(_base(), B)
    s.set_models(cfgs)
    nnzj, nnzh = 243 * 20 + 15, 348 * 20 - 36
    dX, dP, dL = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X, P32, LamG))
    F = torch.empty(B, device="cuda"); G = torch.empty(B, L.ng, device="cuda"); GF = torch.empty(B, L.nx, device="cuda")
    J = torch.empty(B, nnzj, device="cuda"); H = torch.empty(B, nnzh, device="cuda")
    GX = torch.empty(B, L.nx, device="cuda"); GP = torch.empty(B, L.np, device="cuda")
    lib, st = cm._capi.lib(), torch.cuda.current_stream().cuda_stream
    assert lib.cmpc_eval_nlp_device(s._h, dX.data_ptr(), dP.data_ptr(), dL.data_ptr(), C.c_float(0.7), F.data_ptr(), G.data_ptr(), GF.data_ptr(),
                                    J.data_ptr(), H.data_ptr(), st) == 0, s.last_error
    assert lib.cmpc_eval_nlp_grad_device(s._h, dX.data_ptr(), dP.data_ptr(), dL.data_ptr(), C.c_float(0.7), GX.data_ptr(), GP.data_ptr(), st) == 0
    torch.cuda.synchronize()
    F, G, GF, J, H, GX, GP = (t.cpu().numpy().astype(np.float64) for t in (F, G, GF, J, H, GX, GP))
    jr = np.empty(nnzj, np.int32); jc = np.empty(nnzj, np.int32); hr = np.empty(nnzh, np.int32); hc = np.empty(nnzh, np.int32)
    lib.cmpc_nlp_sparsity(20, jr.ctypes.data, jc.ctypes.data, hr.ctypes.data, hc.ctypes.data)

    def close(a, b, rel=1e-5):
        assert np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-30), (np.abs(a - b).max(), np.abs(b).max())

    for b in range(B):
        oc = problem_nlp.oracle_cfg(cfgs[b])
        x, p = X[b].astype(np.float64), P32[b].astype(np.float64)
        f, g = ol.nlp_fg(oc, x, p)
        close(F[b], f); close(G[b], g); close(GF[b], ol.nlp_grad_f(oc, x, p))
        r, c, v = ol.nlp_jac(oc, x, p)
        Jd = np.zeros((L.ng, L.nx)); np.add.at(Jd, (r, c), v)
        close(J[b], Jd[jr, jc])
        r, c, v = ol.nlp_hess(oc, x, p, 0.7, LamG[b].astype(np.float64))
        Hd = np.zeros((L.nx, L.nx)); np.add.at(Hd, (r, c), v)
        close(H[b], Hd[hr, hc])
        gx, gp = ol.nlp_grad(oc, x, p, 0.7, LamG[b].astype(np.float64))
        close(GX[b], gx); close(GP[b], gp)
    # ... and a uniform model would not have passed: the robots' objectives differ
    assert len(np.unique(F[:5])) == 5


def test_plant_step_and_native_tick_follow_each_problems_corners():
    import torch
    from oracle import plant_ref
    B = 32
    cfgs = _randomised(B, 13)
    _, P, X0 = cm.synthetic.walking_push(_base(), B, 50.0, 3, 3)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    L = cm.Layout(20)
    s = cm.BatchSolver(_base(), B)
    s.set_models(cfgs)
    dP = torch.from_numpy(P32).cuda()
    dX, _ = _solve(s, dP, torch.from_numpy(X032).cuda())
    state = dP[:, L.p_com0:L.p_com0 + 9].contiguous()
    new_state, zmp = s.plant_step_device(dX, dP, state, step=0.01, substeps=6)
    torch.cuda.synchronize()
    X = dX.cpu().numpy().astype(np.float64)
    for b in range(B):
        corners = np.asarray([c.corners for c in cfgs[b].contacts], np.float64)
        ref_state, ref_zmp = plant_ref.plant_step(L, corners, X[b], P32[b].astype(np.float64), P32[b, L.p_com0:L.p_com0 + 9], 0.01, 6)
        np.testing.assert_allclose(new_state[b].cpu().numpy(), ref_state, rtol=0, atol=2e-6)
        np.testing.assert_allclose(zmp[b].cpu().numpy(), ref_zmp, rtol=0, atol=2e-6)
    # the one-call tick with models set is the step-by-step path to the last bit
    cfg = _base()
    rng = np.random.default_rng(11)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0, h0 = rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    models = cm.config.model_array(cfgs)
    recs = []
    for native, mdl in ((True, models), (False, torch.from_numpy(models).cuda()), (True, None)):
        ro = cm.rollout.WalkingRollout(cfg, B, native_tick=native, models=mdl)
        recs.append(ro.run(6, com0, dcom0, h0, push=push, push_ticks=3))
    a, b, u = recs
    assert all(a["converged"]) and all(a["merge_ok"])
    for key in ("com", "zmp", "land", "landing_offset"):
        assert np.array_equal(np.stack(a[key]), np.stack(b[key])), key
    assert a["iterations_max"] == b["iterations_max"] and a["iterations_mean"] == b["iterations_mean"]
    assert not np.array_equal(np.stack(a["zmp"]), np.stack(u["zmp"]))    # the models reached the roll-out


def test_launch_retry_solves_stragglers_with_their_own_models():
    """retry="launch" with models: the stragglers are gathered with their model rows into the retry handle and solved there (the roll-out
    keeps the table as a device tensor for that)."""
    import torch
    cfg = _base()
    B = 32
    cfgs = _randomised(B, 17)
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    ro = cm.rollout.WalkingRollout(cfg, B, warm_budget=3, retry="launch", retry_batch=16, models=cfgs)
    rec = ro.run(4, com0, z, z, record="light")
    assert sum(rec["retried"]) > 0 and all(rec["converged"])
    assert ro.models.shape == (B, 34) and ro.models.dtype == torch.float64


def test_invalid_device_rows_give_status_3_and_leave_the_rest_alone():
    import torch
    B = 64
    cfgs = _randomised(B, 2)
    table = cm.config.model_array(cfgs)
    _, P, X0 = cm.synthetic.walking_push(_base(), B, 50.0, 3, 1)
    dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
    s = cm.BatchSolver(_base(), B)
    ok = s.set_models_device(torch.from_numpy(table).cuda())
    good = _cold_and_warm(s, dP, dX0)
    assert (ok.cpu().numpy() == 1).all()
    bad = table.copy()
    bad[5, 0] = 0.0               # friction not positive
    bad[17, 10 + 12 + 4] = np.nan  # a corner of the second foot
    with pytest.raises(ValueError, match="model 5: friction_coefficient"):
        s.set_models(bad)
    ok = s.set_models_device(torch.from_numpy(bad).cuda())
    X, I = _solve(s, dP, dX0)
    X, I = X.cpu().numpy(), I.cpu().numpy()
    okh = ok.cpu().numpy()
    assert okh[5] == 0 and okh[17] == 0 and okh.sum() == B - 2
    assert I[5, 5] == 3 and I[17, 5] == 3
    assert (I[[5, 17], 0] <= 1).all() and np.isfinite(X[[5, 17]]).all()   # not iterated: the initial iterate, as for the subset flag
    rest = np.setdiff1d(np.arange(B), [5, 17])
    assert _same((X, I), good[0], rest)


def test_clearing_the_table_restores_the_handles_own_bits():
    import torch
    B = 48
    _, P, X0 = cm.synthetic.walking_push(_base(), B, 50.0, 3, 4)
    dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
    fresh = cm.BatchSolver(_base(), B)
    ref = _cold_and_warm(fresh, dP, dX0)
    fresh.close()
    s = cm.BatchSolver(_base(), B)
    s.set_models(_randomised(B, 6))
    moved = _cold_and_warm(s, dP, dX0)
    assert not _same(moved[0], ref[0])
    s.set_models(None)
    for k, r in enumerate(_cold_and_warm(s, dP, dX0)):
        assert _same(r, ref[k]), k
    # a table of the handle's own model, either form, is the handle's own record to the bit
    s.set_models([_base()] * B)
    for k, r in enumerate(_cold_and_warm(s, dP, dX0)):
        assert _same(r, ref[k]), k
    s.set_models_device(torch.from_numpy(cm.config.model_array([_base()] * B)).cuda())
    for k, r in enumerate(_cold_and_warm(s, dP, dX0)):
        assert _same(r, ref[k]), k
