"""GPU: derivatives with respect to the stage rotations (include/cmpc.h, "rotation directions": cmpc_solution_jvp_rot_device,
cmpc_solution_vjp_rot_device, cmpc_rotation_value_gradient_device, cmpc_contacts_rotation_vjp_device, solve_differentiable(rot=...)), held to the
float64 dense restatement tests/sens_rot_ref.py at the GPU's own (x, lam_g), to the adjoint identity, to central differences of the float64 oracle's
optimal cost, and to bit-for-bit agreement with the model entry points and independence of batch position, batch size, k and sub-batches.

Limits: REF, ADJ, RESID of tests/test_gpu_sensitivity.py and VG of tests/test_gpu_model_sensitivity.py.  No rotation group needs more than REF.
Measured on MI355X with this file (profiles/rotation_sensitivity.txt), largest over the five cases: JVP 8.2e-8 (cfg3_n16) and VJP 4.6e-8 against
REF = 5e-5 -- rotation-only group columns of both feet, the random per-stage omega and the combined p + theta + omega column alike; adjoint identity
4.2e-5 (cfg2 lds; 9.3e-7 hbm, <= 4.3e-7 on the walking cases) against ADJ = 6e-4; residual 4.9e-9 against RESID = 1e-6; dSens[6] against the
restatement's removed size 6.4e-11 relative (cfg2, where it reaches 0.20 on a problem of the batch; 0 on the walking cases) against 1e-2;
dV*/domega 1.1e-10 against the restatement (limit 1e-6) and 5.4e-7 against the oracle's cost differences (VG = 1e-4)."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import sens_ref
from tests import sens_rot_ref as srr
from tests.test_gpu_model_sensitivity import VG, _theta32
from tests.test_gpu_sensitivity import ADJ, REF, RESID, _case, _solve

pytestmark = pytest.mark.gpu

K = 10   # columns: 8 group directions, one random per-stage omega, one combined p + theta + omega (two chunks of 8)


def _rot_case(name):
    if name == "yaw":
        return cm.synthetic.yawed_steps_n12("tmp", B=16)
    cfg, P, X0 = _case(name)
    return cfg, P[:16], X0[:16]


def _rot_dirs(cfg, P32, rng):
    """(omega [B, K, 2, N, 3], dtheta [B, K, 34], dp [B, K, n_p]): per problem the group directions of sens_rot_ref.rot_directions (both feet, e_z and a
    general axis; repeated in order where a problem has fewer than 8), a random per-stage omega, and a combined column"""
    B, N, L = P32.shape[0], cfg.N, cm.Layout(cfg.N)
    om = np.zeros((B, K, 2, N, 3))
    for b in range(B):
        ds = [d for _, d, _ in srr.rot_directions(N, P32[b])]
        for j in range(8):
            om[b, j] = ds[j % len(ds)]
    om[:, 8:] = rng.standard_normal((B, 2, 2, N, 3)) * 1e-2
    dth = np.zeros((B, K, 34))
    dth[:, 9] = rng.standard_normal((B, 34)) * 1e-2
    dp = np.zeros((B, K, L.np), np.float32)
    dp[:, 9] = (rng.standard_normal((B, L.np)) * 1e-2 * sens_ref.covered_mask(N)).astype(np.float32)
    return om, dth, dp


@pytest.mark.parametrize("name,factors", [("cfg2", "lds"), ("cfg2", "hbm"), ("cfg5", "hbm"), ("cfg3_n16", "hbm"), ("yaw", "hbm")])
def test_rot_kernels_match_sens_rot_ref_and_adjoint(name, factors):
    """JVP (k = 10) and VJP of the kernel against sens_rot_ref at the kernel's own float32 (x, p, lam_g) on problems 0, 1 and B - 1; the removed
    component dSens[6] against the restatement's; the adjoint identity on the device outputs over the whole batch."""
    import torch
    cfg, P, X0 = _rot_case(name)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032, factors=factors)
    X, Lm, info = dX.cpu().numpy(), lam.cpu().numpy(), dI.cpu().numpy()
    assert (info[:, 5] == 0).all()
    B, L = P32.shape[0], cm.Layout(cfg.N)
    rng = np.random.default_rng(23)
    om, dth, dp = _rot_dirs(cfg, P32, rng)
    V = rng.standard_normal((B, L.nx)).astype(np.float32)
    dV = torch.from_numpy(V).cuda()
    dDX, sj = s.solution_jvp_rot_device(dX, dP, lam, torch.from_numpy(dp).cuda(), torch.from_numpy(dth).cuda(), torch.from_numpy(om).cuda())
    gR, _, _, sv = s.solution_vjp_rot_device(dX, dP, lam, dV, grad_p=False, grad_model=False)
    torch.cuda.synchronize()
    DX, GR, sj, sv = dDX.cpu().numpy(), gR.cpu().numpy(), sj.cpu().numpy(), sv.cpu().numpy()
    assert (sj[:, 0] == 0).all() and (sv[:, 0] == 0).all(), (sj[:, 0], sv[:, 0])
    assert sj[:, 1].max() < RESID and sv[:, 1].max() < RESID, (sj[:, 1].max(), sv[:, 1].max())
    th = _theta32(cfg)
    worst = dict(jvp=0.0, vjp=0.0, adj=0.0, rel=0.0)
    for b in (0, 1, B - 1):
        RS = srr.RotSens(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), Lm[b].astype(np.float64), theta=th)
        for j in range(K):
            r = RS.jvp(om[b, j], dth[b, j] if j == 9 else None, dp[b, j].astype(np.float64) if j == 9 else None)
            worst["jvp"] = max(worst["jvp"], np.abs(DX[b, j] - r).max() / max(np.abs(r).max(), 1e-3))
        r = RS.vjp(V[b].astype(np.float64))
        worst["vjp"] = max(worst["vjp"], float(np.abs(GR[b] - r).max() / max(np.abs(r).max(), 1e-12)))
        rj = max(max(RS.removed(om[b, j]) for j in range(K)), RS.MS.removed(dth[b, 9]))
        rv = RS.removed_vjp()
        worst["rel"] = max(worst["rel"], abs(float(sj[b, 6]) - rj) / max(rj, 1e-6), abs(float(sv[b, 6]) - rv) / max(rv, 1e-6))
        assert (RS.n is None) == (sj[b, 4] == 0) and (RS.n is not None or (sj[b, 6] == 0 and sv[b, 6] == 0))
    for b in range(B):   # <v, J_omega u> = <J_omega^T v, u> over the 9 rotation-only columns
        u = om[b, :9].sum(0)
        lhs = sum(float(V[b].astype(np.float64) @ DX[b, j].astype(np.float64)) for j in range(9))
        rhs = float((GR[b] * u).sum())
        worst["adj"] = max(worst["adj"], abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-6))
    print(f"\n{name} {factors}: residual jvp {sj[:, 1].max():.1e} vjp {sv[:, 1].max():.1e}; dSens[6] jvp max {sj[:, 6].max():.1e} vjp max "
          f"{sv[:, 6].max():.1e}; " + " ".join(f"{a} {v:.1e}" for a, v in worst.items()))
    assert worst["jvp"] <= REF and worst["vjp"] <= REF and worst["adj"] <= ADJ and worst["rel"] <= 1e-2, worst


def test_rot_bit_identities_and_independence():
    """dDirRot = NULL: cmpc_solution_jvp_model_device's bits; the rotation VJP's dl/dp and dl/dtheta: cmpc_solution_vjp_model_device's bits, with
    dGradRot or without; a problem's outputs do not depend on its batch position, the batch size or k (chunks of 8)."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(256, seed=730)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(6)
    om, dth, dp = _rot_dirs(cfg, P32, rng)
    Om, Dm, Dp = torch.from_numpy(om).cuda(), torch.from_numpy(dth).cuda(), torch.from_numpy(dp).cuda()
    V = torch.from_numpy(rng.standard_normal((256, L.nx)).astype(np.float32)).cuda()
    ref, sref = s.solution_jvp_model_device(dX, dP, lam, Dp, Dm)
    nul, snul = s.solution_jvp_rot_device(dX, dP, lam, Dp, Dm, None)
    a, sa = s.solution_jvp_rot_device(dX, dP, lam, Dp, Dm, Om)
    gm_ref, gp_ref, sv_ref = s.solution_vjp_model_device(dX, dP, lam, V)
    gR, gM, gP, sv = s.solution_vjp_rot_device(dX, dP, lam, V)
    gR2, gM2, gP2, _ = s.solution_vjp_rot_device(dX, dP, lam, V, grad_p=False, grad_model=False)
    torch.cuda.synchronize()
    gP3, gM3 = torch.empty_like(gP), torch.empty_like(gM)   # (dGradRot not requested: the wrapper always asks for it)
    rc3 = s._lib.cmpc_solution_vjp_rot_device(s._h, dX.data_ptr(), dP.data_ptr(), lam.data_ptr(), V.data_ptr(), gP3.data_ptr(), gM3.data_ptr(), None,
                                              None, None)
    one, _ = s.solution_jvp_rot_device(dX, dP, lam, Dp[:, 9:10].contiguous(), Dm[:, 9:10].contiguous(), Om[:, 9:10].contiguous())
    ro, _ = s.solution_jvp_rot_device(dX, dP, lam, None, None, Om[:, :9].contiguous())
    torch.cuda.synchronize()
    assert rc3 == 0
    assert torch.equal(nul, ref) and torch.equal(snul, sref)
    assert torch.equal(gP, gp_ref) and torch.equal(gM, gm_ref) and torch.equal(gP3, gp_ref) and torch.equal(gM3, gm_ref)
    assert gP2 is None and gM2 is None and torch.equal(gR2, gR)
    assert torch.equal(one[:, 0], a[:, 9]) and torch.equal(ro, a[:, :9])
    assert (sa[:, 0] == 0).all() and (sv[:, 0] == 0).all() and float(gR.abs().max()) > 0 and not torch.equal(a[:, :9], ref[:, :9])
    # problem 37 alone (batch of 1, another handle)
    b = 37
    s1 = cm.BatchSolver(cfg, 1)
    sl = lambda t: t[b:b + 1].contiguous()
    a1, _ = s1.solution_jvp_rot_device(sl(dX), sl(dP), sl(lam), sl(Dp), sl(Dm), sl(Om))
    r1, m1, p1, _ = s1.solution_vjp_rot_device(sl(dX), sl(dP), sl(lam), sl(V))
    torch.cuda.synchronize()
    assert torch.equal(a1[0], a[b]) and torch.equal(r1[0], gR[b]) and torch.equal(m1[0], gM[b]) and torch.equal(p1[0], gP[b])


def test_rot_sub_batches_beyond_the_workspace_are_bit_identical():
    """B = 1100 > CMPC_SENS_SUB_BATCH: problems 3 and 1090 get the same rotation JVP and VJP bits as a batch of one."""
    import torch
    cfg, P, X0 = cm.synthetic.config2_perturbed_com(1100, seed=740)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    L = cm.Layout(cfg.N)
    om = torch.zeros((1100, 2, 2, L.N, 3), dtype=torch.float64, device=dP.device)
    om[:, 0, 0, :, 2] = 1.0
    om[:, 1, 1, :, 0] = 1.0
    V = torch.ones((1100, L.nx), dtype=torch.float32, device=dP.device)
    a, sa = s.solution_jvp_rot_device(dX, dP, lam, None, None, om)
    g, _, _, sg = s.solution_vjp_rot_device(dX, dP, lam, V, grad_p=False, grad_model=False)
    s1 = cm.BatchSolver(cfg, 1)
    for b in (3, 1090):
        sl = lambda t: t[b:b + 1].contiguous()
        a1, s1s = s1.solution_jvp_rot_device(sl(dX), sl(dP), sl(lam), None, None, sl(om))
        g1, _, _, s1g = s1.solution_vjp_rot_device(sl(dX), sl(dP), sl(lam), sl(V), grad_p=False, grad_model=False)
        torch.cuda.synchronize()
        assert torch.equal(a1[0], a[b]) and torch.equal(s1s[0], sa[b]) and torch.equal(g1[0], g[b]) and torch.equal(s1g[0], sg[b])
    assert (sa[:, 0] == 0).all() and (sg[:, 0] == 0).all() and float(g.abs().max()) > 0


def test_rot_flags():
    """A non-finite omega: status 2 and zeros.  A model row that breaks the model rule: status 3 and zeros (JVP, VJP and value gradient).  The
    neighbours keep their bits."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(32, seed=750)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    rows = np.repeat(cm.config.model_row(cfg)[None], 32, 0)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032, models=rows)
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(10)
    om = torch.from_numpy(rng.standard_normal((32, 2, 2, L.N, 3)) * 1e-2).cuda()
    V = torch.from_numpy(rng.standard_normal((32, L.nx)).astype(np.float32)).cuda()
    a, sa = s.solution_jvp_rot_device(dX, dP, lam, None, None, om)
    g, _, _, sg = s.solution_vjp_rot_device(dX, dP, lam, V, grad_p=False, grad_model=False)
    vg = s.rotation_value_gradient_device(dX, dP, lam)
    bad_om = om.clone()
    bad_om[9, 1, 1, 4, 2] = float("nan")
    an, san = s.solution_jvp_rot_device(dX, dP, lam, None, None, bad_om)
    torch.cuda.synchronize()
    assert (sa[:, 0] == 0).all() and (sg[:, 0] == 0).all()
    keep = [i for i in range(32) if i != 9]
    assert san[9, 0].item() == 2 and (an[9] == 0).all() and torch.equal(an[keep], a[keep]) and torch.equal(san[keep], sa[keep])
    bad = rows.copy()
    bad[5, 0] = 0.0
    ok = s.set_models_device(torch.from_numpy(bad).cuda())
    ab, sab = s.solution_jvp_rot_device(dX, dP, lam, None, None, om)
    gb, _, _, sgb = s.solution_vjp_rot_device(dX, dP, lam, V, grad_p=False, grad_model=False)
    vb = s.rotation_value_gradient_device(dX, dP, lam)
    torch.cuda.synchronize()
    assert int(ok[5]) == 0 and int(ok.sum()) == 31
    assert sab[5, 0].item() == 3 and sgb[5, 0].item() == 3
    assert (ab[5] == 0).all() and (gb[5] == 0).all() and (vb[5] == 0).all()
    keep = [i for i in range(32) if i != 5]
    assert torch.equal(ab[keep], a[keep]) and torch.equal(gb[keep], g[keep]) and torch.equal(vb[keep], vg[keep]) and torch.equal(sab[keep], sa[keep])


def test_rotation_value_gradient_matches_restatement_and_oracle():
    """dV*/domega at the device's (x, lam_g) on config 5 (B = 16): against the restatement at the same point on problems 0, 1 and 15, and against
    central differences of the float64 oracle's optimal cost along the directions of sens_rot_ref.rot_directions on problems 0 and 1."""
    import torch
    from oracle import oracle_lib as ol, problem_nlp
    cfg, P, X0 = cm.synthetic.config5_footstep_candidates(16, seed=761)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    vg = s.rotation_value_gradient_device(dX, dP, lam)
    torch.cuda.synchronize()
    VG_, X, Lm = vg.cpu().numpy(), dX.cpu().numpy(), lam.cpu().numpy()
    assert (dI[:, 5] == 0).all() and VG_.shape == (16, 2, cfg.N, 3)
    oc = problem_nlp.oracle_cfg(cfg)
    opts = ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200)
    h = 1e-5
    worst_fd, worst_ref = 0.0, 0.0
    for b in (0, 1, 15):
        p, x = P32[b].astype(np.float64), X[b].astype(np.float64)
        r = srr.RotSens(cfg, x, p, Lm[b].astype(np.float64), theta=_theta32(cfg)).value_gradient()
        worst_ref = max(worst_ref, float(np.abs(VG_[b] - r).max() / np.abs(r).max()))
        if b == 15:
            continue
        dirs = srr.rot_directions(cfg.N, p)
        Pp = np.stack([srr.p_rotated(cfg.N, p, sg * h * d) for sg in (1.0, -1.0) for _, d, _ in dirs])
        Xs, info = ol.ref_solve_batch(oc, Pp, np.repeat(x[None], Pp.shape[0], 0), opts, nthreads=8)
        assert (info[:, 5] == 0).all()
        f = np.array([ol.nlp_fg(oc, Xs[i], Pp[i])[0] for i in range(Pp.shape[0])])
        fds = (f[:len(dirs)] - f[len(dirs):]) / (2 * h)
        scale = np.abs(fds).max()
        for (_, d, _), fv in zip(dirs, fds):
            worst_fd = max(worst_fd, abs(float((VG_[b] * d).sum()) - fv) / scale)
    print(f"\ncfg5: dV*/domega against oracle differences {worst_fd:.1e}, against sens_rot_ref {worst_ref:.1e}")
    assert worst_fd <= VG and worst_ref <= 1e-6, (worst_fd, worst_ref)


@pytest.mark.parametrize("pad", [False, True])
def test_contacts_rotation_vjp_matches_list_sum(pad):
    """The owner sum on the device against the numpy restatement (the same order of float64 sums) on the yawed lists of footstep_candidates, with
    max_contacts of the lists and of 16; a foot that the sampling would not sample gets zeros."""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    B, N, dt = 8, cfg.N, cfg.sampling_time
    t, pose, n = cm.synthetic.footstep_candidate_lists(cfg, B, 9)
    if pad:
        t = np.concatenate([t, np.zeros((B, 2, 16 - t.shape[2], 2))], 2)
    M = t.shape[2]
    n = n.copy()
    n[2, 1] = 0          # an empty list
    n[3, 0] = M + 1      # a list longer than max_contacts
    now = 2 * dt
    g = np.random.default_rng(4).standard_normal((B, 2, N, 3))
    s = cm.BatchSolver(cfg, B)
    out = s.contacts_rotation_vjp_device(now, torch.from_numpy(np.ascontiguousarray(t)).cuda(), torch.from_numpy(n).cuda(), torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == (B, 2, M, 3)
    for b in range(B):
        for c in range(2):
            nn = int(n[b, c])
            own = srr.stage_owner(N, dt, now, t[b, c], nn) if 1 <= nn <= M else np.zeros(N, int)
            r = srr.list_sum(g[b, c], own, nn, M)
            assert np.abs(out[b, c] - r).max() <= 1e-15 * max(1.0, np.abs(r).max()), (b, c)
    assert not out[2, 1].any() and not out[3, 0].any() and out[0].any()


def test_solve_differentiable_with_rot():
    """torch: rot = 0 gives X and P.grad bit-equal to rot=None and rot.grad bit-equal to the rotation VJP; one gradient step on the yaw of each
    foot's last group of stages (at most 0.02 rad) against the first-knot-force tracking loss lowers the loss as a fresh solve at the rotated P
    measures it."""
    import torch
    cfg, P, X0 = cm.synthetic.config5_footstep_candidates(32)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    N, L = cfg.N, cm.Layout(cfg.N)
    idx = torch.as_tensor(np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)])).cuda()
    dX0 = torch.from_numpy(X032).cuda()
    s0 = cm.BatchSolver(cfg, 32)
    P0 = torch.from_numpy(P32).cuda().requires_grad_(True)
    X = cm.solve_differentiable(s0, P0, dX0)
    target = X.detach()[:, idx] * 0.9
    ((X[:, idx] - target) ** 2).sum().backward()
    s = cm.BatchSolver(cfg, 32)
    Pr = torch.from_numpy(P32).cuda().requires_grad_(True)
    rot = torch.zeros((32, 2, N, 3), dtype=torch.float64, device="cuda", requires_grad=True)
    Xr = cm.solve_differentiable(s, Pr, dX0, rot=rot)
    loss = ((Xr[:, idx] - target) ** 2).sum()
    loss.backward()
    assert torch.equal(Xr.detach(), X.detach()) and torch.equal(Pr.grad, P0.grad)
    assert (s.last_sensitivity_info[:, 0] == 0).all()
    lam = s.multipliers_device(Xr.detach(), Pr.detach())
    gX = torch.zeros_like(Xr)
    gX[:, idx] = 2 * (Xr.detach()[:, idx] - target)
    gR, _, gP, _ = s.solution_vjp_rot_device(Xr.detach(), Pr.detach(), lam, gX, grad_model=False)
    torch.cuda.synchronize()
    assert rot.grad.dtype == torch.float64 and torch.equal(rot.grad, gR) and torch.equal(gP, Pr.grad)
    # one step on the yaw of each foot's last group (the tied stages move together: the group's derivative is the sum over it)
    step = torch.zeros_like(rot)
    G = rot.grad.cpu().numpy()
    for b in range(32):
        for c in range(2):
            ks = [g for g in srr.groups(N, P32[b]) if g[0] == c][-1][1]
            step[b, c, ks, 2] = float(G[b, c, ks, 2].sum())
    alpha = 0.02 / float(step.abs().max())
    P2 = cm.rotate_parameters(Pr.detach(), -alpha * step, N)
    X2, I2 = s.solve_device(P2, dX0)
    torch.cuda.synchronize()
    assert (I2[:, 5] == 0).all() and float((-alpha * step).abs().max()) <= 0.02 * (1 + 1e-12)
    loss2 = ((X2[:, idx] - target) ** 2).sum()
    print(f"\nloss {float(loss):.6e} -> {float(loss2):.6e} (yaw moved by at most 0.02 rad)")
    assert float(loss2) < float(loss)
