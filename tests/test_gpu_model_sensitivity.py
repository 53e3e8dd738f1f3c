"""GPU: derivatives with respect to the per-problem model (include/cmpc.h, "model directions": cmpc_solution_jvp_model_device,
cmpc_solution_vjp_model_device, cmpc_model_value_gradient_device, solve_differentiable(models=...)), held to the float64 dense restatement
tests/sens_model_ref.py at the GPU's own (x, lam_g) and float32 model record, to the adjoint identity, to central differences of the float64 oracle's
optimal cost, and to bit-for-bit agreement with the solution sensitivities and independence of batch position, batch size, k, sub-batches and the
model table.

Limits: those of tests/test_gpu_sensitivity.py (REF, ADJ, RESID) unless a field group needed more; measured values next to each
(profiles/model_sensitivity.txt, tools/gpu_model_sensitivity_cost.py --sweep)."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import sens_model_ref as smr, sens_ref
from tests.test_gpu_sensitivity import ADJ, REF, RESID, _case, _solve

pytestmark = pytest.mark.gpu

M = smr.M
GROUPS = {"friction": [0], "weights": list(range(1, 10)), "corners_left": list(range(10, 22)), "corners_right": list(range(22, 34))}
VG = 1e-4       # dV*/dtheta against oracle central differences of the optimal cost, relative to the largest difference


def _theta32(cfg):
    """the model the solve used: the config's model as its float32 record holds it"""
    return cm.config.model_row(cfg).astype(np.float32).astype(np.float64)


def _model_dirs(cfg, B, L, rng, with_p=True):
    """[B, 14, 34] model directions (the 13 of model_directions and a random one) and [B, 14, n_p] p directions (zero but for the last column)"""
    dm = np.zeros((B, 14, M))
    dm[:, :13] = np.stack([d for _, d in smr.model_directions(cfg)])
    dm[:, 13] = rng.standard_normal((B, M)) * 1e-2
    dp = np.zeros((B, 14, L.np), np.float32)
    if with_p:
        dp[:, 13] = (rng.standard_normal((B, L.np)) * 1e-2 * sens_ref.covered_mask(cfg.N)).astype(np.float32)
    return dm, dp


def _group_gap(g, r):
    return {k: float(np.abs(g[ix] - r[ix]).max() / max(np.abs(r[ix]).max(), 1e-12)) for k, ix in GROUPS.items()}


@pytest.mark.parametrize("name,factors", [("cfg2", "lds"), ("cfg2", "hbm"), ("cfg3", "hbm"), ("cfg5", "hbm"), ("cfg3_n16", "hbm"), ("cfg3_n25", "hbm")])
def test_model_kernels_match_sens_model_ref_and_adjoint(name, factors):
    """JVP (13 model directions and one combined p + theta column: k = 14, two chunks) and VJP of the kernel against sens_model_ref at the kernel's own
    float32 (x, p, lam_g) and model record; the VJP per field group; the removed component dSens[6] against the restatement's; the adjoint identity on
    the device outputs."""
    import torch
    cfg, P, X0 = _case(name)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032, factors=factors)
    X, Lm, info = dX.cpu().numpy(), lam.cpu().numpy(), dI.cpu().numpy()
    assert (info[:, 5] == 0).all()
    B, L = P32.shape[0], cm.Layout(cfg.N)
    rng = np.random.default_rng(17)
    dm, dp = _model_dirs(cfg, B, L, rng)
    V = rng.standard_normal((B, L.nx)).astype(np.float32)
    dDX, sj = s.solution_jvp_model_device(dX, dP, lam, torch.from_numpy(dp).cuda(), torch.from_numpy(dm).cuda())
    gM, gP, sv = s.solution_vjp_model_device(dX, dP, lam, torch.from_numpy(V).cuda())
    torch.cuda.synchronize()
    DX, GM, sj, sv = dDX.cpu().numpy(), gM.cpu().numpy(), sj.cpu().numpy(), sv.cpu().numpy()
    assert (sj[:, 0] == 0).all() and (sv[:, 0] == 0).all(), (sj[:, 0], sv[:, 0])
    assert sj[:, 1].max() < RESID and sv[:, 1].max() < RESID, (sj[:, 1].max(), sv[:, 1].max())
    th = _theta32(cfg)
    worst = dict(jvp=0.0, adj=0.0, rel=0.0)
    groups = {k: 0.0 for k in GROUPS}
    for b in (0, 1, B - 1):
        MS = smr.ModelSens(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), Lm[b].astype(np.float64), theta=th)
        for j in range(14):
            r = MS.jvp(dm[b, j], dp[b, j].astype(np.float64) if j == 13 else None)
            worst["jvp"] = max(worst["jvp"], np.abs(DX[b, j] - r).max() / max(np.abs(r).max(), 1e-3))
        for k, v in _group_gap(GM[b], MS.vjp(V[b].astype(np.float64))).items():
            groups[k] = max(groups[k], v)
        rj = max(MS.removed(dm[b, j]) for j in range(14))
        rv = MS.removed_vjp()
        worst["rel"] = max(worst["rel"], abs(float(sj[b, 6]) - rj) / max(rj, 1e-6), abs(float(sv[b, 6]) - rv) / max(rv, 1e-6))
        assert (MS.n is None) == (sj[b, 4] == 0) and (MS.n is not None or (sj[b, 6] == 0 and sv[b, 6] == 0))
    for b in range(B):   # <v, J_theta u> = <J_theta^T v, u> over the 13 model-only columns
        u = dm[b, :13].sum(0)
        lhs = sum(float(V[b].astype(np.float64) @ DX[b, j].astype(np.float64)) for j in range(13))
        rhs = float(GM[b] @ u)
        worst["adj"] = max(worst["adj"], abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-6))
    print(f"\n{name} {factors}: residual jvp {sj[:, 1].max():.1e} vjp {sv[:, 1].max():.1e}; dSens[6] jvp max {sj[:, 6].max():.1e} vjp max "
          f"{sv[:, 6].max():.1e}; " + " ".join(f"{a} {v:.1e}" for a, v in worst.items()) + "; vjp " +
          " ".join(f"{a} {v:.1e}" for a, v in groups.items()))
    assert worst["jvp"] <= REF and worst["adj"] <= ADJ and worst["rel"] <= 1e-2, worst
    assert max(groups.values()) <= REF, groups


def test_bit_identity_with_the_solution_sensitivities_and_independence():
    """dDirModel = NULL: cmpc_solution_jvp_device's bits; the model VJP's dl/dp: cmpc_solution_vjp_device's bits; a problem's model outputs do not
    depend on its batch position, the batch size, k (chunks of 8) or on a model table holding the config's own model."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(256, seed=630)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(5)
    dm, dp = _model_dirs(cfg, 256, L, rng)
    Dm, Dp = torch.from_numpy(dm).cuda(), torch.from_numpy(dp).cuda()
    V = torch.from_numpy(rng.standard_normal((256, L.nx)).astype(np.float32)).cuda()
    ref, sref = s.solution_jvp_device(dX, dP, lam, Dp)
    nul, snul = s.solution_jvp_model_device(dX, dP, lam, Dp, None)
    a, sa = s.solution_jvp_model_device(dX, dP, lam, Dp, Dm)
    gp_ref, _ = s.solution_vjp_device(dX, dP, lam, V)
    gM, gP, sv = s.solution_vjp_model_device(dX, dP, lam, V)
    gM2, gP2, _ = s.solution_vjp_model_device(dX, dP, lam, V, grad_p=False)
    one, _ = s.solution_jvp_model_device(dX, dP, lam, Dp[:, 13:14].contiguous(), Dm[:, 13:14].contiguous())
    mo, _ = s.solution_jvp_model_device(dX, dP, lam, None, Dm[:, :13].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(nul, ref) and torch.equal(snul, sref)
    assert torch.equal(gP, gp_ref) and gP2 is None and torch.equal(gM2, gM)
    assert torch.equal(one[:, 0], a[:, 13]) and torch.equal(mo, a[:, :13])
    assert (sa[:, 0] == 0).all() and (sv[:, 0] == 0).all() and float(gM.abs().max()) > 0
    # problem 37 alone (batch of 1, another handle)
    b = 37
    s1 = cm.BatchSolver(cfg, 1)
    sl = lambda t: t[b:b + 1].contiguous()
    a1, _ = s1.solution_jvp_model_device(sl(dX), sl(dP), sl(lam), sl(Dp), sl(Dm))
    g1, p1, _ = s1.solution_vjp_model_device(sl(dX), sl(dP), sl(lam), sl(V))
    torch.cuda.synchronize()
    assert torch.equal(a1[0], a[b]) and torch.equal(g1[0], gM[b]) and torch.equal(p1[0], gP[b])
    # a table holding the config's own model: the records are bit-equal, so are the outputs
    st = cm.BatchSolver(cfg, 256)
    st.set_models_device(torch.from_numpy(np.repeat(cm.config.model_row(cfg)[None], 256, 0)).cuda())
    at, _ = st.solution_jvp_model_device(dX, dP, lam, Dp, Dm)
    gt, pt, _ = st.solution_vjp_model_device(dX, dP, lam, V)
    vt = st.model_value_gradient_device(dX, dP, lam)
    vn = s.model_value_gradient_device(dX, dP, lam)
    torch.cuda.synchronize()
    assert torch.equal(at, a) and torch.equal(gt, gM) and torch.equal(pt, gP) and torch.equal(vt, vn)


def test_sub_batches_beyond_the_workspace_are_bit_identical():
    """B = 1100 > CMPC_SENS_SUB_BATCH: problems 3 and 1090 get the same model JVP and VJP bits as a batch of one."""
    import torch
    cfg, P, X0 = cm.synthetic.config2_perturbed_com(1100, seed=640)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    L = cm.Layout(cfg.N)
    dm = torch.zeros((1100, 2, M), dtype=torch.float64, device=dP.device)
    dm[:, 0, 0] = 1.0
    dm[:, 1, smr.corner_index(0, 1, 2)] = 1.0
    V = torch.ones((1100, L.nx), dtype=torch.float32, device=dP.device)
    a, sa = s.solution_jvp_model_device(dX, dP, lam, None, dm)
    g, _, sg = s.solution_vjp_model_device(dX, dP, lam, V, grad_p=False)
    s1 = cm.BatchSolver(cfg, 1)
    for b in (3, 1090):
        sl = lambda t: t[b:b + 1].contiguous()
        a1, s1s = s1.solution_jvp_model_device(sl(dX), sl(dP), sl(lam), None, sl(dm))
        g1, _, s1g = s1.solution_vjp_model_device(sl(dX), sl(dP), sl(lam), sl(V), grad_p=False)
        torch.cuda.synchronize()
        assert torch.equal(a1[0], a[b]) and torch.equal(s1s[0], sa[b]) and torch.equal(g1[0], g[b]) and torch.equal(s1g[0], sg[b])
    assert (sa[:, 0] == 0).all() and (sg[:, 0] == 0).all()


def _randomised_rows(cfg, B, seed):
    """friction U(0.25, 1.0), feet scaled U(0.8, 1.2) (as tests/test_gpu_models.py) around cfg's model"""
    rng = np.random.default_rng(seed)
    base = cm.config.model_row(cfg)
    rows = np.repeat(base[None], B, 0)
    rows[:, 0] = rng.uniform(0.25, 1.0, B)
    rows[:, 10:] *= rng.uniform(0.8, 1.2, B)[:, None]
    return rows


def test_randomised_models_each_problem_at_its_own_model():
    """Per-problem models (friction and foot size randomised): each problem's JVP, VJP and dV*/dtheta against the restatement built with that
    problem's model; a row that breaks the model rule gets status 3 and zeros, and its neighbours keep their bits."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(32, seed=650)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    rows = _randomised_rows(cfg, 32, 651)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032, models=rows)
    assert (dI[:, 5] == 0).all()
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(9)
    dm, dp = _model_dirs(cfg, 32, L, rng, with_p=False)
    Dm = torch.from_numpy(dm).cuda()
    V = torch.from_numpy(rng.standard_normal((32, L.nx)).astype(np.float32)).cuda()
    a, sa = s.solution_jvp_model_device(dX, dP, lam, None, Dm)
    g, _, sg = s.solution_vjp_model_device(dX, dP, lam, V, grad_p=False)
    vg = s.model_value_gradient_device(dX, dP, lam)
    torch.cuda.synchronize()
    A, G, VG_, X, Lm = a.cpu().numpy(), g.cpu().numpy(), vg.cpu().numpy(), dX.cpu().numpy(), lam.cpu().numpy()
    assert (sa[:, 0] == 0).all() and (sg[:, 0] == 0).all()
    worst = dict(jvp=0.0, vjp=0.0, vg=0.0)
    for b in (0, 7, 31):
        th = rows[b].astype(np.float32).astype(np.float64)
        MS = smr.ModelSens(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), Lm[b].astype(np.float64), theta=th)
        for j in range(14):
            r = MS.jvp(dm[b, j])
            worst["jvp"] = max(worst["jvp"], np.abs(A[b, j] - r).max() / max(np.abs(r).max(), 1e-3))
        worst["vjp"] = max(worst["vjp"], max(_group_gap(G[b], MS.vjp(V[b].cpu().numpy().astype(np.float64))).values()))
        r = MS.value_gradient()
        worst["vg"] = max(worst["vg"], float(np.abs(VG_[b] - r).max() / np.abs(r).max()))
    print("\nrandomised models: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["jvp"] <= REF and worst["vjp"] <= REF and worst["vg"] <= 1e-6, worst
    # a bad row (friction 0): status 3 and zeros; the neighbours keep their bits
    bad = rows.copy()
    bad[5, 0] = 0.0
    ok = s.set_models_device(torch.from_numpy(bad).cuda())
    ab, sab = s.solution_jvp_model_device(dX, dP, lam, None, Dm)
    gb, _, sgb = s.solution_vjp_model_device(dX, dP, lam, V, grad_p=False)
    vb = s.model_value_gradient_device(dX, dP, lam)
    torch.cuda.synchronize()
    assert int(ok[5]) == 0 and int(ok.sum()) == 31
    assert sab[5, 0].item() == 3 and sgb[5, 0].item() == 3
    assert (ab[5] == 0).all() and (gb[5] == 0).all() and (vb[5] == 0).all()
    keep = [i for i in range(32) if i != 5]
    assert torch.equal(ab[keep], a[keep]) and torch.equal(gb[keep], g[keep]) and torch.equal(vb[keep], vg[keep]) and torch.equal(sab[keep], sa[keep])


@pytest.mark.parametrize("name", ["cfg2", "cfg5"])
def test_model_value_gradient_matches_oracle(name):
    """dV*/dtheta at the device's (x, lam_g) against central differences of the float64 oracle's optimal cost along every direction of
    model_directions (2 problems), and against the restatement at the same point."""
    import torch
    from oracle import oracle_lib as ol
    cfg, P, X0 = (cm.synthetic.config2_perturbed_com(16, seed=660) if name == "cfg2" else cm.synthetic.config5_footstep_candidates(16, seed=661))
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    vg = s.model_value_gradient_device(dX, dP, lam)
    torch.cuda.synchronize()
    VG_, X, Lm = vg.cpu().numpy(), dX.cpu().numpy(), lam.cpu().numpy()
    th = _theta32(cfg)
    dirs = smr.model_directions(cfg)
    opts = ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200)
    worst_fd, worst_ref = 0.0, 0.0
    for b in (0, 1):
        p, x = P32[b].astype(np.float64), X[b].astype(np.float64)
        MS = smr.ModelSens(cfg, x, p, Lm[b].astype(np.float64), theta=th)
        r = MS.value_gradient()
        worst_ref = max(worst_ref, float(np.abs(VG_[b] - r).max() / np.abs(r).max()))
        fds = []
        for _, d in dirs:
            h = max(1e-5 * float(np.abs(th[d != 0]).max()), 1e-6)
            f = []
            for sg in (1.0, -1.0):
                oc = smr.nlp_cfg(cfg, th + sg * h * d)
                Xs, info = ol.ref_solve_batch(oc, p[None], x[None], opts)
                assert (info[:, 5] == 0).all()
                f.append(ol.nlp_fg(oc, Xs[0], p)[0])
            fds.append((f[0] - f[1]) / (2 * h))
        scale = max(abs(v) for v in fds)
        for (_, d), fv in zip(dirs, fds):
            worst_fd = max(worst_fd, abs(VG_[b] @ d - fv) / scale)
    print(f"\n{name}: dV*/dtheta against oracle differences {worst_fd:.1e}, against sens_model_ref {worst_ref:.1e}")
    assert worst_fd <= VG and worst_ref <= 1e-6, (worst_fd, worst_ref)


def test_solve_differentiable_with_models():
    """torch: models.grad equals the model VJP bit for bit, P.grad equals the models=None run bit for bit (the table holds the config's own model),
    and one gradient step on the weights against the first-knot-force tracking loss lowers the loss as a fresh solve measures it."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(64, seed=550)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    L = cm.Layout(cfg.N)
    idx = torch.as_tensor(np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)])).cuda()
    dX0 = torch.from_numpy(X032).cuda()
    # models = None
    s0 = cm.BatchSolver(cfg, 64)
    P0 = torch.from_numpy(P32).cuda().requires_grad_(True)
    X = cm.solve_differentiable(s0, P0, dX0)
    target = X.detach()[:, idx] * 0.9
    ((X[:, idx] - target) ** 2).sum().backward()
    # with the config's own model in a table
    s = cm.BatchSolver(cfg, 64)
    Pm = torch.from_numpy(P32).cuda().requires_grad_(True)
    models = torch.from_numpy(np.repeat(cm.config.model_row(cfg)[None], 64, 0)).cuda().requires_grad_(True)
    Xm = cm.solve_differentiable(s, Pm, dX0, models=models)
    loss = ((Xm[:, idx] - target) ** 2).sum()
    loss.backward()
    assert torch.equal(Xm.detach(), X.detach())
    assert (s.last_sensitivity_info[:, 0] == 0).all() and (s.last_models_ok == 1).all()
    assert torch.equal(Pm.grad, P0.grad)
    lam = s.multipliers_device(Xm.detach(), Pm.detach())
    gX = torch.zeros_like(Xm)
    gX[:, idx] = 2 * (Xm.detach()[:, idx] - target)
    gM, gP, _ = s.solution_vjp_model_device(Xm.detach(), Pm.detach(), lam, gX)
    torch.cuda.synchronize()
    assert models.grad.dtype == torch.float64 and torch.equal(models.grad, gM) and torch.equal(gP, Pm.grad)
    # one step on the weights (fields 1..9), at most 1 % of each weight
    w = models.detach()[:, 1:10]
    step = models.grad[:, 1:10]
    alpha = 1e-2 / max(float((step.abs() / w.clamp_min(1e-9)).max()), 1e-12)
    m2 = models.detach().clone()
    m2[:, 1:10] = (w - alpha * step).clamp_min(1e-6)
    s.set_models_device(m2.contiguous())
    X2, I2 = s.solve_device(Pm.detach(), dX0)
    torch.cuda.synchronize()
    assert (I2[:, 5] == 0).all()
    loss2 = ((X2[:, idx] - target) ** 2).sum()
    print(f"\nloss {float(loss):.6e} -> {float(loss2):.6e} (weights moved by at most 1 %)")
    assert float(loss2) < float(loss)
