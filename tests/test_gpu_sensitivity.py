"""GPU: the solution sensitivities of include/cmpc.h (cmpc_solution_jvp_device / cmpc_solution_vjp_device, BatchSolver.feedback_gain_device,
solve_differentiable), held to the float64 dense restatement tests/sens_ref.py at the GPU's own (x, lam_g), to central differences of the float64
oracle, to the adjoint identity, and to bit-for-bit independence of batch position, batch size, k, repeated calls and per-problem models.

Limits: measured on MI355X over the problems below (profiles/solution_sensitivity.txt); measured value next to each."""
import copy

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity, sens_ref
from tests.test_multipliers_cpu import golden_cfg

pytestmark = pytest.mark.gpu

# Limits a small margin above the worst case of the sweep of 5 seeds x 512 problems per configuration (tools/gpu_sensitivity_cost.py --sweep,
# profiles/solution_sensitivity.txt) and of this file's batches; measured value next to each.
REF = 5e-5      # kernel against sens_ref at the same float32 (x, p, lam_g), relative to the largest entry of the column: sweep 3.0e-5 (config 5),
#                 this file 5.1e-7, goldens 3.6e-6
ADJ = 6e-4      # <v, J u> against <J^T v, u> on the float32 device outputs, relative: sweep 4.5e-4 (config 5), this file 6.0e-6
RESID = 1e-6    # relative residual against the unshifted system: sweep 4.1e-7 (config 3), this file 6.2e-9
FD = 2e-6       # feedback gain against oracle central differences, config 2 (double support): measured 3.4e-7
FD_WALK = 1e-4  # ... config 5 problems without weakly active rows of loaded feet, oracle at mu 1e-12: measured 6.4e-5, the slack-floor bias
#                 curvature x s_min / z of active landing and friction rows (with the floor at 1e-12 sens_ref meets the same differences to 3e-6)


def _solve(cfg, P32, X032, factors=None, models=None):
    import torch
    B = P32.shape[0]
    s = cm.BatchSolver(cfg, B, factors=factors)
    if models is not None:
        s.set_models(models)
    s.set_multiplier_output()
    dP, dX0 = torch.from_numpy(P32).cuda(), torch.from_numpy(X032).cuda()
    dX, dI = s.solve_device(dP, dX0)
    lam = s.multipliers_device(dX, dP)
    torch.cuda.synchronize()
    return s, dP, dX, dI, lam


def _dirs(cfg, p, lam):
    return np.stack([d for _, d in sens_ref.directions(cfg, p.astype(np.float64), lam.astype(np.float64))]).astype(np.float32)


def _case(name):
    if name == "cfg2":
        return cm.synthetic.config2_perturbed_com(64, seed=510)
    if name == "cfg3":
        return cm.synthetic.config3_external_push(64, seed=511)
    if name == "cfg5":
        return cm.synthetic.config5_footstep_candidates(64, seed=512)
    if name == "cfg3_n16":
        return cm.synthetic.config3_external_push(64, N=16, seed=513)
    if name == "cfg3_n25":
        return cm.synthetic.config3_external_push(64, N=25, seed=514)
    raise ValueError(name)


@pytest.mark.parametrize("name,factors", [("cfg2", "lds"), ("cfg2", "hbm"), ("cfg3", "hbm"), ("cfg5", "hbm"), ("cfg3_n16", "hbm"), ("cfg3_n25", "hbm")])
def test_kernel_matches_sens_ref_and_adjoint(name, factors):
    """JVP (several directions in one call) and VJP of the kernel against sens_ref at the kernel's own float32 (x, p, lam_g); the adjoint identity on
    the device outputs; status 0 and a small residual everywhere."""
    cfg, P, X0 = _case(name)
    check_sens_ref_and_adjoint(cfg, P.astype(np.float32), X0.astype(np.float32), factors, name)


def check_sens_ref_and_adjoint(cfg, P32, X032, factors, name):
    """The body of test_kernel_matches_sens_ref_and_adjoint on any batch: solve, then JVP (k = 9) and VJP against sens_ref on problems 0, 1 and
    B - 1, the adjoint identity on every problem, REF / ADJ / RESID as above."""
    import torch
    s, dP, dX, dI, lam = _solve(cfg, P32, X032, factors=factors)
    X, Lm, info = dX.cpu().numpy(), lam.cpu().numpy(), dI.cpu().numpy()
    assert (info[:, 5] == 0).all()
    B, L = P32.shape[0], cm.Layout(cfg.N)
    probe = [0, 1, B - 1]
    rng = np.random.default_rng(7)
    # the eight generic unit directions of sens_ref.directions (com0 x, com0 z, dcom0, h0, comRef, hRef, fExt, tauExt) and one random covered
    # direction (every block, boxes and currentPos included): k = 9, two chunks of the kernel
    gen = _dirs(cfg, P32[0], Lm[0])[:8]
    dirs = np.zeros((B, 9, L.np), np.float32)
    dirs[:, :8] = gen
    dirs[:, 8] = (rng.standard_normal((B, L.np)) * 1e-2 * sens_ref.covered_mask(cfg.N)).astype(np.float32)
    k = 9
    V = rng.standard_normal((B, L.nx)).astype(np.float32)
    dDX, sj = s.solution_jvp_device(dX, dP, lam, torch.from_numpy(dirs).cuda())
    dGP, sv = s.solution_vjp_device(dX, dP, lam, torch.from_numpy(V).cuda())
    torch.cuda.synchronize()
    DX, GP, sj, sv = dDX.cpu().numpy(), dGP.cpu().numpy(), sj.cpu().numpy(), sv.cpu().numpy()
    assert (sj[:, 0] == 0).all() and (sv[:, 0] == 0).all(), (sj[:, 0], sv[:, 0])
    print(f"\n{name} {factors}: residual jvp {sj[:, 1].max():.1e} vjp {sv[:, 1].max():.1e}, weak rows max {sj[:, 2].max():.0f}, "
          f"largest Sigma {sj[:, 3].max():.1e}")
    assert sj[:, 1].max() < RESID and sv[:, 1].max() < RESID
    worst = dict(jvp=0.0, vjp=0.0, adj=0.0)
    for b in probe:
        S = sens_ref.Sens(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), Lm[b].astype(np.float64))
        for j in range(k):
            r = S.jvp(dirs[b, j].astype(np.float64))
            worst["jvp"] = max(worst["jvp"], np.abs(DX[b, j] - r).max() / max(np.abs(r).max(), 1e-3))
        cov = sens_ref.covered_mask(cfg.N)
        gr = S.vjp(V[b].astype(np.float64))
        worst["vjp"] = max(worst["vjp"], np.abs((GP[b] - gr) * cov).max() / np.abs(gr).max())
    for b in range(B):
        u = dirs[b].astype(np.float64).sum(0)
        lhs = sum(float(V[b].astype(np.float64) @ DX[b, j].astype(np.float64)) for j in range(k))
        rhs = float(GP[b].astype(np.float64) @ u)
        worst["adj"] = max(worst["adj"], abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-6))
    print(" ".join(f"{a} {v:.1e}" for a, v in worst.items()))
    assert worst["jvp"] <= REF and worst["vjp"] <= REF and worst["adj"] <= ADJ, worst


def test_feedback_gain_matches_oracle_finite_differences():
    """The nine feedback-gain columns (and the other directions) against central differences of the float64 oracle's x*(p) on problems without
    weakly active rows."""
    import torch
    from oracle import oracle_lib as ol, problem_nlp
    cfg, P, X0 = cm.synthetic.config2_perturbed_com(64, seed=520)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    G, sens = s.feedback_gain_device(dX, dP, lam)
    torch.cuda.synchronize()
    G, sens, X = G.cpu().numpy(), sens.cpu().numpy(), dX.cpu().numpy()
    assert G.shape == (64, 24, 9) and (sens[:, 0] == 0).all()
    L = cm.Layout(cfg.N)
    oc = problem_nlp.oracle_cfg(cfg)
    idx = np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)])
    checked, skipped, worst = 0, 0, 0.0
    for b in range(8):
        if sens[b, 2] > 0:
            skipped += 1
            continue
        p = P32[b].astype(np.float64)
        h = 1e-4
        Pp = np.concatenate([p + h * np.eye(L.np)[L.p_com0:L.p_com0 + 9], p - h * np.eye(L.np)[L.p_com0:L.p_com0 + 9]])
        Xs, info = ol.ref_solve_batch(oc, Pp, np.repeat(X[b:b + 1].astype(np.float64), 18, 0), ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=8)
        assert (info[:, 5] == 0).all()
        n = parity._internal_force_direction(L, p)
        for i in range(9):
            fd = (Xs[i] - Xs[9 + i]) / (2 * h)
            if n is not None:
                fd = fd - n * (n @ fd)
            gap = np.abs(G[b, :, i] - fd[idx]).max() / max(np.abs(fd[idx]).max(), 1e-2)
            worst = max(worst, gap)
        checked += 1
    print(f"\nfeedback gain: {checked} problems checked, {skipped} with weakly active rows skipped, worst gap {worst:.1e}")
    assert checked >= 4 and worst <= FD, worst


def test_bit_identity_position_batch_k_calls_models_and_solves_untouched():
    """A problem's outputs do not depend on its batch position, the batch size, k, repeated calls or on being in a mixed-model batch; the solves'
    x / info are bit-identical before and after sensitivity calls."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(256, seed=530)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    X1, I1 = dX.cpu().numpy().copy(), dI.cpu().numpy().copy()
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(3)
    dirs = np.zeros((256, 16, L.np), np.float32)
    for i, q in enumerate([L.p_com0 + a for a in range(9)] + [L.p_comref + 9 + a for a in range(3)] + [L.p_fext + a for a in range(4)]):
        dirs[:, i, q] = 1.0
    dirs[:, 15] += rng.standard_normal((256, L.np)).astype(np.float32) * sens_ref.covered_mask(cfg.N).astype(np.float32) * 1e-2
    Dd = torch.from_numpy(dirs).cuda()
    a, sa = s.solution_jvp_device(dX, dP, lam, Dd)
    b2, sb = s.solution_jvp_device(dX, dP, lam, Dd)
    one, _ = s.solution_jvp_device(dX, dP, lam, Dd[:, 15:16].contiguous())
    V = torch.from_numpy(rng.standard_normal((256, L.nx)).astype(np.float32)).cuda()
    g1, _ = s.solution_vjp_device(dX, dP, lam, V)
    torch.cuda.synchronize()
    assert torch.equal(a, b2) and torch.equal(sa, sb)
    assert torch.equal(one[:, 0], a[:, 15])
    # x / info of a fresh solve on the same handle: bit-identical to the first
    dX2, dI2 = s.solve_device(dP, torch.from_numpy(X032).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(dX2.cpu().numpy(), X1) and np.array_equal(dI2.cpu().numpy()[:, [0, 1, 2, 3, 4, 5, 7]], I1[:, [0, 1, 2, 3, 4, 5, 7]])
    # problem 37 alone (batch of 1, other handle)
    b = 37
    s1 = cm.BatchSolver(cfg, 1)
    a1, _ = s1.solution_jvp_device(dX[b:b + 1].contiguous(), dP[b:b + 1].contiguous(), lam[b:b + 1].contiguous(), Dd[b:b + 1].contiguous())
    v1, _ = s1.solution_vjp_device(dX[b:b + 1].contiguous(), dP[b:b + 1].contiguous(), lam[b:b + 1].contiguous(), V[b:b + 1].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a1[0], a[b]) and torch.equal(v1[0], g1[b])
    # mixed-model batch: every problem on the handle's own model except problem 5, whose model is another robot's weights; problem 5 against a
    # homogeneous handle of that model, the others against the homogeneous batch above
    cfg2 = copy.deepcopy(cfg)
    cfg2.com_weight = [20.0, 20.0, 150.0]
    cfg2.contact_force_symmetry_weight = 5.0
    models = [cfg] * 256
    models[5] = cfg2
    sm = cm.BatchSolver(cfg, 256)
    sm.set_models(models)
    am, _ = sm.solution_jvp_device(dX, dP, lam, Dd)
    s2 = cm.BatchSolver(cfg2, 256)
    a2, _ = s2.solution_jvp_device(dX, dP, lam, Dd)
    torch.cuda.synchronize()
    assert torch.equal(am[:5], a[:5]) and torch.equal(am[6:], a[6:]) and torch.equal(am[5], a2[5])


def test_flags_zero_outputs_and_leave_neighbours_alone():
    """status 3 (parity.break_subset) and status 2 (NaN in p): zero outputs; the neighbours match a batch without them, bit for bit."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(64, seed=540)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    L = cm.Layout(cfg.N)
    dirs = torch.zeros((64, 3, L.np), dtype=torch.float32, device=dP.device)
    dirs[:, 0, L.p_com0] = 1.0
    dirs[:, 1, L.p_comref + 20] = 1.0
    dirs[:, 2, L.p_fext + 4] = 1.0
    V = torch.ones((64, L.nx), dtype=torch.float32, device=dP.device)
    a, sa = s.solution_jvp_device(dX, dP, lam, dirs)
    g, sg = s.solution_vjp_device(dX, dP, lam, V)
    Pb = dP.clone()
    Pb[3] = torch.from_numpy(parity.break_subset(cfg.N, P32[3], "nominal")).cuda()
    Pb[9, L.p_comref + 4] = float("nan")
    ab, sab = s.solution_jvp_device(dX, Pb, lam, dirs)
    gb, sgb = s.solution_vjp_device(dX, Pb, lam, V)
    torch.cuda.synchronize()
    assert (sa[:, 0] == 0).all() and (sg[:, 0] == 0).all()
    assert sab[3, 0].item() == 3 and sab[9, 0].item() == 2 and sgb[3, 0].item() == 3 and sgb[9, 0].item() == 2
    assert (ab[3] == 0).all() and (ab[9] == 0).all() and (gb[3] == 0).all() and (gb[9] == 0).all()
    keep = [i for i in range(64) if i not in (3, 9)]
    assert torch.equal(ab[keep], a[keep]) and torch.equal(gb[keep], g[keep]) and torch.equal(sab[keep], sa[keep])


def test_solve_differentiable_grad_and_one_descent_step():
    """torch: P.grad equals the VJP output bit for bit; one gradient step on comRef against a first-knot-force tracking loss lowers the loss as a fresh
    solve measures it."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(64, seed=550)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, 64)
    L = cm.Layout(cfg.N)
    idx = torch.as_tensor(np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)])).cuda()
    dP = torch.from_numpy(P32).cuda().requires_grad_(True)
    dX0 = torch.from_numpy(X032).cuda()
    X = cm.solve_differentiable(s, dP, dX0)
    target = X.detach()[:, idx] * 0.9
    loss = ((X[:, idx] - target) ** 2).sum()
    loss.backward()
    assert (s.last_sensitivity_info[:, 0] == 0).all()
    lam = s.multipliers_device(X.detach(), dP.detach())
    gX = torch.zeros_like(X)
    gX[:, idx] = 2 * (X.detach()[:, idx] - target)
    gP, _ = s.solution_vjp_device(X.detach(), dP.detach(), lam, gX)
    torch.cuda.synchronize()
    assert torch.equal(dP.grad, gP)
    # one step on comRef only
    sl = slice(L.p_comref, L.p_comref + 3 * (cfg.N + 1))
    step = dP.grad[:, sl]
    alpha = 1e-2 / max(float(step.abs().max()), 1e-12)
    P2 = dP.detach().clone()
    P2[:, sl] -= alpha * step          # (only comRef is written: the other entries keep their bits, -0.0 included, which subset rule 3 compares)
    X2, I2 = s.solve_device(P2, dX0)
    torch.cuda.synchronize()
    assert (I2[:, 5] == 0).all()
    loss2 = ((X2[:, idx] - target) ** 2).sum()
    print(f"\nloss {float(loss):.6e} -> {float(loss2):.6e}")
    assert float(loss2) < float(loss)


def test_goldens_match_sens_ref():
    """The goldens' problems solved on the device (cfg2, cfg5, yaw, push): the JVP against sens_ref at the device's own (x, lam_g)."""
    import torch
    worst = 0.0
    for name, which in (("cfg2", None), ("cfg5", None), ("yaw", "tmp"), ("push", "tmp")):
        import os
        d = np.load(os.path.join(os.path.dirname(__file__), "golden", f"argmin_ref_{name}_{which}.npz" if which else f"argmin_{name}.npz"))
        cfg = golden_cfg(name, which)
        P32 = d["P"].astype(np.float32)
        B = P32.shape[0]
        X032 = d["X0"].astype(np.float32) if "X0" in d.files else d["x_star"].astype(np.float32)
        s, dP, dX, dI, lam = _solve(cfg, P32, X032)
        X, Lm = dX.cpu().numpy(), lam.cpu().numpy()
        dirs = torch.from_numpy(np.stack([np.resize(_dirs(cfg, P32[b], Lm[b]), (6, P32.shape[1])) for b in range(B)])).cuda()
        DX, sj = s.solution_jvp_device(dX, dP, lam, dirs)
        torch.cuda.synchronize()
        DX, sj, D = DX.cpu().numpy(), sj.cpu().numpy(), dirs.cpu().numpy()
        assert (sj[:, 0] == 0).all()
        for b in range(min(B, 3)):
            S = sens_ref.Sens(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), Lm[b].astype(np.float64))
            for j in range(6):
                r = S.jvp(D[b, j].astype(np.float64))
                worst = max(worst, np.abs(DX[b, j] - r).max() / max(np.abs(r).max(), 1e-3))
    print(f"\ngoldens: kernel vs sens_ref {worst:.1e}")
    assert worst <= REF


def test_feedback_gain_of_walking_problems_matches_oracle_finite_differences():
    """Config 5 (yawed footstep candidates: swing phases with their landing boxes): the nine feedback-gain columns against central differences of the
    float64 oracle converged to mu 1e-12, on the problems without weakly active rows of loaded feet (dSens[2] == 0).  (Config 3's pushes leave an
    unloaded stance corner at the apex of its pyramid in every problem of a 64-batch: those kinks are loaded)"""
    import torch
    from oracle import oracle_lib as ol, problem_nlp
    cfg, P, X0 = cm.synthetic.config5_footstep_candidates(64, seed=560)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    G, sens = s.feedback_gain_device(dX, dP, lam)
    torch.cuda.synchronize()
    G, sens, X = G.cpu().numpy(), sens.cpu().numpy(), dX.cpu().numpy()
    assert (sens[:, 0] == 0).all()
    L = cm.Layout(cfg.N)
    oc = problem_nlp.oracle_cfg(cfg)
    idx = np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)])
    clean = [b for b in range(64) if sens[b, 2] == 0][:6]
    worst = 0.0
    for b in clean:
        p = P32[b].astype(np.float64)
        h = 1e-4
        E = np.eye(L.np)[L.p_com0:L.p_com0 + 9]
        Xs, info = ol.ref_solve_batch(oc, np.concatenate([p + h * E, p - h * E]), np.repeat(X[b:b + 1].astype(np.float64), 18, 0),
                                      ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200), nthreads=8)
        assert (info[:, 5] == 0).all()
        for i in range(9):
            fd = ((Xs[i] - Xs[9 + i]) / (2 * h))[idx]
            worst = max(worst, np.abs(G[b, :, i] - fd).max() / max(np.abs(fd).max(), 1e-2))
    print(f"\nwalking feedback gain: {len(clean)} problems without weakly active rows of loaded feet (of 64, counted {int((sens[:, 2] == 0).sum())}), "
          f"worst gap {worst:.1e}")
    assert len(clean) >= 3 and worst <= FD_WALK, worst


def test_class_feedback_gain_after_advance():
    """CentroidalMPC.get_feedback_gain() after advance() equals BatchSolver.feedback_gain_device at the handle's own solution, parameters and
    multipliers, bit for bit; before initialize() it returns None."""
    import torch
    assert cm.CentroidalMPC(batch=4).get_feedback_gain() is None
    cfg, P, X0 = cm.synthetic.config3_external_push(16)
    N, L = cfg.N, cm.Layout(cfg.N)
    from cmpc_amd.synthetic import _walking_lists
    mpc = cm.CentroidalMPC(batch=16)
    assert mpc.initialize(cfg), mpc.last_error
    st = P[:, L.p_com0:L.p_com0 + 9]
    wrench = np.zeros((16, N, 6), np.float32)
    wrench[:, :, :3] = P[:, L.p_fext:L.p_fext + 3 * N].reshape(16, N, 3)
    assert mpc.set_state(st[:, 0:3], st[:, 3:6], st[:, 6:9], wrench)
    assert mpc.set_reference_trajectory(P[:, L.p_comref:L.p_comref + 3 * (N + 1)], P[:, L.p_href:L.p_href + 3 * (N + 1)])
    assert mpc.set_contact_phase_list(_walking_lists(cfg, 6, 8))
    assert mpc.set_multiplier_output()
    assert mpc.advance(), mpc.last_error
    G = mpc.get_feedback_gain()
    assert G is not None and G.shape == (16, 24, 9) and (mpc.get_feedback_gain_info()[:, 0] == 0).all()
    X, _ = mpc.get_solution()
    Ph = np.empty((16, L.np), np.float32)
    assert cm._capi.lib().cmpc_get_parameters(mpc._h, Ph.ctypes.data) == 0
    lam = mpc.get_multipliers()
    Gd, _ = mpc._solver.feedback_gain_device(*(torch.from_numpy(a).cuda() for a in (X, Ph, lam)))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(G, Gd.cpu().numpy())
    assert np.abs(G).max() > 0


def test_sub_batches_beyond_the_workspace_are_bit_identical():
    """B = 1100 > CMPC_SENS_SUB_BATCH: the launch at b0 = 1024 gives problem 1090 the same bits as a batch of one (and problem 3 likewise)."""
    import torch
    cfg, P, X0 = cm.synthetic.config2_perturbed_com(1100, seed=570)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    L = cm.Layout(cfg.N)
    dirs = torch.zeros((1100, 2, L.np), dtype=torch.float32, device=dP.device)
    dirs[:, 0, L.p_com0] = 1.0
    dirs[:, 1, L.p_href + 7] = 1.0
    a, sa = s.solution_jvp_device(dX, dP, lam, dirs)
    s1 = cm.BatchSolver(cfg, 1)
    for b in (3, 1090):
        a1, s1s = s1.solution_jvp_device(dX[b:b + 1].contiguous(), dP[b:b + 1].contiguous(), lam[b:b + 1].contiguous(), dirs[b:b + 1].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(a1[0], a[b]) and torch.equal(s1s[0], sa[b])
    assert (sa[:, 0] == 0).all()


@pytest.mark.parametrize("which", ["gamma", "held", "nominal"])
def test_subset_rule_agrees_with_the_solver(which):
    """The sensitivity kernel's restatement of the subset rule flags exactly the inputs the solver returns with status 3 (the solve kernel is not
    changed, so the rule is stated twice; this holds the two together)."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(8, seed=580)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    P32[2] = parity.break_subset(cfg.N, P32[2], which)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    L = cm.Layout(cfg.N)
    dirs = torch.zeros((8, 1, L.np), dtype=torch.float32, device=dP.device)
    dirs[:, 0, L.p_com0] = 1.0
    _, sj = s.solution_jvp_device(dX, dP, lam, dirs)
    torch.cuda.synchronize()
    st_solve, st_sens = dI[:, 5].cpu().numpy(), sj[:, 0].cpu().numpy()
    assert st_solve[2] == 3 and st_sens[2] == 3
    assert ((st_solve == 3) == (st_sens == 3)).all()
