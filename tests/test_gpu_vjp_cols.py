"""GPU: the cotangent-column VJP (include/cmpc.h, cmpc_solution_vjp_cols_device; BatchSolver.solution_vjp_cols_device / policy_jacobian_device): every
column held to the single-column entry bit for bit (whatever k and the column's chunk), to the float64 restatement tests/sens_ref.py, to the JVP through
the adjoint identity, at both ends of the horizon range, under flags, across sub-batches, and as the policy Jacobian.

Limits: REF, ADJ and RESID of tests/test_gpu_sensitivity.py.  Measured on MI355X (this file's batches): kernel against sens_ref 1.5e-7 (N = 10) and
7.0e-8 (N = 13), residual 5.3e-9, adjoint identity 2.5e-5 entry by entry, policy Jacobian against the feedback gain 2.1e-8, its rows against sens_ref
3.7e-8 ("Cotangent columns")."""
import dataclasses

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity, sens_ref
from tests.test_gpu_sensitivity import ADJ, REF, RESID, _dirs, _solve

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 9, 17)   # one column, a partial chunk, a full chunk, and the two chunk boundaries
N_DS = 3                # problems 0..2: double support over the whole horizon; 3..5: walking


def _models(cfg, B, seed):
    """one model per problem: friction, weights and corners randomised (problem 1: low friction under a strong push, so that a friction row is loaded)"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        s = rng.uniform(0.85, 1.15)
        contacts = [dataclasses.replace(c, corners=[tuple(s * v for v in cn) for cn in c.corners]) for c in cfg.contacts]
        out.append(dataclasses.replace(cfg, static_friction_coefficient=0.2 if b == 1 else float(rng.uniform(0.3, 0.9)), contacts=contacts,
                                       com_weight=tuple(float(w * rng.uniform(0.7, 1.4)) for w in cfg.com_weight),
                                       contact_force_symmetry_weight=float(cfg.contact_force_symmetry_weight * rng.uniform(0.5, 1.5)),
                                       angular_momentum_weight=float(cfg.angular_momentum_weight * rng.uniform(0.7, 1.4))))
    return out


def _problems(N, dt, n_ds, n_walk, seed):
    """n_ds double-support problems (perturbed state; problem 1 under a lateral push over the first three stages) and n_walk walking problems (the left
    foot lifts at knot N // 3 and lands N // 3 knots later, inside the horizon; a push)"""
    cfg = cm.config.ergocub_gazebo_v1(N, dt)
    L = cm.Layout(N)
    _, Pd, _ = cm.synthetic.config2_perturbed_com(n_ds, N=N, seed=seed)   # (p does not hold dt: the standing schedule is the same at either)
    if n_ds > 1:
        for k in range(3):
            Pd[1, L.p_fext + 3 * k + 1] = 150.0 / cm.synthetic.ROBOT_MASS
    _, Pw, _ = cm.synthetic.walking_push(cfg, n_walk, 50.0, 3, seed + 1)
    P = np.concatenate([Pd, Pw])
    return cfg, P.astype(np.float32), cm.layout.cold_start(N, P).astype(np.float32)


def _cotangents(cfg, P32, k, seed):
    """random float32 cotangents; in the double-support problems every column gets a deliberate component along the internal-force direction"""
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((P32.shape[0], k, L.nx)).astype(np.float32)
    for b in range(P32.shape[0]):
        n = parity._internal_force_direction(L, P32[b].astype(np.float64))
        if n is not None:
            V[b] += (rng.uniform(2.0, 6.0, (k, 1)) * n[None]).astype(np.float32)
    return V


_shared = {}


def _batch():
    """The batch of tests 1, 2, 3, 5 and 7: solved once, the 17 single-column calls made once, shared and left unchanged."""
    if not _shared:
        import torch
        cfg, P32, X032 = _problems(10, 0.06, N_DS, 3, 610)
        models = _models(cfg, 6, 611)
        s, dP, dX, dI, lam = _solve(cfg, P32, X032, models=models)
        assert (dI[:, 5] == 0).all(), dI[:, 5]
        L = cm.Layout(cfg.N)
        V = torch.from_numpy(_cotangents(cfg, P32, max(KS), 612)).cuda()
        single = []
        for j in range(max(KS)):
            gR, gM, gP, sn = s.solution_vjp_rot_device(dX, dP, lam, V[:, j].contiguous())
            single.append((gP, gM, gR, sn))
        torch.cuda.synchronize()
        sn = torch.stack([t[3] for t in single])
        assert (sn[:, :, 0] == 0).all(), sn[:, :, 0]
        assert (sn[0, :N_DS, 4] == 1).all() and (sn[0, N_DS:, 4] == 0).all(), sn[0, :, 4]
        # a loaded friction row in a double-support problem: a multiplier well above the barrier's level on a stance corner's face
        Lm = lam.cpu().numpy()
        fric = np.concatenate([np.arange(15 + 15 * cfg.N + c * 19 * cfg.N + 3 * cfg.N, 15 + 15 * cfg.N + (c + 1) * 19 * cfg.N) for c in range(2)])
        loaded = Lm[:N_DS][:, fric].max(axis=1)
        print(f"\nlargest friction multiplier of the double-support problems {loaded}, largest Sigma {sn[0, :, 3].cpu().numpy()}")
        assert loaded.max() > 1e-1, loaded
        _shared.update(cfg=cfg, P32=P32, models=models, s=s, dP=dP, dX=dX, lam=lam, L=L, V=V, single=single)
    return _shared


def _equal_to_singles(out, single, k, what=""):
    """columns 0 .. k-1 of (gP, gM, gR, sens) against the single calls: outputs in every bit; sens words 0, 2, 3, 4, 5 the single call's, 1 and 6 the
    largest over the single calls"""
    import torch
    gP, gM, gR, sn = out
    for j in range(k):
        for a, b, name in zip((gP, gM, gR), single[j][:3], ("dGradP", "dGradModel", "dGradRot")):
            assert torch.equal(a[:, j], b), (what, name, k, j)
    st = torch.stack([single[j][3] for j in range(k)])
    for w in (0, 2, 3, 4, 5):
        assert torch.equal(sn[:, w], st[0, :, w]), (what, "sens", w, k)
    for w in (1, 6):
        assert torch.equal(sn[:, w], st[:, :, w].max(dim=0).values), (what, "sens", w, k, sn[:, w], st[:, :, w].max(dim=0).values)
    assert (sn[:, 7:] == 0).all()


@pytest.mark.parametrize("k", KS)
def test_columns_are_the_single_calls_to_the_bit(k):
    import torch
    d = _batch()
    out = d["s"].solution_vjp_cols_device(d["dX"], d["dP"], d["lam"], d["V"][:, :k].contiguous(), grad_model=True, grad_rot=True)
    torch.cuda.synchronize()
    assert tuple(out[0].shape) == (6, k, d["L"].np) and tuple(out[1].shape) == (6, k, 34) and tuple(out[2].shape) == (6, k, 2, 10, 3)
    _equal_to_singles(out, d["single"], k)
    assert float(out[0].abs().max()) > 0 and float(out[1].abs().max()) > 0 and float(out[2].abs().max()) > 0
    # an output that is not requested does not change the others
    only_p = d["s"].solution_vjp_cols_device(d["dX"], d["dP"], d["lam"], d["V"][:, :k].contiguous())
    torch.cuda.synchronize()
    assert only_p[1] is None and only_p[2] is None and torch.equal(only_p[0], out[0])


def _against_sens_ref(cfgs, X, P32, Lm, V, GP):
    worst = 0.0
    for b in range(P32.shape[0]):
        S = sens_ref.Sens(cfgs[b], X[b].astype(np.float64), P32[b].astype(np.float64), Lm[b].astype(np.float64))
        cov = sens_ref.covered_mask(cfgs[b].N)
        for j in range(V.shape[1]):
            gr = S.vjp(V[b, j].astype(np.float64))
            worst = max(worst, np.abs((GP[b, j] - gr) * cov).max() / np.abs(gr).max())
    return worst


def test_every_column_matches_the_float64_restatement():
    """k = 9: every column of dGradP against SensRef.vjp at the same float32 (x, p, lam_g) and the problem's own model"""
    import torch
    d = _batch()
    gP, _, _, sn = d["s"].solution_vjp_cols_device(d["dX"], d["dP"], d["lam"], d["V"][:, :9].contiguous())
    torch.cuda.synchronize()
    sn = sn.cpu().numpy()
    assert (sn[:, 0] == 0).all()
    worst = _against_sens_ref(d["models"], d["dX"].cpu().numpy(), d["P32"], d["lam"].cpu().numpy(), d["V"][:, :9].cpu().numpy(), gP.cpu().numpy())
    print(f"\nN = 10: columns vs sens_ref {worst:.1e}, residual {sn[:, 1].max():.1e}")
    assert worst <= REF and sn[:, 1].max() <= RESID


def test_every_column_matches_the_float64_restatement_at_thirteen_knots():
    """the same at N = 13, dt = 0.1 (ergoCubSN000's horizon), B = 4: two double-support and two walking problems"""
    import torch
    cfg, P32, X032 = _problems(13, 0.1, 2, 2, 620)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    assert (dI[:, 5] == 0).all(), dI[:, 5]
    V = _cotangents(cfg, P32, 9, 621)
    gP, _, _, sn = s.solution_vjp_cols_device(dX, dP, lam, torch.from_numpy(V).cuda())
    torch.cuda.synchronize()
    sn = sn.cpu().numpy()
    assert (sn[:, 0] == 0).all(), sn[:, 0]
    worst = _against_sens_ref([cfg] * 4, dX.cpu().numpy(), P32, lam.cpu().numpy(), V, gP.cpu().numpy())
    print(f"\nN = 13: columns vs sens_ref {worst:.1e}, residual {sn[:, 1].max():.1e}")
    assert worst <= REF and sn[:, 1].max() <= RESID


def test_adjoint_identity_with_both_halves_in_columns():
    """U[B, 9, n_p] through the JVP, V[B, 9, n_x] through the cotangent columns: <V_i, J U_j> against <J^T V_i, U_j>, entry by entry"""
    import torch
    d = _batch()
    L, B = d["L"], 6
    rng = np.random.default_rng(7)
    Lm = d["lam"].cpu().numpy()
    U = np.zeros((B, 9, L.np), np.float32)
    U[:, :8] = _dirs(d["cfg"], d["P32"][0], Lm[0])[:8]
    U[:, 8] = (rng.standard_normal((B, L.np)) * 1e-2 * sens_ref.covered_mask(10)).astype(np.float32)
    DX, sj = d["s"].solution_jvp_device(d["dX"], d["dP"], d["lam"], torch.from_numpy(U).cuda())
    GP, _, _, sv = d["s"].solution_vjp_cols_device(d["dX"], d["dP"], d["lam"], d["V"][:, :9].contiguous())
    torch.cuda.synchronize()
    assert (sj[:, 0] == 0).all() and (sv[:, 0] == 0).all()
    V, DX, GP = d["V"][:, :9].cpu().numpy().astype(np.float64), DX.cpu().numpy().astype(np.float64), GP.cpu().numpy().astype(np.float64)
    lhs = np.einsum("bix,bjx->bij", V, DX)
    rhs = np.einsum("bip,bjp->bij", GP, U.astype(np.float64))
    gap = np.abs(lhs - rhs) / np.maximum(np.maximum(np.abs(lhs), np.abs(rhs)), 1e-6)
    print(f"\nadjoint identity, 9 x 9 per problem: worst {gap.max():.1e}")
    assert gap.max() <= ADJ, gap.max()


@pytest.mark.parametrize("family,key", [("push_short", (2, (1, 1))), ("push_long", 40)], ids=["N2", "N40"])
def test_both_ends_of_the_accepted_horizon(family, key):
    """B = 2, k = 8 (the full LDS image) at N = 2 and N = 40: the launch succeeds, status 0, columns bit-equal to the single calls"""
    import torch
    from tests.test_gpu_horizon_ends import batch
    cfg, P, X0 = batch(family, key)
    P32, X032 = P[:2].astype(np.float32), X0[:2].astype(np.float32)
    s, dP, dX, dI, lam = _solve(cfg, P32, X032)
    V = torch.from_numpy(_cotangents(cfg, P32, 8, 630 + cfg.N)).cuda()
    out = s.solution_vjp_cols_device(dX, dP, lam, V, grad_model=True, grad_rot=True)
    single = []
    for j in range(8):
        gR, gM, gP, sn = s.solution_vjp_rot_device(dX, dP, lam, V[:, j].contiguous())
        single.append((gP, gM, gR, sn))
    torch.cuda.synchronize()
    assert (out[3][:, 0] == 0).all(), out[3][:, 0]
    _equal_to_singles(out, single, 8, what=f"N = {cfg.N}")
    assert float(out[0].abs().max()) > 0


def test_flags_zero_every_column_and_leave_neighbours_alone():
    """k = 9, a NaN in column 5 of problem 1 only, problem 3's P outside the supported subset (a Gamma of 0.5): status 2 / status 3 and exact zeros in all
    nine columns of all three outputs; every other problem bit-equal to the clean call"""
    import torch
    d = _batch()
    L = d["L"]
    V = d["V"][:, :9].contiguous()
    clean = d["s"].solution_vjp_cols_device(d["dX"], d["dP"], d["lam"], V, grad_model=True, grad_rot=True)
    Vb = V.clone()
    Vb[1, 5, L.f[0][2] + 4] = float("nan")
    Pb = d["dP"].clone()
    Pb[3] = torch.from_numpy(parity.break_subset(10, d["P32"][3], "gamma")).cuda()
    bad = d["s"].solution_vjp_cols_device(d["dX"], Pb, d["lam"], Vb, grad_model=True, grad_rot=True)
    torch.cuda.synchronize()
    assert (clean[3][:, 0] == 0).all()
    assert bad[3][1, 0].item() == 2 and bad[3][3, 0].item() == 3
    for t in bad[:3]:
        assert (t[1] == 0).all() and (t[3] == 0).all()
    assert (bad[3][[1, 3], 1] == 0).all() and (bad[3][[1, 3], 6] == 0).all()
    keep = [0, 2, 4, 5]
    for a, b in zip(bad, clean):
        assert torch.equal(a[keep], b[keep])


def test_sub_batches_and_batch_position():
    """B = 1026 (CMPC_SENS_SUB_BATCH + 2) at k = 2, four distinct problems repeated: copies of a problem agree in every bit wherever they sit, so problems
    1024 and 1025 (the second launch) equal problems 0 and 1"""
    import torch
    d = _batch()
    B, pick = 1026, [0, 1, 3, 4]
    rep = torch.as_tensor(np.array(pick)[np.arange(B) % 4], device=d["dP"].device)
    s = cm.BatchSolver(d["cfg"], B)
    s.set_models([d["models"][pick[b % 4]] for b in range(B)])
    X, P, Lm, V = (t[rep].contiguous() for t in (d["dX"], d["dP"], d["lam"], d["V"][:, 7:9]))
    out = s.solution_vjp_cols_device(X, P, Lm, V, grad_model=True, grad_rot=True)
    torch.cuda.synchronize()
    assert (out[3][:, 0] == 0).all()
    for t in out:
        assert torch.equal(t, t[:4].repeat((B + 3) // 4, *([1] * (t.dim() - 1)))[:B])
        assert torch.equal(t[1024:], t[:2])
    # and they are the columns of the six-problem batch: columns 7 and 8 there (the last of a chunk and the first of the next), 0 and 1 here
    for j in range(2):
        for a, b in zip(out[:3], d["single"][7 + j][:3]):
            assert torch.equal(a[:4, j], b[pick])


def test_policy_jacobian():
    """the 24 first-knot forces in all parameters from one call: columns com0 .. h0 against feedback_gain_device (the transposed route to the same block),
    two rows against SensRef.vjp, and the model block of one row against solution_vjp_model_device on that unit cotangent, bit for bit"""
    import torch
    d = _batch()
    L, s = d["L"], d["s"]
    Jp, Jm, Jr, sn = s.policy_jacobian_device(d["dX"], d["dP"], d["lam"], model=True)
    G, sg = s.feedback_gain_device(d["dX"], d["dP"], d["lam"])
    torch.cuda.synchronize()
    assert tuple(Jp.shape) == (6, 24, L.np) and tuple(Jm.shape) == (6, 24, 34) and Jr is None
    assert (sn[:, 0] == 0).all() and (sg[:, 0] == 0).all()
    Jp_h, G_h = Jp.cpu().numpy().astype(np.float64), G.cpu().numpy().astype(np.float64)
    gap = max(np.abs(Jp_h[b, :, L.p_com0:L.p_com0 + 9] - G_h[b]).max() / np.abs(G_h[b]).max() for b in range(N_DS))
    rows = np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)])
    X, Lm = d["dX"].cpu().numpy(), d["lam"].cpu().numpy()
    worst = 0.0
    for b, r in ((0, 2), (1, 13)):
        S = sens_ref.Sens(d["models"][b], X[b].astype(np.float64), d["P32"][b].astype(np.float64), Lm[b].astype(np.float64))
        e = np.zeros(L.nx)
        e[rows[r]] = 1.0
        gr = S.vjp(e)
        worst = max(worst, np.abs((Jp_h[b, r] - gr) * sens_ref.covered_mask(10)).max() / np.abs(gr).max())
    print(f"\npolicy Jacobian: against the feedback gain {gap:.1e}, rows against sens_ref {worst:.1e}")
    assert gap <= ADJ and worst <= REF
    e = torch.zeros((6, L.nx), dtype=torch.float32, device=Jp.device)
    e[:, int(rows[17])] = 1.0
    gM, gP, _ = s.solution_vjp_model_device(d["dX"], d["dP"], d["lam"], e)
    torch.cuda.synchronize()
    assert torch.equal(Jm[:, 17], gM) and torch.equal(Jp[:, 17], gP)
    # rows given by the caller, the rotation block with them
    Jp2, _, Jr2, _ = s.policy_jacobian_device(d["dX"], d["dP"], d["lam"], rows=rows[[17, 2]], rot=True)
    torch.cuda.synchronize()
    assert tuple(Jr2.shape) == (6, 2, 2, 10, 3) and torch.equal(Jp2[:, 0], Jp[:, 17]) and torch.equal(Jp2[:, 1], Jp[:, 2])
