"""GPU: the multipliers of the reference NLP from the solver's dual record (cmpc_set_multiplier_output / cmpc_get_multipliers_device), the device KKT
certificate and the gradient of the optimal cost, held in float64 on the host to the oracle's restatement of the generated code (oracle_lib.nlp_grad,
nlp_fg; problem_nlp.bounds) through tests/test_multipliers_cpu.py.

Limits: set from the worst case measured on MI355X over 5 seeds x 512 problems of configs 2, 3 and 5 (tools/gpu_multiplier_cost.py,
profiles/multiplier_output.txt) and over every golden; measured value next to each."""
import os

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity
from tests.test_multipliers_cpu import GOLDEN_REF, golden_cfg, host_kkt, unique_rows, value_gradient, zero_rows

pytestmark = pytest.mark.gpu

# KKT residuals of (returned x, exported lam) against the reference NLP, float64 on the host, worst case of every solve below.
# Measured worst over 5 seeds x 512 (profiles/multiplier_output.txt): stationarity 2.9e-6 / 6.1e-5 / 9.2e-5 (configs 2 / 3 / 5), 8.9e-4 (config 3 at
# N = 25: isolated problems with a nearly degenerate friction row in the last stages); in the solves below 1.5e-4 (N = 25, seed 108),
# 2.4e-5 (goldens).  Infeasibility 1.2e-7, complementarity 1.1e-9, sign 3.3e-14 everywhere.
STAT = 2e-4    # scaled stationarity
FEAS = 1e-6    # primal infeasibility
COMPL = 1e-8   # scaled complementarity
SIGN = 1e-12   # scaled sign violation
UNIQUE = 3e-5  # unique rows against the goldens' lam_g, relative to max(1, max|lam_g| over those rows): measured 1.2e-5 (stand), 8.1e-6 (cfg2)


def _solve(cfg, P32, X032, factors=None, models=None, warm=False, s=None):
    import torch
    B = P32.shape[0]
    if s is None:
        s = cm.BatchSolver(cfg, B, factors=factors)
        if models is not None:
            s.set_models(models)
        s.set_multiplier_output()
    dP, dX0 = torch.from_numpy(P32).cuda(), torch.from_numpy(X032).cuda()
    dX, dI = s.solve_device(dP, dX0, warm=warm)
    lam = s.multipliers_device(dX, dP)
    cert = s.kkt_certificate_device(dX, dP, lam)
    torch.cuda.synchronize()
    return s, dX.cpu().numpy(), dI.cpu().numpy(), lam.cpu().numpy(), cert.cpu().numpy()


def _kkt_all(cfgs, P32, X, info, lam, cert=None, label=""):
    worst = dict(stat=0.0, feas=0.0, compl=0.0, sign=0.0)
    for b in range(P32.shape[0]):
        assert info[b, 5] == 0, (label, b, info[b])
        cfg = cfgs[b] if isinstance(cfgs, list) else cfgs
        k = host_kkt(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), lam[b].astype(np.float64))
        for f in worst:
            worst[f] = max(worst[f], k[f])
        assert (lam[b][zero_rows(cfg.N, P32[b])] == 0).all()
        if cert is not None:
            assert cert[b, 5] == 0
    print(f"\n{label}: " + " ".join(f"{f} {v:.2e}" for f, v in worst.items()))
    assert worst["stat"] <= STAT and worst["feas"] <= FEAS and worst["compl"] <= COMPL and worst["sign"] <= SIGN, (label, worst)
    return worst


@pytest.mark.parametrize("name,which", GOLDEN_REF + [(n, None) for n in ("cfg1", "cfg2", "cfg3", "cfg5")])
def test_exported_multipliers_certify_the_returned_x_on_the_goldens(name, which, golden_dir):
    """Every golden: (x, lam) of the GPU solve is a KKT point of the reference NLP; the unique rows (init com / dcom / h, the com / dcom / h
    dynamics) agree with the goldens' lam_g; the convention's rows are exactly 0."""
    d = np.load(os.path.join(golden_dir, f"argmin_ref_{name}_{which}.npz" if which else f"argmin_{name}.npz"))
    cfg = golden_cfg(name, which)
    P32, X032 = d["P"].astype(np.float32), d["X0"].astype(np.float32)
    s, X, info, lam, cert = _solve(cfg, P32, X032)
    _kkt_all(cfg, P32, X, info, lam, cert, f"golden {name} {which}")
    u = unique_rows(cfg.N)
    worst = 0.0
    for b in range(P32.shape[0]):
        ref = d["lam_g"][b]
        # (scaled by the unique rows themselves: the goldens put thousands on duplicate box rows, which must not loosen this)
        worst = max(worst, np.abs(lam[b][u] - ref[u]).max() / max(1.0, np.abs(ref[u]).max()))
    print(f"unique rows against the golden: {worst:.2e}")
    assert worst <= UNIQUE, worst
    s.close()


@pytest.mark.parametrize("gen,N,seed,factors", [("config2_perturbed_com", 20, 101, None), ("config3_external_push", 20, 102, "lds"),
                                                 ("config3_external_push", 20, 102, "hbm"), ("config5_footstep_candidates", 30, 103, None),
                                                 ("config3_external_push", 16, 107, "lds"), ("config3_external_push", 25, 108, "hbm")])
def test_exported_multipliers_certify_fresh_seeds(gen, N, seed, factors):
    """Unseen seeds of configs 2, 3 (both kernel variants) and 5 (N = 30), and config 3 at horizons that select the runtime-N kernels (N = 16 resident,
    N = 25 HBM-factor).  The tail polish fired on 1, 1, 1 and 2 of the first four sets of 64 problems (printed)."""
    B = 64
    cfg, P, X0 = getattr(cm.synthetic, gen)(B, N=N, seed=seed)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, X, info, lam, cert = _solve(cfg, P32, X032, factors=factors)
    polished = int((info[:, 3] // 100000 % 10 > 0).sum())
    _kkt_all(cfg, P32, X, info, lam, cert, f"{gen} seed {seed} {factors} (tail polished: {polished})")
    s.close()


def test_exported_multipliers_follow_a_warm_solve():
    """A warm solve from the previous solution shifted by one knot: the record is that of the warm solve."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(64, seed=104)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, X, info, lam, cert = _solve(cfg, P32, X032)
    dX0 = torch.empty((64, cm.Layout(cfg.N).nx), dtype=torch.float32, device="cuda")
    s.shift_solution_device(torch.from_numpy(X).cuda(), dX0)
    torch.cuda.synchronize()
    _, X2, info2, lam2, cert2 = _solve(cfg, P32, dX0.cpu().numpy(), warm=True, s=s)
    _kkt_all(cfg, P32, X2, info2, lam2, cert2, "warm")
    s.close()


def test_exported_multipliers_follow_each_problems_model():
    """Per-problem models (friction, weights, corners): the certificate of each problem against its own model."""
    from tests.test_gpu_models import _base, _randomised
    B = 64
    cfgs = _randomised(B, 31)
    _, P, X0 = cm.synthetic.walking_push(_base(), B, 100.0, 3, 12)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s, X, info, lam, cert = _solve(_base(), P32, X032, models=cfgs)
    ok = np.nonzero(info[:, 5] == 0)[0]
    assert len(ok) >= B - 3
    _kkt_all([cfgs[b] for b in ok], P32[ok], X[ok], info[ok], lam[ok], cert[ok], "per-problem models")
    s.close()


def test_device_certificate_matches_the_host_and_flags_status_3():
    """The device certificate (double on the device, float32 model constants) against the float64 host computation of the same fields; a problem
    outside the supported subset comes back with zeros and status 3 in its certificate."""
    cfg, P, X0 = cm.synthetic.config3_external_push(32, seed=105)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    P32[5] = parity.break_subset(cfg.N, P32[5], "gamma")
    s, X, info, lam, cert = _solve(cfg, P32, X032)
    assert info[5, 5] == 3 and cert[5, 5] == 3 and (lam[5] == 0).all()
    worst = np.zeros(5)
    for b in range(32):
        if b == 5:
            continue
        k = host_kkt(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), lam[b].astype(np.float64))
        host = np.array([k["stat"], k["feas"], k["compl"], k["sign"], k["f"]])
        d = np.abs(cert[b, :5] - host) / np.array([1.0, 1.0, 1.0, 1.0, max(1.0, abs(k["f"]))])
        worst = np.maximum(worst, d)
        assert cert[b, 5] == 0 and abs(cert[b, 6] - k["scale"]) <= 1e-6 * k["scale"]
    print("\ncertificate device - host: " + " ".join(f"{v:.2e}" for v in worst))
    # (the device uses the model's float32 constants, the host the configuration's doubles: friction rows differ by ~1e-8 of a force).  Measured:
    # 7.9e-12 3.1e-08 6.2e-11 0 4.8e-08 here; stationarity 6.9e-09 at worst over 5 x 512 problems of configs 2, 3, 5
    assert (worst[:4] <= [5e-8, 1e-6, 1e-9, 1e-12]).all() and worst[4] <= 1e-6, worst
    s.close()


@pytest.mark.parametrize("name", ["cfg2", "cfg5"])
def test_device_value_gradient_matches_the_host_formula(name, golden_dir):
    """dV*/dp on the device at the goldens' (x*, lam*) against the float64 host formula (which tests/test_multipliers_cpu.py holds to central
    differences of the oracle's optimal cost)."""
    import torch
    d = np.load(os.path.join(golden_dir, f"argmin_{name}.npz"))
    cfg = golden_cfg(name)
    B = d["P"].shape[0]
    s = cm.BatchSolver(cfg, B)
    dX, dP, dL = (torch.from_numpy(np.ascontiguousarray(d[k], np.float32)).cuda() for k in ("x_star", "P", "lam_g"))
    gp = s.value_gradient_device(dX, dP, dL)
    torch.cuda.synchronize()
    gp = gp.cpu().numpy()
    worst = 0.0
    for b in range(B):
        ref = value_gradient(cfg, d["x_star"][b].astype(np.float32).astype(np.float64), d["P"][b].astype(np.float64),
                             d["lam_g"][b].astype(np.float32).astype(np.float64))
        worst = max(worst, np.abs(gp[b] - ref).max() / max(1.0, np.abs(ref).max()))
    print(f"\nvalue gradient device - host ({name}): {worst:.2e}")
    assert worst <= 1e-7, worst   # measured 9.1e-10 (cfg5)
    s.close()


@pytest.mark.parametrize("N,factors", [(20, "lds"), (20, "hbm"), (16, "lds"), (16, "hbm"), (25, "hbm")])
def test_output_off_leaves_x_and_info_bit_identical(N, factors):
    """A handle that turned the output on and off again, and one with the output on, return the x and info (but the shader-clock word) of a handle
    that never turned it on: the export and the dual steps touch nothing the primal iterate depends on.  Compile-time horizon (N = 20) and runtime-N
    kernels (N = 16, 25) of both variants."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(64, N=N, seed=102)   # (at N = 20 one problem of this set takes the tail polish in both variants)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    dP, dX0 = torch.from_numpy(P32).cuda(), torch.from_numpy(X032).cuda()
    s0 = cm.BatchSolver(cfg, 64, factors=factors)
    X_ref, I_ref = (t.cpu().numpy() for t in s0.solve_device(dP, dX0))
    s1 = cm.BatchSolver(cfg, 64, factors=factors)
    s1.set_multiplier_output(True)
    X_on, I_on = (t.cpu().numpy() for t in s1.solve_device(dP, dX0))
    s1.set_multiplier_output(False)
    with pytest.raises(RuntimeError):
        s1.multipliers_device(torch.from_numpy(X_on).cuda(), dP)
    X_off, I_off = (t.cpu().numpy() for t in s1.solve_device(dP, dX0))
    keep = [0, 1, 2, 3, 4, 5, 7]
    assert (I_ref[:, 5] == 0).all()
    if N == 20:
        assert int((I_ref[:, 3] // 100000 % 10 > 0).sum()) > 0   # (the tail polish is among what is held bit-identical)
    for X, I in ((X_on, I_on), (X_off, I_off)):
        np.testing.assert_array_equal(X, X_ref)
        np.testing.assert_array_equal(I[:, keep], I_ref[:, keep])
    s0.close(); s1.close()


def test_exported_multipliers_follow_a_rollout_tick():
    """cmpc_rollout_tick_device (one call per warm tick: merge, sample, setState, shift, solve, adjust, plant): the record is that of the tick's solve,
    and (x, lam) certify against the tick's own parameters."""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    B = 32
    ro = cm.rollout.WalkingRollout(cfg, B)
    ro.solver.set_multiplier_output()
    seen = {}
    tick = ro.solver.rollout_tick_device

    def spy(now, plan, prev, lists, ok, land, state, wr, dP, dX0, dX, dInfo, *a, **k):
        seen.update(dP=dP, dX=dX, dInfo=dInfo, ticks=seen.get("ticks", 0) + 1)
        return tick(now, plan, prev, lists, ok, land, state, wr, dP, dX0, dX, dInfo, *a, **k)

    ro.solver.rollout_tick_device = spy
    rng = np.random.default_rng(12)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    rec = ro.run(4, com0, rng.uniform(-0.05, 0.05, (B, 3)), np.zeros((B, 3)), record="light")
    assert all(rec["converged"]) and seen.get("ticks", 0) >= 1, (rec["converged"], seen.get("ticks"))
    lam = ro.solver.multipliers_device(seen["dX"], seen["dP"])
    cert = ro.solver.kkt_certificate_device(seen["dX"], seen["dP"], lam)
    torch.cuda.synchronize()
    P32, X, info = (t.cpu().numpy() for t in (seen["dP"], seen["dX"], seen["dInfo"]))
    _kkt_all(cfg, P32, X, info, lam.cpu().numpy(), cert.cpu().numpy(), "rollout tick")
    ro.solver.close()


def test_class_surface_returns_the_multipliers_of_advance():
    """CentroidalMPC: set_multiplier_output, advance(), get_multipliers() (cmpc_get_multipliers: the handle's own x and p, into host memory) is the
    device mapping of the same solve, bit for bit, and certifies; without the output on get_multipliers() fails and says why."""
    import torch
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
    assert mpc.advance(), mpc.last_error
    assert mpc.get_multipliers() is None and "multiplier output is off" in mpc.last_error
    assert mpc.set_multiplier_output()
    assert mpc.advance(), mpc.last_error
    lam = mpc.get_multipliers()
    X, info = mpc.get_solution()
    Ph = np.empty((16, L.np), np.float32)
    assert cm._capi.lib().cmpc_get_parameters(mpc._h, Ph.ctypes.data) == 0
    dev = mpc._solver.multipliers_device(torch.from_numpy(X).cuda(), torch.from_numpy(Ph).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(lam, dev.cpu().numpy())
    _kkt_all(cfg, Ph, X, info, lam, None, "class surface")
