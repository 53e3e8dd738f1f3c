"""Host checks of the solution-sensitivity definition of include/cmpc.h through its float64 dense restatement tests/sens_ref.py: JVP against central
differences of the float64 oracle's x*(p), the adjoint identity, the internal-force convention, and the dependence on the slack floor.  No GPU:
tests/test_gpu_sensitivity.py holds the device kernels to sens_ref."""
import os

import numpy as np
import pytest

import cmpc_amd as cm
from tests import sens_ref
from tests.test_multipliers_cpu import golden_cfg, map_record, record_from_lam

# (golden, problems).  The finite differences come from the float64 oracle converged to mu 1e-12 (tol 1e-11), and sens_ref is taken with a slack
# floor of 1e-12 to match it: at the default floor (5e-8) an active row's Sigma is capped at z / s_min, which biases the derivative along that row by
# about curvature x s_min / z (1.2e-4 on cfg5 problem 0's lower box row, curvature ~400, z ~0.1).  Measured worst relative gap:
# cfg2 5.6e-7 (currentPos), cfg5 problems 0 and 2 3.1e-6 (hRef; no weakly active row of a loaded foot), yaw 4 6.7e-6 (upper box; one weakly active
# row, within the tight bound).  push 0 has 2 (a loaded corner at the apex of its pyramid): its kink is loaded, and the barrier value lies between the
# one-sided slopes (8.1e-4).
CASES = [("cfg2", None, (0, 1)), ("cfg5", None, (0, 2)), ("yaw", "tmp", (4,)), ("push", "tmp", (0,))]
FD_CLEAN = 2e-5    # problems without weakly active rows of loaded feet (swing stages, landing offsets, box Sigma, active friction rows)
FD_WEAK = 2e-3     # problems with them: the barrier derivative lies between the one-sided slopes of a kink
S_FD = 1e-12       # slack floor of the comparison


def _load(name, which, b, golden_dir):
    d = np.load(os.path.join(golden_dir, f"argmin_ref_{name}_{which}.npz" if which else f"argmin_{name}.npz"))
    cfg = golden_cfg(name, which)
    x, p, lam = (d[k][b].astype(np.float64) for k in ("x_star", "P", "lam_g"))
    lam = map_record(cfg, x, p, *record_from_lam(cfg, x, p, lam))   # (the convention of cmpc_get_multipliers_device)
    return cfg, x, p, lam


@pytest.mark.parametrize("name,which,problems", CASES)
def test_jvp_matches_oracle_finite_differences(name, which, problems, golden_dir):
    from oracle import oracle_lib as ol, problem_nlp
    worst = {}
    weak = 0
    for b in problems:
        cfg, x, p, lam = _load(name, which, b, golden_dir)
        S = sens_ref.Sens(cfg, x, p, lam, s_min=S_FD)
        weak += S.weak > 0
        oc = problem_nlp.oracle_cfg(cfg)
        dirs = sens_ref.directions(cfg, p, lam)
        kinds = {k for k, _ in dirs}
        assert {"com0", "dcom0", "h0", "comRef", "hRef", "fExt", "tauExt", "nominalPos"} <= kinds
        h = 1e-5
        # (double support throughout, cfg2: no inequality row is active and the floor plays no part; the deeper barrier only adds
        # ill-conditioning along the internal-force direction, so its oracle stops at mu 1e-10)
        opts = ol.ipm_opts(tol=1e-9, mu_min=1e-10) if S.n is not None else ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200)
        Pp = np.concatenate([np.stack([p + h * d for _, d in dirs]), np.stack([p - h * d for _, d in dirs])])
        Xs, info = ol.ref_solve_batch(oc, Pp, np.repeat(x[None], Pp.shape[0], 0), opts, nthreads=8)
        assert (info[:, 5] == 0).all()
        for i, (kind, d) in enumerate(dirs):
            fd = (Xs[i] - Xs[len(dirs) + i]) / (2 * h)
            if S.n is not None:
                fd = fd - S.n * (S.n @ fd)
            dx = S.jvp(d)
            gap = np.abs(dx - fd).max() / max(np.abs(fd).max(), 1e-3)
            worst[kind] = max(worst.get(kind, 0.0), gap)
            assert gap <= (FD_WEAK if S.weak else FD_CLEAN), (name, b, kind, gap, S.weak)
    if name == "cfg5":
        assert weak == 0        # (walking problems held to the tight bound: swing stages, landing offsets, box rows)
    print(f"\n{name}: problems with weakly active rows of loaded feet {weak} of {len(problems)}; gap " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("name,which,b", [("cfg2", None, 0), ("cfg5", None, 0), ("yaw", "tmp", 4)])
def test_adjoint_identity(name, which, b, golden_dir):
    """<v, J u> = <J^T v, u> to 1e-10 relative (u in the covered parameters, v arbitrary)"""
    cfg, x, p, lam = _load(name, which, b, golden_dir)
    S = sens_ref.Sens(cfg, x, p, lam)
    rng = np.random.default_rng(11)
    u = rng.standard_normal(p.size) * sens_ref.covered_mask(cfg.N) * 1e-2
    v = rng.standard_normal(x.size)
    a, g = float(v @ S.jvp(u)), S.vjp(v)
    bb = float(g @ u)
    assert abs(a - bb) <= 1e-10 * max(abs(a), abs(bb)), (a, bb)


def test_config2_jvp_has_no_internal_force_component(golden_dir):
    cfg, x, p, lam = _load("cfg2", None, 0, golden_dir)
    S = sens_ref.Sens(cfg, x, p, lam)
    assert S.n is not None
    for _, d in sens_ref.directions(cfg, p, lam):
        dx = S.jvp(d)
        assert abs(S.n @ dx) <= 1e-12 * max(1.0, np.abs(dx).max())


@pytest.mark.parametrize("name,which,b,bound", [("cfg2", None, 0, 1e-6), ("cfg2", None, 1, 1e-6), ("cfg5", None, 0, 1e-3)])
def test_doubling_s_min_moves_little(name, which, b, bound, golden_dir):
    """The slack floor only reaches rows whose slack is below it, i.e. active rows with Sigma ~ z / s_min >> every curvature: doubling it moves the
    derivatives of non-degenerate problems by < 1e-6 relative (measured 0 on cfg2 0 and 1).  cfg5 problem 0, whose swing-foot corners sit at the
    apex of their pyramids (weakly active rows), moves by 1.2e-4: the floor decides where between the one-sided slopes such a row's derivative lies."""
    cfg, x, p, lam = _load(name, which, b, golden_dir)
    S1 = sens_ref.Sens(cfg, x, p, lam)
    S2 = sens_ref.Sens(cfg, x, p, lam, s_min=2 * sens_ref.S_MIN)
    worst = 0.0
    for _, d in sens_ref.directions(cfg, p, lam):
        a, c = S1.jvp(d), S2.jvp(d)
        worst = max(worst, np.abs(a - c).max() / max(np.abs(a).max(), 1e-3))
    print(f"\n{name} {b}: s_min doubled moves the JVP by {worst:.1e}")
    assert worst <= bound
