"""Host checks of the model directions of include/cmpc.h through their float64 dense restatement tests/sens_model_ref.py: the JVP in theta against
central differences of the float64 oracle's x*(theta), the adjoint identity, dV*/dtheta against central differences of the oracle's optimal cost, the
internal-force rule and its reported size, and the field order of cmpc_model against the oracle's NlpCfg.  No GPU: tests/test_gpu_model_sensitivity.py
holds the device kernels to sens_model_ref."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import sens_model_ref as smr
from tests.test_sensitivity_cpu import CASES, FD_CLEAN, FD_WEAK, S_FD, _load

# (the goldens and the FD_CLEAN / FD_WEAK rule of tests/test_sensitivity_cpu.py; a model field is moved by H_REL of its size, at least H_MIN)
H_REL, H_MIN = 1e-5, 1e-6
# A direction whose right-hand side has a component along the internal-force direction n above this relative size has no derivative (include/cmpc.h,
# the internal-force rule): the oracle's differences along it measure a jump of the undetermined internal force, not a slope.  Measured on the
# goldens: cfg2 friction 4.4e-3 and 4.4e-4, push 0 friction 0.2 and one-foot corners 2e-2 (excluded); every other direction <= 5e-9 (held).
NO_DERIVATIVE = 1e-6
# The symmetry and force-rate weights act on every corner force directly, swing feet's included, whose corners sit at the apex of their pyramids
# (weakly active rows of swing feet, dSens[5]): for those two fields such rows are kinks of the map like the loaded ones.  Measured on cfg5 problem 0
# (200 such rows): force_rate_x 2.3e-5, symmetry 1.7e-5, independent of the step and of the oracle's barrier floor; every other field <= 1.4e-6.
SWING_FIELDS = ("symmetry", "force_rate_x", "force_rate_y", "force_rate_z")


def _fd_solves(cfg, x, p, theta, dirs, opts, f_only=False):
    """central differences of the oracle's x* (and optimal cost) along each model direction, from the returned x"""
    from oracle import oracle_lib as ol
    out = []
    for _, d in dirs:
        h = max(H_REL * float(np.abs(theta[d != 0]).max()), H_MIN)
        sides = []
        for s in (1.0, -1.0):
            oc = smr.nlp_cfg(cfg, theta + s * h * d)
            X, info = ol.ref_solve_batch(oc, p[None], x[None], opts)
            assert (info[:, 5] == 0).all()
            f, _ = ol.nlp_fg(oc, X[0], p)
            sides.append((X[0], f))
        out.append(((sides[0][0] - sides[1][0]) / (2 * h), (sides[0][1] - sides[1][1]) / (2 * h)))
    return out


@pytest.mark.parametrize("name,which,problems", CASES)
def test_model_jvp_matches_oracle_finite_differences(name, which, problems, golden_dir):
    from oracle import oracle_lib as ol
    worst, excluded = {}, []
    for b in problems:
        cfg, x, p, lam = _load(name, which, b, golden_dir)
        MS = smr.ModelSens(cfg, x, p, lam, s_min=S_FD)
        dirs = smr.model_directions(cfg)
        assert {k for k, _ in dirs} >= {"friction", "com_weight_z", "symmetry", "force_rate_x", "corner_left", "corner_right", "corner_mirrored"}
        opts = ol.ipm_opts(tol=1e-9, mu_min=1e-10) if MS.n is not None else ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200)
        for (kind, d), (fd, _) in zip(dirs, _fd_solves(cfg, x, p, MS.theta, dirs, opts)):
            if MS.n is not None:
                if MS.removed(d) > NO_DERIVATIVE:
                    excluded.append(f"{b}:{kind}")
                    continue
                fd = fd - MS.n * (MS.n @ fd)
            dx = MS.jvp(d)
            gap = np.abs(dx - fd).max() / max(np.abs(fd).max(), 1e-3)
            worst[kind] = max(worst.get(kind, 0.0), gap)
            weak = MS.S.weak + (MS.S.weak_swing if kind in SWING_FIELDS else 0)
            assert gap <= (FD_WEAK if weak else FD_CLEAN), (name, b, kind, gap, MS.S.weak, MS.S.weak_swing)
    print(f"\n{name}: gap " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f"; no derivative: {excluded}")
    assert len(worst) >= {"cfg2": 12, "push": 10}.get(name, 13)   # (cfg2: friction, push 0: friction and one-foot corners have no derivative)


@pytest.mark.parametrize("name,which,b", [("cfg2", None, 0), ("cfg5", None, 0), ("yaw", "tmp", 4)])
def test_model_adjoint_identity(name, which, b, golden_dir):
    """<v, J_theta u> = <J_theta^T v, u> to 1e-10 relative, and with a p direction in the same column: the p and theta parts add"""
    cfg, x, p, lam = _load(name, which, b, golden_dir)
    MS = smr.ModelSens(cfg, x, p, lam)
    rng = np.random.default_rng(12)
    u = rng.standard_normal(smr.M) * 1e-2
    v = rng.standard_normal(x.size)
    a, g = float(v @ MS.jvp(u)), MS.vjp(v)
    bb = float(g @ u)
    assert abs(a - bb) <= 1e-10 * max(abs(a), abs(bb)), (a, bb)
    from tests import sens_ref
    dp = rng.standard_normal(p.size) * sens_ref.covered_mask(cfg.N) * 1e-2
    both = MS.jvp(u, dp)
    np.testing.assert_allclose(both, MS.jvp(u) + MS.S.jvp(dp), rtol=0, atol=1e-9 * np.abs(both).max())


@pytest.mark.parametrize("name,which,b", [("cfg2", None, 0), ("cfg5", None, 0), ("yaw", "tmp", 4), ("push", "tmp", 0)])
def test_model_value_gradient_matches_oracle_finite_differences(name, which, b, golden_dir):
    """dV*/dtheta (envelope theorem at the golden's (x, lam)) against central differences of the oracle's optimal cost, every direction of
    model_directions; relative to the largest entry (the weights' entries are the cost terms themselves, ~1e0..1e2).  Measured: 3e-7."""
    from oracle import oracle_lib as ol
    cfg, x, p, lam = _load(name, which, b, golden_dir)
    MS = smr.ModelSens(cfg, x, p, lam)
    vg = MS.value_gradient()
    dirs = smr.model_directions(cfg)
    opts = ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200)
    fds = _fd_solves(cfg, x, p, MS.theta, dirs, opts)
    scale = max(abs(fv) for _, fv in fds)
    worst = 0.0
    for (kind, d), (_, fv) in zip(dirs, fds):
        worst = max(worst, abs(vg @ d - fv) / scale)
    print(f"\n{name} {b}: dV*/dtheta against oracle differences {worst:.1e} (scale {scale:.1e})")
    assert worst <= 1e-5, worst


def test_internal_force_rule_on_double_support(golden_dir):
    """cfg2 (both feet in stance over the whole horizon): the removed component |n^T r_x| / |r_x| is at rounding level for the weights and for a
    mirrored corner pair; friction leaves a small one through the Sigma of its rows (measured 1.7e-5 .. 3.4e-2 over the 8 problems).  A one-foot
    corner direction leaves only lam_h-weighted moments sum_k lam_h,k . (R e_b x e): at an optimum those vanish up to the solve's tolerance
    (measured <= 1e-8) because the couples that the internal force can exert about x and z are free in the cost while no friction
    row is loaded.  The JVP has no
    component along n whatever the direction."""
    worst = {}
    for b in range(8):
        cfg, x, p, lam = _load("cfg2", None, b, golden_dir)
        MS = smr.ModelSens(cfg, x, p, lam)
        assert MS.n is not None
        for kind, d in smr.model_directions(cfg):
            worst[kind] = max(worst.get(kind, 0.0), MS.removed(d))
            dx = MS.jvp(d)
            assert abs(MS.n @ dx) <= 1e-12 * max(1.0, np.abs(dx).max())
        if b == 0:
            assert MS.removed(np.eye(smr.M)[0]) > 1e-4        # friction: measurable on problem 0 (4.4e-3)
    print("\ncfg2 removed: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k in ("com_weight_x", "com_weight_y", "com_weight_z", "angular_momentum", "contact_position", "force_rate_x", "force_rate_y",
              "force_rate_z", "symmetry", "corner_mirrored"):
        assert worst[k] <= 1e-12, (k, worst[k])
    assert worst["corner_left"] <= 1e-7 and worst["corner_right"] <= 1e-7
    assert 1e-4 < worst["friction"] < 0.1
    # push problem 0 is in double support throughout too, with loaded friction rows: there the couples are not free and a one-foot corner direction
    # leaves a clearly nonzero component (measured 2.2e-2), the mirrored pair none
    cfg, x, p, lam = _load("push", "tmp", 0, golden_dir)
    MS = smr.ModelSens(cfg, x, p, lam)
    rem = {k: MS.removed(d) for k, d in smr.model_directions(cfg)}
    print("push 0 removed: " + " ".join(f"{k} {v:.1e}" for k, v in rem.items()))
    assert MS.n is not None and rem["corner_left"] > 1e-3 and rem["corner_right"] > 1e-3 and rem["corner_mirrored"] <= 1e-12
    assert MS.removed_vjp() >= max(rem.values()) - 1e-15
    # off double support there is no internal-force direction and nothing is removed
    cfg, x, p, lam = _load("cfg5", None, 0, golden_dir)
    MS = smr.ModelSens(cfg, x, p, lam)
    assert MS.n is None and MS.removed_vjp() == 0.0


def test_model_field_order_matches_the_oracle():
    """cmpc_model's packed order (config.model_row) maps onto the oracle's NlpCfg field by field, and back through cfg_with_model"""
    cfg = cm.config.ergocub_gazebo_v1()
    th = cm.config.model_row(cfg) + np.arange(smr.M) * 1e-3   # (distinct values)
    oc = smr.nlp_cfg(cfg, th)
    assert oc.mu == th[0] and list(oc.w_com) == list(th[1:4]) and oc.w_h == th[4] and oc.w_pos == th[5]
    assert list(oc.w_rate) == list(th[6:9]) and oc.w_sym == th[9] and list(oc.corners) == list(th[10:34])
    np.testing.assert_array_equal(cm.config.model_row(smr.cfg_with_model(cfg, th)), th)
    from oracle import problem_nlp
    ref = problem_nlp.oracle_cfg(cfg)
    mine = smr.nlp_cfg(cfg, cm.config.model_row(cfg))
    for f, _ in ref._fields_:
        a, b = getattr(ref, f), getattr(mine, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else a == b, f
    assert smr.FIELDS[3] == "com_weight_z" and smr.corner_index(1, 3, 2) == 33 and len(smr.FIELDS) == smr.M == cm._capi.MODEL_DOUBLES
