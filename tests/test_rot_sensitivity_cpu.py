"""Host checks of the rotation directions of include/cmpc.h through their float64 dense restatement tests/sens_rot_ref.py: the JVP in omega against
central differences of the float64 oracle's x*(R exp(+-h [omega]x)), the adjoint identity, dV*/domega against central differences of the oracle's
optimal cost, the internal-force rule and its reported size, and the per-stage -> per-list-entry sum against the host sampler.  No GPU:
tests/test_gpu_rot_sensitivity.py holds the device kernels to sens_rot_ref."""
import ctypes
import functools

import numpy as np
import pytest

import cmpc_amd as cm
from tests import sens_ref
from tests import sens_rot_ref as srr
from tests.test_model_sensitivity_cpu import NO_DERIVATIVE
from tests.test_sensitivity_cpu import S_FD, _load

CASES = [("cfg2", None, (0, 1)), ("cfg5", None, (0, 2)), ("yaw", "tmp", (4,)), ("gait", "tmp", (3,)), ("push", "tmp", (0,))]
H = 1e-5
# Gap of the restatement's JVP to the oracle's central differences.  A rotation acts directly on the friction rows of swing feet, whose corners sit at
# the apex of their pyramids (weakly active rows, dSens[5]); there the barrier derivative is one value between the one-sided slopes and differs from
# the oracle's differences by a small ABSOLUTE amount, the same for every group of a problem that contains swing stages and independent of the step
# between 1e-4 and 1e-6 -- the effect the model directions document for the symmetry and force-rate weights.  Measured with this file:
#   groups of stance stages only, relative to max(|fd|, FLOOR): worst 8.0e-5 (cfg2 problem 0, general axis, whose whole effect is 1.06e-3; cfg2
#     z axis 5.5e-6, every walking case <= 6.3e-6)                                                                   -> STANCE = 1.6e-4
#   groups that contain swing stages, absolute: cfg5 4.0e-6 / 5.4e-6, yaw 4 1.63e-5, gait 3 1.52e-5                  -> SWING_ABS = 3e-5
#     (this is the whole gap of a group whose effect is below FLOOR, e.g. a foot in the air at the end of the horizon, |fd| ~ 2e-7)
#   the same groups where |fd| >= SWING_SIZE, relative to |fd|: worst 5.3e-4 (cfg5 0 and yaw 4)                      -> SWING = 1e-3
FLOOR = 1e-3
STANCE, SWING_ABS, SWING, SWING_SIZE = 1.6e-4, 3e-5, 1e-3, 5e-3
VG = 1e-5    # dV*/domega against differences of the optimal cost, relative to the largest (the model test's limit; measured: see the test)


def _opts(has_n):
    """the oracle options of tests/test_sensitivity_cpu.py for x*: double support stops at mu 1e-10 (a deeper barrier only adds ill-conditioning along
    the internal-force direction)"""
    from oracle import oracle_lib as ol
    return ol.ipm_opts(tol=1e-9, mu_min=1e-10) if has_n else ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200)


@functools.lru_cache(maxsize=None)
def _fd(name, which, b, golden_dir):
    """(directions, central differences of the oracle's x* and of its optimal cost along each), computed once per golden problem.  The cost
    differences always come from the deep barrier (tests/test_model_sensitivity_cpu.py's options): the cost is flat along the internal-force
    direction, and at mu ~ 1e-9 the barrier's own derivative, mu sum_i d g_i / s_i over some 600 friction rows, shows in them (4e-7 on cfg2 0)."""
    from oracle import oracle_lib as ol, problem_nlp
    cfg, x, p, lam = _load(name, which, b, golden_dir)
    N = cfg.N
    oc = problem_nlp.oracle_cfg(cfg)
    dirs = srr.rot_directions(N, p)
    has_n = sens_ref.Sens(cfg, x, p, lam).n is not None
    n = len(dirs)
    Pp = np.stack([srr.p_rotated(N, p, s * H * om) for s in (1.0, -1.0) for _, om, _ in dirs])

    def solve(opts):
        Xs, info = ol.ref_solve_batch(oc, Pp, np.repeat(x[None], 2 * n, 0), opts, nthreads=8)
        assert (info[:, 5] == 0).all()
        return Xs
    Xs = solve(_opts(has_n))
    Xf = solve(_opts(False)) if has_n else Xs
    f = np.array([ol.nlp_fg(oc, Xf[i], Pp[i])[0] for i in range(2 * n)])
    return dirs, (Xs[:n] - Xs[n:]) / (2 * H), (f[:n] - f[n:]) / (2 * H)


@pytest.mark.parametrize("name,which,problems", CASES)
def test_rot_jvp_matches_oracle_finite_differences(name, which, problems, golden_dir):
    worst = dict(stance=0.0, swing=0.0, swing_abs=0.0)
    excluded, held = [], 0
    for b in problems:
        cfg, x, p, lam = _load(name, which, b, golden_dir)
        RS = srr.RotSens(cfg, x, p, lam, s_min=S_FD)
        dirs, fdx, _ = _fd(name, which, b, golden_dir)
        assert any(sw for _, _, sw in dirs) or name in ("cfg2", "push")
        for (kind, om, swing), fd in zip(dirs, fdx):
            if RS.n is not None:
                if RS.removed(om) > NO_DERIVATIVE:
                    excluded.append(f"{b}:{kind}")
                    continue
                fd = fd - RS.n * (RS.n @ fd)
            dx = RS.jvp(om)
            err, size = np.abs(dx - fd).max(), np.abs(fd).max()
            held += 1
            if not swing:
                worst["stance"] = max(worst["stance"], err / max(size, FLOOR))
                assert err <= STANCE * max(size, FLOOR), (name, b, kind, err, size)
            else:
                worst["swing_abs"] = max(worst["swing_abs"], err)
                assert err <= SWING_ABS, (name, b, kind, err, size)
                if size >= SWING_SIZE:
                    worst["swing"] = max(worst["swing"], err / size)
                    assert err <= SWING * size, (name, b, kind, err, size)
    print(f"\n{name}: held {held}; gap " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f"; no derivative: {excluded}")
    # only push 0 (double support with loaded friction rows) may lose directions; every cfg2 direction is held
    assert not excluded or name == "push", excluded
    assert held > 0 or name == "push"


@pytest.mark.parametrize("name,which,b", [("cfg2", None, 0), ("cfg5", None, 0), ("yaw", "tmp", 4)])
def test_rot_adjoint_identity(name, which, b, golden_dir):
    """<v, J_omega u> = <J_omega^T v, u> to 1e-10 relative at the default slack floor, and a combined (dp, dtheta, omega) column is the sum of the three"""
    cfg, x, p, lam = _load(name, which, b, golden_dir)
    RS = srr.RotSens(cfg, x, p, lam)
    rng = np.random.default_rng(13)
    u = rng.standard_normal((2, cfg.N, 3)) * 1e-2
    v = rng.standard_normal(x.size)
    a, g = float(v @ RS.jvp(u)), RS.vjp(v)
    bb = float((g * u).sum())
    assert abs(a - bb) <= 1e-10 * max(abs(a), abs(bb)), (a, bb)
    dp = rng.standard_normal(p.size) * sens_ref.covered_mask(cfg.N) * 1e-2
    dth = rng.standard_normal(34) * 1e-2
    both = RS.jvp(u, dth, dp)
    np.testing.assert_allclose(both, RS.jvp(u) + RS.MS.jvp(dth) + RS.S.jvp(dp), rtol=0, atol=1e-9 * np.abs(both).max())


@pytest.mark.parametrize("name,which,b", [("cfg2", None, 0), ("cfg5", None, 0), ("yaw", "tmp", 4), ("gait", "tmp", 3), ("push", "tmp", 0)])
def test_rot_value_gradient_matches_oracle_finite_differences(name, which, b, golden_dir):
    """dV*/domega (envelope theorem at the golden's (x, lam)) against central differences of the oracle's optimal cost on the directions of the JVP
    test, relative to the largest: held to VG as it stands on cfg5 0 (measured 2.1e-8), yaw 4 (1.2e-8), gait 3 (5.3e-8) and push 0 (6.0e-8).
    cfg2 problem 0 is the exception, for two reasons that its tiny effect (largest difference 1.4e-5) brings out.  The value gradient is lam^T d g
    at the GIVEN lam, and the golden's lam carries its solve's barrier residue z = mu / s on the 640 inactive friction rows (1.5e-8 each: 4.2e-7 in
    all), which is zero at the exact optimum that the differences follow: that known share -- rows with a slack above CMPC_SENS_WEAK -- is taken
    out there.  And the differences' own floor is the rounding of the cost: f = 22 is a float64 sum of several hundred terms, so a quotient over
    2 H carries about sqrt(terms) eps |f| / (2 H), taken as 32 eps |f| / (2 H) = 7.8e-9 (measured gap 4.0e-9 after the share is out).  On the other
    cases the share of the inactive rows is asserted to be below 1e-7 of the largest difference (measured <= 2.0e-8), so it stays checked there."""
    from oracle import oracle_lib as ol
    cfg, x, p, lam = _load(name, which, b, golden_dir)
    RS = srr.RotSens(cfg, x, p, lam)
    S = RS.S
    vg = RS.value_gradient()
    dirs, _, fdf = _fd(name, which, b, golden_dir)
    inactive = S.fric[-S.g[S.fric] > sens_ref.WEAK]
    scale = np.abs(fdf).max()
    tiny = name == "cfg2"
    floor = 32 * np.finfo(np.float64).eps * abs(ol.nlp_fg(S.oc, x, p)[0]) / (2 * H) if tiny else 0.0
    worst, worst_share = 0.0, 0.0
    for (_, om, _), fv in zip(dirs, fdf):
        dg, _ = RS._diff(om)
        share = float(S.lam[inactive] @ dg[inactive])
        worst_share = max(worst_share, abs(share) / scale)
        gap = abs(float((vg * om).sum()) - (share if tiny else 0.0) - fv)
        worst = max(worst, max(gap - floor, 0.0) / scale)
    print(f"\n{name} {b}: dV*/domega against oracle differences {worst:.1e} (scale {scale:.1e}, floor {floor:.1e}, inactive rows' share {worst_share:.1e})")
    assert worst <= VG, worst
    assert tiny or worst_share <= 1e-7, worst_share


def test_rot_internal_force_rule(golden_dir):
    """cfg2 (both feet in stance over the whole horizon, no loaded friction row): a rotation direction leaves only lam_h-weighted moments and its
    component along n is at the solve's tolerance (measured <= 3.0e-7); the JVP has no component along n whatever the direction.  push 0 (double
    support with loaded friction rows): rotating one foot gives the internal force a moment arm, the removed size is of order 0.1 and the direction
    has no derivative."""
    worst = 0.0
    for b in range(2):
        cfg, x, p, lam = _load("cfg2", None, b, golden_dir)
        RS = srr.RotSens(cfg, x, p, lam)
        assert RS.n is not None
        for _, om, _ in srr.rot_directions(cfg.N, p):
            worst = max(worst, RS.removed(om))
            dx = RS.jvp(om)
            assert abs(RS.n @ dx) <= 1e-12 * max(1.0, np.abs(dx).max())
    print(f"\ncfg2 removed: {worst:.1e}")
    assert worst <= NO_DERIVATIVE
    cfg, x, p, lam = _load("push", "tmp", 0, golden_dir)
    RS = srr.RotSens(cfg, x, p, lam)
    rem = [RS.removed(om) for _, om, _ in srr.rot_directions(cfg.N, p)]
    print("push 0 removed: " + " ".join(f"{v:.2e}" for v in rem))
    assert RS.n is not None and max(rem) > 0.05
    assert RS.removed_vjp() > 0.05
    cfg, x, p, lam = _load("cfg5", None, 0, golden_dir)
    RS = srr.RotSens(cfg, x, p, lam)
    assert RS.n is None and RS.removed_vjp() == 0.0


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def quat_times_exp(q, w):
    """q (x) exp(w / 2), quaternions (w, x, y, z), float64"""
    t = np.linalg.norm(w)
    e = np.concatenate([[np.cos(t / 2)], np.sin(t / 2) * w / t]) if t > 0 else np.array([1.0, 0, 0, 0])
    a, b = q[0], q[1:]
    return np.concatenate([[a * e[0] - b @ e[1:]], a * e[1:] + e[0] * b + np.cross(b, e[1:])])


def test_list_sum_is_the_transpose_of_the_sampled_rotation(golden_dir):
    """Lists sampled on the host (cmpc_contacts_sample) at quaternions q (x) exp(+-h omega_m / 2): the central difference of P's R block is
    vec(R_k [omega_owner(k)]x), and list_sum is the transpose of that map.  Tolerance: P is float32 (entries <= 1, rounding 6e-8) and the
    difference quotient divides by 2 h = 2e-2, plus the h^2 / 6 truncation of the exponential."""
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    B, N, dt, h = 6, cfg.N, cfg.sampling_time, 1e-2
    t, pose, n = cm.synthetic.footstep_candidate_lists(cfg, B, 9)
    M = t.shape[2]
    L = cm.Layout(N)
    lib = cm._capi.lib()
    rng = np.random.default_rng(2)
    om = rng.standard_normal((B, 2, M, 3))
    om /= np.linalg.norm(om, axis=-1, keepdims=True)
    up = np.array([c.bounding_box_upper_limit for c in cfg.contacts], np.float32)
    lo = np.array([c.bounding_box_lower_limit for c in cfg.contacts], np.float32)

    def sample_R(ps):
        """the R block of P as cmpc_contacts_sample writes it: [B,2,N,3,3], float64"""
        P = np.zeros((B, L.np), np.float32)
        ps = np.ascontiguousarray(ps, np.float32)
        assert lib.cmpc_contacts_sample(N, dt, B, M, 0.0, _ptr(t), _ptr(ps), _ptr(n), _ptr(up), _ptr(lo), _ptr(P), None) == 0
        return np.stack([[[srr.stage_R(L, P[b], c, k) for k in range(N)] for c in range(2)] for b in range(B)])
    sides = []
    for s in (1.0, -1.0):
        ps = pose.copy()
        for idx in np.ndindex(B, 2, M):
            ps[idx][3:] = quat_times_exp(pose[idx][3:].astype(np.float64), s * h * om[idx])
        sides.append(sample_R(ps))
    R0 = sample_R(pose)
    dR = (sides[0] - sides[1]) / (2 * h)            # [B,2,N,3,3]
    tol = 6e-8 / h + h * h / 6 * 1.5
    g_stage = rng.standard_normal((B, 2, N, 3))
    for b in range(B):
        for c in range(2):
            own = srr.stage_owner(N, dt, 0.0, t[b, c], int(n[b, c]))
            assert len(set(own)) >= 1 and (own >= 0).all()
            for k in range(N):
                np.testing.assert_allclose(dR[b, c, k], R0[b, c, k] @ srr.skew(om[b, c, own[k]]), rtol=0, atol=tol)
            # transpose: <g_stage, omega_stage> = <list_sum(g_stage), omega_entry>
            gl = srr.list_sum(g_stage[b, c], own, int(n[b, c]), M)
            lhs = float((g_stage[b, c] * om[b, c, own]).sum())
            assert abs(lhs - float((gl * om[b, c]).sum())) <= 1e-12 * max(1.0, abs(lhs))
            assert not gl[int(n[b, c]):].any()
    assert len({int(v) for v in n.ravel()}) >= 1 and (n >= 2).any()
    # a foot that sampling would not sample gets zeros
    assert not srr.list_sum(g_stage[0, 0], np.zeros(N, int), 0, M).any() and not srr.list_sum(g_stage[0, 0], np.zeros(N, int), M + 1, M).any()
