"""Host checks of the roll-out tick in reverse (include/cmpc.h) through its float64 restatement tests/rollout_adjoint_ref.py: the plant
partials against central differences of oracle/plant_ref.plant_step, the list adjoint against the transposed brute-force matrix of the oracle's merge ->
sample and adjust (oracle/contacts_ref.py, oracle/schedule_ref.py).  tests/test_gpu_rollout_adjoint.py holds the device kernels to the same restatement."""
import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import PlannedContact, pack_lists
from oracle import contacts_ref, plant_ref, schedule_ref
from tests import rollout_adjoint_ref as rar, snap_ref
from tests.test_contacts_cpu import _random_walks

PLANT_FD = 1e-9      # the plant is a polynomial of degree two in its inputs: central differences are exact up to rounding
PLANT_ADJ = 1e-12
LIST_EXACT = 1e-12


def _plant_case(seed, gate_off=None, yaw=0.0, N=8):
    """a random plant input: (L, corners[2][4][3], x, p, state)"""
    rng = np.random.default_rng(seed)
    L = cm.Layout(N)
    x, p = rng.normal(0, 0.3, L.nx), np.zeros(L.np)
    cy, sy = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    for c in range(2):
        for k in range(N):
            p[L.p_R[c] + 9 * k:L.p_R[c] + 9 * k + 9] = (Rz if c == 0 else Rz.T).reshape(-1, order="F")
        p[L.p_gam[c]:L.p_gam[c] + N] = 1.0
        x[L.pos[c]:L.pos[c] + 3] = [0.05 * c, 0.08 * (1 - 2 * c), 0.0] + rng.normal(0, 0.01, 3)
        for j in range(4):
            x[L.f[c][j]:L.f[c][j] + 3] = [rng.normal(0, 0.2), rng.normal(0, 0.2), 9.80665 / 8 + rng.normal(0, 0.3)]
    if gate_off is not None:
        p[L.p_gam[gate_off]] = 0.0
    p[L.p_fext:L.p_fext + 3] = rng.normal(0, 0.5, 3)
    p[L.p_text:L.p_text + 3] = rng.normal(0, 0.1, 3)
    corners = np.array([[[0.08, 0.03, 0], [0.08, -0.03, 0], [-0.08, -0.03, 0], [-0.08, 0.03, 0]]] * 2) + rng.normal(0, 0.005, (2, 4, 3))
    state = np.concatenate([[0.0, 0.0, 0.7] + rng.normal(0, 0.02, 3), rng.normal(0, 0.1, 3), rng.normal(0, 0.05, 3)])
    return L, corners, x, p, state


@pytest.mark.parametrize("gate_off,yaw", [(None, 0.0), (1, 0.0), (None, 0.6), (0, -0.4)])
def test_plant_partials_match_central_differences_of_the_oracle_plant(gate_off, yaw):
    """Every input group (state, pos_0, forces, fExt_0, tauExt_0, corners): relative gap <= 1e-9 with step 1e-4; with one foot gated off and with a yawed R.
    JVP / VJP adjoint identity of the restatement <= 1e-12."""
    L, corners, x, p, state = _plant_case(3, gate_off, yaw)
    step, nsub, eps = 0.01, 6, 1e-4
    J = rar.plant_jacobian(L, corners, x, p, state, step, nsub)
    xi, pi = rar.plant_columns(L)

    def f(state_, x_, p_, cn_):
        return plant_ref.plant_step(L, cn_, x_, p_, state_, step, nsub)[0]
    fd = np.zeros_like(J)
    for col in range(rar.NCOL):
        s1, x1, p1, c1 = state.copy(), x.copy(), p.copy(), corners.copy()
        s0, x0, p0, c0 = state.copy(), x.copy(), p.copy(), corners.copy()
        if col < 9:
            s1[col] += eps; s0[col] -= eps
        elif col < rar.C_FEXT:
            x1[xi[col - 9]] += eps; x0[xi[col - 9]] -= eps
        elif col < rar.C_CORN:
            p1[pi[col - rar.C_FEXT]] += eps; p0[pi[col - rar.C_FEXT]] -= eps
        else:
            c1.reshape(-1)[col - rar.C_CORN] += eps; c0.reshape(-1)[col - rar.C_CORN] -= eps
        fd[:, col] = (f(s1, x1, p1, c1) - f(s0, x0, p0, c0)) / (2 * eps)
    groups = dict(state=(0, 9), pos=(rar.C_POS, rar.C_F), forces=(rar.C_F, rar.C_FEXT), fext=(rar.C_FEXT, rar.C_TEXT), text=(rar.C_TEXT, rar.C_CORN),
                  corners=(rar.C_CORN, rar.NCOL))
    for name, (a, b) in groups.items():
        gap = np.abs(J[:, a:b] - fd[:, a:b]).max() / max(np.abs(fd[:, a:b]).max(), 1e-300)
        print(f"plant partials gate_off={gate_off} yaw={yaw} {name}: relative gap {gap:.2e} (bound {PLANT_FD:.0e})")
        assert gap <= PLANT_FD, (name, gap)
    if gate_off is not None:    # a gated foot: no force derivative, and (no force acts there) no position or corner derivative either
        q = 4 * gate_off
        assert not J[:, rar.C_F + 3 * q:rar.C_F + 3 * q + 12].any() and not J[:, rar.C_POS + 3 * gate_off:rar.C_POS + 3 * gate_off + 3].any()
        assert not J[:, rar.C_CORN + 3 * q:rar.C_CORN + 3 * q + 12].any()
    # adjoint identity <g, J d> = <J^T g, d> through the two entry points
    rng = np.random.default_rng(5)
    ds, dx, dp, dm, g = rng.normal(size=9), rng.normal(size=L.nx), rng.normal(size=L.np), rng.normal(size=34), rng.normal(size=9)
    out = rar.plant_jvp(L, corners, x, p, state, step, nsub, ds, dx, dp, dm)
    gs, gx, gp, gm = rar.plant_vjp(L, corners, x, p, state, step, nsub, g)
    lhs, rhs = g @ out, gs @ ds + gx @ dx + gp @ dp + gm @ dm
    assert abs(lhs - rhs) <= PLANT_ADJ * max(abs(lhs), 1.0), (lhs, rhs)
    assert np.count_nonzero(gx) <= 30 and np.count_nonzero(gp) <= 6 and not gm[:10].any()


# ---------------------------------------------------------------------------------------------------------------- lists
def _to_ref(t, pose, n, names):
    """one problem's packed lists t[2][M][2], pose[2][M][7], n[2] -> the oracle's {name: contact list}"""
    return {nm: [dict(activation=float(t[c, m, 0]), deactivation=float(t[c, m, 1]), position=np.array(pose[c, m, :3], float),
                      quaternion=np.array(pose[c, m, 3:], float)) for m in range(int(n[c]))] for c, nm in enumerate(names)}


def _list_forward(cfg, now, plan, prev, xland, snap):
    """The forward list path of one problem through the oracle: plan / prev = (t, pose, n) of one problem (prev's poses are the positions perturbed; plan
    None: first tick, prev is the caller's list).  -> (nominal[2][N+1][3], current[2][3], out positions[2][M][3], land[2], merged times[2][M][2], n[2])"""
    N, dt = cfg.N, cfg.sampling_time
    names = [c.contact_name for c in cfg.contacts]
    M = prev[0].shape[1]
    if plan is None:
        lst = _to_ref(*prev, names)
    else:
        pt = plan[0]
        if snap:
            pt, ok = snap_ref.snap_lists(dt, pt[None], plan[2][None])
            assert ok.all()
            pt = pt[0]
        good, lst = contacts_ref.update_contact_phase_list(now + 1e-9, _to_ref(pt, plan[1], plan[2], names), _to_ref(*prev, names))
        assert good
    boxes = {nm: (cfg.contacts[c].bounding_box_upper_limit, cfg.contacts[c].bounding_box_lower_limit) for c, nm in enumerate(names)}
    samp = schedule_ref.sample_contact_phase_list(N, dt, now, lst, boxes)
    nominal, current = np.zeros((2, N + 1, 3)), np.zeros((2, 3))
    outp, land, mt, mn = np.zeros((2, M, 3)), np.zeros(2, int), np.zeros((2, M, 2)), np.zeros(2, int)
    for c, nm in enumerate(names):
        nominal[c], current[c], land[c] = samp[nm]["nominal"], samp[nm]["current"], samp[nm]["land"]
        adj = schedule_ref.adjust_contact_list(now, lst[nm], land[c], xland[c])
        mn[c] = len(adj)
        for m, ct in enumerate(adj):
            outp[c, m] = ct["position"]
            mt[c, m] = (ct["activation"], ct["deactivation"])
    return nominal, current, outp, land, mt, mn


def _brute_force_list_matrix(cfg, label, now, t_b, pose_b, n_b, ts, first_tick, snap, rng):
    """one problem of test_list_adjoint_is_the_transposed_brute_force_matrix: t_b / pose_b / n_b the planner's lists, ts the previous tick's times"""
    N, dt = cfg.N, cfg.sampling_time
    L = cm.Layout(N)
    M = t_b.shape[1]
    plan = None if first_tick else (t_b, pose_b, n_b)
    prev_pose = pose_b.astype(np.float64).copy()
    prev_pose[..., :3] += rng.uniform(-0.01, 0.01, prev_pose[..., :3].shape)
    prev = (ts if not first_tick else t_b, prev_pose, n_b)
    xland = rng.normal(0, 0.1, (2, 3))

    def fwd(prev_pos, plan_pos, xl):
        pv = (prev[0], np.concatenate([prev_pos, prev[1][..., 3:]], -1), prev[2])
        pl = None if plan is None else (plan[0], np.concatenate([plan_pos, plan[1][..., 3:]], -1), plan[2])
        nom, cur, outp, land, mt, mn = _list_forward(cfg, now, pl, pv, xl, snap)
        return np.concatenate([nom.ravel(), cur.ravel(), outp.ravel()]), land, mt, mn
    base_in = [prev[1][..., :3].copy(), pose_b[..., :3].astype(np.float64), xland]
    y0, land, mt, mn = fwd(*base_in)
    nin = [a.size for a in base_in]
    A = np.zeros((y0.size, sum(nin)))
    col = 0
    for gi, a in enumerate(base_in):
        for e in range(a.size):
            ins = [v.copy() for v in base_in]
            ins[gi].reshape(-1)[e] += 1.0
            A[:, col] = fwd(*ins)[0] - y0
            col += 1
    # the restated adjoint, one unit cotangent per output entry
    At = np.zeros_like(A.T)
    n_nom = 2 * (N + 1) * 3
    for r in range(y0.size):
        gp, gout = np.zeros(L.np), np.zeros((2, M, 3))
        if r < n_nom:
            c, e = divmod(r, (N + 1) * 3)
            gp[L.p_nom[c] + e] = 1.0
        elif r < n_nom + 6:
            c, e = divmod(r - n_nom, 3)
            gp[L.p_cur[c] + e] = 1.0
        else:
            gout.reshape(-1)[r - n_nom - 6] = 1.0
        res = rar.list_position_vjp(L, dt, now, mt, mn, land, plan=None if plan is None else (plan[0], plan[2]),
                                    prev=None if plan is None else (prev[0], prev[2]), g_out=gout, g_p=gp, force_sample_time=snap)
        gxl = np.array([res["x"][L.pos[c] + 3 * land[c]:L.pos[c] + 3 * land[c] + 3] if 0 <= land[c] <= N else np.zeros(3) for c in range(2)])
        At[:, r] = np.concatenate([res["prev"].ravel(), res["plan"].ravel(), gxl.ravel()])
    gap = np.abs(At - A.T).max()
    assert gap <= LIST_EXACT, (label, gap)
    # (whether the adjustment wrote a landing position into the outgoing list, whether planner positions reached the outputs)
    return int(A[n_nom + 6:, nin[0] + nin[1]:].any()), int(A[:, nin[0]:nin[0] + nin[1]].any())


@pytest.mark.parametrize("case", ["before_lift_off", "in_swing", "landing_tick", "after_landing", "first_tick", "off_grid_snapped", "late"])
def test_list_adjoint_is_the_transposed_brute_force_matrix(case):
    """The forward list maps are linear in the positions: every position entry of random lists is perturbed through the oracle's merge -> sample and
    adjust, at several `now`; the restated adjoint applied to unit cotangents equals the transposed matrix (<= 1e-12)."""
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    N, dt = cfg.N, cfg.sampling_time
    L = cm.Layout(N)
    B = 6
    walks = _random_walks(cfg, B, 17, t_end=3.0)
    rng = np.random.default_rng(2)
    snap = case == "off_grid_snapped"
    if not snap:     # times on the grid (what forceSampleTime leaves); the snapped case keeps the random off-grid times
        for w in walks:
            for lst in w.values():
                for ct in lst:
                    ct.activation_time = round(ct.activation_time / dt) * dt
                    ct.deactivation_time = ct.deactivation_time if ct.deactivation_time >= 1e9 else round(ct.deactivation_time / dt) * dt
    t, pose, n = pack_lists(cfg, walks, max_contacts=12)
    M = t.shape[2]
    checked_landing = checked_merge = 0
    for b in range(B):
        ts = snap_ref.snap_lists(dt, t[b][None], n[b][None])[0][0] if snap else t[b]
        lift, landing = min(ts[c, 0, 1] for c in range(2)), min(ts[c, 1, 0] for c in range(2))     # first lift-off of either foot, first landing
        now = dict(before_lift_off=max(lift - 3 * dt, 0.0), in_swing=lift + dt, landing_tick=landing, after_landing=landing + 2 * dt, first_tick=0.0,
                   off_grid_snapped=lift + dt, late=2.4)[case]
        now = round(now / dt) * dt
        landed, merged = _brute_force_list_matrix(cfg, (case, b), now, t[b], pose[b], n[b], ts, case == "first_tick", snap, rng)
        checked_landing += landed
        checked_merge += merged
    print(f"list adjoint {case}: {B} problems, landing adjusted in {checked_landing}, planner entries used in {checked_merge}")
    if case in ("in_swing", "off_grid_snapped"):
        assert checked_landing == B
    if case != "first_tick":
        assert checked_merge == B


@pytest.mark.parametrize("i", [3, 8, 9, 14])
def test_list_adjoint_is_the_transposed_brute_force_matrix_at_dt_01(i):
    """The same at N = 8, dt = 0.1 on the gait the GPU tests walk on that grid, at now = i * dt for the landing tick 8 and for ticks 3, 9 and 14, whose time
    differs from the plan's (0.3, 0.3 + 0.5 + 0.1, ...) in its last bits (asserted): the oracle's merge and sampling on the plan's own doubles against
    the restatement's integer-nanosecond clock."""
    cfg = cm.config.ergocub_gazebo_v1(8, 0.1)
    plan = cm.rollout.walking_plan(cfg, **GAIT_DT01)
    if i != 8:
        assert_tick_time_differs_from_the_plans(plan, cfg.sampling_time, i)
    t, pose, n = pack_lists(cfg, [plan])
    landed, merged = _brute_force_list_matrix(cfg, ("dt_01", i), i * cfg.sampling_time, t[0], pose[0], n[0], t[0], False, False, np.random.default_rng(i))
    print(f"list adjoint at dt = 0.1, tick {i}: landing adjusted {landed}, planner entries used {merged}")
    assert landed == 1 and merged == 1


# ---------------------------------------------------------------------------------------------------------------- solve + plant
from tests import sens_model_ref as smr, sens_ref  # noqa: E402
from tests.test_model_sensitivity_cpu import H_MIN, H_REL, NO_DERIVATIVE, SWING_FIELDS  # noqa: E402
from tests.test_sensitivity_cpu import CASES, FD_CLEAN, FD_WEAK, S_FD, _load  # noqa: E402

STEP, NSUB = 0.01, 6


def _landing_knots(cfg, p):
    """the landing knot of each foot from Gamma (the rule of cmpc_contacts_sample), -1 if the foot never lifts"""
    L = cm.Layout(cfg.N)
    out = []
    for c in range(2):
        gam = p[L.p_gam[c]:L.p_gam[c] + cfg.N] > 0.5
        land, prev = -1, True
        for k in range(cfg.N):
            if gam[k] and not prev and land < 0:
                land = k
            prev = gam[k]
        out.append(cfg.N if (not prev and land < 0) else land)
    return out


@pytest.mark.parametrize("name,which,problems", CASES)
def test_solve_and_plant_composed_match_oracle_finite_differences(name, which, problems, golden_dir):
    """l = <v, state'> + <w, x.pos[land]>: dl/d(com0, dcom0, h0, currentPos, nominalPos, fExt, tauExt) from the restatement (Sens.vjp after the plant VJP;
    a state direction moves the solve's initial rows and the plant's state together) against central differences of ol.ref_solve_batch followed by
    plant_step.  The five goldens tests/test_sensitivity_cpu.py holds to FD_CLEAN (cfg2 0, 1; cfg5 0, 2; yaw 4) are held to FD_CLEAN here whatever Sens.weak
    says, and push 0 to FD_WEAK where Sens.weak > 0.  cfg2 and cfg5 classify as clean (asserted); yaw 4 does not -- Sens.weak counts 5 weakly active rows
    there (one of them is what that file's comment mentions) -- and passes the tight bound all the same, so the tight bound is what it is held to.  The same
    for one cost weight and one corner direction with sens_model_ref, under the rule of tests/test_model_sensitivity_cpu.py (for yaw 4 again the tight
    bound)."""
    from oracle import oracle_lib as ol, problem_nlp
    rng = np.random.default_rng(31)
    worst = {}
    for b in problems:
        cfg, x, p, lam = _load(name, which, b, golden_dir)
        N = cfg.N
        L = cm.Layout(N)
        theta = smr.theta_of(cfg)
        corners = theta[10:].reshape(2, 4, 3)
        MS = smr.ModelSens(cfg, x, p, lam, s_min=S_FD)
        S = MS.S
        if name in ("cfg2", "cfg5"):
            assert S.weak == 0, (name, b, S.weak)
        bound = FD_CLEAN if name != "push" else (FD_WEAK if S.weak else FD_CLEAN)
        land = _landing_knots(cfg, p)
        v, w = rng.normal(size=9), rng.normal(size=(2, 3))
        state = p[L.p_com0:L.p_com0 + 9].copy()

        def loss(xs, pp, st, cn):
            out = v @ plant_ref.plant_step(L, cn, xs, pp, st, STEP, NSUB)[0]
            return out + sum(w[c] @ xs[L.pos[c] + 3 * land[c]:L.pos[c] + 3 * land[c] + 3] for c in range(2) if land[c] >= 0)
        # the restatement: plant VJP, the landing positions' cotangent, the solution VJP
        gs, gx, gp_plant, gm_plant = rar.plant_vjp(L, corners, x, p, state, STEP, NSUB, v)
        for c in range(2):
            if land[c] >= 0:
                gx[L.pos[c] + 3 * land[c]:L.pos[c] + 3 * land[c] + 3] += w[c]
        gp = S.vjp(gx) + gp_plant
        gm = MS.vjp(gx) + gm_plant
        # directions in p (those of tests/sens_ref.py that belong to the groups asked for, and the knot-0 wrench the plant reads itself)
        keep = {"com0", "dcom0", "h0", "nominalPos", "fExt", "tauExt"}
        dirs = [(k, d) for k, d in sens_ref.directions(cfg, p, lam) if k in keep or "urrent" in k]
        for k, i in (("fExt", L.p_fext), ("fExt", L.p_fext + 2), ("tauExt", L.p_text + 1)):
            d = np.zeros(L.np)
            d[i] = 1.0
            dirs.append((k, d))
        assert {"com0", "dcom0", "h0", "nominalPos", "fExt", "tauExt"} <= {k for k, _ in dirs}
        oc = problem_nlp.oracle_cfg(cfg)
        opts = ol.ipm_opts(tol=1e-9, mu_min=1e-10) if S.n is not None else ol.ipm_opts(tol=1e-11, mu_min=1e-12, max_iter=200)
        h = 1e-5
        Pp = np.concatenate([np.stack([p + h * d for _, d in dirs]), np.stack([p - h * d for _, d in dirs])])
        Xs, info = ol.ref_solve_batch(oc, Pp, np.repeat(x[None], Pp.shape[0], 0), opts, nthreads=8)
        assert (info[:, 5] == 0).all()
        fd, got = {}, {}
        for i, (kind, d) in enumerate(dirs):
            lp = loss(Xs[i], Pp[i], Pp[i][L.p_com0:L.p_com0 + 9], corners)
            lm = loss(Xs[len(dirs) + i], Pp[len(dirs) + i], Pp[len(dirs) + i][L.p_com0:L.p_com0 + 9], corners)
            fd.setdefault(kind, []).append((lp - lm) / (2 * h))
            got.setdefault(kind, []).append(gp @ d + gs @ d[L.p_com0:L.p_com0 + 9])
        for kind in fd:
            a, r = np.array(got[kind]), np.array(fd[kind])
            gap = np.abs(a - r).max() / max(np.abs(r).max(), 1e-3)
            worst[kind] = max(worst.get(kind, 0.0), gap)
            assert gap <= bound, (name, b, kind, gap, S.weak)
        # two model directions that touch no kink: one cost weight, one (mirrored) corner pair
        mdirs = [(k, d) for k, d in smr.model_directions(cfg) if k in ("com_weight_x", "corner_mirrored")]
        assert len(mdirs) == 2
        for kind, d in mdirs:
            if MS.n is not None and MS.removed(d) > NO_DERIVATIVE:
                continue
            hm = max(H_REL * float(np.abs(theta[d != 0]).max()), H_MIN)
            vals = []
            for sgn in (1.0, -1.0):
                th = theta + sgn * hm * d
                X1, inf1 = ol.ref_solve_batch(smr.nlp_cfg(cfg, th), p[None], x[None], opts)
                assert (inf1[:, 5] == 0).all()
                vals.append(loss(X1[0], p, state, th[10:].reshape(2, 4, 3)))
            r = (vals[0] - vals[1]) / (2 * hm)
            gap = abs(gm @ d - r) / max(abs(r), 1e-3)
            worst[kind] = max(worst.get(kind, 0.0), gap)
            weak = (S.weak if name == "push" else 0) + (S.weak_swing if kind in SWING_FIELDS else 0)
            assert gap <= (FD_WEAK if weak else FD_CLEAN), (name, b, kind, gap)
    print(f"\nsolve + plant, {name}: gap " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" (bounds: clean {FD_CLEAN:.0e}, weak {FD_WEAK:.0e})")


# ---------------------------------------------------------------------------------------------------------------- ticks on the float64 oracle
def _oracle_ticks(cfg, plan_lists, state0, first_tick, ticks, push=None, push_ticks=0, com_speed=0.0):
    """`ticks` ticks of the closed loop on the float64 oracle, from tick number first_tick (the lists start as the planner's): lists by the package's
    mirrors of the merge and the sampling, x and lam_g by oracle/ipm_generic.solve + map_record(record_from_lam(...)), the adjustment and the plant in
    numpy.  -> (tapes for rollout_adjoint_ref, nows, final state)"""
    from cmpc_amd.contacts import sample_schedule_batch, update_contact_phase_list
    from oracle import ipm_generic, problem_nlp
    from tests.test_multipliers_cpu import map_record, record_from_lam
    N, dt = cfg.N, cfg.sampling_time
    L = cm.Layout(N)
    oc = problem_nlp.oracle_cfg(cfg)
    corners = smr.theta_of(cfg)[10:].reshape(2, 4, 3)
    t, pose, n = pack_lists(cfg, [plan_lists])
    M = t.shape[2] + 1
    tt, pp = np.zeros((1, 2, M, 2)), np.zeros((1, 2, M, 7), np.float32)
    pp[..., 3] = 1.0
    tt[:, :, :M - 1], pp[:, :, :M - 1] = t, pose
    plan = (tt, pp, n.astype(np.int32))
    prev, state, tapes, nows = None, np.asarray(state0, np.float64).copy(), [], []
    for i in range(first_tick, first_tick + ticks):
        now = i * dt
        if prev is None:
            lists = tuple(a.copy() for a in plan)
        else:
            lists, ok = update_contact_phase_list(now, plan, prev)
            assert ok.all()
        samp, land = sample_schedule_batch(cfg, *lists, now)
        com_ref = np.zeros((1, N + 1, 3))
        com_ref[0, :, 0] = com_speed * (now + dt * np.arange(N + 1))
        com_ref[0, :, 2] = 0.7
        fext = np.zeros((1, N, 3))
        if push is not None and i < push_ticks:
            fext[0, :max(push_ticks - i, 1)] = push
        P = cm.pack_parameters(N, *(samp[k].astype(np.float64) for k in ("R", "upper", "lower", "enabled", "nominal", "current")),
                               state[None, 0:3], state[None, 3:6], state[None, 6:9], com_ref, np.zeros((1, N + 1, 3)), fext, np.zeros((1, N, 3)))
        p = P[0]
        lb, ub = problem_nlp.bounds(cfg, p)
        r = ipm_generic.solve(oc, p, lb, ub, cm.cold_start(N, P)[0], tol=1e-10, max_iter=400)
        assert r["status"] == 0
        x = r["x"]
        lam = map_record(cfg, x, p, *record_from_lam(cfg, x, p, r["lam_g"]))
        tapes.append(dict(X=x, P=p, lam_g=lam, state=state.copy(), status=0, ok=True, land=land[0].copy(), list_t=lists[0][0].copy(),
                          list_n=lists[2][0].copy(), plan=(plan[0][0], plan[2][0]), prev=None if prev is None else (prev[0][0].copy(), prev[2][0].copy()),
                          step=dt / NSUB, substeps=NSUB, force_sample_time=False, push_knots=max(push_ticks - i, 1) if (push is not None and i < push_ticks) else 0))
        nows.append(now)
        lists = tuple(a.copy() for a in lists)
        for c in range(2):      # the step adjustment
            if 0 <= land[0, c] <= N:
                nx = rar._next(rar._as_list(lists[0][0, c], lists[2][0, c]), rar._ns(now))
                if nx >= 0:
                    lists[1][0, c, nx, :3] = x[L.pos[c] + 3 * land[0, c]:L.pos[c] + 3 * land[0, c] + 3]
        state = plant_ref.plant_step(L, corners, x, p, state, dt / NSUB, NSUB)[0]
        prev = lists
    return tapes, nows, state


def test_reverse_sweep_is_the_product_of_its_ticks():
    """Three ticks of rollout.walking_plan at N = 8 on the float64 oracle -- ticks 3, 4, 5 of a plan whose left foot lifts at tick 1 and lands at tick 5:
    tick 4 has the landing inside the horizon (knot 1; the adjustment writes the landing position into the list) and tick 5 merges the landed contact.
    The restated reverse sweep equals the product of the dense per-tick Jacobians of (state, list positions), built column by column from the
    restatement's forward mode, to 1e-10: this pins the bookkeeping (which gradient goes where between ticks), not the solver."""
    cfg = cm.config.ergocub_gazebo_v1(8, 0.06)
    plan = cm.rollout.walking_plan(cfg, steps=4, step_length=0.1, swing=0.24, double_support=0.12, first_lift=0.06)
    _check_reverse_sweep_is_the_product_of_its_ticks(cfg, plan, first_tick=3, ticks=3)


GAIT_DT01 = dict(swing=0.5, double_support=0.1, first_lift=0.3)       # (synthetic.gait_cycle's gait on the grid of dt = 0.1)


def assert_tick_time_differs_from_the_plans(plan, dt, i):
    """tick i falls on a time of the plan on the nanosecond grid, and i * dt is another double than the plan's: the case CMPC_TIME_EPS is there for"""
    same = {t for lst in plan.values() for ct in lst for t in (ct.activation_time, ct.deactivation_time) if rar._ns(t) == i * rar._ns(dt)}
    assert len(same) == 1 and same.pop() != i * dt, (i, same)


def test_reverse_sweep_is_the_product_of_its_ticks_at_dt_01():
    """The same at N = 8, dt = 0.1 on the gait the GPU tests walk on that grid (lift-off at tick 3, landing at tick 8), ticks 6 .. 9: tick 7 has the
    landing at knot 1, tick 8 is the landing tick and merges the landed contact, and tick 9 -- the other foot's lift-off -- is a tick whose time 9 * dt
    differs from the plan's 0.3 + 0.5 + 0.1 in its last bits (asserted): the restatement's integer-nanosecond clock and the package's merge and sampling,
    which the oracle loop runs, must name the same contacts there."""
    cfg = cm.config.ergocub_gazebo_v1(8, 0.1)
    plan = cm.rollout.walking_plan(cfg, **GAIT_DT01)
    assert_tick_time_differs_from_the_plans(plan, cfg.sampling_time, 9)
    _check_reverse_sweep_is_the_product_of_its_ticks(cfg, plan, first_tick=6, ticks=4)


def _check_reverse_sweep_is_the_product_of_its_ticks(cfg, plan, first_tick, ticks):
    """the second taped tick has the landing at knot 1, the third is the landing tick"""
    state0 = np.array([0.01, -0.02, 0.7, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0])
    tapes, nows, _ = _oracle_ticks(cfg, plan, state0, first_tick=first_tick, ticks=ticks, com_speed=0.1)
    assert tapes[1]["land"][0] == 1 and tapes[2]["prev"] is not None
    M = tapes[0]["list_t"].shape[1]
    nz = 9 + 2 * M * 3
    Js = []
    for tp, now in zip(tapes, nows):
        MS = smr.ModelSens(cfg, tp["X"], tp["P"], tp["lam_g"])
        J = np.zeros((nz, nz))
        for col in range(nz):
            d = np.zeros(nz)
            d[col] = 1.0
            ds, dl = rar.tick_jvp(cfg, tp, now, d[:9], d[9:].reshape(2, M, 3), MS=MS)
            J[:, col] = np.concatenate([ds, dl.ravel()])
        Js.append(J)
    assert np.abs(Js[2][:9, 9:]).max() > 1e-6 and np.abs(Js[1][9:, :9]).max() > 1e-6     # the lists and the states do talk to each other
    rng = np.random.default_rng(8)
    gS = rng.normal(size=(ticks + 1, 9))
    out = rar.reverse_sweep(cfg, tapes, nows, gS)
    g = np.concatenate([gS[ticks], np.zeros(nz - 9)])
    for i in reversed(range(ticks)):
        g = Js[i].T @ g
        g[:9] += gS[i]
    got = np.concatenate([out["state0"], out["list0"].ravel()])
    gap = np.abs(got - g).max() / np.abs(g).max()
    print(f"\nreverse sweep over ticks {first_tick} .. {first_tick + ticks - 1} at dt = {cfg.sampling_time} against the product of the per-tick Jacobians: "
          f"{gap:.2e} (bound 1e-10)")
    assert gap <= 1e-10


def test_closed_loop_finite_difference_of_a_standing_robot_under_a_push():
    """Three ticks of a standing robot under a push (double support over the whole horizon, no active inequality: the cfg2 class):
    d <v, state_3> / d (state_0, push) from the restated reverse sweep against central differences of the same float64 oracle loop, bound 3 x FD_CLEAN
    (first-order accumulation over three ticks).  Walking ticks are not held to a closed-loop finite difference: every walking problem has weakly
    active rows somewhere, where the barrier derivative is one value between the one-sided slopes of a kink."""
    cfg = cm.config.ergocub_gazebo_v1(8, 0.06)
    names = [c.contact_name for c in cfg.contacts]
    stand = {names[0]: [PlannedContact(0.0, 1e9, (0.0, 0.08, 0.0))], names[1]: [PlannedContact(0.0, 1e9, (0.0, -0.08, 0.0))]}
    state0 = np.array([0.01, -0.005, 0.7, 0.02, 0.01, 0.0, 0.0, 0.0, 0.0])
    push = np.array([0.2, -0.15, 0.0])
    v = np.random.default_rng(6).normal(size=9)

    def run(s0, pu):
        return _oracle_ticks(cfg, stand, s0, first_tick=0, ticks=3, push=pu, push_ticks=2)
    tapes, nows, final = run(state0, push)
    gS = np.zeros((4, 9))
    gS[3] = v
    out = rar.reverse_sweep(cfg, tapes, nows, gS, push_knots=[tp["push_knots"] for tp in tapes])
    assert out["status"] == [0, 0, 0]
    assert all(smr.ModelSens(cfg, tp["X"], tp["P"], tp["lam_g"]).S.weak == 0 for tp in tapes)
    h = 1e-5
    fd_s = np.array([(v @ run(state0 + h * e, push)[2] - v @ run(state0 - h * e, push)[2]) / (2 * h) for e in np.eye(9)])
    fd_p = np.array([(v @ run(state0, push + h * e)[2] - v @ run(state0, push - h * e)[2]) / (2 * h) for e in np.eye(3)])
    gap_s = np.abs(out["state0"] - fd_s).max() / np.abs(fd_s).max()
    gap_p = np.abs(out["push"] - fd_p).max() / np.abs(fd_p).max()
    print(f"\nclosed-loop finite difference over three ticks: state0 {gap_s:.2e} push {gap_p:.2e} (bound {3 * FD_CLEAN:.0e})")
    assert gap_s <= 3 * FD_CLEAN and gap_p <= 3 * FD_CLEAN
