"""Host checks of the roll-out tick in reverse with the contacts' orientations (include/cmpc.h) through its float64 restatement
tests/rollout_rot_ref.py: the plant's rotation columns against central differences of oracle/plant_ref.plant_step, the orientation list adjoint against
the brute-force incidence of the oracle's merge -> sample (oracle/contacts_ref.py, oracle/schedule_ref.py), and the adjoint identity of the restated tick
on oracle-solved ticks of a yawed walk.  tests/test_gpu_rollout_rot_adjoint.py holds the device kernels to the same restatement."""
import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import pack_lists
from oracle import contacts_ref, plant_ref, schedule_ref
from tests import rollout_adjoint_ref as rar
from tests import rollout_rot_ref as rrr
from tests import sens_rot_ref as srr
from tests.test_contacts_cpu import _random_walks
from tests.test_gpu_rollout_adjoint import _plant_inputs
from tests.test_rollout_adjoint_cpu import _oracle_ticks, _to_ref

PLANT_ROT_FD = 1e-7     # the map is linear in R: what remains is the second-order term of expm and the rounding of h' over 2 h (eps |h'| / h, h = 1e-6)
TICK_ADJ = 1e-9


def test_plant_rotation_columns_match_central_differences_of_the_oracle_plant():
    """d state' / d omega_{c,0} against central differences of plant_step with R_{c,0} replaced by R expm([h omega]x), h = 1e-6, in float64, on the
    inputs of the GPU test (yawed feet, one foot of every third problem gated off, per-problem corners): relative gap <= 1e-7 of the largest entry; a
    gated-off foot's columns are zero; only h' moves."""
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    L = cm.Layout(cfg.N)
    B, step, nsub, h = 16, 0.01, 6, 1e-6
    X, P, state, models = _plant_inputs(cfg, B, 4)
    worst, gated = 0.0, 0
    for b in range(B):
        x, p, s = X[b].astype(np.float64), P[b].astype(np.float64), state[b].astype(np.float64)
        corners = models[b, 10:].reshape(2, 4, 3)
        J = rrr.plant_rot_columns(L, corners, x, p, s, step, nsub)
        fd = np.zeros_like(J)
        for c in range(2):
            R = p[L.p_R[c]:L.p_R[c] + 9].reshape(3, 3, order="F")
            for a in range(3):
                vals = []
                for sgn in (1.0, -1.0):
                    pp = p.copy()
                    pp[L.p_R[c]:L.p_R[c] + 9] = (R @ srr.expm(sgn * h * np.eye(3)[a])).reshape(-1, order="F")
                    vals.append(plant_ref.plant_step(L, corners, x, pp, s, step, nsub)[0])
                fd[:, 3 * c + a] = (vals[0] - vals[1]) / (2 * h)
        gap = np.abs(J - fd).max() / np.abs(fd).max()
        worst = max(worst, gap)
        assert not J[0:6].any() and np.abs(fd[0:6]).max() <= 1e-9
        for c in range(2):
            if not P[b, L.p_gam[c]] > 0.5:
                gated += 1
                assert not J[:, 3 * c:3 * c + 3].any() and not fd[:, 3 * c:3 * c + 3].any()
            else:
                assert J[6:9, 3 * c:3 * c + 3].any()
        # the restated pair is adjoint
        rng = np.random.default_rng(b)
        g, d = rng.normal(size=9), rng.normal(size=(2, 3))
        lhs = g @ (rrr.plant_jvp(L, corners, x, p, s, step, nsub, np.zeros(9), d_rot0=d) )
        rhs = float((rrr.plant_vjp(L, corners, x, p, s, step, nsub, g)[4] * d).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1e-300)
    print(f"\nplant rotation columns against oracle differences: worst relative gap {worst:.2e} (bound {PLANT_ROT_FD:.0e}), gated-off feet {gated}")
    assert worst <= PLANT_ROT_FD and gated >= 4


# ---------------------------------------------------------------------------------------------------------------- lists
def _quat_exp(q, w):
    """q (x) exp(w / 2), quaternions (w, x, y, z)"""
    t = np.linalg.norm(w)
    e = np.concatenate([[np.cos(t / 2)], np.sin(t / 2) * w / t]) if t > 0 else np.array([1.0, 0, 0, 0])
    a, b = q[0], q[1:]
    return np.concatenate([[a * e[0] - b @ e[1:]], a * e[1:] + e[0] * b + np.cross(b, e[1:])])


def _vee(S):
    return np.array([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]]) / 2


def _orientation_forward(cfg, now, plan, prev):
    """The forward list path of one problem through the oracle, orientations only: plan / prev = (t[2][M][2], pose[2][M][7], n[2]) (plan None: first
    tick, prev is the caller's list) -> None when the merge fails, else (R[2][N] stage rotations, Rl[2][M] rotations of the merged list's entries (identity
    beyond its length), land[2], merged times[2][M][2], n[2])."""
    N, dt = cfg.N, cfg.sampling_time
    names = [c.contact_name for c in cfg.contacts]
    M = prev[0].shape[1]
    if plan is None:
        lst = _to_ref(*prev, names)
    else:
        good, lst = contacts_ref.update_contact_phase_list(now + 1e-9, _to_ref(*plan, names), _to_ref(*prev, names))
        if not good:
            return None
    boxes = {nm: (cfg.contacts[c].bounding_box_upper_limit, cfg.contacts[c].bounding_box_lower_limit) for c, nm in enumerate(names)}
    samp = schedule_ref.sample_contact_phase_list(N, dt, now, lst, boxes)
    R, Rl = np.zeros((2, N, 3, 3)), np.tile(np.eye(3), (2, M, 1, 1))
    land, mt, mn = np.zeros(2, int), np.zeros((2, M, 2)), np.zeros(2, int)
    for c, nm in enumerate(names):
        R[c], land[c], mn[c] = np.array(samp[nm]["R"]), samp[nm]["land"], len(lst[nm])
        for m, ct in enumerate(lst[nm]):
            Rl[c, m] = np.array(schedule_ref.quaternion_to_rotation(ct["quaternion"]))
            mt[c, m] = (ct["activation"], ct["deactivation"])
    return R, Rl, land, mt, mn


@pytest.mark.parametrize("case", ["now_9", "now_22", "first_tick", "failed_merge"])
def test_list_orientation_adjoint_is_the_transposed_brute_force_incidence(case):
    """Every quaternion of the previous tick's and of the planner's lists is perturbed by exp(h e_i / 2) on the right, one at a time, through the
    oracle's merge -> sample; R_k^T dR_k / h of every stage and of every entry of the outgoing list, rounded, is a 0/1 incidence matrix.  The
    restatement's forward map equals it exactly and its adjoint is the exact transpose; a failed merge passes nothing on (status 5)."""
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    N, dt = cfg.N, cfg.sampling_time
    L = cm.Layout(N)
    B, h = 6, 1e-3
    walks = _random_walks(cfg, B, 17, t_end=3.0)
    for w in walks:     # times on the grid (what forceSampleTime leaves)
        for lst in w.values():
            for ct in lst:
                ct.activation_time = round(ct.activation_time / dt) * dt
                ct.deactivation_time = ct.deactivation_time if ct.deactivation_time >= 1e9 else round(ct.deactivation_time / dt) * dt
    t, pose, n = pack_lists(cfg, walks, max_contacts=12)
    M = t.shape[2]
    now = dt * dict(now_9=9, now_22=22, first_tick=0, failed_merge=9)[case]
    rng = np.random.default_rng(6)
    merged_entries = planner_entries = 0
    for b in range(B):
        prev = (t[b], pose[b].astype(np.float64), n[b])
        plan = None if case == "first_tick" else (t[b] + (50.0 if case == "failed_merge" else 0.0), pose[b].astype(np.float64), n[b])
        base = _orientation_forward(cfg, now, plan, prev)
        kw = dict(plan=None if plan is None else (plan[0], plan[2]), prev=None if plan is None else (prev[0], prev[2]))
        if case == "failed_merge":
            assert base is None
            r = rrr.list_orientation_vjp(L, dt, now, t[b], n[b], ok=False, g_out=rng.normal(size=(2, M, 3)), g_rot=rng.normal(size=(2, N, 3)), **kw)
            assert r["status"] == 5 and not r["prev"].any() and not r["plan"].any()
            continue
        R0, Rl0, land, mt, mn = base
        nin = 2 * M * 3
        A = np.zeros((2 * N * 3 + nin, 2 * nin))      # rows: stages, then the outgoing list; columns: previous list, then the planner's
        for src in range(1 if plan is None else 2):
            for c in range(2):
                for m in range(int(n[b][c])):
                    for i in range(3):
                        pv, pl = prev[1].copy(), None if plan is None else plan[1].copy()
                        tgt = pv if src == 0 else pl
                        tgt[c, m, 3:] = _quat_exp(tgt[c, m, 3:], h * np.eye(3)[i])
                        R1, Rl1, land1, _, mn1 = _orientation_forward(cfg, now, None if plan is None else (plan[0], pl, plan[2]), (prev[0], pv, prev[2]))
                        assert np.array_equal(land1, land) and np.array_equal(mn1, mn)
                        col = src * nin + (c * M + m) * 3 + i
                        for cc in range(2):
                            for k in range(N):
                                A[(cc * N + k) * 3:(cc * N + k) * 3 + 3, col] = np.rint(_vee(R0[cc, k].T @ (R1[cc, k] - R0[cc, k])) / h)
                            for mm in range(M):
                                A[2 * N * 3 + (cc * M + mm) * 3:2 * N * 3 + (cc * M + mm) * 3 + 3, col] = np.rint(_vee(Rl0[cc, mm].T @ (Rl1[cc, mm] - Rl0[cc, mm])) / h)
        assert set(np.unique(A)) <= {0.0, 1.0}
        # the restatement forwards, one unit direction per column, and transposed, one unit cotangent per row
        Af, At = np.zeros_like(A), np.zeros_like(A.T)
        for col in range(2 * nin):
            d = np.zeros(2 * nin)
            d[col] = 1.0
            d_rot, d_list = rrr.list_orientation_jvp(L, dt, now, mt, mn, d[:nin].reshape(2, M, 3), d[nin:].reshape(2, M, 3), land=land, **kw)
            Af[:, col] = np.concatenate([d_rot.ravel(), d_list.ravel()])
        for row in range(A.shape[0]):
            g = np.zeros(A.shape[0])
            g[row] = 1.0
            r = rrr.list_orientation_vjp(L, dt, now, mt, mn, land=land, g_out=g[2 * N * 3:].reshape(2, M, 3), g_rot=g[:2 * N * 3].reshape(2, N, 3), **kw)
            assert r["status"] == 0
            At[:, row] = np.concatenate([r["prev"].ravel(), r["plan"].ravel()])
        # (columns of entries beyond a list's length are not perturbed by the brute force; the restatement must not read them either)
        assert np.array_equal(Af, A), (case, b)
        assert np.array_equal(At, A.T), (case, b)
        merged_entries += int(A[:, :nin].any())
        planner_entries += int(A[:, nin:].any())
        # unlike positions, the landing entry's orientation reaches the outgoing list: every entry of the merged list has exactly one source
        for c in range(2):
            for m in range(int(mn[c])):
                rows = 2 * N * 3 + (c * M + m) * 3
                assert A[rows:rows + 3].sum() == 3.0
    print(f"\nlist orientation adjoint {case}: {B} problems, previous-list entries used in {merged_entries}, planner entries used in {planner_entries}")
    if case in ("now_9", "now_22"):
        assert merged_entries == B and planner_entries == B
    if case == "first_tick":
        assert merged_entries == B and planner_entries == 0


# ---------------------------------------------------------------------------------------------------------------- ticks on the float64 oracle
def test_restated_tick_with_orientations_is_adjoint():
    """tick_jvp_rot against tick_vjp_rot on two ticks of a yawed walk solved by the float64 oracle at N = 8 -- tick 3 (the left foot in swing, landing
    inside the horizon) and tick 5 (its landing tick: the merge takes the landed contact from the previous list) -- with random directions in the state,
    the previous list's positions and orientations and the planner's orientations, and random cotangents on the state and the outgoing list's positions
    and orientations: <g, J d> = <J^T g, d> to 1e-9 relative."""
    cfg = cm.config.ergocub_gazebo_v1(8, 0.06)
    plan = cm.rollout.walking_plan(cfg, steps=4, step_length=0.1, swing=0.24, double_support=0.12, first_lift=0.06)
    _check_restated_tick_with_orientations_is_adjoint(cfg, plan, first_tick=3, which=(0, 2))


def test_restated_tick_with_orientations_is_adjoint_at_dt_01():
    """The same at N = 8, dt = 0.1 on the gait the GPU tests walk on that grid (lift-off at tick 3, landing at tick 8): tick 7 (in swing, the landing
    inside the horizon), tick 8 (the landing tick) and tick 9, whose time 9 * dt differs from the plan's 0.3 + 0.5 + 0.1 in its last bits (asserted) and at
    which the other foot lifts."""
    from tests.test_rollout_adjoint_cpu import GAIT_DT01, assert_tick_time_differs_from_the_plans
    cfg = cm.config.ergocub_gazebo_v1(8, 0.1)
    plan = cm.rollout.walking_plan(cfg, **GAIT_DT01)
    assert_tick_time_differs_from_the_plans(plan, cfg.sampling_time, 9)
    _check_restated_tick_with_orientations_is_adjoint(cfg, plan, first_tick=7, which=(0, 1, 2))


def _check_restated_tick_with_orientations_is_adjoint(cfg, plan, first_tick, which):
    for c, lst in enumerate(plan.values()):
        for m, ct in enumerate(lst):
            ct.yaw = (0.15 if c == 0 else -0.1) * (m + 1) / 2
    state0 = np.array([0.01, -0.02, 0.7, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0])
    tapes, nows, _ = _oracle_ticks(cfg, plan, state0, first_tick=first_tick, ticks=3, com_speed=0.1)
    assert 0 < tapes[0]["land"][0] <= cfg.N and tapes[2]["prev"] is not None
    L = cm.Layout(cfg.N)
    M = tapes[0]["list_t"].shape[1]
    rng = np.random.default_rng(14)
    for i in which:
        tp, now = tapes[i], nows[i]
        p = np.asarray(tp["P"])
        assert len({(c,) + tuple(np.round(srr.stage_R(L, p, c, k).ravel(), 6)) for c in range(2) for k in range(cfg.N)}) >= 3   # a yawed footstep ahead
        assert abs(srr.stage_R(L, p, 0, 0)[0, 1]) > 0.05
        RS = srr.RotSens(cfg, tp["X"], tp["P"], tp["lam_g"])
        assert RS.n is None
        d_state, d_list, d_lrot, d_prot = rng.normal(size=9), rng.normal(size=(2, M, 3)) * 0.1, rng.normal(size=(2, M, 3)), rng.normal(size=(2, M, 3))
        g_state, g_list, g_lrot = rng.normal(size=9), rng.normal(size=(2, M, 3)), rng.normal(size=(2, M, 3))
        o_state, o_list, o_lrot = rrr.tick_jvp_rot(cfg, tp, now, d_state, d_list, d_lrot, d_prot, RS=RS)
        r = rrr.tick_vjp_rot(cfg, tp, now, g_state, g_list, g_list_rot_out=g_lrot, RS=RS)
        assert r["status"] == 0 and r["rot"].any() and r["rot0"].any() and r["prev_list_rot"].any()
        assert r["plan_rot"].any() == (tp["prev"] is not None)      # (the first taped tick has no merge: its list is the planner's own)
        lhs = g_state @ o_state + (g_list * o_list).sum() + (g_lrot * o_lrot).sum()
        rhs = r["state"] @ d_state + (r["prev_list"] * d_list).sum() + (r["prev_list_rot"] * d_lrot).sum() + (r["plan_rot"] * d_prot).sum()
        gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print(f"\ntick {first_tick + i} dt = {cfg.sampling_time} land {tp['land'].tolist()}: <g, J d> = {lhs:.12e}, <J^T g, d> = {rhs:.12e}, relative gap {gap:.2e} "
              f"(bound {TICK_ADJ:.0e})")
        assert gap <= TICK_ADJ


def test_reverse_sweep_with_orientations_equals_the_forward_chain():
    """Three oracle ticks of the yawed walk (3, 4, 5: swing, landing inside the horizon, the landed contact merged).  A direction D on the planner's
    orientations enters the first tick through its list (the planner's own, entry for entry) and every later tick through the merge; pushed forwards
    through tick_jvp_rot it moves the states, and <gS, d states> equals <list_rot0 + plan_rot, D> of the restated reverse sweep to 1e-9: the
    bookkeeping behind plan_yaw.grad of rollout_differentiable."""
    cfg = cm.config.ergocub_gazebo_v1(8, 0.06)
    plan = cm.rollout.walking_plan(cfg, steps=4, step_length=0.1, swing=0.24, double_support=0.12, first_lift=0.06)
    for c, lst in enumerate(plan.values()):
        for m, ct in enumerate(lst):
            ct.yaw = (0.15 if c == 0 else -0.1) * (m + 1) / 2
    state0 = np.array([0.01, -0.02, 0.7, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0])
    tapes, nows, _ = _oracle_ticks(cfg, plan, state0, first_tick=3, ticks=3, com_speed=0.1)
    M = tapes[0]["list_t"].shape[1]
    rng = np.random.default_rng(3)
    gS = rng.normal(size=(4, 9))
    gS[0] = 0.0
    D = rng.normal(size=(2, M, 3))
    out = rrr.reverse_sweep(cfg, tapes, nows, gS)
    assert out["status"] == [0, 0, 0] and out["rot"].shape == (3, 2, cfg.N, 3) and out["plan_rot"].any() and out["list_rot0"].any()
    d_state, d_list, d_lrot, lhs = np.zeros(9), np.zeros((2, M, 3)), D, 0.0
    for i, (tp, now) in enumerate(zip(tapes, nows)):
        d_state, d_list, d_lrot = rrr.tick_jvp_rot(cfg, tp, now, d_state, d_list, d_lrot, None if i == 0 else D)
        lhs += gS[i + 1] @ d_state
    rhs = float(((out["list_rot0"] + out["plan_rot"]) * D).sum())
    gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"\nreverse sweep with orientations against the forward chain: {lhs:.12e} vs {rhs:.12e}, relative gap {gap:.2e} (bound {TICK_ADJ:.0e})")
    assert gap <= TICK_ADJ


def test_new_entry_points_are_exported_and_yaw_plan_poses_is_the_right_product():
    """The four new C-ABI symbols are in the built library; rollout.yaw_plan_poses is q (x) (cos(psi / 2), 0, 0, sin(psi / 2)) in float64 rounded to
    float32, leaves positions alone and keeps the bits of every entry whose yaw is zero (negative zeros included)."""
    import ctypes
    import torch
    lib = ctypes.CDLL(cm._capi.LIB_PATH)
    for name in ("cmpc_plant_step_jvp_rot_device", "cmpc_plant_step_vjp_rot_device", "cmpc_contacts_orientation_vjp_device", "cmpc_rollout_tick_vjp_rot_device"):
        assert hasattr(lib, name) and name in cm._capi.EXPORTS, name
    rng = np.random.default_rng(1)
    B, M = 3, 4
    pose = rng.normal(size=(B, 2, M, 7)).astype(np.float32)
    pose[..., 3:] /= np.linalg.norm(pose[..., 3:], axis=-1, keepdims=True)
    pose[0, 0, 0, 3:] = [1.0, -0.0, 0.0, -0.0]
    psi = rng.uniform(-0.2, 0.2, (B, 2, M))
    psi[0, 0, 0] = psi[1, 1, 2] = 0.0
    out = cm.rollout.yaw_plan_poses(torch.from_numpy(pose), torch.from_numpy(psi)).numpy()
    assert np.array_equal(out[..., :3], pose[..., :3])
    for idx in np.ndindex(B, 2, M):
        if psi[idx] == 0.0:
            assert out[idx].tobytes() == pose[idx].tobytes()
        else:
            ref = _quat_exp(pose[idx][3:].astype(np.float64), psi[idx] * np.array([0.0, 0.0, 1.0]))
            assert np.abs(out[idx][3:] - ref).max() <= 2.0 ** -24 and not np.array_equal(out[idx][3:], pose[idx][3:])
