"""Host checks of the roll-out tick forwards (include/cmpc.h, "the roll-out tick FORWARDS") through its float64 restatement
tests/rollout_jvp_ref.py: the list JVP is the exact transpose of the restated list adjoints, the tick JVP and the forward sweep are the transposes of
rollout_rot_ref.tick_vjp_rot / reverse_sweep on oracle-solved ticks of a yawed walk, and the forward sweep of a standing robot under a push matches central
differences of the oracle roll-out.  tests/test_gpu_rollout_jvp.py holds the device kernels to the same restatement.  Every bound is one the project
already has, imported."""
import os
import re

import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import PlannedContact, pack_lists
from tests import rollout_adjoint_ref as rar
from tests import rollout_jvp_ref as rjr
from tests import rollout_rot_ref as rrr
from tests import sens_model_ref as smr, snap_ref
from tests import sens_rot_ref as srr
from tests.test_contacts_cpu import _random_walks
from tests.test_gpu_rollout_adjoint import F64
from tests.test_rollout_adjoint_cpu import GAIT_DT01, _list_forward, _oracle_ticks, assert_tick_time_differs_from_the_plans
from tests.test_rollout_rot_adjoint_cpu import TICK_ADJ
from tests.test_sensitivity_cpu import FD_CLEAN


def _gap(lhs, rhs):
    return abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)


@pytest.mark.parametrize("case", ["now_9", "now_22", "first_tick", "failed_merge", "snapped"])
def test_list_jvp_is_the_exact_transpose_of_the_restated_list_adjoints(case):
    """<g, J d> = <J^T g, d> with J d from rollout_jvp_ref.list_jvp (phase 3) and J^T g from rar.list_position_vjp (phase 3) plus
    rrr.list_orientation_vjp, every direction and cotangent group random at once, on lists the oracle's merge -> sample produced: to F64.  The maps
    are 0/1 incidences, so what remains is the rounding of two float64 dot products.  A failed merge gives zeros and status 5; the landing entry (nx >= 0:
    the overwritten one) is exercised in every problem of the snapped case, one tick after its first lift-off -- asserted."""
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    N, dt = cfg.N, cfg.sampling_time
    L = cm.Layout(N)
    B = 6
    snap = case == "snapped"
    walks = _random_walks(cfg, B, 17, t_end=3.0)
    if not snap:     # times on the grid (what forceSampleTime leaves); the snapped case keeps the random off-grid times
        for w in walks:
            for lst in w.values():
                for ct in lst:
                    ct.activation_time = round(ct.activation_time / dt) * dt
                    ct.deactivation_time = ct.deactivation_time if ct.deactivation_time >= 1e9 else round(ct.deactivation_time / dt) * dt
    t, pose, n = pack_lists(cfg, walks, max_contacts=12)
    M = t.shape[2]
    rng = np.random.default_rng(11)
    worst, landings = 0.0, 0
    for b in range(B):
        ts = snap_ref.snap_lists(dt, t[b][None], n[b][None])[0][0] if snap else t[b]
        lift = min(ts[c, 0, 1] for c in range(2))
        now = dt * dict(now_9=9, now_22=22, first_tick=0, failed_merge=9, snapped=round((lift + dt) / dt))[case]
        d = {k: rng.normal(size=(2, M, 3)) for k in ("prev", "prev_rot", "plan", "plan_rot")}
        d_x = rng.normal(size=L.nx)
        g_list, g_lrot, g_p, g_rot = rng.normal(size=(2, M, 3)), rng.normal(size=(2, M, 3)), rng.normal(size=L.np), rng.normal(size=(2, N, 3))
        if case == "failed_merge":
            kw = dict(plan=(t[b] + 50.0, n[b]), prev=(t[b], n[b]), ok=False)
            f = rjr.list_jvp(L, dt, now, t[b], n[b], np.zeros(2, int), d_prev=d["prev"], d_prev_rot=d["prev_rot"], d_plan=d["plan"],
                             d_plan_rot=d["plan_rot"], d_x=d_x, **kw)
            assert f["status"] == 5 and not any(f[k].any() for k in ("list", "list_rot", "p", "rot"))
            continue
        plan = None if case == "first_tick" else (t[b], pose[b], n[b])
        prev = (ts if plan is not None else t[b], pose[b].astype(np.float64), n[b])
        _, _, _, land, mt, mn = _list_forward(cfg, now, plan, prev, np.zeros((2, 3)), snap)
        kw = dict(plan=None if plan is None else (plan[0], plan[2]), prev=None if plan is None else (prev[0], prev[2]), force_sample_time=snap)
        f = rjr.list_jvp(L, dt, now, mt, mn, land, d_prev=d["prev"], d_prev_rot=d["prev_rot"], d_plan=d["plan"], d_plan_rot=d["plan_rot"], d_x=d_x, **kw)
        vp = rar.list_position_vjp(L, dt, now, mt, mn, land, g_out=g_list, g_p=g_p, **kw)
        vr = rrr.list_orientation_vjp(L, dt, now, mt, mn, land=land, g_out=g_lrot, g_rot=g_rot, **kw)
        assert f["status"] == vp["status"] == vr["status"] == 0
        lhs = (g_list * f["list"]).sum() + (g_lrot * f["list_rot"]).sum() + g_p @ f["p"] + (g_rot * f["rot"]).sum()
        rhs = ((vp["prev"] * d["prev"]).sum() + (vp["plan"] * d["plan"]).sum() + vp["x"] @ d_x + (vr["prev"] * d["prev_rot"]).sum() +
               (vr["plan"] * d["plan_rot"]).sum())
        worst = max(worst, _gap(lhs, rhs))
        landings += sum(1 for c in range(2) if f["nx"][c] >= 0)
        for c in range(2):      # the overwritten entry holds the solution's direction and nothing else; entries beyond the list are zero
            if f["nx"][c] >= 0:
                assert np.array_equal(f["list"][c, f["nx"][c]], d_x[L.pos[c] + 3 * land[c]:L.pos[c] + 3 * land[c] + 3])
            assert not f["list"][c, mn[c]:].any() and not f["list_rot"][c, mn[c]:].any()
        if plan is None:        # the first tick: the planner's directions are not read
            f2 = rjr.list_jvp(L, dt, now, mt, mn, land, d_prev=d["prev"], d_prev_rot=d["prev_rot"], d_x=d_x, **kw)
            assert all(np.array_equal(f[k], f2[k]) for k in ("list", "list_rot", "p", "rot"))
    print(f"\nlist JVP against the restated adjoints, {case}: worst gap {worst:.2e} (bound {F64:.0e}), landing entries overwritten {landings}")
    assert worst <= F64
    if case == "snapped":       # (one tick after the first lift-off: a foot of every problem is in swing and lands inside the horizon)
        assert landings >= B


def _yawed_ticks(dt=0.06):
    """three oracle ticks of a yawed walk at N = 8: ticks 3, 4, 5 of the short-stepping plan at dt = 0.06; at dt = 0.1 ticks 7, 8, 9 of the gait the GPU
    tests walk on that grid (lift-off at tick 3, landing at tick 8; 9 * dt differs from the plan's 0.3 + 0.5 + 0.1 in its last bits -- asserted)"""
    cfg = cm.config.ergocub_gazebo_v1(8, dt)
    if dt == 0.06:
        plan, first = cm.rollout.walking_plan(cfg, steps=4, step_length=0.1, swing=0.24, double_support=0.12, first_lift=0.06), 3
    else:
        plan, first = cm.rollout.walking_plan(cfg, **GAIT_DT01), 7
        assert_tick_time_differs_from_the_plans(plan, dt, 9)
    for c, lst in enumerate(plan.values()):
        for m, ct in enumerate(lst):
            ct.yaw = (0.15 if c == 0 else -0.1) * (m + 1) / 2
    state0 = np.array([0.01, -0.02, 0.7, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0])
    tapes, nows, _ = _oracle_ticks(cfg, plan, state0, first_tick=first, ticks=3, com_speed=0.1)
    return cfg, tapes, nows


@pytest.fixture(scope="module")
def yawed_ticks():
    return _yawed_ticks()


@pytest.fixture(scope="module")
def yawed_ticks_dt01():
    return _yawed_ticks(0.1)


def _directions(rng, cfg, M):
    L = cm.Layout(cfg.N)
    return dict(state=rng.normal(size=9), list=rng.normal(size=(2, M, 3)) * 0.1, list_rot=rng.normal(size=(2, M, 3)), plan=rng.normal(size=(2, M, 3)) * 0.1,
                plan_rot=rng.normal(size=(2, M, 3)), wrench=rng.normal(size=(cfg.N, 6)), model=rng.normal(size=34) * smr.theta_of(cfg).clip(1e-2) * 0.1,
                p=rng.normal(size=L.np) * 0.1)


def test_restated_tick_jvp_is_the_transpose_of_the_restated_tick_vjp(yawed_ticks):
    """<g, J d> = <J^T g, d> of one whole tick with all eight input groups (state, previous list positions / orientations, planner positions /
    orientations, wrench, model, extra p) and all four output groups (state', list, list orientations, x) random at once, on tick 3 (swing, landing inside
    the horizon) and tick 5 (the landing tick: the merge takes the landed contact) of the yawed walk on the float64 oracle: to TICK_ADJ."""
    _check_restated_tick_jvp_is_the_transpose(yawed_ticks, (0, 2), 3)


def test_restated_tick_jvp_and_forward_sweep_are_the_transposes_at_dt_01(yawed_ticks_dt01):
    """The two tests around this one at N = 8, dt = 0.1, on ticks 7 (in swing, the landing inside the horizon), 8 (the landing tick) and 9 (a tick whose
    time differs from the plan's in its last bits, at which the other foot lifts) of the yawed walk on the float64 oracle: tick JVP against tick VJP on
    each of the three, the forward sweep against the reverse sweep over the three, to TICK_ADJ."""
    _check_restated_tick_jvp_is_the_transpose(yawed_ticks_dt01, (0, 1, 2), 7)
    _check_forward_sweep_is_the_contraction(yawed_ticks_dt01)


def _check_restated_tick_jvp_is_the_transpose(ticks, which, first_tick):
    cfg, tapes, nows = ticks
    L = cm.Layout(cfg.N)
    M = tapes[0]["list_t"].shape[1]
    rng = np.random.default_rng(23)
    assert 0 < tapes[0]["land"][0] <= cfg.N and tapes[2]["prev"] is not None
    for i in which:
        tp, now = tapes[i], nows[i]
        RS = srr.RotSens(cfg, tp["X"], tp["P"], tp["lam_g"])
        assert RS.n is None
        d = _directions(rng, cfg, M)
        g_state, g_list, g_lrot, g_x = rng.normal(size=9), rng.normal(size=(2, M, 3)), rng.normal(size=(2, M, 3)), rng.normal(size=L.nx) * 0.1
        f = rjr.tick_jvp(cfg, tp, now, d["state"], d["list"], d["list_rot"], d["plan"], d["plan_rot"], d["wrench"], d["model"], d["p"], RS=RS)
        r = rrr.tick_vjp_rot(cfg, tp, now, g_state, g_list, g_x, g_list_rot_out=g_lrot, RS=RS)
        assert f["status"] == r["status"] == 0 and f["rot"].any() and f["x"].any()
        lhs = g_state @ f["state"] + (g_list * f["list"]).sum() + (g_lrot * f["list_rot"]).sum() + g_x @ f["x"]
        terms = dict(state=r["state"] @ d["state"], list=(r["prev_list"] * d["list"]).sum(), list_rot=(r["prev_list_rot"] * d["list_rot"]).sum(),
                     plan=(r["plan"] * d["plan"]).sum(), plan_rot=(r["plan_rot"] * d["plan_rot"]).sum(), wrench=(r["wrench"] * d["wrench"]).sum(),
                     model=r["model"] @ d["model"], p=r["p"] @ d["p"])
        rhs = sum(terms.values())
        gap = _gap(lhs, rhs)
        print(f"\ntick {first_tick + i} dt = {cfg.sampling_time} land {tp['land'].tolist()}: <g, J d> = {lhs:.12e}, <J^T g, d> = {rhs:.12e}, relative gap {gap:.2e} "
              f"(bound {TICK_ADJ:.0e}); "
              "terms " + " ".join(f"{k} {v:.2e}" for k, v in terms.items()))
        assert gap <= TICK_ADJ
        merge = tp["prev"] is not None
        assert all(terms[k] != 0 for k in terms if merge or k not in ("plan", "plan_rot"))      # every group takes part


def test_restated_forward_sweep_is_the_contraction_of_the_restated_reverse_sweep(yawed_ticks):
    """Three oracle ticks of the yawed walk (3, 4, 5): sum_i <gS_i, d state_i> + <gX_i, d x_i> of rollout_jvp_ref.forward_sweep equals the contraction of
    rrr.reverse_sweep's state0, list0, list_rot0, plan, plan_rot, models and wrench with the directions, to TICK_ADJ."""
    _check_forward_sweep_is_the_contraction(yawed_ticks)


def _check_forward_sweep_is_the_contraction(ticks):
    cfg, tapes, nows = ticks
    L = cm.Layout(cfg.N)
    T = len(tapes)
    M = tapes[0]["list_t"].shape[1]
    rng = np.random.default_rng(5)
    gS, gX = rng.normal(size=(T + 1, 9)), rng.normal(size=(T, L.nx)) * 0.1
    d = _directions(rng, cfg, M)
    dw = rng.normal(size=(T, cfg.N, 6))
    out = rrr.reverse_sweep(cfg, tapes, nows, gS, gX)
    f = rjr.forward_sweep(cfg, tapes, nows, d["state"], d["list"], d["list_rot"], d["plan"], d["plan_rot"], None, d["model"], dw)
    assert out["status"] == [0] * T and f["status"] == [0] * T
    lhs = (gS * f["states"]).sum() + (gX * f["X"]).sum()
    rhs = (out["state0"] @ d["state"] + (out["list0"] * d["list"]).sum() + (out["list_rot0"] * d["list_rot"]).sum() + (out["plan"] * d["plan"]).sum() +
           (out["plan_rot"] * d["plan_rot"]).sum() + out["models"] @ d["model"] + (out["wrench"] * dw).sum())
    gap = _gap(lhs, rhs)
    print(f"\nforward sweep against the reverse sweep over three ticks at dt = {cfg.sampling_time}: {lhs:.12e} vs {rhs:.12e}, relative gap {gap:.2e} (bound {TICK_ADJ:.0e})")
    assert gap <= TICK_ADJ


def test_forward_sweep_of_a_standing_robot_under_a_push_matches_oracle_differences():
    """The forward counterpart of test_closed_loop_finite_difference_of_a_standing_robot_under_a_push (tests/test_rollout_adjoint_cpu.py), its case and
    its bound: three ticks standing under a push, d state_3 / d (state_0, push) column by column from the restated forward sweep against central
    differences of the same float64 oracle loop, each group relative to its largest entry, <= 3 x FD_CLEAN."""
    cfg = cm.config.ergocub_gazebo_v1(8, 0.06)
    names = [c.contact_name for c in cfg.contacts]
    stand = {names[0]: [PlannedContact(0.0, 1e9, (0.0, 0.08, 0.0))], names[1]: [PlannedContact(0.0, 1e9, (0.0, -0.08, 0.0))]}
    state0 = np.array([0.01, -0.005, 0.7, 0.02, 0.01, 0.0, 0.0, 0.0, 0.0])
    push = np.array([0.2, -0.15, 0.0])

    def run(s0, pu):
        return _oracle_ticks(cfg, stand, s0, first_tick=0, ticks=3, push=pu, push_ticks=2)
    tapes, nows, _ = run(state0, push)
    pk = [tp["push_knots"] for tp in tapes]
    h = 1e-5
    sens = [srr.RotSens(cfg, tp["X"], tp["P"], tp["lam_g"]) for tp in tapes]
    assert all(RS.S.weak == 0 for RS in sens)
    Js = np.array([rjr.forward_sweep(cfg, tapes, nows, d_state0=e, sens=sens)["states"][3] for e in np.eye(9)]).T
    Jp = np.array([rjr.forward_sweep(cfg, tapes, nows, d_push=e, push_knots=pk, sens=sens)["states"][3] for e in np.eye(3)]).T
    fd_s = np.array([(run(state0 + h * e, push)[2] - run(state0 - h * e, push)[2]) / (2 * h) for e in np.eye(9)]).T
    fd_p = np.array([(run(state0, push + h * e)[2] - run(state0, push - h * e)[2]) / (2 * h) for e in np.eye(3)]).T
    gap_s = np.abs(Js - fd_s).max() / np.abs(fd_s).max()
    gap_p = np.abs(Jp - fd_p).max() / np.abs(fd_p).max()
    print(f"\nforward sweep over three standing ticks against oracle differences: state0 {gap_s:.2e} push {gap_p:.2e} (bound {3 * FD_CLEAN:.0e})")
    assert gap_s <= 3 * FD_CLEAN and gap_p <= 3 * FD_CLEAN


def test_forward_entry_points_are_declared_exported_and_mirrored():
    """The three new C-ABI symbols are declared in include/cmpc.h, listed in _capi.EXPORTS and present in the built library, and the two ctypes
    structs have the header's fields in the header's order (all pointers)."""
    import ctypes
    names = ("cmpc_plant_step_jvp_cols_device", "cmpc_contacts_jvp_device", "cmpc_rollout_tick_jvp_device")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmpc.h")).read()
    lib = ctypes.CDLL(cm._capi.LIB_PATH)
    for name in names:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in cm._capi.EXPORTS and hasattr(lib, name), name
    for struct, mirror in (("cmpc_tick_dirs", "CmpcTickDirs"), ("cmpc_tick_dirs_out", "CmpcTickDirsOut")):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"\*\s*(\w+)\s*;", body)
        cls = getattr(cm._capi, mirror)
        assert [f[0] for f in cls._fields_] == fields and len(fields) >= 6, (struct, fields)
        assert all(f[1] is ctypes.c_void_p for f in cls._fields_)
