"""GPU: the roll-out tick and its derivatives at the horizons, sampling times and weights the shipped robots run, beside the one configuration
(N = 20, dt = 0.06, ergoCubGazeboV1) every other roll-out test uses:

  n13    ergoCubGazeboV1's weights at N = 13, dt = 0.1, the gait synthetic.gait_cycle walks on that grid (swing 0.5 s, double support 0.1 s, first
         lift-off 0.3 s), 12 ticks: lift-off at tick 3, landing at tick 8
  n22    the same weights at N = 22, dt = 0.06, the default gait, 20 ticks: lift-off at tick 6, landing at tick 14
  sn000  tests/golden/ini/ergoCubSN000.ini (N = 13, dt = 0.1, w_pos = 50, its own corners and boxes), the gait of n13, pushed with up to 150 N: landings
         sit on faces of their bounding boxes, so the step adjustment copies a constrained landing into the list

B = 8 everywhere, pushed for three ticks (the walk of tests/test_gpu_rollout_adjoint.py, `_walk`).  At N = 13 and N = 22 the solve inside the tick, the
multiplier export and the sensitivity workspaces take the run-time-N kernels; at dt = 0.1 the tick times i * dt and the plan's times (sums such as
first_lift + swing + double_support) differ in their last bits, which is what CMPC_TIME_EPS (csrc/cmpc_contacts.h) is there for.

Every assertion is one an existing roll-out test makes at N = 20, with its bound: REF, ADJ, F64 and ULP32 of tests/test_gpu_rollout_adjoint.py and
parity.limits, imported.  Measured values: profiles/rollout_horizons.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import force_sample_time, pack_lists, update_contact_phase_list
from oracle import oracle_lib as ol, problem_nlp
from tests import parity
from tests import rollout_jvp_ref as rjr
from tests import rollout_rot_ref as rrr
from tests import sens_rot_ref as srr
from tests.test_gpu_gait_cycle import _assert_rows_within
from tests.test_gpu_rollout_adjoint import ADJ, F64, GROUPS, REF, ULP32, _check_list_adjoint, _check_plant_kernels, _host_tape, _rel, _walk
from tests.test_gpu_rollout_jvp import IN_GROUPS, OUT_GROUPS, _check_list_jvp, _check_plant_columns, _cu, _gap, _tick_directions, _tick_jvp
from tests.test_gpu_rollout_rot_adjoint import ROT_GROUPS, _check_list_orientation

pytestmark = pytest.mark.gpu

B = 8
GAIT_DT01 = dict(swing=0.5, double_support=0.1, first_lift=0.3)       # (synthetic.gait_cycle's gait on the grid of dt = 0.1)
CONFIGS = ("n13", "n22", "sn000")
# ticks of the walk, the ticks differentiated (before lift-off, in swing, the landing tick, after it) and the largest push in newton
WALKS = dict(n13=(12, (2, 5, 8, 10), 20.0), n22=(20, (2, 8, 14, 18), 20.0), sn000=(12, (2, 5, 8, 10), 150.0))
MIN_FACE_PAIRS = 8
_walks, _derivs = {}, {}


def _config(name):
    """-> (cfg, plan or None for the default gait)"""
    if name == "n22":
        return cm.config.ergocub_gazebo_v1(22, 0.06), None
    if name == "n13":
        cfg = cm.config.ergocub_gazebo_v1(13, 0.1)
    else:
        ini = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ini", "ergoCubSN000.ini")
        cfg = cm.config.from_ini(open(ini).read())
        assert (cfg.N, cfg.sampling_time) == (13, 0.1)
    return cfg, cm.rollout.walking_plan(cfg, **GAIT_DT01)


def _taped(name):
    """the configuration's taped walk on the native tick, run once per session and left unchanged: (cfg, plan, roll-out, record)"""
    if name not in _walks:
        cfg, plan = _config(name)
        ticks, _, push = WALKS[name]
        _, ro, rec = _walk(B, ticks, cfg=cfg, plan=plan, push_newton=push)
        assert ro.native_tick and len(rec["tape"]["ticks"]) == ticks and all(rec["merge_ok"])
        _walks[name] = (cfg, plan, ro, rec)
    return _walks[name]


# ---------------------------------------------------------------------------------------------------------------- 1. the forward tick
@pytest.mark.parametrize("name", CONFIGS)
def test_native_tick_is_the_chain_of_entry_points_and_every_tick_matches_the_oracle(name):
    """The assertions of test_native_tick_is_the_seven_entry_points_chained_bit_for_bit (tests/test_gpu_rollout.py) and of
    test_the_rollouts_own_ticks_match_the_oracle (tests/test_gpu_gait_cycle.py) on this configuration's walk: every record of the native tick equals the
    seven entry points chained, bit for bit; every tick's own P solved cold by the float64 oracle holds the tick's X within parity.limits, tick by tick;
    where the oracle has a solution the device has one, and where the device reports one the oracle has one (never status 3).  sn000: at least 8 (tick,
    problem) pairs of the oracle's solutions have a landing on a face of its box, and the device's landing sits on the same faces (the rule of
    tests/test_gpu_robots.py: 1e-5 m inside the horizon, the footstep limit for a foot still in the air at its end)."""
    cfg, plan, ro, rec = _taped(name)
    N = cfg.N
    ticks, _, push = WALKS[name]
    _, ro2, rec2 = _walk(B, ticks, cfg=cfg, plan=plan, push_newton=push, tape=False, native_tick=False)
    assert not ro2.native_tick and len(rec["com"]) == ticks == len(rec2["com"])
    for key in ("com", "zmp", "land", "landing_offset"):
        assert np.array_equal(np.stack(rec[key]), np.stack(rec2[key])), (name, key)
    assert rec["iterations_max"] == rec2["iterations_max"] and rec["iterations_mean"] == rec2["iterations_mean"]
    ro2.solver.close()
    assert len(np.unique(np.stack(rec["land"]))) > 3            # the landing knots moved through the horizon
    tape = rec["tape"]["ticks"]
    P = np.stack([tk["P"].cpu().numpy() for tk in tape])          # [ticks, B, n_p]
    X = np.stack([tk["X"].cpu().numpy() for tk in tape])
    info = np.stack([tk["info"].cpu().numpy() for tk in tape])
    P64 = P.reshape(ticks * B, -1).astype(np.float64)
    Xr, infr = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P64, cm.layout.cold_start(N, P64), ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=16)
    Xr, infr = Xr.reshape(ticks, B, -1), infr.reshape(ticks, B, -1)
    dev_ok, ora_ok = info[:, :, 5] == 0, infr[:, :, 5] == 0
    lim = parity.limits(N)
    rows = []
    print(f"\n{name}: roll-out N = {N} dt = {cfg.sampling_time}, B = {B}: per tick, worst error against the oracle's cold solve of the tick's own P")
    print("tick  iters  com      dcom     h        pos      force0   forces")
    for i in range(ticks):
        sel = np.nonzero(dev_ok[i] & ora_ok[i])[0]
        if sel.size == 0:
            continue
        w = parity.worst_errors(N, P[i][sel], X[i][sel], Xr[i][sel])
        rows.append(((i, "tick"), w))
        it = info[i][:, 0].astype(int)
        print(f"{i:4d}  {it.min():2d}-{it.max():2d}  " + " ".join(f"{w[k]:.2e}" for k in ("com", "dcom", "h", "pos", "force0", "forces")))
    print(f"{name}: forward ticks against the oracle, worst of {len(rows)} ticks: " +
          " ".join(f"{k} {max(w[k] for _, w in rows):.2e} (limit {lim[k]:.0e})" for k in lim) +
          f"; oracle solved {int(ora_ok.sum())}/{ticks * B}, device {int(dev_ok.sum())}/{ticks * B}")
    assert (infr[:, :, 5][dev_ok] == 0).all() and not (infr[:, :, 5] == 3).any(), infr[:, :, 5]
    assert dev_ok[ora_ok].all(), (np.argwhere(ora_ok & ~dev_ok), info[:, :, 5][ora_ok & ~dev_ok])
    assert len(rows) == ticks
    _assert_rows_within(N, rows, f"{name} roll-out ticks")
    if name != "sn000":
        return
    pairs = x_pairs = 0
    missing = []
    for i in range(ticks):
        for b in np.nonzero(ora_ok[i])[0]:
            f = parity.box_faces(N, P[i, b], Xr[i, b])
            if not f:
                continue
            pairs += 1
            x_pairs += int(any(r[2] == 0 for r in f))
            near = parity.box_faces(N, P[i, b], X[i, b], tol=1e-5) | {r for r in parity.box_faces(N, P[i, b], X[i, b], tol=lim["pos"]) if r[1] == N - 1}
            if f - near:
                missing.append((i, int(b), sorted(f), sorted(f - near)))
    print(f"sn000: (tick, problem) pairs of the oracle's solutions with a landing on a box face: {pairs} of {int(ora_ok.sum())} "
          f"(required {MIN_FACE_PAIRS}); on a face in x, +-0.01 m from the nominal footstep: {x_pairs}; device landings off the oracle's faces: {len(missing)}")
    assert pairs >= MIN_FACE_PAIRS, pairs
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------- 2. contact kernels at knife-edge ticks
def _ns(t):
    return int(round(float(t) * 1e9))


def _ns_active(t_ns, now_ns):
    """getActiveContact on integer nanoseconds: activation <= t < deactivation, or -1"""
    for m, (a, d) in enumerate(t_ns):
        if a <= now_ns < d:
            return m
    return -1


def _ns_next(t_ns, now_ns):
    """getNextContact on integer nanoseconds: the first contact that activates after t, or -1"""
    for m, (a, _) in enumerate(t_ns):
        if a > now_ns:
            return m
    return -1


def _ns_snap(t, dt_ns):
    """forceSampleTime's rule (include/cmpc.h): nearest multiple of dt from time 0 on integer nanoseconds, ties to the later one; a time on the grid and
    the 1e9 s sentinel keep their bits"""
    t_ns = _ns(t)
    if abs(t) >= 1e9 or t_ns % dt_ns == 0:
        return t
    return float(((2 * t_ns + dt_ns) // (2 * dt_ns)) * dt_ns) * 1e-9


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("N,dt,edge_ticks", [(13, 0.1, (3, 9, 14)), (22, 0.06, (44, 46, 54, 56))])
def test_contact_kernels_at_ticks_whose_time_differs_from_the_plans_in_the_last_bits(N, dt, edge_ticks):
    """force_sample_time, merge, sample and adjust on the device at now = i * dt for ticks at which a time of a ten-step plan equals i * dt on the
    nanosecond grid and differs from it as a double (asserted first): at dt = 0.1 the tick time is the larger, at dt = 0.06 the smaller.  What is
    expected -- snapped times, the merged lists' lengths, times and positions, Gamma and the owner of every stage (through the nominal positions),
    currentPos, the landing knots, the adjusted lists -- is computed here on integer nanoseconds (round(t * 1e9)), the reference's clock, not taken from
    the library.  Problems 0, 2, 4, 6 carry the plan's own times; 1, 3, 5 the plan moved 13 ms off the grid and 7 by half a sampling time (a tie), so
    that the snapped times, a third spelling of the same instants, go through the merge and the sampling too.  The host entry points then agree with the
    device bit for bit."""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, dt)
    L = cm.Layout(N)
    dt_ns = _ns(dt)
    gait = GAIT_DT01 if dt == 0.1 else {}
    lists = [cm.rollout.walking_plan(cfg, steps=10, **gait) for _ in range(B)]
    grid_times = sorted({t for lst in lists[0].values() for ct in lst for t in (ct.activation_time, ct.deactivation_time) if t < 1e9})
    assert len(grid_times) >= 20
    for i in edge_ticks:
        same = [t for t in grid_times if _ns(t) == i * dt_ns]
        assert len(same) == 1 and same[0] != i * dt, (i, same)       # the edge is there: one instant, two doubles
        print(f"\nN = {N} dt = {dt}: tick {i}: i * dt - plan time = {i * dt - same[0]:+.2e}")
    for b, shift in ((1, 0.013), (3, 0.013), (5, 0.013), (7, dt / 2)):
        for lst in lists[b].values():
            for ct in lst:
                ct.activation_time += shift
                ct.deactivation_time += shift if ct.deactivation_time < 1e9 else 0.0
    M = 12
    plan_t, plan_pose, plan_n = pack_lists(cfg, lists, max_contacts=M)
    want_t = plan_t.copy()
    for idx in np.ndindex(B, 2, M, 2):
        if idx[2] < plan_n[idx[0], idx[1]]:
            want_t[idx] = _ns_snap(plan_t[idx], dt_ns)
    assert np.array_equal(want_t[0::2], plan_t[0::2]) and (want_t[1::2] != plan_t[1::2]).any()
    assert all(_ns(want_t[7, c, m, j]) == _ns(want_t[0, c, m, j]) + (dt_ns if want_t[0, c, m, j] < 1e9 else 0)       # (the tie went to the later knot)
               for c in range(2) for m in range(plan_n[7, c]) for j in range(2))
    mpc_pose = plan_pose.copy()
    mpc_pose[..., :3] += np.random.default_rng(2).uniform(-0.01, 0.01, mpc_pose[..., :3].shape).astype(np.float32)
    X = np.random.default_rng(0).normal(size=(B, L.nx)).astype(np.float32)
    up = np.array([c.bounding_box_upper_limit for c in cfg.contacts], np.float32)
    lo = np.array([c.bounding_box_lower_limit for c in cfg.contacts], np.float32)
    s = cm.BatchSolver(cfg, B)
    dev = lambda t: tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in t)
    d_t, d_pose, d_n = dev((plan_t, plan_pose, plan_n))
    snapped, ok_snap = s.contacts_force_sample_time_device(d_t, d_n)
    torch.cuda.synchronize()
    snap_t = snapped.cpu().numpy()
    assert ok_snap.cpu().numpy().all()
    for idx in np.ndindex(B, 2):
        m = plan_n[idx]
        assert np.array_equal(snap_t[idx][:m], want_t[idx][:m]), (idx, snap_t[idx][:m], want_t[idx][:m])
    h_snap, h_ok = force_sample_time(dt, plan_t, plan_n)
    assert h_ok.all() and all(np.array_equal(h_snap[idx][:plan_n[idx]], snap_t[idx][:plan_n[idx]]) for idx in np.ndindex(B, 2))
    t_ns = [[[(_ns(snap_t[b, c, m, 0]), _ns(snap_t[b, c, m, 1])) for m in range(plan_n[b, c])] for c in range(2)] for b in range(B)]
    lifted = landed = 0
    for i in edge_ticks:
        now, now_ns = i * dt, i * dt_ns
        d_mpc = (snapped, torch.from_numpy(mpc_pose).cuda(), d_n)
        merged, ok = s.contacts_merge_device(now, (snapped, d_pose, d_n), d_mpc)
        dP = torch.full((B, L.np), 3.0, dtype=torch.float32, device="cuda")
        land = s.contacts_sample_device(now, merged, dP)
        torch.cuda.synchronize()
        mt, mp, mn = (a.cpu().numpy() for a in merged)
        Ph, lh = dP.cpu().numpy(), land.cpu().numpy()
        before = mp.copy()
        s.contacts_adjust_device(now, torch.from_numpy(X).cuda(), land, merged)
        torch.cuda.synchronize()
        after = merged[1].cpu().numpy()
        assert ok.cpu().numpy().all()
        for b in range(B):
            for c in range(2):
                src = t_ns[b][c]
                ma, first = _ns_active(src, now_ns), _ns_next(src, now_ns)
                assert ma >= 0 or first >= 0
                # the merge: the current contact with the previous list's pose and the planner's times, then every future contact of the planner
                rows = ([("mpc", ma)] if ma >= 0 else []) + ([("plan", m) for m in range(first, len(src))] if first >= 0 else [])
                assert mn[b, c] == len(rows), (i, b, c, mn[b, c], len(rows))
                for m, (who, j) in enumerate(rows):
                    assert np.array_equal(mt[b, c, m], snap_t[b, c, j]), (i, b, c, m)
                    assert np.array_equal(before[b, c, m], (mpc_pose if who == "mpc" else plan_pose)[b, c, j]), (i, b, c, m)
                # the sampling of the merged list
                lst = [(_ns(mt[b, c, m, 0]), _ns(mt[b, c, m, 1])) for m in range(mn[b, c])]
                gam, owner = [], []
                for k in range(N):
                    a = _ns_active(lst, now_ns + k * dt_ns)
                    nx = _ns_next(lst, now_ns + k * dt_ns)
                    gam.append(a >= 0)
                    owner.append(a if a >= 0 else (nx if nx >= 0 else len(lst) - 1))
                want_land, prev_act = -1, True
                for k in range(N):
                    if gam[k] and not prev_act and want_land < 0:
                        want_land = k
                    prev_act = gam[k]
                if not prev_act and want_land < 0:
                    want_land = N
                assert np.array_equal(Ph[b, L.p_gam[c]:L.p_gam[c] + N], np.array(gam, np.float32)), (i, b, c, Ph[b, L.p_gam[c]:L.p_gam[c] + N], gam)
                assert lh[b, c] == want_land, (i, b, c, lh[b, c], want_land)
                nominal = np.stack([before[b, c, owner[0], :3]] + [before[b, c, o, :3] for o in owner])
                assert np.array_equal(Ph[b, L.p_nom[c]:L.p_nom[c] + 3 * (N + 1)].reshape(N + 1, 3), nominal), (i, b, c)
                assert np.array_equal(Ph[b, L.p_cur[c]:L.p_cur[c] + 3], before[b, c, owner[0], :3])
                assert np.array_equal(Ph[b, L.p_up[c]:L.p_up[c] + 3 * N].reshape(N, 3), np.tile(up[c], (N, 1)))
                assert np.array_equal(Ph[b, L.p_lo[c]:L.p_lo[c] + 3 * N].reshape(N, 3), np.tile(lo[c], (N, 1)))
                lifted += int(not gam[0])
                # the step adjustment: the next contact takes x.pos[land]
                want = before[b, c].copy()
                nx = _ns_next(lst, now_ns)
                if 0 <= want_land <= N and nx >= 0:
                    want[nx, :3] = X[b, L.pos[c] + 3 * want_land:L.pos[c] + 3 * want_land + 3]
                    landed += 1
                assert np.array_equal(after[b, c], want), (i, b, c)
        assert (Ph[:, L.p_com0:] == 3.0).all()                        # state, reference and wrench rows are not the sampler's
        # the host entry points: the same bits
        (ht, hp, hn), hok = update_contact_phase_list(now, (snap_t, plan_pose, plan_n), (snap_t, mpc_pose, plan_n))
        assert hok.all() and np.array_equal(hn, mn)
        for idx in np.ndindex(B, 2):
            assert np.array_equal(ht[idx][:mn[idx]], mt[idx][:mn[idx]]) and np.array_equal(hp[idx][:mn[idx]], before[idx][:mn[idx]]), (i, idx)
        hP, hland = np.full((B, L.np), 3.0, np.float32), np.zeros((B, 2), np.int32)
        assert s._lib.cmpc_contacts_sample(N, dt, B, M, now, _ptr(mt), _ptr(before), _ptr(mn), _ptr(up), _ptr(lo), _ptr(hP), _ptr(hland)) == 0
        assert np.array_equal(hP, Ph) and np.array_equal(hland, lh)
        hadj = before.copy()
        assert s._lib.cmpc_contacts_adjust(N, B, M, now, _ptr(X), _ptr(lh), _ptr(mt), _ptr(hadj), _ptr(mn)) == 0
        assert np.array_equal(hadj, after)
    print(f"N = {N} dt = {dt}: knife-edge ticks {edge_ticks}: feet in the air at stage 0: {lifted}, landing positions written: {landed}, of "
          f"{len(edge_ticks) * B * 2} (tick, problem, foot) triples; every expected value on integer nanoseconds, host == device")
    assert lifted > 0 and landed > 0
    s.close()


# ---------------------------------------------------------------------------------------------------------------- 3. plant-step derivatives
HORIZONS = [(13, 0.1), (22, 0.06)]


@pytest.mark.parametrize("N,dt", HORIZONS)
def test_plant_kernels_match_the_restatement_at_this_horizon(N, dt):
    """test_plant_jvp_vjp_kernels_match_the_restatement (F64 on the double groups, one rounding on the float32 groups, ADJ on the adjoint identity,
    bit-identity across batch position and size) and test_plant_columns_are_bit_equal_to_the_single_column_entry (k = 3) at this horizon: the plant reads
    knot 0 of x and p, whose offsets move with N."""
    cfg = cm.config.ergocub_gazebo_v1(N, dt)
    _check_plant_kernels(cfg)
    _check_plant_columns(cfg)


# ---------------------------------------------------------------------------------------------------------------- 4. list adjoints and list JVP
@pytest.mark.parametrize("N,dt,first_tick,now_k,snap", [(13, 0.1, False, 4, False), (13, 0.1, False, 5, True), (13, 0.1, True, 0, False),
                                                        (22, 0.06, False, 9, False), (22, 0.06, False, 11, True), (22, 0.06, True, 0, False)])
def test_list_kernels_equal_their_restatements_at_this_horizon(N, dt, first_tick, now_k, snap):
    """The bodies of test_list_adjoint_kernel_equals_the_restatement, test_list_orientation_kernel_equals_the_restatement and
    test_list_jvp_kernel_equals_the_restatement_and_is_the_transpose_of_the_list_adjoints, M = 12, on the grid, off the grid with force_sample_time, and on
    the first tick: the position adjoint, the orientation adjoint and contacts_jvp_device equal their restatements to F64, the JVP is the transpose of the
    two adjoints on the device to F64, and problem 5's failed merge gives zeros and status 5."""
    cfg = cm.config.ergocub_gazebo_v1(N, dt)
    _check_list_adjoint(cfg, 12, first_tick, now_k, snap)
    _check_list_orientation(cfg, 12, first_tick, now_k, snap)
    _check_list_jvp(cfg, 12, first_tick, now_k, snap)


# ---------------------------------------------------------------------------------------------------------------- 5. tick VJP, tick VJP in the orientations, tick JVP
def _probe_problems(name, cfg, tk):
    """the two problems of a tick that go to the float64 restatement: 0 and 5; on sn000, 0 and the first other problem whose landing in the tape's X sits on
    a box face -- one in x (0.01 m off the nominal footstep) if there is one -- so that a constrained landing is differentiated wherever the tape has one"""
    if name != "sn000":
        return (0, 5)
    Ph, Xh = tk["P"].cpu().numpy(), tk["X"].cpu().numpy()
    faces = {b: parity.box_faces(cfg.N, Ph[b], Xh[b]) for b in range(1, B)}
    in_x = [b for b, f in faces.items() if any(r[2] == 0 for r in f)]
    any_face = [b for b, f in faces.items() if f]
    return (0, (in_x or any_face or [5])[0])


def _tick_derivatives(name):
    """Every differentiated tick of the configuration's walk through rollout_tick_jvp_device (k = 9 and its first three columns alone) and
    rollout_tick_vjp_device(rot=True, grad_p=True, dGradX=...), once per session; two problems per tick through rollout_jvp_ref.tick_jvp and
    rollout_rot_ref.tick_vjp_rot (which returns rollout_adjoint_ref.tick_vjp's groups unchanged beside the orientation groups), fed with the tape's own
    float32 (x, p, lam_g) and sharing one RotSens.  -> dict of what the tests below assert on."""
    if name in _derivs:
        return _derivs[name]
    import torch
    cfg, plan, ro, rec = _taped(name)
    L, N = cm.Layout(cfg.N), cfg.N
    tape = rec["tape"]["ticks"]
    M = tape[0]["list_t"].shape[2]
    s = ro.solver
    rng = np.random.default_rng(21)
    out = dict(jvp={g: 0.0 for g in OUT_GROUPS}, vjp={g: 0.0 for g in GROUPS + ROT_GROUPS}, adjoint=0.0, status=[], k9=[], face_pairs=[], lines=[])
    for i in WALKS[name][1]:
        tk = tape[i]
        d = _tick_directions(rng, cfg, B, 9, M)
        g = dict(state=rng.normal(size=(B, 9)), list=rng.normal(size=(B, 2, M, 3)) * 0.1, list_rot=rng.normal(size=(B, 2, M, 3)) * 0.1,
                 x=(rng.normal(size=(B, L.nx)) * 0.01).astype(np.float32))
        f9 = _tick_jvp(s, tk, d)
        f3 = _tick_jvp(s, tk, d, slice(0, 3))
        acc = {n: torch.zeros(shape, dtype=torch.float64, device="cuda") for n, shape in (("plan", (B, 2, M, 3)), ("model", (B, 34)), ("plan_rot", (B, 2, M, 3)))}
        v = s.rollout_tick_vjp_device(tk["now"], tk, _cu(g["state"]), _cu(g["list"]), _cu(g["x"]), dGradPlan=acc["plan"], dGradModel=acc["model"], grad_p=True,
                                      dGradListRotOut=_cu(g["list_rot"]), rot=True, dGradPlanRot=acc["plan_rot"])
        torch.cuda.synchronize()
        out["status"].append((i, f9["sens"][:, 0].cpu().numpy(), f3["sens"][:, 0].cpu().numpy(), v["sens"][:, 0].cpu().numpy()))
        out["k9"].append((i, {grp: bool(torch.equal(f9[grp][:, :3], f3[grp])) and bool(f9[grp].any()) for grp in OUT_GROUPS}))
        fh = {grp: f3[grp].cpu().numpy() for grp in OUT_GROUPS}
        vh = {n: a.cpu().numpy() for n, a in dict(state=v["state"], prev_list=v["prev_list"], wrench=v["wrench"], plan=acc["plan"], model=acc["model"], p=v["p"],
                                                  prev_list_rot=v["prev_list_rot"], plan_rot=acc["plan_rot"], rot=v["rot"]).items()}
        sens_j, sens_v = f3["sens"].cpu().numpy(), v["sens"].cpu().numpy()
        # the adjoint identity on the device, all eight problems and three columns
        vin = dict(state=vh["state"], list=vh["prev_list"], list_rot=vh["prev_list_rot"], plan=vh["plan"], plan_rot=vh["plan_rot"], wrench=vh["wrench"],
                   model=vh["model"], p=vh["p"])
        for b in range(B):
            for j in range(3):
                lhs = sum((g[n][b].astype(np.float64) * fh[n][b, j].astype(np.float64)).sum() for n in ("state", "list", "list_rot", "x"))
                rhs = sum(float((vin[n][b].astype(np.float64) * d[n][b, j].astype(np.float64)).sum()) for n in IN_GROUPS)
                out["adjoint"] = max(out["adjoint"], _gap(lhs, rhs))
        # two problems against the restatements
        Ph, Xh = tk["P"].cpu().numpy(), tk["X"].cpu().numpy()
        for b in _probe_problems(name, cfg, tk):
            tp = _host_tape(tk, b)
            faces = parity.box_faces(N, Ph[b], Xh[b])
            RS = srr.RotSens(cfg, tp["X"], tp["P"], tp["lam_g"])
            ref = rrr.tick_vjp_rot(cfg, tp, tk["now"], g["state"][b], g["list"][b], g["x"][b], g_list_rot_out=g["list_rot"][b], RS=RS)
            assert ref["status"] == 0
            vg = {grp: _rel(vh[grp][b], ref[grp]) for grp in GROUPS + ROT_GROUPS}
            jg = {grp: 0.0 for grp in OUT_GROUPS}
            for j in range(3):
                rj = rjr.tick_jvp(cfg, tp, tk["now"], d["state"][b, j], d["list"][b, j], d["list_rot"][b, j], d["plan"][b, j], d["plan_rot"][b, j],
                                  d["wrench"][b, j], d["model"][b, j], d["p"][b, j], RS=RS)
                assert rj["status"] == 0
                for grp in OUT_GROUPS:
                    jg[grp] = max(jg[grp], _rel(fh[grp][b, j], rj[grp]))
            for grp in vg:
                out["vjp"][grp] = max(out["vjp"][grp], vg[grp])
            for grp in jg:
                out["jvp"][grp] = max(out["jvp"][grp], jg[grp])
            if faces:
                out["face_pairs"].append((i, b))
            out["lines"].append(f"{name} tick {i} problem {b} land {tk['land'][b].tolist()} faces {sorted(faces)} weak {ref['weak']} sens words (status, residual, "
                                f"weak rows, largest Sigma, .., weak swing rows, removed) jvp {sens_j[b, :7].tolist()} vjp {sens_v[b, :7].tolist()}: VJP " +
                                " ".join(f"{k} {x:.1e}" for k, x in vg.items()) + "  JVP " + " ".join(f"{k} {x:.1e}" for k, x in jg.items()))
    print("\n" + "\n".join(out["lines"]))
    _derivs[name] = out
    return out


@pytest.mark.parametrize("name", CONFIGS)
def test_tick_vjp_and_its_orientation_groups_match_the_restatements(name):
    """cmpc_rollout_tick_vjp_rot_device on the differentiated ticks, two problems each: every group of rollout_adjoint_ref.tick_vjp (state, prev_list,
    wrench, plan, model, p) and of rollout_rot_ref.tick_vjp_rot (prev_list_rot, plan_rot, rot) <= REF of its largest entry; dTickSens[:, 0] == 0 for all
    eight problems.  sn000: at least one differentiated (tick, problem) has a landing on a box face in the tape's X."""
    r = _tick_derivatives(name)
    print(f"\n{name}: tick VJP against the restatements, worst: " + " ".join(f"{k} {v:.2e}" for k, v in r["vjp"].items()) + f" (bound {REF:.0e})")
    for i, _, _, sv in r["status"]:
        assert (sv == 0).all(), (i, sv)
    if name == "sn000":
        print(f"sn000: differentiated (tick, problem) pairs with a landing on a box face: {r['face_pairs']}")
        assert len(r["face_pairs"]) >= 1
    assert max(r["vjp"].values()) <= REF, r["vjp"]


@pytest.mark.parametrize("name", CONFIGS)
def test_tick_jvp_matches_the_restatement_and_does_not_depend_on_k(name):
    """cmpc_rollout_tick_jvp_device on the same ticks and problems, k = 3, every input group random: every output group <= REF of
    rollout_jvp_ref.tick_jvp; dTickSens[:, 0] == 0; the same columns computed at k = 9 (across a chunk of eight, with this horizon's workspace) are
    bit-equal."""
    r = _tick_derivatives(name)
    print(f"\n{name}: tick JVP against the restatement, worst: " + " ".join(f"{k} {v:.2e}" for k, v in r["jvp"].items()) + f" (bound {REF:.0e})")
    for i, s9, s3, _ in r["status"]:
        assert (s9 == 0).all() and (s3 == 0).all(), (i, s9, s3)
    for i, same in r["k9"]:
        assert all(same.values()), (i, same)
    assert max(r["jvp"].values()) <= REF, r["jvp"]


@pytest.mark.parametrize("name", CONFIGS)
def test_tick_jvp_and_tick_vjp_are_adjoint_at_this_horizon(name):
    """<g, J d> = <J^T g, d> of a whole tick on the device, rollout_tick_jvp_device (k = 3) against rollout_tick_vjp_device(rot=True, grad_p=True,
    dGradX=...), all eight input groups and all four cotangent groups random at once: <= ADJ of the larger side, per problem and column, on all eight
    problems of the differentiated ticks."""
    r = _tick_derivatives(name)
    print(f"\n{name}: tick JVP against tick VJP on the device, worst gap over 4 ticks x 8 problems x 3 columns: {r['adjoint']:.2e} (bound {ADJ:.0e})")
    assert r["adjoint"] <= ADJ


# ---------------------------------------------------------------------------------------------------------------- 6. the whole walk
@pytest.mark.parametrize("name", ["n13", "n22"])
def test_forward_sensitivity_is_the_transpose_of_backward_over_six_ticks(name):
    """The first six ticks of the walk, forward_sensitivity at k = 2 with every direction group random against backward(rot=True) with random cotangents
    on every state and every solution: <= 6 x ADJ per problem and column (the first assertion of
    test_forward_sensitivity_is_the_transpose_of_backward_and_the_jvp_of_rollout_differentiable)."""
    import torch
    cfg, plan, ro, rec = _taped(name)
    T, k = 6, 2
    assert all(rec["converged"][:T])
    tape = dict(rec["tape"], ticks=rec["tape"]["ticks"][:T])
    L = cm.Layout(cfg.N)
    M = tape["ticks"][0]["list_t"].shape[2]
    rng = np.random.default_rng(14)
    d = _tick_directions(rng, cfg, B, k, M)
    d_push = rng.normal(size=(B, k, 3)).astype(np.float32)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (rng.normal(size=(T, B, L.nx)) * 0.01).astype(np.float32)
    f = ro.forward_sensitivity(tape, dir_state0=d["state"], dir_list0=d["list"], dir_list_rot0=d["list_rot"], dir_plan=d["plan"], dir_plan_rot=d["plan_rot"],
                               dir_push=d_push, dir_models=d["model"], solutions=True)
    v = ro.backward(tape, gS, gX, rot=True)
    torch.cuda.synchronize()
    assert (f["status"] == 0).all() and (v["status"] == 0).all()
    fs, fx = f["states"].cpu().numpy(), f["X"].cpu().numpy().astype(np.float64)
    assert np.array_equal(fs[0], d["state"]) and f["list"].any() and f["list_rot"].any()
    pairs = (("state0", d["state"]), ("list0", d["list"]), ("list_rot0", d["list_rot"]), ("push", d_push.astype(np.float64)), ("models", d["model"]),
             ("plan", d["plan"]), ("plan_rot", d["plan_rot"]))
    vh = {n: v[n].cpu().numpy() for n, _ in pairs}
    worst = 0.0
    for b in range(B):
        for j in range(k):
            lhs = (gS[:, b] * fs[:, b, j]).sum() + (gX[:, b].astype(np.float64) * fx[:, b, j]).sum()
            rhs = sum(float((vh[n][b] * dd[b, j]).sum()) for n, dd in pairs)
            worst = max(worst, _gap(lhs, rhs))
    print(f"\n{name}: forward sweep against reverse sweep over {T} ticks, worst gap over 8 problems x 2 columns: {worst:.2e} (bound {6 * ADJ:.1e})")
    assert worst <= 6 * ADJ
