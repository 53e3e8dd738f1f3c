"""forceSampleTime on the GPU (ContactPhaseList::forceSampleTime(m_dT), CentroidalMPCBlock.cpp:586-592): the device kernel against the host entry
point, the snap inside the one-call tick (cmpc_tick_io.force_sample_time) against a tick fed host-snapped lists, the sampled schedule against
oracle/schedule_ref.py on the restated snap (tests/snap_ref.py), the no-op on an on-grid plan, a collapsing contact, and the walking roll-out
on a plan whose every time is off the grid."""
import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import force_sample_time, pack_lists
from oracle import schedule_ref
from tests import snap_ref
from tests.test_contacts_cpu import _random_walks

pytestmark = pytest.mark.gpu

DT = 0.06


def _cfg():
    return cm.config.ergocub_gazebo_v1(20, DT)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _dev(arrs):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


@pytest.mark.parametrize("B", [1, 7, 4096])
@pytest.mark.parametrize("M", [4, 24])
def test_device_kernel_is_bit_equal_to_the_host_entry(B, M):
    import torch
    rng = np.random.default_rng(B * 100 + M)
    t, n = snap_ref.random_lists(rng, B, M, DT)
    t[0] = np.arange(M)[None, :, None] + np.array([0.013, 0.9])        # problem 0: off the grid, nothing collapses
    if B >= 7:
        n[3, 1] = M + 1                 # a list length out of range: ok = 0, that foot's entries neither read nor written
        n[5, 0] = -2
    s = cm.BatchSolver(_cfg(), B)
    dt_, dn = _dev((t, n))
    out = torch.full_like(dt_, 77.0)
    out, ok = s.contacts_force_sample_time_device(dt_, dn, out=out)
    inplace = dt_.clone()
    _, ok2 = s.contacts_force_sample_time_device(inplace, dn, out=inplace)
    torch.cuda.synchronize()
    out, ok, inplace, ok2 = out.cpu().numpy(), ok.cpu().numpy(), inplace.cpu().numpy(), ok2.cpu().numpy()
    bad = np.zeros(B, bool)
    if B >= 7:
        bad[[3, 5]] = True
        assert (out[3, 1] == 77.0).all() and (out[5, 0] == 77.0).all()
        assert np.array_equal(_bits(inplace[3, 1]), _bits(t[3, 1])) and np.array_equal(_bits(inplace[5, 0]), _bits(t[5, 0]))
        assert ok[3] == 0 and ok[5] == 0 and ok2[3] == 0 and ok2[5] == 0
    good = ~bad
    ht, hok = force_sample_time(DT, t[good], n[good])
    assert np.array_equal(_bits(out[good]), _bits(ht)) and np.array_equal(_bits(inplace[good]), _bits(ht))
    assert np.array_equal(ok[good].astype(bool), hok) and np.array_equal(ok2[good].astype(bool), hok)
    assert hok[0]
    if B > 1:
        assert not hok.all()


def _tick(s, cfg, now, plan, prev, lists, ok, dX_prev, flag):
    """one cmpc_rollout_tick_device call on fresh buffers; -> dict of host copies of everything it writes"""
    import torch
    B, L, N = s.batch, cm.Layout(cfg.N), cfg.N
    rng = np.random.default_rng(4)
    state = torch.from_numpy(np.concatenate([np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3)), np.zeros((B, 6))], 1).astype(np.float32)).cuda()
    dP = torch.zeros((B, L.np), dtype=torch.float32, device="cuda")
    dX0 = torch.zeros((B, L.nx), dtype=torch.float32, device="cuda")
    dX = dX_prev.clone() if dX_prev is not None else torch.zeros_like(dX0)
    dInfo = torch.zeros((B, 8), dtype=torch.float32, device="cuda")
    land = torch.full((B, 2), 99, dtype=torch.int32, device="cuda")
    out_state = torch.zeros_like(state)
    zmp = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
    plan_com = torch.zeros((B, 40, 3), dtype=torch.float32, device="cuda")
    s.rollout_tick_device(now, plan, prev, lists, ok, land, state, None, dP, dX0, dX, dInfo, out_state, zmp, dX_prev is not None,
                          step=DT / 6, substeps=6, planner=(plan_com, torch.zeros_like(plan_com), DT, now, 1.0, 0.7), force_sample_time=flag)
    torch.cuda.synchronize()
    info = dInfo.cpu().numpy()
    info[:, 6] = 0                                                  # (the shader-clock count changes from run to run)
    return dict(P=dP.cpu().numpy(), X=dX.cpu().numpy(), land=land.cpu().numpy(), ok=ok.cpu().numpy(), listT=lists[0].cpu().numpy(),
                listPose=lists[1].cpu().numpy(), listN=lists[2].cpu().numpy(), info=info, state=out_state.cpu().numpy(), zmp=zmp.cpu().numpy(), dX=dX)


def _assert_ticks_equal(a, b, rows=None):
    for k in ("P", "X", "land", "ok", "listT", "listPose", "listN", "info", "state", "zmp"):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(_bits(x), _bits(y)), k


@pytest.mark.parametrize("M", [12, 20])
def test_tick_with_the_flag_is_the_tick_on_host_snapped_lists(M):
    """first tick and a merge tick; M = 12 snaps inside the front kernel, M = 20 in the standalone kernel launched before it"""
    import torch
    cfg = _cfg()
    B = 24
    t, pose, n = pack_lists(cfg, _random_walks(cfg, B, 57), max_contacts=M)
    ts, ok_h = force_sample_time(DT, t, n)
    assert ok_h.all() and not np.array_equal(ts, t)
    s = cm.BatchSolver(cfg, B)
    # first tick: the caller's lists are snapped in place and dOk is written
    la = _dev((t, pose, n))
    lb = _dev((ts, pose, n))
    a = _tick(s, cfg, 0.0, _dev((t, pose, n)), None, la, torch.zeros(B, dtype=torch.int32, device="cuda"), None, True)
    b = _tick(s, cfg, 0.0, _dev((ts, pose, n)), None, lb, torch.ones(B, dtype=torch.int32, device="cuda"), None, False)
    _assert_ticks_equal(a, b)
    assert (a["ok"] == 1).all() and np.array_equal(_bits(a["listT"]), _bits(ts))
    # a merge tick seven knots later, warm-started from the first: the planner's lists are snapped, the caller's planner buffer is not written
    now = 7 * DT
    plan_a = _dev((t, pose, n))
    zeros = lambda: (torch.zeros((B, 2, M, 2), dtype=torch.float64, device="cuda"), torch.zeros((B, 2, M, 7), dtype=torch.float32, device="cuda"),
                     torch.zeros((B, 2), dtype=torch.int32, device="cuda"))
    a2 = _tick(s, cfg, now, plan_a, la, zeros(), torch.zeros(B, dtype=torch.int32, device="cuda"), a["dX"], True)
    b2 = _tick(s, cfg, now, _dev((ts, pose, n)), lb, zeros(), torch.zeros(B, dtype=torch.int32, device="cuda"), b["dX"], False)
    _assert_ticks_equal(a2, b2)
    assert (a2["ok"] == 1).all() and np.array_equal(_bits(plan_a[0].cpu().numpy()), _bits(t))
    assert (a2["land"] >= -1).all()


def test_snapped_schedule_matches_the_oracle_and_the_flag_changes_it():
    import torch
    cfg = _cfg()
    B, M, N = 32, 12, cfg.N
    L = cm.Layout(N)
    t, pose, n = pack_lists(cfg, _random_walks(cfg, B, 63), max_contacts=M)
    s = cm.BatchSolver(cfg, B)
    now = 3 * DT
    on = _tick(s, cfg, now, _dev((t, pose, n)), None, _dev((t, pose, n)), torch.zeros(B, dtype=torch.int32, device="cuda"), None, True)
    off = _tick(s, cfg, now, _dev((t, pose, n)), None, _dev((t, pose, n)), torch.zeros(B, dtype=torch.int32, device="cuda"), None, False)
    rs, rok = snap_ref.snap_lists(DT, t, n)
    assert rok.all() and (on["ok"] == 1).all()
    up = [c.bounding_box_upper_limit for c in cfg.contacts]
    lo = [c.bounding_box_lower_limit for c in cfg.contacts]
    differs = 0
    for b in range(B):
        for c in range(2):
            lst = [dict(activation=float(rs[b, c, m, 0]), deactivation=float(rs[b, c, m, 1]), position=pose[b, c, m, :3], quaternion=pose[b, c, m, 3:])
                   for m in range(n[b, c])]
            ref = schedule_ref.sample_contact_list(N, DT, now, lst, up[c], lo[c])
            gam = on["P"][b, L.p_gam[c]:L.p_gam[c] + N]
            assert gam.tolist() == ref["gamma"], (b, c)
            assert on["land"][b, c] == ref["land"], (b, c)
            differs += int(not np.array_equal(gam, off["P"][b, L.p_gam[c]:L.p_gam[c] + N]))
    assert differs > 0          # without the snap the same off-grid plans give another contact pattern


def test_on_grid_walking_plan_is_unchanged_by_the_flag():
    cfg = _cfg()
    B, ticks = 16, 24
    rng = np.random.default_rng(19)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    z = np.zeros((B, 3))
    recs = [cm.rollout.WalkingRollout(cfg, B, force_sample_time=f).run(ticks, com0, dcom0, z) for f in (True, False)]
    a, b = recs
    assert all(a["converged"]) and all(a["merge_ok"]) and len(a["com"]) == ticks
    for key in ("com", "zmp", "land", "landing_offset"):
        assert np.array_equal(np.stack(a[key]), np.stack(b[key])), key
    assert a["iterations_max"] == b["iterations_max"] and a["iterations_mean"] == b["iterations_mean"]


@pytest.mark.parametrize("M", [12, 20])
def test_a_collapsing_contact_fails_its_problem_only(M):
    import torch
    cfg = _cfg()
    B, j = 16, 5
    t, pose, n = pack_lists(cfg, _random_walks(cfg, B, 71), max_contacts=M)
    bad = t.copy()
    a0 = np.round(bad[j, 0, 2, 0] / DT) * DT + 0.005
    bad[j, 0, 2] = (a0, a0 + 0.002)               # 2 ms inside one grid cell: collapses
    _, hok = force_sample_time(DT, bad, n)
    assert hok.tolist() == [b != j for b in range(B)]
    s = cm.BatchSolver(cfg, B)
    others = np.arange(B) != j
    res = []
    for tt in (bad, t):
        lists = _dev((tt, pose, n))
        first = _tick(s, cfg, 0.0, _dev((tt, pose, n)), None, lists, torch.zeros(B, dtype=torch.int32, device="cuda"), None, True)
        merged = _dev((np.zeros_like(t), np.zeros_like(pose), np.zeros_like(n)))
        second = _tick(s, cfg, 4 * DT, _dev((tt, pose, n)), lists, merged, torch.zeros(B, dtype=torch.int32, device="cuda"), first["dX"], True)
        res.append((first, second))
    (fa, sa), (fb, sb) = res
    for x, y in ((fa, fb), (sa, sb)):
        assert x["ok"][j] == 0 and x["land"][j, 0] == -2 and x["listN"][j, 0] == 0
        assert (y["ok"] == 1).all()
        _assert_ticks_equal(x, y, rows=others)


def _jitter(plan, rng, amp):
    out = {}
    for name, lst in plan.items():
        out[name] = []
        for c in lst:
            f = lambda v: v if v == 0.0 or abs(v) >= 1e9 else v + float(rng.uniform(-amp, amp))
            out[name].append(cm.contacts.PlannedContact(f(c.activation_time), f(c.deactivation_time), c.position, c.yaw))
    return out


def test_walking_rollout_on_an_off_grid_plan():
    cfg = _cfg()
    B, ticks = 16, 24
    base = cm.rollout.walking_plan(cfg)
    jit = _jitter(base, np.random.default_rng(3), 0.45 * DT)
    # the host-rounded plan (the C ABI's host entry point on the packed lists, written back into the contacts)
    t, _, n = pack_lists(cfg, [jit])
    ts, ok = force_sample_time(DT, t, n)
    assert ok.all() and not np.array_equal(ts, t)
    names = [c.contact_name for c in cfg.contacts]
    rounded = {nm: [cm.contacts.PlannedContact(float(ts[0, ci, m, 0]), float(ts[0, ci, m, 1]), c.position, c.yaw)
                    for m, c in enumerate(sorted(jit[nm], key=lambda c: c.activation_time))] for ci, nm in enumerate(names)}
    last = max(c.position[0] for lst in base.values() for c in lst)
    speed = last / max(c.activation_time for lst in base.values() for c in lst)
    rng = np.random.default_rng(23)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    z = np.zeros((B, 3))
    run = lambda plan, flag, native=True: cm.rollout.WalkingRollout(cfg, B, plan=plan, com_speed=speed, force_sample_time=flag,
                                                                    native_tick=native).run(ticks, com0, z, z)
    a = run(jit, True)
    b = run(rounded, False)
    c = run(jit, True, native=False)
    assert all(a["converged"]) and all(a["merge_ok"]) and len(a["com"]) == ticks
    com = np.stack(a["com"])
    assert np.abs(com[:, :, 2] - 0.7).max() < 0.03 and np.abs(com[:, :, 1]).max() < 0.08
    for other in (b, c):
        assert np.array_equal(np.stack(a["land"]), np.stack(other["land"]))
        assert a["iterations_max"] == other["iterations_max"] and a["iterations_mean"] == other["iterations_mean"]
        assert np.array_equal(com, np.stack(other["com"]))
    lands = np.stack(a["land"])[:, 0]                # problem 0: the left foot lands at 0.84 s = tick 14, as on the unjittered plan
    assert lands[0, 0] == 14 and lands[13, 0] == 1
    # unsnapped, the same off-grid plan is sampled differently
    d = run(jit, False)
    assert not np.array_equal(np.stack(d["land"]), np.stack(a["land"])) or d["iterations_mean"] != a["iterations_mean"]
