"""A walk of the whole batch on the device (include/cmpc.h): the record kernel against the host form and the numpy restatement, the cold-start kernel
against the torch construction, WalkingRollout.walk_device against run(), a failed merge that ends ONE problem where run() aborts the batch, one call
of cmpc_rollout_walk_device against the same ticks called one by one, and no host read inside walk_device."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import pack_lists
from tests import walk_record_ref as wr
from tests.test_walk_record_cpu import box, host_record, host_record_arrays

pytestmark = pytest.mark.gpu

N = 10
OUTCOME = ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")


def _host(rec):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in rec.items() if k != "_c" and not isinstance(v, tuple)}


def _solver_with_box(cfg, B):
    """a handle whose box is on the device (a sampling uploads it)"""
    import torch
    s = cm.BatchSolver(cfg, B)
    lists = tuple(torch.from_numpy(a).cuda() for a in pack_lists(cfg, [cm.rollout.walking_plan(cfg)] * B))
    s.contacts_sample_device(0.0, lists, torch.zeros((B, s.layout.np), dtype=torch.float32, device="cuda"))
    return s


def _device_record(s, ticks, outcome, stop_mask, tick0=11):
    import torch
    names = [k for k, b in cm._capi.STOP_BITS.items() if stop_mask & b]
    rec = s.walk_record(len(ticks), stop=names)
    for k in OUTCOME:
        rec[k].copy_(torch.from_numpy(outcome[k]))
    rec["stats"].fill_(-7)     # (the call clears its row)
    for i, t in enumerate(ticks):
        d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
        s.rollout_record_device(tick0 + i, i, d["X"], d["P"], d["info"], d["ok"], d["land"], d["state_out"], d["zmp"], rec)
    torch.cuda.synchronize()
    return _host(rec)


@pytest.mark.parametrize("case", [("feet", 7), ("codes", 7), ("codes", 1), ("ended", 3), ("ended", 5), (70, 7), (70, 1), (300, 7), (300, 4)])
def test_record_kernel_matches_the_host_form(case):
    """the crafted ticks of the CPU test, and B = 70 (a partial second wave) and B = 300 (a second workgroup) with random codes and ended flags: the kernel
    against the host form under the CPU test's tolerances, the statistics row against the numpy counts exactly"""
    kind, stop_mask = case
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    up, lo = box(cfg)
    ticks, outcome = wr.crafted_ticks(N, kind) if isinstance(kind, str) else wr.random_ticks(N, kind, seed=kind)
    B = ticks[0]["X"].shape[0]
    h = host_record_arrays(len(ticks), B, outcome, stop_mask)
    host_record(cm._capi.lib(), N, ticks, h, up, lo)
    got = _device_record(_solver_with_box(cfg, B), ticks, outcome, stop_mask)
    rows = [{k: h[k][i] for k in wr.TRACE} for i in range(len(ticks))]
    wr.assert_matches(got, rows, h["stats"], {k: h[k] for k in OUTCOME})
    ref_rows, ref_stats, ref_out = wr.reference(N, ticks, outcome, stop_mask, up, lo)
    np.testing.assert_array_equal(got["stats"], ref_stats)
    wr.assert_matches(got, ref_rows, ref_stats, ref_out)
    if not isinstance(kind, str):
        assert ref_stats[:, 1].sum() > 0 and (ref_stats[:, 0] < B).all() and ref_stats[:, 4].sum() > 0      # the random ticks end problems, and hold ended ones


def test_record_needs_the_box_and_a_row_inside_the_record():
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    ticks, outcome = wr.crafted_ticks(N, "feet")
    s = cm.BatchSolver(cfg, 5)
    rec = s.walk_record(1)
    d = {k: torch.from_numpy(v).cuda() for k, v in ticks[0].items()}
    call = lambda s, row: s._lib.cmpc_rollout_record_device(s._h, 0, row, d["X"].data_ptr(), d["P"].data_ptr(), d["info"].data_ptr(), None, d["land"].data_ptr(),
                                                           d["state_out"].data_ptr(), d["zmp"].data_ptr(), C.byref(rec["_c"]), None)
    assert call(s, 0) != 0 and "box" in s.last_error
    s = _solver_with_box(cfg, 5)
    assert call(s, 1) != 0 and call(s, -1) != 0
    assert call(s, 0) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [10, 13])
def test_cold_start_kernel_is_the_torch_construction(n):
    import torch
    cfg = cm.config.ergocub_gazebo_v1(n, 0.06)
    B, L = 9, cm.Layout(n)
    s = cm.BatchSolver(cfg, B)
    dP = torch.from_numpy(np.random.default_rng(n).normal(size=(B, L.np)).astype(np.float32)).cuda()
    want = torch.zeros((B, L.nx), dtype=torch.float32, device="cuda")      # WalkingRollout._tick_by_steps' cold start
    want[:, L.com:L.com + 3 * (n + 1)] = dP[:, L.p_com0:L.p_com0 + 3].repeat(1, n + 1)
    for c in range(2):
        want[:, L.pos[c]:L.pos[c] + 3 * (n + 1)] = dP[:, L.p_nom[c]:L.p_nom[c] + 3 * (n + 1)]
        for j in range(4):
            want[:, L.f[c][j] + 2:L.f[c][j] + 3 * n:3] = cm.config.GRAVITY / 8.0
    got = s.cold_start_device(dP, torch.full((B, L.nx), 5.0, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(got.cpu().numpy(), cm.layout.cold_start(n, dP.cpu().numpy(), dtype=np.float32))     # (the numpy form of the host cold start)


def _start(B, seed=11):
    rng = np.random.default_rng(seed)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3))
    push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    return com0, dcom0, h0, push


def test_recorded_walk_is_the_existing_walk():
    """walk_device against run(record="full") on a fresh roll-out, 16 ticks at N = 10: the left foot's landing enters the horizon at tick 4 and lands at
    tick 14.  (run's tape gives the last X, the final state and the per-problem iterations; a taped run is bit-identical to an untaped one.)"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    B, ticks = 8, 16
    com0, dcom0, h0, push = _start(B)
    rec = cm.rollout.WalkingRollout(cfg, B).run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="full", tape=True)
    assert all(rec["merge_ok"]) and len(rec["com"]) == ticks
    w = cm.rollout.WalkingRollout(cfg, B).walk_device(ticks, com0, dcom0, h0, push=push, push_ticks=3)
    torch.cuda.synchronize()
    g = _host(w)
    for k in ("com", "zmp", "land"):
        np.testing.assert_array_equal(g[k], np.stack(rec[k]), err_msg=k)
    tape = rec["tape"]
    np.testing.assert_array_equal(g["final_state"], tape["state"].cpu().numpy())
    np.testing.assert_array_equal(g["state"], tape["state"].cpu().numpy())
    np.testing.assert_array_equal(g["X"], tape["ticks"][-1]["X"].cpu().numpy())
    its = np.stack([tk["info"][:, 0].cpu().numpy() for tk in tape["ticks"]]).astype(np.int32)
    np.testing.assert_array_equal(g["iterations"], its)
    off = np.stack(rec["landing_offset"])
    print("landing_offset: largest |walk_device - run| =", np.abs(g["landing_offset"] - off).max(), " largest |offset| =", np.abs(off).max())
    np.testing.assert_allclose(g["landing_offset"], off, rtol=0, atol=1e-12)
    assert np.abs(g["landing_offset"]).max() > 0
    assert g["land"][4, 0, 0] == N and g["land"][13, 0, 0] == 1
    assert (g["end_tick"] == -1).all() and (g["end_code"] == 0).all()
    np.testing.assert_array_equal(g["stats"], wr.stats_of_trace(g["code"], g["iterations"], np.zeros((ticks, B), bool)))
    np.testing.assert_array_equal(g["iterations_sum"], its.sum(0))
    np.testing.assert_array_equal(g["iterations_max"], its.max(0))
    # the least box slack is the trace's: over the ticks, landing feet and axes
    up, lo = box(cfg)
    landing = (g["land"] > 0) & (g["land"] <= N)
    slack = np.minimum(up[None, None] - g["landing_offset"], g["landing_offset"] - lo[None, None]).min(-1)
    want = np.where(landing, slack, np.inf).min((0, 2))
    np.testing.assert_allclose(g["box_slack_min"], want, rtol=0, atol=1e-7)
    for a, b in zip(w["lists"], tape["lists"]):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_a_failed_merge_ends_one_problem_only():
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    B, ticks = 8, 5
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    ro = cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    t[3, 0] += 100.0          # from tick 2 on the planner of problem 3 no longer knows the left foot's current contact
    replan = {2: (t, ro.plan[1], ro.plan[2])}
    rec = ro.run(ticks, com0, z, z, replan=replan)
    assert rec.get("aborted_tick") == 2        # the whole batch stops there ...
    w = _host(cm.rollout.WalkingRollout(cfg, B).walk_device(ticks, com0, z, z, replan=replan))
    base = _host(cm.rollout.WalkingRollout(cfg, B).walk_device(ticks, com0, z, z))
    two = _host(cm.rollout.WalkingRollout(cfg, B).walk_device(2, com0, z, z))
    torch.cuda.synchronize()
    assert w["end_tick"].tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and w["end_code"][3] == 1 and (np.delete(w["end_code"], 3) == 0).all()   # ... one problem here
    np.testing.assert_array_equal(w["final_state"][3], two["state"][3])
    assert w["code"][:, 3].tolist() == [0, 0, 1, -1, -1]
    for k in ("com", "zmp", "landing_offset"):
        assert np.isnan(w[k][2:, 3]).all() and not np.isnan(w[k][:2, 3]).any(), k
    assert (w["land"][2:, 3] == -2).all() and (w["iterations"][2:, 3] == 0).all() and (w["iterations"][:2, 3] > 0).all()
    others = [0, 1, 2, 4, 5, 6, 7]
    take = lambda k, a: np.take(a, others, axis=1 if k in wr.TRACE else 0)      # (the trace is [ticks, B, ..], everything else [B, ..])
    for k in list(wr.TRACE) + ["final_state", "X", "state", "iterations_sum", "iterations_max", "box_slack_min", "end_tick"]:
        x, y = take(k, w[k]), take(k, base[k])
        np.testing.assert_array_equal(x.view(np.uint64 if x.dtype == np.float64 else np.uint32), y.view(np.uint64 if y.dtype == np.float64 else np.uint32), err_msg=k)
    assert w["stats"][:, 0].tolist() == [8, 8, 8, 7, 7] and w["stats"][:, 1].tolist() == [0, 0, 1, 0, 0]
    assert (base["end_tick"] == -1).all()
    # a solver status whose stop bit is off is recorded and the problem walks on
    one = _host(cm.rollout.WalkingRollout(cfg, B, max_iterations=1).walk_device(ticks, com0, z, z, stop=("merge",)))
    torch.cuda.synchronize()
    assert (one["code"] == 2).any() and (one["end_tick"] == -1).all() and not np.isnan(one["com"]).any()
    assert (one["stats"][:, 4] == (one["code"] == 2).sum(1)).all()


class _Walk:
    """the buffers of a walk over the C ABI, laid out as WalkingRollout.walk_device lays them out"""

    def __init__(self, cfg, B, rows, wrench_rows, n_plan):
        import torch
        self.ro = ro = cm.rollout.WalkingRollout(cfg, B)
        self.s, L, dev = ro.solver, ro.L, ro.dev
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        self.dP, self.dX0, self.dX, self.dInfo = z((B, L.np)), z((B, L.nx)), z((B, L.nx)), z((B, 8))
        com0, dcom0, h0, push = _start(B)
        self.state = torch.from_numpy(np.concatenate([com0, dcom0, h0], 1).astype(np.float32)).to(dev)
        self.ok, self.land, self.zmp = torch.ones((B,), dtype=torch.int32, device=dev), z((B, 2), torch.int32), z((B, 2))
        self.wrench = z((wrench_rows, B, cfg.N, 6))
        for i in range(wrench_rows):
            self.wrench[i, :, :wrench_rows - i, :3] = torch.from_numpy(push.astype(np.float32)).to(dev)[:, None, :]
        self.plan_com = z((B, n_plan, 3))
        self.plan_com[:, :, 0] = (ro.com_speed * cfg.sampling_time * torch.arange(n_plan, dtype=torch.float64, device=dev)).to(torch.float32)[None, :]
        self.plan_h = torch.zeros_like(self.plan_com)
        self.sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
        self.rec = self.s.walk_record(rows)
        self.s.outcome_init_device(self.state, self.rec)
        self.cur, self.dt = 0, cfg.sampling_time
        self.kw = dict(step=cfg.sampling_time / ro.substeps, substeps=ro.substeps)

    def call(self, tick0, ticks, wrench=True):
        self.cur = self.s.rollout_walk_device(tick0, ticks, tick0 == 0, self.ro.plan, self.sets[0], self.sets[1], self.cur, self.ok, self.land, self.state,
                                              self.dP, self.dX0, self.dX, self.dInfo, self.zmp, self.rec, row0=tick0,
                                              wrench_ticks=self.wrench if wrench else None, planner=(self.plan_com, self.plan_h, self.dt, 0.0, 1.0, 0.7), **self.kw)

    def loop(self, ticks):
        """the same ticks through cmpc_rollout_tick_device and cmpc_rollout_record_device, one call each"""
        s = self.s
        for i in range(ticks):
            now = i * self.dt
            planner = (self.plan_com, self.plan_h, self.dt, now, 1.0, 0.7)
            wr_ = self.wrench[i] if i < self.wrench.shape[0] else None
            if i == 0:   # a first tick: the rows of dP the cold start reads (the tick writes the same values again), then the cold start, then the tick from it
                s.contacts_sample_device(now, self.sets[0], self.dP)
                s.write_state_device(self.state, self.dP, wr_)
                s.cold_start_device(self.dP, self.dX0)
                prev, lists = None, self.sets[0]
            else:
                prev, lists = self.sets[self.cur], self.sets[1 - self.cur]
                self.cur = 1 - self.cur
            s.rollout_tick_device(now, self.ro.plan, prev, lists, self.ok, self.land, self.state, wr_, self.dP, self.dX0, self.dX, self.dInfo, self.state,
                                  self.zmp, i > 0, planner=planner, **self.kw)
            s.rollout_record_device(i, i, self.dX, self.dP, self.dInfo, self.ok if i > 0 else None, self.land, self.state, self.zmp, self.rec)

    def host(self):
        import torch
        torch.cuda.synchronize()
        out = _host(self.rec)
        info = self.dInfo.cpu().numpy()
        info[:, 6] = 0      # (solve_cycles, the shader clock: not a result)
        out.update(X=self.dX.cpu().numpy(), P=self.dP.cpu().numpy(), info=info, state=self.state.cpu().numpy(), cur=self.cur,
                   **{f"list{j}": a.cpu().numpy() for j, a in enumerate(self.sets[self.cur])})
        return out


def _assert_same_bits(a, b, rows=slice(None)):
    for k in a:
        x, y = (a[k][rows], b[k][rows]) if k in wr.TRACE or k == "stats" else (a[k], b[k])
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32 if x.dtype == np.float32 else np.uint64), y.view(np.uint32 if y.dtype == np.float32 else np.uint64)
        np.testing.assert_array_equal(x, y, err_msg=k)


def test_one_call_of_the_walk_is_the_ticks_called_one_by_one():
    """cmpc_rollout_walk_device for 6 ticks, the first one cold, under a 3-row wrench schedule, against cmpc_rollout_tick_device +
    cmpc_rollout_record_device tick by tick on buffers of their own: every array to the last bit.  A second call with tick0 = 6 continues the walk and
    ends where one call of 12 ticks ends."""
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    B, n_plan = 8, 12 + N + 2
    one = _Walk(cfg, B, 12, 3, n_plan)
    one.call(0, 6)
    first = one.host()
    by_tick = _Walk(cfg, B, 12, 3, n_plan)
    by_tick.loop(6)
    _assert_same_bits(first, by_tick.host(), rows=slice(0, 6))
    assert (first["iterations"][:6] > 0).all() and first["cur"] == 1
    one.call(6, 6, wrench=False)
    whole = _Walk(cfg, B, 12, 3, n_plan)
    whole.call(0, 12)
    _assert_same_bits(one.host(), whole.host())


def test_walk_device_reads_nothing_back():
    """the whole of walk_device under torch's sync debug mode: a host read or a synchronisation inside it raises"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    B = 8
    com0, dcom0, h0, push = _start(B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device(6, com0, dcom0, h0, push=push, push_ticks=2, replan={3: (t, ro.plan[1], ro.plan[2])})
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert (w["end_tick"].cpu().numpy() == -1).all() and (w["iterations"].cpu().numpy() > 0).all()
