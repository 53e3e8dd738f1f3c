"""Ended problems out of the launches of a tick (include/cmpc.h, cmpc_set_ended_device; WalkingRollout.walk_device(skip_ended=True)): the walking
problems are bit-identical with and without the mask, an ended problem's buffers stay what its ending tick left, plain solves honour the mask, the
one-call walk equals the ticks called one by one under the mask, a partial workgroup of the back kernel, and no host read.

The failing problem is tests/test_gpu_walk_record.py's: from tick 2 on the planner of problem 3 no longer knows the left foot's current contact, so its
merge fails at tick 2 (code 1) and the record ends it there.  Tick 2 itself ran in full -- the record that ends a problem runs behind the tick -- so
what is frozen is what a 3-tick walk leaves."""
import dataclasses

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_record_ref as wr
from tests.test_gpu_walk_record import _host, _start

pytestmark = pytest.mark.gpu

OTHERS = [0, 1, 2, 4, 5, 6, 7]
SENTINEL = 0x7FC12345          # a quiet NaN with a payload: no solve writes these bits


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(x, y, msg=""):
    np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=msg)


def _no_clock(info):
    info = np.array(info, copy=True)
    info[:, 6] = 0      # (solve_cycles, the shader clock: not a result)
    return info


def _broken_plan(ro, problems=(3,)):
    t = ro.plan[0].clone()
    for b in problems:
        t[b, 0] += 100.0
    return (t, ro.plan[1], ro.plan[2])


def _models(cfg, B):
    """one model per problem: the friction coefficient differs, so a solve that read another problem's record would not reproduce"""
    return [dataclasses.replace(cfg, static_friction_coefficient=0.3 + 0.05 * b) for b in range(B)]


def _walk_arrays(w):
    out = _host(w)
    out["info"] = _no_clock(out["info"])
    for j, a in enumerate(w["lists"]):
        out[f"list{j}"] = a.cpu().numpy()
    return out


@pytest.mark.parametrize("n,opts", [(10, {}), (13, dict(factors="hbm")), (10, dict(models=True))], ids=["N10-resident", "N13-hbm", "N10-models"])
def test_walking_problems_are_untouched(n, opts):
    """B = 8, 5 ticks, problem 3 ends at tick 2: skip_ended=True against False.  The trace, the outcome and stats to the bit for all eight (the record
    never looks at an ended problem's buffers); X, P, info (the clock word zeroed), state and lists to the bit for the seven others."""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(n, 0.06)
    B, ticks = 8, 5
    com0, dcom0, h0, push = _start(B)
    opts = dict(opts)
    if opts.pop("models", False):
        opts["models"] = _models(cfg, B)
    got = {}
    for skip in (False, True):
        ro = cm.rollout.WalkingRollout(cfg, B, **opts)
        got[skip] = _walk_arrays(ro.walk_device(ticks, com0, dcom0, h0, push=push, push_ticks=2, replan={2: _broken_plan(ro)}, skip_ended=skip))
        torch.cuda.synchronize()
        assert getattr(ro.solver, "_ended", None) is None      # cleared behind the queued segments
    off, on = got[False], got[True]
    assert on["end_tick"].tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and on["end_code"][3] == 1
    assert (on["iterations"][:, OTHERS] > 0).all()
    for k in list(wr.TRACE) + ["end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min", "stats"]:
        _same_bits(on[k], off[k], k)
    for k in ("X", "P", "info", "state", "list0", "list1", "list2"):
        _same_bits(on[k][OTHERS], off[k][OTHERS], k)
    # ... and the mask did something: without it problem 3 walked on
    assert not np.array_equal(_bits(on["state"][3]), _bits(off["state"][3]))


class _Walk:
    """the buffers of a walk over the C ABI, laid out as WalkingRollout.walk_device lays them out, every one of them readable; mask: the record's end_tick
    is the handle's mask for the life of the object"""

    def __init__(self, cfg, B, rows, mask, wrench_rows=2):
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
        n_plan = rows + cfg.N + 2
        self.plan_com = z((B, n_plan, 3))
        self.plan_com[:, :, 0] = (ro.com_speed * cfg.sampling_time * torch.arange(n_plan, dtype=torch.float64, device=dev)).to(torch.float32)[None, :]
        self.plan_h = torch.zeros_like(self.plan_com)
        self.sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
        self.rec = self.s.walk_record(rows)
        self.s.outcome_init_device(self.state, self.rec)
        self.cur, self.dt = 0, cfg.sampling_time
        self.kw = dict(step=cfg.sampling_time / ro.substeps, substeps=ro.substeps)
        if mask:
            self.s.set_ended_device(self.rec["end_tick"])

    def call(self, tick0, ticks, plan=None):
        wr_ = self.wrench[tick0:] if tick0 < self.wrench.shape[0] else None
        self.cur = self.s.rollout_walk_device(tick0, ticks, tick0 == 0, plan or self.ro.plan, self.sets[0], self.sets[1], self.cur, self.ok, self.land,
                                              self.state, self.dP, self.dX0, self.dX, self.dInfo, self.zmp, self.rec, row0=tick0, wrench_ticks=wr_,
                                              planner=(self.plan_com, self.plan_h, self.dt, 0.0, 1.0, 0.7), **self.kw)

    def loop(self, ticks, replan):
        """the same ticks through cmpc_rollout_tick_device and cmpc_rollout_record_device, one call each"""
        s, plan = self.s, self.ro.plan
        for i in range(ticks):
            now = i * self.dt
            plan = replan.get(i, plan)
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
            s.rollout_tick_device(now, plan, prev, lists, self.ok, self.land, self.state, wr_, self.dP, self.dX0, self.dX, self.dInfo, self.state,
                                  self.zmp, i > 0, planner=planner, **self.kw)
            s.rollout_record_device(i, i, self.dX, self.dP, self.dInfo, self.ok if i > 0 else None, self.land, self.state, self.zmp, self.rec)

    def buffers(self, clock=True):
        """every buffer a tick writes, on the host: dP, dX0, dX, dInfo, dOk, dLand, state, dZmp (named apart from the trace's land and zmp) and BOTH list sets"""
        import torch
        torch.cuda.synchronize()
        info = self.dInfo.cpu().numpy()
        out = dict(P=self.dP.cpu().numpy(), X0=self.dX0.cpu().numpy(), X=self.dX.cpu().numpy(), info=info if clock else _no_clock(info),
                   dOk=self.ok.cpu().numpy(), dLand=self.land.cpu().numpy(), state=self.state.cpu().numpy(), dZmp=self.zmp.cpu().numpy())
        for i, st in enumerate(self.sets):
            for j, a in enumerate(st):
                out[f"set{i}_{j}"] = a.cpu().numpy()
        return out

    def host(self):
        out = self.buffers(clock=False)
        out.update(_host(self.rec), cur=self.cur)
        return out


def test_the_ended_problem_is_frozen():
    """Own buffers, the mask set, 5 ticks with problem 3 ending at tick 2.  Its rows of dP, dX0, dX, dInfo, ok, land, state, zmp and of both list sets
    (a) after 5 ticks hold the bits they held after 3 ticks of the SAME walk -- all eight words of dInfo, the clock word included -- and (b) equal the
    rows a 3-tick walk WITHOUT the mask leaves on buffers of its own (the clock word zeroed there: two runs never share it).
    final_state[3] is the state after the last GOOD tick (tick 1: what a 2-tick walk leaves, include/cmpc.h), one plant step before the frozen state[3],
    which is what the ending tick left; both are checked, and that they differ.  Without the mask state[3] walks on and (a), (b) fail."""
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    B = 8
    on = _Walk(cfg, B, 5, mask=True)
    bad = _broken_plan(on.ro)
    on.call(0, 2)
    on.call(2, 1, bad)
    at_end = on.buffers()
    on.call(3, 2, bad)
    after = on.host()
    last = on.buffers()
    assert after["end_tick"].tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and after["code"][:, 3].tolist() == [0, 0, 1, -1, -1]
    for k in at_end:
        _same_bits(last[k][3], at_end[k][3], f"{k}: row 3 after 5 ticks against row 3 after its ending tick")
    assert not np.array_equal(_bits(last["state"][OTHERS]), _bits(at_end["state"][OTHERS]))      # (the others walked on)
    off = _Walk(cfg, B, 3, mask=False)
    off.call(0, 2)
    off.call(2, 1, _broken_plan(off.ro))
    three = off.host()
    for k in at_end:
        _same_bits(after[k][3], three[k][3], f"{k}: row 3 against the 3-tick walk without the mask")
    two = _Walk(cfg, B, 2, mask=False)
    two.call(0, 2)
    two_state = two.host()["state"]
    print("final_state[3]", after["final_state"][3], "state[3]", after["state"][3])
    _same_bits(after["final_state"][3], two_state[3], "final_state: the state after the last good tick")
    _same_bits(after["final_state"][3], three["final_state"][3])
    assert not np.array_equal(_bits(after["final_state"][3]), _bits(after["state"][3]))


def test_ended_by_the_solver():
    """max_iterations = 1: every cold solve of tick 0 comes back with status 1 (code 2), which ends all eight there; the three ticks behind it skip
    every problem, so X, info and state are what 1 tick leaves"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    B = 8
    com0, dcom0, h0, push = _start(B)
    walk = lambda ticks, skip: _walk_arrays(cm.rollout.WalkingRollout(cfg, B, max_iterations=1).walk_device(
        ticks, com0, dcom0, h0, push=push, push_ticks=2, stop=("merge", "solver"), skip_ended=skip))
    four, one = walk(4, True), walk(1, False)
    torch.cuda.synchronize()
    assert (four["end_tick"] == 0).all() and (four["end_code"] == 2).all()
    for k in ("X", "info", "state", "P"):       # (lists: the two sets alternate, and 4 ticks end on the set that tick 0 did not write)
        _same_bits(four[k], one[k], k)
    assert four["stats"][:, 0].tolist() == [8, 0, 0, 0]
    assert four["info"][:, 0].tolist() == [1.0] * B


def _filled(shape, device="cuda"):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


@pytest.mark.parametrize("n,factors", [(10, None), (13, "hbm")], ids=["N10-resident", "N13-hbm"])
def test_plain_solves_honour_the_mask(n, factors):
    """cmpc_solve_device and cmpc_solve_device_warm at B = 9 under the mask [-1, 0, -1, 7, -1, -1, 3, -1, -1] into dX / dInfo filled with a sentinel: the
    masked rows keep the sentinel's bits, the others equal the unmasked solve; the masked rows of the multiplier record are still the earlier solve's;
    with the mask cleared every row is solved again."""
    import torch
    B = 9
    mask_h = np.array([-1, 0, -1, 7, -1, -1, 3, -1, -1], np.int32)
    ended, walking = np.nonzero(mask_h >= 0)[0], np.nonzero(mask_h < 0)[0]
    cfg, P1, X01 = cm.synthetic.config3_external_push(B, N=n, seed=201)
    _, P2, X02 = cm.synthetic.config3_external_push(B, N=n, seed=202)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    dP1, dX01, dP2, dX02 = up(P1), up(X01), up(P2), up(X02)
    s = cm.BatchSolver(cfg, B, factors=factors)
    s.set_multiplier_output()
    host = lambda t: t.cpu().numpy()
    X2, I2 = s.solve_device(dP2, dX02)
    lam2 = host(s.multipliers_device(X2, dP2))
    dXw = torch.empty_like(X2)
    s.shift_solution_device(X2, dXw)
    X2w, I2w = s.solve_device(dP2, dXw, warm=True)
    X1, I1 = s.solve_device(dP1, dX01)                 # the record now holds problem set 1
    lam1 = host(s.multipliers_device(X1, dP1))
    torch.cuda.synchronize()
    assert (host(I1)[:, 5] == 0).all() and (host(I2)[:, 5] == 0).all() and not np.array_equal(lam1, lam2)
    mask = torch.from_numpy(mask_h).cuda()
    s.set_ended_device(mask)
    for warm, x0, Xr, Ir in ((False, dX02, X2, I2), (True, dXw, X2w, I2w)):
        dX, dI = _filled((B, s.layout.nx)), _filled((B, 8))
        s.solve_device(dP2, x0, dX, dI, warm=warm)
        torch.cuda.synchronize()
        x, i = host(dX), host(dI)
        assert (_bits(x[ended]) == SENTINEL).all() and (_bits(i[ended]) == SENTINEL).all(), warm
        _same_bits(x[walking], host(Xr)[walking], f"X warm={warm}")
        _same_bits(_no_clock(i)[walking], _no_clock(host(Ir))[walking], f"info warm={warm}")
    # the record: set 1's rows where the mask held the solve back, set 2's (the warm solve's) elsewhere
    _same_bits(host(s.multipliers_device(X1, dP1))[ended], lam1[ended], "multiplier record of the masked rows")
    lam2w = host(s.multipliers_device(X2w, dP2))
    s.set_ended_device(None)
    dX, dI = _filled((B, s.layout.nx)), _filled((B, 8))
    s.solve_device(dP2, dX02, dX, dI)
    torch.cuda.synchronize()
    _same_bits(host(dX), host(X2), "every row solved again")
    _same_bits(_no_clock(host(dI)), _no_clock(host(I2)))
    # (the unmasked rows of the record followed the masked warm solve: the same rows of an unmasked warm solve's record)
    s.solve_device(dP2, dXw, warm=True)
    _same_bits(lam2w[walking], host(s.multipliers_device(X2w, dP2))[walking], "multiplier record of the walking rows")
    s.close()


def test_tick_by_tick_is_the_one_call_walk_under_the_mask():
    """5 ticks, problem 3 ending at tick 2, the mask set: cmpc_rollout_tick_device + cmpc_rollout_record_device one by one against the walk in one
    call per segment, every array to the bit"""
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    B = 8
    one = _Walk(cfg, B, 5, mask=True)
    bad = _broken_plan(one.ro)
    one.call(0, 2)
    one.call(2, 3, bad)
    a = one.host()
    by_tick = _Walk(cfg, B, 5, mask=True)
    by_tick.loop(5, {2: _broken_plan(by_tick.ro)})
    b = by_tick.host()
    assert a["end_tick"].tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and a["cur"] == b["cur"]
    for k in a:
        _same_bits(np.asarray(a[k]), np.asarray(b[k]), k)


def test_a_partial_workgroup_of_the_back_kernel():
    """B = 300 (a second, partial workgroup of the one-thread-per-problem back kernel), N = 10, one cold and one warm tick under a seeded mask with a third
    of the problems ended: their rows are untouched, the others equal the same ticks without the mask.  The cold start under the mask likewise."""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    B = 300
    mask_h = np.where(np.random.default_rng(7).permutation(B) < B // 3, 4, -1).astype(np.int32)
    ended, walking = np.nonzero(mask_h >= 0)[0], np.nonzero(mask_h < 0)[0]
    assert len(ended) == 100 and (mask_h[256:] >= 0).any() and (mask_h[256:] < 0).any()
    runs = {}
    for masked in (False, True):
        w = _Walk(cfg, B, 2, mask=False)
        s = w.s
        s.contacts_sample_device(0.0, w.sets[0], w.dP)          # the set-up of a first tick, for every problem
        s.write_state_device(w.state, w.dP, w.wrench[0])
        s.cold_start_device(w.dP, w.dX0)
        before = w.buffers()
        if masked:
            s.set_ended_device(torch.from_numpy(mask_h).cuda())
        planner = lambda now: (w.plan_com, w.plan_h, w.dt, now, 1.0, 0.7)
        s.rollout_tick_device(0.0, w.ro.plan, None, w.sets[0], w.ok, w.land, w.state, w.wrench[0], w.dP, w.dX0, w.dX, w.dInfo, w.state, w.zmp, False,
                              planner=planner(0.0), **w.kw)
        s.rollout_tick_device(w.dt, w.ro.plan, w.sets[0], w.sets[1], w.ok, w.land, w.state, w.wrench[1], w.dP, w.dX0, w.dX, w.dInfo, w.state, w.zmp, True,
                              planner=planner(w.dt), **w.kw)
        cold = s.cold_start_device(w.dP, _filled((B, s.layout.nx)))
        runs[masked] = (before, w.buffers(clock=False), cold.cpu().numpy())
    (_, off, cold_off), (before, on, cold_on) = runs[False], runs[True]
    before["info"] = _no_clock(before["info"])
    assert (off["info"][:, 5] == 0).all() and (off["info"][:, 0] > 0).all()
    for k in on:
        _same_bits(on[k][ended], before[k][ended], f"{k}: masked rows")
        _same_bits(on[k][walking], off[k][walking], f"{k}: walking rows")
        if k not in ("dOk", "set1_1") and not k.startswith("set0"):      # (a first tick leaves ok alone; set 0 is adjusted only at a landing; poses' padding)
            assert not np.array_equal(_bits(off[k][ended]), _bits(before[k][ended])), k
    assert (_bits(cold_on[ended]) == SENTINEL).all()
    _same_bits(cold_on[walking], cold_off[walking])


def test_walk_device_with_skipping_reads_nothing_back():
    """the whole of walk_device(skip_ended=True), a replan and an ended problem in it, under torch's sync debug mode"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    B = 8
    com0, dcom0, h0, push = _start(B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    bad = _broken_plan(ro)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device(6, com0, dcom0, h0, push=push, push_ticks=2, replan={2: bad}, skip_ended=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert w["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 2, -1, -1, -1, -1]
    assert (w["iterations"].cpu().numpy()[:, OTHERS] > 0).all()
