"""A queue of trials walked through the slots of one walk (include/cmpc.h, cmpc_walk_refill; WalkingRollout.walk_device_refill): a slot's first tick
inside the merge launches is the cold first tick of walk_device, refilled trials are fresh walks at their own local time, neighbours do not matter, the
queue runs dry cleanly, one call equals many, no host read, the refill kernel against its host form -- at the edges of a wave and of a chunk against the
assignment model too -- and the handle behind a refill walk.  Trials long enough to change their lists: tests/test_gpu_walk_refill_long.py.

The comparison of a refill walk with refill + cmpc_rollout_tick_device-level calls is not made: a tick in refill mode has no entry point of its own (the
front and back kernels take the slots' start ticks only inside cmpc_rollout_walk_refill_device), and the issue rules a new one out for this test."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_record_ref as wr
from tests import walk_refill_ref as rf
from tests.test_gpu_walk_record import _start

pytestmark = pytest.mark.gpu

OUTCOME = ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")
_bits = rf.bits


def _same_bits(x, y, msg=""):
    np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=msg)


def _no_clock(info):
    info = np.array(info, copy=True)
    info[:, 6] = 0      # (solve_cycles, the shader clock: not a result)
    return info


def _walk_arrays(w):
    """every key walk_device returns, on the host: the trace, the outcome, stats, X, P, info (the clock word zeroed), state and the lists"""
    out = {k: v.cpu().numpy() for k, v in w.items() if hasattr(v, "cpu")}
    out["info"] = _no_clock(out["info"])
    for j, a in enumerate(w["lists"]):
        out[f"list{j}"] = a.cpu().numpy()
    return out


class _SlotWalk:
    """the buffers of a walk over the C ABI, laid out as WalkingRollout.walk_device and walk_device_refill lay them out, every one of them readable -- BOTH
    list sets, which the methods do not return"""

    def __init__(self, cfg, B, rows, **opts):
        import torch
        self.ro = ro = cm.rollout.WalkingRollout(cfg, B, **opts)
        self.s, L, dev, self.B, self.rows = ro.solver, ro.L, ro.dev, B, rows
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        self.dP, self.dX0, self.dX, self.dInfo = z((B, L.np)), z((B, L.nx)), z((B, L.nx)), z((B, 8))
        self.state = z((B, 9))
        self.ok, self.land, self.zmp = torch.ones((B,), dtype=torch.int32, device=dev), z((B, 2), torch.int32), z((B, 2))
        self.sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
        self.rec = self.s.walk_record(rows)
        self.fill = None
        self.kw = dict(step=cfg.sampling_time / ro.substeps, substeps=ro.substeps, force_sample_time=ro.force_sample_time)

    def plain(self, ticks, state0, wrench):
        """walk_device's calls: the first tick cold on set 0"""
        self.state.copy_(state0)
        self.s.outcome_init_device(self.state, self.rec)
        self.cur = self.s.rollout_walk_device(0, ticks, True, self.ro.plan, self.sets[0], self.sets[1], 0, self.ok, self.land, self.state, self.dP, self.dX0,
                                              self.dX, self.dInfo, self.zmp, self.rec, row0=0, wrench_ticks=wrench, planner=self.ro._planner_refs(ticks),
                                              **self.kw)
        return self

    def refill(self, calls, trial_ticks, state0, wrench):
        """walk_device_refill's calls, the ticks queued as len(calls) calls with row0 and lists_in carried: tick 0 writes set 0"""
        self.s.outcome_init_device(self.state, self.rec)
        self.fill = self.s.walk_refill(state0, trial_ticks, wrench, trace_rows=self.rows)
        self.cur, t0 = 1, 0
        for n in calls:
            self.cur = self.s.rollout_walk_refill_device(t0, n, self.ro.plan, self.sets[0], self.sets[1], self.cur, self.ok, self.land, self.state, self.dP,
                                                         self.dX0, self.dX, self.dInfo, self.zmp, self.rec, self.fill, row0=t0,
                                                         planner=self.ro._planner_refs(trial_ticks), **self.kw)
            t0 += n
        self.s.rollout_refill_device(t0, self.rec, self.fill, None)
        return self

    def host(self):
        import torch
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.rec.items() if hasattr(v, "cpu")}
        out.update(X=self.dX.cpu().numpy(), P=self.dP.cpu().numpy(), info=_no_clock(self.dInfo.cpu().numpy()), state=self.state.cpu().numpy(), cur=self.cur,
                   ok=self.ok.cpu().numpy(), land=self.land.cpu().numpy())
        for i, st in enumerate(self.sets):
            for j, a in enumerate(st):
                out[f"set{i}_{j}"] = a.cpu().numpy()
        if self.fill is not None:
            out.update({"fill_" + k: v.cpu().numpy() for k, v in self.fill.items() if hasattr(v, "cpu")})
        return out


def _push_rows(push, push_ticks, n):
    """run()'s schedule as wrench rows [push_ticks + 1, len(push), n, 6]"""
    w = np.zeros((push_ticks + 1, push.shape[0], n, 6), np.float32)
    for i in range(push_ticks):
        w[i, :, :max(push_ticks - i, 1), :3] = push[:, None, :]
    return w


# ---- 1. the fresh tick is the cold tick ----
@pytest.mark.parametrize("n,opts", [(10, {}), (13, dict(factors="hbm")), (10, dict(force_sample_time=True))], ids=["N10-resident", "N13-hbm", "N10-snap"])
def test_fresh_tick_is_the_cold_tick(n, opts):
    """B = Q = 8, trial_ticks = ticks = 5: every key of walk_device(5, ...) on a fresh roll-out, bit for bit -- the per-problem cold policy of the solve, the
    cold start inside the front kernel, the lists taken from the plan, dOk -- and trial_of = arange(8) in every row"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(n, 0.06)
    B, ticks = 8, 5
    com0, dcom0, h0, push = _start(B)
    want = _walk_arrays(cm.rollout.WalkingRollout(cfg, B, **opts).walk_device(ticks, com0, dcom0, h0, push=push, push_ticks=2))
    w = cm.rollout.WalkingRollout(cfg, B, **opts).walk_device_refill(ticks, ticks, com0, dcom0, h0, push=push, push_ticks=2)
    torch.cuda.synchronize()
    got = _walk_arrays(w)
    assert (want["end_tick"] == -1).all() and (want["iterations"] > 0).all()
    for k in want:
        _same_bits(got[k], want[k], k)
    assert (got["trial_of"] == np.arange(B)[None, :]).all()
    t = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
    for k in OUTCOME:
        _same_bits(t[k], want[k], "trials " + k)
    assert t["ticks"].tolist() == [ticks] * B and t["slot"].tolist() == list(range(B)) and t["start"].tolist() == [0] * B
    # BOTH list sets, which the methods do not return: the same two walks over the C ABI.  Set 0 starts as the plan's clone on both sides; the cold tick
    # keeps it (snapped in place with force_sample_time) and the fresh tick writes its entries in use over it
    import torch
    state0 = torch.from_numpy(np.concatenate([com0, dcom0, h0], 1).astype(np.float32)).cuda()
    wrench = torch.from_numpy(_push_rows(push.astype(np.float32), 2, n)).cuda()
    cold = _SlotWalk(cfg, B, ticks, **opts).plain(ticks, state0, wrench).host()
    fresh = _SlotWalk(cfg, B, ticks, **opts).refill([ticks], ticks, state0, wrench).host()
    for k in cold:
        _same_bits(fresh[k], cold[k], "C ABI " + k)
    for k in ("X", "P", "state", "com"):
        _same_bits(cold[k], want[k], "C ABI against the method " + k)
    assert (cold["set0_2"] > 0).all() and (cold["set1_2"] > 0).all()


# ---- 2, 3. refilled trials are fresh walks; neighbours are untouched ----
N2, B2, Q2, TT2, T2 = 10, 4, 10, 4, 12
# the hand-made tables of who sits where and when (tests/walk_refill_ref.py, where the assignment model is held to them)
TRIAL_OF, SLOT, START, TICKS, END, SLOT_CALM, START_CALM = rf.TRIAL_OF, rf.SLOT, rf.START, rf.TICKS, rf.END, rf.SLOT_CALM, rf.START_CALM


def _queue(harmless=False):
    """the ten trials: _start's states and, as the wrench rows, its push under run()'s rule for push_ticks = 2 (4 rows = trial_ticks); NaN rows for trial 1
    at local tick 0, trial 2 at local tick 2, trial 6 at local tick 1, and a NaN in trial 4's com0"""
    com0, dcom0, h0, push = (a.astype(np.float32) for a in _start(Q2, seed=21))
    wrench = np.zeros((TT2, Q2, N2, 6), np.float32)
    for i in range(2):
        wrench[i, :, :2 - i, :3] = push[:, None, :]
    if not harmless:
        wrench[0, 1] = np.nan
        wrench[2, 2] = np.nan
        wrench[1, 6] = np.nan
        com0[4, 1] = np.nan
    return com0, dcom0, h0, wrench


def _plain_walk(cfg, trials, com0, dcom0, h0, wrench):
    """walk_device(4, ...) of a batch of 4 that holds trials[b] in slot b, its wrench rows given as they are (walk_device itself builds them from a push):
    WalkingRollout._walk_live's calls with the rows passed through"""
    import torch
    ro = cm.rollout.WalkingRollout(cfg, B2)
    s, L, dev, dt = ro.solver, ro.L, ro.dev, cfg.sampling_time
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    dP, dX0, dX, dInfo = z((B2, L.np)), z((B2, L.nx)), z((B2, L.nx)), z((B2, 8))
    state = torch.from_numpy(np.concatenate([com0[trials], dcom0[trials], h0[trials]], 1)).to(dev).contiguous()
    ok, land, zmp = torch.ones((B2,), dtype=torch.int32, device=dev), z((B2, 2), torch.int32), z((B2, 2))
    rec = s.walk_record(TT2)
    s.outcome_init_device(state, rec)
    sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
    wt = torch.from_numpy(np.ascontiguousarray(wrench[:, trials])).to(dev)
    s.rollout_walk_device(0, TT2, True, ro.plan, sets[0], sets[1], 0, ok, land, state, dP, dX0, dX, dInfo, zmp, rec, row0=0, wrench_ticks=wt,
                          step=dt / ro.substeps, substeps=ro.substeps, planner=ro._planner_refs(TT2))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in rec.items() if hasattr(v, "cpu")}


def _refill_walk(cfg, harmless=False):
    import torch
    com0, dcom0, h0, wrench = _queue(harmless)
    w = cm.rollout.WalkingRollout(cfg, B2).walk_device_refill(T2, TT2, com0, dcom0, h0, wrench_trials=wrench)
    torch.cuda.synchronize()
    return w


@pytest.fixture(scope="module")
def stormy():
    """the refill walk of test 2, computed once: (its dict, per-trial outcome on the host, {q: gathered trace rows on the host})"""
    cfg = cm.config.ergocub_gazebo_v1(N2, 0.06)
    w = _refill_walk(cfg)
    t = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
    traces = {q: {k: v.cpu().numpy() for k, v in w["trials"]["trace"](q).items()} for q in range(Q2)}
    return cfg, w, t, traces


def test_refilled_trials_are_fresh_walks(stormy):
    """B = 4, Q = 10, trial_ticks = 4, 12 ticks, four trials that end early: who sat where and when is the hand-made table, and every trial's outcome and
    trace rows are those of a plain 4-tick walk of a batch of 4 that holds it in the slot it occupied (three reference walks: 0..3 | 7, 4, 6, 8 | 5 and 9)"""
    cfg, w, t, traces = stormy
    assert w["trial_of"].cpu().numpy().tolist() == TRIAL_OF
    assert t["slot"].tolist() == SLOT and t["start"].tolist() == START and t["ticks"].tolist() == TICKS and t["end_tick"].tolist() == END
    assert [int(c) for c in t["end_code"]] == [0, 3, 3, 0, 3, 0, 3, 0, 0, 0]
    com0, dcom0, h0, wrench = _queue()
    for group in ([0, 1, 2, 3], [7, 4, 6, 8], [0, 5, 9, 3]):         # (trial group[b] sits in slot b; trials 0 and 3 fill the last walk's spare slots)
        assert all(SLOT[q] == b for b, q in enumerate(group))
        ref = _plain_walk(cfg, group, com0, dcom0, h0, wrench)
        for b, q in enumerate(group):
            for k in OUTCOME:
                _same_bits(t[k][q], ref[k][b], f"trial {q} {k}")
            rows = TICKS[q]
            assert traces[q]["valid"].tolist() == [True] * rows + [False] * (TT2 - rows)
            for k in wr.TRACE:
                _same_bits(traces[q][k][:rows], ref[k][:rows, b], f"trial {q} {k}")
    # the trials that walked through did walk: finite rows, positive iteration counts
    for q in (0, 3, 5, 7, 8, 9):
        assert (traces[q]["iterations"] > 0).all() and np.isfinite(traces[q]["com"]).all(), q


def test_neighbours_are_untouched(stormy):
    """the same queue with trials 1, 2, 4 and 6 made harmless: the slots turn over differently, and the trials that keep their slot and start tick -- 0
    and 3, beside slots whose occupants changed -- are bit-equal in outcome and trace"""
    cfg, w, t, traces = stormy
    calm = _refill_walk(cfg, harmless=True)
    tc = {k: v.cpu().numpy() for k, v in calm["trials"].items() if hasattr(v, "cpu")}
    assert tc["slot"].tolist() == SLOT_CALM and tc["start"].tolist() == START_CALM and (tc["end_tick"] == -1).all() and tc["ticks"].tolist() == [4] * Q2
    keep = [q for q in range(Q2) if SLOT[q] == SLOT_CALM[q] and START[q] == START_CALM[q] and q not in (1, 2, 4, 6)]
    assert keep == [0, 3]
    for q in keep:
        tr = {k: v.cpu().numpy() for k, v in calm["trials"]["trace"](q).items()}
        for k in OUTCOME:
            _same_bits(tc[k][q], t[k][q], f"trial {q} {k}")
        for k in wr.TRACE:
            _same_bits(tr[k], traces[q][k], f"trial {q} {k}")
    assert not np.array_equal(calm["trial_of"].cpu().numpy(), np.array(TRIAL_OF))


# ---- 4. exhaustion ----
def test_queue_runs_dry():
    """Q = 5, B = 4, trial_ticks = 4, 10 ticks: trial 4 takes slot 0 at tick 4, the other slots are empty from then on and slot 0 from tick 8; the last
    ticks' stats rows show nobody walking, and an exhausted slot's X, P and state hold what its last tick left (a 4-tick and an 8-tick walk of the queue)"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    com0, dcom0, h0, push = _start(5, seed=31)
    walks = {}
    for ticks in (4, 8, 10):
        w = cm.rollout.WalkingRollout(cfg, 4).walk_device_refill(ticks, 4, com0, dcom0, h0, push=push, push_ticks=2)
        torch.cuda.synchronize()
        walks[ticks] = _walk_arrays(w), {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
    g, t = walks[10]
    assert g["trial_of"].tolist() == [[0, 1, 2, 3]] * 4 + [[4, -1, -1, -1]] * 4 + [[-1] * 4] * 2
    assert t["slot"].tolist() == [0, 1, 2, 3, 0] and t["start"].tolist() == [0, 0, 0, 0, 4] and t["ticks"].tolist() == [4] * 5 and (t["end_tick"] == -1).all()
    assert g["stats"][:, 0].tolist() == [4] * 4 + [1] * 4 + [0, 0] and (g["stats"][8:] == 0).all()
    assert g["end_tick"].tolist() == [8, 4, 4, 4]          # (the slots' words: out through the ended mask from the tick the queue had nothing for them)
    assert (g["code"][4:, 1:] == -1).all() and (g["code"][8:] == -1).all() and (g["iterations"][:8, 0] > 0).all()
    for k in ("X", "P", "state"):
        _same_bits(g[k][1:], walks[4][0][k][1:], k + " of slots 1..3")
        _same_bits(g[k][0], walks[8][0][k][0], k + " of slot 0")
    for k in OUTCOME:
        _same_bits(t[k], walks[8][1][k], "trials " + k)


# ---- 5. one call equals many ----
def test_one_call_equals_two(stormy):
    """the 12 ticks of test 2 queued as 5 + 7 (row0 and lists_in carried): every array of the walk and of the queue to the bit"""
    import torch
    cfg, w, t, traces = stormy
    com0, dcom0, h0, wrench = _queue()
    state0 = torch.from_numpy(np.concatenate([com0, dcom0, h0], 1)).cuda()
    dwrench = torch.from_numpy(wrench).cuda()
    one = _SlotWalk(cfg, B2, T2).refill([T2], TT2, state0, dwrench).host()
    two = _SlotWalk(cfg, B2, T2).refill([5, 7], TT2, state0, dwrench).host()
    assert set(one) == set(two)
    for k in one:
        _same_bits(two[k], one[k], k)
    # ... and they are the method's walk
    a = _walk_arrays(w)
    for k in ("com", "code", "stats", "end_tick", "X", "P", "state"):
        _same_bits(one[k], a[k], k)
    _same_bits(one["fill_trial_of"], a["trial_of"])
    for k in OUTCOME:
        _same_bits(one["fill_" + k], t[k], "trials " + k)


def test_refusals_queue_nothing():
    """a real handle: max_contacts = 17 and a non-NULL io.dWrenchTicks return CMPC_ERR_ARG, and no buffer of the walk has moved once the stream has run"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    com0, dcom0, h0, push = _start(6)
    wk = _SlotWalk(cfg, 4, 3)
    s = wk.s
    state0 = torch.from_numpy(np.concatenate([com0, dcom0, h0], 1).astype(np.float32)).cuda()
    wrench = torch.from_numpy(_push_rows(push.astype(np.float32), 2, 10)).cuda()
    s.outcome_init_device(wk.state, wk.rec)
    wk.fill = s.walk_refill(state0, 3, wrench, trace_rows=3)
    wk.cur = 1
    before = wk.host()

    def call(max_contacts, wrench_ticks=None):
        io = cm._capi.CmpcWalkIO()
        io.tick = s._tick_io(wk.ro.plan, None, wk.sets[0], wk.ok, wk.land, wk.state, None, wk.dP, wk.dX0, wk.dX, wk.dInfo, wk.state, wk.zmp, wk.kw["step"],
                             wk.kw["substeps"], 0.08, 0.03, wk.ro._planner_refs(3), False)
        io.dListTB, io.dListPoseB, io.dListNB = (a.data_ptr() for a in wk.sets[1])
        if wrench_ticks is not None:
            io.dWrenchTicks, io.wrench_ticks = wrench_ticks.data_ptr(), int(wrench_ticks.shape[0])
        out = C.c_int(-7)
        rc = s._lib.cmpc_rollout_walk_refill_device(s._h, max_contacts, 0, 3, C.byref(io), C.byref(wk.rec["_c"]), C.byref(wk.fill["_c"]), 0, 1, C.byref(out),
                                                    None)
        return rc, out.value, s.last_error

    rc, out, why = call(17)
    assert rc == -1 and out == -7 and "max_contacts must be 1 .. 16" in why
    rc, out, why = call(wk.ro.M, torch.zeros((1, 4, 10, 6), device="cuda"))
    assert rc == -1 and out == -7 and "dWrenchTicks is not taken" in why
    after = wk.host()
    for k in before:
        _same_bits(after[k], before[k], k)
    # the same call without either is taken
    rc, out, why = call(wk.ro.M)
    assert rc == 0 and out == 0
    assert (wk.host()["fill_trial_of"] == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]]).all()


# ---- 6. no host read ----
def test_no_host_read_inside_the_refill_walk():
    """the whole of walk_device_refill under torch's sync debug mode: a host read or a synchronisation inside it raises"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    com0, dcom0, h0, push = _start(6)
    ro = cm.rollout.WalkingRollout(cfg, 4)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device_refill(6, 3, com0, dcom0, h0, push=push, push_ticks=2)
        tr = w["trials"]["trace"](5)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert w["trials"]["ticks"].cpu().numpy().tolist() == [3] * 6 and w["trials"]["slot"].cpu().numpy().tolist() == [0, 1, 2, 3, 0, 1]
    assert tr["valid"].cpu().numpy().all() and (tr["iterations"].cpu().numpy() > 0).all()


# ---- 7. the kernel against the host form ----
def _both(a, tick_next, trial_ticks, s, live=True, tick_first=0):
    """one refill call on copies of the arrays `a`: the host form and the kernel; both results on the host"""
    import torch
    lib = cm._capi.lib()
    h = {k: v.copy() for k, v in a.items()}
    rec, f = rf.structs(h, trial_ticks, tick_first)
    assert lib.cmpc_rollout_refill(h["trial"].shape[0], tick_next, C.byref(rec), C.byref(f), h["state"].ctypes.data if live else None) == 0
    d = rf.to_cuda(a)
    rec, f = rf.structs(d, trial_ticks, tick_first)
    refill = dict(_c=f, start_tick=d["start_tick"])
    s.rollout_refill_device(tick_next, dict(_c=rec), refill, d["state"] if live else None)
    torch.cuda.synchronize()
    return h, rf.to_host(d)


def test_refill_kernel_matches_the_host_form_crafted():
    """the CPU test's B = 5, Q = 7 case, call by call from the same inputs, the init launch included"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    s = cm.BatchSolver(cfg, 5)
    a = rf.arrays(5, 7, rows=4, seed=3)
    d = rf.to_cuda(a)
    rec, f = rf.structs(d, 3)
    assert cm._capi.lib().cmpc_rollout_refill_init_device(s._h, C.byref(f), None) == 0
    torch.cuda.synchronize()
    rec, f = rf.structs(a, 3)
    assert cm._capi.lib().cmpc_rollout_refill_init(5, C.byref(f)) == 0
    for k, v in rf.to_host(d).items():
        _same_bits(v, a[k], "init " + k)
    steps = [(0, True), (3, True), (3, True), (4, False)]
    for i, (tick_next, live) in enumerate(steps):
        if i == 1:
            a["start_tick"][:4] = 1
            a["end_tick"][[1, 3]] = 1
            a["end_code"][[1, 3]] = 3
        if i == 2:
            a["iterations_sum"][0] += 7
        h, g = _both(a, tick_next, 3, s, live)
        for k in h:
            _same_bits(g[k], h[k], f"call {i} {k}")
        a = h
    assert a["trial"].tolist() == [0, 5, 2, 6, -1] and a["q_ticks"].tolist() == [3, 2, 3, 2, 3, 1, 1]
    s.close()


def test_refill_kernel_matches_the_host_form_chunks():
    """B = 300, Q = 1000, every third slot ended: more than one chunk of the workgroup and a partial last chunk; then a second call that runs the queue dry"""
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    B, Q = 300, 1000
    s = cm.BatchSolver(cfg, B)
    a = rf.arrays(B, Q, rows=3, seed=17)
    rec, f = rf.structs(a, 50)
    assert cm._capi.lib().cmpc_rollout_refill_init(B, C.byref(f)) == 0
    h, g = _both(a, 0, 50, s)
    for k in h:
        _same_bits(g[k], h[k], "fill " + k)
    assert h["trial"].tolist() == list(range(B)) and h["next"][0] == B
    a = h
    a["end_tick"][::3] = 1
    h, g = _both(a, 2, 50, s)
    for k in h:
        _same_bits(g[k], h[k], "refill " + k)
    assert h["trial"][::3].tolist() == list(range(B, B + 100)) and h["next"][0] == B + 100 and (h["trial_of"][2] == h["trial"]).all()
    a = h
    a["next"][0] = Q - 7          # seven trials left for the hundred slots that end now
    a["end_tick"][1::3] = 0
    h, g = _both(a, 3, 50, s, tick_first=1)
    for k in h:
        _same_bits(g[k], h[k], "dry " + k)
    assert h["next"][0] == Q and h["trial"][1::3][:7].tolist() == list(range(Q - 7, Q)) and (h["trial"][1::3][7:] == -1).all()
    assert (h["end_tick"][1::3][7:] == 3).all()
    s.close()


# ---- 8. the kernel at the edges of a wave and of a chunk ----
@pytest.fixture(scope="module")
def solvers():
    """one handle per batch size for the edge cases below (the refill launch takes nothing from a handle but its batch size and stream)"""
    made = {}

    def get(B):
        if B not in made:
            made[B] = cm.BatchSolver(cm.config.ergocub_gazebo_v1(10, 0.06), B)
        return made[B]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("Qrule", ["Q0", "QB-1", "Q3B"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 513])
def test_refill_kernel_at_wave_and_chunk_edges(B, Qrule, solvers):
    """Three calls, the kernel against the host form on every array and both against the assignment model: the first fill (tick 0); tick 2 with a random third
    of the slots ended at local tick 1 -- slot 0, the last slot and the slots either side of every multiple of 64 among them; tick 3 with every occupied slot
    ended and at most seven trials left in the queue (the trials in between are skipped by moving *dNext, and the model's trial numbers with them), so the
    queue runs dry inside a chunk.  trial_ticks = 50: nobody walks through."""
    Q = {"Q0": 0, "QB-1": B - 1, "Q3B": 3 * B}[Qrule]
    s = solvers(B)
    rng = np.random.default_rng(100 * B + Q)
    ended = set(rng.choice(B, B // 3, replace=False).tolist()) | {0, B - 1}
    ended |= {b for k in range(64, B + 2, 64) for b in (k - 1, k, k + 1) if b < B}
    ended = np.array(sorted(ended))
    a = rf.arrays(B, Q, rows=4, seed=B + Q)
    a["end_tick"][:] = -1
    without = tuple(k for _, k, _, _ in rf.TRIAL) + ("state0",) if Q == 0 else ()
    rec, f = rf.structs(a, 50, without=without)
    assert cm._capi.lib().cmpc_rollout_refill_init(B, C.byref(f)) == 0

    def call(a, tick, name):
        h, g = _both(a, tick, 50, s)
        for k in h:
            _same_bits(g[k], h[k], f"{name} {k}")
        return h

    a = call(a, 0, "fill")
    first = min(B, Q)                                   # (the trials of the first fill: trial b in slot b)
    sat = ended[ended < first]
    a["end_tick"][sat], a["end_code"][sat] = 1, 3
    a = call(a, 2, "refill")
    n2 = int(a["next"][0])
    left = min(7, Q - n2)
    skipped = Q - left - n2
    a["next"][0] = Q - left
    occupied = a["trial"] >= 0
    a["end_tick"][occupied] = 2 - a["start_tick"][occupied]
    a["end_code"][occupied] = 3
    a = call(a, 3, "dry")
    assert a["next"][0] == Q

    # the model: the queue without the skipped trials; trials of the first fill end at local tick 1 or 2, the ones spawned at tick 2 at local tick 0
    end_local = np.zeros(Q - skipped, int)
    end_local[:first] = 2
    end_local[sat] = 1
    m = rf.assignment_model(B, Q - skipped, 50, 4, end_local)
    number = lambda q: np.where(q >= n2, q + skipped, q)      # (the model's trial -> the queue's)
    for t in (0, 2, 3):
        np.testing.assert_array_equal(a["trial_of"][t], number(m["trial_of"][t]), err_msg=f"tick {t}")
    np.testing.assert_array_equal(a["trial"], number(m["trial_of"][3]))
    assert n2 == np.count_nonzero(m["start"][:n2] >= 0) and (m["start"][n2:] == 3).sum() == left
    if Q:
        took = number(np.arange(Q - skipped))
        np.testing.assert_array_equal(a["q_slot"][took], m["slot"])
        np.testing.assert_array_equal(a["q_start"][took], m["start"])
        lost = np.setdiff1d(np.arange(Q), took)
        assert (a["q_slot"][lost] == -1).all() and (a["q_start"][lost] == -1).all()
        sits = a["trial"] >= 0
        np.testing.assert_array_equal(a["start_tick"][sits], a["q_start"][a["trial"][sits]])
    assert (a["end_tick"][a["trial"] < 0] >= 0).all()


# ---- 9. the handle after a refill walk ----
def test_handle_is_usable_after_a_refill_walk():
    """the walk puts its record's end_tick in the handle's ended mask and turns the timing off, and restores both: a walk_device on the same object behind a
    refill walk (a trial ended, the queue run dry, so slots went out through the mask) is the walk_device of a fresh object; an ended mask the caller had
    installed is still there behind the refill walk, and a solve leaves the masked problem's rows alone"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(10, 0.06)
    com0, dcom0, h0, push = _start(6, seed=51)
    wrench = _push_rows(push.astype(np.float32), 2, 10)[:, :6]
    wrench = np.concatenate([wrench, np.zeros((1,) + wrench.shape[1:], np.float32)])       # (4 rows = trial_ticks)
    wrench[1, 2] = np.nan                                                                 # (trial 2 ends at its local tick 1)
    c4, d4, h4, p4 = _start(4, seed=52)

    def refill(ro):
        w = ro.walk_device_refill(10, 4, com0, dcom0, h0, wrench_trials=wrench)
        torch.cuda.synchronize()
        t = w["trials"]
        m = rf.assignment_model(4, 6, 4, 10, [-1, -1, 1, -1, -1, -1])
        assert t["end_tick"].cpu().numpy().tolist() == m["end_tick"].tolist() == [-1, -1, 1, -1, -1, -1]
        assert w["trial_of"].cpu().numpy().tolist() == m["trial_of"].tolist() and (m["trial_of"][-1] == -1).all()
        assert (w["end_tick"].cpu().numpy() >= 0).all()
        return w

    want = _walk_arrays(cm.rollout.WalkingRollout(cfg, 4).walk_device(6, c4, d4, h4, push=p4, push_ticks=2))
    torch.cuda.synchronize()
    assert (want["end_tick"] == -1).all() and (want["iterations"] > 0).all()
    ro = cm.rollout.WalkingRollout(cfg, 4)
    refill(ro)
    got = _walk_arrays(ro.walk_device(6, c4, d4, h4, push=p4, push_ticks=2))
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k in want:
        _same_bits(got[k], want[k], k)

    # an ended mask of the caller's
    def masked_solve(walk_first):
        ro = cm.rollout.WalkingRollout(cfg, 4)
        mask = torch.tensor([-1, 5, -1, -1], dtype=torch.int32, device="cuda")
        ro.solver.set_ended_device(mask)
        if walk_first:
            refill(ro)
        dP, dX0 = torch.from_numpy(want["P"]).cuda(), torch.from_numpy(want["X"]).cuda()
        dX, dInfo = torch.full_like(dX0, 777.0), torch.full((4, 8), 777.0, device="cuda")
        ro.solver.solve_device(dP, dX0, dX, dInfo)
        torch.cuda.synchronize()
        assert ro.solver._ended is mask and mask.cpu().numpy().tolist() == [-1, 5, -1, -1]
        return dX.cpu().numpy(), _no_clock(dInfo.cpu().numpy())

    X, info = masked_solve(True)
    assert (X[1] == 777.0).all() and (info[1, [0, 1, 2, 3, 4, 5, 7]] == 777.0).all()
    assert (X[[0, 2, 3]] != 777.0).any(1).all() and (info[[0, 2, 3], 5] == 0).all()
    X0, info0 = masked_solve(False)
    _same_bits(X, X0, "X")
    _same_bits(info, info0, "info")
