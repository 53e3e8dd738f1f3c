"""The device walk in forward mode (include/cmpc.h: cmpc_rollout_walk_jvp_device and its gate; WalkingRollout.forward_sensitivity_device, the jvp of
rollout_differentiable(device_walk=True)).  Comparisons of bits throughout -- the gate kernel against the host form, the device form against
run(tape=True) + forward_sensitivity(), one call against two segments, columns at k = 9 against k = 2, an ended problem against the shorter walk it
amounts to -- but for one adjoint identity against backward_device(), endings included, held to 5 x ADJ (five chained ticks, the per-tick bound of
tests/test_gpu_rollout_jvp.py).  N = 10, dt = 0.06, the ergoCubGazeboV1 weights."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_jvp_ref as wj
from tests import walk_tape_ref as wt
from tests.test_gpu_rollout_jvp import ADJ, _tick_directions
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_tape import _same_bits

pytestmark = pytest.mark.gpu

N = 10
KEYS = ("states", "list", "list_rot", "X", "status", "removed")


def _cfg():
    return cm.config.ergocub_gazebo_v1(N, 0.06)


def _host(r, keys=KEYS):
    return {k: r[k].cpu().numpy() for k in keys if k in r}


def _directions(cfg, B, k, M, T, seed):
    """k random columns of every direction group of forward_sensitivity[_device], as its keyword arguments"""
    rng = np.random.default_rng(seed)
    d = _tick_directions(rng, cfg, B, k, M)
    return dict(dir_state0=d["state"], dir_list0=d["list"], dir_list_rot0=d["list_rot"], dir_plan=d["plan"], dir_plan_rot=d["plan_rot"],
                dir_push=rng.normal(size=(B, k, 3)).astype(np.float32), dir_models=d["model"],
                dir_wrench=rng.normal(size=(T, B, k, N, 6)).astype(np.float32))


def _cols(d, sel):
    return {name: (a[:, :, sel] if name == "dir_wrench" else a[:, sel]) for name, a in d.items()}


# ---- 1. the gate kernel against the host form ----
@pytest.mark.parametrize("B", [70, 300])
def test_gate_kernel_matches_the_host_form(B):
    """the three kinds of gate step -- PRE only (the first of a call), POST + PRE, POST only -- at k = 3, with and without the row of dx, with and without the
    rotation carry, random end ticks, NaN in everything the tick left for an ended problem and in its rows of what enters: every array the kernel writes
    against the host form, to the bit.  B = 70 is a partial wave of columns, B = 300 a second workgroup"""
    import torch
    from tests.test_walk_jvp_cpu import _ptr
    cfg = _cfg()
    s, L, M, K, T = cm.BatchSolver(cfg, B), cm.Layout(N), 5, 3, 6
    lib = cm._capi.lib()
    rng = np.random.default_rng(B)
    e = rng.integers(-1, T + 1, B).astype(np.int32)
    assert (e == -1).any() and (e == 0).any() and (e == T).any()
    e_d = torch.from_numpy(e).cuda()
    outs = ("state", "list", "list_rot", "x", "status", "removed", "ok_out", "first_state", "first_list", "first_list_rot")
    for kind, t_post, with_x, with_rot in [("pre", 3, True, True), ("pre", -1, True, False), ("both", 3, True, True), ("both", 1, False, True),
                                            ("both", 0, True, False), ("post", T - 1, True, True), ("post", 2, False, False)]:
        t_pre = t_post + 1
        h = dict(sens=rng.integers(0, 6, (B, wt.SENS)).astype(np.float32), state=rng.normal(size=(B, K, 9)), list=rng.normal(size=(B, K, 2, M, 3)),
                 list_rot=rng.normal(size=(B, K, 2, M, 3)), x=rng.normal(size=(B, K, L.nx)).astype(np.float32), status=np.full((B,), -9, np.int32),
                 removed=np.full((B,), -9.0, np.float32), ok_row=rng.integers(0, 2, B).astype(np.int32), ok_out=np.full((B,), -9, np.int32),
                 first_state=rng.normal(size=(B, K, 9)), first_list=rng.normal(size=(B, K, 2, M, 3)), first_list_rot=rng.normal(size=(B, K, 2, M, 3)))
        if kind != "pre":
            for k in ("sens", "state", "list", "list_rot", "x"):
                h[k][wt.ended(e, t_post)] = np.nan
        else:
            for k in ("first_state", "first_list", "first_list_rot"):
                h[k][wt.ended(e, t_pre - 1)] = np.nan
        before = {k: v.copy() for k, v in h.items()}
        d = {k: torch.from_numpy(v).cuda() for k, v in h.items()}

        def gate(p, e_ptr):
            g = cm._capi.CmpcWalkJvpGate()
            g.batch, g.max_contacts, g.horizon, g.k, g.end_tick = B, M, N, K, e_ptr
            g.do_post, g.tick_post, g.do_pre, g.tick_pre, g.first = int(kind != "pre"), t_post, int(kind != "post"), t_pre, int(kind == "pre")
            g.tick_sens, g.state_out, g.list_out, g.status_row, g.removed_row = p("sens"), p("state"), p("list"), p("status"), p("removed")
            g.ok_row, g.ok_out, g.first_state, g.first_list = p("ok_row"), p("ok_out"), p("first_state"), p("first_list")
            if with_x:
                g.x_row = p("x")
            if with_rot:
                g.list_rot_out, g.first_list_rot = p("list_rot"), p("first_list_rot")
            return g
        assert lib.cmpc_rollout_walk_jvp_gate(C.byref(gate(lambda k: _ptr(h[k]), _ptr(e)))) == 0
        s.rollout_walk_jvp_gate_device(gate(lambda k: d[k].data_ptr(), e_d.data_ptr()))
        torch.cuda.synchronize()
        for k in outs:
            _same_bits(d[k], h[k], f"{kind}, tick {t_post}: {k}")
        written = set()
        if kind != "pre":
            en = wt.ended(e, t_post)
            want = wj.gate_post(e, t_post, {k: before[k] for k in ("state", "list", "list_rot", "x", "sens")})
            written |= {"state", "list", "status", "removed"} | ({"x"} if with_x else set()) | ({"list_rot"} if with_rot else set())
            for k in written:
                _same_bits(h[k], want[k], f"{kind}, tick {t_post}: {k} against the restatement")
                assert np.isfinite(h[k]).all() and (h[k][en] == (6 if k == "status" else 0)).all(), k
        if kind != "post":
            written |= {"ok_out"}
            np.testing.assert_array_equal(h["ok_out"], np.where(wt.ended(e, t_pre), 0, h["ok_row"]))
        if kind == "pre":
            gone = wt.ended(e, t_pre - 1)
            for k in ("first_state", "first_list") + (("first_list_rot",) if with_rot else ()):
                written.add(k)
                assert np.isfinite(h[k]).all() and (h[k][gone] == 0).all()
                _same_bits(h[k][~gone], before[k][~gone], k)
        for k in set(outs) - written:      # what a part does not own is left alone, NaN and all
            _same_bits(h[k], before[k], f"{kind}, tick {t_post}: {k} must not be written")


# ---- 2, 3: one walk of 16 ticks, taped on the host and on the device ----
@pytest.fixture(scope="module")
def walk16():
    import torch
    cfg = _cfg()
    B, ticks = 8, 16
    com0, dcom0, h0, push = _start(B)
    ro_run = cm.rollout.WalkingRollout(cfg, B)
    rec = ro_run.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False, tape=True)
    assert all(rec["merge_ok"]) and len(rec["tape"]["ticks"]) == ticks
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(ticks, com0, dcom0, h0, push=push, push_ticks=3)
    d9 = _directions(cfg, B, 9, ro.M, ticks, 4)
    d2 = _cols(d9, slice(0, 2))
    ref2 = ro_run.forward_sensitivity(rec["tape"], solutions=True, **d2)
    got2 = ro.forward_sensitivity_device(w, solutions=True, **d2)
    torch.cuda.synchronize()
    return dict(cfg=cfg, B=B, ticks=ticks, rec=rec, w=w, ro=ro, d9=d9, d2=d2, ref2=_host(ref2), got2=_host(got2))


def test_device_form_is_the_host_driven_form(walk16):
    """forward_sensitivity_device at k = 2, every direction group random, against forward_sensitivity on run(tape=True)'s tape: every key to the bit, status
    all 0; and again at k = 9 (two chunks of columns), whose columns 0:2 are the k = 2 result to the bit"""
    import torch
    w, ro, ref2, got2 = walk16["w"], walk16["ro"], walk16["ref2"], walk16["got2"]
    land = w["land"].cpu().numpy()
    assert land[4, 0, 0] == N and land[13, 0, 0] == 1 and (w["end_tick"].cpu().numpy() == -1).all()      # the landings are on the path
    assert set(got2) == set(KEYS) == set(ref2)
    for k in KEYS:
        _same_bits(got2[k], ref2[k], k)
    assert (got2["status"] == 0).all() and np.isfinite(got2["states"]).all()
    assert np.abs(got2["states"][-1]).max() > 0 and np.abs(got2["list"]).max() > 0 and np.abs(got2["list_rot"]).max() > 0 and np.abs(got2["X"]).max() > 0
    got9 = ro.forward_sensitivity_device(w, solutions=True, **walk16["d9"])
    torch.cuda.synchronize()
    got9 = _host(got9)
    assert (got9["status"] == 0).all()
    for k in ("states", "X"):
        _same_bits(got9[k][:, :, :2], got2[k], f"k = 9, columns 0:2: {k}")
        assert np.abs(got9[k][:, :, 8]).max() > 0
    for k in ("list", "list_rot"):
        _same_bits(got9[k][:, :2], got2[k], f"k = 9, columns 0:2: {k}")
    _same_bits(got9["removed"], got2["removed"], "removed")
    # without a rotation direction the results are those of the chain without it, and list_rot comes back zero
    plain = {k: v for k, v in walk16["d2"].items() if k not in ("dir_list_rot0", "dir_plan_rot")}
    a = ro.forward_sensitivity_device(w, solutions=True, **plain)
    b = walk16["ro"].forward_sensitivity(walk16["rec"]["tape"], solutions=True, **plain)
    torch.cuda.synchronize()
    for k in KEYS:
        _same_bits(a[k], b[k], f"no rotation chain: {k}")
    assert not bool(a["list_rot"].any())


def test_segments_compose_on_the_device(walk16):
    """rows 0 .. 7 and then 8 .. 15 through the state rows and the two carries against one call over 0 .. 15, to the bit; and the argument checks that need
    a handle"""
    import torch
    ro, w, d = walk16["ro"], walk16["w"], walk16["d2"]
    B, T, M, dev, k, L = walk16["B"], walk16["ticks"], ro.M, ro.dev, 2, ro.L
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    res = []
    with torch.cuda.stream(ro.solver.launch_stream):
        for calls in (((0, 16),), ((0, 8), (8, 8))):
            o = dict(states=z((T + 1, B, k, 9)), X=z((T, B, k, L.nx), torch.float32), status=z((T, B), torch.int32), removed=z((T, B), torch.float32),
                     list=cu(d["dir_list0"]), list_rot=cu(d["dir_list_rot0"]))
            o["states"][0] = cu(d["dir_state0"])
            for t0, n in calls:
                ro.solver.rollout_walk_jvp_device(t0, n, w["tape"], t0, w["end_tick"], k, o["states"], o["list"], o["status"], carry_list_rot=o["list_rot"],
                                                  dir_plan=cu(d["dir_plan"]), dir_plan_rot=cu(d["dir_plan_rot"]), dir_wrench=cu(d["dir_wrench"]),
                                                  dir_model=cu(d["dir_models"]), dir_x=o["X"], removed=o["removed"])
            res.append(o)
    torch.cuda.synchronize()
    for key in KEYS:
        _same_bits(res[1][key], res[0][key], key)
    assert (res[0]["status"].cpu().numpy() == 0).all() and float(res[0]["list"].abs().max()) > 0
    # an odd number of ticks leaves the carries in the caller's buffers too: 0 .. 6, 7 .. 15
    o = dict(states=z((T + 1, B, k, 9)), status=z((T, B), torch.int32), list=cu(d["dir_list0"]), list_rot=cu(d["dir_list_rot0"]))
    o["states"][0] = cu(d["dir_state0"])
    with torch.cuda.stream(ro.solver.launch_stream):
        for t0, n in ((0, 7), (7, 9)):
            ro.solver.rollout_walk_jvp_device(t0, n, w["tape"], t0, w["end_tick"], k, o["states"], o["list"], o["status"], carry_list_rot=o["list_rot"],
                                              dir_plan=cu(d["dir_plan"]), dir_plan_rot=cu(d["dir_plan_rot"]), dir_wrench=cu(d["dir_wrench"]),
                                              dir_model=cu(d["dir_models"]))
    torch.cuda.synchronize()
    for key in ("states", "list", "list_rot", "status"):
        _same_bits(o[key], res[0][key], f"7 + 9 ticks: {key}")
    # rows outside the tape, k = 0, missing pointers, and a tape whose row 0 is not a first tick
    s, tp = ro.solver, w["tape"]
    full = cm._capi.CmpcWalkDirs(o["states"].data_ptr(), o["list"].data_ptr(), None, None, None, None, None, None, None, o["status"].data_ptr(), None)
    call = lambda tick0, n, row0, kk=k, dd=full: s._lib.cmpc_rollout_walk_jvp_device(s._h, M, tick0, n, C.byref(tp["_c"]), row0, None, kk, C.byref(dd), None)
    assert call(0, T + 1, 0) != 0 and call(0, 1, T) != 0 and call(0, 0, 0) != 0 and call(0, 1, -1) != 0 and call(0, 1, 0, kk=0) != 0
    for missing in ("dDirStates", "dCarryList", "dStatus"):
        dd = cm._capi.CmpcWalkDirs.from_buffer_copy(full)
        setattr(dd, missing, None)
        assert call(0, 1, 0, dd=dd) != 0, missing
    dd = cm._capi.CmpcWalkDirs.from_buffer_copy(full)
    dd.dDirPlanRot = o["list_rot"].data_ptr()
    assert call(0, 1, 0, dd=dd) != 0      # the planner's orientation directions without a carry for them
    tp["_c"].first_row_is_first_tick = 0
    try:
        assert call(0, 1, 0) != 0
    finally:
        tp["_c"].first_row_is_first_tick = 1
    torch.cuda.synchronize()


# ---- 4, 5: an ended problem ----
@pytest.fixture(scope="module", params=[False, True], ids=["stay", "skip_ended"])
def ended_walk(request):
    """the replan of test_an_ended_problem_keeps_its_gradient_and_the_others_theirs: problem 3 ends at tick 2 (code 1) of 5; the same batch without the
    replan; the 2-tick walk"""
    cfg = _cfg()
    B, T = 8, 5
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    push = np.zeros((B, 3)); push[:, 0] = np.linspace(-0.2, 0.2, B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    t[3, 0] += 100.0
    kw = dict(push=push, push_ticks=2, skip_ended=request.param)
    w = ro.walk_device_taped(T, com0, z, z, replan={2: (t, ro.plan[1], ro.plan[2])}, **kw)
    ro_b, ro_2 = cm.rollout.WalkingRollout(cfg, B), cm.rollout.WalkingRollout(cfg, B)
    base = ro_b.walk_device_taped(T, com0, z, z, **kw)
    two = ro_2.walk_device_taped(2, com0, z, z, **kw)
    assert w["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and int(w["end_code"][3]) == 1
    assert (base["end_tick"].cpu().numpy() == -1).all() and (two["end_tick"].cpu().numpy() == -1).all()
    return dict(cfg=cfg, B=B, T=T, ro=ro, w=w, ro_b=ro_b, base=base, ro_2=ro_2, two=two, com0=com0, kw=kw)


def test_an_ended_problem_keeps_its_directions_and_the_others_theirs(ended_walk):
    """NaN in problem 3's rows >= 2 of dir_wrench.  The seven others are bit-equal to the batch without the replan; problem 3's state rows 0 .. 2 and X rows
    0 .. 1 are a 2-tick walk's; its state rows 3 .., X rows 2 .. and final list directions are exactly zero, its status [0, 0, 6, 6, 6]; nothing is
    non-finite anywhere.  A problem whose com0 is NaN ends at tick 0: state row 0 is its dir_state0, everything else zero, status 6 throughout."""
    import torch
    v = ended_walk
    cfg, B, T, ro = v["cfg"], v["B"], v["T"], v["ro"]
    d = _directions(cfg, B, 2, ro.M, T, 8)
    d_nan = dict(d, dir_wrench=d["dir_wrench"].copy())
    d_nan["dir_wrench"][2:, 3] = np.nan
    got = ro.forward_sensitivity_device(v["w"], solutions=True, **d_nan)
    ref = v["ro_b"].forward_sensitivity_device(v["base"], solutions=True, **d)
    short = v["ro_2"].forward_sensitivity_device(v["two"], solutions=True, **dict(d, dir_wrench=d["dir_wrench"][:2]))
    torch.cuda.synchronize()
    got, ref, short = _host(got), _host(ref), _host(short)
    for k in KEYS:
        assert np.isfinite(got[k]).all(), k
    others = [0, 1, 2, 4, 5, 6, 7]
    for k in KEYS:
        ax = 0 if k in ("list", "list_rot") else 1
        _same_bits(np.take(got[k], others, axis=ax), np.take(ref[k], others, axis=ax), k)
    assert (ref["status"] == 0).all() and np.abs(ref["list"]).max() > 0
    _same_bits(got["states"][:3, 3], short["states"][:, 3], "problem 3: states 0 .. 2")
    _same_bits(got["X"][:2, 3], short["X"][:, 3], "problem 3: X rows 0 .. 1")
    _same_bits(got["removed"][:2, 3], short["removed"][:, 3], "problem 3: removed")
    assert np.abs(got["states"][2, 3]).max() > 0 and np.abs(got["X"][:2, 3]).max() > 0
    assert (got["states"][3:, 3] == 0).all() and (got["X"][2:, 3] == 0).all() and (got["list"][3] == 0).all() and (got["list_rot"][3] == 0).all()
    assert got["status"][:, 3].tolist() == [0, 0, 6, 6, 6] and short["status"][:, 3].tolist() == [0, 0] and (got["removed"][2:, 3] == 0).all()
    # a problem that never had a finite state
    bad = v["com0"].copy()
    bad[5] = np.nan
    zz = np.zeros((B, 3))
    ro_n = cm.rollout.WalkingRollout(cfg, B)
    wn = ro_n.walk_device_taped(3, bad, zz, zz, **v["kw"])
    dn = dict(d, dir_wrench=d["dir_wrench"][:3])
    gn = ro_n.forward_sensitivity_device(wn, solutions=True, **dn)
    torch.cuda.synchronize()
    assert int(wn["end_tick"][5]) == 0 and (np.delete(wn["end_tick"].cpu().numpy(), 5) == -1).all()
    gn = _host(gn)
    _same_bits(gn["states"][0, 5], d["dir_state0"][5], "ended at tick 0: state row 0 is its dir_state0")
    assert (gn["states"][1:, 5] == 0).all() and (gn["X"][:, 5] == 0).all() and (gn["list"][5] == 0).all() and (gn["list_rot"][5] == 0).all()
    assert (gn["status"][:, 5] == 6).all() and (gn["removed"][:, 5] == 0).all() and (np.delete(gn["status"], 5, axis=1) == 0).all()
    for k in KEYS:
        assert np.isfinite(gn[k]).all(), k


def test_forward_and_reverse_are_adjoint_on_the_device_endings_included(ended_walk):
    """forward_sensitivity_device (state0, list0, plan, push, models; k = 2; solutions) against backward_device with random grad_states / grad_X on the
    walk problem 3 ends in: per problem and column sum_i <gS_i, dS_i> + sum_i <gX_i, dX_i> over ALL rows equals the contraction of state0, list0, plan,
    push, models with their directions -- the forward zeros and the reverse rule make the rows past the end drop out.  Relative gap <= 5 x ADJ (five
    chained ticks).  Problem 3 is included, both its sides non-zero."""
    import torch
    v = ended_walk
    cfg, B, T, ro, w = v["cfg"], v["B"], v["T"], v["ro"], v["w"]
    d = _directions(cfg, B, 2, ro.M, T, 12)
    d = {k: d[k] for k in ("dir_state0", "dir_list0", "dir_plan", "dir_push", "dir_models")}
    rng = np.random.default_rng(13)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    f = ro.forward_sensitivity_device(w, solutions=True, **d)
    r = ro.backward_device(w, gS, gX)
    torch.cuda.synchronize()
    fs, fx = f["states"].cpu().numpy(), f["X"].cpu().numpy().astype(np.float64)
    pairs = (("state0", d["dir_state0"]), ("list0", d["dir_list0"]), ("plan", d["dir_plan"]), ("push", d["dir_push"].astype(np.float64)),
             ("models", d["dir_models"]))
    rh = {name: r[name].cpu().numpy() for name, _ in pairs}
    assert f["status"].cpu().numpy()[:, 3].tolist() == [0, 0, 6, 6, 6] and r["status"].cpu().numpy()[:, 3].tolist() == [0, 0, 6, 6, 6]
    worst = 0.0
    for b in range(B):
        for j in range(2):
            lhs = float((gS[:, b] * fs[:, b, j]).sum() + (gX[:, b].astype(np.float64) * fx[:, b, j]).sum())
            terms = {name: float((rh[name][b] * dd[b, j]).sum()) for name, dd in pairs}
            rhs = sum(terms.values())
            gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)
            worst = max(worst, gap)
            print(f"problem {b} column {j}: forward {lhs:.9e}  reverse {rhs:.9e}  gap {gap:.2e}  terms " + " ".join(f"{n} {t:.1e}" for n, t in terms.items()))
            if b == 3:
                assert lhs != 0.0 and rhs != 0.0
    print(f"forward walk against reverse walk on the device over {T} ticks, worst gap over {B} problems x 2 columns: {worst:.2e} (bound {5 * ADJ:.1e})")
    assert worst <= 5 * ADJ


# ---- 6. no host read ----
def test_nothing_is_read_back(walk16):
    """walk_device_taped(replan, skip_ended=True) + forward_sensitivity_device under torch's sync debug mode, after a first call has allocated the workspaces"""
    import torch
    ro, B, cfg = walk16["ro"], walk16["B"], walk16["cfg"]
    com0, dcom0, h0, push = _start(B)
    t = ro.plan[0].clone()
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(ro.dev) for k, v in _directions(cfg, B, 2, ro.M, 6, 5).items()}
    kw = dict(push=push, push_ticks=2, replan={3: (t, ro.plan[1], ro.plan[2])}, skip_ended=True)
    ro.forward_sensitivity_device(ro.walk_device_taped(6, com0, dcom0, h0, **kw), solutions=True, **d)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device_taped(6, com0, dcom0, h0, **kw)
        r = ro.forward_sensitivity_device(w, solutions=True, **d)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert (w["end_tick"].cpu().numpy() == -1).all() and (r["status"].cpu().numpy() == 0).all() and w["tape"]["segments"] == [0, 3]
    assert np.isfinite(r["states"].cpu().numpy()).all() and float(r["states"][-1].abs().max()) > 0 and r["end_tick"] is w["end_tick"]


# ---- 7. autograd ----
def test_forward_mode_autograd_through_the_device_walk():
    """torch.autograd.forward_ad through rollout_differentiable(device_walk=True, models=dual) at B = 4, 6 ticks: the tangent equals
    forward_sensitivity_device's column bit for bit, and the non-device path's tangent when nothing ends; with problem 1 ended by a replan at tick 2 its
    tangent rows 3 .. equal its row 2, the others keep their bits, and everything is finite"""
    import torch
    import torch.autograd.forward_ad as fwAD
    cfg = _cfg()
    B, T = 4, 6
    com0, dcom0, h0, pushv = _start(B, seed=3)
    s0 = np.concatenate([com0, dcom0, h0], 1).astype(np.float32)
    theta = torch.from_numpy(np.tile(cm.config.model_row(cfg), (B, 1))).cuda()
    t_theta = torch.from_numpy(_tick_directions(np.random.default_rng(4), cfg, B, 1, 3)["model"][:, 0].copy()).cuda()

    def tangent(**kw):
        ro = cm.rollout.WalkingRollout(cfg, B)
        state0, push = torch.from_numpy(s0).cuda(), torch.from_numpy(pushv.astype(np.float32)).cuda()
        with fwAD.dual_level():
            states = cm.rollout_differentiable(ro, T, state0, push=push, models=fwAD.make_dual(theta, t_theta), push_ticks=3, **kw)
            primal, tan = fwAD.unpack_dual(states)
            assert tan is not None and tan.dtype == torch.float32 and tuple(tan.shape) == (T + 1, B, 9)
            primal, tan = primal.clone(), tan.clone()
        torch.cuda.synchronize()
        return ro, primal, tan
    _, st_a, tn_a = tangent()
    ro, st_b, tn_b = tangent(device_walk=True)
    _same_bits(st_b, st_a, "states")
    _same_bits(tn_b, tn_a, "the tangent against the non-device path's")
    assert (ro.last_walk["end_tick"].cpu().numpy() == -1).all() and bool(tn_b[1:].any()) and not bool(tn_b[0].any())
    col = ro.forward_sensitivity_device(ro.last_walk, dir_models=t_theta[:, None].contiguous())
    torch.cuda.synchronize()
    _same_bits(tn_b, col["states"][:, :, 0].to(torch.float32), "the tangent against forward_sensitivity_device's column")
    assert (ro.last_forward["status"].cpu().numpy() == 0).all()
    plan = cm.rollout.WalkingRollout(cfg, B).plan
    t = plan[0].clone()
    t[1, 0] += 100.0
    ro, st_c, tn_c = tangent(device_walk=True, replan={2: (t, plan[1], plan[2])})
    assert ro.last_walk["end_tick"].cpu().numpy().tolist() == [-1, 2, -1, -1]
    others = [0, 2, 3]
    _same_bits(tn_c[:, others], tn_a[:, others], "the tangents of the others")
    _same_bits(tn_c[:3, 1], tn_a[:3, 1], "the ended problem's tangent up to its end")
    _same_bits(tn_c[3:, 1], tn_c[2, 1][None].expand(T - 2, 9), "rows behind the end take the tangent of row e")
    assert bool(torch.isfinite(tn_c).all()) and bool(tn_c[2, 1].any())
    assert (ro.last_forward["status"][:, 1].cpu().numpy() == [0, 0, 6, 6, 6, 6]).all()
    col = ro.forward_sensitivity_device(ro.last_walk, dir_models=t_theta[:, None].contiguous())
    torch.cuda.synchronize()
    _same_bits(tn_c[:3], col["states"][:3, :, 0].to(torch.float32), "the tangent against forward_sensitivity_device's column, one problem ended")
    assert not bool(col["states"][3:, 1].any())
