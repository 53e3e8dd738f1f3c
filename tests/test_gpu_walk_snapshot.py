"""Walk snapshots on the GPU: (1) the copy kernel against the host form; (2) a checkpointed walk is the walk, and a walk resumed from a checkpoint on
another roll-out is the unbroken walk, with problems ended before and behind the checkpoint and at tick 0; (3) branching by index; (4) the reverse walk
from checkpoints against the full-tape reverse walk, orientations, a callable seed and ended problems included; (5) autograd; (6) no host read.
Every comparison is of bits.  N = 10, dt = 0.06, the ergoCubGazeboV1 weights."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_snapshot_ref as ws
from tests.test_gpu_walk_record import OUTCOME, _start
from tests.test_gpu_walk_tape import GRADS, _cfg, _same_bits

pytestmark = pytest.mark.gpu

N = 10
TRACE = ("com", "zmp", "land", "landing_offset", "iterations", "code")
KEYS = {"dState": "state", "dP": "P", "dX": "X", "dX0": "X0", "dInfo": "info", "dZmp": "zmp", "dOk": "ok", "dLand": "land", "dEndTick": "end_tick",
        "dEndCode": "end_code", "dIterationsSum": "iterations_sum", "dIterationsMax": "iterations_max", "dFinalState": "final_state",
        "dBoxSlackMin": "box_slack_min"}
LISTS = (("dListT", "dListPose", "dListN"), ("dListTB", "dListPoseB", "dListNB"))


def _to_snapshot(s, arr, M, batch, without=()):
    """host arrays (walk_snapshot_ref.arrays) as a snapshot dict of CUDA tensors"""
    import torch
    up = lambda a: torch.from_numpy(a).cuda()
    t = {v: (None if k in without else up(arr[k])) for k, v in KEYS.items()}
    t["lists"] = [tuple(up(arr[k]) for k in names) for names in LISTS]
    return s.walk_snapshot(3, 1, M, batch=batch, tensors=t)


def _from_snapshot(snap):
    out = {k: (None if snap[v] is None else snap[v].cpu().numpy()) for k, v in KEYS.items()}
    for names, st in zip(LISTS, snap["lists"]):
        out.update({k: a.cpu().numpy() for k, a in zip(names, st)})
    return out


# ---- 1. the kernel against the host form ----
@pytest.mark.parametrize("B", [70, 300])
@pytest.mark.parametrize("wide_lists", [False, True])
def test_snapshot_kernel_matches_the_host_form(B, wide_lists):
    import torch
    ro = cm.rollout.WalkingRollout(_cfg(), B)
    s, M, SB = ro.solver, 17 if wide_lists else ro.M, 9
    lib = cm._capi.lib()
    rng = np.random.default_rng(B + M)
    cases = {"identity": (None, B), "permutation": (rng.permutation(B).astype(np.int32), B), "all_equal": (np.full((B,), 4, np.int32), SB)}
    mixed = rng.integers(0, SB, B).astype(np.int32)
    mixed[[3, B - 1]] = -1
    mixed[[0, 17]] = SB
    cases["out_of_range"] = (mixed, SB)
    for name, (index, sb) in cases.items():
        without = ws.OPTIONAL if name == "all_equal" else ()         # (the optional arrays NULL in the destination once)
        src, dst = ws.arrays(N, M, sb, rng), ws.arrays(N, M, B, fill=0xA5)
        want = {k: v.copy() for k, v in dst.items()}
        ok_want = np.full((B,), -9, np.int32)
        hs, hd = ws.struct(src), ws.struct(want, without=without)
        assert lib.cmpc_rollout_snapshot(N, B, sb, M, C.byref(hs), C.byref(hd), None if index is None else index.ctypes.data_as(C.c_void_p),
                                         ok_want.ctypes.data_as(C.c_void_p)) == 0
        dsrc, ddst = _to_snapshot(s, src, M, sb), _to_snapshot(s, dst, M, B, without=without)
        ok = torch.full((B,), -9, dtype=torch.int32, device="cuda")
        s.rollout_snapshot_device(dsrc, ddst, None if index is None else torch.from_numpy(index).cuda(), ok)
        torch.cuda.synchronize()
        assert (ddst["tick"], ddst["lists_in"]) == (3, 1)
        got = _from_snapshot(ddst)
        np.testing.assert_array_equal(ok.cpu().numpy(), ok_want, err_msg=name)
        for k in want:
            if k not in without:
                np.testing.assert_array_equal(ws.bits(got[k]), ws.bits(want[k]), err_msg=f"{name}: {k}")
        if name == "out_of_range":
            assert (ok_want == 0).sum() == 4
            for k in got:
                assert (got[k][ok_want == 0].view(np.uint8) == 0xA5).all(), k
    # aliasing and sizes are refused by the device form too
    a, b = _to_snapshot(s, ws.arrays(N, M, B, rng), M, B), _to_snapshot(s, ws.arrays(N, M, B, fill=0), M, B)
    b["_c"].dLand = a["_c"].dLand
    with pytest.raises(RuntimeError):
        s.rollout_snapshot_device(a, b)
    b["_c"].dLand = b["land"].data_ptr()
    with pytest.raises(RuntimeError):
        s.rollout_snapshot_device(a, b, src_batch=B - 1)      # identity with src_batch != batch


# ---- 2. resume is the walk ----
def _walk_case(case, B=8):
    """(com0, dcom0, h0, kwargs, replan of a roll-out `ro`): the benign replan at tick 7; the one whose planner forgets problem 3's RIGHT foot -- the stance
    foot at tick 7, so that the merge fails there (the left foot of test_a_failed_merge_ends_one_problem_only is in the air at tick 7); a NaN com0"""
    com0, dcom0, h0, push = _start(B)
    if case == "nan":
        com0[6] = np.nan

    def replan(ro):
        t = ro.plan[0].clone()
        if case == "ends3":
            t[3, 1] += 100.0
        return {7: (t, ro.plan[1], ro.plan[2])}
    return com0, dcom0, h0, dict(push=push, push_ticks=3), replan


def _same_walk(got, ref, rows=None, msg=""):
    """every key of a walk's dict; rows: the rows of ref's trace and statistics that got's hold"""
    for k, v in ref.items():
        if k == "lists":
            for a, b in zip(got[k], v):
                _same_bits(a, b, msg + k)
        elif k == "info":        # (word 6 is the clock)
            _same_bits(got[k][:, :6], v[:, :6], msg + k)
            _same_bits(got[k][:, 7], v[:, 7], msg + k)
        elif k in TRACE or k == "stats":
            _same_bits(got[k], v if rows is None else v[rows], msg + k)
        else:
            _same_bits(got[k], v, msg + k)


@pytest.mark.parametrize("skip_ended", [False, True])
@pytest.mark.parametrize("case", ["benign", "ends3", "nan"])
def test_resume_is_the_walk(case, skip_ended):
    import torch
    cfg, B, T = _cfg(), 8, 16
    com0, dcom0, h0, kw, replan = _walk_case(case)
    ro_a, ro_b, ro_c = (cm.rollout.WalkingRollout(cfg, B) for _ in range(3))
    kw.update(skip_ended=skip_ended, replan=replan(ro_a))
    plain = ro_a.walk_device(T, com0, dcom0, h0, **kw)
    w = ro_b.walk_device_checkpointed(T, com0, dcom0, h0, 5, **kw)
    torch.cuda.synchronize()
    assert set(w) == set(plain) | {"checkpoints", "inputs"} and sorted(w["checkpoints"]) == [5, 10, 15]
    _same_walk(w, plain, msg="checkpointed: ")
    end = plain["end_tick"].cpu().numpy().tolist()
    assert end == {"benign": [-1] * 8, "ends3": [-1, -1, -1, 7, -1, -1, -1, -1], "nan": [-1] * 6 + [0, -1]}[case]
    # resumed on another roll-out of the same batch: checkpoint 10 (an end at tick 7 lies before it), checkpoint 5 (behind it)
    for c in (10, 5):
        r = ro_c.walk_resume_device(w["checkpoints"][c], T - c, replan=kw["replan"], skip_ended=skip_ended)
        torch.cuda.synchronize()
        assert r["tick0"] == c and (r["index_ok"].cpu().numpy() == 1).all() and tuple(r["com"].shape) == (T - c, B, 3)
        _same_walk(r, plain, rows=slice(c, T), msg=f"resumed at {c}: ")
    for k in OUTCOME:
        assert k in r


# ---- 3. branch ----
def test_branching_by_index():
    import torch
    cfg, B, T = _cfg(), 8, 16
    com0, dcom0, h0, push = _start(B)
    w = cm.rollout.WalkingRollout(cfg, B).walk_device_checkpointed(T, com0, dcom0, h0, 5, push=push, push_ticks=3)
    ro = cm.rollout.WalkingRollout(cfg, B)
    index = np.array([2, 2, 2, 2, 5, 5, 5, 5], np.int32)
    r = ro.walk_resume_device(w["checkpoints"][5], T - 5, index=index)
    torch.cuda.synchronize()
    per_problem = lambda d, k: d[k].movedim(1, 0) if k in TRACE else d[k]
    for k in list(TRACE) + list(OUTCOME) + ["X", "P", "state"]:
        a = per_problem(r, k)
        b = per_problem(w, k)[:, 5:] if k in TRACE else per_problem(w, k)
        for group, src in ((range(0, 4), 2), (range(4, 8), 5)):
            for d in group:
                _same_bits(a[d], a[group[0]], f"{k}: destination {d}")
            _same_bits(a[group[0]], b[src], f"{k}: destination {group[0]} against problem {src}")
    for j in range(3):
        _same_bits(r["lists"][j][0], w["lists"][j][2], "lists")
        _same_bits(r["lists"][j][7], w["lists"][j][5], "lists")
    assert (r["end_tick"].cpu().numpy() == -1).all()
    # the same robot under eight pushes from tick 5 on: eight outcomes, all finite
    pushes = np.zeros((B, 3))
    pushes[:, 0] = np.linspace(-0.3, 0.3, B)
    pushes[:, 1] = np.linspace(0.2, -0.2, B)
    r = ro.walk_resume_device(w["checkpoints"][5], 6, index=np.full((B,), 2, np.int32), push=pushes, push_ticks=2)
    torch.cuda.synchronize()
    fs = r["final_state"].cpu().numpy()
    assert np.isfinite(fs).all() and (r["end_tick"].cpu().numpy() == -1).all()
    assert len({fs[b].tobytes() for b in range(B)}) == B
    # an index outside the snapshot's batch: reported, and (taken out of the launches) the problem keeps its fill
    index = np.array([2, 2, 2, 8, 5, -1, 5, 5], np.int32)
    r = ro.walk_resume_device(w["checkpoints"][5], 3, index=index, skip_ended=True)
    torch.cuda.synchronize()
    assert r["index_ok"].cpu().numpy().tolist() == [1, 1, 1, 0, 1, 0, 1, 1]
    for k in ("X", "P", "state", "info"):
        assert (r[k][[3, 5]] == 0).all() and float(r[k][0].abs().max()) > 0, k
    assert r["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 0, -1, 0, -1, -1]


# ---- 4. the reverse walk from checkpoints ----
@pytest.fixture(scope="module")
def ref16():
    """the walk16 shape: B = 8, 16 ticks, random seeds on states and solutions; the full-tape reverse walk without and with the replan at 7, and with
    orientations"""
    import torch
    cfg, B, T = _cfg(), 8, 16
    com0, dcom0, h0, push = _start(B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    rng = np.random.default_rng(2)
    gS = torch.from_numpy(rng.normal(size=(T + 1, B, 9))).cuda()
    gX = torch.from_numpy((1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)).cuda()
    kw = dict(push=push, push_ticks=3)
    t = ro.plan[0].clone()
    replan = {7: (t, ro.plan[1], ro.plan[2])}
    w = ro.walk_device_taped(T, com0, dcom0, h0, **kw)
    ref, ref_rot = ro.backward_device(w, gS, gX), ro.backward_device_rot(w, gS, gX)
    ref_replan = ro.backward_device(ro.walk_device_taped(T, com0, dcom0, h0, replan=replan, **kw), gS, gX)
    torch.cuda.synchronize()
    assert (ref["status"].cpu().numpy() == 0).all() and float(ref["list0"].abs().max()) > 0
    return dict(cfg=cfg, B=B, T=T, start=(com0, dcom0, h0), kw=kw, replan=replan, gS=gS, gX=gX, ref=ref, ref_rot=ref_rot, ref_replan=ref_replan)


@pytest.mark.parametrize("case", ["every5", "every8", "every16", "every5_replan", "rot", "callable"])
def test_checkpointed_reverse_is_the_reverse(ref16, case):
    import torch
    T, gS, gX = ref16["T"], ref16["gS"], ref16["gX"]
    every = {"every8": 8, "every16": 16}.get(case, 5)
    kw = dict(ref16["kw"], replan=ref16["replan"]) if case == "every5_replan" else ref16["kw"]
    ro = cm.rollout.WalkingRollout(ref16["cfg"], ref16["B"])
    w = ro.walk_device_checkpointed(T, *ref16["start"], every, **kw)
    assert "tape" not in w and sorted(w["checkpoints"]) == list(range(every, T, every))
    seen = []

    def seeds(t0, t1, seg):      # the same rows, made per segment; the segment's tape rows are the ticks t0 .. t1 - 1
        seen.append((t0, t1, tuple(seg["X"].shape), tuple(seg["states"].shape)))
        return gX[t0:t1]
    got = ro.backward_device_checkpointed(w, gS, seeds if case == "callable" else gX, rot=case == "rot")
    torch.cuda.synchronize()
    ref = ref16["ref_rot" if case == "rot" else "ref_replan" if case == "every5_replan" else "ref"]
    assert set(got) == set(ref) | {"tape_rows_peak"}
    for k in ref:
        _same_bits(got[k], ref[k], k)
    assert got["tape_rows_peak"] == {5: 6, 8: 9, 16: 16}[every] and got["tape_rows_peak"] <= every + 1
    if case == "callable":
        assert [(a, b) for a, b, _, _ in seen] == [(15, 16), (10, 15), (5, 10), (0, 5)]
        assert seen[1][2] == (5, ref16["B"], ro.L.nx) and seen[1][3] == (6, ref16["B"], 9)


@pytest.mark.parametrize("skip_ended", [False, True])
@pytest.mark.parametrize("every", [2, 3])
def test_checkpointed_reverse_with_an_ended_problem(every, skip_ended):
    """the 5-tick case of test_an_ended_problem_keeps_its_gradient_and_the_others_theirs: problem 3 ends at tick 2 -- on a checkpoint boundary
    (every = 2) and inside a segment (every = 3); the seeds behind its end are NaN and nothing in the result is"""
    import torch
    cfg, B, T = _cfg(), 8, 5
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    push = np.zeros((B, 3)); push[:, 0] = np.linspace(-0.2, 0.2, B)
    ro_f, ro = cm.rollout.WalkingRollout(cfg, B), cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    t[3, 0] += 100.0
    kw = dict(push=push, push_ticks=2, skip_ended=skip_ended, replan={2: (t, ro.plan[1], ro.plan[2])})
    rng = np.random.default_rng(6)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    gS[3:, 3], gX[2:, 3] = np.nan, np.nan
    ref = ro_f.backward_device(ro_f.walk_device_taped(T, com0, z, z, **kw), gS, gX)
    w = ro.walk_device_checkpointed(T, com0, z, z, every, **kw)
    got = ro.backward_device_checkpointed(w, gS, gX)
    torch.cuda.synchronize()
    assert w["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 2, -1, -1, -1, -1]
    for k in GRADS:
        assert np.isfinite(got[k].cpu().numpy()).all(), k
        _same_bits(got[k], ref[k], k)
    assert got["status"][:, 3].cpu().numpy().tolist() == [0, 0, 6, 6, 6] and got["tape_rows_peak"] <= every + 1


# ---- 5. autograd ----
def test_autograd_from_checkpoints():
    import torch
    cfg, B, T = _cfg(), 4, 6
    com0, dcom0, h0, pushv = _start(B, seed=3)
    s0 = np.concatenate([com0, dcom0, h0], 1).astype(np.float32)
    theta = np.tile(cm.config.model_row(cfg), (B, 1))
    target = torch.tensor([0.05, 0.0, 0.7], device="cuda")

    def grads(fn, **kw):
        ro = cm.rollout.WalkingRollout(cfg, B)
        state0 = torch.from_numpy(s0).cuda().requires_grad_(True)
        push = torch.from_numpy(pushv.astype(np.float32)).cuda().requires_grad_(True)
        models = torch.from_numpy(theta).cuda().requires_grad_(True)
        states = fn(ro, T, state0, push=push, models=models, push_ticks=3, **kw)
        (((states[:, :, 0:3] - target) ** 2).sum() + (states[-1] ** 2).sum()).backward()
        torch.cuda.synchronize()
        return ro, states.detach(), state0.grad, push.grad, models.grad
    _, st_a, gs_a, gp_a, gm_a = grads(cm.rollout_differentiable, device_walk=True)
    ro, st_b, gs_b, gp_b, gm_b = grads(lambda ro, T, s, **kw: cm.rollout_differentiable_checkpointed(ro, T, s, 4, **kw))
    _same_bits(st_b, st_a, "states")
    _same_bits(gs_b, gs_a, "state0.grad")
    _same_bits(gp_b, gp_a, "push.grad")
    _same_bits(gm_b, gm_a, "models.grad")
    assert float(gs_a.abs().max()) > 0 and float(gp_a.abs().max()) > 0 and float(gm_a.abs().max()) > 0
    assert sorted(ro.last_walk["checkpoints"]) == [4] and "tape" not in ro.last_walk and ro.last_backward["tape_rows_peak"] == 4


# ---- 6. no host read ----
def test_nothing_is_read_back():
    """walk_device_checkpointed, walk_resume_device and -- its workspaces made by a first call -- backward_device_checkpointed under torch's sync debug
    mode: a host read or a synchronisation inside raises"""
    import torch
    cfg, B = _cfg(), 8
    com0, dcom0, h0, push = _start(B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    kw = dict(push=push, push_ticks=2, replan={3: (t, ro.plan[1], ro.plan[2])}, skip_ended=True)
    gS = torch.ones((7, B, 9), dtype=torch.float64, device=ro.dev)
    gX = torch.zeros((6, B, ro.L.nx), dtype=torch.float32, device=ro.dev)
    index = torch.arange(B, dtype=torch.int32, device=ro.dev).flip(0)
    ro.backward_device_checkpointed(ro.walk_device_checkpointed(6, com0, dcom0, h0, 2, **kw), gS, gX)      # (the workspaces)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device_checkpointed(6, com0, dcom0, h0, 2, **kw)
        r = ro.walk_resume_device(w["checkpoints"][4], 2, index=index, replan=kw["replan"], skip_ended=True, taped=True)
        g = ro.backward_device_checkpointed(w, gS, gX)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert (w["end_tick"].cpu().numpy() == -1).all() and (g["status"].cpu().numpy() == 0).all() and (r["index_ok"].cpu().numpy() == 1).all()
    assert np.isfinite(g["state0"].cpu().numpy()).all() and float(g["state0"].abs().max()) > 0
    _same_bits(r["final_state"], w["final_state"].flip(0), "the resumed walk, problems reversed")
    assert r["tape"]["rows"] == 3 and float(r["tape"]["lam_g"][1:].abs().max()) > 0
