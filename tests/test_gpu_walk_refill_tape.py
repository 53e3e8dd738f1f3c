"""GPU: the refill walk taped, its tape regrouped by trial, and every trial's gradient (include/cmpc.h, cmpc_rollout_walk_refill_taped_device and
cmpc_walk_tape_regroup; WalkingRollout.walk_device_refill_taped, refill_trial_walk, backward_device_refill).  Who sits where comes from the assignment model
(tests/walk_refill_ref.py).  Every trial is held, to the bit, to a taped walk of its own -- WalkingRollout._walk_live's calls (cmpc_rollout_walk_mismatch_device
with a tape, cold_first = 1, tick_first = 0, the ended problems out of the launches) with the trial's wrench rows passed through, on a roll-out of the same batch
size, factor storage and options that holds it in the slot the model gives it with set_models_device's row `slot` the trial's model -- and every trial's
gradient to backward_device on that walk.  Every check is equality of bits or of integers.
Of the merged lists' times only the entries in use are compared: include/cmpc.h leaves a refilled slot's entries past a foot's count "whatever the set held
before", and no reverse or forward kernel reads them."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_refill_ref as rf
from tests.test_gpu_walk_refill_long import _pack, _scenario
from tests.test_gpu_walk_refill_trials import _cuda, _no_clock, _same_bits, _trial_mismatch, _trial_models

pytestmark = pytest.mark.gpu

DT = 0.06
B, Q, TT = 4, 10, 8
ENDS = {1: 0, 6: 3}      # a NaN wrench row ends trial 1 at its local tick 0 and trial 6 mid-way
TAPE = ("X", "P", "lam_g", "info", "ok", "land", "plan_t", "plan_n", "list_n")
PER_TICK = ("wrench", "status", "hidden_wrench", "state_noise")      # keys of a reverse walk whose batch axis is the second
GRAD = ("state0", "list0", "wrench", "push", "models", "plan", "status", "end_tick", "hidden_wrench", "state_noise", "force_gain")
_cache = {}


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items() if hasattr(v, "cpu")}


def _own_taped_walk(ro, trials, ticks, scenario, mm):
    """walk_device_taped(ticks, ..., mismatch=<the trials' columns>, skip_ended=True) of a batch that holds trials[b] in slot b, its wrench rows given as
    they are (walk_device_taped itself builds them from a push, and a NaN row is no push): WalkingRollout._walk_live's calls with the rows passed
    through.  -> walk_device_taped's dict: the record, and the tape with what backward_device and forward_sensitivity_device_mismatch read of it"""
    import torch
    com0, dcom0, h0, wrench = scenario
    s, L, dev, dt, n = ro.solver, ro.L, ro.dev, ro.cfg.sampling_time, len(trials)
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    dP, dX0, dX, dInfo = z((n, L.np)), z((n, L.nx)), z((n, L.nx)), z((n, 8))
    state = torch.from_numpy(np.concatenate([com0[trials], dcom0[trials], h0[trials]], 1)).to(dev).contiguous()
    ok, land, zmp = torch.ones((n,), dtype=torch.int32, device=dev), z((n, 2), torch.int32), z((n, 2))
    rec = s.walk_record(ticks)
    s.outcome_init_device(state, rec)
    s.set_multiplier_output(True)
    tp = s.walk_tape(ticks, ro.M, step=dt / ro.substeps, substeps=ro.substeps, force_sample_time=ro.force_sample_time, device=dev)
    sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
    wt = torch.from_numpy(np.ascontiguousarray(wrench[:ticks, trials])).to(dev)
    held = s.plant_mismatch(hidden_wrench=mm["hidden_wrench"][:, trials], state_noise=mm["state_noise"][:, trials], force_gain=mm["force_gain"][trials],
                            tick_first=0, device=dev)
    refs = ro._planner_refs(ticks)
    s.set_ended_device(rec["end_tick"])
    try:
        s.rollout_walk_device(0, ticks, True, ro.plan, sets[0], sets[1], 0, ok, land, state, dP, dX0, dX, dInfo, zmp, rec, row0=0, wrench_ticks=wt,
                              step=dt / ro.substeps, substeps=ro.substeps, planner=refs, force_sample_time=ro.force_sample_time, tape=tp, mismatch=held)
        torch.cuda.synchronize()
    finally:
        s.set_ended_device(None)
    del rec["_c"]
    tp.update(dt=dt, push_ticks=0, segments=[0], mismatch=held,
              references=dict(knots=int(refs[0].shape[1]), dt=refs[2], t_first=refs[3], robot_mass=refs[4], com_height=refs[5]))
    rec["tape"] = tp
    return rec


def _seeds(nx, ends, seed):
    """random seeds on every trial's states and solutions, not finite in the rows behind an ending: a trial ended at local tick e contributes its states
    0 .. e and its solutions 0 .. e - 1, and the rest is not to be read"""
    rng = np.random.default_rng(seed)
    gS, gX = rng.normal(size=(TT + 1, Q, 9)), rng.normal(size=(TT, Q, nx)).astype(np.float32)
    for q, e in ends.items():
        gS[e + 1:, q] = np.nan
        gX[e:, q] = np.inf
    return gS, gX


def _study(N, opts, ends, seed, ticks=None):
    """the study of the file: Q = 10 trials of 8 ticks through B = 4 slots, a model and a mismatch per trial, the walk taped; the walks of their own as
    _pack packs them, and both reverse walks.  One per configuration, shared by the tests and left unchanged"""
    import torch
    key = (N, tuple(sorted(opts.items())), tuple(sorted(ends.items())), seed, ticks)
    if key in _cache:
        return _cache[key]
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, seed, ends)
    scenario = (com0, dcom0, h0, wrench)
    models = _trial_models(Q)
    mm = _trial_mismatch(Q, 7, 6, 1, seed=seed + 100)
    T = rf.walk_length(B, Q, TT, end_local) if ticks is None else ticks
    m = rf.assignment_model(B, Q, TT, T, end_local)
    ro = cm.rollout.WalkingRollout(cfg, B, **opts)
    w = ro.walk_device_refill_taped(T, TT, com0, dcom0, h0, models=models, mismatch=mm, wrench_trials=wrench)
    torch.cuda.synchronize()
    t = _host(w["trials"])
    for k in ("slot", "start", "ticks", "end_tick"):
        np.testing.assert_array_equal(t[k], m[k], err_msg=k)
    st = dict(cfg=cfg, ro=ro, w=w, m=m, t=t, scenario=scenario, models=models, mm=mm, end_local=end_local, T=T, opts=opts, ends=ends, seed=seed)
    _cache[key] = st
    return st


def _own_walks(st):
    """the walks of their own of a study in which every trial started, and backward_device on each with the trials' seeds"""
    import torch
    if "own" in st:
        return st["own"], st["where"], st["own_grad"], st["seeds"]
    assert (st["m"]["start"] >= 0).all(), "every trial must have started"
    walks, where, _ = _pack(st["m"], B, Q, st["end_local"])
    gS, gX = _seeds(st["ro"].L.nx, st["ends"], st["seed"] + 200)
    own, own_grad = [], []
    for trials in walks:
        ref_ro = cm.rollout.WalkingRollout(st["cfg"], B, models=_cuda(st["models"][trials]), **st["opts"])
        o = _own_taped_walk(ref_ro, trials, TT, st["scenario"], st["mm"])
        g = ref_ro.backward_device(o, gS[:, trials], gX[:, trials])
        torch.cuda.synchronize()
        own.append((ref_ro, o))
        own_grad.append(_host(g))
    st.update(own=own, where=where, own_grad=own_grad, seeds=(gS, gX), walks=walks)
    return own, where, own_grad, (gS, gX)


def _view_equals_own_walk(view, j, own, b, rows, msg):
    """rows r < `rows` of every tape array and states 0 .. rows of column j of a regrouped view against column b of a walk of its own"""
    vt, ot = _host(view["tape"]), _host(own["tape"])
    for k in TAPE:
        _same_bits(_no_clock(k, vt[k][:rows, j]), _no_clock(k, ot[k][:rows, b]), f"{msg} tape {k}")
    _same_bits(vt["states"][:rows + 1, j], ot["states"][:rows + 1, b], f"{msg} tape states")
    for r in range(rows):
        for c in range(2):
            n = int(ot["list_n"][r, b, c])
            _same_bits(vt["list_t"][r, j, c, :n], ot["list_t"][r, b, c, :n], f"{msg} tape list_t row {r} foot {c}")


def _grad_equals_own(got, q, want, b, msg, rows=TT):
    for k in GRAD:
        if k in PER_TICK:
            _same_bits(got[k][:rows, q], want[k][:rows, b], f"{msg} {k}")
        else:
            _same_bits(got[k][q], want[k][b], f"{msg} {k}")


def _tape_and_gradient(st, sample):
    """tests 2 and 3 on the trials of `sample`"""
    import torch
    own, where, own_grad, (gS, gX) = _own_walks(st)
    ro, w, t = st["ro"], st["w"], st["t"]
    for q0 in range(0, Q, B):
        group = list(range(q0, min(q0 + B, Q)))
        if not set(group) & set(sample):
            continue
        view = ro.refill_trial_walk(w, group)
        torch.cuda.synchronize()
        assert view["ok"].cpu().tolist() == [1] * len(group) + [0] * (B - len(group))
        assert view["end_tick"].cpu().tolist() == [int(st["end_local"][q]) for q in group] + [0] * (B - len(group))
        assert view["tape"]["rows"] == TT and view["tape"]["segments"] == [0] and view["tape"]["_c"].first_row_is_first_tick == 1
        for j, q in enumerate(group):
            if q in sample:
                wj, b = where[q]
                _view_equals_own_walk(view, j, own[wj][1], b, int(t["ticks"][q]), f"trial {q} (walk {wj}, slot {b})")
    got = st.get("grad")
    if got is None:
        got = st["grad"] = _host(ro.backward_device_refill(w, gS, gX))
        torch.cuda.synchronize()
    assert set(got) == set(GRAD)
    assert got["state0"].shape == (Q, 9) and got["wrench"].shape == (TT, Q, st["cfg"].N, 6) and got["status"].shape == (TT, Q)
    assert got["hidden_wrench"].shape == (TT, Q, 6) and got["state_noise"].shape == (TT, Q, 9) and got["force_gain"].shape == (Q,)
    assert got["models"].shape == (Q, 34) and got["list0"].shape == got["plan"].shape == (Q, 2, ro.M, 3) and got["push"].shape == (Q, 3)
    for q in sample:
        wj, b = where[q]
        _grad_equals_own(got, q, own_grad[wj], b, f"trial {q} (walk {wj}, slot {b})")
    for k in GRAD:      # pad columns and the seeds behind an ending leave no trace: finite, as the walks of their own are
        if got[k].dtype.kind == "f":
            assert np.isfinite(got[k][:, sample] if k in PER_TICK else got[k][sample]).all(), k
    through = [q for q in sample if st["end_local"][q] < 0]
    assert any((got["hidden_wrench"][:, q] != 0).any() and (got["models"][q] != 0).any() and (got["state0"][q] != 0).any() for q in through), \
        "no trial that walked through has a gradient: an all-zero pass is not a pass"
    return got


def test_taping_changes_nothing():
    """every key walk_device_refill_trials returns, to the bit (info without its clock word); and the multiplier output must be on"""
    import torch
    st = _study(10, {}, ENDS, 61)
    w = st["w"]
    ro = cm.rollout.WalkingRollout(st["cfg"], B)
    want = ro.walk_device_refill_trials(st["T"], TT, *st["scenario"][:3], models=st["models"], mismatch=st["mm"], wrench_trials=st["scenario"][3])
    torch.cuda.synchronize()
    assert set(w) == set(want) | {"tape"} and set(w["trials"]) == set(want["trials"])
    for k, v in want.items():
        if hasattr(v, "cpu"):
            _same_bits(_no_clock(k, w[k].cpu().numpy()), _no_clock(k, v.cpu().numpy()), k)
    for k, v in want["trials"].items():
        if hasattr(v, "cpu"):
            _same_bits(w["trials"][k].cpu().numpy(), v.cpu().numpy(), "trials " + k)
    for x, y in zip(w["lists"], want["lists"]):
        _same_bits(x.cpu().numpy(), y.cpu().numpy(), "lists")
    tape = w["tape"]
    assert tape["rows"] == st["T"] and tape["X"].shape[:2] == (st["T"], B) and tape["states"].shape == (st["T"] + 1, B, 9)
    assert tape["models"] is not None and tape["mismatch"]["hidden_wrench"] is not None and tape["state0"].shape == (Q, 9)
    for q, e in ENDS.items():
        assert st["t"]["end_tick"][q] == e
    # the multiplier output off: refused before anything is queued
    ro.solver.set_multiplier_output(False)
    ro.solver.set_multiplier_output = lambda *a, **k: None
    with pytest.raises(RuntimeError, match="multiplier output is off"):
        ro.walk_device_refill_taped(st["T"], TT, *st["scenario"][:3], wrench_trials=st["scenario"][3])


def test_the_regrouped_tape_is_the_trials_own_tape_and_its_gradient_its_own_walks():
    """tests 2 and 3 of the study at N = 10: every trial's rows r < ticks[q] of every tape array, lam_g included, and its states 0 .. ticks[q]; then
    backward_device_refill key by key and trial by trial, status and the three mismatch gradients included"""
    st = _study(10, {}, ENDS, 61)
    assert (st["m"]["start"] >= 0).all() and st["m"]["end_tick"][1] == 0 and st["m"]["end_tick"][6] == 3
    got = _tape_and_gradient(st, list(range(Q)))
    assert got["end_tick"].tolist() == [int(e) for e in st["end_local"]]
    for q, e in ENDS.items():      # behind an ending: zero rows, status 6
        assert (got["wrench"][e:, q] == 0).all() and (got["status"][e:, q] == 6).all() and (got["hidden_wrench"][e:, q] == 0).all()


def test_a_walk_too_short_for_its_queue():
    """12 ticks: trial 8 is cut off after 3 ticks by the walk's end and trial 9 never starts.  The cut-off trial's gradient is backward_device's on a walk
    of its own of ticks[q] ticks with the seeds truncated to those rows; the trial never started returns its seed on state 0 and zeros"""
    import torch
    st = _study(10, {}, ENDS, 61, ticks=12)
    m, ro, w = st["m"], st["ro"], st["w"]
    q, never = 8, 9
    n = int(m["ticks"][q])
    assert m["end_tick"][q] < 0 and 0 < n < TT and m["start"][q] + n == 12 and m["start"][never] < 0 and m["ticks"][never] == 0
    gS, gX = _seeds(ro.L.nx, ENDS, 262)
    got = _host(ro.backward_device_refill(w, gS, gX))
    torch.cuda.synchronize()
    assert got["end_tick"].tolist() == [-1, 0, -1, -1, -1, 4, 3, 4, 3, 0]      # (trials 5 and 7 are cut off too, after 4 ticks; trial 6 ended at 3)
    b = int(m["slot"][q])
    trials = [q] * B
    ref_ro = cm.rollout.WalkingRollout(st["cfg"], B, models=_cuda(st["models"][trials]))
    own = _own_taped_walk(ref_ro, trials, n, st["scenario"], st["mm"])
    assert own["end_tick"].cpu().tolist() == [-1] * B
    view = ro.refill_trial_walk(w, [q, never])
    torch.cuda.synchronize()
    assert view["end_tick"].cpu().tolist() == [n, 0, 0, 0] and view["ok"].cpu().tolist() == [1, 1, 0, 0]
    _view_equals_own_walk(view, 0, own, b, n, f"trial {q}")
    _same_bits(view["tape"]["states"][0, 1].cpu().numpy(), np.concatenate([a[never] for a in st["scenario"][:3]]))
    want = _host(ref_ro.backward_device(own, gS[:n + 1, trials], gX[:n, trials]))
    torch.cuda.synchronize()
    for k in GRAD:
        if k == "end_tick":
            continue
        if k in PER_TICK:
            _same_bits(got[k][:n, q], want[k][:, b], f"trial {q} {k}")
            assert (got[k][n:, q] == (6 if k == "status" else 0)).all(), k
        else:
            _same_bits(got[k][q], want[k][b], f"trial {q} {k}")
    assert (got["state0"][q] != 0).any() and (got["hidden_wrench"][:n, q] != 0).any()
    _same_bits(got["state0"][never], gS[0, never])
    for k in GRAD:
        if k not in ("state0", "end_tick", "status"):
            assert (got[k][:, never] == 0).all() if k in PER_TICK else (got[k][never] == 0).all(), k


def test_the_kernel_is_the_host_form():
    """cmpc_rollout_tape_regroup_device against cmpc_rollout_tape_regroup on the tape of the 12-tick walk, every word of every destination array over a
    sentinel: trials ended at local tick 0 and mid-way, cut off, never started, walked through, a repeated index, indices -1 and Q, and a tick_first that
    puts the trials of tick 0 in front of the tape"""
    import ctypes as C
    import torch
    from tests import walk_refill_tape_ref as rt
    st = _study(10, {}, ENDS, 61, ticks=12)
    ro, w, m = st["ro"], st["w"], st["m"]
    s, tape, N = ro.solver, w["tape"], st["cfg"].N
    fill = tape["refill"]
    names = dict(dX="X", dP="P", dLamG="lam_g", dInfo="info", dStates="states", dOk="ok", dLand="land", dPlanT="plan_t", dListT="list_t", dPlanN="plan_n",
                 dListN="list_n")
    src = {k: np.ascontiguousarray(tape[v].cpu().numpy()) for k, v in names.items()}
    q_arrays = [np.ascontiguousarray(fill[k].cpu().numpy()) for k in ("state0", "slot", "start", "ticks", "end_tick")]
    f = rt.refill_struct(TT, *q_arrays)
    kinds = set()
    for tf, idx in ((0, (1, 6, 8, 9)), (0, (0, 0, -1, Q)), (1, (2, 4, 5, 7))):
        kinds |= {(tf, rt.kind(q, Q, B, 12, TT, tf, m["slot"], m["start"], m["ticks"])) for q in idx}
        host = rt.arrays(N, ro.M, TT, B)
        index, end_h, ok_h = np.array(idx, np.int32), np.full(B, -7, np.int32), np.full(B, -7, np.int32)
        sc, dc, g = rt.struct(src, 12, step=tape["step"], substeps=tape["substeps"]), rt.struct(host, TT), rt.regroup_struct(tf, index, end_h, ok_h)
        assert s._lib.cmpc_rollout_tape_regroup(N, B, ro.M, C.byref(sc), C.byref(f), C.byref(g), C.byref(dc)) == 0
        dst = s.walk_tape(TT, ro.M, step=tape["step"], substeps=tape["substeps"], device=ro.dev)
        for v in names.values():
            dst[v].view(torch.uint8).fill_(rt.SENTINEL)
        _, end_d, ok_d = s.tape_regroup_device(tape, fill, torch.from_numpy(index).to(ro.dev), dst, tick_first=tf)
        torch.cuda.synchronize()
        assert end_d.cpu().tolist() == end_h.tolist() and ok_d.cpu().tolist() == ok_h.tolist(), (tf, idx)
        for k, v in names.items():
            _same_bits(dst[v].cpu().numpy(), host[k], f"tick_first {tf} trials {idx} {k}")
        if tf == 0 and idx[0] == 1:
            assert end_h.tolist() == [0, 3, 3, 0] and ok_h.tolist() == [1, 1, 1, 1]
        if tf == 1:
            assert end_h.tolist() == [0, -1, 4, 4] and ok_h.tolist() == [0, 1, 1, 1]      # (trial 2 started at tick 0: in front of the tape)
    assert kinds == {(0, "started"), (0, "never"), (0, "none"), (1, "none"), (1, "started")}


def test_the_hbm_factor_solver():
    """N = 13, factors="hbm", slots turning over inside the walk: tests 2 and 3 on a sample of trials -- one ended mid-way, its follower in the slot, two
    walked through, one of the last group"""
    ends = {0: 3, 5: 1}
    st = _study(13, dict(factors="hbm"), ends, 65)
    m = st["m"]
    starts = sorted({int(v) for v in m["start"] if v > 0 and v % TT})
    assert len(starts) >= 2, starts
    follower = next(q for q in range(Q) if m["slot"][q] == m["slot"][0] and m["start"][q] == 4)
    sample = sorted({0, 5, follower, 2, 9})
    assert st["ro"].solver.factor_storage == "hbm"
    _tape_and_gradient(st, sample)


def test_forward_mode_on_a_view():
    """forward_sensitivity_device_mismatch(view, dir_state0, dir_hidden_wrench), k = 2, against the walk of its own's for two trials, one of them ended"""
    import torch
    st = _study(10, {}, ENDS, 61)
    own, where, _, _ = _own_walks(st)
    ro, w = st["ro"], st["w"]
    rng = np.random.default_rng(66)
    d0, dh = rng.normal(size=(Q, 2, 9)), rng.normal(size=(TT, Q, 2, 6))
    group = [6, 3]
    pad = lambda a, axis: np.concatenate([a, np.zeros_like(a)], axis)
    view = ro.refill_trial_walk(w, group)
    ro.solver.set_models_device(_cuda(st["models"][group + group]))
    try:
        got = _host(ro.forward_sensitivity_device_mismatch(view, dir_state0=pad(d0[group], 0), dir_hidden_wrench=pad(dh[:, group], 1)))
        torch.cuda.synchronize()
    finally:
        ro.solver.set_models(None)
    assert got["end_tick"].tolist() == [3, -1, 0, 0]
    for j, q in enumerate(group):
        wj, b = where[q]
        ref_ro, o = own[wj]
        cols = st["walks"][wj]
        assert cols[b] == q
        want = _host(ref_ro.forward_sensitivity_device_mismatch(o, dir_state0=d0[cols], dir_hidden_wrench=dh[:, cols]))
        torch.cuda.synchronize()
        _same_bits(got["states"][:, j], want["states"][:, b], f"trial {q} states")
        _same_bits(got["status"][:, j], want["status"][:, b], f"trial {q} status")
        _same_bits(got["removed"][:, j], want["removed"][:, b], f"trial {q} removed")
        _same_bits(got["list"][j], want["list"][b], f"trial {q} list")
    assert (got["states"][1:, 1] != 0).any() and np.isfinite(got["states"][:, :2]).all()


def test_group_boundaries():
    """Q = 10 through B = 4: groups of 4, 4 and 2.  The padded group's results equal the same trials regrouped alone in another order, and the pad columns
    leave no trace"""
    import torch
    st = _study(10, {}, ENDS, 61)
    _, _, _, (gS, gX) = _own_walks(st)
    ro, w = st["ro"], st["w"]
    got = st.get("grad")
    if got is None:
        got = st["grad"] = _host(ro.backward_device_refill(w, gS, gX))
    for k in GRAD:
        assert got[k].shape[1 if k in PER_TICK else 0] == Q, k
    order = [9, 8, 9]
    view = ro.refill_trial_walk(w, order)
    cols = order + [0]
    ro.solver.set_models_device(_cuda(st["models"][cols]))
    try:
        gs, gx = gS[:, cols].copy(), gX[:, cols].copy()
        gs[:, 3], gx[:, 3] = np.nan, np.nan      # (a pad column's seeds are not read)
        alone = _host(ro.backward_device(view, gs, gx))
        torch.cuda.synchronize()
    finally:
        ro.solver.set_models(None)
    assert alone["end_tick"].tolist() == [-1, -1, -1, 0]
    for j, q in enumerate(order):
        _grad_equals_own(got, q, alone, j, f"trial {q} alone in column {j}")
    assert (got["hidden_wrench"][:, 9] != 0).any() and (got["models"][8] != 0).any()
