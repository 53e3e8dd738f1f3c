"""GPU: per-trial models and a per-trial plant mismatch on the refill walk (include/cmpc.h, cmpc_walk_refill_trials;
WalkingRollout.walk_device_refill_trials).  Who sits where comes from the assignment model (tests/walk_refill_ref.py) and is asserted on the CPU before
the walk; every trial is then held, to the bit, to a walk of its own -- cmpc_rollout_walk_device, or cmpc_rollout_walk_mismatch_device with tick_first = 0
-- on a roll-out of the same batch size, factor storage and options that holds it in the slot the model gives it, with set_models_device's row `slot` the
trial's model and the schedules' column `slot` the trial's rows.  Every check is equality of bits or of integers.
Trials of 18 ticks at N = 10 see the left foot lift (tick 6), its landing enter the horizon (tick 4), the touchdown with the step adjustment (tick 14) and
the right foot's lift (tick 16), as tests/test_gpu_walk_refill_long.py notes."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_record_ref as wr
from tests import walk_refill_ref as rf
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_refill_long import _pack, _plain_walk, _scenario, _slot_models

pytestmark = pytest.mark.gpu

OUTCOME = ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")
DT = 0.06


def _same_bits(x, y, msg=""):
    np.testing.assert_array_equal(rf.bits(x), rf.bits(y), err_msg=msg)


def _no_clock(k, a):
    """info's column 6 is the solve's clock count (tests/test_bench_dump_cpu.py leaves it out as well): not a result"""
    return np.delete(a, 6, axis=-1) if k == "info" else a


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _trial_models(Q):
    """Q distinct model rows: friction 0.3 .. 1.65 and foot scale 0.85 .. 1.75, tests/test_gpu_walk_refill_long._slot_models' rows for Q <= 10, the same
    range in finer steps above"""
    if Q <= 10:
        return _slot_models(Q)
    rows = np.repeat(_slot_models(1), Q, 0)
    base = rows[0].copy()
    for q in range(Q):
        rows[q, 0] = 0.3 + 1.35 * q / (Q - 1)
        rows[q, 10:] = base[10:] / 0.85 * (0.85 + 0.9 * q / (Q - 1))
    return rows


def _trial_mismatch(Q, hidden_rows, noise_rows, first, seed, nan_at=None):
    """the three parts per trial: hidden pushes (about 0.3 m/s^2 and 0.05 N m / kg, tests/test_gpu_mismatch.py's magnitudes) on local ticks first ..
    hidden_rows - 1, a centimetre-scale noise on first .. noise_rows - 1 (the rows in front are zeros: inside the range, added), gains in [0.8, 1.2];
    nan_at (q, r): trial q's hidden row r is NaN"""
    rng = np.random.default_rng(seed)
    hidden = np.zeros((hidden_rows, Q, 6), np.float32)
    hidden[first:] = np.concatenate([rng.normal(0, 0.3, (hidden_rows - first, Q, 3)), rng.normal(0, 0.05, (hidden_rows - first, Q, 3))], -1)
    noise = np.zeros((noise_rows, Q, 9), np.float32)
    noise[first:] = np.concatenate([rng.normal(0, 3e-3, (noise_rows - first, Q, 3)), rng.normal(0, 1e-2, (noise_rows - first, Q, 3)),
                                    rng.normal(0, 2e-3, (noise_rows - first, Q, 3))], -1)
    gain = rng.uniform(0.8, 1.2, Q).astype(np.float32)
    if nan_at is not None:
        hidden[nan_at[1], nan_at[0]] = np.nan
    return dict(hidden_wrench=hidden, state_noise=noise, force_gain=gain)


def _mismatch_walk(ro, trials, trial_ticks, com0, dcom0, h0, wrench, mm):
    """tests/test_gpu_walk_refill_long._plain_walk under the trials' columns of the per-trial mismatch, tick_first = 0: walk_device_mismatch's call
    (cmpc_rollout_walk_mismatch_device, cold_first = 1) with the wrench rows passed through and the ended problems out of the launches"""
    import torch
    B = len(trials)
    s, L, dev, dt = ro.solver, ro.L, ro.dev, ro.cfg.sampling_time
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    dP, dX0, dX, dInfo = z((B, L.np)), z((B, L.nx)), z((B, L.nx)), z((B, 8))
    state = torch.from_numpy(np.concatenate([com0[trials], dcom0[trials], h0[trials]], 1)).to(dev).contiguous()
    ok, land, zmp = torch.ones((B,), dtype=torch.int32, device=dev), z((B, 2), torch.int32), z((B, 2))
    rec = s.walk_record(trial_ticks)
    s.outcome_init_device(state, rec)
    sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
    wt = torch.from_numpy(np.ascontiguousarray(wrench[:, trials])).to(dev)
    held = s.plant_mismatch(hidden_wrench=mm["hidden_wrench"][:, trials], state_noise=mm["state_noise"][:, trials], force_gain=mm["force_gain"][trials],
                            tick_first=0, device=dev)
    s.set_ended_device(rec["end_tick"])
    try:
        cur = s.rollout_walk_device(0, trial_ticks, True, ro.plan, sets[0], sets[1], 0, ok, land, state, dP, dX0, dX, dInfo, zmp, rec, row0=0, wrench_ticks=wt,
                                    step=dt / ro.substeps, substeps=ro.substeps, planner=ro._planner_refs(trial_ticks),
                                    force_sample_time=ro.force_sample_time, mismatch=held)
        torch.cuda.synchronize()
    finally:
        s.set_ended_device(None)
    assert cur == (trial_ticks - 1) % 2
    out = {k: v.cpu().numpy() for k, v in rec.items() if hasattr(v, "cpu")}
    out.update(X=dX.cpu().numpy(), P=dP.cpu().numpy(), state=state.cpu().numpy(), sets=[tuple(a.cpu().numpy() for a in st) for st in sets],
               plan=tuple(a.cpu().numpy() for a in ro.plan))
    return out


def _table(B, Q, TT, end_local):
    """the assignment on the CPU: the fewest ticks at which every trial has started and finished, asserted -> (T, the model's table)"""
    T = rf.walk_length(B, Q, TT, end_local)
    m = rf.assignment_model(B, Q, TT, T, end_local)
    length = np.where(end_local >= 0, end_local + 1, TT)
    assert (m["start"] >= 0).all() and (m["ticks"] == length).all() and (m["start"] + m["ticks"]).max() == T
    short = rf.assignment_model(B, Q, TT, T - 1, end_local)
    assert (short["start"] < 0).any() or (short["ticks"] != length).any(), "one tick fewer would do"
    assert (m["end_tick"] == end_local).all()
    return T, m


def _walk_and_check(N, B, Q, TT, opts, scenario, end_local, models=None, mm=None, sample=None):
    """the refill walk with per-trial data against walks that hold every trial in its slot -> (the walk on the host, its per-trial dict, the model's table,
    the reference walks, where[q] = (walk, slot), the slots' trials)"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0, wrench = scenario
    T, m = _table(B, Q, TT, end_local)
    ro = cm.rollout.WalkingRollout(cfg, B, **opts)
    w = ro.walk_device_refill_trials(T, TT, com0, dcom0, h0, models=models, mismatch=mm, wrench_trials=wrench)
    torch.cuda.synchronize()
    t = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
    g = {k: v.cpu().numpy() for k, v in w.items() if hasattr(v, "cpu")}
    lists = tuple(a.cpu().numpy() for a in w["lists"])
    np.testing.assert_array_equal(g["trial_of"], m["trial_of"])
    for k in ("slot", "start", "ticks", "end_tick"):
        np.testing.assert_array_equal(t[k], m[k], err_msg=k)

    walks, where, by_slot = _pack(m, B, Q, end_local)
    refs = []
    for trials in walks:
        ref_ro = cm.rollout.WalkingRollout(cfg, B, models=None if models is None else _cuda(models[trials]), **opts)
        refs.append(_plain_walk(ref_ro, trials, TT, com0, dcom0, h0, wrench) if mm is None else
                    _mismatch_walk(ref_ro, trials, TT, com0, dcom0, h0, wrench, mm))
    # every trial (or the sample): outcome and trace rows
    for q in range(Q) if sample is None else sample:
        j, b = where[q]
        ref, rows, s0 = refs[j], int(m["ticks"][q]), int(m["start"][q])
        for k in OUTCOME:
            _same_bits(t[k][q], ref[k][b], f"trial {q} {k}")
        for k in wr.TRACE:
            _same_bits(g[k][s0:s0 + rows, b], ref[k][:rows, b], f"trial {q} (slot {b}, start {s0}) {k}")
    # the last trial of each slot: X, P, state and the in-use entries of the lists the walk returns (tests/test_gpu_walk_refill_long.py: tick t writes set
    # t % 2; a stopped slot's rows of the returned set are its last local tick's if that tick and T - 1 have the same parity, else the tick before's)
    compared = 0
    for b in range(B) if sample is None else sorted({where[q][1] for q in sample}):
        q = int(by_slot[b][-1])
        j, _ = where[q]
        ref, e = refs[j], int(m["ticks"][q]) - 1
        last = int(m["start"][q]) + e
        for k in ("X", "P", "state"):
            _same_bits(g[k][b], ref[k][b], f"slot {b} (last trial {q}) {k}")
        e_lists = e if last % 2 == (T - 1) % 2 else e - 1
        if e_lists < 0:
            continue
        rt, rpose, rn = ref["sets"][e_lists % 2]
        np.testing.assert_array_equal(lists[2][b], rn[b], err_msg=f"slot {b} list counts")
        for c in range(2):
            n = int(rn[b, c])
            _same_bits(lists[0][b, c, :n], rt[b, c, :n], f"slot {b} foot {c} list times")
            _same_bits(lists[1][b, c, :n], rpose[b, c, :n], f"slot {b} foot {c} list poses")
        compared += 1
    assert compared >= 1
    return g, t, m, refs, where, by_slot


def _queue(N, Q, TT, seed, ends):
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, seed, ends)
    return (com0, dcom0, h0, wrench), end_local


def test_per_trial_models():
    """B = 4, Q = 10, 18-tick trials, ten distinct models, two trials ended early by a NaN wrench row"""
    import torch
    N, B, Q, TT = 10, 4, 10, 18
    scenario, end_local = _queue(N, Q, TT, 51, {1: 2, 6: 9})
    models = _trial_models(Q)
    assert len({r.tobytes() for r in models}) == Q
    g, t, m, refs, where, _ = _walk_and_check(N, B, Q, TT, {}, scenario, end_local, models=models)
    assert t["model_ok"].tolist() == [1] * Q
    for q, e in ((1, 2), (6, 9)):
        assert t["end_tick"][q] == e and t["end_code"][q] == 3
    through = [q for q in range(Q) if end_local[q] < 0]
    for q in through:      # the reference walks walked, and through the contact changes
        j, b = where[q]
        assert refs[j]["end_tick"][b] == -1 and (refs[j]["iterations"][:, b] > 0).all(), q
        assert ((refs[j]["land"][:, b] >= 0).any(1) & (refs[j]["landing_offset"][:, b] != 0).any((1, 2))).any(), q
    # the model reached the solve: the same queue walked with the configuration's model ends somewhere else
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    T = g["trial_of"].shape[0]
    plain = cm.rollout.WalkingRollout(cfg, B).walk_device_refill(T, TT, *scenario[:3], wrench_trials=scenario[3])
    torch.cuda.synchronize()
    final = plain["trials"]["final_state"].cpu().numpy()
    differ = [q for q in through if not np.array_equal(rf.bits(final[q]), rf.bits(t["final_state"][q]))]
    assert differ, "no trial's final state moved with its model"


def test_a_bad_model_row_ends_its_trial_at_its_first_tick():
    """trial 2's friction is 0: model_ok 0, the trial ends at local tick 0 with the solver's code for a model outside the rule (status 3: code 4), and the
    trial that follows it in slot 2 is its walk to the bit"""
    N, B, Q, TT = 10, 4, 8, 8
    scenario, end_local = _queue(N, Q, TT, 52, {})
    end_local[2] = 0
    models = _trial_models(Q)
    models[2, 0] = 0.0
    g, t, m, refs, where, by_slot = _walk_and_check(N, B, Q, TT, {}, scenario, end_local, models=models)
    assert t["model_ok"].tolist() == [1, 1, 0, 1, 1, 1, 1, 1]
    assert t["end_tick"][2] == 0 and t["end_code"][2] == 4 and t["ticks"][2] == 1 and t["iterations_sum"][2] == 0
    _same_bits(t["final_state"][2], np.concatenate([a[2] for a in scenario[:3]]))
    follower = int(by_slot[2][1])
    assert follower == 4 and m["start"][follower] == 1 and where[follower][1] == 2
    j, b = where[follower]
    assert t["end_tick"][follower] == -1 and refs[j]["end_tick"][b] == -1 and (refs[j]["iterations"][:, b] > 0).all()


def test_per_trial_mismatch():
    """hidden pushes on local ticks 5 .. 16 (17 rows), noise on 5 .. 14 (15 rows: both range selects are taken, at different ticks), gains in [0.8, 1.2],
    trial 3 ended by a NaN hidden row at local tick 8; the trial that takes its slot walks its walk, so nothing non-finite stays behind"""
    N, B, Q, TT = 10, 4, 10, 18
    scenario, end_local = _queue(N, Q, TT, 53, {})
    end_local[3] = 8
    mm = _trial_mismatch(Q, 17, 15, 5, seed=54, nan_at=(3, 8))
    g, t, m, refs, where, by_slot = _walk_and_check(N, B, Q, TT, {}, scenario, end_local, mm=mm)
    assert t["end_tick"][3] == 8 and t["end_code"][3] == 5 and (t["model_ok"] == -1).all()
    follower = int(by_slot[m["slot"][3]][1])
    j, b = where[follower]
    assert m["start"][follower] == 9 and t["end_tick"][follower] == -1 and np.isfinite(refs[j]["com"][:, b]).all() and np.isfinite(g["state"]).all()
    through = [q for q in range(Q) if end_local[q] < 0]
    for q in through:
        j, b = where[q]
        assert refs[j]["end_tick"][b] == -1 and (refs[j]["iterations"][:, b] > 0).all(), q


def test_models_and_mismatch_on_the_hbm_factor_solver():
    """N = 13 with factors="hbm", 8-tick trials: fresh and warm workgroups share one launch and read different records; hidden rows on local ticks 1 .. 5,
    noise on 1 .. 4, two trials ended by a NaN wrench row so that slots turn over inside the walk"""
    N, B, Q, TT = 13, 4, 10, 8
    scenario, end_local = _queue(N, Q, TT, 55, {0: 3, 5: 1})
    models = _trial_models(Q)
    mm = _trial_mismatch(Q, 6, 5, 1, seed=56)
    g, t, m, _, _, _ = _walk_and_check(N, B, Q, TT, dict(factors="hbm"), scenario, end_local, models=models, mm=mm)
    assert t["model_ok"].tolist() == [1] * Q
    starts = sorted({int(v) for v in m["start"] if v > 0 and v % TT})
    assert len(starts) >= 2, starts      # (ticks on which a fresh workgroup sits among warm ones)


def test_a_batch_above_the_cu_count_with_a_model_per_trial():
    """B = 264, Q = 300, 8-tick trials: the assignment kernel's second chunk hands trials out inside the walk, each with its own model"""
    N, B, Q, TT = 10, 264, 300, 8
    ends = {3: 2, 100: 4, 255: 1, 256: 1, 260: 3, 263: 0, 264: 2, 265: 1}
    scenario, end_local = _queue(N, Q, TT, 57, ends)
    models = _trial_models(Q)
    T, m = _table(B, Q, TT, end_local)
    late = [q for q in range(B, Q) if 0 < m["start"][q] < TT]
    assert any(m["slot"][q] < 256 for q in late) and sum(m["slot"][q] >= 256 for q in late) >= 3, "no refill in the second chunk inside the walk"
    sample = sorted(set(ends) | set(late) | {0, 1, 128, 254, 258, 262, 270, 299} | {q for q in range(B, Q) if m["slot"][q] in (0, 1, 29)})
    assert any(m["slot"][q] < 256 for q in sample) and any(m["slot"][q] >= 256 for q in sample)
    g, t, _, _, _, _ = _walk_and_check(N, B, Q, TT, {}, scenario, end_local, models=models, sample=sample)
    assert (t["model_ok"] == 1).all()


def test_nothing_per_trial_is_the_refill_walk():
    """walk_device_refill_trials with no models and no mismatch (None, and a mismatch with nothing in it) against walk_device_refill: every key"""
    import torch
    N, B, Q, TT = 10, 4, 7, 6
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    (com0, dcom0, h0, wrench), end_local = _queue(N, Q, TT, 58, {2: 3})
    T = rf.walk_length(B, Q, TT, end_local)
    want = cm.rollout.WalkingRollout(cfg, B).walk_device_refill(T, TT, com0, dcom0, h0, wrench_trials=wrench)
    for kw in ({}, dict(mismatch={}), dict(mismatch=dict(hidden_wrench=np.zeros((0, Q, 6), np.float32), tick_first=0))):
        got = cm.rollout.WalkingRollout(cfg, B).walk_device_refill_trials(T, TT, com0, dcom0, h0, wrench_trials=wrench, **kw)
        torch.cuda.synchronize()
        assert set(got) == set(want) and set(got["trials"]) == set(want["trials"]) | {"model_ok"}
        for k, v in want.items():
            if hasattr(v, "cpu"):
                _same_bits(_no_clock(k, got[k].cpu().numpy()), _no_clock(k, v.cpu().numpy()), k)
        for k, v in want["trials"].items():
            if hasattr(v, "cpu"):
                _same_bits(got["trials"][k].cpu().numpy(), v.cpu().numpy(), "trials " + k)
        for x, y in zip(got["lists"], want["lists"]):
            _same_bits(x.cpu().numpy(), y.cpu().numpy(), "lists")
        assert (got["trials"]["model_ok"].cpu().numpy() == -1).all()
        assert got["trials"]["end_tick"][2].item() == 3


@pytest.mark.parametrize("slot_models", [False, True])
def test_the_rollouts_own_models_are_back_afterwards(slot_models):
    """a walk_device on the same roll-out before and after a walk with per-trial models: equal bits, with slot models set and without"""
    import torch
    N, B, Q, TT = 10, 4, 6, 5
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    own = _slot_models(B)[::-1].copy() if slot_models else None
    ro = cm.rollout.WalkingRollout(cfg, B, models=own)
    start = [a.astype(np.float32) for a in _start(B, seed=59)[:3]]
    (com0, dcom0, h0, wrench), end_local = _queue(N, Q, TT, 60, {})
    walk = lambda: {k: v.cpu().numpy() for k, v in ro.walk_device(6, *start).items() if hasattr(v, "cpu")}
    before = walk()
    w = ro.walk_device_refill_trials(rf.walk_length(B, Q, TT, end_local), TT, com0, dcom0, h0, models=_trial_models(10)[4:], wrench_trials=wrench)
    torch.cuda.synchronize()
    assert w["trials"]["model_ok"].cpu().numpy().tolist() == [1] * Q
    after = walk()
    assert set(before) == set(after) and (before["end_tick"] == -1).all()
    for k in before:
        _same_bits(_no_clock(k, after[k]), _no_clock(k, before[k]), k)
    # the per-trial models were not the roll-out's: the same queue without them ends somewhere else
    plain = ro.walk_device_refill(rf.walk_length(B, Q, TT, end_local), TT, com0, dcom0, h0, wrench_trials=wrench)
    torch.cuda.synchronize()
    assert not np.array_equal(rf.bits(plain["trials"]["final_state"].cpu().numpy()), rf.bits(w["trials"]["final_state"].cpu().numpy()))
