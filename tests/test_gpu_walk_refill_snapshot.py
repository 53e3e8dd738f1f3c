"""GPU: a refill walk whose trials start from a snapshot of a walk in progress (include/cmpc.h, cmpc_walk_refill_snapshot;
WalkingRollout.walk_device_refill_from_snapshot).  The pilot is walk_device_checkpointed on B = 4 with no push (N = 10, dt = 0.06: the left foot lifts at
tick 6, touches down with its step adjustment at tick 14, the right foot lifts at 16); a checkpoint of it -- of tick 8, 5 or 14 -- is the pool.  Trials end at chosen resumed ticks
through a NaN hidden-wrench row, so who sits where is known from the assignment model (tests/walk_refill_ref.py) and asserted on the CPU before the walk.
Every trial is then held, to the bit, to a walk_resume_device_mismatch of its own (tick_first = the pool's tick, skip_ended=True) on a roll-out of the same
batch size, factor storage and options that holds it in the slot the model gives it, with models row `slot` the trial's model and the schedules' column
`slot` the trial's rows.  Every check is equality of bits or of integers."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_record_ref as wr
from tests import walk_refill_ref as rf
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_refill_long import _pack
from tests.test_gpu_walk_refill_trials import _cuda, _no_clock, _queue, _same_bits, _table, _trial_mismatch, _trial_models

pytestmark = pytest.mark.gpu

OUTCOME = ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")
DT = 0.06
B = 4
_PILOTS = {}


def _host(w):
    return {k: v.cpu().numpy() for k, v in w.items() if hasattr(v, "cpu")}


def _pilot(N, opts=(), nan_at=None):
    """the pilot walk of 15 ticks with a checkpoint in front of every tick 1 .. 14, computed once per case and left unchanged; nan_at (problem, tick): a NaN row
    of state noise ends that problem there"""
    import torch
    key = (N, tuple(opts), nan_at)
    if key not in _PILOTS:
        cfg = cm.config.ergocub_gazebo_v1(N, DT)
        com0, dcom0, h0, _ = (a.astype(np.float32) for a in _start(B, seed=71))
        mm = None
        if nan_at is not None:
            noise = np.zeros((nan_at[1] + 1, B, 9), np.float32)
            noise[nan_at[1], nan_at[0]] = np.nan
            mm = dict(state_noise=noise)
        w = cm.rollout.WalkingRollout(cfg, B, **dict(opts)).walk_device_checkpointed(15, com0, dcom0, h0, 1, skip_ended=True, mismatch=mm)
        torch.cuda.synchronize()
        assert sorted(w["checkpoints"]) == list(range(1, 15))
        _PILOTS[key] = (cfg, w)
    return _PILOTS[key]


def _mismatch(Q, TT, seed, end_local):
    """per-trial hidden pushes on the ticks 1 .. TT - 2 since spawn (TT - 1 rows), noise on 1 .. TT - 3 (TT - 2 rows: both range selects are taken, at
    different ticks), gains in [0.8, 1.2]; a NaN hidden row ends trial q at its resumed tick end_local[q]"""
    mm = _trial_mismatch(Q, TT - 1, TT - 2, 1, seed=seed)
    for q, e in enumerate(end_local):
        if e >= 0:
            assert e < TT - 1
            mm["hidden_wrench"][e, q] = np.nan
    return mm


def _resume(cfg, opts, pool, trials, ticks, snapshot_of, mm, models):
    """walk_resume_device_mismatch of a batch that holds trials[b] in slot b, on the host"""
    import torch
    t_s = int(pool["tick"])
    ro = cm.rollout.WalkingRollout(cfg, B, models=None if models is None else _cuda(models[trials]), **dict(opts))
    held = dict(hidden_wrench=mm["hidden_wrench"][:, trials], state_noise=mm["state_noise"][:, trials], force_gain=mm["force_gain"][trials], tick_first=t_s)
    r = ro.walk_resume_device_mismatch(pool, ticks, held, index=np.ascontiguousarray(snapshot_of[trials], np.int32), skip_ended=True)
    torch.cuda.synchronize()
    out = _host(r)
    out["lists"] = tuple(a.cpu().numpy() for a in r["lists"])
    assert r["tick0"] == t_s
    return out


def _walk_and_check(cfg, opts, pool, Q, TT, snapshot_of, end_local, mm, models=None, at_spawn=()):
    """the refill walk from the pool against resumed walks that hold every trial in its slot.  at_spawn: trials that are ended at their spawn (a bad index,
    a pool row that had ended): the model holds them one tick, the record never sees them, and the caller checks them.  -> (the walk on the host, its
    per-trial dict, the model's table, the reference walks, where[q] = (walk, slot), the slots' trials, T)"""
    import torch
    t_s = int(pool["tick"])
    snapshot_of = np.asarray(snapshot_of, np.int32)
    T, m = _table(B, Q, TT, end_local)
    ro = cm.rollout.WalkingRollout(cfg, B, **dict(opts))
    w = ro.walk_device_refill_from_snapshot(pool, T, TT, snapshot_of, models=models, mismatch=mm)
    torch.cuda.synchronize()
    t = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
    g = _host(w)
    lists = tuple(a.cpu().numpy() for a in w["lists"])
    assert w["tick0"] == t_s
    np.testing.assert_array_equal(g["trial_of"], m["trial_of"])
    for k in ("slot", "start"):
        np.testing.assert_array_equal(t[k], m[k], err_msg=k)
    seen = np.array([q not in at_spawn for q in range(Q)])
    np.testing.assert_array_equal(t["ticks"], np.where(seen, m["ticks"], 0))
    np.testing.assert_array_equal(t["end_tick"][seen], np.where(end_local >= 0, t_s + end_local, -1)[seen])      # (tick numbers of the whole walk)
    np.testing.assert_array_equal(t["snapshot_ok"], ((snapshot_of >= 0) & (snapshot_of < int(pool["batch"]))).astype(np.int32))

    walks, where, by_slot = _pack(m, B, Q, end_local)
    refs = [_resume(cfg, opts, pool, trials, TT, snapshot_of, mm, models) for trials in walks]
    short = {}      # (the same resumed walks one tick shorter, made when a slot's lists need the other set)
    for q in range(Q):
        if q in at_spawn:
            continue
        j, b = where[q]
        ref, rows, s0 = refs[j], int(m["ticks"][q]), int(m["start"][q])
        for k in OUTCOME:
            _same_bits(t[k][q], ref[k][b], f"trial {q} {k}")
        for k in wr.TRACE:
            _same_bits(g[k][s0:s0 + rows, b], ref[k][:rows, b], f"trial {q} (slot {b}, start {s0}) {k}")
        if q < 3 or q == Q - 1:   # ... and the gather on the device gives those rows
            tr = {k: v.cpu().numpy() for k, v in w["trials"]["trace"](q).items()}
            assert tr["valid"].tolist() == [True] * rows + [False] * (TT - rows)
            for k in wr.TRACE:
                _same_bits(tr[k][:rows], ref[k][:rows, b], f"trial {q} gathered {k}")
        if end_local[q] < 0:      # the reference walked, through its TT ticks
            assert ref["end_tick"][b] == -1 and (ref["iterations"][:, b] > 0).all() and np.isfinite(ref["com"][:, b]).all(), q
        else:
            assert ref["end_tick"][b] == t_s + end_local[q] and ref["end_code"][b] == 5, q
    # the last trial of each slot: X, P, state, and the in-use entries of the returned lists.  Tick t of the refill walk writes set t % 2 and the walk returns
    # the set of tick T - 1; a slot whose last trial, spawned at s, stopped at its resumed tick e is out of every later launch, so its rows of the returned
    # set are tick e's if T - 1 - s - e is even, else the tick before's.  The resumed walk returns the set of its tick TT - 1 under the same rule: the two
    # agree when TT and T - s have the same parity, and otherwise the resumed walk one tick shorter returns the set that is wanted
    compared = 0
    for b in range(B):
        if not by_slot[b] or int(by_slot[b][-1]) in at_spawn:
            continue
        q = int(by_slot[b][-1])
        j, _ = where[q]
        for k in ("X", "P", "state"):
            _same_bits(g[k][b], refs[j][k][b], f"slot {b} (last trial {q}) {k}")
        if (TT - (T - int(m["start"][q]))) % 2:
            if j not in short:
                short[j] = _resume(cfg, opts, pool, walks[j], TT - 1, snapshot_of, mm, models)
            rt, rpose, rn = short[j]["lists"]
        else:
            rt, rpose, rn = refs[j]["lists"]
        np.testing.assert_array_equal(lists[2][b], rn[b], err_msg=f"slot {b} list counts")
        for c in range(2):
            n = int(rn[b, c])
            assert n >= 1
            _same_bits(lists[0][b, c, :n], rt[b, c, :n], f"slot {b} foot {c} list times")
            _same_bits(lists[1][b, c, :n], rpose[b, c, :n], f"slot {b} foot {c} list poses")
        compared += 1
    assert compared >= 1
    return g, t, m, refs, where, by_slot, T


def test_pushes_from_one_mid_gait_snapshot():
    """the checkpoint of tick 8 (the left foot in the air), Q = 10 trials of 9 resumed ticks -- the touchdown with its step adjustment at tick 14 and the
    right foot's lift at 16 are inside -- with repeated rows, per-trial hidden pushes, noise and gains; trials 1, 2 and 4 end early"""
    Q, TT = 10, 9
    cfg, pilot = _pilot(10)
    pool = pilot["checkpoints"][8]
    assert pool["tick"] == 8 and pool["lists_in"] == 1 and pool.get("wrench") is None
    end_local = np.full(Q, -1)
    end_local[[1, 2, 4]] = [2, 3, 4]
    T, m = _table(B, Q, TT, end_local)
    starts = {int(s) for s in m["start"] if s > 0}
    assert {s % 2 for s in starts} == {0, 1} and {int(e) % 2 for e in end_local if e >= 0} == {0, 1}, starts      # (spawns on walk ticks of both parities)
    snapshot_of = np.array([0, 1, 2, 3, 0, 0, 1, 2, 3, 1], np.int32)
    g, t, m, refs, where, _, _ = _walk_and_check(cfg, (), pool, Q, TT, snapshot_of, end_local, _mismatch(Q, TT, 72, end_local))
    for q, e in ((1, 2), (2, 3), (4, 4)):
        assert t["end_tick"][q] == 8 + e and t["end_code"][q] == 5
    # the scenario is the one the test is about: a landing inside the horizon from the first resumed tick, a step adjustment, and trials of one pool row
    # that differ (the hidden pushes are real)
    for q in (0, 5, 7):
        j, b = where[q]
        assert (refs[j]["land"][0, b] > 0).any() and (refs[j]["landing_offset"][:, b] != 0).any(), q
    assert snapshot_of[0] == snapshot_of[5] and not np.array_equal(rf.bits(t["final_state"][0]), rf.bits(t["final_state"][5]))


def test_pool_of_the_other_list_set():
    """the checkpoint of tick 5: the other lists_in, one tick before lift-off"""
    Q, TT = 7, 9
    cfg, pilot = _pilot(10)
    pool = pilot["checkpoints"][5]
    assert pool["tick"] == 5 and pool["lists_in"] == 0
    end_local = np.full(Q, -1)
    end_local[2] = 4
    snapshot_of = np.array([3, 2, 1, 0, 1, 1, 2], np.int32)
    g, t, m, _, _, _, _ = _walk_and_check(cfg, (), pool, Q, TT, snapshot_of, end_local, _mismatch(Q, TT, 73, end_local))
    assert {int(s) % 2 for s in m["start"]} == {0, 1}


def test_pool_of_the_touchdown_tick():
    """the checkpoint of tick 14, the tick the left foot lands on its adjusted step: the contact that is active from here on holds the pose the step
    adjustment wrote, and a merge carries it from the previous tick's list alone -- the pool's two list sets differ in it (asserted), so the set that
    reaches "previous" matters from the first resumed tick.  Trials of 12 ticks reach walk ticks 24 and 25, where the left foot's NEXT landing is inside the
    horizon and the back kernel looks for the next contact behind the whole-walk time: behind the ticks since spawn it would find the contact of tick 14"""
    Q, TT = 6, 12
    cfg, pilot = _pilot(10)
    pool = pilot["checkpoints"][14]
    assert pool["tick"] == 14 and pool["lists_in"] == 1
    (ta, pa, na), (tb, pb, nb) = [tuple(a.cpu().numpy() for a in st) for st in pool["lists"]]
    assert not np.array_equal(rf.bits(pa), rf.bits(pb)), "the pool's two list sets hold the same poses"
    end_local = np.full(Q, -1)
    end_local[1] = 2
    snapshot_of = np.array([0, 1, 2, 3, 2, 0], np.int32)
    g, t, m, refs, where, _, _ = _walk_and_check(cfg, (), pool, Q, TT, snapshot_of, end_local, _mismatch(Q, TT, 80, end_local))
    assert {int(s) % 2 for s in m["start"]} == {0, 1}
    j, b = where[0]
    assert (refs[j]["land"][-2:, b, 0] > 0).all(), "the left foot's next landing is not inside the horizon at walk ticks 24 and 25"


@pytest.mark.parametrize("n,opts", [(10, ()), (13, (("factors", "hbm"),))], ids=["N10-resident", "N13-hbm"])
def test_per_trial_models_together_with_the_snapshot(n, opts):
    """eight distinct models over a pool of the default model: the slot's record is rewritten at the spawn tick, which is not a first tick any more"""
    Q, TT = 8, 6
    cfg, pilot = _pilot(n, opts)
    pool = pilot["checkpoints"][8]
    end_local = np.full(Q, -1)
    end_local[[1, 3]] = [2, 3]
    models = _trial_models(Q)
    snapshot_of = np.array([0, 1, 2, 3, 3, 2, 1, 0], np.int32)
    mm = _mismatch(Q, TT, 74, end_local)
    g, t, m, _, _, _, T = _walk_and_check(cfg, opts, pool, Q, TT, snapshot_of, end_local, mm, models=models)
    assert t["model_ok"].tolist() == [1] * Q
    assert {int(s) % 2 for s in m["start"] if s > 0} == {0, 1}
    # the model reached the solve: the same queue without per-trial models ends somewhere else
    import torch
    plain = cm.rollout.WalkingRollout(cfg, B, **dict(opts)).walk_device_refill_from_snapshot(pool, T, TT, snapshot_of, mismatch=mm)
    torch.cuda.synchronize()
    final = plain["trials"]["final_state"].cpu().numpy()
    assert any(not np.array_equal(rf.bits(final[q]), rf.bits(t["final_state"][q])) for q in range(Q) if end_local[q] < 0)
    assert (plain["trials"]["model_ok"].cpu().numpy() == -1).all()


def test_an_index_outside_the_pool():
    """trial 5's index is the pool's batch size: snapshot_ok 0, nothing recorded, ended at spawn with the pool's tick and code 0; the trial that follows it in
    its slot is its resumed walk to the bit, and the trials spawned before it are bit-identical to the run in which the index is good"""
    import torch
    Q, TT = 10, 9
    cfg, pilot = _pilot(10)
    pool = pilot["checkpoints"][8]
    end_local = np.full(Q, -1)
    end_local[[1, 2]] = [2, 3]
    good_of = np.array([0, 1, 2, 3, 0, 0, 1, 2, 3, 1], np.int32)
    mm = _mismatch(Q, TT, 75, end_local)
    bad_of, bad_end = good_of.copy(), end_local.copy()
    bad_of[5], bad_end[5] = B, 0          # (held one tick: the model's trial that ends at its first tick)
    mm_bad = {k: v.copy() for k, v in mm.items()}
    g, t, m, refs, where, by_slot, T = _walk_and_check(cfg, (), pool, Q, TT, bad_of, bad_end, mm_bad, at_spawn=(5,))
    assert t["snapshot_ok"].tolist() == [1] * 5 + [0] + [1] * 4
    assert t["ticks"][5] == 0 and t["end_tick"][5] == 8 and t["end_code"][5] == 0 and t["iterations_sum"][5] == 0 and t["iterations_max"][5] == 0
    b5, s5 = int(m["slot"][5]), int(m["start"][5])
    assert g["code"][s5, b5] == -1 and np.isnan(g["com"][s5, b5]).all()          # (the record saw a problem that had ended before the tick)
    follower = int(by_slot[b5][by_slot[b5].index(5) + 1])
    assert m["start"][follower] == s5 + 1 and t["end_tick"][follower] == -1 and t["ticks"][follower] == TT      # (checked against its resumed walk above)
    # the run with a good index: every trial spawned at or before trial 5's tick sits where it sat, and is the same to the bit
    T2, m2 = _table(B, Q, TT, end_local)
    w2 = cm.rollout.WalkingRollout(cfg, B).walk_device_refill_from_snapshot(pool, T2, TT, good_of, mismatch=mm)
    torch.cuda.synchronize()
    t2, g2 = {k: v.cpu().numpy() for k, v in w2["trials"].items() if hasattr(v, "cpu")}, _host(w2)
    assert (t2["snapshot_ok"] == 1).all()
    same = [q for q in range(Q) if q != 5 and m["start"][q] <= s5 and m["start"][q] == m2["start"][q] and m["slot"][q] == m2["slot"][q]]
    assert len(same) >= 4 and any(m["start"][q] + m["ticks"][q] > s5 for q in same), same        # (neighbours that were walking while it was spawned)
    for q in same:
        rows, s0, b = int(m["ticks"][q]), int(m["start"][q]), int(m["slot"][q])
        for k in OUTCOME:
            _same_bits(t[k][q], t2[k][q], f"trial {q} {k}")
        for k in wr.TRACE:
            _same_bits(g[k][s0:s0 + rows, b], g2[k][s0:s0 + rows, b], f"trial {q} {k}")


def test_a_pool_row_that_ended_in_the_pilot():
    """the pilot's problem 2 measures a NaN state at tick 3 and ends there; a trial forked from that row is ended at spawn with the pilot's outcome, its slot
    goes to the next trial, and the trials forked from the other rows walk"""
    Q, TT = 7, 6
    cfg, pilot = _pilot(10, (), nan_at=(2, 3))
    pool = pilot["checkpoints"][8]
    p = {k: pool[k].cpu().numpy() for k in OUTCOME}
    assert p["end_tick"].tolist() == [-1, -1, 3, -1] and p["end_code"][2] >= 2
    snapshot_of = np.array([0, 1, 2, 3, 1, 0, 3], np.int32)
    end_local = np.full(Q, -1)
    end_local[2], end_local[4] = 0, 2          # (trial 2 is held one tick; trial 4 ends by its NaN row)
    mm = _mismatch(Q, TT, 76, np.where(np.arange(Q) == 2, -1, end_local))
    g, t, m, _, _, by_slot, _ = _walk_and_check(cfg, (), pool, Q, TT, snapshot_of, end_local, mm, at_spawn=(2,))
    for k in OUTCOME:
        _same_bits(t[k][2], p[k][2], f"the ended row's {k}")
    assert t["snapshot_ok"][2] == 1 and t["ticks"][2] == 0 and t["end_tick"][2] == 3
    b2, s2 = int(m["slot"][2]), int(m["start"][2])
    assert g["code"][s2, b2] == -1 and int(by_slot[b2][1]) == 4 and m["start"][4] == 1 and t["end_tick"][4] == 8 + 2


def test_fewer_trials_than_slots():
    Q, TT = 2, 5
    cfg, pilot = _pilot(10)
    pool = pilot["checkpoints"][8]
    end_local = np.full(Q, -1)
    g, t, m, _, _, _, T = _walk_and_check(cfg, (), pool, Q, TT, np.array([2, 2], np.int32), end_local, _mismatch(Q, TT, 77, end_local))
    assert T == TT and g["trial_of"].tolist() == [[0, 1, -1, -1]] * TT and (g["end_tick"][2:] == 0).all() and (t["end_tick"] == -1).all()
    assert (g["code"][:, 2:] == -1).all() and (g["X"][2:] == 0).all()          # (the empty slots: out of every launch, nothing restored)


def test_without_a_snapshot_the_new_entry_point_is_the_refill_trials_walk():
    """cmpc_rollout_walk_refill_snapshot_device with from == NULL against cmpc_rollout_walk_refill_trials_device: per-trial models and mismatch, a trial ended
    early, every key"""
    import torch
    N, Q, TT = 10, 7, 6
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    (com0, dcom0, h0, wrench), end_local = _queue(N, Q, TT, 78, {2: 3})
    T = rf.walk_length(B, Q, TT, end_local)
    models, mm = _trial_models(Q), _trial_mismatch(Q, TT - 1, TT - 2, 1, seed=79)
    want = cm.rollout.WalkingRollout(cfg, B).walk_device_refill_trials(T, TT, com0, dcom0, h0, models=models, mismatch=mm, wrench_trials=wrench)
    ro = cm.rollout.WalkingRollout(cfg, B)
    calls = []

    def through_the_new_entry(*a, **k):
        calls.append(len(a))
        return cm.BatchSolver.rollout_walk_refill_snapshot_device(ro.solver, *a, None, **k)
    ro.solver.rollout_walk_refill_device = through_the_new_entry
    got = ro.walk_device_refill_trials(T, TT, com0, dcom0, h0, models=models, mismatch=mm, wrench_trials=wrench)
    torch.cuda.synchronize()
    assert calls == [16]
    assert set(got) == set(want) and set(got["trials"]) == set(want["trials"])
    for k, v in want.items():
        if hasattr(v, "cpu"):
            _same_bits(_no_clock(k, got[k].cpu().numpy()), _no_clock(k, v.cpu().numpy()), k)
    for k, v in want["trials"].items():
        if hasattr(v, "cpu"):
            _same_bits(got["trials"][k].cpu().numpy(), v.cpu().numpy(), "trials " + k)
    for x, y in zip(got["lists"], want["lists"]):
        _same_bits(x.cpu().numpy(), y.cpu().numpy(), "lists")
    assert got["trials"]["end_tick"][2].item() == 3 and (got["trials"]["model_ok"].cpu().numpy() == 1).all()
