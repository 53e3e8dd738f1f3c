"""Full-length refilled trials against plain walks (include/cmpc.h, cmpc_walk_refill; WalkingRollout.walk_device_refill): trials of 18 ticks at N = 10 see
the left foot lift (tick 6), its landing enter the horizon (tick 4), the touchdown with the step adjustment (tick 14) and the right foot's lift (tick 16), so
a refilled trial's lists leave the planner's and the back kernel's next contact depends on the LOCAL time.  Who sits where comes from the assignment model
(tests/walk_refill_ref.py); every trial is held, to the bit, to a plain walk of the same batch size, factor storage, options, models and references that
holds it in the slot the model gives it.  Cases: the resident solver, the HBM-factor solver with fresh and warm workgroups in one launch, the snap on fresh
ticks at s > 0, per-slot models and references read at a local time with t_first != 0, and a batch above the CU count (the assignment kernel's second chunk
inside a real walk)."""
import dataclasses

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_record_ref as wr
from tests import walk_refill_ref as rf
from tests.test_gpu_walk_record import _start

pytestmark = pytest.mark.gpu

OUTCOME = ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")
DT = 0.06


def _same_bits(x, y, msg=""):
    np.testing.assert_array_equal(rf.bits(x), rf.bits(y), err_msg=msg)


def _scenario(N, Q, trial_ticks, seed, ends, scale=1.0):
    """the queue: _start's states and, as wrench rows [trial_ticks, Q, N, 6] (every local tick has a row), its push under run()'s rule for push_ticks = 2;
    ends {q: local tick}: a NaN wrench row ends trial q there.  -> (com0, dcom0, h0, wrench, end_local[Q])"""
    com0, dcom0, h0, push = (a.astype(np.float32) for a in _start(Q, seed=seed))
    wrench = np.zeros((trial_ticks, Q, N, 6), np.float32)
    for i in range(2):
        wrench[i, :, :2 - i, :3] = np.float32(scale) * push[:, None, :]
    end_local = np.full(Q, -1)
    for q, e in ends.items():
        wrench[e, q] = np.nan
        end_local[q] = e
    return com0, dcom0, h0, wrench, end_local


def _slot_models(B):
    """B different model rows, built as tests/test_gpu_models.py builds its randomised ones: friction and foot size per slot"""
    base = cm.config.ergocub_gazebo_v1(10, DT)
    cfgs = []
    for b in range(B):
        s = 0.85 + 0.1 * b
        contacts = [dataclasses.replace(c, corners=[tuple(s * v for v in cn) for cn in c.corners]) for c in base.contacts]
        cfgs.append(dataclasses.replace(base, static_friction_coefficient=0.3 + 0.15 * b, contacts=contacts))
    return cm.config.model_array(cfgs)


def _rollout(cfg, B, opts, slots, trial_ticks):
    """a fresh roll-out of the case; slots: per-slot models and per-slot planner trajectories -- the straight line plus a lateral sinusoid of slot-dependent
    phase, a knot every 0.05 s (not dt) from t_first = -0.1 s, the height taken from the trajectory (com_height=None)"""
    ro = cm.rollout.WalkingRollout(cfg, B, models=_slot_models(B) if slots else None, **opts)
    if slots:
        in_dt, t_first = 0.05, -0.1
        knots = int(np.ceil((trial_ticks * DT + cfg.N * DT - t_first) / in_dt)) + 2
        t = t_first + in_dt * np.arange(knots)
        phase = 2.0 * np.pi * np.arange(B)[:, None] / B
        com = np.zeros((B, knots, 3))
        com[:, :, 0] = ro.com_speed * t[None, :]
        com[:, :, 1] = 0.01 * np.sin(2.0 * np.pi * t[None, :] / 0.9 + phase)
        com[:, :, 2] = 0.7 + 0.002 * np.cos(2.0 * np.pi * t[None, :] / 0.9 + phase)
        h = np.zeros((B, knots, 3))
        h[:, :, 0] = 0.005 * np.sin(2.0 * np.pi * t[None, :] / 0.9 + phase)
        ro.set_references(com, h, in_dt=in_dt, t_first=t_first, com_height=None)
        assert knots * in_dt + t_first >= trial_ticks * DT + cfg.N * DT
    return ro


def _plain_walk(ro, trials, trial_ticks, com0, dcom0, h0, wrench):
    """walk_device(trial_ticks, ..., skip_ended=True) of a batch that holds trials[b] in slot b, its wrench rows given as they are (walk_device itself builds
    them from a push): WalkingRollout._walk_live's calls with the rows passed through.  -> the record, X, P, state and BOTH list sets on the host (tick i
    wrote set i % 2), and the plan"""
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
    s.set_ended_device(rec["end_tick"])
    try:
        cur = s.rollout_walk_device(0, trial_ticks, True, ro.plan, sets[0], sets[1], 0, ok, land, state, dP, dX0, dX, dInfo, zmp, rec, row0=0, wrench_ticks=wt,
                                    step=dt / ro.substeps, substeps=ro.substeps, planner=ro._planner_refs(trial_ticks),
                                    force_sample_time=ro.force_sample_time)
        torch.cuda.synchronize()
    finally:
        s.set_ended_device(None)
    assert cur == (trial_ticks - 1) % 2
    out = {k: v.cpu().numpy() for k, v in rec.items() if hasattr(v, "cpu")}
    out.update(X=dX.cpu().numpy(), P=dP.cpu().numpy(), state=state.cpu().numpy(), sets=[tuple(a.cpu().numpy() for a in st) for st in sets],
               plan=tuple(a.cpu().numpy() for a in ro.plan))
    return out


def _pack(m, B, Q, end_local):
    """the slot table of the model as plain walks: walk j holds the j-th trial of every slot; a spare slot holds the first walked-through trial of the NEXT slot
    that has one (so some trial also walks in a slot that is not its own).  -> [trials[B]], {q: (walk, slot)} and the slots' trials in order"""
    by_slot = [[q for q in np.argsort(m["start"], kind="stable") if m["slot"][q] == b and m["start"][q] >= 0] for b in range(B)]
    assert sum(len(v) for v in by_slot) == Q, "ticks must be long enough for every trial to start"
    first = [next(q for i in range(1, B + 1) for q in by_slot[(b + i) % B] if end_local[q] < 0) for b in range(B)]
    walks, where = [], {}
    for j in range(max(len(v) for v in by_slot)):
        walks.append([int(by_slot[b][j]) if j < len(by_slot[b]) else int(first[b]) for b in range(B)])
        where.update({int(by_slot[b][j]): (j, b) for b in range(B) if j < len(by_slot[b])})
    return walks, where, by_slot


def _adjusted(ref, b):
    """(a foot's count differs from the planner's, an in-use pose is none of the planner's) in problem b's lists of a plain walk's last tick"""
    last = ref["sets"][(ref["com"].shape[0] - 1) % 2]
    (_, pose, n), (_, ppose, pn) = last, ref["plan"]
    count = bool((n[b] != pn[b]).any())
    moved = any(not any(np.array_equal(rf.bits(pose[b, c, i]), rf.bits(ppose[b, c, j])) for j in range(pn[b, c])) for c in range(2) for i in range(n[b, c]))
    return count, moved


CASES = {
    # id: N, B, Q, trial_ticks, roll-out options, per-slot models and references, endings {q: local tick}, seed
    "N10-resident": (10, 4, 10, 18, {}, False, {1: 2, 2: 8, 3: 15}, 41),
    "N13-hbm": (13, 4, 10, 18, dict(factors="hbm"), False, {1: 2, 2: 8, 3: 15}, 42),
    "N10-snap": (10, 4, 9, 18, dict(force_sample_time=True), False, {0: 4, 2: 7, 3: 16, 5: 0}, 43),
    "N10-slots": (10, 4, 10, 18, {}, True, {1: 2, 2: 8, 3: 15}, 44),
    # B = 264 > 256 CUs: two chunks of the assignment kernel.  Ten of the first 264 trials end early, in slots below and above 256 (3 and 257 at the same tick, 255
    # and 256 at the same tick: the second chunk's base is carried), and ten of the trials that follow them
    "above-CU": (10, 264, 400, 8, {}, False, {3: 2, 70: 0, 130: 5, 200: 2, 250: 3, 255: 1, 256: 1, 257: 2, 260: 5, 263: 0,
                                               264: 1, 265: 2, 266: 3, 267: 4, 270: 0, 272: 1, 300: 4, 330: 2, 350: 6, 399: 1}, 45),
}


@pytest.mark.parametrize("case", list(CASES))
def test_full_length_refilled_trials_are_plain_walks(case):
    import torch
    N, B, Q, TT, opts, slots, ends, seed = CASES[case]
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, seed, ends)
    T = rf.walk_length(B, Q, TT, end_local)
    m = rf.assignment_model(B, Q, TT, T, end_local)
    through = [q for q in range(Q) if end_local[q] < 0]
    # ---- the scenario is the one the test is about (the model's table)
    starts = sorted({int(v) for v in m["start"] if v > 0 and v % TT})
    assert len(starts) >= 3, starts
    assert any(1 <= m["start"][q] <= 9 for q in through)          # (its global time passes 0.84 s while its local time has not)
    assert (m["ticks"][through] == TT).all() and (m["start"] >= 0).all()
    if TT == 18:
        assert any(e > 6 for e in ends.values()) and any(e > 14 for e in ends.values())
    else:
        low, high = [m["slot"][q] for q in ends if m["slot"][q] < 256], [m["slot"][q] for q in ends if m["slot"][q] >= 256]
        assert len(ends) >= 20 and len(low) >= 5 and len(high) >= 5
        both = [t for t in range(1, T) if (m["slot"][m["start"] == t] < 256).any() and (m["slot"][m["start"] == t] >= 256).any()]
        assert len(both) >= 2, "no tick hands trials out in both chunks"

    # ---- the refill walk, and its assignment against the model
    w = _rollout(cfg, B, opts, slots, TT).walk_device_refill(T, TT, com0, dcom0, h0, wrench_trials=wrench)
    torch.cuda.synchronize()
    t = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
    g = {k: v.cpu().numpy() for k, v in w.items() if hasattr(v, "cpu")}
    lists = tuple(a.cpu().numpy() for a in w["lists"])
    np.testing.assert_array_equal(g["trial_of"], m["trial_of"])
    for k in ("slot", "start", "ticks", "end_tick"):
        np.testing.assert_array_equal(t[k], m[k], err_msg=k)

    # ---- the plain walks: as few as the slot table allows
    walks, where, by_slot = _pack(m, B, Q, end_local)
    assert len(walks) == max(len(v) for v in by_slot) <= 4
    refs = [_plain_walk(_rollout(cfg, B, opts, slots, TT), trials, TT, com0, dcom0, h0, wrench) for trials in walks]

    # ---- the conditions on the inputs, on the reference walks only
    offsets = {}
    flags = []
    for q in through:
        j, b = where[q]
        ref = refs[j]
        assert ref["end_tick"][b] == -1 and np.isfinite(ref["com"][:, b]).all() and (ref["iterations"][:, b] > 0).all(), q
        rows = (ref["land"][:, b] >= 0).any(1) & (ref["landing_offset"][:, b] != 0).any((1, 2))
        assert rows.any(), f"trial {q}: no row with a landing in the horizon and a non-zero landing offset"
        offsets[q] = ref["landing_offset"][:, b].tobytes()
        flags.append(_adjusted(ref, b))
    assert len(set(offsets.values())) == len(through), "two walked-through trials have the same landing offsets"
    print(f"{case}: T = {T}, {len(walks)} plain walks, walked through {len(through)}, count differs {sum(f[0] for f in flags)}, pose written "
          f"{sum(f[1] for f in flags)}")
    assert all(f[0] for f in flags), "a walked-through trial's last lists have the planner's counts"
    assert all(f[1] for f in flags), "the step adjustment wrote no pose"
    for q, e in ends.items():
        j, b = where[q]
        assert refs[j]["end_tick"][b] == e and refs[j]["end_code"][b] == 3, q

    # ---- every trial: outcome and trace rows, to the bit
    for q in range(Q):
        j, b = where[q]
        ref, rows, s0 = refs[j], int(m["ticks"][q]), int(m["start"][q])
        for k in OUTCOME:
            _same_bits(t[k][q], ref[k][b], f"trial {q} {k}")
        for k in wr.TRACE:
            _same_bits(g[k][s0:s0 + rows, b], ref[k][:rows, b], f"trial {q} (slot {b}, start {s0}) {k}")
    if Q <= 10:          # ... and the gather on the device gives those rows
        for q in range(Q):
            tr = {k: v.cpu().numpy() for k, v in w["trials"]["trace"](q).items()}
            rows, (j, b) = int(m["ticks"][q]), where[q]
            assert tr["valid"].tolist() == [True] * rows + [False] * (TT - rows)
            for k in wr.TRACE:
                _same_bits(tr[k][:rows], refs[j][k][:rows, b], f"trial {q} gathered {k}")

    # ---- the last trial of each slot: what the slot's buffers hold when the walk returns.  Tick t of the refill walk writes list set t % 2 and the walk returns
    # set (T - 1) % 2; local tick i of a plain walk writes set i % 2.  A slot whose last trial stopped at global tick last (local tick e) is left out of every later
    # launch, so its rows of the returned set are local tick e's if last and T - 1 have the same parity, else local tick e - 1's
    compared = 0
    for b in range(B):
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
    assert compared >= B - 2

    # ---- per-slot models and references are real: one trial walked plainly in two different slots differs
    if slots:
        q = walks[-1][next(b for b in range(B) if where.get(walks[-1][b]) != (len(walks) - 1, b))]
        (j0, b0), b1 = where[q], walks[-1].index(q)
        assert b0 != b1 and not np.array_equal(rf.bits(refs[j0]["com"][:, b0]), rf.bits(refs[-1]["com"][:, b1]))
