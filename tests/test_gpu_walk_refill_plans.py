"""GPU: a footstep plan and reference trajectories per trial of a refill walk (include/cmpc.h, cmpc_walk_refill_plans;
WalkingRollout.walk_device_refill_plans).  Who sits where comes from the assignment model (tests/walk_refill_ref.py) and is asserted on the CPU before the
walk; every trial is then held, to the bit, to a walk of its own -- cmpc_rollout_walk_device, or cmpc_rollout_walk_mismatch_device with tick_first = 0 -- on
a roll-out of the same batch size, factor storage and options that holds it in the slot the model gives it, whose planner rows and reference rows of that
slot are the trial's pool row (the reference roll-out is given the padded pool rows as its plan tensors, and the pool's trajectories through
set_references).  Every check is equality of bits or of integers.
The shapes are tests/test_gpu_walk_refill_trials.py's: N = 10, dt = 0.06, B = 4, Q = 10, 18-tick trials."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_record_ref as wr
from tests import walk_refill_plans_ref as pr
from tests import walk_refill_ref as rf
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_refill_long import _pack, _plain_walk, _scenario
from tests.test_gpu_walk_refill_tape import GRAD, PER_TICK, _own_taped_walk
from tests.test_gpu_walk_refill_trials import OUTCOME, _cuda, _mismatch_walk, _no_clock, _same_bits, _table, _trial_mismatch, _trial_models

pytestmark = pytest.mark.gpu

DT = 0.06
_cache = {}


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items() if hasattr(v, "cpu")}


def _plans(cfg, off_grid=False):
    """the pool of the file: the default plan; a longer, faster step that lifts earlier (with off_grid every time 0.02 s off the MPC grid); a shorter list"""
    wp = cm.rollout.walking_plan
    return [wp(cfg), wp(cfg, step_length=0.16, swing=0.36, first_lift=0.26 if off_grid else 0.24), wp(cfg, steps=4)]


def _ref_rollout(cfg, B, opts, pool, prefs, rows, models=None):
    """a roll-out whose slot b holds pool row rows[b] as its plan and references"""
    import torch
    ro = cm.rollout.WalkingRollout(cfg, B, models=models, **opts)
    assert ro.M == pool[0].shape[2]
    ro.plan = tuple(torch.from_numpy(np.ascontiguousarray(a[rows])).to(ro.dev) for a in pool)
    if prefs is not None:
        idx = torch.as_tensor(np.asarray(rows, np.int64), device=ro.dev)
        ro.set_references(prefs["com"].index_select(0, idx), prefs["h"].index_select(0, idx), in_dt=prefs["in_dt"], t_first=prefs["t_first"],
                          robot_mass=prefs["robot_mass"], com_height=prefs["com_height"])
    return ro


def _walk_and_check(N, B, Q, TT, opts, scenario, end_local, plans, plan_of, models=None, mm=None, bad=(), taped=False):
    """the refill walk with plans per trial against walks that hold every trial in its slot with its pool row.  bad: the trials whose index lies outside
    the pool (ended at spawn: the model's table has them end at local tick 0; nothing of them is compared with a walk)
    -> (the roll-out, the walk's dict, its arrays on the host, its per-trial dict, the model's table, the reference walks, where[q] = (walk, slot))"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0, wrench = scenario
    T, m = _table(B, Q, TT, end_local)
    ro = cm.rollout.WalkingRollout(cfg, B, **opts)
    pool = ro.plan_pool(plans)
    prefs = ro.plan_references(plans, TT)
    before = [a.clone() for a in ro.plan]
    w = ro.walk_device_refill_plans(T, TT, com0, dcom0, h0, plans, plan_of, references=prefs, models=models, mismatch=mm, taped=taped, wrench_trials=wrench)
    torch.cuda.synchronize()
    for x, y in zip(ro.plan, before):      # the slots' planner rows passed to the walk were clones
        _same_bits(x.cpu().numpy(), y.cpu().numpy(), "the roll-out's plan")
    assert ro.references is None
    t, g = _host(w["trials"]), _host(w)
    lists = tuple(a.cpu().numpy() for a in w["lists"])
    np.testing.assert_array_equal(g["trial_of"], m["trial_of"])
    for k in ("slot", "start", "ticks", "end_tick"):
        np.testing.assert_array_equal(t[k], m[k], err_msg=k)
    np.testing.assert_array_equal(t["plan"], plan_of)
    assert t["plan_ok"].tolist() == [0 if q in bad else 1 for q in range(Q)]

    walks, where, by_slot = _pack(m, B, Q, end_local)
    rows_of = lambda trials: [int(plan_of[q]) if q not in bad else 0 for q in trials]
    refs = []
    for trials in walks:
        ref_ro = _ref_rollout(cfg, B, opts, pool, prefs, rows_of(trials), None if models is None else _cuda(models[trials]))
        refs.append(_plain_walk(ref_ro, trials, TT, com0, dcom0, h0, wrench) if mm is None else
                    _mismatch_walk(ref_ro, trials, TT, com0, dcom0, h0, wrench, mm))
    for q in range(Q):
        if q in bad:
            continue
        j, b = where[q]
        ref, rows, s0 = refs[j], int(m["ticks"][q]), int(m["start"][q])
        for k in OUTCOME:
            _same_bits(t[k][q], ref[k][b], f"trial {q} {k}")
        for k in wr.TRACE:
            _same_bits(g[k][s0:s0 + rows, b], ref[k][:rows, b], f"trial {q} (slot {b}, start {s0}) {k}")
    # the last trial of each slot: X, P, info, state and the in-use entries of the lists the walk returns (tests/test_gpu_walk_refill_trials.py's rule)
    compared = 0
    for b in range(B):
        q = int(by_slot[b][-1])
        assert q not in bad, "a trial ended at spawn must not be its slot's last (its rows are the trial's before it)"
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
    return ro, w, g, t, m, refs, where, by_slot, pool, prefs


def _successions(m, B, Q, end_local, plan_of):
    """the (row before, row after) pairs of consecutive trials of one slot, from the model's table"""
    _, _, by_slot = _pack(m, B, Q, end_local)
    return [(int(plan_of[a]), int(plan_of[b])) for v in by_slot for a, b in zip(v[:-1], v[1:])]


def _study():
    """test 1's walk, shared with test 3 and left unchanged"""
    if "study" in _cache:
        return _cache["study"]
    N, B, Q, TT = 10, 4, 10, 18
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, 71, {1: 2, 6: 9})
    plans, plan_of = _plans(cfg), (np.arange(Q) % 3).astype(np.int32)
    out = _walk_and_check(N, B, Q, TT, {}, (com0, dcom0, h0, wrench), end_local, plans, plan_of)
    _cache["study"] = dict(N=N, B=B, Q=Q, TT=TT, cfg=cfg, scenario=(com0, dcom0, h0, wrench), end_local=end_local, plans=plans, plan_of=plan_of, out=out)
    return _cache["study"]


def test_plans_per_trial():
    """a pool of three plans and their straight-line references, plan_of = q % 3, two trials ended early by a NaN wrench row"""
    N, B, Q, TT = 10, 4, 10, 18
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    _, _, _, _, end_local = _scenario(N, Q, TT, 71, {1: 2, 6: 9})
    plan_of = (np.arange(Q) % 3).astype(np.int32)
    # ---- the precondition, from the assignment model alone
    T, m = _table(B, Q, TT, end_local)
    pairs = _successions(m, B, Q, end_local, plan_of)
    assert any(a != b for a, b in pairs) and any(a in (0, 1) and b == 2 for a, b in pairs), pairs      # (rows 0 and 1 hold 4 contacts a foot, row 2 three)
    st = _study()
    ro, w, g, t, m, refs, where, by_slot, pool, prefs = st["out"]
    assert pool[2].tolist() == [[4, 4], [4, 4], [3, 3]] and ro.M == 5
    for q, e in ((1, 2), (6, 9)):
        assert t["end_tick"][q] == e and t["end_code"][q] == 3
    through = [q for q in range(Q) if end_local[q] < 0]
    for q in through:      # the reference walks walked, and through the contact changes
        j, b = where[q]
        assert refs[j]["end_tick"][b] == -1 and (refs[j]["iterations"][:, b] > 0).all(), q
        assert ((refs[j]["land"][:, b] >= 0).any(1) & (refs[j]["landing_offset"][:, b] != 0).any((1, 2))).any(), q
    assert {int(plan_of[q]) for q in through} == {0, 1, 2}
    # the pool's references are those of a roll-out constructed with the plan
    own = cm.rollout.WalkingRollout(cm.config.ergocub_gazebo_v1(N, DT), B, plan=st["plans"][1])
    _same_bits(own._planner_refs(TT)[0][0].cpu().numpy(), prefs["com"][1].cpu().numpy(), "pool references row 1")
    assert not np.array_equal(prefs["com"][1].cpu().numpy(), prefs["com"][0].cpu().numpy())


@pytest.mark.parametrize("case", ["N10-resident", "N13-hbm"])
def test_with_everything_else_per_trial(case):
    """a model and the full mismatch per trial, force_sample_time, and one pool plan whose times are 0.02 s off the grid: the snap inside a first tick and
    inside merge ticks reads copied rows.  N = 13 runs the HBM-factor solver on 8-tick trials"""
    N, TT, opts, ends = {"N10-resident": (10, 18, {}, {1: 2, 6: 9}), "N13-hbm": (13, 8, dict(factors="hbm"), {0: 3, 5: 1})}[case]
    B, Q = 4, 10
    opts = dict(opts, force_sample_time=True)
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, 72 if N == 10 else 73, ends)
    plans, plan_of = _plans(cfg, off_grid=True), (np.arange(Q) % 3).astype(np.int32)
    t1 = cm.contacts.pack_lists(cfg, [plans[1]])[0]
    off = np.abs(t1[t1 < 1e8] / DT - np.round(t1[t1 < 1e8] / DT)) * DT
    assert (off[t1[t1 < 1e8] > 0] > 0.019).all(), "plan 1 is 0.02 s off the grid at every time but zero"
    models = _trial_models(Q)
    mm = _trial_mismatch(Q, TT - 1, TT - 3, 1, seed=74)
    ro, w, g, t, m, refs, where, _, _, _ = _walk_and_check(N, B, Q, TT, opts, (com0, dcom0, h0, wrench), end_local, plans, plan_of, models=models, mm=mm)
    assert t["model_ok"].tolist() == [1] * Q
    through = [q for q in range(Q) if end_local[q] < 0]
    for q in through:
        j, b = where[q]
        assert refs[j]["end_tick"][b] == -1 and (refs[j]["iterations"][:, b] > 0).all(), q
    assert any(plan_of[q] == 1 for q in through)
    starts = sorted({int(v) for v in m["start"] if v > 0 and v % TT})
    assert len(starts) >= 2, starts      # (ticks on which a first tick with a copied plan sits among merge ticks)


def test_a_bad_index_ends_its_trial_at_spawn():
    """plan_of = Pn for trial 4 and -1 for trial 5: plan_ok 0, ended at spawn (local tick 0, code 0), the slot takes the next trial a tick later; every
    other trial is its walk to the bit, and a trial whose start the bad ones do not move is test 1's trial to the bit"""
    st = _study()
    N, B, Q, TT = st["N"], st["B"], st["Q"], st["TT"]
    end_local = st["end_local"].copy()
    plan_of = st["plan_of"].copy()
    plan_of[4], plan_of[5] = 3, -1
    end_local[[4, 5]] = 0
    ro, w, g, t, m, refs, where, by_slot, _, _ = _walk_and_check(N, B, Q, TT, {}, st["scenario"], end_local, st["plans"], plan_of, bad=(4, 5))
    for q in (4, 5):
        assert t["end_tick"][q] == 0 and t["end_code"][q] == 0 and t["ticks"][q] == 1 and t["iterations_sum"][q] == 0
        _same_bits(t["final_state"][q], np.concatenate([a[q] for a in st["scenario"][:3]]))
        s0, b = int(m["start"][q]), int(m["slot"][q])
        follower = by_slot[b][by_slot[b].index(q) + 1]
        assert m["start"][follower] == s0 + 1
    # the trials in front of the bad ones are test 1's, outcome and all (the same slot, the same start)
    t1, m1 = st["out"][3], st["out"][4]
    same = [q for q in range(Q) if q not in (4, 5) and m["slot"][q] == m1["slot"][q] and m["start"][q] == m1["start"][q]]
    assert len(same) >= 4
    for q in same:
        for k in OUTCOME:
            _same_bits(t[k][q], t1[k][q], f"trial {q} {k}")


def _equal_dicts(got, want, more=(), more_trials=()):
    assert set(got) == set(want) | set(more) and set(got["trials"]) == set(want["trials"]) | set(more_trials)
    for k, v in want.items():
        if hasattr(v, "cpu"):
            _same_bits(_no_clock(k, got[k].cpu().numpy()), _no_clock(k, v.cpu().numpy()), k)
    for k, v in want["trials"].items():
        if hasattr(v, "cpu"):
            _same_bits(got["trials"][k].cpu().numpy(), v.cpu().numpy(), "trials " + k)
    for x, y in zip(got["lists"], want["lists"]):
        _same_bits(x.cpu().numpy(), y.cpu().numpy(), "lists")
    if "tape" in want:
        for k, v in want["tape"].items():
            if hasattr(v, "cpu"):
                _same_bits(_no_clock(k, got["tape"][k].cpu().numpy()), _no_clock(k, v.cpu().numpy()), "tape " + k)


@pytest.mark.parametrize("taped", [False, True])
def test_nothing_per_trial(taped):
    """plans=None is walk_device_refill_trials (walk_device_refill_taped with taped=True) in every key; and a pool of one row equal to the roll-out's own
    plan, with the slots' references as the pool's, is bit-equal in every key both dicts share: the launch is a pure copy"""
    import torch
    N, B, Q, TT = 10, 4, 7, 6
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, 75, {2: 3})
    models, mm = _trial_models(Q), _trial_mismatch(Q, 5, 4, 1, seed=76)
    T = rf.walk_length(B, Q, TT, end_local)
    ro = cm.rollout.WalkingRollout(cfg, B)
    old = ro.walk_device_refill_taped if taped else ro.walk_device_refill_trials
    want = old(T, TT, com0, dcom0, h0, models=models, mismatch=mm, wrench_trials=wrench)
    got = cm.rollout.WalkingRollout(cfg, B).walk_device_refill_plans(T, TT, com0, dcom0, h0, None, None, models=models, mismatch=mm, taped=taped,
                                                                   wrench_trials=wrench)
    torch.cuda.synchronize()
    _equal_dicts(got, want)
    assert "plan_of" not in got.get("tape", {})
    ro2 = cm.rollout.WalkingRollout(cfg, B)
    plans = [cm.rollout.walking_plan(cfg)]
    for a, b in zip(ro2.plan_pool(plans), ro2.plan):
        _same_bits(a[0], b[0].cpu().numpy(), "the pool row of the roll-out's own plan")
    for refs in (None, ro2.plan_references(plans, TT)):
        one = ro2.walk_device_refill_plans(T, TT, com0, dcom0, h0, plans, np.zeros(Q, np.int32), references=refs, models=models, mismatch=mm, taped=taped,
                                           wrench_trials=wrench)
        torch.cuda.synchronize()
        _equal_dicts(one, want, more_trials=("plan", "plan_ok"))
        assert one["trials"]["plan_ok"].cpu().tolist() == [1] * Q
        if taped:
            assert one["tape"]["pool_plans"] == 1 and one["tape"]["plan_of"].cpu().tolist() == [0] * Q


def test_the_rollout_is_left_as_it_was():
    """a walk_device on the same roll-out before and after a plans walk: equal bits; self.plan and self.references are what they were"""
    import torch
    N, B, Q, TT = 10, 4, 6, 5
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    ro = cm.rollout.WalkingRollout(cfg, B)
    start = [a.astype(np.float32) for a in _start(B, seed=77)[:3]]
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, 78, {})
    walk = lambda: {k: v.cpu().numpy() for k, v in ro.walk_device(8, *start).items() if hasattr(v, "cpu")}
    before = walk()
    plan_before = [a.clone() for a in ro.plan]
    plans = _plans(cfg)
    w = ro.walk_device_refill_plans(rf.walk_length(B, Q, TT, end_local), TT, com0, dcom0, h0, plans, (np.arange(Q) % 3).astype(np.int32),
                                    references=ro.plan_references(plans, TT), models=_trial_models(Q), wrench_trials=wrench)
    torch.cuda.synchronize()
    assert w["trials"]["plan_ok"].cpu().tolist() == [1] * Q and ro.references is None and ro.models is None
    for x, y in zip(ro.plan, plan_before):
        _same_bits(x.cpu().numpy(), y.cpu().numpy(), "plan")
    after = walk()
    assert set(before) == set(after) and (before["end_tick"] == -1).all()
    for k in before:
        _same_bits(_no_clock(k, after[k]), _no_clock(k, before[k]), k)
    # the plans were not the roll-out's: the same queue on the roll-out's plan ends somewhere else
    plain = ro.walk_device_refill_trials(rf.walk_length(B, Q, TT, end_local), TT, com0, dcom0, h0, models=_trial_models(Q), wrench_trials=wrench)
    torch.cuda.synchronize()
    assert not np.array_equal(rf.bits(plain["trials"]["final_state"].cpu().numpy()), rf.bits(w["trials"]["final_state"].cpu().numpy()))


def test_gradient_and_the_pools_fold():
    """taped, seeds [19, Q, 9] and [18, Q, n_x]: every trial's keys of backward_device_refill against backward_device on a taped walk of its own with its
    plan; plan_pool against the host fold of plan + list0; a pool row no started trial used is exactly zero"""
    import torch
    N, B, Q, TT = 10, 4, 10, 18
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    ends = {1: 2, 6: 9}
    com0, dcom0, h0, wrench, end_local = _scenario(N, Q, TT, 79, ends)
    scenario = (com0, dcom0, h0, wrench)
    plans = _plans(cfg) + [cm.rollout.walking_plan(cfg, step_length=0.12)]      # row 3: nobody's
    plan_of = (np.arange(Q) % 3).astype(np.int32)
    mm = _trial_mismatch(Q, TT - 1, TT - 3, 1, seed=80)
    ro, w, g, t, m, _, where, _, pool, prefs = _walk_and_check(N, B, Q, TT, {}, scenario, end_local, plans, plan_of, mm=mm, taped=True)
    assert w["tape"]["pool_plans"] == 4 and w["tape"]["plan_of"].cpu().tolist() == plan_of.tolist()
    rng = np.random.default_rng(81)
    gS, gX = rng.normal(size=(TT + 1, Q, 9)), rng.normal(size=(TT, Q, ro.L.nx)).astype(np.float32)
    for q, e in ends.items():      # (the rows behind an ending are not to be read)
        gS[e + 1:, q] = np.nan
        gX[e:, q] = np.inf
    got = _host(ro.backward_device_refill(w, gS, gX))
    torch.cuda.synchronize()
    assert set(got) == set(GRAD) | {"plan_pool"} and got["plan_pool"].shape == (4, 2, ro.M, 3)
    walks, where, _ = _pack(m, B, Q, end_local)
    for j, trials in enumerate(walks):
        ref_ro = _ref_rollout(cfg, B, {}, pool, prefs, [int(plan_of[q]) for q in trials])
        own = _own_taped_walk(ref_ro, trials, TT, scenario, mm)
        want = _host(ref_ro.backward_device(own, gS[:, trials], gX[:, trials]))
        torch.cuda.synchronize()
        for b, q in enumerate(trials):
            if where[q] != (j, b):
                continue
            for k in GRAD:
                if k in PER_TICK:
                    _same_bits(got[k][:, q], want[k][:, b], f"trial {q} (walk {j}, slot {b}) {k}")
                else:
                    _same_bits(got[k][q], want[k][b], f"trial {q} (walk {j}, slot {b}) {k}")
    # the pool's gradient: the host fold, the restatement, and by hand
    lib = cm._capi.lib()
    per = np.ascontiguousarray(got["plan"] + got["list0"])
    host = np.full((4, 2, ro.M, 3), 7.0)
    assert lib.cmpc_rollout_plan_fold(Q, 6 * ro.M, plan_of.ctypes.data, per.ctypes.data, 4, host.ctypes.data) == 0
    _same_bits(got["plan_pool"], host, "plan_pool against the host fold")
    _same_bits(got["plan_pool"], pr.fold(plan_of, per, 4), "plan_pool against the restatement")
    assert (rf.bits(got["plan_pool"][3]) == 0).all()
    assert all((got["plan_pool"][p] != 0).any() for p in range(3)) and np.isfinite(got["plan_pool"]).all()


def _buffers(ro, Q, TT, T, state0):
    """the buffers WalkingRollout._walk_refill gives the walk, with a plan pool of two rows over clones of the roll-out's plan and references"""
    import torch
    s, L, dev, B = ro.solver, ro.L, ro.dev, ro.B
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    a = dict(dP=z((B, L.np)), dX0=z((B, L.nx)), dX=z((B, L.nx)), dInfo=z((B, 8)), state=z((B, 9)), ok=torch.ones((B,), dtype=torch.int32, device=dev),
             land=z((B, 2), torch.int32), zmp=z((B, 2)))
    a["rec"] = s.walk_record(T)
    s.outcome_init_device(a["state"], a["rec"])
    a["fill"] = s.walk_refill(torch.from_numpy(np.ascontiguousarray(state0, np.float32)).to(dev), TT, None, trace_rows=T, device=dev)
    a["plan"] = tuple(x.clone() for x in ro.plan)
    a["sets"] = [tuple(x.clone() for x in ro.plan), tuple(torch.zeros_like(x) for x in ro.plan)]
    refs = ro._planner_refs(TT)
    a["refs"] = (refs[0].clone(), refs[1].clone()) + tuple(refs[2:])
    return a


def test_c_entry_refusals_on_a_live_handle():
    """every refusal of cmpc_rollout_walk_refill_plans_device with plans, on a live handle, with its reason in cmpc_last_error; nothing is queued: the
    buffers keep their bits; and the same arguments, unspoilt, walk"""
    import torch
    N, B, Q, TT, T = 10, 4, 5, 3, 4
    cfg = cm.config.ergocub_gazebo_v1(N, DT)
    ro = cm.rollout.WalkingRollout(cfg, B)
    s = ro.solver
    a = _buffers(ro, Q, TT, T, np.concatenate([x.astype(np.float32) for x in _start(Q, seed=82)[:3]], 1))
    plans = [cm.rollout.walking_plan(cfg), cm.rollout.walking_plan(cfg, steps=4)]
    pool = ro.plan_pool(plans)
    prefs = ro.plan_references(plans, TT)
    of = np.array([0, 1, 1, 0, 1], np.int32)
    sel = s.walk_refill_plans(pool, of, a["plan"], (prefs["com"], prefs["h"]), planner=a["refs"], device=ro.dev)
    good = sel["_c"]
    spare = torch.zeros_like(a["plan"][0])

    def walk(c, planner=a["refs"], tape=None, tape_row0=0, plan=a["plan"]):
        sel["_c"] = c
        return s.rollout_walk_refill_plans_device(0, T, plan, a["sets"][0], a["sets"][1], 1, a["ok"], a["land"], a["state"], a["dP"], a["dX0"], a["dX"],
                                                  a["dInfo"], a["zmp"], a["rec"], a["fill"], sel, step=DT / ro.substeps, substeps=ro.substeps,
                                                  planner=planner, tape=tape, tape_row0=tape_row0)

    def spoilt(**fields):
        c = cm._capi.CmpcWalkRefillPlans.from_buffer_copy(good)
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def refused(words, c, **kw):
        with pytest.raises(RuntimeError) as e:
            walk(c, **kw)
        assert words in str(e.value), (words, str(e.value))

    refused("pool_plans must be at least 1", spoilt(pool_plans=0))
    refused("a pool list array is NULL", spoilt(dPoolN=None))
    refused("dTrialPlan is NULL", spoilt(dTrialPlan=None))
    refused("both or neither", spoilt(dPoolCom=None))
    refused("pool trajectories need io->tick.dPlanCom and dPlanH", good, planner=None)
    refused("a writable view is not io's pointer", spoilt(dPlanT=spare.data_ptr()))
    refused("a writable view is not io's pointer", spoilt(dPlanH=a["refs"][0].data_ptr()))
    refused("a writable view is not io's pointer", good, plan=tuple(x.clone() for x in a["plan"]))
    refused("a pool array is also a live array", spoilt(dPoolN=a["sets"][1][2].data_ptr()))
    refused("a pool array is also a live array", spoilt(dPoolT=a["plan"][0].data_ptr()))
    # what the taped call refuses stays refused: a tape with too few rows, and the multiplier output off
    tape = s.walk_tape(T - 1, ro.M, step=DT / ro.substeps, substeps=ro.substeps, device=ro.dev)
    refused("the tape has too few rows", good, tape=tape)
    refused("the multiplier output is off", good, tape=s.walk_tape(T, ro.M, step=DT / ro.substeps, substeps=ro.substeps, device=ro.dev))
    torch.cuda.synchronize()
    assert (a["dX"] == 0).all() and (a["fill"]["slot"].cpu().numpy() == -1).all() and (sel["plan_ok"] == -1).all()      # nothing was queued
    # ... and unspoilt, the call walks: every started trial has its flag and its plan row in its slot
    assert walk(good) in (0, 1)
    torch.cuda.synchronize()
    assert sel["plan_ok"].cpu().tolist() == [1] * Q and (a["rec"]["iterations"].cpu().numpy()[0] > 0).all()
    slot_of_4 = int(a["fill"]["slot"][4])
    _same_bits(a["plan"][0][slot_of_4].cpu().numpy(), pool[0][1], "slot's planner times")
    _same_bits(a["refs"][0][slot_of_4].cpu().numpy(), prefs["com"][1].cpu().numpy(), "slot's reference trajectory")
