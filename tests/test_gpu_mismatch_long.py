"""GPU: the plant-model mismatch ("Mismatch") through lift-off, touchdown, resume and replan.  tests/test_gpu_mismatch.py walks 6 ticks at
N = 10, on which no contact changes; here the walk is 18 ticks long -- the left foot lifts at tick 6, its landing enters the horizon at tick 4, touchdown
with the step adjustment is at tick 14 and the right foot lifts at tick 16 -- under hidden pushes on ticks 5 .. 16, noise on ticks 5 .. 14 and gains in
[0.9, 1.1].  Every tick's plant is held to the float64 restatement (tests/mismatch_ref.walk_plant_gaps, bound 2e-6: the plant kernel's), the tick VJP to the
restated tick (bound REF); everything else is equality of bits, with the helpers of tests/test_gpu_mismatch.py: one call against the steps, the reverse walk
against the tick VJPs chained by hand, a replan inside the schedule against the unsegmented walk, an ending in single support, the checkpointed walk and
its resumed walks, the reverse of a resumed tape (the one place where tick number and tape row differ), a batch above the CU count with per-problem models,
N = 13 on the HBM-factor solver, and the order of the problems."""
import dataclasses

import numpy as np
import pytest

import cmpc_amd as cm
from tests import mismatch_ref as mr
from tests.test_gpu_mismatch import (NEW, REC_KEYS, TAPE_KEYS, _cu, _h, _mismatch, _reverse_by_hand, _steps_by_hand, _steps_by_tick_entry,
                                     _tick_vjp_gaps)
from tests.test_gpu_rollout_adjoint import REF
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_tape import GRADS, _same_bits

pytestmark = pytest.mark.gpu

N, B, T = 10, 8, 18
DT = 0.06
PER_TICK = ("com", "zmp", "land", "landing_offset", "iterations", "code")      # record keys [ticks, B, ..]; the others of REC_KEYS are [B, ..] (stats: [ticks, 6])
ROWS = ("wrench", "status", "hidden_wrench", "state_noise")                    # gradient keys [ticks, B, ..]
PLANT = 2e-6                                                                   # test_plant_kernel_matches_the_restatement's bound


def _cfg(n=N, dt=DT):
    return cm.config.ergocub_gazebo_v1(n, dt)


def _mm18():
    """hidden pushes on ticks 5 .. 16 (lift-off, touchdown and the second lift inside), noise on ticks 5 .. 14 (touchdown its last row, tick 16 outside),
    gains in [0.9, 1.1]; the magnitudes are _mismatch()'s, unshrunk"""
    return _mismatch(B, hidden_ticks=12, noise_ticks=10, tick_first=5, seed=31)


def _host(tape):
    return dict(X=_h(tape["X"]), P=_h(tape["P"]), states=_h(tape["states"]), step=tape["step"], substeps=tape["substeps"])


def _corners_of(cfg, models=None):
    """problem b's foot corners as the device holds them (float32), float64"""
    if models is None:
        one = np.asarray([c.corners for c in cfg.contacts], np.float64).astype(np.float32).astype(np.float64)
        return lambda b: one
    return lambda b: np.asarray(models[b, 10:], np.float64).astype(np.float32).astype(np.float64)


def _models(nb):
    """nb different model rows, built as tests/test_gpu_walk_refill_long._slot_models builds its four: friction and foot size per problem, cycling with
    periods 7 and 5 so that no two neighbours share a row"""
    base = _cfg()
    cfgs = []
    for b in range(nb):
        s = 0.85 + 0.075 * (b % 5)
        contacts = [dataclasses.replace(c, corners=[tuple(s * v for v in cn) for cn in c.corners]) for c in base.contacts]
        cfgs.append(dataclasses.replace(base, static_friction_coefficient=0.3 + 0.075 * (b % 7), contacts=contacts))
    return cm.config.model_array(cfgs)


def _contact_events(gamma):
    """gamma[T, B, 2] (the contact flags of knot 0, the same for every problem: one plan) -> (ticks the left foot is off, ticks the right foot is off,
    ticks at which a foot comes back)"""
    assert (gamma == gamma[:, :1]).all()
    g = gamma[:, 0]
    off = [[i for i in range(len(g)) if not g[i, c]] for c in range(2)]
    down = [i for i in range(1, len(g)) for c in range(2) if g[i, c] and not g[i - 1, c]]
    return off[0], off[1], down


# ---- 1. the full-length walk ----
@pytest.fixture(scope="module")
def walk18():
    """the 18-tick walk under _mm18(), taped, its reverse under random seeds, and the plain walk; the conditions on the scene are asserted here"""
    import torch
    cfg = _cfg()
    start = _start(B)[:3]
    mm = _mm18()
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(T, *start, mismatch=mm)
    ro_p = cm.rollout.WalkingRollout(cfg, B)
    plain = ro_p.walk_device(T, *start)
    gS = _cu(np.random.default_rng(2).normal(size=(T + 1, B, 9)))
    got = ro.backward_device(w, gS)
    torch.cuda.synchronize()
    assert (_h(w["end_tick"]) == -1).all() and (_h(plain["end_tick"]) == -1).all()
    moved = np.abs(_h(w["state"]) - _h(plain["state"])).max(1)
    off, off_p = _h(w["landing_offset"]), _h(plain["landing_offset"])
    adjusted = [b for b in range(B) if not np.array_equal(off[:, b], off_p[:, b])]
    print(f"\n18 ticks: the mismatch moved the final states by {moved.min():.2e} .. {moved.max():.2e}; landing_offset differs in problems {adjusted}")
    assert (moved > 1e-4).all()
    assert adjusted, "the mismatch did not reach the step adjustment"
    for r in (w, plain):       # the events are on the path (tests/test_gpu_walk_jvp.py's condition): the landing enters the horizon at tick 4, knot 1 at tick 13
        land = _h(r["land"])
        assert land[4, 0, 0] == N and land[13, 0, 0] == 1, land[:, 0, 0]
    return dict(cfg=cfg, start=start, mm=mm, ro=ro, w=w, plain=plain, gS=gS, got=got)


def test_every_ticks_plant_is_the_float64_plant(walk18):
    """all 18 ticks, all 8 problems: the restated plant on the tape's own X, P and true state, under that tick's hidden row (or none) and the gain, against the
    state the tick left, within 2e-6.  Independent of the plant kernel, which the comparisons of bits are not.  The left foot is off on ticks 6 .. 13
    (touchdown at 14), the right one on 16 and 17: X and P of single support and of the adjusted touchdown tick are among the inputs."""
    cfg, mm, tape = walk18["cfg"], walk18["mm"], walk18["w"]["tape"]
    gap, gamma = mr.walk_plant_gaps(cm.Layout(N), _corners_of(cfg), _host(tape), mm)
    left, right, down = _contact_events(gamma)
    print(f"\nplant of every tick against float64: worst gap per tick {np.array2string(gap.max(1), precision=1)} (bound {PLANT:.0e}); left foot off {left}, "
          f"right foot off {right}, touchdown {down}")
    assert left == list(range(6, 14)) and right == [16, 17] and down == [14]
    assert gap.max() <= PLANT, gap.max(1)
    # the check sees the mismatch: without the hidden rows and the gain the restated plant is further than that from the tape
    none, _ = mr.walk_plant_gaps(cm.Layout(N), _corners_of(cfg), _host(tape), dict(tick_first=0))
    assert none.max(1)[5:17].min() > 10 * PLANT, none.max(1)


def test_one_call_is_the_steps_through_every_contact_change(walk18):
    """the 18 ticks composed by hand and through the tick entry point (tests/test_gpu_mismatch.py's two loops) against the tape's P, X and states, and the
    untaped walk_device_mismatch against the taped walk in every record key: to the bit"""
    import torch
    cfg, mm, w = walk18["cfg"], walk18["mm"], walk18["w"]
    make_ro = lambda: cm.rollout.WalkingRollout(cfg, B)
    _steps_by_hand(make_ro, walk18["start"], mm, T, w["tape"])
    _steps_by_tick_entry(make_ro, walk18["start"], mm, T, w["tape"])
    untaped = make_ro().walk_device_mismatch(T, *walk18["start"], mm)
    torch.cuda.synchronize()
    for k in REC_KEYS:
        _same_bits(untaped[k], w[k], f"untaped against taped: {k}")
    # the noise reached the MPC's state on ticks 5 .. 14 and on no other
    L = cm.Layout(N)
    P, states = _h(w["tape"]["P"]), _h(w["tape"]["states"])
    differs = [i for i in range(T) if (P[i][:, L.p_com0:L.p_com0 + 9] != states[i]).any()]
    assert differs == list(range(5, 15)), differs


def test_tick_vjp_at_the_contact_changes(walk18):
    """cmpc_rollout_tick_vjp_mismatch_device against the restated tick on ticks 6 (lift-off), 14 (touchdown and adjustment), 16 (the second lift, outside the
    noise schedule) and 17 (outside both), problems 0 and 5: every group, hidden, noise and gain among them, within REF"""
    cfg, mm, tape, s = walk18["cfg"], walk18["mm"], walk18["w"]["tape"], walk18["ro"].solver
    worst = _tick_vjp_gaps(cfg, mm, tape, s, (6, 14, 16, 17), (0, 5), np.random.default_rng(22))
    print("mismatch tick VJP at the contact changes, worst: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {REF:.0e})")
    assert max(worst.values()) <= REF, worst


def _reverse_is_the_chain(ro, w, gS, mm, got):
    out, carry_s, carry_l = _reverse_by_hand(ro, w, gS, mm)
    _same_bits(carry_s, got["state0"], "state0")
    _same_bits(carry_l, got["list0"], "list0")
    for k in ("wrench", "models", "plan", "status") + NEW:
        _same_bits(out[k], got[k], k)
    assert (_h(got["status"]) == 0).all()
    for k in NEW:
        assert np.isfinite(_h(got[k])).all() and np.abs(_h(got[k])).max() > 0, k


def test_reverse_walk_through_the_landing(walk18):
    """backward_device on the 18-tick tape against the tick VJPs chained by hand through the gate: every key of GRADS + NEW to the bit (push is zero: the walk
    had no told push).  list0 and plan are non-zero -- the adjustment was on the gradient's path -- and the reverse walk through the entry without the
    mismatch, on the same tape, disagrees."""
    import torch
    mm, ro, w, gS, got = walk18["mm"], walk18["ro"], walk18["w"], walk18["gS"], walk18["got"]
    assert set(GRADS + NEW) <= set(got) and tuple(got["hidden_wrench"].shape) == (T, B, 6) and tuple(got["state_noise"].shape) == (T, B, 9)
    _reverse_is_the_chain(ro, w, gS, mm, got)
    assert not _h(got["push"]).any()
    assert np.abs(_h(got["list0"])).max() > 0 and np.abs(_h(got["plan"])).max() > 0
    old = dict(w, tape={k: v for k, v in w["tape"].items() if k != "mismatch"})
    plain = ro.backward_device(old, gS)
    torch.cuda.synchronize()
    assert not np.array_equal(_h(plain["state0"]), _h(got["state0"])) and not set(NEW) & set(plain)


def test_a_replan_inside_the_schedule_changes_no_bit(walk18):
    """replan = {9: the same plan}: two forward calls and two reverse calls, the cut inside both schedules.  Every tape key, every record key and every key of
    backward_device equals the unsegmented walk's to the bit -- force_gain, which the two reverse calls add to in place, and plan and models, among them"""
    import torch
    cfg, mm, w, gS, got = walk18["cfg"], walk18["mm"], walk18["w"], walk18["gS"], walk18["got"]
    ro = cm.rollout.WalkingRollout(cfg, B)
    w2 = ro.walk_device_taped(T, *walk18["start"], replan={9: tuple(ro.plan)}, mismatch=mm)
    got2 = ro.backward_device(w2, gS)
    torch.cuda.synchronize()
    assert w2["tape"]["segments"] == [0, 9] and w["tape"]["segments"] == [0]
    for k in TAPE_KEYS:
        _same_bits(w2["tape"][k], w["tape"][k], f"tape {k}")
    for k in REC_KEYS:
        _same_bits(w2[k], w[k], k)
    for k in GRADS + NEW:
        _same_bits(got2[k], got[k], f"backward_device: {k}")


@pytest.mark.parametrize("skip_ended", [False, True])
def test_an_ending_in_single_support(walk18, skip_ended):
    """NaN in problem 3's hidden row of tick 8, the left foot in the air.  Forwards: problem 3 ends alone at tick 8 with code 5, the seven others keep the
    bits of the undisturbed walk.  In reverse, with NaN seeds behind the end: rows 8 .. of hidden_wrench and state_noise are exact zeros for problem 3, its
    gradient is the 8-tick walk's, and the others' gradients keep the bits of the undisturbed reverse walk."""
    import torch
    cfg, mm, ref, gS, got_ref = walk18["cfg"], walk18["mm"], walk18["w"], walk18["gS"], walk18["got"]
    bad = dict(mm, hidden_wrench=mm["hidden_wrench"].copy())
    bad["hidden_wrench"][8 - mm["tick_first"], 3, 1] = np.nan
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(T, *walk18["start"], mismatch=bad, skip_ended=skip_ended)
    ro8 = cm.rollout.WalkingRollout(cfg, B)
    eight = ro8.walk_device_taped(8, *walk18["start"], mismatch=mm, skip_ended=skip_ended)
    seeds = _h(gS).copy()
    seeds_nan = seeds.copy()
    seeds_nan[9:, 3] = np.nan
    got = ro.backward_device(w, seeds_nan)
    short = ro8.backward_device(eight, seeds[:9])
    torch.cuda.synchronize()
    assert _h(w["end_tick"]).tolist() == [-1, -1, -1, 8, -1, -1, -1, -1] and int(w["end_code"][3]) == 5
    assert _h(w["code"])[:, 3].tolist() == [0] * 8 + [5] + [-1] * 9 and (_h(eight["end_tick"]) == -1).all()
    others = [0, 1, 2, 4, 5, 6, 7]
    for k in REC_KEYS:
        if k == "stats":
            continue
        ax = 1 if k in PER_TICK else 0
        _same_bits(np.take(_h(w[k]), others, axis=ax), np.take(_h(ref[k]), others, axis=ax), k)
    np.testing.assert_array_equal(_h(w["final_state"])[3, :3], _h(ref["com"])[7, 3])
    got, short, want = ({k: _h(r[k]) for k in GRADS + NEW} for r in (got, short, got_ref))
    for k in GRADS + NEW:
        assert np.isfinite(got[k]).all(), k
        ax = 1 if k in ROWS else 0
        _same_bits(np.take(got[k], others, axis=ax), np.take(want[k], others, axis=ax), f"the others: {k}")
    for k in ("state0", "list0", "push", "models", "plan", "force_gain"):
        _same_bits(got[k][3], short[k][3], f"problem 3: {k}")
    for k in ("wrench", "hidden_wrench", "state_noise"):
        _same_bits(got[k][:8, 3], short[k][:, 3], f"problem 3: {k}")
        assert not got[k][8:, 3].any(), k
    assert np.abs(got["hidden_wrench"][:8, 3]).max() > 0 and np.abs(got["state_noise"][:8, 3]).max() > 0 and got["force_gain"][3] != 0
    assert got["status"][:, 3].tolist() == [0] * 8 + [6] * 10


# ---- 2. checkpoints and a resumed tape ----
@pytest.fixture(scope="module")
def checkpointed18(walk18):
    import torch
    ro = cm.rollout.WalkingRollout(walk18["cfg"], B)
    wc = ro.walk_device_checkpointed(T, *walk18["start"], 7, mismatch=walk18["mm"])
    torch.cuda.synchronize()
    return dict(ro=ro, wc=wc)


def test_checkpointed_walk_and_its_resumed_walks(walk18, checkpointed18):
    """walk_device_checkpointed(18, every = 7) under the mismatch -- its calls cut at ticks 7 and 14, inside both schedules -- equals the one-call walk in every
    record key; walk_resume_device_mismatch from the snapshot of tick 7 (11 ticks) and of tick 14 (4 ticks) reaches the same final bits and the same rows
    on the way; backward_device_checkpointed still refuses"""
    import torch
    cfg, mm, w = walk18["cfg"], walk18["mm"], walk18["w"]
    ro, wc = checkpointed18["ro"], checkpointed18["wc"]
    assert sorted(wc["checkpoints"]) == [7, 14]
    for k in REC_KEYS:
        _same_bits(wc[k], w[k], f"checkpointed against one call: {k}")
    for t0 in (7, 14):
        r = cm.rollout.WalkingRollout(cfg, B).walk_resume_device_mismatch(wc["checkpoints"][t0], T - t0, mm)
        torch.cuda.synchronize()
        assert (_h(r["index_ok"]) == 1).all() and r["tick0"] == t0
        for k in REC_KEYS:
            if k == "stats":       # (counted per call: a resumed walk's rows are its own)
                continue
            _same_bits(r[k], w[k][t0:] if k in PER_TICK else w[k], f"resumed at tick {t0}: {k}")
    with pytest.raises(NotImplementedError):
        ro.backward_device_checkpointed(wc, np.zeros((T + 1, B, 9)))


def test_reverse_of_a_resumed_tape(walk18, checkpointed18):
    """walk_resume_device_mismatch(snapshot of tick 7, 11 ticks, taped=True): its tape rows 1 .. 11 are rows 7 .. 17 of the one-call walk's tape, and
    cmpc_rollout_walk_vjp_mismatch_device on it with tick0 = 7 and row0 = 1 -- tape row and tick number differ, the hidden row is selected by the tick, the
    gradient rows by the tape row -- returns the carries, the rows of wrench, hidden_wrench and state_noise, force_gain, plan and models of the same call on
    the one-call tape with tick0 = row0 = 7, to the bit"""
    import torch
    cfg, mm, w, gS = walk18["cfg"], walk18["mm"], walk18["w"], walk18["gS"]
    t0, n = 7, T - 7
    ro_r = cm.rollout.WalkingRollout(cfg, B)
    r = ro_r.walk_resume_device_mismatch(checkpointed18["wc"]["checkpoints"][t0], n, mm, taped=True)
    torch.cuda.synchronize()
    tape_r, tape = r["tape"], w["tape"]
    assert tape_r["rows"] == n + 1 and tape_r["tick0"] == t0 and tape_r["row0"] == 1 and "mismatch" in tape_r
    for k in TAPE_KEYS:
        _same_bits(tape_r[k][1:], tape[k][t0:], f"resumed tape: {k}")
    _same_bits(tape_r["list_t"][0], tape["list_t"][t0 - 1], "resumed tape: the stub row's list times")
    _same_bits(tape_r["list_n"][0], tape["list_n"][t0 - 1], "resumed tape: the stub row's list counts")

    def reverse(ro, tp, rows, tick0, row0, seeds, end_tick, carry0):
        M, dev = ro.M, ro.dev
        z = lambda shape, dtp=torch.float64: torch.zeros(shape, dtype=dtp, device=dev)
        out = dict(wrench=z((rows, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((rows, B), torch.int32),
                   hidden_wrench=z((rows, B, 6)), state_noise=z((rows, B, 9), torch.float32), force_gain=z((B,)))
        out["carry_state"], out["carry_list"] = (gS[T].clone() if carry0 else z((B, 9))), z((B, 2, M, 3))
        with torch.cuda.stream(ro.solver.launch_stream):
            ro.solver.rollout_walk_vjp_device(tick0, n, tp, row0, end_tick, seeds, out["carry_state"], out["carry_list"], out["status"], wrench=out["wrench"],
                                              dGradPlan=out["plan"], dGradModel=out["models"], mismatch=tp["mismatch"], grad_hidden=out["hidden_wrench"],
                                              grad_noise=out["state_noise"], grad_gain=out["force_gain"])
        torch.cuda.synchronize()
        return {k: _h(v) for k, v in out.items()}
    seeds_r = torch.zeros((n + 2, B, 9), dtype=torch.float64, device="cuda")
    seeds_r[1:] = gS[t0:]
    for carry0 in (False, True):      # from zero carries, and from the seed on the last state as backward_device starts
        a = reverse(ro_r, tape_r, n + 1, t0, 1, seeds_r, r["end_tick"], carry0)
        b = reverse(walk18["ro"], tape, T, t0, t0, gS, w["end_tick"], carry0)
        for k in ("carry_state", "carry_list", "models", "plan", "force_gain"):
            _same_bits(a[k], b[k], k)
            assert np.abs(b[k]).max() > 0, k
        for k in ROWS:
            _same_bits(a[k][1:], b[k][t0:], k)
            assert not a[k][0].any() and not b[k][:t0].any(), k          # no row outside the call was written
        assert (b["status"][t0:] == 0).all() and np.abs(b["hidden_wrench"][t0:]).max() > 0 and np.abs(b["state_noise"][t0:]).max() > 0


# ---- 3. other shapes ----
def _hold_a_walk(cfg, nb, ticks, mm, models, opts, plant_problems=None):
    """one taped walk under mm: all problems walk through; one call is the steps (by hand, and through the tick entry); every tick's plant is the float64
    plant (of plant_problems, or of all); backward_device is the tick VJPs chained by hand.  -> (the walk, gamma[ticks, nb, 2])"""
    import torch
    start = _start(nb)[:3]
    make_ro = lambda: cm.rollout.WalkingRollout(cfg, nb, models=models, **opts)
    ro = make_ro()
    w = ro.walk_device_taped(ticks, *start, mismatch=mm)
    gS = _cu(np.random.default_rng(3).normal(size=(ticks + 1, nb, 9)))
    got = ro.backward_device(w, gS)
    torch.cuda.synchronize()
    assert (_h(w["end_tick"]) == -1).all(), _h(w["end_tick"])
    _steps_by_hand(make_ro, start, mm, ticks, w["tape"])
    _steps_by_tick_entry(make_ro, start, mm, ticks, w["tape"])
    problems = list(range(nb)) if plant_problems is None else plant_problems
    gap, gamma = mr.walk_plant_gaps(cm.Layout(cfg.N), _corners_of(cfg, models), _host(w["tape"]), mm, problems)
    print(f"\nB = {nb}, N = {cfg.N}: plant of every tick against float64 ({len(problems)} problems), worst gap per tick "
          f"{np.array2string(gap[:, problems].max(1), precision=1)} (bound {PLANT:.0e})")
    assert gap[:, problems].max() <= PLANT
    _reverse_is_the_chain(ro, w, gS, mm, got)
    return w, gamma[:, problems]


def test_above_the_cu_count_with_per_problem_models():
    """B = 264 > 256 CUs, N = 10, 8 ticks (lift-off at tick 6 inside), per-problem models, the schedule on ticks 2 .. 7: the HBM-factor solver, a second
    workgroup of 8 lanes in the one-thread-per-problem kernels, a combine grid of 264, corners read at a stride under the mismatched plant.  The float64
    plant check runs on every eighth problem and on all 8 of the second workgroup (4 ms a call on the host)."""
    nb, ticks = 264, 8
    mm = _mismatch(nb, hidden_ticks=6, noise_ticks=5, tick_first=2, seed=37)
    w, gamma = _hold_a_walk(_cfg(), nb, ticks, mm, _models(nb), {}, list(range(0, 256, 8)) + list(range(256, 264)))
    left, right, down = _contact_events(gamma)
    assert left == [6, 7] and right == [] and down == []


def test_another_horizon_on_the_hbm_factor_solver():
    """N = 13, dt = 0.1, factors = "hbm", B = 8, 10 ticks, the schedule on ticks 1 .. 8; the contact changes are read from the tape and at least one lies
    inside the walk"""
    ticks = 10
    mm = _mismatch(B, hidden_ticks=8, noise_ticks=6, tick_first=1, seed=38)
    w, gamma = _hold_a_walk(_cfg(13, 0.1), B, ticks, mm, None, dict(factors="hbm"))
    left, right, down = _contact_events(gamma)
    land = _h(w["tape"]["land"])[:, 0]
    print(f"N = 13, dt = 0.1: left foot off {left}, right foot off {right}, touchdown {down}; landing knots of problem 0 per tick {land.tolist()}")
    changes = [i for i in range(1, ticks) if (gamma[i] != gamma[i - 1]).any()]
    assert changes, "no contact change inside the walk"


def _reversed_problems(cfg, nb, ticks, mm, models, start):
    """the walk under mm (None: the plain walk) and the walk of the same problems in reverse order, mismatch rows, gains, starts and models with them"""
    import torch
    flip = lambda a: None if a is None else np.ascontiguousarray(a[::-1])
    out = []
    for rev in (False, True):
        st = tuple(flip(a) for a in start) if rev else start
        md = flip(models) if rev else models
        m = mm
        if rev and mm is not None:
            m = dict(mm, hidden_wrench=np.ascontiguousarray(mm["hidden_wrench"][:, ::-1]), state_noise=np.ascontiguousarray(mm["state_noise"][:, ::-1]),
                     force_gain=flip(mm["force_gain"]))
        ro = cm.rollout.WalkingRollout(cfg, nb, models=md)
        out.append(ro.walk_device(ticks, *st) if m is None else ro.walk_device_mismatch(ticks, *st, m))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("nb,ticks", [(8, 18), (264, 8)])
def test_the_order_of_the_problems_changes_no_bit(nb, ticks):
    """the problems in reverse order, with their mismatch rows, gains, starts and models: every record key is the reversed original, to the bit -- first on the
    plain walk, the control, then under the mismatch"""
    cfg = _cfg()
    start = _start(nb)[:3]
    models = _models(nb)
    mm = _mm18() if nb == B else _mismatch(nb, hidden_ticks=6, noise_ticks=5, tick_first=2, seed=37)
    for name, m in (("plain", None), ("mismatch", mm)):
        a, b = _reversed_problems(cfg, nb, ticks, m, models, start)
        assert (_h(a["end_tick"]) == -1).all()
        for k in REC_KEYS:
            ha, hb = _h(a[k]), _h(b[k])
            _same_bits(hb, ha if k == "stats" else (ha[:, ::-1] if k in PER_TICK else ha[::-1]), f"{name}: {k}")
