"""GPU: sensed pushes on the device walk (include/cmpc.h, "sensed pushes"; DESIGN.md 7f, "Sensed pushes"): a wrench sensor between the hidden-wrench
schedule and the MPC.  The three kernels against their host forms, to the bit; one call of the sensed walk against the existing mismatch walk fed the host
form's two schedules, to the bit; the blind sensor and no sensor against the mismatch walk; what the MPC does with what it is told; segments and a resume
across which the delay reaches; a NaN push that ends one problem alone, forwards and in the gradients; the gradients against the host transpose and by the
adjoint identity; no host read.
N = 10, dt = 0.06, the ergoCubGazeboV1 weights, B = 8, 6 ticks; the schedules are those of tests/test_wrench_sensor_cpu.py (tick_first = 1, 4 hidden rows,
3 noise rows, deadband 0.5: both branches of the dead-band in every row that has a source row, the threshold case in problem 3)."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests.test_gpu_mismatch import REC_KEYS, TAPE_KEYS, _cfg, _cu, _h
from tests.test_gpu_rollout_adjoint import ADJ
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_tape import GRADS, _same_bits
from tests.test_wrench_sensor_cpu import B, BAND, N, TICK_FIRST, TICKS as T, fixture

pytestmark = pytest.mark.gpu

ws = cm.wrench_sensor
DELAY, HOLD = 1, 3
WALK_ADJ = T * ADJ      # tests/test_gpu_mismatch_jvp.py: T chained ticks are held to T x ADJ
OTHERS = [0, 1, 2, 4, 5, 6, 7]


def _gain():
    return np.random.default_rng(8).uniform(0.9, 1.1, B).astype(np.float32)


def _sensor(ro, noise, delay=DELAY, hold=HOLD, deadband=BAND):
    return ro.wrench_sensor(delay=delay, hold_knots=hold, deadband=deadband, noise=None if noise is None else _cu(noise))


def _mm(hidden, **more):
    return dict(hidden_wrench=_cu(hidden), force_gain=_cu(_gain()), tick_first=TICK_FIRST, **more)


@pytest.fixture(scope="module")
def sensed6():
    """one sensed walk of 6 ticks, taped (delay 1, hold 3, sensor noise, a force gain), its reverse and its forward walk in k = 2 columns; the blind walk
    (deadband = inf) and the mismatch walk under the same hidden pushes"""
    import torch
    cfg = _cfg()
    com0, dcom0, h0, _ = _start(B)
    hidden, noise = fixture()
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_sensed(T, com0, dcom0, h0, _mm(hidden), _sensor(ro, noise), tape=True)
    rng = np.random.default_rng(2)
    gS = rng.normal(size=(T + 1, B, 9))
    dh, dn = rng.normal(size=(hidden.shape[0], B, 2, 6)), rng.normal(size=(noise.shape[0], B, 2, 6))
    got = ro.backward_device_sensed(w, _cu(gS))
    fwd = ro.forward_sensitivity_device_sensed(w, 2, dir_hidden_wrench=_cu(dh), dir_sensor_noise=_cu(dn))
    ro_b = cm.rollout.WalkingRollout(cfg, B)
    blind = ro_b.walk_device_sensed(T, com0, dcom0, h0, _mm(hidden), _sensor(ro_b, noise, deadband=np.inf), tape=True)
    ro_m = cm.rollout.WalkingRollout(cfg, B)
    hid = ro_m.walk_device_taped(T, com0, dcom0, h0, mismatch=_mm(hidden))
    torch.cuda.synchronize()
    host = ws.sense(N, hidden, TICK_FIRST, 0, T, DELAY, HOLD, BAND, noise)
    return dict(cfg=cfg, start=(com0, dcom0, h0), hidden=hidden, noise=noise, ro=ro, w=w, gS=gS, dh=dh, dn=dn, got=got, fwd=fwd, blind=blind, hid=hid,
                host=host)


def _same_walk(a, b, what, tape=True):
    if tape:
        for k in TAPE_KEYS:
            _same_bits(a["tape"][k], b["tape"][k], f"{what}: tape {k}")
        _same_bits(a["tape"]["info"][:, :, :6], b["tape"]["info"][:, :, :6], f"{what}: tape info")      # (word 6 is the clock)
    for k in REC_KEYS:
        _same_bits(a[k], b[k], f"{what}: {k}")


# ---- 1. the kernels ----
def test_kernels_are_the_host_forms():
    """B = 70 (one full wave and a partial one), rows = 5, k = 3: the sense, VJP and JVP launches bit-equal to the host forms, with and without the wrench
    rows; and hold_knots = N + 1 is refused on a handle that knows N"""
    import torch
    nb, rows, k, th, tn = 70, 5, 3, 4, 3
    rng = np.random.default_rng(70)
    hidden = np.concatenate([rng.normal(0, 0.45, (th, nb, 3)), rng.normal(0, 0.2, (th, nb, 3))], -1).astype(np.float32)
    hidden[1, 5, :3] = (0.5, 0, 0)      # (a force on the threshold)
    noise = rng.normal(0, 0.05, (tn, nb, 6)).astype(np.float32)
    noise[:, 5] = 0
    s = cm.BatchSolver(_cfg(), nb)
    mm = s.plant_mismatch(hidden_wrench=_cu(hidden), tick_first=1)
    sn = s._wrench_sensor(1, 3, BAND, _cu(noise))
    wr, pl, ps = s._wrench_sense_device(0, rows, mm, sn)
    _, pl2, ps2 = s._wrench_sense_device(0, rows, mm, sn, wrench_rows=False)
    gw, gh = rng.normal(size=(rows, nb, N, 6)).astype(np.float32), rng.normal(size=(rows, nb, 6))
    gt, gn = s._wrench_sense_vjp_device(0, rows, mm, sn, _cu(gw), _cu(gh))
    dh, dn = rng.normal(size=(th, nb, k, 6)), rng.normal(size=(tn, nb, k, 6))
    dw, dp = s._wrench_sense_jvp_device(0, rows, k, mm, sn, _cu(dh), _cu(dn))
    torch.cuda.synchronize()
    h_wr, h_pl, h_ps = ws.sense(N, hidden, 1, 0, rows, 1, 3, BAND, noise)
    assert 0 < h_ps.sum() < h_ps.size and h_ps[2, 5] == 1
    for a, b, what in ((wr, h_wr, "wrench rows"), (pl, h_pl, "plant rows"), (ps, h_ps, "pass"), (pl2, h_pl, "plant rows alone"), (ps2, h_ps, "pass alone")):
        _same_bits(a, b, what)
    h_gt, h_gn = ws.sense_vjp(N, hidden, 1, 0, rows, gw, gh, 1, 3, BAND, noise)
    _same_bits(gt, h_gt, "VJP: hidden")
    _same_bits(gn, h_gn, "VJP: noise")
    h_dw, h_dp = ws.sense_jvp(N, hidden, 1, 0, rows, k, dh, dn, 1, 3, BAND, noise)
    _same_bits(dw, h_dw, "JVP: wrench")
    _same_bits(dp, h_dp, "JVP: plant")
    assert np.abs(h_gt).max() > 0 and np.abs(h_gn).max() > 0 and np.abs(h_dw).max() > 0
    with pytest.raises(RuntimeError, match="hold_knots"):
        s._wrench_sense_device(0, rows, mm, s._wrench_sensor(1, N + 1, BAND, None))


# ---- 2. one call is the steps ----
def test_one_call_is_the_steps(sensed6):
    """walk_device_sensed(tape=True) against cmpc_rollout_walk_mismatch_device fed the host form's two schedules -- the wrench rows through
    cmpc_walk_io.dWrenchTicks, the plant rows through cmpc_plant_mismatch.dHiddenWrench (tick_first = 0) -- in every tape key and record key, to the bit;
    plant_wrench against the host form; the wrench rows of tape P non-zero exactly where dPass says, on the first hold_knots knots"""
    import torch
    v = sensed6
    com0, dcom0, h0 = v["start"]
    h_wr, h_pl, h_ps = v["host"]
    ro = cm.rollout.WalkingRollout(v["cfg"], B)
    rows = _cu(h_wr)
    ro._push_schedule = lambda dpush, push_ticks, columns: rows      # (the schedule walk_device would have built from push=: the host form's rows instead)
    by_hand = ro.walk_device_taped(T, com0, dcom0, h0, push=np.zeros((B, 3)), push_ticks=T,
                                   mismatch=dict(hidden_wrench=_cu(h_pl), force_gain=_cu(_gain()), tick_first=0))
    torch.cuda.synchronize()
    _same_walk(v["w"], by_hand, "sensed walk against the mismatch walk under the host form's schedules")
    _same_bits(v["w"]["plant_wrench"], h_pl, "plant_wrench")
    _same_bits(v["w"]["tape"]["plant_wrench"], h_pl, "the tape's plant_wrench")
    L, P = cm.Layout(N), _h(v["w"]["tape"]["P"])
    fext, text = P[:, :, L.p_fext:L.p_fext + 3 * N].reshape(T, B, N, 3), P[:, :, L.p_text:L.p_text + 3 * N].reshape(T, B, N, 3)
    told = np.concatenate([fext, text], -1)
    _same_bits(told, h_wr, "the wrench rows the solve saw")
    np.testing.assert_array_equal((told != 0).any((2, 3)), h_ps == 1)
    assert not told[:, :, HOLD:].any() and 0 < h_ps.sum() < h_ps.size
    print(f"\npass words by tick: {h_ps.sum(1).tolist()} of {B}; end ticks {_h(v['w']['end_tick']).tolist()}")


# ---- 3. blind is hidden, off is off ----
def test_blind_is_hidden_and_off_is_off(sensed6):
    """deadband = inf: walk_device_mismatch in every key (the MPC is told nothing, the plant feels the true wrench).  sensor = None: the same, and the tape
    has no sensor key"""
    import torch
    v = sensed6
    com0, dcom0, h0 = v["start"]
    _same_walk(v["blind"], v["hid"], "blind")
    ro = cm.rollout.WalkingRollout(v["cfg"], B)
    off = ro.walk_device_sensed(T, com0, dcom0, h0, _mm(v["hidden"]), None, tape=True)
    off_u = cm.rollout.WalkingRollout(v["cfg"], B).walk_device_sensed(T, com0, dcom0, h0, _mm(v["hidden"]), None)
    torch.cuda.synchronize()
    _same_walk(off, v["hid"], "sensor None")
    _same_walk(off_u, v["hid"], "sensor None, no tape", tape=False)
    assert "sensor" not in off["tape"] and "plant_wrench" not in off and set(off["tape"]) == set(v["hid"]["tape"])
    assert "sensor" in v["w"]["tape"] and "mismatch" in v["w"]["tape"]


# ---- 4. the MPC uses what it is told ----
def test_the_mpc_uses_what_it_is_told(sensed6):
    """on the ticks where the reading passes, the knot-0 corner forces of tape X differ from the blind walk's; before a problem's first passing tick the
    two walks are the same walk, to the bit.  The CoM deviations are printed and nothing is claimed of their size."""
    import torch
    v = sensed6
    com0, dcom0, h0 = v["start"]
    plain = cm.rollout.WalkingRollout(v["cfg"], B).walk_device(T, com0, dcom0, h0)
    torch.cuda.synchronize()
    L, ps = cm.Layout(N), v["host"][2]
    f0 = lambda w: np.concatenate([_h(w["tape"]["X"])[:, :, L.f[c][j]:L.f[c][j] + 3] for c in range(2) for j in range(4)], -1)
    fs, fb = f0(v["w"]), f0(v["blind"])
    seen = 0
    for b in range(B):
        first = np.flatnonzero(ps[:, b])
        for i in range(T):
            if ps[i, b] and _h(v["w"]["end_tick"])[b] < 0:
                assert (fs[i, b] != fb[i, b]).any(), (i, b)
                seen += 1
            if first.size == 0 or i < first[0]:
                _same_bits(fs[i, b], fb[i, b], f"problem {b} tick {i}: nothing told yet")
    assert seen > 0
    dev = lambda w: np.linalg.norm(_h(w["com"]).astype(np.float64) - _h(plain["com"]), axis=-1)
    print(f"\nCoM deviation from the unpushed walk, per problem at the last tick: sensed {np.round(dev(v['w'])[-1], 4).tolist()}")
    print(f"                                                                     blind  {np.round(dev(v['blind'])[-1], 4).tolist()}")


# ---- 5. segments and resume ----
def test_segments_and_resume_compose(sensed6):
    """ticks 0 .. 2 then 3 .. 5 through a snapshot and walk_resume_device_sensed against the single call, to the bit, with delay_ticks = 2 reaching across
    the cut (and state noise besides); skip_ended = True leaves the walking problems bit-equal"""
    import torch
    v = sensed6
    cfg, hidden, noise = v["cfg"], v["hidden"], v["noise"]
    com0, dcom0, h0 = v["start"]
    rng = np.random.default_rng(12)
    sn9 = np.concatenate([rng.normal(0, 3e-3, (3, B, 3)), rng.normal(0, 1e-2, (3, B, 3)), rng.normal(0, 2e-3, (3, B, 3))], -1).astype(np.float32)
    mm = lambda: _mm(hidden, state_noise=_cu(sn9))
    walk = lambda ticks, **kw: (lambda ro: ro.walk_device_sensed(ticks, com0, dcom0, h0, mm(), _sensor(ro, noise, delay=2), **kw))(
        cm.rollout.WalkingRollout(cfg, B))
    whole = walk(T)
    skipped = walk(T, skip_ended=True)
    first = walk(4, every=3)
    ro = cm.rollout.WalkingRollout(cfg, B)
    rest = ro.walk_resume_device_sensed(first["checkpoints"][3], 3, mm(), _sensor(ro, noise, delay=2))
    torch.cuda.synchronize()
    for k in ("state", "X", "P", "final_state", "iterations_sum", "iterations_max", "box_slack_min", "end_tick", "end_code"):
        _same_bits(rest[k], whole[k], f"resumed against the single call: {k}")
    for k in ("com", "zmp", "land", "landing_offset", "iterations", "code", "plant_wrench"):
        _same_bits(rest[k], whole[k][3:], f"resumed against the single call: {k}")
        _same_bits(first[k][:3], whole[k][:3], f"the first segment against the single call: {k}")
    h_ps = ws.sense(N, hidden, TICK_FIRST, 0, T, 2, HOLD, BAND, noise)[2]
    assert h_ps[3:].any() and h_ps[3:, 3].all()      # (the readings behind the cut are of rows in front of it)
    walking = np.flatnonzero(_h(whole["end_tick"]) < 0)
    assert walking.size > 0
    for k in REC_KEYS + ("plant_wrench",):
        if k == "stats":
            continue
        ax = 1 if k in ("com", "zmp", "land", "landing_offset", "iterations", "code", "plant_wrench") else 0
        _same_bits(np.take(_h(skipped[k]), walking, axis=ax), np.take(_h(whole[k]), walking, axis=ax), f"skip_ended: {k}")
    with pytest.raises(NotImplementedError):
        ro.backward_device_checkpointed(first, v["gS"][:5])


# ---- 6. a NaN reading ----
@pytest.mark.parametrize("delay", [0, 1])
def test_a_nan_push_ends_its_problem_alone(sensed6, delay):
    """NaN in problem 3's hidden row of tick 2.  delay 0: the reading of tick 2 is NaN, passes, and the solve sees it in P; delay 1: the plant feels it first.
    Either way problem 3 ends at tick 2 by one of the library's codes (2 .. 4 the solve's, 5 a non-finite state) and the seven others are bit-equal to the
    clean walk; in backward_device_sensed problem 3's rows of hidden_wrench and sensor_noise are exactly zero from its end tick on, the others' rows
    bit-equal to the clean walk's"""
    import torch
    v = sensed6
    cfg, hidden, noise = v["cfg"], v["hidden"], v["noise"]
    com0, dcom0, h0 = v["start"]
    bad = hidden.copy()
    bad[2 - TICK_FIRST, 3, 1] = np.nan
    out = {}
    for name, hw in (("clean", hidden), ("nan", bad)):
        ro = cm.rollout.WalkingRollout(cfg, B)
        w = ro.walk_device_sensed(T, com0, dcom0, h0, _mm(hw), _sensor(ro, noise, delay=delay), tape=True)
        out[name] = (w, ro.backward_device_sensed(w, _cu(v["gS"])))
    torch.cuda.synchronize()
    (w, g), (wc, gc) = out["nan"], out["clean"]
    code = int(w["end_code"][3])
    print(f"\ndelay {delay}: problem 3 ended at tick {int(w['end_tick'][3])} with code {code}; clean end ticks {_h(wc['end_tick']).tolist()}")
    assert int(w["end_tick"][3]) == 2 and code in (2, 3, 4, 5) and int(wc["end_tick"][3]) == -1
    if delay == 0:
        L = cm.Layout(N)
        assert np.isnan(_h(w["tape"]["P"])[2, 3, L.p_fext + 1])      # (the NaN reading passed the dead-band and reached the solve)
    for k in REC_KEYS + ("plant_wrench",):
        if k == "stats":
            continue
        ax = 1 if k in ("com", "zmp", "land", "landing_offset", "iterations", "code", "plant_wrench") else 0
        _same_bits(np.take(_h(w[k]), OTHERS, axis=ax), np.take(_h(wc[k]), OTHERS, axis=ax), k)
    for k in ("hidden_wrench", "sensor_noise", "plant_wrench", "wrench"):
        _same_bits(_h(g[k])[:, OTHERS], _h(gc[k])[:, OTHERS], f"gradient {k}: the other problems")
    # schedule row r is tick r + TICK_FIRST: from the end tick on nothing of problem 3 is left, and the row in front of it keeps the plant's own share
    assert not _h(g["hidden_wrench"])[2 - TICK_FIRST:, 3].any() and not _h(g["sensor_noise"])[2 - TICK_FIRST:, 3].any()
    assert not _h(g["plant_wrench"])[2:, 3].any() and _h(g["hidden_wrench"])[0, 3].any()
    assert np.isfinite(_h(g["hidden_wrench"])).all() and np.isfinite(_h(g["sensor_noise"])).all()


# ---- 7. gradients ----
def test_gradients_are_the_host_transpose_and_adjoint_to_the_forward_walk(sensed6):
    """backward_device_sensed's hidden_wrench and sensor_noise bit-equal to the host VJP form applied to the reverse walk's own wrench and plant rows; and
    per problem and column sum over the rows of <grad_states, forward states> == <hidden_wrench, dir> + <sensor_noise, dir>, relative gap <= T x ADJ, all
    groups at once and each alone (a missing term cannot hide: each right-hand side non-zero -- but for the sensor noise of a problem whose reading never
    passes the dead-band on a tick that has a noise row: there both sides are exactly zero)"""
    import torch
    v = sensed6
    ro, w, got, hidden, noise = v["ro"], v["w"], v["got"], v["hidden"], v["noise"]
    for k in GRADS + ("plant_wrench", "hidden_wrench", "sensor_noise", "force_gain"):
        assert k in got, k
    h_gt, h_gn = ws.sense_vjp(N, hidden, TICK_FIRST, 0, T, _h(got["wrench"]), _h(got["plant_wrench"]), DELAY, HOLD, BAND, noise)
    _same_bits(got["hidden_wrench"], h_gt, "hidden_wrench")
    _same_bits(got["sensor_noise"], h_gn, "sensor_noise")
    gS, gh, gn = v["gS"], _h(got["hidden_wrench"]), _h(got["sensor_noise"])
    only_h = ro.forward_sensitivity_device_sensed(w, 2, dir_hidden_wrench=_cu(v["dh"]))
    only_n = ro.forward_sensitivity_device_sensed(w, 2, dir_sensor_noise=_cu(v["dn"]))
    torch.cuda.synchronize()
    worst = 0.0
    ps = v["host"][2]
    heard = [bool(ps[TICK_FIRST:TICK_FIRST + noise.shape[0], b].any()) for b in range(B)]      # (noise row r is tick r + TICK_FIRST)
    assert any(heard) and not all(heard)
    for name, f, use_h, use_n in (("both", v["fwd"], True, True), ("hidden_wrench alone", only_h, True, False), ("sensor_noise alone", only_n, False, True)):
        fs = _h(f["states"])
        for b in range(B):
            for j in range(2):
                lhs = float((gS[:, b] * fs[:, b, j]).sum())
                rhs = (float((gh[:, b] * v["dh"][:, b, j]).sum()) if use_h else 0.0) + (float((gn[:, b] * v["dn"][:, b, j]).sum()) if use_n else 0.0)
                gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)
                print(f"{name}: problem {b} column {j}: forward {lhs:.9e}  reverse {rhs:.9e}  gap {gap:.2e}")
                if use_h or heard[b]:
                    assert abs(rhs) > 0 and gap <= WALK_ADJ, (name, b, j, gap)
                else:
                    assert lhs == 0.0 and rhs == 0.0, (name, b, j, lhs, rhs)
                worst = max(worst, gap)
    print(f"worst gap {worst:.2e} (bound {WALK_ADJ:.1e})")


# ---- 8. no host read ----
def test_nothing_is_read_back(sensed6):
    """walk_device_sensed, backward_device_sensed and forward_sensitivity_device_sensed under torch's sync debug mode, after the fixture's calls have
    allocated the workspaces"""
    import torch
    v = sensed6
    ro = v["ro"]
    com0, dcom0, h0 = (_cu(a.astype(np.float32)) for a in v["start"])
    mm, noise = _mm(v["hidden"]), _cu(v["noise"])
    gS, dh, dn = _cu(v["gS"]), _cu(v["dh"]), _cu(v["dn"])
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device_sensed(T, com0, dcom0, h0, mm, ro.wrench_sensor(DELAY, HOLD, BAND, noise), tape=True)
        r = ro.backward_device_sensed(w, gS)
        f = ro.forward_sensitivity_device_sensed(w, 2, dir_hidden_wrench=dh, dir_sensor_noise=dn)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for k in GRADS + ("plant_wrench", "hidden_wrench", "sensor_noise", "force_gain"):
        _same_bits(r[k], v["got"][k], k)
    _same_bits(f["states"], v["fwd"]["states"], "forward states")
