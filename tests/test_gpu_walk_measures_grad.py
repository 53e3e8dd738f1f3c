"""GPU: the derivative of a device walk's stability measures (include/cmpc.h, "the measures, differentiated"; WalkingRollout.backward_device_measures,
forward_sensitivity_device_measures, rollout_differentiable_measures).  The three kernels against the host forms, bit for bit; the reverse walk on the
augmented seeds recomposed from the host form on the tape; the adjoint identity on the device, endings included, held to T x ADJ (the per-tick bound of
tests/test_gpu_rollout_jvp.py, as tests/test_gpu_walk_jvp.py uses it); the autograd layer; no host read.  N = 10, dt = 0.06, the ergoCubGazeboV1
weights."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_measures_grad_ref as mg
from tests.test_gpu_rollout_jvp import ADJ
from tests.test_gpu_walk_limits import PUSHES, STOP, _between, _cfg_corners, _hidden, _stand
from tests.test_gpu_walk_record import _solver_with_box, _start
from tests.test_gpu_walk_tape import _same_bits
from tests.test_walk_measures_grad_cpu import random_tape

pytestmark = pytest.mark.gpu

N, DT, G = 10, 0.06, cm.config.GRAVITY


def _cfg():
    return cm.config.ergocub_gazebo_v1(N, DT)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the kernels against the host forms ----
@pytest.mark.parametrize("case", [(70, False), (70, True), (300, False)], ids=["B70", "B70-models", "B300"])
def test_kernels_are_the_host_forms(case):
    """VJP, fold and JVP (k = 3) on the CPU test's tapes, rows = 2: B = 70 (a partial second wave), B = 300 (a second workgroup); the handle's corners
    and per-problem models (the corner stride of the model records); random end ticks with NaN behind them in the tape, the seeds and the directions"""
    import torch
    B, models = case
    cfg, lib = _cfg(), cm._capi.lib()
    X, P, S, _ = random_tape(B)
    s = _solver_with_box(cfg, B)
    corners = _cfg_corners(cfg)
    if models:
        rng = np.random.default_rng(B)
        rows = np.tile(cm.config.model_row(cfg), (B, 1))
        rows[:, 10:] *= rng.uniform(0.9, 1.1, (B, 1))
        s.set_models(rows)
        corners = rows[:, 10:].astype(np.float32).reshape(B, 2, 4, 3)
    rng = np.random.default_rng(B + 1)
    tick0, k = 3, 3
    e = mg.random_end_tick(rng, B, 2, tick0)
    counted = np.array([[(e[b] < 0) or (tick0 + r < e[b]) for b in range(B)] for r in range(2)])
    X, P, S = mg.poison_behind(X, P, S, e, tick0)
    gM, gS, gX = mg.random_seeds(rng, N, 2, B)
    gM[~counted], gX[~counted] = np.nan, np.nan
    gS[1:][~counted] = np.nan
    dS, dX, dP, dModel = mg.random_dirs(rng, N, 2, B, k)
    dS[1:][~counted], dX[~counted], dP[~counted] = np.nan, np.nan, np.nan
    hS, hX, hD = mg.host_vjp(lib, N, X, P, S, e, corners, G, gM, gS, gX, tick0)
    hM = mg.host_jvp(lib, N, X, P, S, e, corners, G, dS, dX, dP, dModel, tick0)
    hP, hMod = np.random.default_rng(5).standard_normal((2, B, s.layout.np)).astype(np.float32), np.random.default_rng(6).standard_normal((B, 34))
    fP, fMod = hP.copy(), hMod.copy()
    assert lib.cmpc_walk_measures_vjp_fold(N, B, 2, mg._ptr(hD), mg._ptr(fP), mg._ptr(fMod)) == 0
    tape = s.walk_tape(2, 3)
    tape["X"].copy_(_dev(X)); tape["P"].copy_(_dev(P)); tape["states"].copy_(_dev(S))
    dE, dgS, dgX = _dev(e), _dev(gS), _dev(gX)
    direct = torch.full((2, B, 32), 99.0, dtype=torch.float64, device="cuda")
    s.walk_measures_vjp_device(tick0, 2, tape, 0, dE, _dev(gM), dgS, dgX, direct)
    dgP, dgMod = _dev(hP), _dev(hMod)
    s.walk_measures_vjp_fold_device(direct, dgP, dgMod)
    dMe = torch.full((2, B, k, 4), 99.0, dtype=torch.float64, device="cuda")
    s.walk_measures_jvp_device(tick0, 2, tape, 0, dE, k, _dev(dS), _dev(dX), dMe, dir_p=_dev(dP), dir_model=_dev(dModel))
    torch.cuda.synchronize()
    for name, got, want in (("grad_states", dgS, hS), ("grad_X", dgX, hX), ("direct", direct, hD), ("grad_P", dgP, fP), ("grad_model", dgMod, fMod),
                            ("dir_measures", dMe, hM)):
        _same_bits(got.cpu().numpy(), want, name)
    assert (hD[~counted] == 0).all() and np.isfinite(hD).all() and np.abs(hD[counted]).max() > 0 and (hM[~counted] == 0).all()
    assert np.abs(hM[counted]).max() > 0 and np.isfinite(hM).all()


def test_device_forms_refuse_bad_arguments():
    """rows outside the tape and k < 1: CMPC_ERR_ARG before anything is queued"""
    import torch
    cfg, B = _cfg(), 4
    s = _solver_with_box(cfg, B)
    tape = s.walk_tape(2, 3)
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")
    gM, gS, gX, direct = z((2, B, 4)), z((3, B, 9)), z((2, B, s.layout.nx), torch.float32), z((2, B, 32))
    s.walk_measures_vjp_device(0, 2, tape, 0, None, gM, gS, gX, direct)
    for tick0, ticks, row0 in ((0, 3, 0), (0, 2, 1), (0, 0, 0), (-1, 1, 0), (0, 1, -1)):
        with pytest.raises(RuntimeError, match="cmpc_walk_measures_vjp_device"):
            s.walk_measures_vjp_device(tick0, ticks, tape, row0, None, gM, gS, gX, direct)
    dS, dX, dM = z((3, B, 1, 9)), z((2, B, 1, s.layout.nx), torch.float32), z((2, B, 1, 4))
    s.walk_measures_jvp_device(0, 2, tape, 0, None, 1, dS, dX, dM)
    with pytest.raises(RuntimeError, match="cmpc_walk_measures_jvp_device"):
        s.walk_measures_jvp_device(0, 3, tape, 0, None, 1, dS, dX, dM)
    lib = cm._capi.lib()
    d = cm._capi.CmpcWalkMeasureDirs(dS.data_ptr(), dX.data_ptr(), None, None, dM.data_ptr())
    assert lib.cmpc_walk_measures_jvp_device(s._h, 0, 2, tape["_c"], 0, None, 0, d, None) != 0      # k < 1
    assert lib.cmpc_walk_measures_vjp_fold_device(s._h, 0, direct.data_ptr(), None, None, None) != 0     # rows < 1
    torch.cuda.synchronize()
    assert (direct == 0).all() and (dM == 0).all()


# ---- 2. recomposition: a taped walk under graded hidden pushes, limits that end somebody ----
@pytest.fixture(scope="module")
def limited():
    import torch
    cfg, B, T = _cfg(), 8, 6
    ro = cm.rollout.WalkingRollout(cfg, B)
    table = [(a, m, t0, min(t1, T)) for a, m, t0, t1 in PUSHES]
    start, mm = _stand(B), dict(hidden_wrench=_hidden(T, table))
    ro.set_limits()
    free = ro.walk_device_taped(T, *start, mismatch=mm)
    torch.cuda.synchronize()
    track = free["measures"][..., 3].cpu().numpy().max(0)
    ro.set_limits(track_max=_between(track, B - 3))      # the two problems pushed hardest off their reference end
    w = ro.walk_device_taped(T, *start, mismatch=mm, stop=STOP)
    torch.cuda.synchronize()
    end = w["end_tick"].cpu().numpy()
    assert (end >= 0).sum() == 2 and (end[end >= 0] > 0).all(), end
    ro.clear_limits()
    tp = w["tape"]
    host = dict(X=tp["X"].cpu().numpy(), P=tp["P"].cpu().numpy(), S=tp["states"].cpu().numpy(), end=end, corners=_cfg_corners(cfg))
    return dict(cfg=cfg, B=B, T=T, ro=ro, w=w, host=host)


def _seeds(c, seed):
    rng = np.random.default_rng(seed)
    T, B, nx = c["T"], c["B"], c["ro"].L.nx
    return rng.normal(size=(T, B, 4)), rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, nx))).astype(np.float32)


def test_reverse_walk_on_the_augmented_seeds(limited):
    """backward_device_measures(w, gM, gS, gX) against backward_device(w, gS', gX') with the seeds augmented by the HOST form on the tape: every shared
    key bit-equal (models: plus the host fold of the corners' term), measure_direct the host form's; with gM = 0 bit-equal to backward_device"""
    import torch
    c, lib = limited, cm._capi.lib()
    ro, w, h, T, B = c["ro"], c["w"], c["host"], c["T"], c["B"]
    gM, gS, gX = _seeds(c, 21)
    for b in np.flatnonzero(h["end"] >= 0):      # (the cotangents of the row that fired and of the rows behind it are not read)
        gM[h["end"][b]:, b] = np.nan
    hS, hX, hD = mg.host_vjp(lib, N, h["X"], h["P"], h["S"], h["end"], h["corners"], G, gM, gS, gX)
    got = ro.backward_device_measures(w, gM, gS, gX)
    want = ro.backward_device(w, hS, hX)
    zero = ro.backward_device_measures(w, np.zeros_like(gM), gS, gX)
    plain = ro.backward_device(w, gS, gX)
    torch.cuda.synchronize()
    assert set(got) == set(want) | {"measure_direct", "measure_rot"}
    models = want["models"].cpu().numpy().copy()
    assert lib.cmpc_walk_measures_vjp_fold(N, B, T, mg._ptr(hD), None, mg._ptr(models)) == 0
    for k in want:
        _same_bits(got[k].cpu().numpy(), models if k == "models" else want[k].cpu().numpy(), k)
    _same_bits(got["measure_direct"].cpu().numpy(), hD, "measure_direct")
    _same_bits(got["measure_rot"].cpu().numpy(), hD[:, :, 2:8].reshape(T, B, 2, 3), "measure_rot")
    assert np.isfinite(hD).all() and np.abs(hD[..., 2:8]).max() > 0 and np.abs(models - want["models"].cpu().numpy()).max() > 0
    assert np.abs(got["state0"].cpu().numpy() - plain["state0"].cpu().numpy()).max() > 0
    for b in np.flatnonzero(h["end"] >= 0):
        assert (hD[h["end"][b]:, b] == 0).all() and np.abs(hD[:h["end"][b], b]).max() > 0
    for k in plain:
        _same_bits(zero[k].cpu().numpy(), plain[k].cpu().numpy(), k + " with zero cotangents")
    assert (zero["measure_direct"].cpu().numpy() == 0).all()


def test_reverse_walk_with_references(limited):
    """refs=True against backward_device_refs on the augmented seeds plus the folded comRef term: grad_P to the bit, and ref_com / ref_h those of the
    reference VJP on that grad_P"""
    import torch
    c, lib = limited, cm._capi.lib()
    ro, w, h, T, B = c["ro"], c["w"], c["host"], c["T"], c["B"]
    gM, gS, gX = _seeds(c, 22)
    hS, hX, hD = mg.host_vjp(lib, N, h["X"], h["P"], h["S"], h["end"], h["corners"], G, gM, gS, gX)
    got = ro.backward_device_measures(w, gM, gS, gX, refs=True)
    want = ro.backward_device_refs(w, hS, hX)
    zero = ro.backward_device_measures(w, np.zeros_like(gM), gS, gX, refs=True)
    plain = ro.backward_device_refs(w, gS, gX)
    torch.cuda.synchronize()
    assert set(got) == set(want) | {"measure_direct", "measure_rot"}
    gP, models = want["grad_P"].cpu().numpy().copy(), want["models"].cpu().numpy().copy()
    assert lib.cmpc_walk_measures_vjp_fold(N, B, T, mg._ptr(hD), mg._ptr(gP), mg._ptr(models)) == 0
    n_ref = w["tape"]["references"]["knots"]
    rc, rh = torch.zeros((B, n_ref, 3), dtype=torch.float64, device="cuda"), torch.zeros((B, n_ref, 3), dtype=torch.float64, device="cuda")
    ro.solver.reference_from_planner_vjp_device(0, T, w["tape"]["references"], w["end_tick"], _dev(gP), rc, rh)
    torch.cuda.synchronize()
    expect = dict(grad_P=gP, models=models, ref_com=rc.cpu().numpy(), ref_h=rh.cpu().numpy())
    for k in want:
        _same_bits(got[k].cpu().numpy(), expect[k] if k in expect else want[k].cpu().numpy(), k)
    assert np.abs(gP - want["grad_P"].cpu().numpy()).max() > 0 and np.abs(expect["ref_com"] - want["ref_com"].cpu().numpy()).max() > 0
    for k in plain:
        _same_bits(zero[k].cpu().numpy(), plain[k].cpu().numpy(), k + " with zero cotangents")


# ---- 3. the adjoint identity on the device, endings included ----
@pytest.fixture(scope="module")
def ended():
    """the replan of tests/test_gpu_walk_jvp.py: problem 3 ends at tick 2 (code 1) of 5"""
    cfg, B, T = _cfg(), 8, 5
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    push = np.zeros((B, 3)); push[:, 0] = np.linspace(-0.2, 0.2, B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    t[3, 0] += 100.0
    w = ro.walk_device_taped(T, com0, z, z, replan={2: (t, ro.plan[1], ro.plan[2])}, push=push, push_ticks=2)
    assert w["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 2, -1, -1, -1, -1]
    return dict(cfg=cfg, B=B, T=T, ro=ro, w=w)


def test_forward_and_reverse_are_adjoint_on_the_device(ended):
    """forward_sensitivity_device_measures at k = 2 over state0, push and models against backward_device_measures with random cotangents of the
    measures alone: per problem and column sum <gM, dM> equals the contraction of state0, push and models with their directions, within T x ADJ;
    problem 3, ended at tick 2, is included with both sides non-zero"""
    import torch
    from tests.test_gpu_rollout_jvp import _tick_directions
    v = ended
    cfg, B, T, ro, w = v["cfg"], v["B"], v["T"], v["ro"], v["w"]
    rng = np.random.default_rng(31)
    dd = _tick_directions(rng, cfg, B, 2, ro.M)
    d = dict(dir_state0=dd["state"], dir_push=rng.normal(size=(B, 2, 3)).astype(np.float32), dir_models=dd["model"])
    gM = rng.normal(size=(T, B, 4))
    f = ro.forward_sensitivity_device_measures(w, **d)
    r = ro.backward_device_measures(w, gM)
    torch.cuda.synchronize()
    dM = f["measures"].cpu().numpy()
    assert dM.shape == (T, B, 2, 4) and np.isfinite(dM).all() and (dM[2:, 3] == 0).all() and np.abs(dM[:2, 3]).max() > 0
    pairs = (("state0", d["dir_state0"]), ("push", d["dir_push"].astype(np.float64)), ("models", d["dir_models"]))
    rh = {name: r[name].cpu().numpy() for name, _ in pairs}
    worst = 0.0
    for b in range(B):
        for j in range(2):
            lhs = float((gM[:, b] * dM[:, b, j]).sum())
            terms = {name: float((rh[name][b] * x[b, j]).sum()) for name, x in pairs}
            rhs = sum(terms.values())
            gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)
            worst = max(worst, gap)
            print(f"problem {b} column {j}: forward {lhs:.9e}  reverse {rhs:.9e}  gap {gap:.2e}  terms " + " ".join(f"{n} {t:.1e}" for n, t in terms.items()))
            if b == 3:
                assert lhs != 0.0 and rhs != 0.0
    print(f"measures forward against reverse over {T} ticks, worst gap {worst:.2e} (bound {T * ADJ:.1e})")
    assert worst <= T * ADJ


# ---- 4. autograd ----
def test_autograd_layer():
    """loss = -(min over ticks of the margin, NaN rows masked) summed over the batch: .backward() gives state0.grad and push.grad equal to
    backward_device_measures on the same tape, to the bit; forward_ad at k = 1 equals column 0 of a k = 2 call"""
    import torch
    import torch.autograd.forward_ad as fwAD
    cfg, B, T = _cfg(), 4, 6
    com0, dcom0, h0, pushv = _start(B, seed=3)
    s0 = np.concatenate([com0, dcom0, h0], 1).astype(np.float32)
    ro = cm.rollout.WalkingRollout(cfg, B)
    state0 = torch.from_numpy(s0).cuda().requires_grad_(True)
    push = torch.from_numpy(pushv.astype(np.float32)).cuda().requires_grad_(True)
    states, measures = cm.rollout_differentiable_measures(ro, T, state0, push=push, push_ticks=3)
    assert tuple(states.shape) == (T + 1, B, 9) and tuple(measures.shape) == (T, B, 4) and measures.dtype == torch.float32 and ro.limits is None
    margin = measures[:, :, 2]
    masked = torch.where(torch.isnan(margin), torch.full_like(margin, float("inf")), margin)
    loss = -(masked.min(0).values).sum()
    loss.backward()
    torch.cuda.synchronize()
    w = ro.last_walk
    _same_bits(measures.detach().cpu().numpy(), w["measures"].cpu().numpy(), "measures")
    gM = np.zeros((T, B, 4))
    m = masked.detach().cpu().numpy()
    gM[m.argmin(0), np.arange(B), 2] = -1.0
    r = ro.backward_device_measures(w, gM, np.zeros((T + 1, B, 9)))
    torch.cuda.synchronize()
    _same_bits(state0.grad.cpu().numpy(), r["state0"].cpu().numpy().astype(np.float32), "state0.grad")
    _same_bits(push.grad.cpu().numpy(), r["push"].cpu().numpy().astype(np.float32), "push.grad")
    assert float(state0.grad.abs().max()) > 0 and float(push.grad.abs().max()) > 0 and bool(torch.isfinite(state0.grad).all())
    # forward mode
    rng = np.random.default_rng(41)
    t_state, t_push = rng.normal(size=(B, 2, 9)), rng.normal(size=(B, 2, 3)).astype(np.float32)
    ro2 = cm.rollout.WalkingRollout(cfg, B)
    with fwAD.dual_level():
        st, ms = cm.rollout_differentiable_measures(ro2, T, fwAD.make_dual(torch.from_numpy(s0).cuda(), torch.from_numpy(t_state[:, 0].astype(np.float32)).cuda()),
                                                    push=fwAD.make_dual(torch.from_numpy(pushv.astype(np.float32)).cuda(), torch.from_numpy(t_push[:, 0].copy()).cuda()),
                                                    push_ticks=3)
        tan_s, tan_m = fwAD.unpack_dual(st).tangent.clone(), fwAD.unpack_dual(ms).tangent.clone()
    two = ro2.forward_sensitivity_device_measures(ro2.last_walk, dir_state0=t_state.astype(np.float32).astype(np.float64), dir_push=t_push)
    torch.cuda.synchronize()
    _same_bits(tan_m.cpu().numpy(), two["measures"][:, :, 0].to(torch.float32).cpu().numpy(), "the measures' tangent against column 0 at k = 2")
    _same_bits(tan_s.cpu().numpy(), two["states"][:, :, 0].to(torch.float32).cpu().numpy(), "the states' tangent against column 0 at k = 2")
    assert float(tan_m.abs().max()) > 0 and tuple(tan_m.shape) == (T, B, 4)


# ---- 5. no host read ----
def test_nothing_is_read_back(ended):
    """backward_device_measures and forward_sensitivity_device_measures under torch's sync debug mode, after a first call has allocated the workspaces"""
    import torch
    v = ended
    ro, w, T, B = v["ro"], v["w"], v["T"], v["B"]
    rng = np.random.default_rng(51)
    gM, gS = _dev(rng.normal(size=(T, B, 4))), _dev(rng.normal(size=(T + 1, B, 9)))
    ds = _dev(rng.normal(size=(B, 2, 9)))
    ro.backward_device_measures(w, gM, gS, refs=True)
    ro.forward_sensitivity_device_measures(w, dir_state0=ds)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = ro.backward_device_measures(w, gM, gS, refs=True)
        f = ro.forward_sensitivity_device_measures(w, dir_state0=ds)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert np.isfinite(r["state0"].cpu().numpy()).all() and float(r["measure_direct"].abs().max()) > 0 and float(f["measures"].abs().max()) > 0
    assert r["status"].cpu().numpy()[:, 3].tolist() == [0, 0, 6, 6, 6]
