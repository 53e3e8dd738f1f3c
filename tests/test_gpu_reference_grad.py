"""The device walk differentiated in the planner's reference trajectories (include/cmpc.h: cmpc_reference_from_planner_vjp_device / _jvp_device;
WalkingRollout.set_references, backward_device_refs, forward_sensitivity_device_refs, rollout_differentiable(ref_com=, ref_h=)).  Comparisons of bits
throughout -- the kernels against the host forms, the host JVP against the handle's own forward, walk_device against run() with references set, the default
walk before and after, every key of backward_device, an ended problem against the shorter walk it amounts to, autograd against the methods -- but for one
adjoint identity, endings included, held to 5 x ADJ (five chained ticks, the per-tick bound of tests/test_gpu_rollout_jvp.py).  N = 10, dt = 0.06, the
ergoCubGazeboV1 weights."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import reference_grad_ref as rg
from tests.test_gpu_rollout_jvp import ADJ
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_tape import GRADS, _same_bits

pytestmark = pytest.mark.gpu

N, DT, MASS = 10, 0.06, 56.0
NAN = float("nan")


def _cfg():
    return cm.config.ergocub_gazebo_v1(N, DT)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _trajectories(ro, B, n=60, in_dt=0.02, t_first=-0.01, seed=0):
    """a planner's output for a walk of up to 6 ticks: the straight line at the plan's speed with a y sway of 2 cm, its own height (replaced by 0.7 unless
    the test frees it), and a non-zero angular momentum (divided by the mass of 56 kg: about 0.01 in the MPC's units), different per problem"""
    rng = np.random.default_rng(seed)
    t = t_first + in_dt * np.arange(n)
    ph = rng.uniform(0, 2 * np.pi, (B, 1))
    com = np.stack([np.broadcast_to(ro.com_speed * t, (B, n)), 0.02 * np.sin(2 * np.pi * t / 0.96 + ph), 0.7 + 0.005 * np.cos(2 * np.pi * t / 0.48 + ph)], -1)
    h = 0.5 * np.stack([np.sin(2 * np.pi * t / 0.6 + ph), np.cos(2 * np.pi * t / 0.6 + ph), 0.3 * np.sin(2 * np.pi * t / 1.2 + ph)], -1)
    return com.astype(np.float32), h.astype(np.float32), dict(in_dt=in_dt, t_first=t_first, robot_mass=MASS)


# ---- 1. the kernels against the host forms ----
@pytest.mark.parametrize("height", [0.7, NAN], ids=["height", "free_z"])
@pytest.mark.parametrize("B,knots,rows", [(70, 7, 1), (3, 70, 5), (300, 130, 37)])
def test_kernels_match_the_host_forms(B, knots, rows, height):
    """VJP and JVP (k = 3) on the device against the host forms, to the bit: a partial wave of problems' knots, more knots than a workgroup's tile of 128
    (a second tile), more rows than the staging chunk of eight, more than one workgroup; random end ticks with NaN behind the ends, in every entry outside
    the reference rows and (fixed height) in comRef's z entries; a non-zero start value in the VJP's outputs, a NaN sentinel in the JVP's unowned entries"""
    import torch
    cfg = _cfg()
    s, L, lib = cm.BatchSolver(cfg, B), cm.Layout(N), cm._capi.lib()
    tick0, in_dt, t_first, K = 3, (0.02 if knots == 7 else 0.05), 0.25, 3
    rng = np.random.default_rng(B + knots)
    e = rng.integers(-1, tick0 + rows + 2, B).astype(np.int32)
    e[:3] = [-1, tick0 + rows, tick0] if B > 3 else [-1, tick0 + 2, tick0]
    pl = cm._capi.CmpcPlannerRefs(knots, in_dt, t_first, MASS, height)
    inside = np.zeros(L.np, bool)
    inside[L.p_comref:L.p_href + 3 * (N + 1)] = True
    g = rng.normal(size=(rows, B, L.np)).astype(np.float32)
    g[:, :, ~inside] = np.nan
    if height == height:
        g[:, :, L.p_comref + 2:L.p_href:3] = np.nan
    for b in range(B):
        g[rg.admitted_rows(e, b, tick0, rows):, b] = np.nan
    start = rng.normal(size=(2, B, knots, 3))
    hc, hh = start[0].copy(), start[1].copy()
    assert lib.cmpc_reference_from_planner_vjp(N, DT, B, tick0, rows, C.byref(pl), _ptr(e), _ptr(g), _ptr(hc), _ptr(hh)) == 0
    dc, dh = torch.from_numpy(start[0]).cuda(), torch.from_numpy(start[1]).cuda()
    s.reference_from_planner_vjp_device(tick0, rows, pl, torch.from_numpy(e).cuda(), torch.from_numpy(g).cuda(), dc, dh)
    only_c, only_h = torch.from_numpy(start[0]).cuda(), torch.from_numpy(start[1]).cuda()
    s.reference_from_planner_vjp_device(tick0, rows, pl, torch.from_numpy(e).cuda(), torch.from_numpy(g).cuda(), only_c, None)
    s.reference_from_planner_vjp_device(tick0, rows, pl, torch.from_numpy(e).cuda(), torch.from_numpy(g).cuda(), None, only_h)
    torch.cuda.synchronize()
    assert np.isfinite(hc).all() and np.isfinite(hh).all() and np.abs(hc - start[0]).max() > 0 and np.abs(hh - start[1]).max() > 0
    _same_bits(dc, hc, "VJP: grad_com")
    _same_bits(dh, hh, "VJP: grad_h")
    _same_bits(only_c, hc, "VJP: grad_com alone")
    _same_bits(only_h, hh, "VJP: grad_h alone")
    gone = np.array([rg.admitted_rows(e, b, tick0, rows) == 0 for b in range(B)])
    assert gone.any() and (hc[gone] == start[0][gone]).all() and (hh[gone] == start[1][gone]).all()
    # the JVP
    dirs = rng.normal(size=(2, B, K, knots, 3))
    hp = np.full((rows, B, K, L.np), np.nan, np.float32)
    assert lib.cmpc_reference_from_planner_jvp(N, DT, B, tick0, rows, K, C.byref(pl), _ptr(dirs[0]), _ptr(dirs[1]), _ptr(hp)) == 0
    dp = torch.full((rows, B, K, L.np), NAN, dtype=torch.float32, device="cuda")
    s.reference_from_planner_jvp_device(tick0, rows, K, pl, dp, torch.from_numpy(dirs[0]).cuda(), torch.from_numpy(dirs[1]).cuda())
    torch.cuda.synchronize()
    _same_bits(dp, hp, "JVP: dir_p")
    assert np.isnan(hp[..., ~inside]).all() and np.isfinite(hp[..., inside]).all() and np.abs(hp[..., inside]).max() > 0
    if height == height:
        assert (hp[..., L.p_comref + 2:L.p_href:3].view(np.int32) == 0).all()
    s.close()


@pytest.mark.parametrize("height", [0.7, NAN], ids=["height", "free_z"])
def test_host_jvp_is_the_handle_forward(height):
    """float32-valued directions: every entry the host JVP writes is bit-equal to what cmpc_set_reference_from_planner computes with the direction passed as
    the trajectory (robot_mass the same), except comRef's z row under a fixed height, which is +0.0f"""
    cfg = _cfg()
    B, knots, in_dt, t_first, rows, tick0 = 3, 70, 0.05, 0.25, 4, 2
    s, L, lib = cm.BatchSolver(cfg, B), cm.Layout(N), cm._capi.lib()
    rng = np.random.default_rng(9)
    d32 = rng.normal(size=(2, B, knots, 3)).astype(np.float32)
    d64 = d32.astype(np.float64)[:, :, None].copy()       # [2][B][k = 1][knots][3]
    pl = cm._capi.CmpcPlannerRefs(knots, in_dt, t_first, MASS, height)
    hp = np.full((rows, B, 1, L.np), np.nan, np.float32)
    assert lib.cmpc_reference_from_planner_jvp(N, DT, B, tick0, rows, 1, C.byref(pl), _ptr(d64[0]), _ptr(d64[1]), _ptr(hp)) == 0
    n3 = 3 * (N + 1)
    for r in range(rows):
        assert lib.cmpc_set_reference_from_planner(s._h, _ptr(d32[0]), _ptr(d32[1]), knots, in_dt, rg.t_offset(tick0 + r, DT, t_first), MASS, NAN) == 0
        P = np.zeros((B, L.np), np.float32)
        assert lib.cmpc_get_parameters(s._h, _ptr(P)) == 0
        want = P[:, L.p_comref:L.p_comref + 2 * n3].copy()
        if height == height:
            want[:, 2:n3:3] = 0.0
        _same_bits(hp[r, :, 0, L.p_comref:L.p_comref + 2 * n3], want, f"row {r}")
        assert np.abs(want).max() > 0
    s.close()


# ---- 2. the forward walk with references ----
def test_walk_with_references_is_run_with_references():
    """set_references (a y sway of 2 cm, a non-zero h, in_dt = 0.02): walk_device_taped equals run(tape=True) to the bit over 6 ticks at B = 8 -- every
    tick's P (the resampled rows among them), X and state -- and differs from the default walk; after set_references(None) the default walk's bits are
    back"""
    import torch
    cfg = _cfg()
    B, T = 8, 6
    com0, dcom0, h0, push = _start(B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    kw = dict(push=push, push_ticks=3)
    keys = ("X", "P", "states", "info")
    grab = lambda w: {k: w["tape"][k].cpu().numpy().copy() for k in keys}
    w0 = ro.walk_device_taped(T, com0, dcom0, h0, **kw)
    torch.cuda.synchronize()
    t0, refs0 = grab(w0), w0["tape"]["references"]
    assert refs0 == dict(knots=T + N + 2, dt=DT, t_first=0.0, robot_mass=1.0, com_height=0.7)
    com, h, timing = _trajectories(ro, B)
    ro.set_references(com, h, **timing)
    w1 = ro.walk_device_taped(T, com0, dcom0, h0, **kw)
    torch.cuda.synchronize()
    t1 = grab(w1)
    assert w1["tape"]["references"] == dict(knots=60, dt=0.02, t_first=-0.01, robot_mass=MASS, com_height=0.7)
    assert (w1["end_tick"].cpu().numpy() == -1).all() and (w0["end_tick"].cpu().numpy() == -1).all()
    ro_run = cm.rollout.WalkingRollout(cfg, B)
    ro_run.set_references(torch.from_numpy(com).cuda(), torch.from_numpy(h).cuda(), **timing)
    rec = ro_run.run(T, com0, dcom0, h0, record="light", timing=False, tape=True, **kw)
    assert all(rec["merge_ok"]) and len(rec["tape"]["ticks"]) == T
    for i, tk in enumerate(rec["tape"]["ticks"]):
        for k, name in (("X", "X"), ("P", "P"), ("state", "states")):
            _same_bits(t1[name][i], tk[k], f"tick {i}: {k}")
    _same_bits(t1["states"][T], rec["tape"]["state"], "the final state")
    # the references are in P, and they moved the walk
    L = ro.L
    hr = t1["P"][:, :, L.p_href:L.p_href + 3 * (N + 1)]
    assert np.abs(hr).max() > 1e-3 and (t0["P"][:, :, L.p_href:L.p_href + 3 * (N + 1)] == 0).all()
    assert np.abs(t1["P"][:, :, L.p_comref + 1:L.p_href:3]).max() > 1e-3 and (t1["P"][:, :, L.p_comref + 2:L.p_href:3] == np.float32(0.7)).all()
    assert np.abs(t1["states"][T] - t0["states"][T]).max() > 0 and np.abs(t1["X"] - t0["X"]).max() > 0
    ro.set_references(None)
    w2 = ro.walk_device_taped(T, com0, dcom0, h0, **kw)
    torch.cuda.synchronize()
    t2 = grab(w2)
    for k in ("X", "P", "states"):
        _same_bits(t2[k], t0[k], f"the default walk again: {k}")
    assert w2["tape"]["references"] == refs0


# ---- 3, 4: an ended problem, references set ----
@pytest.fixture(scope="module", params=[False, True], ids=["stay", "skip_ended"])
def ended_walk(request):
    """the set-up of tests/test_gpu_walk_jvp.py's ended_walk with references set on every roll-out: problem 3 ends at tick 2 (code 1) of 5 by a replan; the
    same batch without the replan; the 2-tick walk"""
    cfg = _cfg()
    B, T = 8, 5
    com0 = np.tile([0.0, 0.0, 0.7], (B, 1)); z = np.zeros((B, 3))
    push = np.zeros((B, 3)); push[:, 0] = np.linspace(-0.2, 0.2, B)
    ros = [cm.rollout.WalkingRollout(cfg, B) for _ in range(3)]
    com, h, timing = _trajectories(ros[0], B)
    for r in ros:
        r.set_references(com, h, **timing)
    ro, ro_b, ro_2 = ros
    t = ro.plan[0].clone()
    t[3, 0] += 100.0
    kw = dict(push=push, push_ticks=2, skip_ended=request.param)
    w = ro.walk_device_taped(T, com0, z, z, replan={2: (t, ro.plan[1], ro.plan[2])}, **kw)
    base = ro_b.walk_device_taped(T, com0, z, z, **kw)
    two = ro_2.walk_device_taped(2, com0, z, z, **kw)
    assert w["end_tick"].cpu().numpy().tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and int(w["end_code"][3]) == 1
    assert (base["end_tick"].cpu().numpy() == -1).all() and (two["end_tick"].cpu().numpy() == -1).all()
    return dict(cfg=cfg, B=B, T=T, ro=ro, w=w, ro_b=ro_b, base=base, ro_2=ro_2, two=two, com0=com0, kw=kw, refs=(com, h, timing))


def test_reverse_walk_with_reference_gradients(ended_walk):
    """backward_device_refs on the walk problem 3 ends in, NaN in its seeds behind the end: every key backward_device has is bit-equal to it; ref_com /
    ref_h equal the host VJP applied to the returned grad_P, to the bit; the seven others equal the batch without the replan; problem 3 equals the 2-tick
    walk's result and is non-zero; a problem started from a NaN state has exact zeros; with com_height = 0.7 ref_com[..., 2] is exactly zero; rot=True
    leaves ref_* bit-equal"""
    import torch
    v = ended_walk
    cfg, B, T, ro, w = v["cfg"], v["B"], v["T"], v["ro"], v["w"]
    rng = np.random.default_rng(6)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    gS_nan, gX_nan = gS.copy(), gX.copy()
    gS_nan[3:, 3], gX_nan[2:, 3] = np.nan, np.nan
    got = ro.backward_device_refs(w, gS_nan, gX_nan)
    plain = ro.backward_device(w, gS_nan, gX_nan)
    got_rot = ro.backward_device_refs(w, gS_nan, gX_nan, rot=True)
    plain_rot = ro.backward_device_rot(w, gS_nan, gX_nan)
    ref = v["ro_b"].backward_device_refs(v["base"], gS, gX)
    short = v["ro_2"].backward_device_refs(v["two"], gS[:3], gX[:2])
    torch.cuda.synchronize()
    assert set(got) == set(plain) | {"ref_com", "ref_h", "grad_P"} and set(got_rot) == set(plain_rot) | {"ref_com", "ref_h", "grad_P"}
    for k in GRADS:
        _same_bits(got[k], plain[k], f"against backward_device: {k}")
    for k in GRADS + ("plan_rot", "rot", "removed", "list_rot0"):
        _same_bits(got_rot[k], plain_rot[k], f"against backward_device_rot: {k}")
    for k in ("ref_com", "ref_h", "grad_P"):
        _same_bits(got_rot[k], got[k], f"rot=True: {k}")
    h = lambda r: {k: r[k].cpu().numpy() for k in ("ref_com", "ref_h", "grad_P")}
    g, rf, sh = h(got), h(ref), h(short)
    for k in g:
        assert np.isfinite(g[k]).all(), k
    assert g["ref_com"].dtype == np.float64 and g["ref_com"].shape == (B, 60, 3) == g["ref_h"].shape and g["grad_P"].shape == (T, B, ro.L.np)
    # the host form on the returned grad_P
    pl = cm.BatchSolver.planner_refs(**w["tape"]["references"])
    hc, hh = np.zeros((B, 60, 3)), np.zeros((B, 60, 3))
    e = w["end_tick"].cpu().numpy()
    assert cm._capi.lib().cmpc_reference_from_planner_vjp(N, DT, B, 0, T, C.byref(pl), _ptr(e), _ptr(g["grad_P"]), _ptr(hc), _ptr(hh)) == 0
    _same_bits(g["ref_com"], hc, "ref_com against the host VJP of grad_P")
    _same_bits(g["ref_h"], hh, "ref_h against the host VJP of grad_P")
    # ... and against the restatement, for what those bits are worth
    wc, wh, mc, mh, nc, nh = rg.vjp(ro.L, DT, 0, T, 60, 0.02, -0.01, MASS, 0.7, e, g["grad_P"], np.zeros((B, 60, 3)), np.zeros((B, 60, 3)))
    assert (np.abs(g["ref_com"] - wc) <= 4 * (nc + 2) * 2.0 ** -53 * mc).all() and (np.abs(g["ref_h"] - wh) <= 4 * (nh + 2) * 2.0 ** -53 * mh).all()
    others = [0, 1, 2, 4, 5, 6, 7]
    for k in ("ref_com", "ref_h"):
        _same_bits(g[k][others], rf[k][others], f"the others: {k}")
        _same_bits(g[k][3], sh[k][3], f"problem 3 against the 2-tick walk: {k}")
        assert np.abs(g[k][3]).max() > 0 and np.abs(g[k][others]).max() > 0
    _same_bits(g["grad_P"][:, others], rf["grad_P"][:, others], "the others: grad_P")
    _same_bits(g["grad_P"][:2, 3], sh["grad_P"][:, 3], "problem 3: grad_P rows 0 .. 1")
    assert (g["grad_P"][2:, 3] == 0).all()
    assert (g["ref_com"][..., 2] == 0).all() and np.abs(g["ref_com"][..., 1]).max() > 0
    # a problem that never had a finite state
    bad = v["com0"].copy()
    bad[5] = np.nan
    zz = np.zeros((B, 3))
    ro_n = cm.rollout.WalkingRollout(cfg, B)
    ro_n.set_references(v["refs"][0], v["refs"][1], **v["refs"][2])
    wn = ro_n.walk_device_taped(3, bad, zz, zz, **v["kw"])
    gn = ro_n.backward_device_refs(wn, gS[:4], gX[:3])
    torch.cuda.synchronize()
    assert int(wn["end_tick"][5]) == 0 and (np.delete(wn["end_tick"].cpu().numpy(), 5) == -1).all()
    gn = h(gn)
    for k in gn:
        assert np.isfinite(gn[k]).all(), k
    assert (gn["ref_com"][5] == 0).all() and (gn["ref_h"][5] == 0).all() and (gn["grad_P"][:, 5] == 0).all() and np.abs(gn["ref_h"][4]).max() > 0


def test_free_height_has_a_z_gradient():
    """com_height=None: the trajectory's own z row is the reference, and ref_com[..., 2] is no longer zero"""
    import torch
    cfg = _cfg()
    B, T = 4, 3
    com0, dcom0, h0, push = _start(B, seed=2)
    ro = cm.rollout.WalkingRollout(cfg, B)
    com, h, timing = _trajectories(ro, B)
    ro.set_references(com, h, com_height=None, **timing)
    w = ro.walk_device_taped(T, com0, dcom0, h0, push=push, push_ticks=2)
    r = ro.backward_device_refs(w, np.random.default_rng(1).normal(size=(T + 1, B, 9)))
    torch.cuda.synchronize()
    assert np.isnan(w["tape"]["references"]["com_height"]) and (w["end_tick"].cpu().numpy() == -1).all() and (r["status"].cpu().numpy() == 0).all()
    assert float(r["ref_com"][..., 2].abs().max()) > 0 and bool(torch.isfinite(r["ref_com"]).all())


def test_forward_and_reverse_are_adjoint_with_references(ended_walk):
    """forward_sensitivity_device_refs (state0, dir_ref_com, dir_ref_h; k = 2; solutions) against backward_device_refs with random grad_states / grad_X on
    the walk problem 3 ends in: per problem and column sum_i <gS_i, dS_i> + sum_i <gX_i, dX_i> over ALL rows equals the contraction of state0, ref_com,
    ref_h with their directions.  Relative gap <= 5 x ADJ (five chained ticks).  The reference terms are a share of the right-hand side ten times above
    that bound at least (the identity would not see them otherwise), and problem 3 is non-zero on both sides."""
    import torch
    v = ended_walk
    B, T, ro, w = v["B"], v["T"], v["ro"], v["w"]
    rng = np.random.default_rng(12)
    # (the directions' scales are chosen so that the reference terms are well above the bound: a share below it would leave them untested)
    d = dict(dir_state0=0.1 * rng.normal(size=(B, 2, 9)), dir_ref_com=rng.normal(size=(B, 2, 60, 3)), dir_ref_h=MASS * rng.normal(size=(B, 2, 60, 3)))
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    f = ro.forward_sensitivity_device_refs(w, solutions=True, **d)
    r = ro.backward_device_refs(w, gS, gX)
    torch.cuda.synchronize()
    fs, fx = f["states"].cpu().numpy(), f["X"].cpu().numpy().astype(np.float64)
    pairs = (("state0", d["dir_state0"]), ("ref_com", d["dir_ref_com"]), ("ref_h", d["dir_ref_h"]))
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
            share = (abs(terms["ref_com"]) + abs(terms["ref_h"])) / sum(abs(t) for t in terms.values())
            print(f"problem {b} column {j}: forward {lhs:.9e}  reverse {rhs:.9e}  gap {gap:.2e}  reference share {share:.2e}  terms "
                  + " ".join(f"{n} {t:.1e}" for n, t in terms.items()))
            assert terms["ref_com"] != 0.0 and terms["ref_h"] != 0.0 and share > 10 * 5 * ADJ
            if b == 3:
                assert lhs != 0.0 and rhs != 0.0
    print(f"forward walk against reverse walk with references over {T} ticks, worst gap over {B} problems x 2 columns: {worst:.2e} (bound {5 * ADJ:.1e})")
    assert worst <= 5 * ADJ


# ---- 5. autograd ----
def test_autograd_with_reference_trajectories():
    """rollout_differentiable(device_walk=True, ref_com=, ref_h=) at B = 4, 6 ticks: .grad is bit-equal to backward_device_refs, the forward_ad tangent to
    the k = 1 column of forward_sensitivity_device_refs; with problem 1 ended by a replan at tick 2 the others keep their bits and everything is finite"""
    import torch
    import torch.autograd.forward_ad as fwAD
    cfg = _cfg()
    B, T = 4, 6
    com0, dcom0, h0, pushv = _start(B, seed=3)
    s0 = np.concatenate([com0, dcom0, h0], 1).astype(np.float32)
    com, h, timing = _trajectories(cm.rollout.WalkingRollout(cfg, B), B)
    rng = np.random.default_rng(8)
    gout = torch.from_numpy(rng.normal(size=(T + 1, B, 9)).astype(np.float32)).cuda()
    t_com, t_h = torch.from_numpy(rng.normal(size=(B, 60, 3))).cuda(), torch.from_numpy(MASS * rng.normal(size=(B, 60, 3))).cuda()

    def reverse(**kw):
        ro = cm.rollout.WalkingRollout(cfg, B)
        ro.set_references(np.zeros_like(com), np.zeros_like(h), **timing)      # (the timing is the installed one; the trajectories are this call's)
        state0, push = torch.from_numpy(s0).cuda().requires_grad_(), torch.from_numpy(pushv.astype(np.float32)).cuda()
        rc = torch.from_numpy(com.astype(np.float64)).cuda().requires_grad_()
        rh = torch.from_numpy(h.astype(np.float64)).cuda().requires_grad_()
        states = cm.rollout_differentiable(ro, T, state0, push=push, push_ticks=3, device_walk=True, ref_com=rc, ref_h=rh, **kw)
        states.backward(gout)
        torch.cuda.synchronize()
        return ro, states.detach(), state0.grad, rc.grad, rh.grad
    ro, st, g0, gc, gh = reverse()
    assert (ro.last_walk["end_tick"].cpu().numpy() == -1).all() and gc.dtype == torch.float64 and tuple(gc.shape) == (B, 60, 3)
    direct = ro.backward_device_refs(ro.last_walk, gout.to(torch.float64))
    torch.cuda.synchronize()
    _same_bits(gc, direct["ref_com"], "ref_com.grad")
    _same_bits(gh, direct["ref_h"], "ref_h.grad")
    _same_bits(g0, direct["state0"].to(torch.float32), "state0.grad")
    assert bool(gc[..., :2].any()) and bool(gh.any()) and not bool(gc[..., 2].any())
    # the call's trajectories were used, not the installed zeros: the same walk as with them installed
    ro_i = cm.rollout.WalkingRollout(cfg, B)
    ro_i.set_references(com, h, **timing)
    wi = ro_i.walk_device_taped(T, com0.astype(np.float32), dcom0.astype(np.float32), h0.astype(np.float32), push=pushv, push_ticks=3, trace=False)
    torch.cuda.synchronize()
    _same_bits(st, wi["tape"]["states"], "the states against the walk with the trajectories installed")
    assert ro.references is not None and not bool(ro.references["com"].any()) and ro._ref_override is None
    # forward mode
    ro_f = cm.rollout.WalkingRollout(cfg, B)
    ro_f.set_references(np.zeros_like(com), np.zeros_like(h), **timing)
    with fwAD.dual_level():
        rc = fwAD.make_dual(torch.from_numpy(com.astype(np.float64)).cuda(), t_com)
        rh = fwAD.make_dual(torch.from_numpy(h.astype(np.float64)).cuda(), t_h)
        states = cm.rollout_differentiable(ro_f, T, torch.from_numpy(s0).cuda(), push=torch.from_numpy(pushv.astype(np.float32)).cuda(), push_ticks=3,
                                           device_walk=True, ref_com=rc, ref_h=rh)
        primal, tan = fwAD.unpack_dual(states)
        assert tan is not None and tan.dtype == torch.float32 and tuple(tan.shape) == (T + 1, B, 9)
        primal, tan = primal.clone(), tan.clone()
    col = ro_f.forward_sensitivity_device_refs(ro_f.last_walk, dir_ref_com=t_com[:, None].contiguous(), dir_ref_h=t_h[:, None].contiguous())
    torch.cuda.synchronize()
    _same_bits(primal, st, "the forward-mode primal")
    _same_bits(tan, col["states"][:, :, 0].to(torch.float32), "the tangent against forward_sensitivity_device_refs' column")
    assert bool(tan[1:].any()) and not bool(tan[0].any()) and (ro_f.last_forward["status"].cpu().numpy() == 0).all()
    # one problem ended by a replan
    plan = cm.rollout.WalkingRollout(cfg, B).plan
    t = plan[0].clone()
    t[1, 0] += 100.0
    ro_e, st_e, g0_e, gc_e, gh_e = reverse(replan={2: (t, plan[1], plan[2])})
    assert ro_e.last_walk["end_tick"].cpu().numpy().tolist() == [-1, 2, -1, -1]
    others = [0, 2, 3]
    _same_bits(gc_e[others], gc[others], "the others: ref_com.grad")
    _same_bits(gh_e[others], gh[others], "the others: ref_h.grad")
    _same_bits(g0_e[others], g0[others], "the others: state0.grad")
    for a in (gc_e, gh_e, g0_e):
        assert bool(torch.isfinite(a).all())
    assert bool(gc_e[1].any()) and (ro_e.last_backward["status"][:, 1].cpu().numpy() == [0, 0, 6, 6, 6, 6]).all()


# ---- 6. no host read ----
def test_nothing_is_read_back():
    """walk_device_taped + backward_device_refs + forward_sensitivity_device_refs under torch's sync debug mode, after a first call has allocated the
    workspaces"""
    import torch
    cfg = _cfg()
    B, T = 8, 6
    com0, dcom0, h0, push = _start(B)
    ro = cm.rollout.WalkingRollout(cfg, B)
    com, h, timing = _trajectories(ro, B)
    ro.set_references(com, h, **timing)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ro.dev)
    rng = np.random.default_rng(5)
    gS, gX = cu(rng.normal(size=(T + 1, B, 9))), cu((1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32))
    d = dict(dir_state0=cu(rng.normal(size=(B, 2, 9))), dir_ref_com=cu(rng.normal(size=(B, 2, 60, 3))), dir_ref_h=cu(rng.normal(size=(B, 2, 60, 3))))
    ins = [cu(np.asarray(a, np.float32)) for a in (com0, dcom0, h0, push)]
    t = ro.plan[0].clone()
    kw = dict(push=ins[3], push_ticks=2, replan={3: (t, ro.plan[1], ro.plan[2])}, skip_ended=True)

    def once():
        w = ro.walk_device_taped(T, ins[0], ins[1], ins[2], **kw)
        return w, ro.backward_device_refs(w, gS, gX), ro.forward_sensitivity_device_refs(w, solutions=True, **d)
    once()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w, r, f = once()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert (w["end_tick"].cpu().numpy() == -1).all() and (r["status"].cpu().numpy() == 0).all() and (f["status"].cpu().numpy() == 0).all()
    assert w["tape"]["segments"] == [0, 3] and float(r["ref_com"].abs().max()) > 0 and float(r["ref_h"].abs().max()) > 0
    assert bool(torch.isfinite(f["states"]).all()) and float(f["states"][-1].abs().max()) > 0
