"""GPU: the plant-model mismatch on the device walk (include/cmpc.h, "plant-model mismatch on the device walk"; DESIGN.md 7f, "Mismatch"): hidden pushes the
MPC is not told about, noise on the state it measures, a gain on the forces the plant applies -- the plant kernel and its VJP against the float64
restatement tests/mismatch_ref.py, and everything above them as comparisons of bits: one call of the walk against the ticks composed by hand and against
the tick entry point, off against the entry points that existed, a NaN push that ends one problem alone, a fork of one snapshot under B pushes against the
unbroken walks, the reverse walk against the tick VJPs chained by hand through the gate, an ended problem against the shorter walk, autograd.
N = 10, dt = 0.06, the ergoCubGazeboV1 weights, B = 8, 6 ticks unless stated.  Hand-made problems hold the two 0.001 thresholds of the ZMP and gain = 0
(THRESHOLD_CASES).  No contact changes within 6 ticks: tests/test_gpu_mismatch_long.py walks 18 with the helpers defined here."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import mismatch_ref as mr
from tests import rollout_adjoint_ref as rar
from tests.test_gpu_rollout_adjoint import REF, _plant_inputs, _rel
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_tape import GRADS, _same_bits

pytestmark = pytest.mark.gpu

N, B, T = 10, 8, 6
NEW = ("hidden_wrench", "state_noise", "force_gain")
TAPE_KEYS = ("X", "P", "lam_g", "states", "ok", "land", "plan_t", "list_t", "plan_n", "list_n")
REC_KEYS = ("com", "zmp", "land", "landing_offset", "iterations", "code", "end_tick", "end_code", "iterations_sum", "iterations_max", "final_state",
            "box_slack_min", "stats", "X", "P", "state")


def _cfg():
    return cm.config.ergocub_gazebo_v1(N, 0.06)


def _mismatch(batch=B, hidden_ticks=3, noise_ticks=2, tick_first=1, seed=31):
    """all three: pushes of about 0.3 m/s^2 (17 N on the 56 kg robot) and 0.05 N m / kg, a centimetre-scale estimator error, gains in [0.9, 1.1]"""
    rng = np.random.default_rng(seed)
    hidden = np.concatenate([rng.normal(0, 0.3, (hidden_ticks, batch, 3)), rng.normal(0, 0.05, (hidden_ticks, batch, 3))], -1).astype(np.float32)
    noise = np.concatenate([rng.normal(0, 3e-3, (noise_ticks, batch, 3)), rng.normal(0, 1e-2, (noise_ticks, batch, 3)),
                            rng.normal(0, 2e-3, (noise_ticks, batch, 3))], -1).astype(np.float32)
    gain = rng.uniform(0.9, 1.1, batch).astype(np.float32)
    return dict(hidden_wrench=hidden, state_noise=noise, force_gain=gain, tick_first=tick_first)


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


# ---- 1. the plant kernel against the restatement ----
def test_plant_kernel_matches_the_restatement():
    """B = 300 (two workgroups, a partial wave), gains in [0.8, 1.25], pushes that move the state, one foot of every third problem off: state and ZMP within
    2e-6 of the restatement (the bound tests/test_gpu_next_rows.py holds the plant to); both pointers NULL, and gain = 1 with an all-zero wrench, are
    cmpc_plant_step_device to the bit"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    L, nb, step, nsub = cm.Layout(N), 300, 0.01, 6
    X, P, state, _ = _plant_inputs(cfg, nb, 12)
    rng = np.random.default_rng(13)
    gain = rng.uniform(0.8, 1.25, nb).astype(np.float32)
    hidden = np.concatenate([rng.normal(0, 0.5, (nb, 3)), rng.normal(0, 0.1, (nb, 3))], 1).astype(np.float32)
    s = cm.BatchSolver(cfg, nb)
    dX, dP, dS = _cu(X), _cu(P), _cu(state)
    got_s, got_z = s.plant_step_mismatch_device(dX, dP, dS, step=step, substeps=nsub, hidden_wrench=_cu(hidden), force_gain=_cu(gain))
    only_h = s.plant_step_mismatch_device(dX, dP, dS, step=step, substeps=nsub, hidden_wrench=_cu(hidden))
    only_g = s.plant_step_mismatch_device(dX, dP, dS, step=step, substeps=nsub, force_gain=_cu(gain))
    plain = s.plant_step_device(dX, dP, dS, step=step, substeps=nsub)
    null = s.plant_step_mismatch_device(dX, dP, dS, step=step, substeps=nsub)
    unit = s.plant_step_mismatch_device(dX, dP, dS, step=step, substeps=nsub, hidden_wrench=_cu(np.zeros((nb, 6), np.float32)),
                                        force_gain=_cu(np.ones(nb, np.float32)))
    torch.cuda.synchronize()
    corners = np.asarray([c.corners for c in cfg.contacts], np.float64).astype(np.float32).astype(np.float64)
    kw = dict(gravity=float(np.float32(rar.GRAVITY)))
    worst = dict(state=0.0, zmp=0.0, moved=0.0)
    for name, (gs, gz), hh, gg in (("both", (got_s, got_z), hidden, gain), ("hidden", only_h, hidden, None), ("gain", only_g, None, gain)):
        gs, gz = _h(gs), _h(gz)
        for b in range(nb):
            ref_s, ref_z = mr.plant_step(L, corners, X[b], P[b], state[b], float(np.float32(step)), nsub, None if hh is None else hh[b],
                                         1.0 if gg is None else float(gg[b]), **kw)
            worst["state"] = max(worst["state"], float(np.abs(gs[b] - ref_s).max()))
            both_nan = np.isnan(gz[b]) & np.isnan(ref_z)
            worst["zmp"] = max(worst["zmp"], float(np.abs(np.where(both_nan, 0.0, gz[b] - ref_z)).max()))
            assert (np.isnan(gz[b]) == np.isnan(ref_z)).all()
    worst["moved"] = float(np.abs(_h(got_s) - _h(plain[0])).max())
    print(f"\nmismatched plant kernel, B = {nb}: state gap {worst['state']:.2e}, ZMP gap {worst['zmp']:.2e} (bound 2e-6); the mismatch moved the state by "
          f"{worst['moved']:.2e}")
    assert worst["state"] <= 2e-6 and worst["zmp"] <= 2e-6
    assert worst["moved"] > 1e-3                      # the check sees the mismatch
    for a, b_, what in ((null, plain, "both NULL"), (unit, plain, "gain 1, zero wrench")):
        _same_bits(a[0], b_[0], what + ": state")
        _same_bits(a[1], b_[1], what + ": zmp")
    assert not np.array_equal(_h(only_h[0]), _h(only_g[0]))


# ---- 1b. the two 0.001 thresholds of the ZMP see the APPLIED force ----
G2 = 9.80665 / 2
# (F_z of the left foot, of the right foot, the contact flags, the gain) as the MPC gives them; each side of 0.001 is at least 10 % away before and after the
# gain (0.0008 * 1.5 = 0.0012, 0.0012 * 0.7 = 0.00084, 0.0006 * 1.5 = 0.0009), so that float32 and float64 agree on the side
THRESHOLD_CASES = [
    (0.0008, G2, (1, 1), 1.5), (0.0012, G2, (1, 1), 0.7),            # the gain puts the left foot into the ZMP / takes it out, beside a loaded right foot
    (0.01, 0.0008, (1, 1), 1.5), (0.01, 0.0012, (1, 1), 0.7),        # the same for the right foot, beside a left foot that hardly outweighs it
    (0.0008, 0.0008, (1, 1), 1.5), (0.0012, 0.0012, (1, 1), 0.7),    # ztot across 0.001: the ZMP appears / turns NaN
    (G2, 0.0008, (0, 1), 1.5), (0.0012, G2, (1, 0), 0.7),            # ztot across 0.001 on one foot, the loaded one gated off
    (G2, G2, (1, 1), 0.0), (G2, G2, (0, 1), 0.0), (G2, G2, (1, 0), 0.0),      # gain = 0: NaN ZMP, free fall plus the external wrenches
    (0.0006, 0.0006, (1, 1), 1.5),                                   # neither foot reaches 0.001 though their sum does: NaN with and without the gain
]
THRESHOLD_IN = [(1, 1), (0, 1), (1, 1), (1, 0), (1, 1), (0, 0), (0, 1), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)]       # feet in the ZMP under the gain
THRESHOLD_IN_PLAIN = [(0, 1), (1, 1), (1, 0), (1, 1), (0, 0), (1, 1), (0, 0), (1, 0), (1, 1), (0, 1), (1, 0), (0, 0)]   # ... and without it


def _threshold_problems(cfg, seed=23):
    """_plant_inputs' geometry, wrenches and states with the knot-0 forces of THRESHOLD_CASES: a foot's F_z spread unevenly over its corners (so that the local
    ZMP is off-centre), lateral forces a fifth of it -> float32 (X, P, state, models, hidden[12, 6], gain[12])"""
    L, nb = cm.Layout(cfg.N), len(THRESHOLD_CASES)
    X, P, state, models = _plant_inputs(cfg, nb, seed)
    share = np.array([0.4, 0.3, 0.2, 0.1])
    for b, (fz0, fz1, gam, _) in enumerate(THRESHOLD_CASES):
        for c, fz in enumerate((fz0, fz1)):
            P[b, L.p_gam[c]] = float(gam[c])
            for j in range(4):
                X[b, L.f[c][j]:L.f[c][j] + 3] = np.float32(fz * share[j]) * np.array([0.2, -0.1, 1.0], np.float32)
    rng = np.random.default_rng(seed + 1)
    hidden = np.concatenate([rng.normal(0, 0.5, (nb, 3)), rng.normal(0, 0.1, (nb, 3))], 1).astype(np.float32)
    return X, P, state, models, hidden, np.array([c[3] for c in THRESHOLD_CASES], np.float32)


def test_plant_thresholds_see_the_applied_force():
    """12 hand-made problems (THRESHOLD_CASES) whose gain decides F_z > 0.001 of a foot or ztot > 0.001: state and ZMP within 2e-6 of the restatement (the
    bound of test_plant_kernel_matches_the_restatement), the ZMP's NaN pattern identical; the restatement takes the branches written down by hand, and -- in
    the 11 problems that are pairs -- the plain plant takes the other one, on the device too; gain = 0 is free fall under the two wrenches, closed form"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    L, nb, step, nsub = cm.Layout(N), len(THRESHOLD_CASES), 0.01, 6
    X, P, state, _, hidden, gain = _threshold_problems(cfg)
    s = cm.BatchSolver(cfg, nb)
    dX, dP, dS = _cu(X), _cu(P), _cu(state)
    got_s, got_z = (_h(a) for a in s.plant_step_mismatch_device(dX, dP, dS, step=step, substeps=nsub, hidden_wrench=_cu(hidden), force_gain=_cu(gain)))
    pl_s, pl_z = (_h(a) for a in s.plant_step_mismatch_device(dX, dP, dS, step=step, substeps=nsub, hidden_wrench=_cu(hidden)))
    torch.cuda.synchronize()
    corners = np.asarray([c.corners for c in cfg.contacts], np.float64).astype(np.float32).astype(np.float64)
    kw = dict(gravity=float(np.float32(rar.GRAVITY)))
    worst = dict(state=0.0, zmp=0.0, plain_state=0.0, plain_zmp=0.0, free_fall=0.0)
    for b in range(nb):
        feet, defined, margin = mr.zmp_branches(L, corners, X[b], P[b], float(gain[b]))
        feet_p, defined_p, margin_p = mr.zmp_branches(L, corners, X[b], P[b], 1.0)
        assert feet == tuple(map(bool, THRESHOLD_IN[b])) and feet_p == tuple(map(bool, THRESHOLD_IN_PLAIN[b])), (b, feet, feet_p)
        assert defined == any(feet) and defined_p == any(feet_p)
        assert margin >= 0.1 and margin_p >= 0.1, (b, margin, margin_p)
        if b < 11:
            assert feet != feet_p, b                   # the plain plant takes the other branch
        for name, gs, gz, gg in (("", got_s, got_z, float(gain[b])), ("plain_", pl_s, pl_z, 1.0)):
            ref_s, ref_z = mr.plant_step(L, corners, X[b], P[b], state[b], float(np.float32(step)), nsub, hidden[b], gg, **kw)
            assert (np.isnan(gz[b]) == np.isnan(ref_z)).all() and np.isnan(ref_z).all() == (not (defined if name == "" else defined_p)), (b, name, gz[b], ref_z)
            worst[name + "state"] = max(worst[name + "state"], float(np.abs(gs[b] - ref_s).max()))
            worst[name + "zmp"] = max(worst[name + "zmp"], float(np.abs(np.where(np.isnan(ref_z), 0.0, gz[b] - ref_z)).max()))
        if b < 11:      # ... on the device too: the ZMP with the gain is not the ZMP without it
            assert not np.array_equal(got_z[b], pl_z[b], equal_nan=True), b
        if gain[b] == 0.0:
            fall = mr.free_fall(state[b], P[b, L.p_fext:L.p_fext + 3].astype(np.float64) + hidden[b, :3], P[b, L.p_text:L.p_text + 3].astype(np.float64) + hidden[b, 3:],
                                nsub * float(np.float32(step)), **kw)
            worst["free_fall"] = max(worst["free_fall"], float(np.abs(got_s[b] - fall).max()))
    print("\nthreshold problems: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + " (bound 2e-6)")
    assert max(worst.values()) <= 2e-6, worst


def test_plant_vjp_kernel_at_the_thresholds_and_gain_zero():
    """the 12 threshold problems through cmpc_plant_step_vjp_mismatch_device against the restatement within REF; at gain = 0 grad_x is exactly zero on the
    forces (and everywhere: no force is applied, so no position or corner has a lever arm) and grad_gain is not"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    L, nb, step, nsub = cm.Layout(N), len(THRESHOLD_CASES), 0.01, 6
    X, P, state, models, hidden, gain = _threshold_problems(cfg)
    g = np.random.default_rng(10).normal(size=(nb, 9))
    s = cm.BatchSolver(cfg, nb)
    s.set_models(models)
    r = s.plant_step_vjp_mismatch_device(_cu(X), _cu(P), _cu(state), _cu(g), step=step, substeps=nsub, hidden_wrench=_cu(hidden), force_gain=_cu(gain))
    torch.cuda.synchronize()
    got = {k: _h(v) for k, v in r.items() if v is not None}
    xi, _ = rar.plant_columns(L)
    worst = {k: 0.0 for k in ("state", "x", "p", "model", "hidden", "gain")}
    for b in range(nb):
        corners = models[b, 10:].astype(np.float32).astype(np.float64)
        ref = mr.plant_vjp(L, corners, X[b], P[b], state[b], float(np.float32(step)), nsub, g[b], hidden[b], float(gain[b]), gravity=float(np.float32(rar.GRAVITY)))
        for k, v in zip(("state", "x", "p", "model", "hidden"), ref[:5]):
            if np.abs(v).max() == 0:       # (a group without a gradient: exact zeros are asked for, not a ratio)
                assert not got[k][b].any(), (b, k)
                continue
            worst[k] = max(worst[k], _rel(got[k][b], v))
        worst["gain"] = max(worst["gain"], abs(got["gain"][b] - ref[5]) / max(abs(ref[5]), 1e-300))
        assert np.abs(ref[4]).max() > 0 and ref[5] != 0
        if gain[b] == 0.0:
            assert not got["x"][b][xi[6:]].any() and not ref[1][xi[6:]].any() and got["gain"][b] != 0, b
    print("\nthreshold problems, plant VJP: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {REF:.0e})")
    assert max(worst.values()) <= REF, worst


# ---- 2. the plant VJP ----
def test_plant_vjp_kernel_matches_the_restatement():
    """every output of cmpc_plant_step_vjp_mismatch_device against the restatement within REF (relative to the group's largest entry), with the rotation
    output on and off; with both inputs NULL the shared outputs are cmpc_plant_step_vjp_rot_device's to the bit"""
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    L, nb, step, nsub = cm.Layout(N), 16, 0.01, 6
    X, P, state, models = _plant_inputs(cfg, nb, 4)
    rng = np.random.default_rng(9)
    g = rng.normal(size=(nb, 9))
    gain = rng.uniform(0.8, 1.25, nb).astype(np.float32)
    hidden = np.concatenate([rng.normal(0, 0.5, (nb, 3)), rng.normal(0, 0.1, (nb, 3))], 1).astype(np.float32)
    s = cm.BatchSolver(cfg, nb)
    s.set_models(models)
    dX, dP, dS, dg = _cu(X), _cu(P), _cu(state), _cu(g)
    r = s.plant_step_vjp_mismatch_device(dX, dP, dS, dg, step=step, substeps=nsub, hidden_wrench=_cu(hidden), force_gain=_cu(gain), grad_rot=True)
    r_norot = s.plant_step_vjp_mismatch_device(dX, dP, dS, dg, step=step, substeps=nsub, hidden_wrench=_cu(hidden), force_gain=_cu(gain))
    null = s.plant_step_vjp_mismatch_device(dX, dP, dS, dg, step=step, substeps=nsub, grad_rot=True)
    old = s.plant_step_vjp_device(dX, dP, dS, dg, step=step, substeps=nsub, grad_rot=True)
    torch.cuda.synchronize()
    worst = {k: 0.0 for k in ("state", "x", "p", "model", "hidden", "gain")}
    got = {k: _h(v) for k, v in r.items() if v is not None}
    for b in range(nb):
        corners = models[b, 10:].astype(np.float32).astype(np.float64)
        ref = mr.plant_vjp(L, corners, X[b], P[b], state[b], float(np.float32(step)), nsub, g[b], hidden[b], float(gain[b]),
                           gravity=float(np.float32(rar.GRAVITY)))
        for k, v in zip(("state", "x", "p", "model", "hidden"), ref[:5]):
            worst[k] = max(worst[k], _rel(got[k][b], v))
        worst["gain"] = max(worst["gain"], abs(got["gain"][b] - ref[5]) / max(abs(ref[5]), 1e-300))
        assert np.abs(ref[4]).max() > 0 and ref[5] != 0
    print("\nmismatched plant VJP against the restatement: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {REF:.0e})")
    assert max(worst.values()) <= REF, worst
    for k in ("state", "x", "p", "model", "hidden", "gain"):
        _same_bits(r[k], r_norot[k], f"rotation output on / off: {k}")
    for k, v in zip(("state", "x", "p", "model", "rot0"), old):
        _same_bits(null[k], v, f"both inputs NULL: {k}")
    # the gradient of a wrench that was not added is the plant's own on fExt_0 / tauExt_0 (float32 there)
    gp = _h(null["p"])
    np.testing.assert_array_equal(_h(null["hidden"]).astype(np.float32), np.concatenate([gp[:, L.p_fext:L.p_fext + 3], gp[:, L.p_text:L.p_text + 3]], 1))


# ---- the two compositions of a mismatched walk out of its steps, shared with tests/test_gpu_mismatch_long.py ----
def _sched_row(sched, mm, i):
    """row of tick i of a schedule (numpy or CUDA, or None) under mm's tick_first, None outside it"""
    r = i - mm.get("tick_first", 0)
    return sched[r] if sched is not None and 0 <= r < sched.shape[0] else None


def _step_buffers(make_ro, start, ticks):
    import torch
    ro = make_ro()
    L, nb = ro.L, ro.B
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=ro.dev)
    state = _cu(np.concatenate(start, 1).astype(np.float32))
    return ro, z((nb, L.np)), z((nb, L.nx)), z((nb, L.nx)), z((nb, 8)), state, ro._planner_refs(ticks)


def _steps_by_hand(make_ro, start, mm, ticks, tape):
    """a walk of `ticks` ticks under mm composed by hand on a fresh roll-out of make_ro() -- merge, sample, the references, setState of state + noise added
    by torch in float32, cold start / shift, solve, adjust, cmpc_plant_step_mismatch_device -- against the tape's P, X and states, to the bit"""
    hidden, noise, gain = (None if mm.get(k) is None else _cu(mm[k]) for k in ("hidden_wrench", "state_noise", "force_gain"))
    ro, dP, dX0, dX, dInfo, state, refs = _step_buffers(make_ro, start, ticks)
    s, dt = ro.solver, ro.cfg.sampling_time
    kw = dict(step=dt / ro.substeps, substeps=ro.substeps)
    prev = None
    for i in range(ticks):
        now = i * dt
        lists = tuple(a.clone() for a in ro.plan) if prev is None else s.contacts_merge_device(now, ro.plan, prev)[0]
        land = s.contacts_sample_device(now, lists, dP)
        s.write_reference_from_planner_device(refs[0], refs[1], refs[2], now - refs[3], refs[4], refs[5], dP)
        nz = _sched_row(noise, mm, i)
        s.write_state_device(state if nz is None else state + nz, dP, None)
        if prev is None:
            s.cold_start_device(dP, dX0)
        else:
            s.shift_solution_device(dX, dX0)
        s.solve_device(dP, dX0, dX, dInfo, warm=prev is not None)
        s.contacts_adjust_device(now, dX, land, lists)
        _same_bits(tape["states"][i], state, f"by hand, tick {i}: the state the tick started from")
        state, _ = s.plant_step_mismatch_device(dX, dP, state, hidden_wrench=_sched_row(hidden, mm, i), force_gain=gain, **kw)
        _same_bits(tape["P"][i], dP, f"by hand, tick {i}: P")
        _same_bits(tape["X"][i], dX, f"by hand, tick {i}: X")
        _same_bits(tape["states"][i + 1], state, f"by hand, tick {i}: the state it left")
        prev = lists


def _steps_by_tick_entry(make_ro, start, mm, ticks, tape):
    """the same walk through cmpc_rollout_tick_mismatch_device called tick by tick, against the tape's P, X and states, to the bit
    -> (the roll-out, its solver, the plant_mismatch dict it walked under)"""
    import torch
    ro, dP, dX0, dX, dInfo, state, refs = _step_buffers(make_ro, start, ticks)
    s, dt, nb = ro.solver, ro.cfg.sampling_time, ro.B
    kw = dict(step=dt / ro.substeps, substeps=ro.substeps)
    mmc = s.plant_mismatch(**mm)
    ok, land, zmp = torch.ones((nb,), dtype=torch.int32, device=ro.dev), torch.zeros((nb, 2), dtype=torch.int32, device=ro.dev), torch.zeros((nb, 2), device=ro.dev)
    sets, cur = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)], 0
    for i in range(ticks):
        now = i * dt
        planner = (refs[0], refs[1], refs[2], now - refs[3], refs[4], refs[5])
        if i == 0:
            s.contacts_sample_device(now, sets[0], dP)
            s.write_state_device(state, dP, None)
            s.cold_start_device(dP, dX0)
            prv, lists = None, sets[0]
        else:
            prv, lists = sets[cur], sets[1 - cur]
            cur = 1 - cur
        s.rollout_tick_mismatch_device(i, mmc, now, ro.plan, prv, lists, ok, land, state, None, dP, dX0, dX, dInfo, state, zmp, i > 0, planner=planner, **kw)
        _same_bits(tape["P"][i], dP, f"tick entry, tick {i}: P")
        _same_bits(tape["X"][i], dX, f"tick entry, tick {i}: X")
        _same_bits(tape["states"][i + 1], state, f"tick entry, tick {i}: state")
    return ro, s, mmc


# ---- 3 .. 5, 7, 8: one walk of 6 ticks under all three, taped, and the same walk plain ----
@pytest.fixture(scope="module")
def walk6():
    import torch
    cfg = _cfg()
    com0, dcom0, h0, _ = _start(B)
    mm = _mismatch()
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(T, com0, dcom0, h0, mismatch=mm)
    ro_p = cm.rollout.WalkingRollout(cfg, B)
    plain = ro_p.walk_device_taped(T, com0, dcom0, h0)
    rng = np.random.default_rng(2)
    gS = _cu(rng.normal(size=(T + 1, B, 9)))
    got = ro.backward_device(w, gS)
    torch.cuda.synchronize()
    return dict(cfg=cfg, start=(com0, dcom0, h0), mm=mm, ro=ro, w=w, ro_p=ro_p, plain=plain, gS=gS, got=got)


def test_one_call_is_the_steps(walk6):
    """walk_device under all three (tick_first = 1, three rows of pushes, two of noise) over 6 ticks, in every tick's P, X and state: against the ticks
    composed by hand -- merge, sample, the references, setState of state + noise added by torch in float32, cold start / shift, solve, adjust,
    cmpc_plant_step_mismatch_device -- and against cmpc_rollout_tick_mismatch_device called tick by tick, to the bit.  The com0 rows of P differ from the
    true state exactly on ticks 1 and 2; no wrench row of P differs from the plain walk's input (zero: nobody told the MPC); the final state differs from
    the plain walk's."""
    import torch
    cfg, mm, w = walk6["cfg"], walk6["mm"], walk6["w"]
    L, dt = cm.Layout(N), cfg.sampling_time
    com0, dcom0, h0 = walk6["start"]
    tape = w["tape"]
    untaped = cm.rollout.WalkingRollout(cfg, B).walk_device_mismatch(T, com0, dcom0, h0, mm)
    make_ro = lambda: cm.rollout.WalkingRollout(cfg, B)
    _steps_by_hand(make_ro, walk6["start"], mm, T, tape)
    ro, s, mmc = _steps_by_tick_entry(make_ro, walk6["start"], mm, T, tape)
    hidden = _cu(mm["hidden_wrench"])
    torch.cuda.synchronize()
    for k in REC_KEYS:
        _same_bits(untaped[k], w[k], f"untaped against taped: {k}")
    P, states = _h(tape["P"]), _h(tape["states"])
    differs = [bool((P[i][:, L.p_com0:L.p_com0 + 9] != states[i]).any()) for i in range(T)]
    assert differs == [False, True, True, False, False, False], differs
    _same_bits(P[1][:, L.p_com0:L.p_com0 + 9], states[1] + mm["state_noise"][0], "the measured state is one float32 add")
    Pp = _h(walk6["plain"]["tape"]["P"])
    for i in range(T):
        _same_bits(P[i][:, L.p_fext:L.p_fext + 6 * N], Pp[i][:, L.p_fext:L.p_fext + 6 * N], f"tick {i}: the wrench rows of P")
    assert not P[:, :, L.p_fext:L.p_fext + 6 * N].any()
    moved = np.abs(_h(w["state"]) - _h(walk6["plain"]["state"])).max(1)
    print(f"\nthe mismatch moved the final states by {moved.min():.2e} .. {moved.max():.2e}")
    assert (moved > 1e-4).all() and (_h(w["end_tick"]) == -1).all()
    # the argument checks of the three forward entry points
    io = cm._capi.CmpcWalkIO()
    bad = cm._capi.CmpcPlantMismatch(0, hidden.data_ptr(), 0, None, 0, None)
    assert s._lib.cmpc_rollout_tick_mismatch_device(s._h, ro.M, 0.0, 0, io.tick, 0, bad, None) != 0
    bad = cm._capi.CmpcPlantMismatch(0, None, -1, None, 0, None)
    assert s._lib.cmpc_rollout_walk_mismatch_device(s._h, ro.M, 0, 1, 1, io, None, 0, 0, None, None, 0, bad, None) != 0
    assert s._lib.cmpc_rollout_tick_mismatch_device(s._h, ro.M, 0.0, 0, io.tick, -1, mmc["_c"], None) != 0
    torch.cuda.synchronize()


def test_off_is_off(walk6):
    """mismatch=None, a mismatch of zero-length schedules and no gain, and walk_device_taped as it was: the same bits in every tape key and record key, no
    "mismatch" on the tape, and backward_device returns the keys it always did"""
    import torch
    cfg, plain = walk6["cfg"], walk6["plain"]
    com0, dcom0, h0 = walk6["start"]
    empty = dict(hidden_wrench=np.zeros((0, B, 6), np.float32), state_noise=np.zeros((0, B, 9), np.float32), force_gain=None, tick_first=2)
    for name, m in (("None", None), ("empty", empty)):
        ro = cm.rollout.WalkingRollout(cfg, B)
        w = ro.walk_device_taped(T, com0, dcom0, h0, mismatch=m)
        torch.cuda.synchronize()
        assert set(w) == set(plain) and set(w["tape"]) == set(plain["tape"]) and "mismatch" not in w["tape"]
        for k in TAPE_KEYS:
            _same_bits(w["tape"][k], plain["tape"][k], f"{name}: tape {k}")
        _same_bits(w["tape"]["info"][:, :, :6], plain["tape"]["info"][:, :, :6], f"{name}: tape info")      # (word 6 is the clock)
        for k in REC_KEYS:
            _same_bits(w[k], plain[k], f"{name}: {k}")
        r = ro.backward_device(w, walk6["gS"])
        torch.cuda.synchronize()
        assert not set(NEW) & set(r)
    # a mismatch struct of NULL pointers through cmpc_rollout_walk_mismatch_device is the plain walk too
    ro2 = cm.rollout.WalkingRollout(cfg, B)
    nul = ro2.solver.plant_mismatch()
    ro2._mismatch_of = lambda m: nul      # (let the all-NULL struct through, where the method would have dropped it)
    w2 = ro2.walk_device_taped(T, com0, dcom0, h0, mismatch=dict())
    torch.cuda.synchronize()
    assert "mismatch" in w2["tape"]
    for k in TAPE_KEYS:
        _same_bits(w2["tape"][k], plain["tape"][k], f"NULL struct: tape {k}")
    for k in REC_KEYS:
        _same_bits(w2[k], plain[k], f"NULL struct: {k}")


@pytest.mark.parametrize("skip_ended", [False, True])
def test_a_nan_push_ends_its_problem_alone(walk6, skip_ended):
    """NaN in problem 3's hidden-wrench row of tick 2: problem 3 ends at tick 2 with code 5, the seven others are bit-equal to the walk without the NaN"""
    import torch
    cfg, mm = walk6["cfg"], walk6["mm"]
    com0, dcom0, h0 = walk6["start"]
    bad = dict(mm, hidden_wrench=mm["hidden_wrench"].copy())
    bad["hidden_wrench"][2 - mm["tick_first"], 3, 1] = np.nan
    w = cm.rollout.WalkingRollout(cfg, B).walk_device_mismatch(T, com0, dcom0, h0, bad, skip_ended=skip_ended)
    ref = cm.rollout.WalkingRollout(cfg, B).walk_device_mismatch(T, com0, dcom0, h0, mm, skip_ended=skip_ended)
    torch.cuda.synchronize()
    assert _h(w["end_tick"]).tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and int(w["end_code"][3]) == 5
    assert _h(w["code"])[:, 3].tolist() == [0, 0, 5, -1, -1, -1] and (_h(ref["end_tick"]) == -1).all()
    others = [0, 1, 2, 4, 5, 6, 7]
    for k in REC_KEYS:
        if k == "stats":
            continue
        ax = 1 if k in ("com", "zmp", "land", "landing_offset", "iterations", "code") else 0
        _same_bits(np.take(_h(w[k]), others, axis=ax), np.take(_h(ref[k]), others, axis=ax), k)
    np.testing.assert_array_equal(_h(w["final_state"])[3, :3], _h(ref["com"])[1, 3])


# ---- 6. resume ----
def test_one_snapshot_forks_under_b_hidden_pushes():
    """a pilot walk of 4 ticks with a snapshot in front of tick 3; walk_resume_device_mismatch(index = zeros, B different hidden pushes, tick_first = 3):
    problem b equals the unbroken 6-tick walk of a batch of copies of the pilot's problem 0 whose problem b carries that push, to the bit; with a
    zero-length schedule the fork is the plain continuation"""
    import torch
    cfg = _cfg()
    com0, dcom0, h0, _ = _start(B)
    pilot = cm.rollout.WalkingRollout(cfg, B).walk_device_checkpointed(4, com0, dcom0, h0, 3)
    snap = pilot["checkpoints"][3]
    rng = np.random.default_rng(41)
    pushes = np.concatenate([rng.normal(0, 0.4, (2, B, 3)), rng.normal(0, 0.05, (2, B, 3))], -1).astype(np.float32)
    mm = dict(hidden_wrench=pushes, tick_first=3)
    index = np.zeros(B, np.int32)
    fork = cm.rollout.WalkingRollout(cfg, B).walk_resume_device_mismatch(snap, 3, mm, index=index)
    tile = lambda a: np.tile(a[0], (B, 1))
    whole = cm.rollout.WalkingRollout(cfg, B).walk_device_mismatch(6, tile(com0), tile(dcom0), tile(h0), mm)
    none = cm.rollout.WalkingRollout(cfg, B).walk_resume_device_mismatch(snap, 3, dict(hidden_wrench=np.zeros((0, B, 6), np.float32), tick_first=3), index=index)
    cont = cm.rollout.WalkingRollout(cfg, B).walk_resume_device(snap, 3, index=index)
    torch.cuda.synchronize()
    assert (_h(fork["index_ok"]) == 1).all() and (_h(fork["end_tick"]) == -1).all() and (_h(whole["end_tick"]) == -1).all()
    for k in ("state", "X", "P", "final_state", "iterations_sum", "box_slack_min"):
        _same_bits(fork[k], whole[k], f"fork against the unbroken walk: {k}")
    for k in ("com", "zmp", "land", "iterations", "code"):
        _same_bits(fork[k], whole[k][3:], f"fork against the unbroken walk: {k}")
    for k in ("state", "X", "P", "final_state", "com", "zmp"):
        _same_bits(none[k], cont[k], f"a zero-length schedule is the plain continuation: {k}")
    st = _h(fork["state"])
    assert len({st[b].tobytes() for b in range(B)}) == B        # B different pushes, B different robots
    assert np.abs(st - _h(cont["state"])).max(1).min() > 1e-4


# ---- 7. the tick VJP ----
def _tick_tape(tape, i):
    """row i of a device tape as rollout_tick_vjp_device's tape dict, built as the reverse walk builds its cmpc_tick_tape"""
    d = dict(X=tape["X"][i], P=tape["P"][i], lam_g=tape["lam_g"][i], state=tape["states"][i], info=tape["info"][i], ok=tape["ok"][i], land=tape["land"][i],
             plan_t=tape["plan_t"][i], plan_n=tape["plan_n"][i], prev_t=tape["list_t"][i - 1] if i > 0 else None,
             prev_n=tape["list_n"][i - 1] if i > 0 else None, list_t=tape["list_t"][i], list_n=tape["list_n"][i], step=tape["step"], substeps=tape["substeps"],
             force_sample_time=tape["force_sample_time"])
    return d


def _host_tape(tk, b, hidden, gain):
    h = lambda k: _h(tk[k][b])
    return dict(X=h("X"), P=h("P"), lam_g=h("lam_g"), state=h("state"), status=int(h("info")[5]), ok=bool(h("ok")), land=h("land"), list_t=h("list_t"),
                list_n=h("list_n"), plan=(h("plan_t"), h("plan_n")), prev=None if tk["prev_t"] is None else (h("prev_t"), h("prev_n")),
                step=float(np.float32(tk["step"])), substeps=tk["substeps"], force_sample_time=tk["force_sample_time"], hidden=hidden, gain=gain)


def _rows(mm, i):
    r = i - mm["tick_first"]
    return mm["hidden_wrench"][r] if 0 <= r < mm["hidden_wrench"].shape[0] else None


def test_tick_vjp_matches_the_restated_tick(walk6):
    """cmpc_rollout_tick_vjp_mismatch_device on ticks 1 and 2 (inside both schedules) and 4 (outside) of the taped walk against the restated tick fed with
    the tape's own float32 (x, p, lam_g): dGradHidden, dGradNoise, dGradGain and the existing groups within REF, the three new ones non-zero.  A problem
    whose merge failed gets exact zeros and adds nothing to dGradGain; its neighbours keep their bits."""
    import torch
    cfg, mm, tape, s = walk6["cfg"], walk6["mm"], walk6["w"]["tape"], walk6["ro"].solver
    M = tape["list_t"].shape[3]
    rng = np.random.default_rng(21)
    gain = _cu(mm["force_gain"])
    worst = _tick_vjp_gaps(cfg, mm, tape, s, (1, 2, 4), (0, 5), rng)
    print("mismatch tick VJP against the restated tick, worst: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {REF:.0e})")
    assert max(worst.values()) <= REF, worst
    # a flagged problem
    tk = _tick_tape(tape, 2)
    flagged = dict(tk, ok=tk["ok"].clone())
    flagged["ok"][6] = 0
    g_state, g_list = _cu(rng.normal(size=(B, 9))), _cu(rng.normal(size=(B, 2, M, 3)) * 0.1)
    gain0 = rng.normal(size=B)
    res = []
    for t_ in (flagged, tk):
        ggain = _cu(gain0)
        r = s.rollout_tick_vjp_device(2 * cfg.sampling_time, t_, g_state, g_list, grad_p=True, mismatch=True, hidden_wrench=_cu(_rows(mm, 2)), force_gain=gain,
                                      dGradGain=ggain, rot=True)
        torch.cuda.synchronize()
        res.append({k: _h(v) for k, v in dict(r, gain=ggain).items()})
    a, c = res
    assert a["sens"][6, 0] == 5 and (np.delete(a["sens"][:, 0], 6) == 0).all() and (c["sens"][:, 0] == 0).all()
    assert not a["hidden"][6].any() and not a["noise"][6].any() and a["gain"][6] == gain0[6] and c["gain"][6] != gain0[6]
    for k in ("state", "prev_list", "wrench", "p", "hidden", "noise", "gain", "rot", "prev_list_rot"):
        _same_bits(np.delete(a[k], 6, axis=0), np.delete(c[k], 6, axis=0), f"neighbours of the flagged problem: {k}")
    # with both inputs NULL every output the existing entry has is its
    old = s.rollout_tick_vjp_device(2 * cfg.sampling_time, tk, g_state, g_list, grad_p=True)
    new = s.rollout_tick_vjp_device(2 * cfg.sampling_time, tk, g_state, g_list, grad_p=True, mismatch=True)
    torch.cuda.synchronize()
    for k in old:
        _same_bits(new[k], old[k], f"both inputs NULL: {k}")


TICK_GROUPS = ("state", "prev_list", "wrench", "plan", "model", "p", "hidden", "noise", "gain")


def _tick_vjp_gaps(cfg, mm, tape, s, ticks, problems, rng):
    """cmpc_rollout_tick_vjp_mismatch_device on the given ticks of a taped walk against the restated tick (tests/mismatch_ref.tick_vjp) fed with the tape's own
    float32 (x, p, lam_g), for the given problems: -> the worst relative gap per group (TICK_GROUPS); the three new groups are asserted non-zero"""
    import torch
    nb, M = tape["X"].shape[1], tape["list_t"].shape[3]
    gain = _cu(mm["force_gain"])
    groups = TICK_GROUPS
    worst = {k: 0.0 for k in groups}
    for i in ticks:
        tk = _tick_tape(tape, i)
        hid = _rows(mm, i)
        g_state, g_list = rng.normal(size=(nb, 9)), rng.normal(size=(nb, 2, M, 3)) * 0.1
        gplan, gmodel = torch.zeros((nb, 2, M, 3), dtype=torch.float64, device="cuda"), torch.zeros((nb, 34), dtype=torch.float64, device="cuda")
        ggain = torch.zeros((nb,), dtype=torch.float64, device="cuda")
        now = i * cfg.sampling_time
        r = s.rollout_tick_vjp_device(now, tk, _cu(g_state), _cu(g_list), dGradPlan=gplan, dGradModel=gmodel, grad_p=True, mismatch=True,
                                      hidden_wrench=None if hid is None else _cu(hid), force_gain=gain, dGradGain=ggain)
        torch.cuda.synchronize()
        assert (_h(r["sens"])[:, 0] == 0).all(), _h(r["sens"])[:, 0]
        got = {k: _h(v) for k, v in dict(state=r["state"], prev_list=r["prev_list"], wrench=r["wrench"], plan=gplan, model=gmodel, p=r["p"], hidden=r["hidden"],
                                         noise=r["noise"], gain=ggain).items()}
        for b in problems:
            ref = mr.tick_vjp(cfg, _host_tape(tk, b, None if hid is None else hid[b], float(mm["force_gain"][b])), now, g_state[b], g_list[b])
            assert ref["status"] == 0
            gaps = {k: _rel(got[k][b], ref[k]) for k in groups}
            print(f"tick {i} problem {b}: " + " ".join(f"{k} {v:.1e}" for k, v in gaps.items()) +
                  f"  |hidden| {np.abs(got['hidden'][b]).max():.1e} |noise| {np.abs(got['noise'][b]).max():.1e} |gain| {abs(got['gain'][b]):.1e}")
            for k in groups:
                worst[k] = max(worst[k], gaps[k])
            assert np.abs(got["hidden"][b]).max() > 0 and np.abs(got["noise"][b]).max() > 0 and abs(got["gain"][b]) > 0
    return worst


# ---- 8. the reverse walk ----
def _reverse_by_hand(ro, w, gS, mm):
    """the reverse of a taped mismatched walk as cmpc_rollout_tick_vjp_mismatch_device chained by hand, last tick first, with one
    cmpc_rollout_walk_vjp_gate_device step between the ticks -> (backward_device's row and sum outputs, the state carry, the list carry)"""
    import torch
    tape, s, M, dev, dt = w["tape"], ro.solver, ro.M, ro.dev, ro.cfg.sampling_time
    T, B, N = int(tape["rows"]), ro.B, ro.cfg.N
    z = lambda shape, dtp=torch.float64: torch.zeros(shape, dtype=dtp, device=dev)
    out = dict(wrench=z((T, B, N, 6), torch.float32), models=z((B, 34)), plan=z((B, 2, M, 3)), status=z((T, B), torch.int32), hidden_wrench=z((T, B, 6)),
               state_noise=z((T, B, 9), torch.float32), force_gain=z((B,)))
    carry_s, carry_l, ok_out = gS[T].clone(), z((B, 2, M, 3)), z((B,), torch.int32)
    gain = _cu(mm["force_gain"])
    r = None
    with torch.cuda.stream(s.launch_stream):
        for i in range(T, -1, -1):
            g = cm._capi.CmpcWalkGate()
            g.batch, g.max_contacts, g.horizon, g.end_tick = B, M, N, w["end_tick"].data_ptr()
            g.do_post, g.tick_post = int(i < T), i
            if i < T:
                out["wrench"][i].copy_(r["wrench"])
                out["hidden_wrench"][i].copy_(r["hidden"])
                out["state_noise"][i].copy_(r["noise"])
                g.seed_state, g.tick_state, g.tick_list, g.tick_sens = gS[i].data_ptr(), r["state"].data_ptr(), r["prev_list"].data_ptr(), r["sens"].data_ptr()
                g.wrench_row, g.status_row = out["wrench"][i].data_ptr(), out["status"][i].data_ptr()
            g.carry_state, g.carry_list = carry_s.data_ptr(), carry_l.data_ptr()
            g.do_pre, g.tick_pre, g.first = int(i > 0), i - 1, int(i == T)
            if i > 0:
                g.ok_row, g.ok_out = tape["ok"][i - 1].data_ptr(), ok_out.data_ptr()
            s.rollout_walk_vjp_gate_device(g, dev)
            if i == 0:
                break
            tk = dict(_tick_tape(tape, i - 1), ok=ok_out)
            hid = _rows(mm, i - 1)
            r = s.rollout_tick_vjp_device((i - 1) * dt, tk, carry_s, carry_l, dGradPlan=out["plan"], dGradModel=out["models"], mismatch=True,
                                          hidden_wrench=None if hid is None else _cu(hid), force_gain=gain, dGradGain=out["force_gain"])
    torch.cuda.synchronize()
    return out, carry_s, carry_l


def test_reverse_walk_is_the_tick_vjps_chained_by_hand(walk6):
    """backward_device on the mismatch tape against cmpc_rollout_tick_vjp_mismatch_device chained by hand, last tick first, with one
    cmpc_rollout_walk_vjp_gate_device step between the ticks: every key to the bit; backward_device_rot leaves the three new keys (and the old ones) bit-equal"""
    import torch
    cfg, mm, ro, w, gS, got = walk6["cfg"], walk6["mm"], walk6["ro"], walk6["w"], walk6["gS"], walk6["got"]
    tape, s, M, dev, dt = w["tape"], ro.solver, ro.M, ro.dev, cfg.sampling_time
    assert set(NEW) <= set(got) and tuple(got["hidden_wrench"].shape) == (T, B, 6) and tuple(got["state_noise"].shape) == (T, B, 9)
    out, carry_s, carry_l = _reverse_by_hand(ro, w, gS, mm)
    _same_bits(carry_s, got["state0"], "state0")
    _same_bits(carry_l, got["list0"], "list0")
    for k in ("wrench", "models", "plan", "status") + NEW:
        _same_bits(out[k], got[k], k)
    assert (_h(got["status"]) == 0).all()
    for k in NEW:
        assert np.isfinite(_h(got[k])).all() and np.abs(_h(got[k])).max() > 0, k
    assert np.abs(_h(got["hidden_wrench"])[0]).max() > 0      # tick 0 lies outside the schedule: the gradient of a wrench that was zero is still there
    rot = ro.backward_device_rot(w, gS)
    refs = ro.backward_device_refs(w, gS)
    torch.cuda.synchronize()
    for k in GRADS + NEW:
        _same_bits(rot[k], got[k], f"rot=True: {k}")
        _same_bits(refs[k], got[k], f"refs: {k}")
    # the existing reverse walk on this tape differentiates another plant: it must not agree
    old = dict(w, tape={k: v for k, v in tape.items() if k != "mismatch"})
    plain = ro.backward_device(old, gS)
    torch.cuda.synchronize()
    assert not np.array_equal(_h(plain["state0"]), _h(got["state0"]))


def test_an_ended_problem_keeps_its_mismatch_gradient_and_the_others_theirs(walk6):
    """problem 3 ends at tick 2 by a replan its planner cannot merge, with NaN seeds behind the end: in the three new keys it equals the 2-tick walk's
    gradient, has exact zeros from row 2 on, and the others keep the bits of the walk without the replan"""
    import torch
    cfg, mm, gS = walk6["cfg"], walk6["mm"], walk6["gS"]
    com0, dcom0, h0 = walk6["start"]
    ro = cm.rollout.WalkingRollout(cfg, B)
    t = ro.plan[0].clone()
    t[3, 0] += 100.0
    w = ro.walk_device_taped(T, com0, dcom0, h0, replan={2: (t, ro.plan[1], ro.plan[2])}, mismatch=mm)
    ro2 = cm.rollout.WalkingRollout(cfg, B)
    two = ro2.walk_device_taped(2, com0, dcom0, h0, mismatch=mm)
    seeds = _h(gS).copy()
    seeds_nan = seeds.copy()
    seeds_nan[3:, 3] = np.nan
    got = ro.backward_device(w, seeds_nan)
    short = ro2.backward_device(two, seeds[:3])
    torch.cuda.synchronize()
    assert _h(w["end_tick"]).tolist() == [-1, -1, -1, 2, -1, -1, -1, -1] and int(w["end_code"][3]) == 1
    got, short, ref = ({k: _h(r[k]) for k in GRADS + NEW} for r in (got, short, walk6["got"]))
    others = [0, 1, 2, 4, 5, 6, 7]
    for k in GRADS + NEW:
        assert np.isfinite(got[k]).all(), k
        ax = 1 if k in ("wrench", "status", "hidden_wrench", "state_noise") else 0
        _same_bits(np.take(got[k], others, axis=ax), np.take(ref[k], others, axis=ax), f"the others: {k}")
    _same_bits(got["hidden_wrench"][:2, 3], short["hidden_wrench"][:, 3], "problem 3: hidden_wrench")
    _same_bits(got["state_noise"][:2, 3], short["state_noise"][:, 3], "problem 3: state_noise")
    _same_bits(got["force_gain"][3], short["force_gain"][3], "problem 3: force_gain")
    assert not got["hidden_wrench"][2:, 3].any() and not got["state_noise"][2:, 3].any()
    assert np.abs(got["hidden_wrench"][:2, 3]).max() > 0 and got["force_gain"][3] != 0
    assert got["status"][:, 3].tolist() == [0, 0, 6, 6, 6, 6]


# ---- 9. autograd ----
def test_autograd_through_the_mismatch():
    """.grad of hidden_wrench, state_noise and force_gain is the method's keys to the bit; one gradient step on the hidden pushes lowers |com_T - target|^2;
    the refusals raise NotImplementedError"""
    import torch
    import torch.autograd.forward_ad as fwad
    cfg = _cfg()
    nb = 4
    com0, dcom0, h0, _ = _start(nb, seed=3)
    s0 = np.concatenate([com0, dcom0, h0], 1).astype(np.float32)
    mm = _mismatch(nb, hidden_ticks=4, noise_ticks=3, tick_first=0)
    target = torch.tensor([0.05, 0.02, 0.7], dtype=torch.float64, device="cuda")

    def loss_of(hidden, grad=True):
        ro = cm.rollout.WalkingRollout(cfg, nb)
        H = _cu(hidden).requires_grad_(grad)
        Z, G = _cu(mm["state_noise"]).requires_grad_(grad), _cu(mm["force_gain"]).requires_grad_(grad)
        states = cm.rollout_differentiable(ro, T, _cu(s0), device_walk=True, hidden_wrench=H, state_noise=Z, force_gain=G)
        loss = ((states[-1, :, 0:3].to(torch.float64) - target) ** 2).sum()
        if grad:
            loss.backward()
        torch.cuda.synchronize()
        return ro, float(loss.detach()), H.grad, Z.grad, G.grad
    ro, l0, gH, gZ, gG = loss_of(mm["hidden_wrench"])
    r = ro.last_backward
    _same_bits(gH, r["hidden_wrench"][:4].to(torch.float32), "hidden_wrench.grad")
    _same_bits(gZ, r["state_noise"][:3], "state_noise.grad")
    _same_bits(gG, r["force_gain"].to(torch.float32), "force_gain.grad")
    assert float(gH.abs().max()) > 0 and float(gZ.abs().max()) > 0 and float(gG.abs().max()) > 0 and (_h(ro.last_walk["end_tick"]) == -1).all()
    # one step of steepest descent on the pushes, at most 0.01 m/s^2 per entry: small against the pushes' 0.3, so that the first-order decrease dominates
    lr = 0.01 / float(gH.abs().max())
    _, l1, _, _, _ = loss_of((_cu(mm["hidden_wrench"]) - lr * gH).cpu().numpy(), grad=False)
    print(f"\nloss |com_T - target|^2: {l0:.8e} -> {l1:.8e} after one gradient step on the hidden pushes (predicted decrease {lr * float((gH.double() ** 2).sum()):.3e})")
    assert l1 < l0
    # refusals
    w = ro.last_walk
    with pytest.raises(NotImplementedError):
        ro.forward_sensitivity_device(w, dir_state0=torch.zeros((nb, 1, 9), dtype=torch.float64, device="cuda"))
    with pytest.raises(NotImplementedError):
        ro.forward_sensitivity_device_refs(w, dir_ref_com=None, dir_ref_h=None, dir_state0=torch.zeros((nb, 1, 9), dtype=torch.float64, device="cuda"))
    wc = ro.walk_device_checkpointed(4, com0, dcom0, h0, 2, mismatch=mm)
    with pytest.raises(NotImplementedError):
        ro.backward_device_checkpointed(wc, np.zeros((5, nb, 9)))
    with pytest.raises(NotImplementedError):
        ro.run(2, com0, dcom0, h0, mismatch=mm)
    with pytest.raises(NotImplementedError):
        cm.rollout_differentiable(ro, T, _cu(s0), hidden_wrench=_cu(mm["hidden_wrench"]))
    with pytest.raises(NotImplementedError):
        with fwad.dual_level():
            dual = fwad.make_dual(_cu(s0), torch.ones_like(_cu(s0)))
            cm.rollout_differentiable(ro, T, dual, device_walk=True, force_gain=_cu(mm["force_gain"]))
    torch.cuda.synchronize()


# ---- 10. no host read ----
def test_nothing_is_read_back(walk6):
    """walk_device_taped under a mismatch and backward_device under torch's sync debug mode, after the fixture's calls have allocated the workspaces"""
    import torch
    ro, mm = walk6["ro"], walk6["mm"]
    com0, dcom0, h0 = walk6["start"]
    dmm = dict(hidden_wrench=_cu(mm["hidden_wrench"]), state_noise=_cu(mm["state_noise"]), force_gain=_cu(mm["force_gain"]), tick_first=1)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = ro.walk_device_taped(T, com0, dcom0, h0, mismatch=dmm, skip_ended=True)
        r = ro.backward_device(w, walk6["gS"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for k in GRADS + NEW:
        _same_bits(r[k], walk6["got"][k], k)
