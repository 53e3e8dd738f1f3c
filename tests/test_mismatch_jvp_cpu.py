"""The plant-model mismatch forwards without a GPU (include/cmpc.h, "the mismatch FORWARDS"; DESIGN.md 7f, "Mismatch, forwards"): the three symbols and the
two structs against the header, the Python surface with the pinned signatures unchanged, the float64 restatement tests/mismatch_jvp_ref.py against
tests/mismatch_ref.py -- its tick JVP is the transpose of mismatch_ref.tick_vjp, its plant JVP agrees with central differences of mismatch_ref.plant_step,
gain = 0 and a foot off among the cases -- and the refusals of the C entries that need no device.  Every bound is one the project already has, and the
transpose gaps are the project's measure, |lhs - rhs| / max(|lhs|, |rhs|) (tests/test_rollout_jvp_cpu._gap).
The three tests of the restatement hold the REFERENCE the GPU tests compare the kernels with, not product code: they run no new symbol and would pass on a
tree that has the reference file alone.  test_symbols_structs_and_surface and test_c_entries_refuse_before_anything_touches_a_gpu need the product."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cmpc_amd as cm
from tests import mismatch_jvp_ref as mj
from tests import mismatch_ref as mr
from tests import rollout_adjoint_ref as ra
from tests import sens_rot_ref as srr
from tests.test_mismatch_cpu import FD
from tests.test_rollout_adjoint_cpu import _plant_case
from tests.test_rollout_jvp_cpu import _directions, _gap, _yawed_ticks

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmpc.h")
NAMES = ("cmpc_plant_step_jvp_mismatch_cols_device", "cmpc_rollout_tick_jvp_mismatch_device", "cmpc_rollout_walk_jvp_mismatch_device")
TRANSPOSE = 1e-12      # the restated tick JVP against the restated tick VJP: two float64 contractions of the same linear maps


def test_symbols_structs_and_surface():
    """the three symbols are declared, exported and built; the two ctypes structs have the header's field order and the size its comment states; the new
    Python methods exist and the pinned signatures are what they were"""
    text = open(HEADER).read()
    lib = cm._capi.lib()
    for name in NAMES:
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and re.search(r"\b" + name + r"\(", text), name
    for cname, mirror in (("cmpc_tick_dirs_mismatch", cm._capi.CmpcTickDirsMismatch), ("cmpc_walk_dirs_mismatch", cm._capi.CmpcWalkDirsMismatch)):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert names == [f[0] for f in mirror._fields_] == ["dDirHidden", "dDirNoise", "dDirGain"], cname
        size = int(re.search(r"sizeof\(" + cname + r"\) == (\d+)", text).group(1))
        assert C.sizeof(mirror) == size == 24, cname
    assert len(lib.cmpc_plant_step_jvp_mismatch_cols_device.argtypes) == len(lib.cmpc_plant_step_jvp_cols_device.argtypes) + 4
    assert len(lib.cmpc_rollout_tick_jvp_mismatch_device.argtypes) == len(lib.cmpc_rollout_tick_jvp_device.argtypes) + 3
    assert len(lib.cmpc_rollout_walk_jvp_mismatch_device.argtypes) == len(lib.cmpc_rollout_walk_jvp_device.argtypes) + 2
    ro = cm.rollout.WalkingRollout
    for name in ("forward_sensitivity_device_mismatch", "backward_device_checkpointed_mismatch"):
        assert hasattr(ro, name), name
    for name in ("plant_step_jvp_mismatch_cols_device", "rollout_tick_jvp_mismatch_device", "rollout_walk_jvp_mismatch_device"):
        assert hasattr(cm.BatchSolver, name), name
    assert hasattr(cm, "rollout_differentiable_checkpointed_mismatch")
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.forward_sensitivity_device_mismatch) == ["self", "w", "dir_hidden_wrench", "dir_state_noise", "dir_force_gain", "dir_ref_com", "dir_ref_h",
                                                           "dirs"]
    assert par(ro.backward_device_checkpointed_mismatch) == ["self", "w", "grad_states", "grad_X", "rot"]
    assert par(cm.rollout_differentiable_checkpointed_mismatch) == ["rollout", "ticks", "state0", "every", "hidden_wrench", "state_noise", "force_gain", "push",
                                                                    "models", "push_ticks", "replan"]
    assert par(cm.BatchSolver.rollout_walk_jvp_mismatch_device)[10:14] == ["mismatch", "dir_hidden", "dir_noise", "dir_gain"]
    assert par(cm.BatchSolver.rollout_walk_jvp_mismatch_device)[:10] == par(cm.BatchSolver.rollout_walk_jvp_device)[:10]
    assert not {"mismatch", "dir_hidden", "dir_noise", "dir_gain"} & set(par(cm.BatchSolver.rollout_walk_jvp_device))
    # the pinned signatures are unchanged (the lists of tests/test_walk_snapshot_cpu.py)
    assert par(ro.backward_device_checkpointed) == ["self", "w", "grad_states", "grad_X", "rot"]
    assert par(cm.rollout_differentiable_checkpointed) == ["rollout", "ticks", "state0", "every", "push", "models", "push_ticks", "replan"]
    assert par(ro.backward_device_refs) == ["self", "w", "grad_states", "grad_X", "rot"]
    assert par(ro.backward_device) == ["self", "w", "grad_states", "grad_X"] == par(ro.backward_device_rot)
    assert par(ro.forward_sensitivity_device) == ["self", "w", "dir_state0", "dir_list0", "dir_list_rot0", "dir_plan", "dir_plan_rot", "dir_push", "dir_models",
                                                  "dir_wrench", "solutions"]
    assert par(ro.forward_sensitivity_device_refs) == ["self", "w", "dir_ref_com", "dir_ref_h", "dirs"]
    assert par(ro.walk_device_checkpointed) == ["self", "ticks", "com0", "dcom0", "h0", "every", "kwargs"]
    assert par(ro.walk_device_taped) == ["self", "ticks", "com0", "dcom0", "h0", "kwargs"]
    # the refusing methods name the new ones
    assert "forward_sensitivity_device_mismatch" in ro.forward_sensitivity_device.__doc__
    assert "backward_device_checkpointed_mismatch" in ro.backward_device_checkpointed.__doc__ and "Out of scope" in ro.backward_device_checkpointed.__doc__


@pytest.mark.parametrize("gate_off,yaw,gain", [(None, 0.0, 0.87), (1, 0.0, 0.87), (None, 0.6, 1.1), (0, 0.3, 0.0), (None, 0.3, 0.0)])
def test_restated_plant_jvp_matches_central_differences(gate_off, yaw, gain):
    """mismatch_jvp_ref.plant_jvp along each of the 76 coordinates (state, pos_0, the MPC's forces, fExt_0, tauExt_0, corners, hidden wrench, gain) against
    central differences of mismatch_ref.plant_step, step 1e-4, per group relative to the group's largest entry: <= 1e-8 (tests/test_mismatch_cpu.py's FD:
    the map is at most quadratic along a coordinate, so what remains is rounding).  A foot off and gain = 0 among the cases: there the force columns are
    exactly zero on both sides and the gain's column is not."""
    L, corners, x, p, state = _plant_case(7, gate_off, yaw)
    rng = np.random.default_rng(17)
    hidden = rng.normal(0, 0.4, 6)
    step, nsub, eps = 0.01, 6, 1e-4
    xi, pi = ra.plant_columns(L)
    f = lambda **kw: mr.plant_step(L, kw.get("corners", corners), kw.get("x", x), kw.get("p", p), kw.get("state", state), step, nsub, kw.get("hidden", hidden),
                                   kw.get("gain", gain))[0]

    def moved(col, s):
        """the inputs with coordinate `col` of the 76 moved by s"""
        if col < ra.C_POS:
            v = state.copy(); v[col] += s
            return dict(state=v)
        if col < ra.C_FEXT:
            v = x.copy(); v[xi[col - ra.C_POS]] += s
            return dict(x=v)
        if col < ra.C_CORN:
            v = p.copy(); v[pi[col - ra.C_FEXT]] += s
            return dict(p=v)
        if col < ra.NCOL:
            v = np.array(corners, np.float64).reshape(-1).copy(); v[col - ra.C_CORN] += s
            return dict(corners=v.reshape(2, 4, 3))
        if col < mr.C_GAIN:
            v = hidden.copy(); v[col - mr.C_HID] += s
            return dict(hidden=v)
        return dict(gain=gain + s)
    groups = dict(state=(0, ra.C_POS), pos=(ra.C_POS, ra.C_F), forces=(ra.C_F, ra.C_FEXT), wrench=(ra.C_FEXT, ra.C_CORN), corners=(ra.C_CORN, ra.NCOL),
                  hidden=(mr.C_HID, mr.C_GAIN), gain=(mr.C_GAIN, mr.NCOL))
    got, fd = np.zeros((9, mr.NCOL)), np.zeros((9, mr.NCOL))
    for col in range(mr.NCOL):
        e = np.zeros(mr.NCOL); e[col] = 1.0
        dx, dp, dm = np.zeros(L.nx), np.zeros(L.np), np.zeros(34)
        dx[xi] = e[ra.C_POS:ra.C_FEXT]; dp[pi] = e[ra.C_FEXT:ra.C_CORN]; dm[10:] = e[ra.C_CORN:ra.NCOL]
        got[:, col] = mj.plant_jvp(L, corners, x, p, state, step, nsub, e[:9], dx, dp, dm, None, hidden, gain, e[mr.C_HID:mr.C_GAIN], e[mr.C_GAIN])
        fd[:, col] = (f(**moved(col, eps)) - f(**moved(col, -eps))) / (2 * eps)
    for k, (a, b) in groups.items():
        if k in ("forces", "pos", "corners") and gain == 0.0:      # no force is applied: none of these has a derivative, exactly, on either side
            assert not got[:, a:b].any() and not fd[:, a:b].any(), k
            continue
        gap = np.abs(got[:, a:b] - fd[:, a:b]).max() / np.abs(fd[:, a:b]).max()
        print(f"restated mismatch plant JVP gate_off={gate_off} yaw={yaw} gain={gain} {k}: relative gap {gap:.2e} (bound {FD:.0e})")
        assert gap <= FD, (k, gap)
    assert np.abs(got[:, mr.C_GAIN]).max() > 0 and np.abs(got[:, mr.C_HID:mr.C_GAIN]).max() > 0
    if gate_off is not None:      # the gated-off foot's forces have no derivative
        assert not got[:, ra.C_F + 12 * gate_off:ra.C_F + 12 * gate_off + 12].any()
    # a random direction is the combination of the columns, and the plain plant is the mismatched one at gain 1 without a hidden wrench
    d = rng.normal(size=mr.NCOL)
    dx, dp, dm = np.zeros(L.nx), np.zeros(L.np), np.zeros(34)
    dx[xi] = d[ra.C_POS:ra.C_FEXT]; dp[pi] = d[ra.C_FEXT:ra.C_CORN]; dm[10:] = d[ra.C_CORN:ra.NCOL]
    np.testing.assert_allclose(mj.plant_jvp(L, corners, x, p, state, step, nsub, d[:9], dx, dp, dm, None, hidden, gain, d[mr.C_HID:mr.C_GAIN], d[mr.C_GAIN]),
                               got @ d, rtol=0, atol=1e-13 * np.abs(got).max() * np.abs(d).sum())
    plain = ra.plant_jvp(L, corners, x, p, state, step, nsub, d[:9], dx, dp, dm)      # (a product of 69 columns against one of 76: summed in other blocks)
    np.testing.assert_allclose(mj.plant_jvp(L, corners, x, p, state, step, nsub, d[:9], dx, dp, dm), plain, rtol=0, atol=1e-14 * np.abs(plain).max())


@pytest.fixture(scope="module")
def yawed_ticks():
    return _yawed_ticks()


@pytest.mark.parametrize("gain", [0.87, 0.0])
def test_restated_tick_jvp_is_the_transpose_of_the_restated_tick_vjp(yawed_ticks, gain):
    """<g, J d> = <J^T g, d> of one whole mismatched tick: mismatch_jvp_ref.tick_jvp against mismatch_ref.tick_vjp on ticks 3 (a foot in swing: off) and 5
    (the landing tick) of the yawed walk on the float64 oracle, under a hidden wrench and a gain (0.87, and 0: no contact force applied), with the position
    groups, the wrench, the model, the extra p direction and the three mismatch directions random at once, and once more with each mismatch direction
    alone: to 1e-12.  The noise direction's cotangent is the solve's gradient on com0 / dcom0 / h0 and nothing of the plant's."""
    cfg, tapes, nows = yawed_ticks
    L = cm.Layout(cfg.N)
    M = tapes[0]["list_t"].shape[1]
    rng = np.random.default_rng(29)
    assert not all(tapes[0]["P"][L.p_gam[c]] > 0.5 for c in range(2)), "no foot is off on the first of the ticks"
    for i in (0, 2):
        tp = dict(tapes[i], hidden=rng.normal(0, 0.4, 6), gain=gain)
        now = nows[i]
        d = _directions(rng, cfg, M)
        dm = dict(hidden=rng.normal(size=6), noise=rng.normal(size=9) * 0.1, gain=float(rng.normal()))
        g_state, g_list, g_x = rng.normal(size=9), rng.normal(size=(2, M, 3)), rng.normal(size=L.nx) * 0.1
        r = mr.tick_vjp(cfg, tp, now, g_state, g_list, g_x)
        assert r["status"] == 0
        RS = srr.RotSens(cfg, tp["X"], tp["P"], tp["lam_g"])
        for only in (None, "hidden", "noise", "gain"):
            on = lambda k: dm[k] if only in (None, k) else None
            base = only is None
            f = mj.tick_jvp(cfg, tp, now, d["state"] if base else None, d["list"] if base else None, None, d["plan"] if base else None, None,
                            d["wrench"] if base else None, d["model"] if base else None, d["p"] if base else None, on("hidden"), on("noise"), on("gain"), RS=RS)
            assert f["status"] == 0
            lhs = g_state @ f["state"] + (g_list * f["list"]).sum() + g_x @ f["x"]
            terms = dict(hidden=r["hidden"] @ dm["hidden"], noise=r["noise"] @ dm["noise"], gain=r["gain"] * dm["gain"])
            terms = {k: v for k, v in terms.items() if only in (None, k)}
            if base:
                terms.update(state=r["state"] @ d["state"], list=(r["prev_list"] * d["list"]).sum(), plan=(r["plan"] * d["plan"]).sum(),
                             wrench=(r["wrench"] * d["wrench"]).sum(), model=r["model"] @ d["model"], p=r["p"] @ d["p"])
            rhs = sum(terms.values())
            gap = _gap(lhs, rhs)
            print(f"tick {3 + i} gain {gain} directions {only or 'all'}: <g, J d> = {lhs:.12e}, <J^T g, d> = {rhs:.12e}, gap {gap:.2e} (bound {TRANSPOSE:.0e}); "
                  "terms " + " ".join(f"{k} {v:.2e}" for k, v in terms.items()))
            assert gap <= TRANSPOSE, (i, only, gap)
            merge = tp["prev"] is not None      # (the first of the ticks starts from the planner's lists: no merge reads the planner's directions)
            assert all(v != 0 for k, v in terms.items() if merge or k != "plan")      # every group takes part, each mismatch group also alone
    # the noise direction reaches the solve and nothing else: with the solution held (a flagged tick passes nothing on) ...
    tp = dict(tapes[0], hidden=None, gain=1.0, ok=False)
    assert not mj.tick_jvp(cfg, tp, nows[0], d_noise=dm["noise"])["state"].any()
    # ... and on a live tick it moves the next state only through dx: the plant's own state columns see d_state alone
    tp = dict(tapes[0], hidden=None, gain=1.0)
    a = mj.tick_jvp(cfg, tp, nows[0], d_noise=dm["noise"])
    b = mj.tick_jvp(cfg, tp, nows[0], d_state=dm["noise"])
    np.testing.assert_array_equal(a["x"], b["x"])
    assert not np.array_equal(a["state"], b["state"])


def test_restated_forward_sweep_is_the_contraction_of_the_restated_reverse_sweep(yawed_ticks):
    """three mismatched ticks: sum_i <gS_i, d state_i> + <gX_i, d x_i> of mismatch_jvp_ref.forward_sweep equals the contraction of mismatch_ref.reverse_sweep's
    state0, list0, plan, models, wrench, hidden_wrench, state_noise and force_gain with the directions, to 1e-12"""
    cfg, tapes, nows = yawed_ticks
    L = cm.Layout(cfg.N)
    T, M = len(tapes), tapes[0]["list_t"].shape[1]
    rng = np.random.default_rng(6)
    tapes = [dict(tp, hidden=rng.normal(0, 0.4, 6) if i != 1 else None, gain=1.07) for i, tp in enumerate(tapes)]
    gS, gX = rng.normal(size=(T + 1, 9)), rng.normal(size=(T, L.nx)) * 0.1
    d = _directions(rng, cfg, M)
    dw, dh, dn, dg = rng.normal(size=(T, cfg.N, 6)), rng.normal(size=(T, 6)), rng.normal(size=(T, 9)) * 0.1, float(rng.normal())
    out = mr.reverse_sweep(cfg, tapes, nows, gS, gX)
    f = mj.forward_sweep(cfg, tapes, nows, d["state"], d["list"], d["plan"], d["model"], dw, dh, dn, dg)
    assert list(out["status"]) == [0] * T and f["status"] == [0] * T
    lhs = (gS * f["states"]).sum() + (gX * f["X"]).sum()
    terms = dict(state0=out["state0"] @ d["state"], list0=(out["list0"] * d["list"]).sum(), plan=(out["plan"] * d["plan"]).sum(), models=out["models"] @ d["model"],
                 wrench=(out["wrench"] * dw).sum(), hidden=(out["hidden_wrench"] * dh).sum(), noise=(out["state_noise"] * dn).sum(), gain=out["force_gain"] * dg)
    rhs = sum(terms.values())
    gap = _gap(lhs, rhs)
    print(f"\nmismatched forward sweep against the reverse sweep over three ticks: {lhs:.12e} vs {rhs:.12e}, gap {gap:.2e} (bound {TRANSPOSE:.0e}); terms " +
          " ".join(f"{k} {v:.2e}" for k, v in terms.items()))
    assert gap <= TRANSPOSE and all(v != 0 for v in terms.values())


def test_c_entries_refuse_before_anything_touches_a_gpu():
    """each of the three entries refuses a NULL handle, and the walk a non-NULL schedule with a zero count and a negative count, with CMPC_ERR_ARG and the
    entry's own name in cmpc_last_error(NULL); no handle exists, so nothing can have been queued.  Without a GPU there is no handle to give: only the
    schedule refusals, which are checked ahead of the handle, are told apart by their reason here.  The k < 1 and tick0 < 0 calls below return -1 through the
    handle check whatever k and tick0 are; their own checks are held on a live handle, reason and all, by
    tests/test_gpu_mismatch_jvp.py::test_c_entries_refuse_bad_arguments_on_a_live_handle."""
    lib = cm._capi.lib()
    lib.cmpc_last_error.restype = C.c_char_p
    why = lambda: lib.cmpc_last_error(None).decode()
    buf = (C.c_double * 64)()
    a = C.cast(buf, C.c_void_p)
    plant, tick, walk = (getattr(lib, n) for n in NAMES)
    for k in (1, 0, -2):
        assert plant(None, a, a, a, 0.01, 6, k, a, None, None, None, None, a, a, a, a, a, None) == -1 and NAMES[0] in why()
        tape, dout = cm._capi.CmpcTickTape(), cm._capi.CmpcTickDirsOut(a, a)
        md = cm._capi.CmpcTickDirsMismatch(a, a, a)
        assert tick(None, 4, 0.0, C.byref(tape), k, None, C.byref(dout), a, a, a, C.byref(md), None) == -1 and NAMES[1] in why()
        assert tick(None, 4, 0.0, C.byref(tape), k, None, C.byref(dout), a, None, None, None, None) == -1 and NAMES[1] in why()
        wt, wd = cm._capi.CmpcWalkTape(), cm._capi.CmpcWalkDirs(a, a)
        assert walk(None, 4, 0, 1, C.byref(wt), 0, None, k, C.byref(wd), None, None, None) == -1 and NAMES[2] in why()
    # the mismatch's own rules, checked first: a schedule without rows, a negative count
    wt, wd = cm._capi.CmpcWalkTape(), cm._capi.CmpcWalkDirs(a, a)
    wm = cm._capi.CmpcWalkDirsMismatch(a, a, a)
    for mm in (cm._capi.CmpcPlantMismatch(0, a, 0, None, 0, None), cm._capi.CmpcPlantMismatch(0, None, 0, a, 0, None),
               cm._capi.CmpcPlantMismatch(0, a, -1, None, 0, None), cm._capi.CmpcPlantMismatch(0, None, 0, None, -3, a)):
        assert walk(None, 4, 0, 1, C.byref(wt), 0, None, 2, C.byref(wd), C.byref(mm), C.byref(wm), None) == -1
        assert NAMES[2] in why() and "bad mismatch" in why()
    # tick0 < 0 is refused as the plain forward walk refuses it
    assert walk(None, 4, -1, 1, C.byref(wt), 0, None, 2, C.byref(wd), None, C.byref(wm), None) == -1 and NAMES[2] in why()
