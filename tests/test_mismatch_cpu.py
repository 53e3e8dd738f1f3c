"""The plant-model mismatch without a GPU (include/cmpc.h, "plant-model mismatch on the device walk"): the float64 restatement tests/mismatch_ref.py against
central differences of its own plant and against oracle/plant_ref at gain 1 / no hidden wrench, the ctypes mirror against the header, and the refusals that
need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cmpc_amd as cm
from oracle import plant_ref
from tests import mismatch_ref as mr
from tests import rollout_adjoint_ref as ra
from tests.test_rollout_adjoint_cpu import _plant_case

# The map is at most quadratic along any coordinate direction (bilinear in (state, pos, corners, wrench, gain) x forces), so a central difference has no
# truncation error: the gap is rounding, eps_machine * |f| / step ~ 1e-16 / 1e-4 = 1e-12 relative to entries of order one.  1e-8 leaves four decades.
FD = 1e-8
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmpc.h")


@pytest.mark.parametrize("gate_off,yaw", [(None, 0.0), (1, 0.0), (None, 0.6)])
def test_mismatch_columns_match_central_differences(gate_off, yaw):
    """the restatement's Jacobian columns for the hidden wrench, the gain and the MPC's forces against central differences of the restated plant, step 1e-4"""
    _check_columns(gate_off, yaw, 0.87)


@pytest.mark.parametrize("gate_off", [None, 0])
def test_mismatch_columns_at_gain_zero(gate_off):
    """gain = 0, where the plant applies no contact force at all: the force columns are exactly zero on both sides, the gain column is not (the plant is
    linear in the gain, so the central difference across zero is exact), the hidden wrench's is the plain plant's; and the state is free fall under the
    two external wrenches, closed form"""
    _check_columns(gate_off, 0.3, 0.0)
    L, corners, x, p, state = _plant_case(7, gate_off, 0.3)
    hidden = np.random.default_rng(17).normal(0, 0.4, 6)
    got, zmp = mr.plant_step(L, corners, x, p, state, 0.01, 6, hidden, 0.0)
    want = mr.free_fall(state, p[L.p_fext:L.p_fext + 3] + hidden[:3], p[L.p_text:L.p_text + 3] + hidden[3:], 0.06)
    assert np.abs(got - want).max() <= 1e-13 and np.isnan(zmp).all()
    assert mr.zmp_branches(L, corners, x, p, 0.0)[:2] == ((False, False), False)


def _check_columns(gate_off, yaw, gain):
    L, corners, x, p, state = _plant_case(7, gate_off, yaw)
    rng = np.random.default_rng(17)
    hidden = rng.normal(0, 0.4, 6)
    step, nsub, eps = 0.01, 6, 1e-4
    J = mr.plant_jacobian(L, corners, x, p, state, step, nsub, hidden, gain)
    xi, _ = ra.plant_columns(L)
    f = lambda x_, h_, g_: mr.plant_step(L, corners, x_, p, state, step, nsub, h_, g_)[0]
    fd = {}
    cols = []
    for q in range(24):
        x1, x0 = x.copy(), x.copy()
        x1[xi[6 + q]] += eps; x0[xi[6 + q]] -= eps
        cols.append((f(x1, hidden, gain) - f(x0, hidden, gain)) / (2 * eps))
    fd["forces"] = np.array(cols).T
    cols = []
    for i in range(6):
        h1, h0 = hidden.copy(), hidden.copy()
        h1[i] += eps; h0[i] -= eps
        cols.append((f(x, h1, gain) - f(x, h0, gain)) / (2 * eps))
    fd["hidden"] = np.array(cols).T
    fd["gain"] = ((f(x, hidden, gain + eps) - f(x, hidden, gain - eps)) / (2 * eps))[:, None]
    got = dict(forces=J[:, ra.C_F:ra.C_FEXT], hidden=J[:, mr.C_HID:mr.C_HID + 6], gain=J[:, mr.C_GAIN:mr.C_GAIN + 1])
    for k in fd:
        if gain == 0.0 and k == "forces":      # no force is applied: no derivative, exactly, on either side
            assert not got[k].any() and not fd[k].any()
            continue
        gap = np.abs(got[k] - fd[k]).max() / np.abs(fd[k]).max()
        print(f"mismatch partials gate_off={gate_off} yaw={yaw} {k}: relative gap {gap:.2e} (bound {FD:.0e})")
        assert gap <= FD, (k, gap)
        assert np.abs(fd[k]).max() > 0
    if gate_off is not None:      # the gated-off foot's forces have no derivative and take no part in the gain's
        assert not got["forces"][:, 12 * gate_off:12 * gate_off + 12].any()
    # the VJP is the transpose
    g = rng.normal(size=9)
    gs, gx, gp, gm, gh, gg = mr.plant_vjp(L, corners, x, p, state, step, nsub, g, hidden, gain)
    np.testing.assert_allclose(gh, J[:, mr.C_HID:mr.C_HID + 6].T @ g, rtol=0, atol=0)
    np.testing.assert_allclose(gh, gp[[L.p_fext, L.p_fext + 1, L.p_fext + 2, L.p_text, L.p_text + 1, L.p_text + 2]], rtol=0, atol=0)
    assert abs(gg - float(J[:, mr.C_GAIN] @ g)) <= 1e-14 * max(1.0, abs(gg))      # (one dot product summed in two orders)


def test_no_mismatch_is_the_oracle_plant():
    """gain = 1 and hidden = 0 (and hidden = None): the restatement equals plant_ref.plant_step exactly, state and ZMP, and its Jacobian the existing one"""
    for seed, gate_off in ((3, None), (4, 0)):
        L, corners, x, p, state = _plant_case(seed, gate_off)
        want = plant_ref.plant_step(L, corners, x, p, state, 0.01, 6)
        for hidden in (None, np.zeros(6)):
            got = mr.plant_step(L, corners, x, p, state, 0.01, 6, hidden, 1.0)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
            J = mr.plant_jacobian(L, corners, x, p, state, 0.01, 6, hidden, 1.0)
            np.testing.assert_array_equal(J[:, :ra.NCOL], ra.plant_jacobian(L, corners, x, p, state, 0.01, 6))


def test_struct_mirror_exports_and_surface():
    """the ctypes mirror has the header's field order and the size the header comment states; the six symbols are declared, exported and built; the Python
    surface exists and the pinned signatures are untouched"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct cmpc_plant_mismatch \{(.*?)\} cmpc_plant_mismatch;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in cm._capi.CmpcPlantMismatch._fields_]
    size = int(re.search(r"sizeof\(cmpc_plant_mismatch\) == (\d+)", text).group(1))
    assert C.sizeof(cm._capi.CmpcPlantMismatch) == size == 48
    assert [f[0] for f in cm._capi.CmpcWalkGradsMismatch._fields_] == ["dGradHidden", "dGradNoise", "dGradGain"]
    assert C.sizeof(cm._capi.CmpcWalkGradsMismatch) == 3 * 8
    lib = cm._capi.lib()
    for name in ("cmpc_plant_step_mismatch_device", "cmpc_rollout_tick_mismatch_device", "cmpc_rollout_walk_mismatch_device",
                 "cmpc_plant_step_vjp_mismatch_device", "cmpc_rollout_tick_vjp_mismatch_device", "cmpc_rollout_walk_vjp_mismatch_device"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name) and name in text, name
    ro = cm.rollout.WalkingRollout
    for name in ("walk_device_mismatch", "walk_resume_device_mismatch"):
        assert hasattr(ro, name), name
    for name in ("plant_mismatch", "plant_step_mismatch_device", "plant_step_vjp_mismatch_device", "rollout_tick_mismatch_device"):
        assert hasattr(cm.BatchSolver, name), name
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(ro.walk_device_mismatch)[:6] == ["self", "ticks", "com0", "dcom0", "h0", "mismatch"]
    assert par(ro.walk_resume_device_mismatch)[:4] == ["self", "snapshot", "ticks", "mismatch"]
    for k in ("hidden_wrench", "state_noise", "force_gain"):
        assert inspect.signature(cm.rollout_differentiable).parameters[k].default is None
    assert par(ro.walk_device)[-1] == "skip_ended" and par(ro.backward_device) == ["self", "w", "grad_states", "grad_X"]


def test_refusals_that_need_no_device():
    """a mismatch off the device walk is refused before anything touches a GPU"""
    with pytest.raises(NotImplementedError):
        cm.rollout_differentiable(None, 1, None, hidden_wrench=object())
    with pytest.raises(NotImplementedError):
        cm.rollout_differentiable(None, 1, None, force_gain=object(), device_walk=False)
    with pytest.raises(NotImplementedError):
        cm.rollout.WalkingRollout.run(None, 1, None, None, None, mismatch=dict(force_gain=np.ones(1)))
