"""Per-problem models on the CPU (include/cmpc.h, cmpc_model): the host check of the model rule (cmpc_check_models, which cmpc_set_models runs
before it touches the handle), the packing of configurations into model rows (config.model_array), and cmpc_model_from_config against it for every
shipped robot."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cmpc_amd as cm
_capi = cm._capi
_c_config = cm.solver._c_config

ROBOTS = ["ergoCubGazeboV1", "ergoCubGazeboV1_1", "ergoCubSN000", "ergoCubSN001", "iCubGazeboV3"]


def _ini(robot, golden_dir):
    return cm.config.from_ini(open(os.path.join(golden_dir, "ini", f"{robot}.ini")).read())


def _check(a):
    a = np.ascontiguousarray(a, np.float64)
    rc = _capi.lib().cmpc_check_models(a.ctypes.data, a.shape[0])
    return rc, _capi.lib().cmpc_last_error(None).decode()


def test_model_struct_is_34_packed_doubles():
    assert C.sizeof(_capi.CmpcModel) == 8 * _capi.MODEL_DOUBLES == 8 * cm.config.MODEL_DOUBLES


@pytest.mark.parametrize("robot", ROBOTS)
def test_model_from_config_round_trips_every_shipped_ini(robot, golden_dir):
    cfg = _ini(robot, golden_dir)
    cc = _c_config(cfg)
    m = _capi.CmpcModel()
    _capi.lib().cmpc_model_from_config(C.byref(cc), C.byref(m))
    got = np.frombuffer(bytes(m), np.float64)
    want = cm.config.model_row(cfg)
    assert got.shape == want.shape == (34,)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), np.nonzero(got != want)
    # and the row names the config's fields in cmpc_config's order
    assert got[0] == cfg.static_friction_coefficient and tuple(got[1:4]) == tuple(cfg.com_weight)
    assert tuple(got[6:9]) == tuple(cfg.force_rate_of_change_weight) and got[9] == cfg.contact_force_symmetry_weight
    assert np.array_equal(got[10:].reshape(2, 4, 3), np.asarray([c.corners for c in cfg.contacts]))
    assert _check(want[None])[0] == 0


def test_check_accepts_valid_tables(golden_dir):
    rng = np.random.default_rng(5)
    base = cm.config.model_array([_ini(r, golden_dir) for r in ROBOTS])
    a = np.repeat(base, 40, 0)
    a[:, 0] = rng.uniform(0.05, 2.0, a.shape[0])
    a[:, 10:] *= rng.uniform(0.8, 1.2, (a.shape[0], 1))
    a[:, 1:6] *= rng.uniform(0.0, 3.0, (a.shape[0], 5))     # weights may be 0 (iCubGazeboV3 has no symmetry cost) ...
    a[:3, 1:6] = 0.0
    a[:, 6:9] = rng.uniform(1e-3, 50.0, (a.shape[0], 3))     # ... the force-rate weights may not
    a[5, 10:] = 0.0                                          # corners: any finite value
    assert _check(a)[0] == 0


FIELDS = (["friction_coefficient"] + [f"com_weight[{i}]" for i in range(3)] + ["angular_momentum_weight", "contact_position_weight"]
          + [f"force_rate_of_change_weight[{i}]" for i in range(3)] + ["contact_force_symmetry_weight"]
          + [f"corners[{c}][{j}][{i}]" for c in range(2) for j in range(4) for i in range(3)])
POSITIVE = {0, 6, 7, 8}


def _bad_values(i):
    vals = [math.nan, math.inf, -math.inf]
    if i in POSITIVE:
        vals += [0.0, -0.0, -1e-300, -0.5]
    elif i < 10:
        vals += [-1e-300, -2.0]
    return vals


@pytest.mark.parametrize("field", range(34))
def test_check_rejects_each_invalid_field_at_its_index(field):
    a = np.repeat(cm.config.model_array([cm.config.ergocub_gazebo_v1()]), 9, 0)
    for n, v in enumerate(_bad_values(field)):
        b = (0, 3, 8)[n % 3]
        t = a.copy()
        t[b, field] = v
        rc, err = _check(t)
        assert rc == -1, (field, v)
        assert err.startswith(f"model {b}: {FIELDS[field]} = "), err
    # the first failing problem is named, and within it the first failing field
    t = a.copy()
    t[6, field] = math.nan
    t[7, 0] = 0.0
    t[6, 33] = math.nan
    rc, err = _check(t)
    assert rc == -1 and err.startswith(f"model 6: {FIELDS[field]} = nan"), err


def test_zero_weights_pass_where_the_rule_allows_them():
    a = cm.config.model_array([cm.config.icub_gazebo_v3()])
    assert a[0, 9] == 0.0
    assert _check(a)[0] == 0
    for i in range(1, 6):
        t = a.copy(); t[0, i] = 0.0
        assert _check(t)[0] == 0, FIELDS[i]
    for i in POSITIVE:
        t = a.copy(); t[0, i] = 0.0
        assert _check(t)[0] == -1, FIELDS[i]


def test_check_rejects_null_and_empty_tables():
    L = _capi.lib()
    assert L.cmpc_check_models(None, 4) == -1
    a = cm.config.model_array([cm.config.ergocub_gazebo_v1()])
    assert L.cmpc_check_models(a.ctypes.data, 0) == -1


def test_solver_set_models_checks_shape_without_a_device():
    _model_array = cm.solver._model_array
    cfgs = [cm.config.ergocub_gazebo_v1(), cm.config.icub_gazebo_v3(20, 0.06)]
    a = _model_array(cfgs, 2)
    assert a.flags.c_contiguous and a.dtype == np.float64 and a.shape == (2, 34)
    assert np.array_equal(a, _model_array(a.tolist(), 2))
    with pytest.raises(ValueError):
        _model_array(cfgs, 3)
