"""forceSampleTime on the CPU (ContactPhaseList::forceSampleTime(m_dT), CentroidalMPCBlock.cpp:586-592): the host entry point of the C ABI
(cmpc_contacts_force_sample_time) against the independent restatement of the rule (tests/snap_ref.py), its properties, its argument checks, and
the stand-in ContactPhaseList::forceSampleTime of csrc/shim/ against the C ABI."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cmpc_amd as cm
from cmpc_amd.contacts import force_sample_time, pack_lists
from tests import snap_ref
from tests.test_contacts_cpu import _random_walks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("dt", [0.06, 0.1, 0.05, 0.0371, 0.001])
def test_host_entry_matches_the_restatement_bit_for_bit(dt):
    rng = np.random.default_rng(int(dt * 1e4))
    t, n = snap_ref.random_lists(rng, 600, 5, dt)
    got, ok = force_sample_time(dt, t, n)
    ref, rok = snap_ref.snap_lists(dt, t, n)
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    np.testing.assert_array_equal(ok, rok)
    # the draw covers the corners of the rule: failures and successes, ties, the sentinel, negative and non-finite times
    assert ok.any() and not ok.all()
    assert (np.abs(t) >= 1e9).any() and (t < 0).any() and (~np.isfinite(t)).any()
    dt_ns = snap_ref.dt_in_ns(dt)
    if dt_ns % 2 == 0:
        fin = np.isfinite(t) & (np.abs(t) < 1e9)
        ties = [x for x in t[fin] if snap_ref.llround(float(x) * 1e9) % dt_ns == dt_ns // 2]
        assert len(ties) > 10
        for x in ties[:50]:       # ties go to the later multiple
            assert snap_ref.snap_time(float(x), dt_ns)[0] > float(x)


def test_in_place_and_out_of_place_agree_and_unused_entries_are_copied():
    rng = np.random.default_rng(3)
    t, n = snap_ref.random_lists(rng, 300, 6, 0.06)
    lib = cm._capi.lib()
    out = np.full_like(t, 123.0)
    ok1 = np.zeros(300, np.int32)
    lib.cmpc_contacts_force_sample_time(300, 6, 0.06, _ptr(t), _ptr(n), _ptr(out), _ptr(ok1))
    inplace = t.copy()
    ok2 = np.zeros(300, np.int32)
    lib.cmpc_contacts_force_sample_time(300, 6, 0.06, _ptr(inplace), _ptr(n), _ptr(inplace), _ptr(ok2))
    np.testing.assert_array_equal(_bits(out), _bits(inplace))
    np.testing.assert_array_equal(ok1, ok2)
    unused = np.arange(6)[None, None, :] >= n[:, :, None]
    np.testing.assert_array_equal(_bits(out[unused]), _bits(t[unused]))


def test_snapping_is_idempotent_keeps_on_grid_lists_and_the_order():
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    # on the grid: walking_plan's times (multiples of 0.06 s) come back with the same bits
    t, _, n = pack_lists(cfg, [cm.rollout.walking_plan(cfg)])
    got, ok = force_sample_time(0.06, t, n)
    assert ok.all() and np.array_equal(_bits(got), _bits(t))
    # off the grid: random walks (footstep times drawn from a continuum)
    for dt in (0.06, 0.1):
        t, _, n = pack_lists(cfg, _random_walks(cfg, 200, 13))
        once, ok = force_sample_time(dt, t, n)
        assert ok.all()
        assert not np.array_equal(once, t)
        twice, ok2 = force_sample_time(dt, once, n)
        assert ok2.all() and np.array_equal(_bits(twice), _bits(once))
        dt_ns = snap_ref.dt_in_ns(dt)
        for b in range(t.shape[0]):
            for c in range(2):
                seq = once[b, c, :n[b, c]].reshape(-1)
                assert (np.diff(seq) >= 0).all()          # activation <= deactivation <= next activation: order and non-overlap kept
                fin = seq[np.abs(seq) < 1e9]
                assert all(snap_ref.llround(float(x) * 1e9) % dt_ns == 0 for x in fin)
        assert (np.abs(once - t)[np.abs(t) < 1e9] <= dt / 2 + 1e-12).all()


def test_a_collapsing_contact_fails_only_its_problem():
    t = np.zeros((3, 2, 2, 2))
    n = np.full((3, 2), 2, np.int32)
    t[:, :, 0] = (0.0, 0.3)
    t[:, :, 1] = (0.5, 1e9)
    t[1, 1, 1] = (0.61, 0.62)                 # 10 ms inside one 60 ms cell: collapses
    t[2, 0, 1] = (0.61, 0.61)                 # zero duration stays zero: not a failure
    got, ok = force_sample_time(0.06, t, n)
    assert ok.tolist() == [True, False, True]
    s600 = 600_000_000 * 1e-9                 # (q dt_ns) 1e-9 s: 0.6000000000000001
    assert got[1, 1, 1].tolist() == [s600, s600] and got[2, 0, 1].tolist() == [s600, s600]
    assert got[0, 0, 1, 0] == 480_000_000 * 1e-9 and got[0, 0, 0, 1] == 0.3   # 0.5 -> 0.48; 0.3 is on the grid: its own bits
    t[0, 0, 0, 1] = np.nan
    _, ok = force_sample_time(0.06, t, n)
    assert ok.tolist() == [False, False, True]


def test_argument_errors_are_reported():
    lib = cm._capi.lib()
    t = np.zeros((2, 2, 3, 2))
    n = np.ones((2, 2), np.int32)
    out = np.zeros_like(t)
    ok = np.zeros(2, np.int32)
    f = lambda B=2, M=3, dt=0.06, tp=_ptr(t), np_=_ptr(n), op=_ptr(out): lib.cmpc_contacts_force_sample_time(B, M, dt, tp, np_, op, _ptr(ok))
    assert f() == 0 and ok.tolist() == [1, 1]
    for bad in (0.0, -0.06, float("nan"), 1e-12, 2e9):
        assert f(dt=bad) == -1, bad
    assert f(B=0) == -1 and f(M=0) == -1 and f(tp=None) == -1 and f(np_=None) == -1 and f(op=None) == -1
    for v in (-1, 4):
        n2 = n.copy(); n2[1, 0] = v
        assert f(np_=_ptr(n2)) == -1
        assert "length" in lib.cmpc_last_error(None).decode()
    with pytest.raises(ValueError):
        force_sample_time(0.0, t, n)


@pytest.fixture(scope="module")
def shim_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("fst") / "force_sample_time_driver")
    pkg = os.path.dirname(cm.config.__file__)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(pkg, "csrc", "shim"), os.path.join(ROOT, "tests", "force_sample_time_driver.cpp"),
                           "-o", exe])
    return exe


@pytest.mark.parametrize("dt", [0.06, 0.1, 0.25])
def test_shim_contact_phase_list_gives_the_c_abi_times(shim_driver, dt):
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    t, _, n = pack_lists(cfg, _random_walks(cfg, 120, 41))
    t[:5, :, :, :] += 0.0125                   # a few plans shifted off the grid from the start
    got, ok = force_sample_time(dt, t, n)
    dt_ns = snap_ref.dt_in_ns(dt)
    lines = [f"{dt_ns} {t.shape[0]}"]
    for b in range(t.shape[0]):
        for c in range(2):
            lines.append(" ".join([str(int(n[b, c]))] + [str(snap_ref.llround(float(x) * 1e9)) for x in t[b, c, :n[b, c]].reshape(-1)]))
    res = subprocess.run([shim_driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    for b in range(t.shape[0]):
        vals = [int(v) for v in res[b].split()]
        assert vals[0] == int(ok[b]), b
        i = 1
        for c in range(2):
            assert vals[i] == n[b, c]
            shim_ns = vals[i + 1:i + 1 + 2 * n[b, c]]
            i += 1 + 2 * n[b, c]
            if ok[b]:
                assert shim_ns == [snap_ref.llround(float(x) * 1e9) for x in got[b, c, :n[b, c]].reshape(-1)], (b, c)
    if dt == 0.25:
        assert not ok.all() and ok.any()       # double supports of 0.1-0.25 s collapse on a 0.25 s grid in some plans
    else:
        assert ok.all()
