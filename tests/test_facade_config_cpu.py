"""The C++ facade's initialize() on every shipped robot's ini file, without a GPU: tests/facade_config_driver.cpp compiles the header against
the csrc/shim/ headers with stub cmpc_* functions and prints the cmpc_config the class hands to cmpc_create.

The tolerance it passes must resolve (cmpc_create: <= 0 -> cmpc_default_tolerance(N)) to the library's default for the robot's horizon: the
shipped ipopt_tolerance values (1e-4 / 1e-2) are looser than the parity target, and a positive value would keep cmpc_create from applying its
tighter default beyond N = 20 (ergoCubSN001, N = 22)."""
import os
import shutil
import subprocess

import pytest

import cmpc_amd as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS = ["ergoCubGazeboV1", "ergoCubGazeboV1_1", "ergoCubSN000", "ergoCubSN001", "iCubGazeboV3"]


def _param_lines(text):
    out = []
    for group, kv in cm.config.parse_ini(text).items():
        for k, v in kv.items():
            g = group or "-"
            if isinstance(v, bool):
                out.append(f"{g} {k} b {int(v)}")
            elif isinstance(v, int):
                out.append(f"{g} {k} i {v}")
            elif isinstance(v, float):
                out.append(f"{g} {k} d {v!r}")
            elif isinstance(v, tuple):
                out.append(f"{g} {k} v " + " ".join(repr(float(a)) for a in v))
            else:
                out.append(f"{g} {k} s {v}")
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("facade")
    exe = str(d / "facade_config_driver")
    pkg = os.path.dirname(cm.config.__file__)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkg, "csrc", "shim"),
                           os.path.join(ROOT, "tests", "facade_config_driver.cpp"), "-o", exe])
    lib = cm._capi.lib()
    tol = d / "default_tolerance.txt"
    tol.write_text("".join(f"{n} {lib.cmpc_default_tolerance(n)!r}\n" for n in range(2, 41)))
    return exe, str(tol), d


def test_default_tolerance_rule():
    lib = cm._capi.lib()
    assert [lib.cmpc_default_tolerance(n) for n in (4, 10, 13, 20)] == [1e-6] * 4
    assert [lib.cmpc_default_tolerance(n) for n in (2, 3)] == [3e-7] * 2   # (two and three stages: no tail polish, the first velocities need it)
    assert [lib.cmpc_default_tolerance(n) for n in (21, 22, 30)] == [3e-7] * 3


@pytest.mark.parametrize("robot", ROBOTS)
def test_facade_passes_the_default_tolerance_for_every_shipped_robot(robot, driver, golden_dir):
    exe, tol, d = driver
    text = open(os.path.join(golden_dir, "ini", f"{robot}.ini")).read()
    cfg = cm.config.from_ini(text)
    params = d / f"{robot}.params"
    params.write_text(_param_lines(text))
    out = subprocess.run([exe, str(params), tol], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    seen = {k: float(v) for k, v in (ln.split() for ln in out.stdout.splitlines())}
    assert seen["horizon"] == cfg.N and seen["sampling_time"] == cfg.sampling_time
    assert seen["contact_position_weight"] == cfg.contact_position_weight
    default = cm._capi.lib().cmpc_default_tolerance(cfg.N)
    effective = seen["tolerance"] if seen["tolerance"] > 0 else default
    assert effective == default, (robot, cfg.N, cfg.ipopt_tolerance, seen["tolerance"])
    # the Python class builds the same cmpc_config
    assert cm.solver._c_config(cfg).tolerance == seen["tolerance"]


@pytest.mark.parametrize("ipopt_tol,N,expect", [(1e-2, 22, 0.0), (1e-4, 13, 0.0), (4e-7, 22, 0.0), (4e-7, 20, 4e-7), (1e-7, 30, 1e-7)])
def test_python_config_passes_only_a_tighter_tolerance(ipopt_tol, N, expect):
    """solver._c_config applies the facade's rule: 4e-7 is tighter than 1e-6 (N = 20) but looser than 3e-7 (N = 22)."""
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    cfg.ipopt_tolerance = ipopt_tol
    assert cm.solver._c_config(cfg).tolerance == expect
