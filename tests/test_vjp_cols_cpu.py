"""No GPU: the cotangent-column VJP (include/cmpc.h, cmpc_solution_vjp_cols_device; BatchSolver.solution_vjp_cols_device / policy_jacobian_device) as far
as it can be held without a device -- the declaration and the export list, the refusals that need no handle, the argument checks of the Python methods, and
the linearity of tests/sens_ref.py's VJP, which is what lets tests/test_gpu_vjp_cols.py hold every column to it on its own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cmpc_amd as cm
from tests import sens_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cmpc_solution_vjp_cols_device"


def test_header_declares_the_entry_and_exports_carry_it():
    hdr = open(os.path.join(ROOT, "include", "cmpc.h")).read()
    m = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m is not None
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["cmpc_handle h", "const float* dX", "const float* dP", "const float* dLamG", "const float* dGradX", "int k", "float* dGradP",
                    "double* dGradModel", "double* dGradRot", "float* dSens", "void* stream"], args
    assert NAME in cm._capi.EXPORTS
    lib = cm._capi.lib()
    assert hasattr(lib, NAME) and len(getattr(lib, NAME).argtypes) == len(args)


def test_refusals_need_no_handle():
    """k = 0, all outputs NULL and a NULL input are refused before anything is queued, each with its own reason in cmpc_last_error(NULL); with nothing
    else wrong, the NULL handle is the reason"""
    lib = cm._capi.lib()
    lib.cmpc_last_error.restype = C.c_char_p
    buf = (C.c_float * 8)()
    dbl = (C.c_double * 8)()
    a, d = C.cast(buf, C.c_void_p), C.cast(dbl, C.c_void_p)
    fn = getattr(lib, NAME)
    why = lambda: lib.cmpc_last_error(None).decode()
    assert fn(None, a, a, a, a, 0, a, None, None, None, None) == -1 and NAME in why() and "k must be >= 1" in why()
    assert fn(None, a, a, a, a, -3, a, d, d, None, None) == -1 and "k must be >= 1" in why()
    assert fn(None, a, a, a, a, 2, None, None, None, a, None) == -1 and "no output requested" in why()
    for miss in range(4):
        ins = [a, a, a, a]
        ins[miss] = None
        assert fn(None, *ins, 2, a, None, None, None, None) == -1 and "null input" in why()
    assert fn(None, a, a, a, a, 2, None, d, None, None, None) == -1 and "null handle" in why()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def _bare_solver(N=10, B=2):
    s = cm.BatchSolver.__new__(cm.BatchSolver)
    s.layout, s.batch, s._lib, s._h = cm.Layout(N), B, _NoLibrary(), None
    return s


def test_python_methods_check_their_arguments_before_the_library():
    import torch
    s = _bare_solver()
    L = s.layout
    X, P, Lm = torch.zeros((2, L.nx)), torch.zeros((2, L.np)), torch.zeros((2, L.ng))
    with pytest.raises(AssertionError, match=r"\[B, k, n_x\]"):
        s.solution_vjp_cols_device(X, P, Lm, torch.zeros((2, L.nx)))
    with pytest.raises(AssertionError, match="float32"):
        s.solution_vjp_cols_device(X, P, Lm, torch.zeros((2, 3, L.nx), dtype=torch.float64))
    with pytest.raises(AssertionError, match="no output requested"):
        s.solution_vjp_cols_device(X, P, Lm, torch.zeros((2, 3, L.nx)), grad_p=False, grad_model=False, grad_rot=False)
    with pytest.raises(AssertionError, match="rows index x"):
        s.policy_jacobian_device(X, P, Lm, rows=[L.nx])
    with pytest.raises(AssertionError, match="rows index x"):
        s.policy_jacobian_device(X, P, Lm, rows=[])


def test_sens_ref_vjp_is_linear_in_its_cotangent():
    """SensRef.vjp of a combination of k cotangents is the combination of its columns (a double-support point, so the internal-force projection is in
    it): each column of a k-column call can be held to sens_ref on its own"""
    from tests.test_sensitivity_cpu import _load
    cfg, x, p, lam = _load("cfg2", None, 0, os.path.join(ROOT, "tests", "golden"))
    S = sens_ref.Sens(cfg, x, p, lam)
    assert S.n is not None
    L = cm.Layout(cfg.N)
    rng = np.random.default_rng(5)
    V = rng.standard_normal((3, L.nx))
    V[1] += 4.0 * S.n
    idx = [L.p_com0, L.p_com0 + 4, L.p_comref + 5, L.p_href + 7, L.p_fext + 2, L.p_text + 1, L.p_nom[0] + 6]
    cols = np.stack([S.vjp(V[j], idx) for j in range(3)])
    w = np.array([0.5, -2.0, 1.25])
    both = S.vjp(w @ V, idx)
    assert np.abs(cols[:, idx]).max() > 0
    np.testing.assert_allclose(both[idx], (w @ cols)[idx], rtol=1e-9, atol=1e-9 * np.abs(cols).max())


def test_host_form_of_the_column_path_under_sanitizers(tmp_path):
    """sens_problem on the host (one-thread team) from a stand-alone program with its own main, the host side built with -fsanitize=address,undefined: at
    the cfg2 golden (double support: the internal-force projection) and the cfg5 golden (swing phases), k = 9 columns in one call against nine single-column
    calls -- no sanitizer report, status 0, every column's outputs the single call's bytes, dSens as include/cmpc.h states it"""
    import shutil
    import subprocess
    import __graft_entry__ as ge
    from tests.test_sensitivity_cpu import _load
    hipcc = shutil.which(ge.HIPCC) or ge.HIPCC
    assert os.path.exists(hipcc), f"no hipcc at {hipcc}"   # (no compiler is a failure, not a skip)
    exe = str(tmp_path / "vjp_cols_host_driver")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-I", ge.CSRC, os.path.join(ROOT, "tests", "vjp_cols_host_driver.cpp"), "-o", exe])
    files = []
    for name in ("cfg2", "cfg5"):
        cfg, x, p, lam = _load(name, None, 0, os.path.join(ROOT, "tests", "golden"))
        path = str(tmp_path / f"{name}.bin")
        with open(path, "wb") as f:
            f.write(np.int32(cfg.N).tobytes() + np.float64(cfg.sampling_time).tobytes() + cm.config.model_row(cfg).astype(np.float64).tobytes())
            for a in (x, p, lam):
                f.write(a.astype(np.float32).tobytes())
        files.append((cfg.N, path))
    r = subprocess.run([exe] + [p for _, p in files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines == [f"N {N} status 0 internal {i} columns-equal 1 sens-words-equal 1 residual-is-max 1 removed-is-max 1 nonzero 1"
                     for (N, _), i in zip(files, (1, 0))], lines
