"""No GPU: the argument checks in front of the library calls of BatchSolver (_args.py; solver.py, solver_rollout.py, solver_walk_grad.py) -- that they
are not `assert` statements and so hold under `python -O`, that our own sources keep no hand-written tensor assert, and that a refusal comes before
the library is touched in each of the three modules."""
import ast
import os
import types

import pytest
import torch

import cmpc_amd as cm

PKG = os.path.dirname(os.path.abspath(cm.solver.__file__))
MODULES = ("solver.py", "solver_rollout.py", "solver_walk_grad.py", "_args.py")


class _FakeCuda:
    """stands in for a CUDA tensor in the checks: what _args reads of a tensor, settable"""

    def __init__(self, dtype=torch.float32, shape=(2, 3), cuda=True, contiguous=True):
        self.dtype, self.shape, self.is_cuda, self._contiguous = dtype, shape, cuda, contiguous

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return 4096


def _optimised_args():
    """_args.py compiled as `python -OO` compiles it (assert statements and docstrings dropped) and executed in this process"""
    path = os.path.join(PKG, "_args.py")
    mod = types.ModuleType("_args_optimised")
    exec(compile(open(path).read(), path, "exec", optimize=2), mod.__dict__)
    return mod


@pytest.mark.parametrize("args", [_optimised_args(), cm._args], ids=["optimize=2", "as imported"])
def test_the_checks_survive_optimisation(args):
    f32, f64 = torch.float32, torch.float64
    assert args.ptr(_FakeCuda(), f32, (2, 3), "a") == 4096 and args.ptr(None, f32, (2, 3), "a") is None
    assert args.ptr(_FakeCuda(shape=(7, 3)), f32, (None, 3), "a") == 4096      # (None: any length of that axis)
    good = _FakeCuda()
    assert args.out(good, f32, (2, 3), "o", None) is good
    made = args.out(None, f64, (2, 3), "o", "cpu")
    assert made.dtype == f64 and tuple(made.shape) == (2, 3)
    bad = dict(dtype=_FakeCuda(dtype=f64), shape=_FakeCuda(shape=(2, 2)), rank=_FakeCuda(shape=(2, 3, 1)), view=_FakeCuda(contiguous=False),
               host=_FakeCuda(cuda=False), real_host_tensor=torch.zeros((2, 3)), real_view=torch.zeros((3, 2)).t())
    for what, t in bad.items():
        for call in (lambda: args.ptr(t, f32, (2, 3), "the_argument"), lambda: args.ptr(t, f32, (2, 3), "the_argument", True),
                     lambda: args.out(t, f32, (2, 3), "the_argument", None)):
            with pytest.raises(AssertionError, match=r"^the_argument: expected torch\.float32 \(2, 3\)$"):
                call()
    with pytest.raises(AssertionError, match=r"^the_argument: expected torch\.float32 \(2, 3\)$"):
        args.ptr(None, f32, (2, 3), "the_argument", required=True)
    with pytest.raises(AssertionError, match=r"^a text of its own$"):
        args.ptr(_FakeCuda(shape=(4, 4)), f32, (None, 3), "a", msg="a text of its own")
    assert args.opt_ptr(None) is None and args.opt_ptr(good) == 4096


def test_no_tensor_assert_is_left_in_the_solver_modules():
    """an `assert` statement whose test reads is_cuda, is_contiguous, .dtype or .shape vanishes under -O and leaves a raw data_ptr() unguarded"""
    found = []
    for name in MODULES:
        tree = ast.parse(open(os.path.join(PKG, name)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.Assert):
                attrs = {n.attr for n in ast.walk(node.test) if isinstance(n, ast.Attribute)}
                if attrs & {"is_cuda", "is_contiguous", "dtype", "shape"}:
                    found.append(f"{name}:{node.lineno}")
    assert found == []


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def _bare_solver(N=10, B=2):
    s = cm.BatchSolver.__new__(cm.BatchSolver)
    s.layout, s.batch, s._lib, s._h = cm.Layout(N), B, _NoLibrary(), None
    s.cfg = types.SimpleNamespace(N=N)
    return s


def test_one_method_of_each_module_refuses_before_the_library():
    """host tensors of the right shapes: every one of them is refused by name, in solver.py, solver_rollout.py and solver_walk_grad.py alike"""
    s = _bare_solver()
    L, B = s.layout, s.batch
    X, P, Lm = torch.zeros((B, L.nx)), torch.zeros((B, L.np)), torch.zeros((B, L.ng))
    with pytest.raises(AssertionError, match=r"^dGradX: expected torch\.float32 \(2, %d\)$" % L.nx):
        s.solution_vjp_device(X, P, Lm, torch.zeros((B, L.nx)))                                      # solver.py
    with pytest.raises(AssertionError, match=r"^dP: expected torch\.float32"):
        s.solve_device(P, X)
    with pytest.raises(AssertionError, match=r"^dP: expected torch\.float32 \(2, %d\)$" % L.np):
        s.cold_start_device(P)                                                                       # solver_rollout.py
    tape = dict(rows=3, max_contacts=2, _c=None)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    with pytest.raises(AssertionError, match=r"^grad_states: expected torch\.float64 \(4, 2, 9\)$"):
        s.rollout_walk_vjp_device(0, 3, tape, 0, None, z(4, B, 9), z(B, 9), z(B, 2, 2, 3), torch.zeros((3, B), dtype=torch.int32))   # solver_walk_grad.py
    with pytest.raises(AssertionError, match=r"^grad_states: expected torch\.float64 \[>= 4, \(2, 9\)\]$"):
        s.rollout_walk_vjp_rows_device(0, 3, tape, 0, None, z(4, B, 9), z(B, 9), z(B, 2, 2, 3), torch.zeros((3, B), dtype=torch.int32))
    with pytest.raises(AssertionError, match="the segment must lie inside its tape"):
        s.rollout_walk_vjp_rows_device(0, 4, tape, 0, None, None, None, None, None)
