"""No GPU: the shape of the roll-out layer's modules after their split -- no `assert` statement, so every check holds under
`python -O`; the launch stream and torch's current stream wait for each other in ONE helper; one argument binding; no lambda that converts "numpy or
tensor" by hand -- and the pure checks raising with their texts from modules compiled as `python -OO` compiles them."""
import ast
import os
import types

import numpy as np
import pytest
import torch

import cmpc_amd as cm

PKG = os.path.dirname(os.path.abspath(cm.rollout.__file__))
MODULES = ("rollout.py", "rollout_common.py", "rollout_walk.py", "rollout_refill.py", "rollout_grad.py", "rollout_autograd.py")
TREES = {name: ast.parse(open(os.path.join(PKG, name)).read()) for name in MODULES}


def _calls(node, attr):
    return [n for n in ast.walk(node) if isinstance(n, ast.Attribute) and n.attr == attr]


def test_no_module_is_longer_than_the_solver_module_and_the_sum_is_not_above_the_one_file_it_was():
    lines = {name: len(open(os.path.join(PKG, name)).read().splitlines()) for name in MODULES}
    assert max(lines.values()) <= 823 and sum(lines.values()) <= 2094, lines


def test_no_assert_statement_is_left():
    found = [f"{name}:{n.lineno}" for name, tree in TREES.items() for n in ast.walk(tree) if isinstance(n, ast.Assert)]
    assert found == []


def test_the_streams_wait_for_each_other_in_one_helper():
    where = {(name, f.name) for name, tree in TREES.items() for f in ast.walk(tree) if isinstance(f, ast.FunctionDef) and _calls(f, "wait_stream")
             and not any(isinstance(g, ast.FunctionDef) and g is not f and _calls(g, "wait_stream") for g in ast.walk(f))}
    assert where == {("rollout_common.py", "_on_launch_stream")}
    assert sum(len(_calls(tree, "wait_stream")) for tree in TREES.values()) == 2
    assert sum(len(_calls(tree, "current_stream")) for tree in TREES.values()) == 1


def test_one_argument_binding_and_no_hand_written_conversion():
    assert sum(len(_calls(tree, "signature")) for tree in TREES.values()) == 1
    lambdas = [f"{name}:{n.lineno}" for name, tree in TREES.items() for n in ast.walk(tree) if isinstance(n, ast.Lambda)
               and {"to", "contiguous"} <= {a.attr for a in ast.walk(n.body) if isinstance(a, ast.Attribute)}]
    assert lambdas == []
    assert sum(len(_calls(tree, "from_numpy")) for name, tree in TREES.items() if name != "rollout.py") <= 2      # (tensor itself, and refill_trial_walk's index)


def _optimised(name):
    """a module of the layer compiled as `python -OO` compiles it and executed in this process, in its package"""
    path = os.path.join(PKG, name)
    mod = types.ModuleType(cm.rollout.__package__ + "._optimised_" + name[:-3])
    mod.__package__ = cm.rollout.__package__
    exec(compile(open(path).read(), path, "exec", optimize=2), mod.__dict__)
    return mod


@pytest.mark.parametrize("optimised", [True, False], ids=["optimize=2", "as imported"])
def test_the_pure_checks_raise_with_their_texts(optimised):
    common = _optimised("rollout_common.py") if optimised else cm.rollout_common
    rollout = _optimised("rollout.py") if optimised else cm.rollout
    assert common.walk_schedule(14, 5, {7: None}) == ([(0, 5), (5, 7), (7, 10), (10, 14)], [5, 10])
    for bad in ((0, None), (3, 0), (3, None, (), -1)):
        with pytest.raises(AssertionError, match=r"^walk_schedule: ticks >= 1, tick0 >= 0, every >= 1$"):
            common.walk_schedule(*bad)
    with pytest.raises(AssertionError, match=r"^a text$"):
        common.need(False, "a text")
    assert common.need(True, "a text") is None
    # set_references on a bare object: the argument rule, then the shape rule behind the one conversion
    ro = types.SimpleNamespace(torch=torch, dev=torch.device("cpu"), B=3, references="untouched")
    with pytest.raises(AssertionError, match=r"^set_references\(com, h, in_dt, \.\.\.\)$"):
        rollout.WalkingRollout.set_references(ro, np.zeros((3, 4, 3)))
    with pytest.raises(AssertionError, match=r"^set_references: com and h of shape \[3, n >= 2, 3\]$"):
        rollout.WalkingRollout.set_references(ro, np.zeros((2, 4, 3)), np.zeros((2, 4, 3)), in_dt=0.1)
    assert ro.references == "untouched"
    rollout.WalkingRollout.set_references(ro, np.zeros((3, 4, 3)), torch.zeros((3, 4, 3), dtype=torch.float64), in_dt=0.1)
    assert ro.references["com"].dtype == ro.references["h"].dtype == torch.float32 and ro.references["in_dt"] == 0.1
    # the refusals that more than one method raises: one text each
    with pytest.raises(NotImplementedError, match=r"^who: lists longer than 16 contacts are out of scope of a refill walk$"):
        common.refuse_long_lists("who", 17)
    with pytest.raises(NotImplementedError, match=r"^who: lists longer than 16 contacts are out of scope \(why\)$"):
        common.refuse_long_lists("who", 17, " (why)")
    with pytest.raises(ValueError, match=r"^who: push or wrench_trials, not both$"):
        common.refuse_push_and_wrench_trials("who", 1, 2)
    with pytest.raises(ValueError, match=r"^push= with a sensor: a known push and a sensed one are not summed \(hidden_wrench is what the sensor reads\)$"):
        common.refuse_push_with_sensor({}, 1)
    assert common.refuse_long_lists("who", 16) is None and common.refuse_push_and_wrench_trials("who", None, 2) is None
    assert common.refuse_push_with_sensor(None, 1) is None and common.refuse_push_with_sensor({}, None) is None
    with pytest.raises(AssertionError, match=r"^direction of shape \(3, 2, 8\): expected \(3, 'k', 9\)$"):
        common.direction(np.zeros((3, 2, 8)), "cpu", 3, torch.float64, (9,))
    assert common.direction(None, "cpu", 3, torch.float64, (9,)) is None


def test_the_one_conversion_adds_no_copy():
    t = torch.zeros((2, 3), dtype=torch.float64)
    assert cm.rollout_common.tensor(t, "cpu", torch.float64) is t
    a = np.arange(6.0).reshape(2, 3)
    assert cm.rollout_common.tensor(a, "cpu", torch.float64).data_ptr() == a.ctypes.data                 # (from_numpy shares the array's memory)
    got = cm.rollout_common.tensor(a.T, "cpu", torch.float32, np.float32)
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, torch.from_numpy(a.T.copy()).to(torch.float32))
    bound = cm.rollout_common.bound(cm.WalkingRollout.walk_device, None, 3, 1, 2, 3, trace=False)
    assert bound.args[1:5] == (3, 1, 2, 3) and bound.arguments["trace"] is False and bound.arguments["push_ticks"] == 0
