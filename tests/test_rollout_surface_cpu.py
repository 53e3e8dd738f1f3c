"""No GPU: the Python surface of the rollout module -- WalkingRollout and the module's functions and names -- against tests/golden/rollout_surface.json,
which tools/solver_surface.py (--module rollout --classes WalkingRollout --names) recorded at the commit before rollout.py was split into rollout.py,
rollout_walk.py, rollout_refill.py, rollout_grad.py, rollout_autograd.py and rollout_common.py.  The rules are tests/test_solver_surface_cpu.py's: names
that do not start with "_" must match the record exactly and no new one may appear; a name with one leading underscore must still exist with the same
kind and may only have gained trailing parameters with defaults; a function may have moved to another module as long as rollout.<name> reaches it."""
import inspect
import json
import os
import sys

import cmpc_amd as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import solver_surface  # noqa: E402
from tests.test_solver_surface_cpu import _params  # noqa: E402

GOLDEN = json.load(open(solver_surface.golden("rollout")))
NOW = solver_surface.surface("rollout", ("WalkingRollout",), names=True)
LAYERS = (cm.rollout_common.LaunchStream, cm.rollout_walk.DeviceWalks, cm.rollout_refill.RefillWalks, cm.rollout_grad.WalkGrads)


def _now(owner, name):
    """the record of a name today; a function that moved to another module is read through rollout.<name>"""
    if owner == "functions" and name not in NOW[owner] and hasattr(cm.rollout, name):
        return solver_surface._record(cm.rollout, name)
    assert name in NOW[owner], f"{owner}.{name} is gone"
    return NOW[owner][name]


def test_public_names_signatures_and_properties_are_the_recorded_ones():
    assert sorted(NOW) == sorted(GOLDEN) == ["WalkingRollout", "functions", "names"]
    public = lambda names: {n: r for n, r in names.items() if not n.startswith("_")}
    assert public(GOLDEN["WalkingRollout"]) == public(NOW["WalkingRollout"])
    assert public(GOLDEN["functions"]) == {n: _now("functions", n) for n in public(GOLDEN["functions"])}
    assert not set(public(NOW["functions"])) - set(GOLDEN["functions"]), "a new public function in rollout.py"
    assert len(public(GOLDEN["WalkingRollout"])) == 36 and len(public(GOLDEN["functions"])) == 9


def test_private_names_still_exist_and_only_gained_defaulted_parameters():
    for owner in ("WalkingRollout", "functions"):
        for n, rec in GOLDEN[owner].items():
            if not n.startswith("_"):
                continue
            now = _now(owner, n)
            assert now["property"] == rec["property"] and ("signature" in now) == ("signature" in rec), f"{owner}.{n}"
            if "signature" in rec:
                old, new = _params(rec["signature"]), _params(now["signature"])
                assert new[:len(old)] == old and all("=" in p for p in new[len(old):]), f"{owner}.{n}: {rec['signature']} -> {now['signature']}"


def test_every_name_of_the_module_is_still_reached_through_it():
    """rollout.<name> for every name the module had"""
    missing = [n for n in GOLDEN["names"] if not hasattr(cm.rollout, n)]
    assert missing == [] and len(GOLDEN["names"]) >= 24, missing
    assert cm.WalkingRollout is cm.rollout.WalkingRollout
    for name in ("walk_schedule", "rollout_differentiable", "rollout_differentiable_checkpointed", "rollout_differentiable_checkpointed_mismatch",
                 "rollout_differentiable_measures"):
        assert getattr(cm, name) is getattr(cm.rollout, name), name
    assert cm.rollout.walk_schedule is cm.rollout_common.walk_schedule and cm.rollout._jr_transposed is cm.rollout_autograd._jr_transposed
    assert "from .rollout import walking_plan" in inspect.getsource(cm.synthetic) and callable(cm.rollout.walking_plan)
    assert "from .solver import BatchSolver, _model_array, _upload" in inspect.getsource(cm.rollout)


def test_the_layers_are_base_classes_without_state_and_a_method_lives_with_its_family():
    """the placement rule: WalkingRollout's own dict holds the constructor, limits, references and the host-stepped path; a
    device walk is DeviceWalks', a refill walk (and what regroups its tape) RefillWalks', a device derivative WalkGrads'"""
    for base in LAYERS:
        assert issubclass(cm.WalkingRollout, base) and "__init__" not in vars(base), base
    assert "__init__" in vars(cm.WalkingRollout)
    own = {n for n, f in vars(cm.WalkingRollout).items() if inspect.isfunction(f)}
    assert own == {"__init__", "set_limits", "clear_limits", "_limits_on", "_limits_off", "set_references", "_planner_refs", "run", "_run", "_tick_by_steps",
                   "backward", "forward_sensitivity"}
    home = {n: base for base in LAYERS for n in vars(base) if not n.startswith("__")}
    for n in GOLDEN["WalkingRollout"]:
        if n in own:
            continue
        want = (cm.rollout_refill.RefillWalks if "refill" in n or n.startswith(("plan_", "_plan_")) else
                cm.rollout_grad.WalkGrads if n.lstrip("_").startswith(("backward_", "forward_sensitivity_", "sensed_tape")) else
                cm.rollout_common.LaunchStream if n == "_queued" else cm.rollout_walk.DeviceWalks)
        assert home.get(n) is want, f"{n} is defined in {home.get(n)}, its family is {want.__name__}"
    for n in ("_planner_refs", "_mismatch_of", "_push_schedule", "_walk_refill_trials", "_queued"):      # (read or patched on an instance by tests and tools)
        assert inspect.isfunction(inspect.getattr_static(cm.WalkingRollout, n)), n
