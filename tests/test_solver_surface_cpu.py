"""No GPU: the Python surface of the solver module -- BatchSolver, CentroidalMPC, CentroidalMPCOutput and the module's functions -- against
tests/golden/solver_surface.json, which tools/solver_surface.py recorded at the commit before solver.py was split into solver.py, solver_rollout.py,
solver_walk_grad.py and facade.py: every name, every signature, every property.  Names that do not start with "_" must match the record exactly, and no
new one may appear.  A name with one leading underscore must still exist with the same kind; a helper may have gained trailing parameters that have
defaults (_launch's name=, _nlp_out's what= / lam=, and _opt, now the module function without self), nothing else, and new helpers may exist; a module
function may have moved to a leaf module as long as solver.<name> still reaches it (_upload, now in _args.py)."""
import inspect
import json
import os
import sys

import cmpc_amd as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import solver_surface  # noqa: E402

GOLDEN = json.load(open(solver_surface.GOLDEN))
NOW = solver_surface.surface()


def _params(signature):
    """the parameter texts of "(a, b=1, *c)" without a leading self"""
    inner = signature.strip()[1:-1]
    parts, depth, cur = [], 0, ""
    for ch in inner:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur.strip())
    return parts[1:] if parts[:1] == ["self"] else parts


def test_public_names_signatures_and_properties_are_the_recorded_ones():
    assert sorted(NOW) == sorted(GOLDEN)
    for owner, names in GOLDEN.items():
        public = {n: r for n, r in names.items() if not n.startswith("_")}
        assert public == {n: r for n, r in NOW[owner].items() if not n.startswith("_")}, owner
    assert len(GOLDEN["BatchSolver"]) >= 90 and len(GOLDEN["CentroidalMPC"]) >= 10 and len(GOLDEN["functions"]) == 5


def test_private_names_still_exist_and_only_gained_defaulted_parameters():
    for owner, names in GOLDEN.items():
        for n, rec in names.items():
            if not n.startswith("_"):
                continue
            if owner == "functions" and n not in NOW[owner] and hasattr(cm.solver, n):
                now = solver_surface._record(cm.solver, n)      # (a helper that moved to a leaf module and is still reached as solver.<name>)
            else:
                assert n in NOW[owner], f"{owner}.{n} is gone"
                now = NOW[owner][n]
            assert now["property"] == rec["property"] and ("signature" in now) == ("signature" in rec), f"{owner}.{n}"
            if "signature" in rec:
                old, new = _params(rec["signature"]), _params(now["signature"])
                assert new[:len(old)] == old and all("=" in p for p in new[len(old):]), f"{owner}.{n}: {rec['signature']} -> {now['signature']}"


def test_params_splits_defaults_that_hold_commas():
    assert _params("(self, a, stop=('merge', 'solver'), b=None)") == ["a", "stop=('merge', 'solver')", "b=None"]
    assert _params("(t, dtype)") == ["t", "dtype"] and _params("()") == []


def test_names_reached_from_outside_resolve_where_they_are_reached():
    """what tests, tools and rollout.py import or read today"""
    for name in ("_c_config", "_model_array", "_upload", "BatchSolver", "CentroidalMPC", "CentroidalMPCOutput", "rotate_parameters", "solve_differentiable"):
        assert hasattr(cm.solver, name), name
    assert cm.BatchSolver is cm.solver.BatchSolver and cm.CentroidalMPC is cm.solver.CentroidalMPC is cm.facade.CentroidalMPC
    assert cm.solver.CentroidalMPCOutput is cm.facade.CentroidalMPCOutput
    for name in ("_launch", "_tick_io", "_opt", "_stream_pair", "_box_arrays", "_dev", "launch_stream", "last_error"):
        assert hasattr(cm.BatchSolver, name), name
    # the two layers are base classes without state: no __init__ of their own, and every method of theirs is BatchSolver's
    for base in (cm.solver_rollout.RolloutCalls, cm.solver_walk_grad.WalkGradCalls):
        assert issubclass(cm.BatchSolver, base) and "__init__" not in vars(base)
    src = inspect.getsource(cm.rollout)
    assert "from .solver import BatchSolver, _model_array, _upload" in src


def test_a_method_lives_in_the_module_named_after_its_c_file():
    """every cmpc_* symbol a method body names is defined in the C file its module mirrors (a symbol in a docstring does not count)"""
    import ast
    import re
    csrc = os.path.join(ROOT, "paper_romualdi_2022_icra_centroidal-mpc-walking_amd", "csrc")
    where = {}
    for cfile in ("cmpc_api.hip", "cmpc_api_rollout.hip", "cmpc_api_walk_grad.hip"):
        for m in re.finditer(r"^[A-Za-z_][\w \*]*?\b(cmpc_\w+)\s*\(", open(os.path.join(csrc, cfile)).read(), re.M):
            where.setdefault(m.group(1), cfile)
    pairs = (("solver.py", "cmpc_api.hip"), ("solver_rollout.py", "cmpc_api_rollout.hip"), ("solver_walk_grad.py", "cmpc_api_walk_grad.hip"))
    seen = 0
    for pyfile, cfile in pairs:
        tree = ast.parse(open(os.path.join(os.path.dirname(csrc), pyfile)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and node.attr.startswith("cmpc_") and isinstance(node.value, ast.Attribute) and node.value.attr == "_lib":
                if node.attr in where:     # (cmpc_sensitivity_workspace_bytes and the like live in other C files)
                    assert where[node.attr] == cfile, f"{pyfile} calls {node.attr}, which {where[node.attr]} defines"
                    seen += 1
    assert seen >= 80
