#!/usr/bin/env python3
"""The Python surface of the solver module as JSON: for BatchSolver, CentroidalMPC, CentroidalMPCOutput (as reached through <package>.solver) every
attribute name that does not start with "__", with str(inspect.signature(...)) for callables and whether it is a property; and the same for the functions
the module defines.  tests/golden/solver_surface.json is this tool's output at the commit before solver.py was split by layer;
tests/test_solver_surface_cpu.py holds every later tree to it.

    python tools/solver_surface.py            # prints the record
    python tools/solver_surface.py --write    # rewrites tests/golden/solver_surface.json (only when the surface is MEANT to change)
"""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "solver_surface.json")
CLASSES = ("BatchSolver", "CentroidalMPC", "CentroidalMPCOutput")


def _record(owner, name):
    static = inspect.getattr_static(owner, name)
    rec = {"property": isinstance(static, property)}
    value = getattr(owner, name)
    if callable(value) and not rec["property"]:
        rec["signature"] = str(inspect.signature(value))
    return rec


def surface():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import cmpc_amd as cm
    mod = cm.solver
    out = {c: {n: _record(getattr(mod, c), n) for n in dir(getattr(mod, c)) if not n.startswith("__")} for c in CLASSES}
    out["functions"] = {n: _record(mod, n) for n, f in sorted(vars(mod).items())
                        if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("__")}
    return out


if __name__ == "__main__":
    text = json.dumps(surface(), indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
