#!/usr/bin/env python3
"""The Python surface of one module of the package as JSON: for the named classes (as reached through <package>.<module>) every attribute name that
does not start with "__", with str(inspect.signature(...)) for callables and whether it is a property; and the same for the functions the module
defines.  The default is the solver module with BatchSolver, CentroidalMPC, CentroidalMPCOutput: tests/golden/solver_surface.json is that output at the
commit before solver.py was split by layer, and tests/test_solver_surface_cpu.py holds every later tree to it.  tests/golden/rollout_surface.json is
    python tools/solver_surface.py --module rollout --classes WalkingRollout --names
at the commit before rollout.py was split by layer (--names adds every name of vars(module) that does not start with "__"), held by
tests/test_rollout_surface_cpu.py.  To record a parent commit, copy this file into a checkout of it, as tools/walk_digests.py's header says of its own.

    python tools/solver_surface.py [--module M --classes A,B --names]            # prints the record
    python tools/solver_surface.py [--module M --classes A,B --names] --write    # rewrites tests/golden/<M>_surface.json (only when the surface is
                                                                                 # MEANT to change)
"""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "solver_surface.json")
CLASSES = ("BatchSolver", "CentroidalMPC", "CentroidalMPCOutput")


def golden(module):
    return os.path.join(ROOT, "tests", "golden", f"{module}_surface.json")


def _record(owner, name):
    static = inspect.getattr_static(owner, name)
    rec = {"property": isinstance(static, property)}
    value = getattr(owner, name)
    if callable(value) and not rec["property"]:
        rec["signature"] = str(inspect.signature(value))
    return rec


def surface(module="solver", classes=CLASSES, names=False):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import cmpc_amd as cm
    mod = getattr(cm, module)
    out = {c: {n: _record(getattr(mod, c), n) for n in dir(getattr(mod, c)) if not n.startswith("__")} for c in classes}
    out["functions"] = {n: _record(mod, n) for n, f in sorted(vars(mod).items())
                        if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("__")}
    if names:
        out["names"] = sorted(n for n in vars(mod) if not n.startswith("__"))
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    value = lambda flag, default: argv[argv.index(flag) + 1] if flag in argv else default
    module = value("--module", "solver")
    text = json.dumps(surface(module, tuple(value("--classes", ",".join(CLASSES)).split(",")), "--names" in argv), indent=1, sort_keys=True) + "\n"
    if "--write" in argv:
        with open(golden(module), "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
