"""GPU: the device walks of WalkingRollout against the bits of the commit before its walk drivers were merged into one.  tools/walk_digests.py runs a
fixed list of tiny walks -- plain, skip_ended, taped under a mismatch, checkpointed, resumed with a forking index, and the five refill forms, two of
them with the measures on -- and takes a SHA-256 of every tensor they return; tests/golden/walk_digests.json holds what that tool printed on the tree of
the commit named in the file (taken twice there, equal both times).  The device walks are deterministic between handles of the same batch size and
factor storage, so there is no tolerance: a digest that differs means the roll-out layer computes something else.  Word 6 of info, the
clock, is left out by the tool."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join("tools", "walk_digests.py")
GOLDEN = os.path.join("tests", "golden", "walk_digests.json")


def test_every_walk_has_the_reference_commits_bits():
    spec = importlib.util.spec_from_file_location("walk_digests", os.path.join(ROOT, TOOL))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, GOLDEN)) as f:
        want = json.load(f)
    assert len(want["cases"]) == 14 and all(want["cases"].values())
    lines = tool.differences(tool.compute(), want["cases"])
    assert not lines, (f"{len(lines)} keys differ from {GOLDEN} (commit {want['commit'][:7]}, ROCm {want['rocm']}); `python {TOOL} --check {GOLDEN}` "
                       "lists them:\n" + "\n".join(lines))
