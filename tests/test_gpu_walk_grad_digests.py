"""GPU: the derivatives and autograd wrappers of the roll-out layer against the bits of the commit before rollout.py was split by layer.
tools/walk_digests.py --set grads runs a fixed list of tiny cases on the shapes of tests/test_gpu_walk_digests.py -- the reverse device walk (plain, with
orientations, references, measures, checkpointed, sensed, per refill trial), the forward-mode walk in k = 2 columns (plain, references, mismatch,
measures, sensed), run() + backward() + forward_sensitivity(), and the four rollout_differentiable* functions through .backward() and forward_ad -- and
takes a SHA-256 of every tensor they return; tests/golden/walk_grad_digests.json holds what the tool printed on the tree of the commit named in the
file (taken twice there, equal both times).  No tolerance: the existing tests hold the device derivatives to the host ones to the bit, so a digest
that differs means the layer computes something else.  State seeds carry a NaN behind the end of the problem that ends."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join("tools", "walk_digests.py")
GOLDEN = os.path.join("tests", "golden", "walk_grad_digests.json")


def test_every_derivative_has_the_reference_commits_bits():
    spec = importlib.util.spec_from_file_location("walk_digests", os.path.join(ROOT, TOOL))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, GOLDEN)) as f:
        want = json.load(f)
    assert want["set"] == "grads" and len(want["cases"]) == 26 and all(want["cases"].values())
    lines = tool.differences(tool.compute("grads"), want["cases"])
    assert not lines, (f"{len(lines)} keys differ from {GOLDEN} (commit {want['commit'][:7]}, ROCm {want['rocm']}); `python {TOOL} --set grads --check "
                       f"{GOLDEN}` lists them:\n" + "\n".join(lines))
