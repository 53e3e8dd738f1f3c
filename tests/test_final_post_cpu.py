"""The fused passes of a resident iteration -- phase_residuals, phase_affine_post, phase_final_post -- in their lean form, checked in the compiled code (one device-only
compile of csrc/cmpc_solver.hip to gfx950 assembly, no GPU; skipped without hipcc).

PARENT_* are the figures of commit 814b6e6 (the parent of the change that added this file), same compiler flags, counted with tools/lds_wait_census.py.

Workgroup barriers per pass, resident eight-wave instantiations with a compile-time horizon (kLeanPasses in the source):

  phase_residuals    1   the barrier of its one reduction.  The barrier in front of the slot writes is gone: c.red was last read in phase_final_post's first reduction,
                         in front of the barrier of its second one (which uses the second slot set, c.red1); c.redd in front of the closing barrier of
                         phase_affine_post / phase_multipliers.  (parent: 2)
  phase_affine_post  4   the barrier it starts with (the sweep is complete), one per reduction (step lengths: c.red; mu_aff: c.redd -- both last read in front of the
                         starting barrier), the closing barrier (targets visible to the corrector sweep).  (parent: 6)
  phase_final_post   3   the barrier it starts with, one for the step lengths (c.red), one for the step norm (c.red1: a slower wave may still be reading c.red).
                         None inside the role branch (costate waves / row waves): every wave executes the same three.  (parent: 5)

The HBM-factor instantiations (four waves) and the runtime-N instantiation keep the parent's form: two barriers per reduction, the costates on one wave."""
import hashlib
import os
import re
import shutil
import subprocess
import sys

import pytest

import __graft_entry__ as ge

sys.path.insert(0, os.path.join(ge.ROOT, "tools"))
import lds_wait_census as census  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(ge.HIPCC) or shutil.which(ge.HIPCC)), reason="needs hipcc")

HORIZONS = (10, 12, 13, 15, 20, 22)
# commit 814b6e6: instructions of the resident instantiations
PARENT_INSTRUCTIONS = {
    "phase_affine_post": {10: 514, 12: 514, 13: 514, 15: 514, 20: 672, 22: 672},
    "phase_final_post": {10: 1373, 12: 1373, 13: 1373, 15: 1524, 20: 1549, 22: 1551},
}
BARRIERS = {"phase_residuals": 1, "phase_affine_post": 4, "phase_final_post": 3}
PARENT_BARRIERS = {"phase_residuals": 2, "phase_affine_post": 6, "phase_final_post": 5}
# commit 814b6e6: the instantiations that keep their form -- (instructions, sha1 of the mnemonics in program order, first 16 hex digits).  The three passes of the
# HBM-factor variants are instruction for instruction the parent's.  phase_residuals<512,0,0> (runtime N) holds the parent's instructions in another order -- the
# scheduler's, nothing in its source changed -- so its digest is taken over the SORTED mnemonics.
PARENT_KEPT = {
    "phase_affine_post<256,20,1>": (804, "ce1dae08758fbf0d"),
    "phase_affine_post<256,30,1>": (1128, "4d9de142e4a53b5a"),
    "phase_final_post<256,20,1>": (1958, "3812f359135da01f"),
    "phase_final_post<256,30,1>": (2146, "605dfde24220d0b4"),
    "phase_residuals<256,0,1>": (852, "942b28f1b6ee48b0"),
    "phase_residuals<256,20,1>": (838, "3a5ec7fa9fe88de8"),
    "phase_residuals<256,30,1>": (1004, "ff504abfdc79c90b"),
}
PARENT_KEPT_SORTED = {"phase_residuals<512,0,0>": (872, "57290208539dcb0b")}


@pytest.fixture(scope="module")
def passes(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_final_post") / "solver.s"
    flags = [f for f in ge.FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-S"]
    p = subprocess.run([ge.HIPCC] + flags + [os.path.join(ge.CSRC, "cmpc_solver.hip"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]
    return census.functions(out.read_text(), r"^(phase_residuals|phase_affine_post|phase_final_post)<\d+,\d+,[01]>$")


def _mnemonics(body):
    return [m.group(1) for m in (census._INSN.match(line) for line in body.splitlines()) if m]


def _digest(mnemonics):
    return hashlib.sha1("\n".join(mnemonics).encode()).hexdigest()[:16]


def _count(body, prefix):
    return len(re.findall(r"^\s+%s" % prefix, body, re.M))


_SHORTER = [(fn, n) for fn in sorted(PARENT_INSTRUCTIONS) for n in HORIZONS]


@pytest.mark.parametrize("fn,n", _SHORTER, ids=["%s-N%d" % c for c in _SHORTER])
def test_resident_pass_is_shorter_than_the_parent(passes, fn, n):
    count = census.tokens(passes["%s<512,%d,0>" % (fn, n)])[1]
    print(fn, n, "instructions:", count, "parent:", PARENT_INSTRUCTIONS[fn][n])
    assert count < PARENT_INSTRUCTIONS[fn][n], (fn, n, count)


def test_no_pass_uses_scratch(passes):
    for name, body in sorted(passes.items()):
        assert _count(body, "scratch_") == 0, name


def test_barriers_per_pass_are_what_the_design_says(passes):
    for name, body in sorted(passes.items()):
        fn = name.split("<")[0]
        nt, nc, fg = (int(x) for x in re.findall(r"\d+", name.split("<")[1]))
        lean = nt == 512 and nc > 0 and fg == 0
        got = _count(body, "s_barrier")
        print(name, "s_barrier:", got)
        assert got == (BARRIERS if lean else PARENT_BARRIERS)[fn], (name, got)


def test_hbm_factor_and_runtime_horizon_passes_keep_the_parents_instructions(passes):
    kept = [k for k in passes if not re.search(r"<512,[1-9]\d*,0>", k)]
    assert sorted(kept) == sorted(list(PARENT_KEPT) + list(PARENT_KEPT_SORTED)), sorted(kept)
    for name, (count, digest) in PARENT_KEPT.items():
        ops = _mnemonics(passes[name])
        assert (len(ops), _digest(ops)) == (count, digest), (name, len(ops), _digest(ops))
    for name, (count, digest) in PARENT_KEPT_SORTED.items():
        ops = sorted(_mnemonics(passes[name]))
        assert (len(ops), _digest(ops)) == (count, digest), (name, len(ops), _digest(ops))
