"""The passes of an iteration beside the sweeps -- the corrector (delta) sweep on wave 0, the residual pass, the two fused passes behind the forward sweeps -- checked in
the compiled code (one device-only compile of csrc/cmpc_solver.hip to gfx950 assembly, no GPU; skipped without hipcc).

Each of them is as long as the instruction stream of its longest wave, so what is held is what that wave pays for:

  * the resident corrector sweep keeps inside the caller-saved registers: no scratch_ instruction.  Its parent saved 25 callee-saved registers at entry and restored
    them, behind a wait on memory, at exit -- on wave 0, every iteration, with seven waves at the barrier;
  * the HBM-factor instantiations (held to 168 registers) use no more scratch_ instructions than the parent;
  * no resident instantiation of the four functions has more instructions than the parent.

PARENT_* are the counts of commit a5f4938 (the parent of the change that added this file), same compiler flags, counted with tools/lds_wait_census.py."""
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

FUNCTIONS = ("phase_delta_part", "phase_residuals", "phase_affine_post", "phase_final_post")
HORIZONS = (10, 12, 13, 15, 20, 22)
RESIDENT = [(512, n, 0) for n in HORIZONS + (0,)]      # (threads, horizon or 0 = runtime-N, HBM-factor)
HBM_FACTOR = [(256, 20, 1), (256, 30, 1), (256, 0, 1)]
# (the two fused passes exist for compile-time horizons only)
INSTANCES = {"phase_delta_part": RESIDENT + HBM_FACTOR, "phase_residuals": RESIDENT + HBM_FACTOR,
             "phase_affine_post": [i for i in RESIDENT + HBM_FACTOR if i[1] > 0], "phase_final_post": [i for i in RESIDENT + HBM_FACTOR if i[1] > 0]}

# commit a5f4938: scratch_ instructions of the HBM-factor instantiations (every other function and instantiation: 0, but the resident corrector sweep's 50)
PARENT_SCRATCH = {("phase_delta_part", (256, 20, 1)): 84, ("phase_delta_part", (256, 30, 1)): 84, ("phase_delta_part", (256, 0, 1)): 72}
# commit a5f4938: instructions of the resident instantiations
PARENT_INSTRUCTIONS = {
    "phase_delta_part": {10: 1359, 12: 1094, 13: 1286, 15: 1359, 20: 1094, 22: 1359, 0: 636},
    "phase_residuals": {10: 962, 12: 962, 13: 964, 15: 969, 20: 1026, 22: 1050, 0: 1110},
    "phase_affine_post": {10: 514, 12: 514, 13: 514, 15: 514, 20: 672, 22: 672},
    "phase_final_post": {10: 1373, 12: 1373, 13: 1373, 15: 1524, 20: 1549, 22: 1551},
}


@pytest.fixture(scope="module")
def passes(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "solver.s"
    flags = [f for f in ge.FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-S"]
    p = subprocess.run([ge.HIPCC] + flags + [os.path.join(ge.CSRC, "cmpc_solver.hip"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]
    found = {}
    for name, body in census.functions(out.read_text(), r"^(%s)<\d+,\d+,[01]>$" % "|".join(FUNCTIONS)).items():
        fn = name.split("<")[0]
        nt, nc, fg = (int(x) for x in re.findall(r"\d+", name.split("<")[1]))
        found[(fn, (nt, nc, fg))] = body
    return found


def _scratch(body):
    return len(re.findall(r"^\s+scratch_", body, re.M))


def _ids(cases):
    return ["%s-NT%d-N%d-G%d" % ((fn,) + inst) for (fn, inst) in cases]


def test_every_instantiation_is_there(passes):
    want = {(fn, inst) for fn in FUNCTIONS for inst in INSTANCES[fn]}
    assert set(passes) == want, sorted(set(passes) ^ want)


@pytest.mark.parametrize("inst", RESIDENT, ids=lambda i: "NT%d-N%d-G%d" % i)
def test_resident_corrector_sweep_uses_no_scratch(passes, inst):
    n = _scratch(passes[("phase_delta_part", inst)])
    print(inst, "scratch_ instructions:", n)
    assert n == 0, (inst, n)


_HBM_CASES = [(fn, inst) for fn in FUNCTIONS for inst in INSTANCES[fn] if inst[2] == 1]


@pytest.mark.parametrize("fn,inst", _HBM_CASES, ids=_ids(_HBM_CASES))
def test_hbm_factor_passes_add_no_scratch(passes, fn, inst):
    n = _scratch(passes[(fn, inst)])
    print(fn, inst, "scratch_ instructions:", n, "parent:", PARENT_SCRATCH.get((fn, inst), 0))
    assert n <= PARENT_SCRATCH.get((fn, inst), 0), (fn, inst, n)


_RESIDENT_CASES = [(fn, inst) for fn in FUNCTIONS for inst in INSTANCES[fn] if inst[2] == 0]


@pytest.mark.parametrize("fn,inst", _RESIDENT_CASES, ids=_ids(_RESIDENT_CASES))
def test_resident_passes_have_no_more_instructions_than_the_parent(passes, fn, inst):
    n = census.tokens(passes[(fn, inst)])[1]
    parent = PARENT_INSTRUCTIONS[fn][inst[1]]
    print(fn, inst, "instructions:", n, "parent:", parent, "scratch_:", _scratch(passes[(fn, inst)]))
    assert n <= parent, (fn, inst, n, parent)
    assert _scratch(passes[(fn, inst)]) == 0, (fn, inst)


def test_kernel_registers_and_private_segment_do_not_grow(passes, tmp_path_factory):
    """.vgpr_count and .private_segment_fixed_size of every cmpc_solve_kernel instantiation against commit a5f4938."""
    parent = {(256, 30, 1): (168, 392), (256, 0, 1): (168, 404), (256, 20, 1): (168, 392), (512, 0, 0): (248, 264)}
    parent.update({(512, n, 0): (248, 352) for n in HORIZONS})
    text = next(tmp_path_factory.getbasetemp().glob("isa*/solver.s")).read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+\S*cmpc_solve_kernelILi(\d+)ELi(\d+)ELb([01])E\S*\n(.*?)\.wavefront_size", text, re.S):
        inst = (int(m.group(1)), int(m.group(2)), int(m.group(3)))
        seen[inst] = (int(re.search(r"\.vgpr_count:\s+(\d+)", m.group(4)).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(4)).group(1)))
    assert set(seen) == set(parent), sorted(seen)
    for inst, (vg, ps) in seen.items():
        print(inst, "vgpr_count", vg, "private_segment_fixed_size", ps, "parent", parent[inst])
        assert vg <= parent[inst][0] and ps <= parent[inst][1], (inst, vg, ps, parent[inst])
