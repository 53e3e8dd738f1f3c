"""The forward sweep's LDS schedule, checked in the compiled code (a device-only compile of csrc/cmpc_solver.hip to gfx950 assembly, no GPU;
skipped without hipcc).  The sweep runs on one wave, so every LDS round trip it waits for in full is on the solve's critical path.

Between the store of y and the store of du a stage reads the row of y as four 16-byte reads.  Measured with tools/lds_wait_census.py
(sweep_stage_copies: per stage copy, the full waits `s_waitcnt lgkmcnt(0)` between the two stores):

    before this check existed   resident instantiations (N = 10, 12, 13, 15, 20, 22): 4 in each of the four unrolled stage copies (each read behind a wait
                                of its own, in the same destination registers), 1 in the remainder copy; runtime-N: 4 and 2;
                                HBM-factor instantiations (N = 20, 30, runtime-N): 2 and 2 (two reads per wait), runtime-N 2 and 1;
                                scratch_ instructions: resident 0; HBM-factor 68 / 68 / 62 (callee-saved registers, outside the stage loop)
    now                         resident and runtime-N: 1 in every copy (lds_ld4x4: the four reads and one wait in one block)
                                HBM-factor: still 2 -- see test_hbm_factor_du_step_keeps_its_form

The trip boundary shows in the same census: the first stage copy of a trip used to take its twenty operands two at a time, each pair behind a full wait
(27 full waits in phase_forward_part<512,20,0,1>, 13 of them behind a single read instruction; 10 and 0 now)."""
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

RESIDENT = [(512, n, 0) for n in (10, 12, 13, 15, 20, 22, 0)]     # (threads, horizon or 0 = runtime-N, HBM-factor)
HBM_FACTOR = [(256, 20, 1), (256, 30, 1), (256, 0, 1)]
# scratch_ instructions of phase_forward_part<.., 1> in the parent of the change that batched the reads
PARENT_SCRATCH = {(256, 20, 1): 68, (256, 30, 1): 68, (256, 0, 1): 62}


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "solver.s"
    flags = [f for f in ge.FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-S"]
    p = subprocess.run([ge.HIPCC] + flags + [os.path.join(ge.CSRC, "cmpc_solver.hip"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]
    found = {}
    for name, body in census.functions(out.read_text(), r"^phase_forward_part<\d+,\d+,[01],1>$").items():
        nt, nc, fg, _ = (int(x) for x in re.findall(r"\d+", name))
        found[(nt, nc, fg)] = body
    return found


def test_every_instantiation_of_the_sweep_is_there(sweeps):
    assert set(sweeps) == set(RESIDENT + HBM_FACTOR), sorted(sweeps)


def _du_step(body):
    copies = census.sweep_stage_copies(census.tokens(body)[0])
    assert len(copies) >= 2, copies                                  # (the unrolled trip and the remainder loop)
    assert all(reads == 4 for (reads, full, counted) in copies), copies
    return [full for (reads, full, counted) in copies]


@pytest.mark.parametrize("inst", RESIDENT, ids=lambda i: "NT%d-N%d-G%d" % i)
def test_resident_du_step_reads_y_in_one_round_trip(sweeps, inst):
    full = _du_step(sweeps[inst])
    print(inst, "full waits between the store of y and the store of du, per stage copy:", full)
    assert full == [1] * len(full), full


@pytest.mark.parametrize("inst", HBM_FACTOR, ids=lambda i: "NT%d-N%d-G%d" % i)
def test_hbm_factor_du_step_keeps_its_form(sweeps, inst):
    """The HBM-factor form is NOT batched: it keeps the two round trips it had (full waits per stage copy [2, 2], runtime-N [2, 1]).  Held to 168 registers,
    every batched form tried cost it scratch_ instructions -- 68 -> 120 with the block of four reads (volatile or not: 26 more callee-saved registers saved and
    restored per call), 68 -> 72 with scheduling-group barriers, which did not batch the reads either ([3, 4] full waits) -- and the register budget comes first
    (test_no_scratch_is_added).  profiles/forward_sweep_lds_waits.txt has the figures.  What is held here: no more round trips than it had."""
    full = _du_step(sweeps[inst])
    print(inst, "full waits between the store of y and the store of du, per stage copy:", full)
    assert all(f <= 2 for f in full), full


@pytest.mark.parametrize("inst", RESIDENT + HBM_FACTOR, ids=lambda i: "NT%d-N%d-G%d" % i)
def test_no_scratch_is_added(sweeps, inst):
    n = len(re.findall(r"^\s+scratch_", sweeps[inst], re.M))
    print(inst, "scratch_ instructions:", n)
    assert n <= PARENT_SCRATCH.get(inst, 0), (inst, n)
