"""Developer tool (no GPU): where a function of the solver waits for LDS.

From a device-only assembly of csrc/cmpc_solver.hip (hipcc ... --cuda-device-only -S) it prints, per function whose name matches,
the order of its LDS reads, LDS writes and lgkmcnt waits as one compact string:

    r      ds_read*            (rN: N in a row)
    W      ds_write*
    a      another LDS instruction that returns through lgkmcnt (atomics, ds_bpermute, ds_swizzle ...)
    [n]    s_waitcnt ... lgkmcnt(n)    -- [0] is a full drain: everything behind it has paid a whole LDS round trip
    |      a basic-block label (loop heads and exits)

A single-wave phase is as long as its instructions PLUS its exposed round trips: "r[0] r[0] r[0] r[0]" is four dependent round trips
(~50+ cycles each) where "r4[0]" is one.  Only the mnemonics of LDS and wait instructions are read; everything else is counted, not parsed.

    python tools/lds_wait_census.py solver.s phase_forward_part phase_delta_part
    python tools/lds_wait_census.py --summary solver.s phase_final_post phase_residuals phase_affine_post
"""
import re
import sys

_FUNC = re.compile(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end", re.M | re.S)
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")
_LABEL = re.compile(r"^\.LBB\w+:")


def short_name(sym):
    """_ZN12_GLOBAL__N_118phase_forward_partILi512ELi20ELb0ELi1EEEvPU3AS3ciPfb -> phase_forward_part<512,20,0,1>"""
    m = re.search(r"\d+([a-z_][a-z_0-9]*?)I((?:L[ib]\d+E)+)E", sym)
    if not m:
        m = re.search(r"\d+([a-z_][a-z_0-9]+)", sym)
        return m.group(1) if m else sym
    return "%s<%s>" % (m.group(1), ",".join(re.findall(r"L[ib](\d+)E", m.group(2))))


def functions(text, pattern):
    """{short name: body} of every function whose short name matches the regular expression."""
    out = {}
    for m in _FUNC.finditer(text):
        name = short_name(m.group(1))
        if re.search(pattern, name):
            out[name] = m.group(2)
    return out


def tokens(body):
    """The function's LDS reads ('r'), writes ('W'), other LDS instructions ('a'), lgkmcnt waits (int) and labels ('|'), in program order; and its instruction count."""
    toks, n = [], 0
    for line in body.splitlines():
        if _LABEL.match(line):
            toks.append("|")
            continue
        m = _INSN.match(line)
        if not m:
            continue
        n += 1
        op = m.group(1)
        if op.startswith("ds_read"):
            toks.append("r")
        elif op.startswith("ds_write"):
            toks.append("W")
        elif op.startswith("ds_"):
            toks.append("a")
        elif op == "s_waitcnt":
            w = _LGKM.search(m.group(2))
            if w:
                toks.append(int(w.group(1)))
    return toks, n


def compact(toks):
    out, i = [], 0
    while i < len(toks):
        t = toks[i]
        if t == "r":
            j = i
            while j < len(toks) and toks[j] == "r":
                j += 1
            out.append("r" if j - i == 1 else "r%d" % (j - i))
            i = j
            continue
        if isinstance(t, int):
            out[-1:] = [(out[-1] if out else "") + "[%d]" % t]
        else:
            out.append(t)
        i += 1
    return " ".join(out)


def summary(toks, n):
    full = sum(1 for t in toks if t == 0)
    part = sum(1 for t in toks if isinstance(t, int) and t > 0)
    # a "lone" full wait: exactly one read since the last wait or write of any kind -- the signature of a serialised chain
    lone, since = 0, 0
    for t in toks:
        if t == "r":
            since += 1
        elif isinstance(t, int):
            if t == 0 and since == 1:
                lone += 1
            since = 0
        elif t in ("W", "a"):
            since = 0
    return dict(instructions=n, reads=toks.count("r"), writes=toks.count("W"), full_waits=full, counted_waits=part, lone_read_full_waits=lone)


def sweep_stage_copies(toks):
    """The stage copies of a forward sweep (phase_forward_part<..,1>).  A stage ends with three stores in a row (ds+, its copy in the staging buffer, -D du);
    the two stores before them are y and du.  Per copy: (reads, full waits, counted waits) between the store of y and the store of du."""
    seq = [t for t in toks if t in ("r", "W", "a") or isinstance(t, int)]
    runs = []                              # maximal runs of stores with no other LDS instruction between them: (first, last) positions
    for i, t in enumerate(seq):
        if t != "W":
            continue
        if runs and not any(u in ("r", "a") for u in seq[runs[-1][1]:i]):
            runs[-1] = (runs[-1][0], i, runs[-1][2] + 1)
        else:
            runs.append((i, i, 1))
    out = []
    for a in range(2, len(runs)):
        if runs[a][2] == 3 and runs[a - 1][2] == 1 and runs[a - 2][2] == 1:
            mid = seq[runs[a - 2][1] + 1:runs[a - 1][0]]
            out.append((mid.count("r"), sum(1 for t in mid if t == 0), sum(1 for t in mid if isinstance(t, int) and t > 0)))
    return out


def main(argv):
    brief = "--summary" in argv
    argv = [a for a in argv if a != "--summary"]
    if len(argv) < 2:
        print(__doc__)
        return 2
    text = open(argv[0]).read()
    for pat in argv[1:]:
        for name, body in sorted(functions(text, pat).items()):
            toks, n = tokens(body)
            s = summary(toks, n)
            print("%s: %d instructions, %d LDS reads, %d writes, %d full waits [0] (%d behind a single read), %d counted waits"
                  % (name, n, s["reads"], s["writes"], s["full_waits"], s["lone_read_full_waits"], s["counted_waits"]))
            if not brief:
                print("    " + compact(toks))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
