"""Developer probe (GPU box): what the device tape of a walk costs and what the reverse walk saves.
N = 20, 60 ticks, B = 256 and B = 1024, in one process after a warm-up; the variants alternate, three repeats each, the median kept, whole-call wall clock
(the call ends in a device synchronise) divided by the ticks, set-up included on every side:
    (a) walk_device_taped() against walk_device(): what the tape costs per tick -- one copy kernel and the multiplier kernel.  Reported, no threshold.
    (b) walk_device_taped() + backward_device against run(tape=True, record="light", timing=False) + backward(), seeds on every state: the Python loop
        of clones and synchronisations it replaces.  Expected <= 1.0; if it is not, the line says so and nothing is tuned around it.
    (c) with --baseline LIB (another build of the library in the package directory, e.g. the parent commit's): the untaped path must not pay.  The headline
        solve of bench.py through tools/ab_multi.sh, and walk_device() untaped at both batch sizes, both builds in turn in child processes started before
        this one touches the GPU.   bound: this build / LIB <= 1.01 (three times the 0.3 % in-call spread README.md records for ab_multi.sh runs)
The verdict is printed, and the exit status is 1 when the bound of (c) is missed.  Writes its lines to --out (default profiles/r07_walk_tape.txt) as well."""
import argparse, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_walk_tape.txt"))
ap.add_argument("--ticks", type=int, default=60)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--baseline", default=None, help="file name of another build of the library in the package directory: part (c)")
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--child-walk", action="store_true", help="internal: time walk_device() untaped with the library CMPC_LIB names and print the medians")
args = ap.parse_args()
BOUND = 1.01
T, lines, missed = args.ticks, [], []
SIZES = (256, 1024)


def say(s):
    print(s, flush=True)
    lines.append(s)


def check(name, ratio):
    good = ratio <= BOUND
    if not good:
        missed.append(name)
    return f"{ratio:.4f} ({'within' if good else 'ABOVE'} the bound {BOUND})"


def start(cm, B):
    rng = np.random.default_rng(5)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    return com0, dcom0, h0, push


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / T, r


if args.child_walk:
    import torch
    import cmpc_amd as cm
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    for B in SIZES:
        com0, dcom0, h0, push = start(cm, B)
        ro = cm.rollout.WalkingRollout(cfg, B)
        ro.walk_device(8, com0, dcom0, h0, push=push, push_ticks=3)
        ms = [timed(torch, lambda: ro.walk_device(T, com0, dcom0, h0, push=push, push_ticks=3))[0] for _ in range(args.repeats)]
        print("walk", B, float(np.median(ms)))
    sys.exit(0)

ab, abw = None, None
if args.baseline:      # (c) first: fresh child processes, this one has not opened the GPU yet
    libs = [args.baseline, "libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True).stdout
    ab = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab:
            ab[w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab.values()), out
    abw = {(lib, B): [] for lib in libs for B in SIZES}
    for _ in range(args.ab_reps):
        for lib in libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-walk", "--ticks", str(T), "--repeats", str(args.repeats)], cwd=ROOT,
                               capture_output=True, text=True, env=dict(os.environ, CMPC_LIB=lib))
            assert o.returncode == 0, o.stderr[-2000:]
            for ln in o.stdout.splitlines():
                w = ln.split()
                if len(w) == 3 and w[0] == "walk":
                    abw[(lib, int(w[1]))].append(float(w[2]))
    assert all(len(v) == args.ab_reps for v in abw.values()), abw

import torch
import cmpc_amd as cm

cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)
med = lambda a: float(np.median(a))
L = cm.Layout(cfg.N)
say(f"the device walk taped and run in reverse: N = {cfg.N}, {T} ticks, variants alternating, median of {args.repeats} repeats, ms per tick (whole call / "
    f"ticks); {torch.cuda.get_device_name(0)}")
for B in SIZES:
    com0, dcom0, h0, push = start(cm, B)
    ro, ro_run, ro_plain = (cm.rollout.WalkingRollout(cfg, B) for _ in range(3))      # (ro_plain never tapes: its multiplier output stays off)
    gS = torch.from_numpy(np.random.default_rng(1).normal(size=(T + 1, B, 9))).cuda()
    walk = lambda tape: ro.walk_device_taped(T, com0, dcom0, h0, push=push, push_ticks=3) if tape else ro_plain.walk_device(T, com0, dcom0, h0, push=push, push_ticks=3)

    def device_pair():
        w = walk(True)
        return w, ro.backward_device(w, gS)

    def host_pair():
        rec = ro_run.run(T, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False, tape=True)
        return rec, ro_run.backward(rec["tape"], gS)
    # warm-up (module load, allocator, the workspaces of both reverse paths)
    ro_plain.walk_device(8, com0, dcom0, h0, push=push, push_ticks=3)
    w8 = ro.walk_device_taped(8, com0, dcom0, h0, push=push, push_ticks=3)
    ro.backward_device(w8, gS[:9])
    r8 = ro_run.run(8, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False, tape=True)
    ro_run.backward(r8["tape"], gS[:9])
    ms = {k: [] for k in ("plain", "taped", "device", "host")}
    last = {}
    for _ in range(args.repeats):
        for k, fn in (("plain", lambda: walk(False)), ("taped", lambda: walk(True)), ("device", device_pair), ("host", host_pair)):
            t, last[k] = timed(torch, fn)
            ms[k].append(t)
    m = {k: med(v) for k, v in ms.items()}
    same_walk = all(torch.equal(last["plain"][k], last["taped"][k]) for k in ("X", "state", "iterations", "end_tick"))
    rec, ref = last["host"]
    w, got = last["device"]
    same_grad = len(rec["tape"]["ticks"]) == T and all(torch.equal(got[k], ref[k]) for k in ("state0", "list0", "wrench", "push", "models", "plan", "status"))
    assert same_walk, "the taped walk differs from the untaped one"
    bytes_row = 4 * (L.nx + L.np + L.ng) + 64 * ro.M + 96
    say(f"B = {B} (a) walk_device untaped {m['plain']:.4f} ({fmt(ms['plain'])}) | taped {m['taped']:.4f} ({fmt(ms['taped'])}) | taped / untaped = "
        f"{m['taped'] / m['plain']:.4f}, the tape costs {1e3 * (m['taped'] - m['plain']):.1f} us per tick ({bytes_row} bytes per problem and tick, "
        f"{bytes_row * B * T / 2**20:.1f} MiB in all) | bit-identical walks: {same_walk}")
    say(f"B = {B} (b) walk_device_taped() + backward_device {m['device']:.4f} ({fmt(ms['device'])}) | run(tape=True) + backward() {m['host']:.4f} "
        f"({fmt(ms['host'])}) | device / host loop = {m['device'] / m['host']:.4f}"
        + ("" if m["device"] <= m["host"] else "  ABOVE 1.0: the device pair is slower here; reported as measured, nothing tuned around it")
        + f" | gradients bit-identical: {same_grad}; ended problems {int((w['end_tick'] >= 0).sum())}, aborted tick of run() {rec.get('aborted_tick')}")
if ab:
    new, old = med(ab["libcmpc_hip.so"]), med(ab[args.baseline])
    say(f"(c) headline solve (bench.py config2 through tools/ab_multi.sh, {args.ab_reps} rounds), ms per step: {args.baseline} {old:.4f} "
        f"({fmt(ab[args.baseline])}) | this build {new:.4f} ({fmt(ab['libcmpc_hip.so'])}) | this build / baseline = {check('(c) solve', new / old)}")
    for B in SIZES:
        new, old = med(abw[("libcmpc_hip.so", B)]), med(abw[(args.baseline, B)])
        say(f"(c) walk_device() untaped, B = {B}, child processes alternating, {args.ab_reps} rounds of the median of {args.repeats}, ms per tick: "
            f"{args.baseline} {old:.4f} ({fmt(abw[(args.baseline, B)])}) | this build {new:.4f} ({fmt(abw[('libcmpc_hip.so', B)])}) | this build / baseline = "
            f"{check(f'(c) walk B = {B}', new / old)}")
else:
    say("(c) not run (no --baseline)")
say("verdict: " + ("bound missed: " + "; ".join(missed) if missed else "every bound holds"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if missed else 0)
