"""Developer probe (GPU box): what the wrench sensor costs on the device walk (include/cmpc.h, "sensed pushes").  A record, not a gate: the exit status is
0 whatever it measures.  N = 20, B = 256, 24 ticks, in one process after a warm-up; the variants alternate, `--repeats` repeats each, the median kept,
whole-call wall clock (the call ends in a device synchronise) divided by the ticks, set-up included on every side:
    (a) walk_device_mismatch() against walk_device_sensed() under the same hidden pushes -- with the reference's dead-band (the MPC is told, the robots
        walk another walk and their solves take other iteration counts, reported beside it) and with the BLIND sensor (deadband = inf: the same walk to the
        bit through one sense launch more per tick -- what the launch itself costs).
    (b) the launches alone, by events around `--launches` back-to-back launches: the sense launch of one tick (rows = 1, as the walk queues it), the VJP over
        all rows and the JVP over all rows in k = 2 columns, beside one reverse tick (backward_device's wall clock / ticks).  With --trace DIR the sensed walk
        is also run under `rocprofv3 --kernel-trace --stats` in a child process started before this one touches the GPU, and the launches of this
        library's kernels in its database are summarised in the record.
    (c) with --baseline LIB [--baseline2 LIB2] (other builds of the library in the package directory: the parent commit's, twice): the headline solve of
        bench.py through tools/ab_multi.sh and walk_device(), every build in turn in child processes started before this one touches the GPU; the
        parent-against-parent ratio from the same call stands beside this-build-against-parent.
Writes its lines to --out (default profiles/r20_wrench_sensor.txt) as well."""
import argparse, glob, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_wrench_sensor.txt"))
ap.add_argument("--ticks", type=int, default=24)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--baseline", default=None, help="file name of another build of the library in the package directory: part (c)")
ap.add_argument("--baseline2", default=None, help="a second copy of the baseline build: the parent-against-parent spread of the same call")
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--trace", default=None, help="directory for a rocprofv3 kernel trace of the sensed walk: part (b)")
ap.add_argument("--child-walk", action="store_true", help="internal: time walk_device() with the library CMPC_LIB names and print the median")
ap.add_argument("--child-sensed", action="store_true", help="internal: three sensed walks, for the kernel trace")
args = ap.parse_args()
T, B, lines = args.ticks, args.batch, []


def say(s):
    print(s, flush=True)
    lines.append(s)


def start():
    rng = np.random.default_rng(5)
    return np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3)), rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.02, 0.02, (B, 3))


def pushes(torch):
    """hidden pushes on ticks 2 .. 9 of about 0.7 m/s^2 (40 N on the 56 kg robot: across the reference's dead-band of 0.7 both ways), sensor noise"""
    rng = np.random.default_rng(7)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    hidden = cu(np.concatenate([rng.normal(0, 0.45, (8, B, 3)), rng.normal(0, 0.05, (8, B, 3))], -1))
    noise = cu(np.concatenate([rng.normal(0, 0.05, (T, B, 3)), rng.normal(0, 0.01, (T, B, 3))], -1))
    return dict(hidden_wrench=hidden, force_gain=cu(rng.uniform(0.9, 1.1, B)), tick_first=2), noise


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / T, r


if args.child_walk or args.child_sensed:
    import torch
    import cmpc_amd as cm
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    com0, dcom0, h0 = start()
    ro = cm.rollout.WalkingRollout(cfg, B)
    if args.child_sensed:
        mm, noise = pushes(torch)
        sn = ro.wrench_sensor(delay=1, hold_knots=3, deadband=0.7, noise=noise)
        for _ in range(3):
            ro.walk_device_sensed(T, com0, dcom0, h0, mm, sn)
        torch.cuda.synchronize()
        sys.exit(0)
    ro.walk_device(8, com0, dcom0, h0)
    ms = [timed(torch, lambda: ro.walk_device(T, com0, dcom0, h0))[0] for _ in range(args.repeats)]
    print("walk", B, float(np.median(ms)))
    sys.exit(0)

me = [sys.executable, os.path.abspath(__file__), "--ticks", str(T), "--batch", str(B), "--repeats", str(args.repeats)]
trace_lines = []
if args.trace:      # (b), the trace: a fresh child process under the profiler, this one has not opened the GPU yet
    os.makedirs(args.trace, exist_ok=True)
    o = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "-o", "sensed", "--"] + me + ["--child-sensed"], cwd=ROOT,
                       capture_output=True, text=True)
    for path in sorted(glob.glob(os.path.join(args.trace, "**", "*.db"), recursive=True)):      # (the profiler's database: its `kernels` view)
        import collections, re, sqlite3
        per = collections.defaultdict(list)
        for name, ns in sqlite3.connect(path).execute("select name, (end - start) from kernels"):
            hit = re.search(r"cmpc_\w+", name)
            if hit:
                per[hit.group(0)].append(ns / 1e3)
        for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
            trace_lines.append(f"{name}: {len(v)} launches, mean {np.mean(v):.2f} us, median {np.median(v):.2f}, min {min(v):.2f}, max {max(v):.2f}")
    if not trace_lines:
        trace_lines.append(f"the profiler left no kernel statistics (exit status {o.returncode}): {o.stderr.strip()[-300:]}")
ab, abw = None, None
if args.baseline:      # (c): fresh child processes
    libs = [args.baseline] + ([args.baseline2] if args.baseline2 else []) + ["libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True).stdout
    ab = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab:
            ab[w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab.values()), out
    abw = {lib: [] for lib in libs}
    for _ in range(args.ab_reps):
        for lib in libs:
            o = subprocess.run(me + ["--child-walk"], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, CMPC_LIB=lib))
            assert o.returncode == 0, o.stderr[-2000:]
            for ln in o.stdout.splitlines():
                w = ln.split()
                if len(w) == 3 and w[0] == "walk":
                    abw[lib].append(float(w[2]))
    assert all(len(v) == args.ab_reps for v in abw.values()), abw

import torch
import cmpc_amd as cm

cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)
med = lambda a: float(np.median(a))
say(f"wrench sensor on the device walk: N = {cfg.N}, B = {B}, {T} ticks, variants alternating, median of {args.repeats} repeats, ms per tick (whole call / "
    f"ticks); {torch.cuda.get_device_name(0)}")
com0, dcom0, h0 = start()
mm, noise = pushes(torch)
ro, ro_t = cm.rollout.WalkingRollout(cfg, B), cm.rollout.WalkingRollout(cfg, B)      # (ro never tapes: its multiplier output stays off)
sensor = ro.wrench_sensor(delay=1, hold_knots=3, deadband=0.7, noise=noise)
blind = ro.wrench_sensor(delay=1, hold_knots=3, deadband=float("inf"), noise=noise)
gS = torch.from_numpy(np.random.default_rng(1).normal(size=(T + 1, B, 9))).cuda()


def pair():
    w = ro_t.walk_device_sensed(T, com0, dcom0, h0, mm, ro_t.wrench_sensor(delay=1, hold_knots=3, deadband=0.7, noise=noise), tape=True)
    return w, ro_t.backward_device_sensed(w, gS)


variants = (("hidden", lambda: ro.walk_device_mismatch(T, com0, dcom0, h0, mm)), ("sensed", lambda: ro.walk_device_sensed(T, com0, dcom0, h0, mm, sensor)),
            ("blind", lambda: ro.walk_device_sensed(T, com0, dcom0, h0, mm, blind)), ("pair", pair))
for _, fn in variants:      # warm-up (module load, allocator, the workspaces of the reverse walk)
    fn()
ms = {k: [] for k, _ in variants}
last = {}
for _ in range(args.repeats):
    for k, fn in variants:
        t, last[k] = timed(torch, fn)
        ms[k].append(t)
m = {k: med(v) for k, v in ms.items()}
its = {k: float(last[k]["iterations_sum"].double().mean()) / T for k in ("hidden", "sensed", "blind")}
ended = {k: int((last[k]["end_tick"] >= 0).sum()) for k in ("hidden", "sensed", "blind")}
same_blind = all(torch.equal(last["blind"][k], last["hidden"][k]) for k in ("X", "state", "iterations", "end_tick"))
dev = lambda k: float((last[k]["final_state"][:, :3] - last["hidden"]["final_state"][:, :3]).norm(dim=1).max())
say(f"(a) walk_device_mismatch (hidden pushes) {m['hidden']:.4f} ({fmt(ms['hidden'])}), {its['hidden']:.2f} iterations per solve | blind sensor {m['blind']:.4f} "
    f"({fmt(ms['blind'])}), {its['blind']:.2f} iterations, the same walk to the bit: {same_blind} | blind / hidden = {m['blind'] / m['hidden']:.4f}, "
    f"{1e3 * (m['blind'] - m['hidden']):+.1f} us per tick: the sense launch's own cost")
say(f"(a) sensed (delay 1, hold 3, deadband 0.7, noise) {m['sensed']:.4f} ({fmt(ms['sensed'])}), {its['sensed']:.2f} iterations per solve | sensed / hidden = "
    f"{m['sensed'] / m['hidden']:.4f}, {1e3 * (m['sensed'] - m['hidden']):+.1f} us per tick, the re-planning robots' other solves included | ended problems "
    f"{ended['hidden']} / {ended['sensed']}, largest CoM difference of a final state {dev('sensed'):.3e}")


def launches(fn):
    """us per launch: events around --launches back-to-back launches on the launch stream"""
    fn()
    torch.cuda.synchronize()
    ls = ro_t.solver.launch_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ls):
        e0.record(ls)
        for _ in range(args.launches):
            fn()
        e1.record(ls)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.launches


s, w, g = ro_t.solver, last["pair"][0], last["pair"][1]
mmc, snc = w["tape"]["mismatch"], w["tape"]["sensor"]
dh, dn = torch.randn((8, B, 2, 6), dtype=torch.float64, device="cuda"), torch.randn((T, B, 2, 6), dtype=torch.float64, device="cuda")
us = dict(sense=launches(lambda: s._wrench_sense_device(3, 1, mmc, snc, passed=False)),
          vjp=launches(lambda: s._wrench_sense_vjp_device(0, T, mmc, snc, g["wrench"], g["plant_wrench"])),
          jvp=launches(lambda: s._wrench_sense_jvp_device(0, T, 2, mmc, snc, dh, dn)))
t_rev = med([timed(torch, lambda: ro_t.backward_device_sensed(w, gS))[0] for _ in range(args.repeats)])
say(f"(b) by events over {args.launches} back-to-back launches (output allocation included), us per launch: the sense launch of one tick {us['sense']:.1f} | the "
    f"VJP over {T} rows {us['vjp']:.1f} | the JVP over {T} rows, k = 2, {us['jvp']:.1f} | one reverse tick (backward_device_sensed / ticks) {1e3 * t_rev:.1f} | "
    f"taped sensed walk + reverse {m['pair']:.4f} ms per tick ({fmt(ms['pair'])}) | largest |d/d hidden_wrench| {float(g['hidden_wrench'].abs().max()):.3e}, "
    f"|d/d sensor_noise| {float(g['sensor_noise'].abs().max()):.3e}")
for ln in trace_lines:
    say("(b) kernel trace: " + ln)
if ab:
    new, old = med(ab["libcmpc_hip.so"]), med(ab[args.baseline])
    twin = f" | {args.baseline2} / {args.baseline} = {med(ab[args.baseline2]) / old:.4f} (parent against parent)" if args.baseline2 else ""
    say(f"(c) headline solve (bench.py config2 through tools/ab_multi.sh, {args.ab_reps} rounds), ms per step: " +
        " | ".join(f"{lib} {med(v):.4f} ({fmt(v)})" for lib, v in ab.items()) + f" | this build / {args.baseline} = {new / old:.4f}" + twin)
    new, old = med(abw["libcmpc_hip.so"]), med(abw[args.baseline])
    twin = f" | {args.baseline2} / {args.baseline} = {med(abw[args.baseline2]) / old:.4f} (parent against parent)" if args.baseline2 else ""
    say(f"(c) walk_device(), child processes alternating, {args.ab_reps} rounds of the median of {args.repeats}, ms per tick: " +
        " | ".join(f"{lib} {med(v):.4f} ({fmt(v)})" for lib, v in abw.items()) + f" | this build / {args.baseline} = {new / old:.4f}" + twin)
else:
    say("(c) not run (no --baseline)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
