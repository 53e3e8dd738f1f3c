"""Developer probe (GPU box): what the physical limits of a device walk (cmpc_set_walk_limits, WalkingRollout.set_limits) cost, and that nothing existing
moved.  B = 256, N = 20, walks of 24 ticks, medians of five.
(a) limits off, this build against --baseline LIB (another build of the library in the package directory, e.g. the parent commit's), in child processes
    started before this one touches the GPU, the variants alternating: the headline solve (bench.py config2 with tools/ab_multi.sh's settings) and
    walk_device.  The baseline runs TWICE per round, as two variants: baseline / baseline is the spread the ratio this build / baseline is held against.
(b) limits on against off on this build, in this process, alternating: walk_device with all five limits set wide (nobody ends: the same ticks both ways)
    and the measures trace and the extremes written.
--profile-child: three walks with limits on and three with limits off, and leave (for `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/gpu_walk_limits.py --profile-child`, a run of its own); --kernel-stats FILE: that run's kernel_stats.csv, the record kernels' rows appended to --out (no GPU is touched);
--resources "TEXT": the record kernels' registers and scratch as the compile reported them, appended to --out.  Writes its lines to --out as well."""
import argparse, csv, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_walk_limits.txt"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", default=None)
ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
ap.add_argument("--walk-only", action="store_true", help="print the median ms per tick of the 24-tick walk_device at B = 256, limits off, and leave")
ap.add_argument("--profile-child", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--resources", default=None)
args = ap.parse_args()
TT, B, lines = 24, 256, []
WIDE = dict(height=(0.1, 2.0), reach_max=5.0, margin_min=-5.0, track_max=50.0)
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish():
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)


if args.kernel_stats is not None or args.resources is not None:
    if args.kernel_stats is not None:
        with open(args.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if any(k in r["Name"] for k in ("cmpc_rollout_record_kernel", "cmpc_tick_post_kernel", "cmpc_extremes_init_kernel"))]
        say("kernel times of a --profile-child run (rocprofv3 --kernel-trace --stats; 24-tick walks at B = 256, a warm-up and three with limits on, <true>, "
            "and as many with limits off, <false>): calls, average ns, share of the kernel time")
        for r in rows:
            name = r["Name"][r["Name"].index("cmpc_"):]
            say(f"  {name[:name.index('(')] if '(' in name else name}: {r['Calls']} calls, {float(r['AverageNs']):.0f} ns on average (min {r['MinNs']}, "
                f"max {r['MaxNs']}), {r['Percentage']} %")
    if args.resources:
        say(args.resources)
    args.append = True
    finish()


def start(n, seed=5):
    rng = np.random.default_rng(seed)
    com0 = (np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (n, 3))).astype(np.float32)
    dcom0 = rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    h0 = rng.uniform(-0.02, 0.02, (n, 3)).astype(np.float32)
    push = np.zeros((n, 3), np.float32)
    push[:, :2] = rng.uniform(-20.0, 20.0, (n, 2)) / 56.0
    return com0, dcom0, h0, push


ab = None
if args.baseline:
    variants = [("baseline", args.baseline), ("baseline again", args.baseline), ("this build", "libcmpc_hip.so")]
    ab = {"solve": {v: [] for v, _ in variants}, "walk": {v: [] for v, _ in variants}}
    for _ in range(args.repeats):
        for v, lib in variants:
            env = dict(os.environ, CMPC_LIB=lib)
            r = subprocess.run([sys.executable, "bench.py", "--workload", "config2", "--no-cpu-baseline", "--secondary", "none", "--steps", "30", "--warmup", "3"],
                               cwd=ROOT, capture_output=True, text=True, env=env, timeout=180)
            assert r.returncode == 0, r.stderr[-2000:]
            ab["solve"][v].append(float(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--walk-only"], cwd=ROOT, capture_output=True, text=True, env=env, timeout=180)
            assert r.returncode == 0, r.stderr[-2000:]
            ab["walk"][v].append(float(r.stdout.split()[-1]))
            print(v, ab["solve"][v][-1], ab["walk"][v][-1], flush=True)

import torch
import cmpc_amd as cm

cfg = cm.config.ergocub_gazebo_v1(20, 0.06)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


com0, dcom0, h0, push = start(B)
ro = cm.rollout.WalkingRollout(cfg, B)
walk = lambda: ro.walk_device(TT, com0, dcom0, h0, push=push, push_ticks=3)
walk()      # warm-up (module load, allocator)
if args.walk_only:
    print("walk_device ms per tick", float(np.median([timed(walk)[0] for _ in range(5)])) / TT)
    sys.exit(0)


def walk_on():
    ro.set_limits(**WIDE)
    try:
        return ro.walk_device(TT, com0, dcom0, h0, push=push, push_ticks=3, stop=("merge", "solver", "nonfinite", "limits"))
    finally:
        ro.clear_limits()


walk_on()
if args.profile_child:
    for _ in range(3):
        walk_on()
        walk()
    torch.cuda.synchronize()
    sys.exit(0)

say(f"physical limits of a device walk: N = {cfg.N}, B = {B}, walk_device of {TT} ticks, medians of {args.repeats}, the variants alternating; "
    f"{torch.cuda.get_device_name(0)}")
if ab:
    for what, unit in (("solve", "headline solve (bench.py config2, 30 steps), ms per step"), ("walk", f"walk_device, limits off, ms per tick (median of 5 per child)")):
        a, a2, b = (ab[what][v] for v in ("baseline", "baseline again", "this build"))
        say(f"(a) {unit}: {args.baseline} {np.median(a):.4f} ({fmt(a)}) | the same again {np.median(a2):.4f} ({fmt(a2)}) | this build {np.median(b):.4f} ({fmt(b)}) | "
            f"baseline again / baseline = {np.median(a2) / np.median(a):.4f} (the spread) | this build / baseline = {np.median(b) / np.median(a):.4f}")
ms = {"off": [], "on": []}
for _ in range(args.repeats):
    m, w0 = timed(walk)
    ms["off"].append(m)
    m, w1 = timed(walk_on)
    ms["on"].append(m)
same = all(bool((w0[k] == w1[k]).all()) for k in ("end_tick", "iterations_sum", "final_state"))
m = w1["measures"].cpu().numpy()
mo, mn = float(np.median(ms["off"])), float(np.median(ms["on"]))
say(f"(b) limits on (five wide limits, the measures trace [24, {B}, 4] and the extremes written) against off, ms per walk: off {mo:.3f} ({fmt(ms['off'])}) | on {mn:.3f} "
    f"({fmt(ms['on'])}) | on / off = {mn / mo:.4f} | {(mn - mo) * 1e3 / TT:.2f} us per tick | nobody ended and the outcome is the same: {same}")
say(f"    measures over the walk: height {np.nanmin(m[..., 0]):.4f} .. {np.nanmax(m[..., 0]):.4f}, reach up to {np.nanmax(m[..., 1]):.4f}, margin down to "
    f"{np.nanmin(m[..., 2]):.4f}, track up to {np.nanmax(m[..., 3]):.4f}; codes 6..9 recorded: {int((w1['code'] >= 6).sum().item())}")
finish()
