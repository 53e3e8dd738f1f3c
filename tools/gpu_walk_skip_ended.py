"""Developer probe (GPU box): what taking ended problems out of the launches (cmpc_set_ended_device, walk_device(skip_ended=True)) costs and saves.
walk_device, 60 ticks at N = 20, B = 256 and B = 1024, in one process after a warm-up; skip off and on alternate, three repeats each, the median kept,
whole-call wall clock divided by the ticks (set-up included on both sides):
    (a) nothing ended: the mask is read by every launch and never fires.   bound: on / off <= 1.01
    (b) a replan at tick 2 breaks the planner's list of 4 problems (t[b, 0] += 100: their merge fails from tick 2 on, the record ends them there).
        ms per tick off and on, the iteration words info[:, 0] of the four after the skip-off walk and at a few ticks on the way (what they were
        costing), and the per-tick maximum of the iterations over the walking problems.   bound: on <= off x 1.01; the gain itself is reported, no threshold
    (c) with --baseline LIB (another build of the library in the package directory, e.g. the parent commit's): the headline solve of bench.py, mask NULL,
        both builds in turn through tools/ab_multi.sh in child processes started before this one touches the GPU.   bound: this build / LIB <= 1.01
The 1.01 is three times the 0.3 % in-call spread README.md records for ab_multi.sh runs.  The verdict is printed, and the exit status is 1 when a bound
is missed.  Writes its lines to --out (default profiles/r06_walk_skip_ended.txt) as well."""
import argparse, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_walk_skip_ended.txt"))
ap.add_argument("--ticks", type=int, default=60)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--baseline", default=None, help="file name of another build of the library in the package directory: part (c)")
ap.add_argument("--ab-reps", type=int, default=3)
args = ap.parse_args()
BOUND = 1.01
T, lines, missed = args.ticks, [], []


def say(s):
    print(s, flush=True)
    lines.append(s)


def check(name, ratio):
    good = ratio <= BOUND
    if not good:
        missed.append(name)
    return f"{ratio:.4f} ({'within' if good else 'ABOVE'} the bound {BOUND})"


ab = None
if args.baseline:      # (c) first: fresh child processes, this one has not opened the GPU yet
    libs = [args.baseline, "libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True).stdout
    ab = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab:
            ab[w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab.values()), out

import torch
import cmpc_amd as cm

cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)
say(f"ended problems out of the launches: walk_device, N = {cfg.N}, {T} ticks, skip off / on alternating, median of {args.repeats} repeats, "
    f"ms per tick (whole call / ticks); {torch.cuda.get_device_name(0)}")
for B in (256, 1024):
    rng = np.random.default_rng(5)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    ro = cm.rollout.WalkingRollout(cfg, B)
    broken = [B // 7, B // 3, B // 2, B - 5]
    t = ro.plan[0].clone()
    for b in broken:
        t[b, 0] += 100.0
    for label, replan in (("(a) nothing ended", None), ("(b) 4 problems ended at tick 2", {2: (t, ro.plan[1], ro.plan[2])})):
        walk = lambda skip: ro.walk_device(T, com0, dcom0, h0, push=push, push_ticks=3, replan=replan, skip_ended=skip)
        for skip in (False, True):        # warm-up (module load, allocator)
            ro.walk_device(8, com0, dcom0, h0, push=push, push_ticks=3, replan=replan, skip_ended=skip)
        ms, last = {False: [], True: []}, {}
        for _ in range(args.repeats):
            for skip in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[skip] = walk(skip)
                torch.cuda.synchronize()
                ms[skip].append((time.perf_counter() - t0) * 1e3 / T)
        off, on = float(np.median(ms[False])), float(np.median(ms[True]))
        end = {k: w["end_tick"].cpu().numpy() for k, w in last.items()}
        walking = end[True] < 0
        same = all(np.array_equal(last[True][k].cpu().numpy()[..., walking] if k == "iterations" else last[True][k].cpu().numpy()[walking],
                                  last[False][k].cpu().numpy()[..., walking] if k == "iterations" else last[False][k].cpu().numpy()[walking])
                   for k in ("iterations", "X", "state"))
        assert np.array_equal(end[True], end[False]) and same, "the walking problems differ between skip off and on"
        say(f"B = {B} {label}: skip off {off:.4f} ({fmt(ms[False])}) | skip on {on:.4f} ({fmt(ms[True])}) | on / off = {check(f'{label[:3]} B = {B}', on / off)}"
            f" | walking problems bit-identical: {same}")
        if replan:
            assert sorted(np.nonzero(~walking)[0].tolist()) == sorted(broken) and (end[True][~walking] == 2).all()
            its = last[False]["iterations"].cpu().numpy()[:, walking].max(1)
            info = last[False]["info"].cpu().numpy()
            # (the trace holds 0 for an ended problem; the walk is deterministic, so shorter skip-off walks show what the four were solving on the way)
            at = [k for k in (3, 4, 6, 10, 20, 40) if k < T]
            seen = [ro.walk_device(k, com0, dcom0, h0, push=push, push_ticks=3, replan=replan)["info"].cpu().numpy()[~walking][:, [0, 5]].astype(int) for k in at]
            say(f"B = {B} (b): the four ended problems under skip off, (iterations, status) of their solve at tick "
                + "; ".join(f"{k - 1}: {[tuple(r) for r in v.tolist()]}" for k, v in zip(at, seen)))
            say(f"B = {B} (b): last tick of the skip-off walk, solve_cycles (info word 6) of the four {info[~walking, 6].astype(int).tolist()} against the walking "
                f"problems' median {int(np.median(info[walking, 6]))} and largest {int(info[walking, 6].max())}; their safeguard words (info word 3) "
                f"{info[~walking, 3].astype(int).tolist()}, the walking problems' largest {int(info[walking, 3].max())}")
            say(f"B = {B} (b): off / on = {off / on:.3f}; after the skip-off walk the four ended problems' info[:, 0] (iterations of their last solve) = "
                f"{info[~walking, 0].astype(int).tolist()}, status words {info[~walking, 5].astype(int).tolist()}; per-tick maximum of the iterations over "
                f"the walking problems: median {int(np.median(its))}, largest {int(its.max())}, ticks 2.. {its[2:12].tolist()} ..")
if ab:
    new, old = float(np.median(ab["libcmpc_hip.so"])), float(np.median(ab[args.baseline]))
    say(f"(c) headline solve (bench.py config2 through tools/ab_multi.sh, {args.ab_reps} rounds, mask NULL), ms per step: {args.baseline} {old:.4f} "
        f"({fmt(ab[args.baseline])}) | this build {new:.4f} ({fmt(ab['libcmpc_hip.so'])}) | this build / baseline = {check('(c)', new / old)}")
else:
    say("(c) not run (no --baseline)")
say("verdict: " + ("bound missed: " + "; ".join(missed) if missed else "every bound holds"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if missed else 0)
