"""Developer probe (GPU box): what a footstep plan and reference trajectories per trial cost a refill walk (cmpc_rollout_walk_refill_plans_device,
cmpc_rollout_plan_fold_device; WalkingRollout.walk_device_refill_plans) -- and that nothing existing moved.  The study is r13's: N = 20, B = 256, Q = 1024
trials of 24 ticks from standing, a model and the full mismatch (hidden pushes, noise, gains) per trial, a quarter of the trials ended at a uniform local
tick by a NaN wrench row.  In one process after a warm-up the variants alternate, --repeats times, the median kept:
    trials    ONE walk_device_refill_trials of as many ticks as the queue needs
    plans     ONE walk_device_refill_plans of the same ticks over an IDENTICAL pool: --pool rows, every one the roll-out's own plan and straight-line
              references, plan_of = q % rows -- the same walk to the bit, one launch more per tick
    fold      cmpc_rollout_plan_fold_device alone over [Q, 2, M, 3] float64 onto the pool's rows, device events over --fold-reps back-to-back launches
Reported per trial-tick; no pass mark.  --new-only: the plans walk alone, three times, and leave (for a kernel trace);  --select-stats FILE: the
kernel_stats.csv of a separate `rocprofv3 --kernel-trace --stats -- python tools/gpu_walk_refill_plans.py --new-only` run, or the .db that rocprofv3
writes by default; the select kernel's and its neighbours' rows are appended to --out and nothing else is done (no GPU is touched).
With --baseline LIB [--baseline LIB2 ...] (other builds of the library in the package directory: the parent commit's, and a copy of it for the
parent-against-parent scatter), first, in child processes started before this one touches the GPU, the builds alternating: the headline solve of bench.py
through tools/ab_multi.sh, and walk_device and walk_device_refill_trials at B = 256 (--child walk | trials); every build / the first baseline.  Writes its
lines to --out as well."""
import argparse, csv, dataclasses, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_walk_refill_plans.txt"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--pool", type=int, default=16)
ap.add_argument("--fold-reps", type=int, default=200)
ap.add_argument("--baseline", action="append", default=None)
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
ap.add_argument("--new-only", action="store_true", help="the plans walk alone, three times (for a kernel trace), and leave")
ap.add_argument("--select-stats", default=None, help="a rocprofv3 kernel_stats.csv, or results .db, of a --new-only run: quote the select kernel's row")
ap.add_argument("--child", choices=("walk", "trials"), default=None, help="print the median ms of one existing path at B = 256 and leave")
args = ap.parse_args()
TT, B, Q, lines = 24, 256, 1024, []


def say(s):
    print(s, flush=True)
    lines.append(s)


def write():
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


def children(mode, libs, reps, timeout):
    out = {lib: [] for lib in libs}
    for _ in range(reps):
        for lib in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], cwd=ROOT, capture_output=True, text=True,
                               env=dict(os.environ, CMPC_LIB=lib), timeout=timeout)
            assert r.returncode == 0, r.stderr[-2000:]
            out[lib].append(float(r.stdout.split()[-1]))
            print(mode, lib, out[lib][-1], flush=True)
    return out


if args.select_stats is not None:
    assert os.path.isfile(args.select_stats), f"--select-stats: no such file {args.select_stats!r}"
    if args.select_stats.endswith(".db"):      # (rocprofv3's default output: a rocpd database; its `kernels` view has a row per dispatch, times in ns)
        import sqlite3
        with sqlite3.connect(args.select_stats) as db:
            total = db.execute("select sum(duration) from kernels").fetchone()[0]
            every = [dict(Name=n, Calls=c, AverageNs=a, MinNs=lo, MaxNs=hi, Percentage=f"{100.0 * t / total:.2f}") for n, c, a, lo, hi, t in db.execute(
                "select name, count(*), avg(duration), min(duration), max(duration), sum(duration) from kernels group by name order by sum(duration) desc")]
    else:
        with open(args.select_stats) as f:
            every = list(csv.DictReader(f))
    rows = [r for r in every if any(k in r["Name"] for k in ("cmpc_refill_plans_kernel", "cmpc_refill_kernel", "cmpc_tick_pre_kernel",
                                                              "cmpc_tick_post_kernel", "cmpc_rollout_record_kernel", "cmpc_solve"))]
    say("kernel times of a --new-only run (rocprofv3 --kernel-trace --stats, three plans walks): calls, average ns, share of the kernel time")
    for r in rows:
        name = r["Name"][r["Name"].index("cmpc_"):]
        say(f"  {name[:name.index('(')] if '(' in name else name}: {r['Calls']} calls, {float(r['AverageNs']):.0f} ns on average (min {r['MinNs']}, max {r['MaxNs']}), {r['Percentage']} %")
    args.append = True
    write()
    sys.exit(0)

ab = {}
if args.baseline and not args.child:
    libs = list(args.baseline) + ["libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True,
                         timeout=90 * args.ab_reps * len(libs)).stdout      # (a bench.py child takes about 15 s)
    ab["solve"] = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab["solve"]:
            ab["solve"][w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab["solve"].values()), out
    for mode in ("walk", "trials"):
        ab[mode] = children(mode, libs, args.ab_reps, 180)

import torch
import cmpc_amd as cm

cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
N = cfg.N
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms, out


def ticks_needed(ends):
    """the assignment rule on the host: ends[q] = the local tick trial q ends at, or -1 -> the ticks the queue needs"""
    left = np.zeros(B, np.int64)      # ticks the slot's trial still runs
    nxt, t = 0, 0
    while True:
        free = np.flatnonzero(left == 0)
        take = min(len(free), Q - nxt)
        for b in free[:take]:
            left[b] = TT if ends[nxt] < 0 else ends[nxt] + 1
            nxt += 1
        if nxt >= Q and not left.any():
            return t
        left[left > 0] -= 1
        t += 1


# ---- r13's queue: standing starts, the push the MPC is told about on three ticks, a quarter ended by a NaN wrench row, 35 models, the full mismatch
rng = np.random.default_rng(5)
com0 = (np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (Q, 3))).astype(np.float32)
dcom0 = rng.uniform(-0.05, 0.05, (Q, 3)).astype(np.float32)
h0 = rng.uniform(-0.02, 0.02, (Q, 3)).astype(np.float32)
push = np.zeros((Q, 3), np.float32)
push[:, :2] = rng.uniform(-20.0, 20.0, (Q, 2)) / cm.synthetic.ROBOT_MASS
ro = cm.rollout.WalkingRollout(cfg, B)
if args.child == "walk":
    ro.walk_device(8, com0[:B], dcom0[:B], h0[:B], push=push[:B], push_ticks=3)
    print("walk_device ms", timed(lambda: ro.walk_device(TT, com0[:B], dcom0[:B], h0[:B], push=push[:B], push_ticks=3), 5)[0])
    sys.exit(0)
rng = np.random.default_rng(7)
ends = np.full(Q, -1)
falls = rng.permutation(Q)[:Q // 4]
ends[falls] = rng.integers(0, TT, len(falls))
wrench = np.zeros((TT, Q, N, 6), np.float32)
for i in range(3):
    wrench[i, :, :3 - i, :3] = push[:, None, :]
wrench[ends[falls], falls] = np.nan
dwrench = torch.from_numpy(wrench).to(ro.dev)
d0 = [torch.from_numpy(a).to(ro.dev) for a in (com0, dcom0, h0)]
rows = []
for q in range(35):
    s = 0.85 + 0.075 * (q % 5)
    contacts = [dataclasses.replace(c, corners=[tuple(s * v for v in cn) for cn in c.corners]) for c in cfg.contacts]
    rows.append(dataclasses.replace(cfg, static_friction_coefficient=0.3 + 0.075 * (q % 7), contacts=contacts))
models = torch.from_numpy(np.ascontiguousarray(cm.config.model_array(rows)[np.arange(Q) % 35])).to(ro.dev)
r2 = np.random.default_rng(11)
mm = dict(hidden_wrench=np.concatenate([r2.normal(0, 0.3, (TT, Q, 3)), r2.normal(0, 0.05, (TT, Q, 3))], -1).astype(np.float32),
          state_noise=np.concatenate([r2.normal(0, 3e-3, (TT, Q, 3)), r2.normal(0, 1e-2, (TT, Q, 3)), r2.normal(0, 2e-3, (TT, Q, 3))], -1).astype(np.float32),
          force_gain=r2.uniform(0.9, 1.1, Q).astype(np.float32))
mm = {k: torch.from_numpy(v).to(ro.dev) for k, v in mm.items()}
T = ticks_needed(ends)
run_ticks = int(np.where(ends < 0, TT, ends + 1).sum())
trials = lambda: ro.walk_device_refill_trials(T, TT, *d0, models=models, mismatch=mm, wrench_trials=dwrench)
if args.child == "trials":
    trials()
    print("trials ms", timed(trials, 5)[0])
    sys.exit(0)

# ---- an identical pool: every row the roll-out's own plan and the slots' straight line
own = [cm.rollout.walking_plan(cfg)] * args.pool
pool = tuple(torch.from_numpy(a).to(ro.dev) for a in ro.plan_pool(own))
prefs = ro.plan_references(own, TT)
plan_of = torch.from_numpy((np.arange(Q) % args.pool).astype(np.int32)).to(ro.dev)
plans = lambda: ro.walk_device_refill_plans(T, TT, *d0, pool, plan_of, references=prefs, models=models, mismatch=mm, wrench_trials=dwrench)
if args.new_only:
    for _ in range(3):
        w = plans()
    torch.cuda.synchronize()
    print("plan_ok", int((w["trials"]["plan_ok"] == 1).sum().item()), "of", Q)
    sys.exit(0)

a, b = trials(), plans()      # warm-up
torch.cuda.synchronize()
bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
same = all(bool((bits(a[k]) == bits(b[k])).all().item()) for k in ("X", "P", "state", "com", "zmp", "code", "iterations", "end_tick", "final_state")) and \
    all(bool((bits(a["trials"][k]) == bits(b["trials"][k])).all().item()) for k in ("end_tick", "end_code", "final_state", "ticks", "slot", "start"))
ms = {"trials": [], "plans": []}
for _ in range(args.repeats):
    ms["trials"].append(timed(trials, 1)[0])
    ms["plans"].append(timed(plans, 1)[0])
mu, mp = float(np.median(ms["trials"])), float(np.median(ms["plans"]))
L, M = ro.L, ro.M
knots = int(prefs["com"].shape[1])
say(f"refill walk, plans per trial: N = {N}, B = {B}, Q = {Q} trials of {TT} ticks, a model and the full mismatch per trial, {int((ends >= 0).sum())} trials ended "
    f"early by a NaN wrench row, {run_ticks} trial-ticks run of {Q * TT}, {T} ticks; a pool of {args.pool} identical rows (M = {M}: {8 * M} + {14 * M} + 2 words of "
    f"lists and 2 x {3 * knots} words of trajectories per spawn), plan_of = q % {args.pool}; the variants alternate, median of {args.repeats}; "
    f"{torch.cuda.get_device_name(0)}")
say(f"outcome, trace, X, P and state of the plans walk bit-equal to the trials walk: {same}; every started trial flagged: "
    f"{int((b['trials']['plan_ok'] == 1).sum().item())} of {Q}")
say(f"walk_device_refill_trials {mu:.2f} ms ({fmt(ms['trials'])}) = {mu * 1e3 / run_ticks:.3f} us per trial-tick | walk_device_refill_plans {mp:.2f} ms "
    f"({fmt(ms['plans'])}) = {mp * 1e3 / run_ticks:.3f} us per trial-tick | plans / trials = {mp / mu:.4f} (one launch more per tick: the plan select; "
    f"{(mp - mu) * 1e3 / T:.2f} us per tick)")

# ---- the fold alone
per = torch.randn((Q, 2, M, 3), dtype=torch.float64, device=ro.dev)
out = torch.empty((args.pool, 2, M, 3), dtype=torch.float64, device=ro.dev)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
with torch.cuda.stream(ro.solver.launch_stream):
    ro.solver.plan_fold_device(plan_of, per, args.pool, out)
    ev[0].record()
    for _ in range(args.fold_reps):
        ro.solver.plan_fold_device(plan_of, per, args.pool, out)
    ev[1].record()
torch.cuda.synchronize()
us = ev[0].elapsed_time(ev[1]) * 1e3 / args.fold_reps
ref = torch.zeros_like(out).index_add_(0, plan_of.to(torch.int64), per)
say(f"plan fold alone ([{Q}, 2, {M}, 3] float64 onto {args.pool} rows, {6 * M * args.pool} threads each walking the queue in ascending order): {us:.1f} us on "
    f"average over {args.fold_reps} back-to-back launches; largest difference from torch's index_add_ (an atomic sum, any order): "
    f"{float((out - ref).abs().max().item()):.3e}")
names = dict(solve="headline solve (bench.py config2 through tools/ab_multi.sh), ms per step", walk=f"walk_device, B = {B}, {TT} ticks, ms per walk",
             trials="walk_device_refill_trials, this queue with models and the full mismatch per trial, ms per walk")
for mode, v in ab.items():
    base = np.median(v[args.baseline[0]])
    say(f"{names[mode]} ({'median of 5 in a child process, ' if mode != 'solve' else ''}{args.ab_reps} children per build, alternating): " +
        " | ".join(f"{'this build' if lib == 'libcmpc_hip.so' else lib} {np.median(x):.4f} ({fmt(x)}), / {args.baseline[0]} = {np.median(x) / base:.4f}"
                   for lib, x in v.items()))
write()
