"""Developer probe (GPU box): whether refilling slots pays when a trial starts from a snapshot (cmpc_rollout_walk_refill_snapshot_device,
WalkingRollout.walk_device_refill_from_snapshot), and that nothing existing moved.  N = 20, B = 256; a pilot walk_device_checkpointed gives the snapshot of
tick 12; Q = 1024 trials of 24 resumed ticks fork from rows of it drawn at random, each under a hidden push of its own direction and size on its first
--push-ticks resumed ticks (default 4: a shove; 24: a constant force), the sizes scaled (--scale, or found by bisection on the fraction that ends, --fall) so that about a quarter of the trials end early.  In one process after a
warm-up the two ways alternate, --repeats times, the median kept:
    today   Q / B walk_resume_device_mismatch(skip_ended=True) calls of 24 ticks, one after the other, each with its 256 columns of the pushes
    refill  ONE walk_device_refill_from_snapshot of as many ticks as the queue needs (the assignment rule run on the host from the end ticks seen)
Reported: wall time per trial-tick run (a trial that ends at its resumed tick r ran r + 1 ticks), the ratio refill / today -- no pass mark -- and the
iteration counts of both (no tick of the refill walk holds a cold solve).  --restore-stats FILE: the kernel_stats.csv of a separate
`rocprofv3 --kernel-trace --stats -- python tools/gpu_walk_refill_snapshot.py --new-only --scale S` run; the restore kernel's and its neighbours' rows are
appended to --out and nothing else is done (no GPU is touched).
With --baseline LIB (another build of the library in the package directory, e.g. the parent commit's), first, in child processes started before this one
touches the GPU, the builds alternating: the headline solve of bench.py through tools/ab_multi.sh, and walk_device, walk_device_refill and
walk_device_refill_trials at B = 256 (--child walk | refill | trials), this build / LIB.  With --reach-max R the study's trials end by the reach limit R
(WalkingRollout.set_limits, tick code 7) under their hidden pushes, on both sides; without it they end as recorded so far.  Writes its lines to --out as
well."""
import argparse, csv, dataclasses, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_walk_refill_snapshot.txt"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", default=None)
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--fall", type=float, default=0.25, help="the fraction of the trials that should end early")
ap.add_argument("--scale", type=float, default=None, help="the largest hidden push in m/s^2 (default: bisection towards --fall)")
ap.add_argument("--push-ticks", type=int, default=4, help="the resumed ticks the hidden push lasts (24: the whole trial)")
ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
ap.add_argument("--new-only", action="store_true", help="the refill walk from the snapshot alone, three times (for a kernel trace), and leave")
ap.add_argument("--restore-stats", default=None, help="a rocprofv3 kernel_stats.csv of a --new-only run: quote the restore kernel's row")
ap.add_argument("--child", choices=("walk", "refill", "trials"), default=None, help="print the median ms of one existing path at B = 256 and leave")
ap.add_argument("--reach-max", type=float, default=None, help="the study's trials end by this physical limit on the CoM's distance from a supporting foot, in m "
                "(set_limits, tick code 7) under their hidden pushes, on both sides; default: they end when the solve or the state fails, as recorded so far")
args = ap.parse_args()
STOP = ("merge", "solver", "nonfinite") + (("limits",) if args.reach_max is not None else ())
TT, TS, B, Q, lines = 24, 12, 256, 1024, []


def say(s):
    print(s, flush=True)
    lines.append(s)


def start(n, seed=5):
    rng = np.random.default_rng(seed)
    com0 = (np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (n, 3))).astype(np.float32)
    dcom0 = rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    h0 = rng.uniform(-0.02, 0.02, (n, 3)).astype(np.float32)
    push = np.zeros((n, 3), np.float32)
    push[:, :2] = rng.uniform(-20.0, 20.0, (n, 2)) / cm.synthetic.ROBOT_MASS
    return com0, dcom0, h0, push


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


if args.restore_stats:
    with open(args.restore_stats) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Name"] for k in ("cmpc_refill_restore_kernel", "cmpc_refill_kernel", "cmpc_tick_pre_kernel",
                                                                              "cmpc_tick_post_kernel", "cmpc_rollout_record_kernel", "cmpc_solve"))]
    say("kernel times of a --new-only run (rocprofv3 --kernel-trace --stats, three refill walks from the snapshot): calls, average ns, share of the kernel time")
    for r in rows:
        name = r["Name"][r["Name"].index("cmpc_"):]
        say(f"  {name[:name.index('(')] if '(' in name else name}: {r['Calls']} calls, {float(r['AverageNs']):.0f} ns on average (min {r['MinNs']}, max {r['MaxNs']}), {r['Percentage']} %")
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)

ab = {}
if args.baseline and not args.child:
    libs = [args.baseline, "libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True,
                         timeout=90 * args.ab_reps * len(libs)).stdout      # (a bench.py child takes about 15 s)
    ab["solve"] = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab["solve"]:
            ab["solve"][w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab["solve"].values()), out
    for mode in ("walk", "refill", "trials"):
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
    """the assignment rule on the host: ends[q] = the resumed tick trial q ends at, or -1 -> the ticks the queue needs"""
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


if args.child:      # ---- the existing paths, for the comparison of two builds: r12's and r13's workloads (a queue from standing, a quarter ends by a NaN wrench row)
    com0, dcom0, h0, push = start(Q)
    ro = cm.rollout.WalkingRollout(cfg, B)
    if args.child == "walk":
        ro.walk_device(8, com0[:B], dcom0[:B], h0[:B], push=push[:B], push_ticks=3)
        med, _, _ = timed(lambda: ro.walk_device(TT, com0[:B], dcom0[:B], h0[:B], push=push[:B], push_ticks=3), 5)
        print("walk_device ms", med)
        sys.exit(0)
    rng = np.random.default_rng(7)
    ends = np.full(Q, -1)
    falls = rng.permutation(Q)[:Q // 4]
    ends[falls] = rng.integers(0, TT, len(falls))
    wrench = np.zeros((TT, Q, N, 6), np.float32)
    for i in range(3):
        wrench[i, :, :3 - i, :3] = push[:, None, :]
    wrench[ends[falls], falls] = np.nan
    T = ticks_needed(ends)
    dwrench = torch.from_numpy(wrench).to(ro.dev)
    d0 = [torch.from_numpy(a).to(ro.dev) for a in (com0, dcom0, h0)]
    if args.child == "refill":
        fn = lambda: ro.walk_device_refill(T, TT, *d0, wrench_trials=dwrench)
    else:
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
        fn = lambda: ro.walk_device_refill_trials(T, TT, *d0, models=models, mismatch=mm, wrench_trials=dwrench)
    fn()
    print(args.child, "ms", timed(fn, 5)[0])
    sys.exit(0)

# ---- the study
com0, dcom0, h0, _ = start(B)
ro = cm.rollout.WalkingRollout(cfg, B)
pilot = ro.walk_device_checkpointed(TS + 1, com0, dcom0, h0, TS)
torch.cuda.synchronize()
pool = pilot["checkpoints"][TS]
assert pool["tick"] == TS and (pilot["end_tick"] == -1).all().item()
rng = np.random.default_rng(13)
snapshot_of = rng.integers(0, B, Q).astype(np.int32)
angle, size = rng.uniform(0, 2 * np.pi, Q), rng.uniform(0, 1, Q)
unit = np.zeros((TT, Q, 6), np.float32)
unit[:args.push_ticks, :, 0], unit[:args.push_ticks, :, 1] = (size * np.cos(angle))[None, :], (size * np.sin(angle))[None, :]
d_of = torch.from_numpy(snapshot_of).to(ro.dev)


if args.reach_max is not None:      # (after the pilot, which walks without limits; sticky on the roll-out: both sides walk under it)
    ro.set_limits(reach_max=args.reach_max)


def refill_walk(hidden, T):
    return ro.walk_device_refill_from_snapshot(pool, T, TT, d_of, mismatch=dict(hidden_wrench=hidden), stop=STOP)


def ended(scale):
    """the trials' resumed end ticks under pushes of at most `scale` m/s^2, from a refill walk long enough for any outcome"""
    w = refill_walk(torch.from_numpy(unit * np.float32(scale)).to(ro.dev), Q // B * TT)
    torch.cuda.synchronize()
    e = w["trials"]["end_tick"].cpu().numpy()
    assert (w["trials"]["start"] >= 0).all().item()
    return np.where(e >= 0, e - TS, -1)


scale = args.scale
if scale is None:      # bisection on the fraction that ends (it grows with the push, up to the noise of a few trials)
    lo, hi = 0.0, 4.0
    while (ended(hi) >= 0).mean() < args.fall and hi < 64:
        lo, hi = hi, 2 * hi
    for _ in range(8):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if (ended(mid) >= 0).mean() < args.fall else (lo, mid)
    scale = hi
print("scale", scale, flush=True)
ends = ended(scale)
hidden = torch.from_numpy(unit * np.float32(scale)).to(ro.dev)
T = ticks_needed(ends)
run_ticks = int(np.where(ends < 0, TT, ends + 1).sum())
new = lambda: refill_walk(hidden, T)
if args.new_only:
    for _ in range(3):
        new()
    torch.cuda.synchronize()
    print("refill walk from the snapshot:", T, "ticks, scale", scale)
    sys.exit(0)


def today():
    return [ro.walk_resume_device_mismatch(pool, TT, dict(hidden_wrench=hidden[:, c * B:(c + 1) * B].contiguous(), tick_first=TS),
                                           index=d_of[c * B:(c + 1) * B].contiguous(), skip_ended=True, stop=STOP) for c in range(Q // B)]


today(); new()       # warm-up
ms = {"today": [], "refill": []}
for _ in range(args.repeats):
    m, _, recs = timed(today, 1)
    ms["today"].append(m)
    m, _, w = timed(new, 1)
    ms["refill"].append(m)
tr = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
end_today = torch.cat([r["end_tick"] for r in recs]).cpu().numpy()
same = bool((end_today == tr["end_tick"]).all() and (np.where(tr["end_tick"] >= 0, tr["end_tick"] - TS, -1) == ends).all() and int(tr["ticks"].sum()) == run_ticks
            and (tr["snapshot_ok"] == 1).all())
it_today = int(sum(int(r["iterations_sum"].sum().item()) for r in recs))
mt, mr = float(np.median(ms["today"])), float(np.median(ms["refill"]))
say(f"refill walk whose trials start from a snapshot: N = {N}, B = {B}, Q = {Q} trials of {TT} resumed ticks from the snapshot of tick {TS} of a {TS + 1}-tick "
    f"pilot, rows drawn at random; a hidden push per trial on its first {args.push_ticks} resumed ticks, at most {scale:.4f} m/s^2; {'' if args.reach_max is None else f'trials end by reach_max = {args.reach_max:g} m (tick code 7); '}today ={Q // B} walk_resume_device_mismatch(skip_ended=True), "
    f"refill = one walk_device_refill_from_snapshot; the two alternate, median of {args.repeats}; {torch.cuda.get_device_name(0)}")
say(f"{int((ends >= 0).sum())} trials end early ({(ends >= 0).mean():.3f}), {run_ticks} trial-ticks run of {Q * TT}; today {Q // B} x {TT} = {Q // B * TT} ticks, refill "
    f"{T} ticks ({len(np.unique(tr['start']))} of them with at least one spawn); end ticks agree, every trial ran and was restored: {same}")
say(f"today {mt:.2f} ms ({fmt(ms['today'])}) = {mt * 1e3 / run_ticks:.3f} us per trial-tick, {mt / (Q // B * TT):.4f} ms per tick | refill {mr:.2f} ms "
    f"({fmt(ms['refill'])}) = {mr * 1e3 / run_ticks:.3f} us per trial-tick, {mr / T:.4f} ms per tick | refill / today = {mr / mt:.4f}")
say(f"iterations per trial-tick: today {it_today / run_ticks:.2f}, refill {int(tr['iterations_sum'].sum()) / run_ticks:.2f}; the sum over the ticks of the "
    f"tick's largest iteration count: today {int(sum(int(r['stats'][:, 3].sum().item()) for r in recs))}, refill {int(w['stats'][:, 3].sum().item())}")
names = dict(solve="headline solve (bench.py config2 through tools/ab_multi.sh), ms per step", walk=f"walk_device, B = {B}, {TT} ticks, ms per walk",
             refill=f"walk_device_refill, B = {B}, Q = {Q}, a quarter ends early, ms per walk",
             trials="walk_device_refill_trials, the same queue with models and the full mismatch per trial, ms per walk")
for mode, v in ab.items():
    a, b = v[args.baseline], v["libcmpc_hip.so"]
    say(f"{names[mode]} ({'median of 5 in a child process, ' if mode != 'solve' else ''}{args.ab_reps} children per build, alternating): {args.baseline} "
        f"{np.median(a):.4f} ({fmt(a)}) | this build {np.median(b):.4f} ({fmt(b)}) | this build / baseline = {np.median(b) / np.median(a):.4f}")
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
