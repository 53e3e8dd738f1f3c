"""Developer probe (GPU box): what a tape behind a refill walk costs, what the regroup launch moves, and what every trial's gradient costs against split
walks (cmpc_rollout_walk_refill_taped_device, cmpc_rollout_tape_regroup_device; WalkingRollout.walk_device_refill_taped, refill_trial_walk,
backward_device_refill) -- and that nothing existing moved.  The study is r13's: N = 20, B = 256, Q = 1024 trials of 24 ticks from standing, a model and the
full mismatch (hidden pushes, noise, gains) per trial, a quarter of the trials ended at a uniform local tick.  In one process after a warm-up the variants
alternate, --repeats times, the median kept:
    untaped   ONE walk_device_refill_trials of as many ticks as the queue needs
    taped     ONE walk_device_refill_taped of the same ticks
    regroup   the regroup launch alone (256 trials a launch), timed with device events over --regroup-reps back-to-back launches that take the four groups
              in turn, each into a tape of its own, so that the working set exceeds the last-level cache; bytes moved = read + written
    reverse   backward_device_refill over all 1024 trials
    split     Q / B walk_device_taped(mismatch=..., skip_ended=True) + backward_device pairs over the same trials with the slots' models (the push the MPC
              is told about instead of the NaN row: the trials of a split walk do not end, so this side runs MORE ticks -- both counts are reported)
Reported per trial-tick; no pass mark.  With --baseline LIB (another build of the library in the package directory, e.g. the parent commit's), first, in child
processes started before this one touches the GPU, the builds alternating: the headline solve of bench.py through tools/ab_multi.sh, and walk_device and
walk_device_refill_trials at B = 256 (--child walk | trials), this build / LIB.  With --reach-max R the falling trials end by the reach limit R
(WalkingRollout.set_limits, tick code 7) under --fall-push more of hidden sideways push from their drawn tick on, on the refill side and on the split side
alike, the end ticks read from a pilot walk; the NaN rows stay the default.  Writes its lines to --out as well."""
import argparse, dataclasses, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_walk_refill_tape.txt"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--regroup-reps", type=int, default=400)
ap.add_argument("--baseline", default=None)
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--child", choices=("walk", "trials"), default=None, help="print the median ms of one existing path at B = 256 and leave")
ap.add_argument("--reach-max", type=float, default=None, help="the study's falling trials end by this physical limit on the CoM's distance from a supporting foot, "
                "in m (set_limits, tick code 7), under a hidden sideways push of --fall-push more from their drawn tick on, instead of by a NaN wrench row (the "
                "default, which the recorded profile used); the end ticks are then read from a pilot walk, and the split walks end the same way")
ap.add_argument("--fall-push", type=float, default=8.0, help="with --reach-max: the extra hidden push of a falling trial, m/s^2 (tools/gpu_walk_refill.py's "
                "default; with --reach-max 0.8 and 3 m/s^2 only 21 trials end)")
args = ap.parse_args()
if args.reach_max is not None and args.child:
    ap.error("--reach-max goes with the study, not with --child")
STOP = ("merge", "solver", "nonfinite") + (("limits",) if args.reach_max is not None else ())
TT, B, Q, lines = 24, 256, 1024, []


def say(s):
    print(s, flush=True)
    lines.append(s)


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
if args.reach_max is None:
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
if args.reach_max is not None:      # the falling trials are pushed sideways from their drawn tick on; a pilot walk says when each ends
    for q in falls:
        mm["hidden_wrench"][ends[q]:, q, 1] += np.float32(args.fall_push)
mm = {k: torch.from_numpy(v).to(ro.dev) for k, v in mm.items()}
if args.reach_max is not None:
    ro.set_limits(reach_max=args.reach_max)
    pilot = ro.walk_device_refill_trials(Q // B * TT, TT, *d0, models=models, mismatch=mm, wrench_trials=dwrench, stop=STOP)
    torch.cuda.synchronize()
    assert (pilot["trials"]["start"] >= 0).all().item()
    ends = pilot["trials"]["end_tick"].cpu().numpy()
    print(f"--reach-max {args.reach_max:g}: {int((ends >= 0).sum())} trials end early, {int((pilot['trials']['end_code'] == 7).sum().item())} by tick code 7", flush=True)
T = ticks_needed(ends)
run_ticks = int(np.where(ends < 0, TT, ends + 1).sum())
untaped = lambda: ro.walk_device_refill_trials(T, TT, *d0, models=models, mismatch=mm, wrench_trials=dwrench, stop=STOP)
if args.child == "trials":
    untaped()
    print("trials ms", timed(untaped, 5)[0])
    sys.exit(0)
taped = lambda: ro.walk_device_refill_taped(T, TT, *d0, models=models, mismatch=mm, wrench_trials=dwrench, stop=STOP)

# ---- the taped walk against the untaped one
untaped(); w = taped()      # warm-up
ms = {"untaped": [], "taped": []}
for _ in range(args.repeats):
    ms["untaped"].append(timed(untaped, 1)[0])
    m, _, w = timed(taped, 1)
    ms["taped"].append(m)
tr = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
same = bool((tr["end_tick"] == ends).all() and int(tr["ticks"].sum()) == run_ticks and (tr["start"] >= 0).all())
mu, mt = float(np.median(ms["untaped"])), float(np.median(ms["taped"]))
say(f"refill walk taped: N = {N}, B = {B}, Q = {Q} trials of {TT} ticks, a model and the full mismatch per trial, {int((ends >= 0).sum())} trials ended early by "
    f"{'a NaN wrench row' if args.reach_max is None else f'reach_max = {args.reach_max:g} m under hidden pushes of {args.fall_push:g} m/s^2 more'}, {run_ticks} trial-ticks run of {Q * TT}, {T} ticks; the variants alternate, median of {args.repeats}; {torch.cuda.get_device_name(0)}")
say(f"end ticks as drawn, every trial ran: {same}")
say(f"untaped {mu:.2f} ms ({fmt(ms['untaped'])}) = {mu * 1e3 / run_ticks:.3f} us per trial-tick | taped {mt:.2f} ms ({fmt(ms['taped'])}) = "
    f"{mt * 1e3 / run_ticks:.3f} us per trial-tick | taped / untaped = {mt / mu:.4f} (two launches more per tick: the copy kernel and the multipliers)")

# ---- the regroup launch alone
L, M = ro.L, ro.M
row_bytes = 4 * (L.nx + L.np + L.ng) + 64 * M + 96
views = [ro.refill_trial_walk(w, list(range(c * B, (c + 1) * B))) for c in range(Q // B)]      # (a destination tape per group: 4 x 77 MB beside the 307 MB source)
torch.cuda.synchronize()
moved = 2 * int(TT * B) * row_bytes      # (every destination row is written, from a source row of the same size: rows past a trial's last repeat it)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
with torch.cuda.stream(ro.solver.launch_stream):
    ev[0].record()
    for i in range(args.regroup_reps):
        v = views[i % len(views)]
        ro.solver.tape_regroup_device(w["tape"], w["tape"]["refill"], v["trials"], v["tape"])
    ev[1].record()
torch.cuda.synchronize()
us = ev[0].elapsed_time(ev[1]) * 1e3 / args.regroup_reps
say(f"regroup launch alone ({B} trials a launch, the {Q // B} groups in turn, each into a tape of its own -- {Q // B * moved / 2e6:.0f} MB of destinations beside "
    f"{T * B * row_bytes / 1e6:.0f} MB of source, more than the 256 MB last-level cache; {row_bytes} bytes per row and column): {us:.1f} us on average over "
    f"{args.regroup_reps} back-to-back launches, {moved / 1e6:.1f} MB read + written a launch, {moved / us / 1e3:.1f} GB/s; all {Q} trials: "
    f"{Q // B} launches, {Q // B * moved / 1e6:.0f} MB, {Q // B * us:.0f} us")

# ---- every trial's gradient against split walks
gS = torch.randn((TT + 1, Q, 9), dtype=torch.float64, device=ro.dev)
gX = torch.randn((TT, Q, L.nx), dtype=torch.float32, device=ro.dev)
reverse = lambda: ro.backward_device_refill(w, gS, gX)
dpush = torch.from_numpy(push).to(ro.dev)
split_ros = [cm.rollout.WalkingRollout(cfg, B, models=models[c * B:(c + 1) * B].contiguous()) for c in range(Q // B)]
if args.reach_max is not None:      # (the split walks end the same way)
    for r in split_ros:
        r.set_limits(reach_max=args.reach_max)


def split():
    out = []
    for c, r in enumerate(split_ros):
        sl = slice(c * B, (c + 1) * B)
        o = r.walk_device_taped(TT, d0[0][sl], d0[1][sl], d0[2][sl], push=dpush[sl], push_ticks=3, skip_ended=True, stop=STOP,
                                mismatch={k: (v[sl] if k == "force_gain" else v[:, sl]).contiguous() for k, v in mm.items()})
        out.append((o, r.backward_device(o, gS[:, sl].contiguous(), gX[:, sl].contiguous())))
    return out


reverse(); split()      # warm-up
ms = {"reverse": [], "split": []}
for _ in range(args.repeats):
    m, _, g = timed(reverse, 1)
    ms["reverse"].append(m)
    m, _, sp = timed(split, 1)
    ms["split"].append(m)
mr, msp = float(np.median(ms["reverse"])), float(np.median(ms["split"]))
split_ticks = int(sum(int(torch.where(o["end_tick"] >= 0, o["end_tick"] + 1, torch.full_like(o["end_tick"], TT)).sum().item()) for o, _ in sp))
finite = bool(all(torch.isfinite(v).all().item() for k, v in g.items() if v.dtype.is_floating_point))
say(f"backward_device_refill over all {Q} trials ({Q // B} groups: regroup, set_models_device, the reverse walk): {mr:.2f} ms ({fmt(ms['reverse'])}) = "
    f"{mr * 1e3 / run_ticks:.3f} us per trial-tick; every gradient finite: {finite}")
say(f"taped refill walk + backward_device_refill = {mt + mr:.2f} ms = {(mt + mr) * 1e3 / run_ticks:.3f} us per trial-tick | {Q // B} walk_device_taped(mismatch, "
    f"skip_ended) + backward_device pairs (no NaN row: {split_ticks} trial-ticks run) = {msp:.2f} ms ({fmt(ms['split'])}) = {msp * 1e3 / split_ticks:.3f} us per "
    f"trial-tick | per trial-tick, refill / split = {((mt + mr) / run_ticks) / (msp / split_ticks):.4f}")
names = dict(solve="headline solve (bench.py config2 through tools/ab_multi.sh), ms per step", walk=f"walk_device, B = {B}, {TT} ticks, ms per walk",
             trials="walk_device_refill_trials, this queue with models and the full mismatch per trial, ms per walk")
for mode, v in ab.items():
    a, b = v[args.baseline], v["libcmpc_hip.so"]
    say(f"{names[mode]} ({'median of 5 in a child process, ' if mode != 'solve' else ''}{args.ab_reps} children per build, alternating): {args.baseline} "
        f"{np.median(a):.4f} ({fmt(a)}) | this build {np.median(b):.4f} ({fmt(b)}) | this build / baseline = {np.median(b) / np.median(a):.4f}")
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
