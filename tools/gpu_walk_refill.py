"""Developer probe (GPU box): what refilling ended slots from a queue of trials (cmpc_rollout_walk_refill_device, WalkingRollout.walk_device_refill) buys,
and that nothing existing moved.  N = 20, trials of 24 ticks, Q = 4 B trials of which a quarter (--fall) end at a uniformly drawn local tick (a NaN wrench row: the
solve returns status 2 and the record ends the trial there), B = 256 and, with --large, B = 1024.  In one process after a warm-up, the two ways alternate,
--repeats times, the median kept:
    plain   Q / B walks of 24 ticks with the ended problems out of the launches (cmpc_set_ended_device), one after the other: the path before this feature
    refill  ONE walk_device_refill of as many ticks as the queue needs (the assignment rule run on the host beforehand)
Reported: wall time per trial-tick run (a trial that ends at local tick r ran r + 1 ticks; the sum is the same on both sides), the refill walk's mean tick
time, and how many of its ticks held at least one fresh (cold) solve.  No pass mark: at B <= the CU count a tick lasts as long as its slowest problem and
a cold solve takes more iterations than a warm one, so refills spread over the ticks may cost much of what they save.
With --baseline LIB (another build of the library in the package directory, e.g. the parent commit's), first, in child processes started before this one
touches the GPU: the headline solve of bench.py through tools/ab_multi.sh, and the 24-tick walk_device at B = 256 (--walk-only children, the builds
alternating), this build / LIB for both; and, with --refill-ab, the refill study itself at B = 256 in --refill-only children, the builds alternating.
With --trials, after the study: the same queue once more through walk_device_refill_trials with a model per trial (friction and foot size) and all three
parts of the plant mismatch on every local tick (hidden pushes, noise, a gain per trial), alternating with the walk_device_refill above, per trial-tick
actually run (a mismatch ends some more trials early).  With --reach-max R the falling trials end for a physical reason instead of a NaN row: a hidden
sideways push (--fall-push) from their drawn tick on, and the reach limit R (WalkingRollout.set_limits, tick code 7) on both sides; the end ticks come from
a pilot walk.  The NaN rows stay the default, so that the recorded profiles remain comparable.  Writes its lines to --out (default
profiles/r12_walk_refill.txt) as well."""
import argparse, dataclasses, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_walk_refill.txt"))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--baseline", default=None)
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--fall", type=float, default=0.25, help="the fraction of the trials that end early (the study's is a quarter)")
ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
ap.add_argument("--large", action="store_true", help="the study at B = 1024 as well")
ap.add_argument("--walk-only", action="store_true", help="print the median ms per tick of the 24-tick walk_device at B = 256 and leave")
ap.add_argument("--refill-only", action="store_true", help="print the median ms of the refill study at B = 256 (no per-trial data) and leave")
ap.add_argument("--refill-ab", action="store_true", help="with --baseline: the refill study in child processes, this build / LIB")
ap.add_argument("--trials", action="store_true", help="the study once more with per-trial models and the full per-trial mismatch")
ap.add_argument("--reach-max", type=float, default=None, help="the trials that fall end by this physical limit on the CoM's distance from a supporting foot, in m "
                "(set_limits, tick code 7), under a hidden sideways push of --fall-push from their drawn tick on, instead of by a NaN wrench row (the "
                "default, which the recorded profiles used); the end ticks are then read from a pilot walk")
ap.add_argument("--fall-push", type=float, default=8.0, help="with --reach-max: the hidden push of a falling trial, m/s^2 (at N = 20, --reach-max 0.75 and "
                "8 m/s^2 end 224 of the 256 pushed trials inside their 24 ticks, 223 by tick code 7; 0.8 m and 3 m/s^2 only 33, all at their last tick)")
args = ap.parse_args()
if args.reach_max is not None and (args.trials or args.refill_only or args.refill_ab):
    ap.error("--reach-max goes with the study alone (not with --trials, --refill-only or --refill-ab)")
STOP = ("merge", "solver", "nonfinite") + (("limits",) if args.reach_max is not None else ())
TT, lines = 24, []


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


ab = walk_ab = refill_ab = None
if args.baseline:
    libs = [args.baseline, "libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True,
                         timeout=90 * args.ab_reps * len(libs)).stdout      # (a bench.py child takes about 15 s)
    ab = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab:
            ab[w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab.values()), out
    walk_ab = {lib: [] for lib in libs}
    for _ in range(args.ab_reps):
        for lib in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--walk-only"], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, CMPC_LIB=lib),
                               timeout=120)      # (a child takes about 10 s)
            assert r.returncode == 0, r.stderr[-2000:]
            walk_ab[lib].append(float(r.stdout.split()[-1]))
    if args.refill_ab:
        refill_ab = {lib: [] for lib in libs}
        for _ in range(args.ab_reps):
            for lib in libs:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--refill-only"], cwd=ROOT, capture_output=True, text=True,
                                   env=dict(os.environ, CMPC_LIB=lib), timeout=180)
                assert r.returncode == 0, r.stderr[-2000:]
                refill_ab[lib].append(float(r.stdout.split()[-1]))

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


if args.walk_only:
    com0, dcom0, h0, push = start(256)
    ro = cm.rollout.WalkingRollout(cfg, 256)
    ro.walk_device(8, com0, dcom0, h0, push=push, push_ticks=3)
    med, _, _ = timed(lambda: ro.walk_device(TT, com0, dcom0, h0, push=push, push_ticks=3), 5)
    print("walk_device ms per tick", med / TT)
    sys.exit(0)


def plain_walks(ro, B, state0, wrench, hidden=None):
    """the queue as Q / B walks of TT ticks, ended problems out of the launches: WalkingRollout._walk_live's calls with the wrench rows passed through;
    hidden [TT, Q, 6] (--reach-max): the walks run under their columns of the hidden pushes and under the reach limit"""
    s, L, dev, dt = ro.solver, ro.L, ro.dev, cfg.sampling_time
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    recs = []
    refs = ro._planner_refs(TT)
    ls = s.launch_stream
    ls.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(ls):
        for c in range(state0.shape[0] // B):
            dP, dX0, dX, dInfo = z((B, L.np)), z((B, L.nx)), z((B, L.nx)), z((B, 8))
            state = state0[c * B:(c + 1) * B].clone()
            ok, land, zmp = torch.ones((B,), dtype=torch.int32, device=dev), z((B, 2), torch.int32), z((B, 2))
            rec = s.walk_record(TT, stop=STOP, trace=True)
            s.outcome_init_device(state, rec)
            sets = [tuple(a.clone() for a in ro.plan), tuple(torch.zeros_like(a) for a in ro.plan)]
            wt = wrench[:, c * B:(c + 1) * B].contiguous()
            held = None if hidden is None else s.plant_mismatch(hidden_wrench=hidden[:, c * B:(c + 1) * B].contiguous(), device=dev)
            s.set_ended_device(rec["end_tick"])
            if hidden is not None:
                s.set_walk_limits(reach_max=args.reach_max)
            try:
                s.rollout_walk_device(0, TT, True, ro.plan, sets[0], sets[1], 0, ok, land, state, dP, dX0, dX, dInfo, zmp, rec, row0=0, wrench_ticks=wt,
                                      step=dt / ro.substeps, substeps=ro.substeps, planner=refs, mismatch=held)
            finally:
                s.set_ended_device(None)
                if hidden is not None:
                    s.set_walk_limits(off=True)
            recs.append((rec, wt, state, dP, dX0, dX, dInfo, held))
    torch.cuda.current_stream(dev).wait_stream(ls)
    return recs


def ticks_needed(B, Q, ends):
    """the assignment rule on the host: ends[q] = the local tick trial q ends at, or -1 -> (ticks the queue needs, ticks with at least one spawn)"""
    left = np.zeros(B, np.int64)      # ticks the slot's trial still runs
    nxt, t, fresh = 0, 0, 0
    while True:
        free = np.flatnonzero(left == 0)
        take = min(len(free), Q - nxt)
        for b in free[:take]:
            left[b] = TT if ends[nxt] < 0 else ends[nxt] + 1
            nxt += 1
        fresh += 1 if take else 0
        if nxt >= Q and not left.any():
            return t, fresh
        left[left > 0] -= 1
        t += 1


def trial_data(Q, seed=11):
    """a model per trial (friction 0.3 .. 0.75, foot scale 0.85 .. 1.15, periods 7 and 5) and the three mismatch parts on every local tick: pushes of about
    0.3 m/s^2 and 0.05 N m / kg, a centimetre-scale estimator error, gains in [0.9, 1.1] (tests/test_gpu_mismatch.py's magnitudes)"""
    rows = []
    for q in range(7 * 5):
        s = 0.85 + 0.075 * (q % 5)
        contacts = [dataclasses.replace(c, corners=[tuple(s * v for v in cn) for cn in c.corners]) for c in cfg.contacts]
        rows.append(dataclasses.replace(cfg, static_friction_coefficient=0.3 + 0.075 * (q % 7), contacts=contacts))
    models = np.ascontiguousarray(cm.config.model_array(rows)[np.arange(Q) % 35])
    rng = np.random.default_rng(seed)
    hidden = np.concatenate([rng.normal(0, 0.3, (TT, Q, 3)), rng.normal(0, 0.05, (TT, Q, 3))], -1).astype(np.float32)
    noise = np.concatenate([rng.normal(0, 3e-3, (TT, Q, 3)), rng.normal(0, 1e-2, (TT, Q, 3)), rng.normal(0, 2e-3, (TT, Q, 3))], -1).astype(np.float32)
    return models, dict(hidden_wrench=hidden, state_noise=noise, force_gain=rng.uniform(0.9, 1.1, Q).astype(np.float32))


say(f"refill of ended slots from a queue of trials: N = {N}, trials of {TT} ticks, Q = 4 B, {args.fall:g} of the trials end at a uniform local tick; plain = Q / B "
    f"walks with the ended problems out of the launches, refill = one walk_device_refill; the two alternate, median of {args.repeats}; "
    f"{torch.cuda.get_device_name(0)}")
for B in (256, 1024) if args.large else (256,):
    Q = 4 * B
    rng = np.random.default_rng(7)
    com0, dcom0, h0, push = start(Q)
    ends = np.full(Q, -1)
    falls = rng.permutation(Q)[:int(Q * args.fall)]
    ends[falls] = rng.integers(0, TT, len(falls))
    wrench = np.zeros((TT, Q, N, 6), np.float32)
    for i in range(3):
        wrench[i, :, :3 - i, :3] = push[:, None, :]
    ro = cm.rollout.WalkingRollout(cfg, B)
    dstate0 = torch.from_numpy(np.concatenate([com0, dcom0, h0], 1)).to(ro.dev)
    dhidden = None
    if args.reach_max is None:
        wrench[ends[falls], falls] = np.nan
    else:      # the falling trials are pushed sideways from their drawn tick on, a force the MPC is never told about; a pilot walk says when each ends
        hidden = np.zeros((TT, Q, 6), np.float32)
        for q in falls:
            hidden[ends[q]:, q, 1] = args.fall_push
        dhidden = torch.from_numpy(hidden).to(ro.dev)
        ro.set_limits(reach_max=args.reach_max)
        pilot = ro.walk_device_refill_trials(Q // B * TT, TT, dstate0[:, 0:3], dstate0[:, 3:6], dstate0[:, 6:9], mismatch=dict(hidden_wrench=dhidden),
                                             wrench_trials=torch.from_numpy(wrench).to(ro.dev), stop=STOP)
        torch.cuda.synchronize()
        assert (pilot["trials"]["start"] >= 0).all().item()
        ends = pilot["trials"]["end_tick"].cpu().numpy()
        codes = pilot["trials"]["end_code"].cpu().numpy()
        falls = np.flatnonzero(ends >= 0)
        say(f"--reach-max {args.reach_max:g} m under hidden pushes of {args.fall_push:g} m/s^2: {len(falls)} trials end early, "
            f"{int((codes[falls] == 7).sum())} of them by tick code 7")
    run_ticks = int(np.where(ends < 0, TT, ends + 1).sum())
    T, fresh_ticks = ticks_needed(B, Q, ends)
    dwrench = torch.from_numpy(wrench).to(ro.dev)
    plain = lambda: plain_walks(ro, B, dstate0, dwrench, dhidden)
    if dhidden is None:
        refill = lambda: ro.walk_device_refill(T, TT, dstate0[:, 0:3], dstate0[:, 3:6], dstate0[:, 6:9], wrench_trials=dwrench)
    else:
        refill = lambda: ro.walk_device_refill_trials(T, TT, dstate0[:, 0:3], dstate0[:, 3:6], dstate0[:, 6:9], mismatch=dict(hidden_wrench=dhidden),
                                                      wrench_trials=dwrench, stop=STOP)
    if args.refill_only:
        refill()
        print("refill study ms", timed(refill, 5)[0])
        sys.exit(0)
    plain(); refill()       # warm-up (module load, allocator)
    ms = {"plain": [], "refill": []}
    for _ in range(args.repeats):
        m, _, recs = timed(plain, 1)
        ms["plain"].append(m)
        m, _, w = timed(refill, 1)
        ms["refill"].append(m)
    # the two ways walked the same trials: end ticks agree, and every trial ran
    end_plain = torch.cat([r[0]["end_tick"] for r in recs]).cpu().numpy()
    tr = {k: v.cpu().numpy() for k, v in w["trials"].items() if hasattr(v, "cpu")}
    same = bool((end_plain == tr["end_tick"]).all() and (tr["end_tick"] == ends).all() and int(tr["ticks"].sum()) == run_ticks)
    fresh_seen = len(np.unique(tr["start"]))
    mp, mr = float(np.median(ms["plain"])), float(np.median(ms["refill"]))
    say(f"B = {B}, Q = {Q}: {len(falls)} trials end early, {run_ticks} trial-ticks run of {Q * TT}; plain {Q // B} x {TT} = {Q // B * TT} ticks, refill {T} ticks "
        f"({fresh_seen} of them with at least one fresh solve; the host rule said {fresh_ticks}); end ticks agree and every trial ran: {same}")
    say(f"B = {B}: plain {mp:.2f} ms ({fmt(ms['plain'])}) = {mp * 1e3 / run_ticks:.3f} us per trial-tick, {mp / (Q // B * TT):.4f} ms per tick | refill {mr:.2f} ms "
        f"({fmt(ms['refill'])}) = {mr * 1e3 / run_ticks:.3f} us per trial-tick, {mr / T:.4f} ms per tick | refill / plain = {mr / mp:.4f}")
    if args.trials:
        models, mm = trial_data(Q)
        same_model = np.repeat(cm.config.model_array([cfg]), Q, 0)
        no_mm = dict(hidden_wrench=np.zeros_like(mm["hidden_wrench"]), state_noise=np.zeros_like(mm["state_noise"]), force_gain=np.ones(Q, np.float32))
        cu = lambda d: {k: torch.from_numpy(v).to(ro.dev) for k, v in d.items()}
        # identity: the configuration's own model for every trial, zero pushes and noise, gain 1 -- the problems of the study, through the per-trial kernels
        variants = {"identity": (torch.from_numpy(same_model).to(ro.dev), cu(no_mm)), "models": (torch.from_numpy(models).to(ro.dev), None),
                    "mismatch": (None, cu(mm)), "both": (torch.from_numpy(models).to(ro.dev), cu(mm))}
        run = lambda v: ro.walk_device_refill_trials(T, TT, dstate0[:, 0:3], dstate0[:, 3:6], dstate0[:, 6:9], models=variants[v][0], mismatch=variants[v][1],
                                                     wrench_trials=dwrench)
        for v in variants:
            run(v)
        ms2, last = {v: [] for v in ["none"] + list(variants)}, {}
        for _ in range(args.repeats):
            m, _, last["none"] = timed(refill, 1)
            ms2["none"].append(m)
            for v in variants:
                m, _, last[v] = timed(lambda: run(v), 1)
                ms2[v].append(m)
        m0 = float(np.median(ms2["none"]))
        say(f"B = {B}, per-trial data (walk_device_refill_trials, the same queue and the same {T} ticks; the five walks alternate, median of {args.repeats}); "
            f"identity = the configuration's model for every trial, zero pushes and noise, gain 1; models = friction 0.3 .. 0.75 and foot scale 0.85 .. 1.15; "
            f"mismatch = pushes, noise and gains in [0.9, 1.1] on every local tick; max-sum = the sum over the ticks of the largest iteration count in the tick")
        for v in ms2:
            t2 = {k: x.cpu().numpy() for k, x in last[v]["trials"].items() if hasattr(x, "cpu")}
            ran, med = int(t2["ticks"].sum()), float(np.median(ms2[v]))
            ok = "" if v in ("none", "mismatch") else f", model_ok all 1 {bool((t2['model_ok'] == 1).all())}"
            say(f"B = {B}, {v}: {med:.2f} ms ({fmt(ms2[v])}) = {med * 1e3 / max(ran, 1):.3f} us per trial-tick, {med / T:.4f} ms per tick, / none = {med / m0:.4f} | "
                f"every trial started {bool((t2['start'] >= 0).all())}{ok}, {int((t2['end_tick'] >= 0).sum())} trials end early, {ran} trial-ticks run, "
                f"{int(t2['iterations_sum'].sum()) / max(ran, 1):.2f} iterations per trial-tick, max-sum {int(last[v]['stats'][:, 3].sum().item())}")
if ab:
    a, b = ab[args.baseline], ab["libcmpc_hip.so"]
    say(f"headline solve (bench.py config2 through tools/ab_multi.sh, {args.ab_reps} rounds), ms per step: {args.baseline} {np.median(a):.4f} ({fmt(a)}) | "
        f"this build {np.median(b):.4f} ({fmt(b)}) | this build / baseline = {np.median(b) / np.median(a):.4f}")
    a, b = walk_ab[args.baseline], walk_ab["libcmpc_hip.so"]
    say(f"walk_device, B = 256, {TT} ticks, ms per tick (median of 5 in a child process, {args.ab_reps} children per build, alternating): {args.baseline} "
        f"{np.median(a):.4f} ({fmt(a)}) | this build {np.median(b):.4f} ({fmt(b)}) | this build / baseline = {np.median(b) / np.median(a):.4f}")
if refill_ab:
    a, b = refill_ab[args.baseline], refill_ab["libcmpc_hip.so"]
    say(f"refill study, B = 256, no per-trial data, ms per walk (median of 5 in a child process, {args.ab_reps} children per build, alternating): "
        f"{args.baseline} {np.median(a):.2f} ({fmt(a)}) | this build {np.median(b):.2f} ({fmt(b)}) | this build / baseline = {np.median(b) / np.median(a):.4f}")
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
