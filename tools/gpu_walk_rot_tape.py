"""Developer probe (GPU box): what the orientation chain costs the reverse device walk, and what the device pair saves over the host-driven sweep.
B = 256, N = 20, 24 ticks over a yawed plan (the footsteps after each foot's first yawed U(-0.2, 0.2) rad per problem), seeds on every state, in one process
after a warm-up that allocates the workspaces of every path; the variants alternate, `--repeats` timed regions each, the median kept, whole-call wall clock
(each region ends in a device synchronise):
    rot     backward_device_rot(w): cmpc_rollout_walk_vjp_rot_device, one C call, the rotation tick VJP per row (one launch more a tick)
    plain   backward_device(w): cmpc_rollout_walk_vjp_device on the same tape
    host    run(tape=True, record="light", timing=False) + backward(rot=True): the Python loop, two host reads a tick; its walk is timed apart
No ratio between these is fixed in advance: the lines say what came out.
With --baseline LIB (another build of the library in the package directory, e.g. the parent commit's) the untouched paths must not pay: the headline solve
of bench.py through tools/ab_multi.sh, and backward_device() in child processes started before this one touches the GPU, both builds in turn.
    bound: this build / LIB <= 1.01 (three times the 0.3 % in-call spread README.md records for ab_multi.sh runs)
The exit status is 1 when that bound is missed.  Writes its lines to --out (default profiles/r08_walk_rot_tape.txt) as well."""
import argparse, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_walk_rot_tape.txt"))
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--ticks", type=int, default=24)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", default=None, help="file name of another build of the library in the package directory")
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--child-backward", action="store_true", help="internal: time backward_device() with the library CMPC_LIB names and print the median")
args = ap.parse_args()
B, T, BOUND, lines, missed = args.batch, args.ticks, 1.01, [], []


def say(s):
    print(s, flush=True)
    lines.append(s)


def check(name, ratio):
    good = ratio <= BOUND
    if not good:
        missed.append(name)
    return f"{ratio:.4f} ({'within' if good else 'ABOVE'} the bound {BOUND})"


def scene(cm, torch):
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    rng = np.random.default_rng(5)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS

    def rollout():
        ro = cm.rollout.WalkingRollout(cfg, B)
        yaw = np.zeros((B, 2, ro.M))
        yaw[:, :, 1:] = np.random.default_rng(21).uniform(-0.2, 0.2, (B, 2, ro.M - 1))
        ro.plan = (ro.plan[0], cm.rollout.yaw_plan_poses(ro.plan[1], torch.from_numpy(yaw).to(ro.dev)), ro.plan[2])
        return ro
    gS = torch.from_numpy(np.random.default_rng(1).normal(size=(T + 1, B, 9))).cuda()
    return cfg, rollout, (com0, dcom0, h0), dict(push=push, push_ticks=3), gS


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


if args.child_backward:
    import torch
    import cmpc_amd as cm
    cfg, rollout, start, kw, gS = scene(cm, torch)
    ro = rollout()
    ro.backward_device(ro.walk_device_taped(4, *start, **kw), gS[:5])
    w = ro.walk_device_taped(T, *start, **kw)
    print("backward", float(np.median([timed(torch, lambda: ro.backward_device(w, gS))[0] for _ in range(args.repeats)])))
    sys.exit(0)

ab, abb = None, None
if args.baseline:      # first: fresh child processes, this one has not opened the GPU yet
    libs = [args.baseline, "libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True).stdout
    ab = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab:
            ab[w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab.values()), out
    abb = {lib: [] for lib in libs}
    for _ in range(args.ab_reps):
        for lib in libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-backward", "--batch", str(B), "--ticks", str(T), "--repeats", str(args.repeats)],
                               cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, CMPC_LIB=lib))
            assert o.returncode == 0, o.stderr[-2000:]
            abb[lib] += [float(ln.split()[1]) for ln in o.stdout.splitlines() if ln.startswith("backward ")]
    assert all(len(v) == args.ab_reps for v in abb.values()), abb

import torch
import cmpc_amd as cm

cfg, rollout, start, kw, gS = scene(cm, torch)
ro, ro_run = rollout(), rollout()
walk_host = lambda n=T: ro_run.run(n, *start, record="light", timing=False, tape=True, **kw)
# warm-up: module load, allocator, the tick VJP's and the walk's workspaces on both handles
w4 = ro.walk_device_taped(4, *start, **kw)
ro.backward_device_rot(w4, gS[:5]); ro.backward_device(w4, gS[:5])
ro_run.backward(walk_host(4)["tape"], gS[:5], rot=True)
torch.cuda.synchronize()
w = ro.walk_device_taped(T, *start, **kw)
ms = {k: [] for k in ("rot", "plain", "host_walk", "host_sweep")}
for _ in range(args.repeats):
    t, gr = timed(torch, lambda: ro.backward_device_rot(w, gS)); ms["rot"].append(t)
    t, gp = timed(torch, lambda: ro.backward_device(w, gS)); ms["plain"].append(t)
    t, rec = timed(torch, walk_host); ms["host_walk"].append(t)
    t, gh = timed(torch, lambda: ro_run.backward(rec["tape"], gS, rot=True)); ms["host_sweep"].append(t)
ended = int((w["end_tick"] >= 0).sum())
assert len(rec["tape"]["ticks"]) == T and ended == 0, "a problem ended: the paths did not do the same work"
same_host = all(torch.equal(gr[k], gh[k]) for k in ("state0", "list0", "wrench", "push", "models", "plan", "status", "list_rot0", "plan_rot", "rot", "removed"))
same_plain = all(torch.equal(gr[k], gp[k]) for k in ("state0", "list0", "wrench", "push", "models", "plan", "status"))
med = lambda a: float(np.median(a))
fmt = lambda a: ", ".join(f"{x:.2f}" for x in a)
say(f"the reverse device walk with orientations: B = {B}, N = {cfg.N}, {T} ticks over a yawed plan, seeds on every state, variants alternating, median of "
    f"{args.repeats} timed regions, ms per whole call; {torch.cuda.get_device_name(0)}")
say(f"  backward_device_rot {med(ms['rot']):.2f} [{fmt(ms['rot'])}] | backward_device {med(ms['plain']):.2f} [{fmt(ms['plain'])}] | rot / plain = "
    f"{med(ms['rot']) / med(ms['plain']):.4f}, {1e3 * (med(ms['rot']) - med(ms['plain'])) / T:.1f} us per tick more | shared keys bit-equal: {same_plain}")
say(f"  host-driven: run(tape=True) {med(ms['host_walk']):.2f} [{fmt(ms['host_walk'])}] + backward(rot=True) {med(ms['host_sweep']):.2f} "
    f"[{fmt(ms['host_sweep'])}] | backward_device_rot / backward(rot=True) = {med(ms['rot']) / med(ms['host_sweep']):.4f} | every key bit-equal: {same_host}; "
    f"max |plan_rot| {float(gr['plan_rot'].abs().max()):.3e}, ticks with removed = 0 everywhere: {int((gr['removed'] == 0).all(1).sum())} of {T}")
if ab:
    new, old = med(ab["libcmpc_hip.so"]), med(ab[args.baseline])
    say(f"  untouched paths against {args.baseline}: headline solve (bench.py config2 through tools/ab_multi.sh, {args.ab_reps} rounds), ms per step: baseline "
        f"{old:.4f} [{', '.join(f'{x:.4f}' for x in ab[args.baseline])}] | this build {new:.4f} [{', '.join(f'{x:.4f}' for x in ab['libcmpc_hip.so'])}] | this "
        f"build / baseline = {check('solve', new / old)}")
    new, old = med(abb["libcmpc_hip.so"]), med(abb[args.baseline])
    say(f"  untouched paths against {args.baseline}: backward_device(), child processes alternating, {args.ab_reps} rounds of the median of {args.repeats}, ms "
        f"per call: baseline {old:.2f} [{fmt(abb[args.baseline])}] | this build {new:.2f} [{fmt(abb['libcmpc_hip.so'])}] | this build / baseline = "
        f"{check('backward_device', new / old)}")
else:
    say("  untouched paths against a baseline build: not run (no --baseline)")
say("  verdict: " + ("bound missed: " + "; ".join(missed) if missed else "every bound holds" if ab else "nothing was bounded"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if missed else 0)
