"""Developer probe (GPU box): what the derivative of a device walk's stability measures costs (cmpc_walk_measures_vjp_device and its fold,
WalkingRollout.backward_device_measures), and that nothing existing moved.  B = 256, N = 20, walks of 24 ticks, medians.
(a) this build against --baseline LIB (another build of the library in the package directory, e.g. the parent commit's), in child processes started
    before this one touches the GPU: the headline solve through tools/ab_multi.sh (config2, the variants alternating inside it) and walk_device.  The
    baseline runs TWICE per round, as two variants: baseline / baseline is the spread the ratio this build / baseline is held against.
(b) the measures-VJP launch and the fold launch on a taped walk, timed by events on the launch stream, against one reverse tick of the same tape.
(c) backward_device_measures against backward_device on the same tape, alternating.
--fd "TEXT" / --resources "TEXT": lines measured elsewhere (the CPU finite-difference figures, the compiler's resource remarks), appended to --out."""
import argparse, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_walk_measures_grad.txt"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", default=None)
ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
ap.add_argument("--walk-only", action="store_true", help="print the median ms per tick of the 24-tick walk_device at B = 256 and leave")
ap.add_argument("--fd", default=None)
ap.add_argument("--resources", default=None)
args = ap.parse_args()
TT, B, lines = 24, 256, []
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish():
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)


if args.fd is not None or args.resources is not None:
    for s in (args.fd, args.resources):
        if s:
            say(s)
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
    names = ("baseline", "baseline again", "this build")
    libs = (args.baseline, args.baseline, "libcmpc_hip.so")
    ab = {"solve": {v: [] for v in names}, "walk": {v: [] for v in names}}
    r = subprocess.run(["bash", os.path.join("tools", "ab_multi.sh"), "config2", str(args.repeats)] + list(libs), cwd=ROOT, capture_output=True, text=True,
                       timeout=60 * args.repeats * len(libs))
    rows = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert r.returncode == 0 and len(rows) == args.repeats * len(libs), (r.stdout[-2000:], r.stderr[-2000:])
    for i, row in enumerate(rows):      # (lib, workload, value, ms_per_step), the variants in turn
        assert row[0] == libs[i % 3], row
        ab["solve"][names[i % 3]].append(float(row[3]))
    for _ in range(args.repeats):
        for v, lib in zip(names, libs):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--walk-only"], cwd=ROOT, capture_output=True, text=True,
                               env=dict(os.environ, CMPC_LIB=lib), timeout=180)
            assert r.returncode == 0, r.stderr[-2000:]
            ab["walk"][v].append(float(r.stdout.split()[-1]))
            print(v, ab["walk"][v][-1], flush=True)

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

say(f"the measures of a device walk, differentiated: N = {cfg.N}, B = {B}, a taped walk of {TT} ticks, medians of {args.repeats}; {torch.cuda.get_device_name(0)}")
if ab:
    for what, unit in (("solve", "headline solve (tools/ab_multi.sh config2, 30 steps), ms per step"), ("walk", "walk_device, ms per tick (median of 5 per child)")):
        a, a2, b = (ab[what][v] for v in ("baseline", "baseline again", "this build"))
        say(f"(a) {unit}: {args.baseline} {np.median(a):.4f} ({fmt(a)}) | the same again {np.median(a2):.4f} ({fmt(a2)}) | this build {np.median(b):.4f} ({fmt(b)}) | "
            f"baseline again / baseline = {np.median(a2) / np.median(a):.4f} (the spread) | this build / baseline = {np.median(b) / np.median(a):.4f}")

w = ro.walk_device_taped(TT, com0, dcom0, h0, push=push, push_ticks=3)
tape, s, L = w["tape"], ro.solver, ro.L
rng = np.random.default_rng(7)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ro.dev)
gM, gS = dev(rng.normal(size=(TT, B, 4))), dev(rng.normal(size=(TT + 1, B, 9)))
gX = dev((1e-2 * rng.normal(size=(TT, B, L.nx))).astype(np.float32))
ro.backward_device_measures(w, gM, gS, gX, refs=True)      # warm-up: the reverse walk's workspaces
ro.backward_device(w, gS, gX)
torch.cuda.synchronize()


def on_stream(fn, n=20):
    """fn queued on the launch stream between two events, n times -> ms each"""
    out = []
    with torch.cuda.stream(s.launch_stream):
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    return out


seedS, seedX, direct = gS.clone(), gX.clone(), torch.zeros((TT, B, 32), dtype=torch.float64, device=ro.dev)
gP, gModel = torch.zeros((TT, B, L.np), dtype=torch.float32, device=ro.dev), torch.zeros((B, 34), dtype=torch.float64, device=ro.dev)
vjp = on_stream(lambda: s.walk_measures_vjp_device(0, TT, tape, 0, w["end_tick"], gM, seedS, seedX, direct))
fold = on_stream(lambda: s.walk_measures_vjp_fold_device(direct, gP, gModel))
z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=ro.dev)
g, gl, status = gS[TT].clone(), z((B, 2, ro.M, 3)), z((TT, B), torch.int32)
tick = on_stream(lambda: s.rollout_walk_vjp_device(TT - 1, 1, tape, TT - 1, w["end_tick"], gS, g, gl, status, grad_X=gX), n=10)
say(f"(b) events on the launch stream, ms: the measures VJP over all {TT} rows x {B} problems {np.median(vjp):.4f} (min {min(vjp):.4f}) | the fold "
    f"{np.median(fold):.4f} (min {min(fold):.4f}) | ONE reverse tick of the same tape (two gate launches and the tick VJP) {np.median(tick):.4f} (min {min(tick):.4f}) | "
    f"VJP / one reverse tick = {np.median(vjp) / np.median(tick):.4f}, (VJP + fold) / the {TT} reverse ticks = "
    f"{(np.median(vjp) + np.median(fold)) / (TT * np.median(tick)):.5f}")
ms = {"plain": [], "measures": []}
for _ in range(args.repeats):
    ms["plain"].append(timed(lambda: ro.backward_device(w, gS, gX))[0])
    ms["measures"].append(timed(lambda: ro.backward_device_measures(w, gM, gS, gX))[0])
mp, mm = float(np.median(ms["plain"])), float(np.median(ms["measures"]))
say(f"(c) backward_device_measures against backward_device on the same tape, ms per reverse walk: plain {mp:.3f} ({fmt(ms['plain'])}) | with the measures "
    f"{mm:.3f} ({fmt(ms['measures'])}) | ratio {mm / mp:.4f} | {(mm - mp) * 1e3:.0f} us more per reverse walk of {TT} ticks (two launches and the copies of the two seeds)")
finish()
