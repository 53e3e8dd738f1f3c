"""Developer probe (GPU box): what a tick of the device walk costs against the host-driven roll-out.  60 ticks at N = 20, B = 256 and B = 1024, three
repeats each after a warm-up, the median kept, whole-call wall clock divided by the ticks (set-up included on every side):
    run(record="light", timing=False)   the yardstick: three launches per tick, the host reads ok and the status words after every tick
    run(record="full")                  the same plus the trajectory copied out and the landing offsets formed on the host
    walk_device(trace=True)             four launches per tick, nothing read back (the record kernel writes the trace)
and the record launch on its own (60 launches back to back on ticks the walk left, one synchronisation).  walk_device must not be slower per tick than
the yardstick by more than 2 % (the box-to-box spread of README's benchmark section); the verdict is printed, and the exit status is 1 when it is.
Writes its lines to --out (default profiles/r05_walk_device.txt) as well."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import cmpc_amd as cm

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_walk_device.txt"))
ap.add_argument("--ticks", type=int, default=60)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
T, lines, slow = args.ticks, [], False


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / T)
    return float(np.median(ms)), ms, r


say(f"device walk against the host-driven roll-out: N = {cfg.N}, {T} ticks, median of {args.repeats} repeats, ms per tick (whole call / ticks); {torch.cuda.get_device_name(0)}")
for B in (256, 1024):
    rng = np.random.default_rng(5)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    ro = cm.rollout.WalkingRollout(cfg, B)
    ro.run(8, com0, dcom0, h0, push=push, push_ticks=3, record="light")          # warm-up (module load, allocator)
    ro.walk_device(8, com0, dcom0, h0, push=push, push_ticks=3)
    light, l_all, rec = timed(lambda: ro.run(T, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False))
    full, f_all, _ = timed(lambda: ro.run(T, com0, dcom0, h0, push=push, push_ticks=3, record="full"))
    walk, w_all, w = timed(lambda: ro.walk_device(T, com0, dcom0, h0, push=push, push_ticks=3, trace=True))
    assert "aborted_tick" not in rec and (w["end_tick"] == -1).all().item()
    same = np.array_equal(w["iterations"].cpu().numpy().max(1), np.array(rec["iterations_max"]))
    # the record launch alone, on what the walk left
    s, r1 = ro.solver, ro.solver.walk_record(T)
    s.outcome_init_device(w["state"], r1)
    land, zmp = w["land"][-1].contiguous(), w["zmp"][-1].contiguous()
    with torch.cuda.stream(s.launch_stream):
        def records():
            for i in range(T):
                s.rollout_record_device(i, i, w["X"], w["P"], w["info"], None, land, w["state"], zmp, r1)
        records()
        one, _, _ = timed(records)
    fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)
    say(f"B = {B}: run(light, timing=False) {light:.4f} ({fmt(l_all)}) | run(full) {full:.4f} ({fmt(f_all)}) | walk_device(trace) {walk:.4f} ({fmt(w_all)}) | "
        f"record launch alone (a memset and a kernel) {one * 1e3:.1f} us | run's own tick_ms p50 {np.median(rec['tick_ms'][1:]):.4f}")
    ratio = walk / light
    slow = slow or ratio > 1.02
    say(f"B = {B}: walk_device / run(light) = {ratio:.4f} ({'within' if ratio <= 1.02 else 'ABOVE'} the 2 % bound); run(full) / walk_device = {full / walk:.2f}; "
        f"per-tick iteration maxima equal to run's: {same}")
say("verdict: " + ("walk_device is slower than the yardstick by more than 2 %" if slow else "walk_device is not slower than the yardstick by more than 2 %"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if slow else 0)
