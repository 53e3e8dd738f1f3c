"""Developer probe (GPU box): what the reverse walk from checkpoints costs against the reverse walk from a whole-walk tape, in time and in memory.
B = 256, N = 20, 24 ticks, one process; after a warm-up of every variant (module load, allocator, workspaces) five timed regions each, the variants
alternating, the median kept; a region is the whole pair of calls and ends in a device synchronise:
    full     walk_device_taped() + backward_device()
    every4   walk_device_checkpointed(every=4) + backward_device_checkpointed()
    every8   the same at every = 8
with seeds on every state and every solution.  Also recorded: torch.cuda.max_memory_allocated over one region of each (the peak statistics reset in
front of it; what lives from before -- the inputs, the seeds, the handles' workspaces -- is reported as the floor), and the snapshot launch alone over
200 back-to-back launches.  The gradients of the three variants are compared bit for bit.  No threshold: nobody has measured this before; the
expectation is one extra forward walk, about a tenth of the pair.  Writes its lines to --out (default profiles/r10_walk_checkpoint.txt) as well."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_walk_checkpoint.txt"))
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--ticks", type=int, default=24)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

import torch
import cmpc_amd as cm

B, T, lines = args.batch, args.ticks, []


def say(s):
    print(s, flush=True)
    lines.append(s)


cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
L = cm.Layout(cfg.N)
rng = np.random.default_rng(5)
com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
h0 = rng.uniform(-0.02, 0.02, (B, 3))
push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
gS = torch.from_numpy(rng.normal(size=(T + 1, B, 9))).cuda()
gX = torch.from_numpy((1e-2 * rng.normal(size=(T, B, L.nx))).astype(np.float32)).cuda()
kw = dict(push=push, push_ticks=3, trace=False)
ros = {k: cm.rollout.WalkingRollout(cfg, B) for k in ("full", "every4", "every8")}


def pair(k):
    ro = ros[k]
    if k == "full":
        return ro.backward_device(ro.walk_device_taped(T, com0, dcom0, h0, **kw), gS, gX)
    return ro.backward_device_checkpointed(ro.walk_device_checkpointed(T, com0, dcom0, h0, int(k[5:]), **kw), gS, gX)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


for k in ros:      # warm-up
    pair(k)
torch.cuda.synchronize()
ms, last = {k: [] for k in ros}, {}
for _ in range(args.repeats):
    for k in ros:
        t, last[k] = timed(lambda: pair(k))
        ms[k].append(t)
same = {k: all(torch.equal(last[k][g], last["full"][g]) for g in ("state0", "list0", "wrench", "push", "models", "plan", "status")) for k in ("every4", "every8")}
del last
peak = {}
for k in ros:
    torch.cuda.synchronize()
    floor = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = pair(k)
    torch.cuda.synchronize()
    peak[k] = (torch.cuda.max_memory_allocated(), floor, int(r.get("tape_rows_peak", T)))
    del r
# the snapshot launch alone
ro = ros["every4"]
s = ro.solver
w = ro.walk_device_checkpointed(8, com0, dcom0, h0, 4, **kw)
src, dst = w["checkpoints"][4], s.walk_snapshot(0, 0, ro.M)
with torch.cuda.stream(s.launch_stream):
    for _ in range(20):
        s.rollout_snapshot_device(src, dst)
    t_snap, _ = timed(lambda: [s.rollout_snapshot_device(src, dst) for _ in range(200)])
snap_bytes = int(cm._capi.lib().cmpc_walk_snapshot_bytes(cfg.N, ro.M))

med = lambda a: float(np.median(a))
fmt = lambda a: ", ".join(f"{x:.2f}" for x in a)
mib = lambda b: f"{b / 2**20:.1f} MiB"
say(f"the reverse walk from checkpoints: B = {B}, N = {cfg.N}, {T} ticks, variants alternating, median of {args.repeats} timed regions after a warm-up, "
    f"ms per region (forward walk + reverse walk, seeds on states and solutions); {torch.cuda.get_device_name(0)}")
m = {k: med(v) for k, v in ms.items()}
say(f"full tape: walk_device_taped() + backward_device() {m['full']:.2f} ({fmt(ms['full'])})")
for k in ("every4", "every8"):
    say(f"{k}: walk_device_checkpointed() + backward_device_checkpointed() {m[k]:.2f} ({fmt(ms[k])}) | / full tape = {m[k] / m['full']:.4f} | "
        f"gradients bit-identical to the full tape's: {same[k]}")
tape_row = 4 * (L.nx + L.np + L.ng) + 64 * ro.M + 96
for k in ros:
    p, floor, rows = peak[k]
    say(f"{k}: peak torch.cuda.max_memory_allocated {mib(p)}, {mib(p - floor)} above the {mib(floor)} allocated in front of the region | tape rows at "
        f"most {rows} ({mib(rows * B * tape_row)})" + ("" if k == "full" else f", {len(range(int(k[5:]), T, int(k[5:])))} snapshots ({mib(len(range(int(k[5:]), T, int(k[5:]))) * B * snap_bytes)})"))
say(f"snapshot launch alone: 200 back-to-back launches {t_snap:.3f} ms, {1e3 * t_snap / 200:.2f} us each; {snap_bytes} bytes per problem read and written, "
    f"{2 * snap_bytes * B * 200 / (t_snap * 1e-3) / 1e9:.1f} GB/s at B = {B}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
