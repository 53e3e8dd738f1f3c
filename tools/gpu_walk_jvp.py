"""Developer probe (GPU box): what the forward-mode device walk costs against the host-driven forward sweep.
B = 256, N = 20, 24 ticks, k = 8 direction columns (state0, push and models), in one process after a warm-up that allocates the workspaces of both paths; the
two variants alternate, `--repeats` timed regions each, the median kept, whole-call wall clock (each region ends in a device synchronise):
    host    run(tape=True, record="light", timing=False) + forward_sensitivity(): a Python loop of clones and one tick JVP call per tick
    device  walk_device_taped() + forward_sensitivity_device(): one C call per segment for the walk and one for the sweep, no host read
The two halves (walk, sweep) are timed apart as well.  Expected: device / host <= 1.0 beyond the ~2 % box-to-box spread README.md records; the line says
which way it went and by how much, and nothing is tuned around it.  Writes its lines to --out (default profiles/r07_walk_jvp.txt) as well."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_walk_jvp.txt"))
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--ticks", type=int, default=24)
ap.add_argument("--cols", type=int, default=8)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
B, T, K, lines = args.batch, args.ticks, args.cols, []

import torch
import cmpc_amd as cm


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
rng = np.random.default_rng(5)
com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
h0 = rng.uniform(-0.02, 0.02, (B, 3))
push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
theta = cm.config.model_row(cfg)
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
dirs = dict(dir_state0=cu(rng.normal(size=(B, K, 9))), dir_push=cu(rng.normal(size=(B, K, 3)).astype(np.float32)),
            dir_models=cu(rng.normal(size=(B, K, 34)) * np.abs(theta).clip(1e-2) * 0.1))
ro_run, ro = cm.rollout.WalkingRollout(cfg, B), cm.rollout.WalkingRollout(cfg, B)
walk_host = lambda n=T: ro_run.run(n, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False, tape=True)
walk_dev = lambda n=T: ro.walk_device_taped(n, com0, dcom0, h0, push=push, push_ticks=3)
# warm-up: module load, allocator, the tick JVP's workspace at k = K on both handles and the walk's own on the device side
ro_run.forward_sensitivity(walk_host(4)["tape"], **dirs)
ro.forward_sensitivity_device(walk_dev(4), **dirs)
torch.cuda.synchronize()
ms = {k: [] for k in ("host_walk", "host_sweep", "dev_walk", "dev_sweep")}
for _ in range(args.repeats):
    t, rec = timed(walk_host); ms["host_walk"].append(t)
    t, fh = timed(lambda: ro_run.forward_sensitivity(rec["tape"], **dirs)); ms["host_sweep"].append(t)
    t, w = timed(walk_dev); ms["dev_walk"].append(t)
    t, fd = timed(lambda: ro.forward_sensitivity_device(w, **dirs)); ms["dev_sweep"].append(t)
assert len(rec["tape"]["ticks"]) == T and int((w["end_tick"] >= 0).sum()) == 0, "a problem ended: the two paths did not do the same work"
same = all(torch.equal(fd[k], fh[k]) for k in ("states", "list", "status", "removed"))
med = lambda a: float(np.median(a))
fmt = lambda a: ", ".join(f"{x:.2f}" for x in a)
host, dev = med(ms["host_walk"]) + med(ms["host_sweep"]), med(ms["dev_walk"]) + med(ms["dev_sweep"])
say(f"the device walk forwards: B = {B}, N = {cfg.N}, {T} ticks, k = {K} columns (state0, push, models), median of {args.repeats} timed regions, ms per "
    f"whole call; {torch.cuda.get_device_name(0)}")
say(f"  host   run(tape=True) {med(ms['host_walk']):.2f} [{fmt(ms['host_walk'])}]  + forward_sensitivity {med(ms['host_sweep']):.2f} [{fmt(ms['host_sweep'])}]  = {host:.2f}")
say(f"  device walk_device_taped {med(ms['dev_walk']):.2f} [{fmt(ms['dev_walk'])}]  + forward_sensitivity_device {med(ms['dev_sweep']):.2f} [{fmt(ms['dev_sweep'])}]  = {dev:.2f}")
say(f"  device / host: whole {dev / host:.4f}, sweep alone {med(ms['dev_sweep']) / med(ms['host_sweep']):.4f} "
    f"({'no slower' if dev <= 1.02 * host else 'SLOWER'} than the host loop, 2 % spread allowed); results bit-equal: {same}")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
