"""Developer probe (GPU box): what the gradient of the planner's reference trajectories costs on the device walk.
B = 256, N = 20, 24 ticks, references set (a planner knot every 0.02 s), in one process after a warm-up that allocates the workspaces; the variants alternate,
`--repeats` timed regions each, the median kept, whole-call wall clock (each region ends in a device synchronise):
    reverse   backward_device()  against  backward_device_refs(): the reverse walk with its grad_p rows on + ONE launch of the reference VJP
              ... and the reverse walk alone with grad_p off against on (BatchSolver.rollout_walk_vjp_device, the same seeds and carries)
              ... and the reference VJP launch on its own: `--launches` launches between two device events, per launch
    forwards  forward_sensitivity_device()  against  forward_sensitivity_device_refs() at k = `--cols` columns of state0 (+ the reference directions): a zeroed
              dir_p, ONE launch of the reference JVP, and the walk's assemble kernel reading dir_p
No threshold: nobody has measured this before, and the forward walk itself is untouched.  Writes its lines to --out (default
profiles/r09_walk_reference_grad.txt) as well."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_walk_reference_grad.txt"))
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--ticks", type=int, default=24)
ap.add_argument("--cols", type=int, default=8)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
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
N, dt = cfg.N, cfg.sampling_time
rng = np.random.default_rng(5)
com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
h0 = rng.uniform(-0.02, 0.02, (B, 3))
push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
ro = cm.rollout.WalkingRollout(cfg, B)
in_dt = 0.02
n = int(np.ceil((T + N + 2) * dt / in_dt)) + 1
t = in_dt * np.arange(n)
ph = rng.uniform(0, 2 * np.pi, (B, 1))
com = np.stack([np.broadcast_to(ro.com_speed * t, (B, n)), 0.02 * np.sin(2 * np.pi * t / 0.96 + ph), np.full((B, n), 0.7)], -1).astype(np.float32)
h = (0.5 * np.stack([np.sin(2 * np.pi * t / 0.6 + ph), np.cos(2 * np.pi * t / 0.6 + ph), 0.3 * np.sin(2 * np.pi * t / 1.2 + ph)], -1)).astype(np.float32)
ro.set_references(com, h, in_dt, robot_mass=cm.synthetic.ROBOT_MASS)
w = ro.walk_device_taped(T, com0, dcom0, h0, push=push, push_ticks=3)
torch.cuda.synchronize()
assert int((w["end_tick"] >= 0).sum()) == 0, "a problem ended"
L, M, s, tape = ro.L, ro.M, ro.solver, w["tape"]
gS, gX = cu(rng.normal(size=(T + 1, B, 9))), cu((1e-2 * rng.normal(size=(T, B, L.nx))).astype(np.float32))
dirs = dict(dir_state0=cu(rng.normal(size=(B, K, 9))))
rdirs = dict(dir_ref_com=cu(rng.normal(size=(B, K, n, 3))), dir_ref_h=cu(rng.normal(size=(B, K, n, 3))))
z = lambda shape, d=torch.float64: torch.zeros(shape, dtype=d, device=ro.dev)


def reverse_walk(grad_p):
    """the reverse walk alone, one segment, on the solver's launch stream as _backward_device runs it"""
    with torch.cuda.stream(s.launch_stream):
        s.rollout_walk_vjp_device(0, T, tape, 0, w["end_tick"], gS, gS[T].clone(), z((B, 2, M, 3)), z((T, B), torch.int32), grad_X=gX,
                                  wrench=z((T, B, N, 6), torch.float32), grad_p=z((T, B, L.np), torch.float32) if grad_p else None,
                                  dGradPlan=z((B, 2, M, 3)), dGradModel=z((B, 34)))


# warm-up: the workspaces of the reverse and the forward walk at k = K, both kernels' code objects
r1 = ro.backward_device_refs(w, gS, gX); ro.backward_device(w, gS, gX); reverse_walk(True); reverse_walk(False)
ro.forward_sensitivity_device(w, **dirs); ro.forward_sensitivity_device_refs(w, **dirs, **rdirs)
torch.cuda.synchronize()
ms = {k: [] for k in ("bwd", "bwd_refs", "walk_off", "walk_on", "fwd", "fwd_refs")}
for _ in range(args.repeats):
    ms["bwd"].append(timed(lambda: ro.backward_device(w, gS, gX))[0])
    tt, r1 = timed(lambda: ro.backward_device_refs(w, gS, gX)); ms["bwd_refs"].append(tt)
    ms["walk_off"].append(timed(lambda: reverse_walk(False))[0])
    ms["walk_on"].append(timed(lambda: reverse_walk(True))[0])
    ms["fwd"].append(timed(lambda: ro.forward_sensitivity_device(w, **dirs))[0])
    ms["fwd_refs"].append(timed(lambda: ro.forward_sensitivity_device_refs(w, **dirs, **rdirs))[0])
# the two new launches on their own, device events around a run of them (a single one is a few microseconds)
gc, gh, dp = z((B, n, 3)), z((B, n, 3)), z((T, B, K, L.np), torch.float32)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
with torch.cuda.stream(s.launch_stream):
    s.reference_from_planner_vjp_device(0, T, tape["references"], w["end_tick"], r1["grad_P"], gc, gh)
    s.reference_from_planner_jvp_device(0, T, K, tape["references"], dp, rdirs["dir_ref_com"], rdirs["dir_ref_h"])
    ev[0].record()
    for _ in range(args.launches):
        s.reference_from_planner_vjp_device(0, T, tape["references"], w["end_tick"], r1["grad_P"], gc, gh)
    ev[1].record(); ev[2].record()
    for _ in range(args.launches):
        s.reference_from_planner_jvp_device(0, T, K, tape["references"], dp, rdirs["dir_ref_com"], rdirs["dir_ref_h"])
    ev[3].record()
torch.cuda.synchronize()
vjp_us, jvp_us = ev[0].elapsed_time(ev[1]) / args.launches * 1e3, ev[2].elapsed_time(ev[3]) / args.launches * 1e3
plain = ro.backward_device(w, gS, gX)
torch.cuda.synchronize()
same = all(torch.equal(r1[k], plain[k]) for k in ("state0", "list0", "wrench", "push", "models", "plan", "status"))
med = lambda a: float(np.median(a))
fmt = lambda a: ", ".join(f"{x:.2f}" for x in a)
say(f"reference gradients on the device walk: B = {B}, N = {N}, {T} ticks, {n} planner knots every {in_dt} s, median of {args.repeats} timed regions, ms per "
    f"whole call; {torch.cuda.get_device_name(0)}")
say(f"  reverse  backward_device {med(ms['bwd']):.2f} [{fmt(ms['bwd'])}]  backward_device_refs {med(ms['bwd_refs']):.2f} [{fmt(ms['bwd_refs'])}]  "
    f"ratio {med(ms['bwd_refs']) / med(ms['bwd']):.4f}; the other keys bit-equal: {same}")
say(f"  reverse walk alone (one call of rollout_walk_vjp_device)  grad_p off {med(ms['walk_off']):.2f} [{fmt(ms['walk_off'])}]  on {med(ms['walk_on']):.2f} "
    f"[{fmt(ms['walk_on'])}]  ratio {med(ms['walk_on']) / med(ms['walk_off']):.4f}")
say(f"  the reference VJP launch on its own ({T} rows -> [{B}, {n}, 3] x 2): {vjp_us:.1f} us per launch over {args.launches} back-to-back launches (device "
    f"events; enqueue-bound if the kernel is shorter than a launch)")
say(f"  forwards k = {K}  forward_sensitivity_device {med(ms['fwd']):.2f} [{fmt(ms['fwd'])}]  forward_sensitivity_device_refs {med(ms['fwd_refs']):.2f} "
    f"[{fmt(ms['fwd_refs'])}]  ratio {med(ms['fwd_refs']) / med(ms['fwd']):.4f}")
say(f"  the reference JVP launch on its own ({T} x {B} x {K} x {6 * (N + 1)} entries): {jvp_us:.1f} us per launch over {args.launches} back-to-back launches")
say(f"  |ref_com| max {float(r1['ref_com'].abs().max()):.3e}  |ref_h| max {float(r1['ref_h'].abs().max()):.3e}  status all 0: {bool((r1['status'] == 0).all())}")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
