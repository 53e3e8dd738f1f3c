"""Developer probe (GPU box): what the plant-model mismatch costs on the device walk (include/cmpc.h, "plant-model mismatch on the device walk").
N = 20, B = 256, 24 ticks, in one process after a warm-up; the variants alternate, `--repeats` repeats each, the median kept, whole-call wall clock (the
call ends in a device synchronise) divided by the ticks, set-up included on every side:
    (a) walk_device() against walk_device_mismatch() with all three set (24 rows of hidden pushes, 24 of state noise, a gain per problem), and against
        the UNIT mismatch (zero pushes, zero noise, gain 1: the same walk to the bit through the mismatch kernels -- what the kernels themselves cost; the
        disturbed walk also pays for the iterations its solves need more, reported beside it).
    (b) walk_device_taped() + backward_device for both: the reverse walk then runs the mismatch instantiation of the plant VJP and writes three more outputs.
    (c) with --baseline LIB (another build of the library in the package directory: the parent commit's): the walk WITHOUT a mismatch must not pay for the
        feature.  The headline solve of bench.py through tools/ab_multi.sh, and walk_device() without a mismatch, both builds in turn in child processes
        started before this one touches the GPU.  README.md gives the in-call spread of such runs as about 0.3 %; a larger gap is said in the file.  It is a
        finding, not a gate: the exit status is 0 either way.
Writes its lines to --out (default profiles/r11_walk_mismatch.txt) as well."""
import argparse, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_walk_mismatch.txt"))
ap.add_argument("--ticks", type=int, default=24)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", default=None, help="file name of another build of the library in the package directory: part (c)")
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--child-walk", action="store_true", help="internal: time walk_device() with the library CMPC_LIB names and print the median")
args = ap.parse_args()
SPREAD = 0.003
T, B, lines = args.ticks, args.batch, []


def say(s):
    print(s, flush=True)
    lines.append(s)


def start(cm):
    rng = np.random.default_rng(5)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    return com0, dcom0, h0


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / T, r


if args.child_walk:
    import torch
    import cmpc_amd as cm
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    com0, dcom0, h0 = start(cm)
    ro = cm.rollout.WalkingRollout(cfg, B)
    ro.walk_device(8, com0, dcom0, h0)
    ms = [timed(torch, lambda: ro.walk_device(T, com0, dcom0, h0))[0] for _ in range(args.repeats)]
    print("walk", B, float(np.median(ms)))
    sys.exit(0)

ab, abw = None, None
if args.baseline:      # (c) first: fresh child processes, this one has not opened the GPU yet
    libs = [args.baseline, "libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True).stdout
    ab = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab:
            ab[w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab.values()), out
    abw = {lib: [] for lib in libs}
    for _ in range(args.ab_reps):
        for lib in libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-walk", "--ticks", str(T), "--batch", str(B), "--repeats", str(args.repeats)],
                               cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, CMPC_LIB=lib))
            assert o.returncode == 0, o.stderr[-2000:]
            for ln in o.stdout.splitlines():
                w = ln.split()
                if len(w) == 3 and w[0] == "walk":
                    abw[lib].append(float(w[2]))
    assert all(len(v) == args.ab_reps for v in abw.values()), abw

import torch
import cmpc_amd as cm

cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)
med = lambda a: float(np.median(a))
say(f"plant-model mismatch on the device walk: N = {cfg.N}, B = {B}, {T} ticks, variants alternating, median of {args.repeats} repeats, ms per tick (whole "
    f"call / ticks); {torch.cuda.get_device_name(0)}")
com0, dcom0, h0 = start(cm)
rng = np.random.default_rng(7)
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
mm = dict(hidden_wrench=cu(np.concatenate([rng.normal(0, 0.3, (T, B, 3)), rng.normal(0, 0.05, (T, B, 3))], -1)),
          state_noise=cu(np.concatenate([rng.normal(0, 3e-3, (T, B, 3)), rng.normal(0, 1e-2, (T, B, 3)), rng.normal(0, 2e-3, (T, B, 3))], -1)),
          force_gain=cu(rng.uniform(0.9, 1.1, B)), tick_first=0)
unit = dict(hidden_wrench=torch.zeros_like(mm["hidden_wrench"]), state_noise=torch.zeros_like(mm["state_noise"]), force_gain=torch.ones_like(mm["force_gain"]),
            tick_first=0)
ro, ro_plain = cm.rollout.WalkingRollout(cfg, B), cm.rollout.WalkingRollout(cfg, B)      # (ro_plain never tapes: its multiplier output stays off)
gS = torch.from_numpy(np.random.default_rng(1).normal(size=(T + 1, B, 9))).cuda()


def pair(m):
    w = ro.walk_device_taped(T, com0, dcom0, h0, mismatch=m)
    return w, ro.backward_device(w, gS)


variants = (("plain", lambda: ro_plain.walk_device(T, com0, dcom0, h0)), ("mismatch", lambda: ro_plain.walk_device_mismatch(T, com0, dcom0, h0, mm)),
            ("unit", lambda: ro_plain.walk_device_mismatch(T, com0, dcom0, h0, unit)),
            ("pair_plain", lambda: pair(None)), ("pair_mismatch", lambda: pair(mm)))
for _, fn in variants:      # warm-up (module load, allocator, the workspaces of the reverse walk)
    fn()
ms = {k: [] for k, _ in variants}
last = {}
for _ in range(args.repeats):
    for k, fn in variants:
        t, last[k] = timed(torch, fn)
        ms[k].append(t)
m = {k: med(v) for k, v in ms.items()}
ended = {k: int((w["end_tick"] >= 0).sum()) for k, w in (("plain", last["plain"]), ("mismatch", last["mismatch"]))}
moved = float((last["mismatch"]["final_state"] - last["plain"]["final_state"]).abs().max())
its = {k: float(last[k]["iterations_sum"].double().mean()) / T for k in ("plain", "mismatch", "unit")}
same_unit = all(torch.equal(last["unit"][k], last["plain"][k]) for k in ("X", "state", "iterations", "end_tick"))
say(f"(a) walk_device without a mismatch {m['plain']:.4f} ({fmt(ms['plain'])}), {its['plain']:.2f} iterations per solve | unit mismatch {m['unit']:.4f} "
    f"({fmt(ms['unit'])}), {its['unit']:.2f} iterations, the same walk to the bit: {same_unit} | unit / without = {m['unit'] / m['plain']:.4f}, "
    f"{1e3 * (m['unit'] - m['plain']):+.1f} us per tick: the kernels' own cost")
say(f"(a) with all three {m['mismatch']:.4f} ({fmt(ms['mismatch'])}), {its['mismatch']:.2f} iterations per solve | with / without = "
    f"{m['mismatch'] / m['plain']:.4f}, {1e3 * (m['mismatch'] - m['plain']):+.1f} us per tick, the disturbed robots' harder solves included | ended problems "
    f"{ended['plain']} / {ended['mismatch']}, largest difference of a final state {moved:.3e}")
g = last["pair_mismatch"][1]
say(f"(b) walk_device_taped + backward_device without a mismatch {m['pair_plain']:.4f} ({fmt(ms['pair_plain'])}) | with all three {m['pair_mismatch']:.4f} "
    f"({fmt(ms['pair_mismatch'])}) | with / without = {m['pair_mismatch'] / m['pair_plain']:.4f}, {1e3 * (m['pair_mismatch'] - m['pair_plain']):+.1f} us per tick | "
    f"largest |d/d hidden_wrench| {float(g['hidden_wrench'].abs().max()):.3e}, |d/d state_noise| {float(g['state_noise'].abs().max()):.3e}, |d/d force_gain| "
    f"{float(g['force_gain'].abs().max()):.3e}")
if ab:
    note = lambda r: f"{r:.4f} (" + ("inside" if abs(r - 1.0) <= SPREAD else "OUTSIDE: this build " + ("slower" if r > 1.0 else "faster") + " by more than") + \
        f" the in-call spread of {100 * SPREAD:.1f} %)"
    new, old = med(ab["libcmpc_hip.so"]), med(ab[args.baseline])
    say(f"(c) headline solve (bench.py config2 through tools/ab_multi.sh, {args.ab_reps} rounds), ms per step: {args.baseline} {old:.4f} "
        f"({fmt(ab[args.baseline])}) | this build {new:.4f} ({fmt(ab['libcmpc_hip.so'])}) | this build / baseline = {note(new / old)}")
    new, old = med(abw["libcmpc_hip.so"]), med(abw[args.baseline])
    say(f"(c) walk_device() without a mismatch, child processes alternating, {args.ab_reps} rounds of the median of {args.repeats}, ms per tick: "
        f"{args.baseline} {old:.4f} ({fmt(abw[args.baseline])}) | this build {new:.4f} ({fmt(abw['libcmpc_hip.so'])}) | this build / baseline = {note(new / old)}")
else:
    say("(c) not run (no --baseline)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
