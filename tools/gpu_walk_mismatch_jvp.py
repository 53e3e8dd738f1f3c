"""Developer probe (GPU box): what forward mode and the checkpointed reverse cost under a plant mismatch (include/cmpc.h, "the mismatch FORWARDS";
WalkingRollout.forward_sensitivity_device_mismatch, backward_device_checkpointed_mismatch).
N = 20, B = 256, 24 ticks, k = 8, in one process after a warm-up that allocates; the variants alternate, `--repeats` timed regions each, the median kept,
whole-call wall clock (the call ends in a device synchronise) divided by the ticks:
    (a) forward_sensitivity_device_mismatch on a UNIT-mismatch tape (zero pushes, zero noise, gain 1: the plain walk to the bit, through the mismatched
        plant instantiation) with the state0 direction alone, against forward_sensitivity_device on the plain tape with the same direction: what the
        instantiation itself costs.
    (b) the same with all three parts set and all three direction groups given.
    (c) backward_device_checkpointed_mismatch at every = 4 and every = 8 (walk_device_checkpointed + the reverse; the forward walk of a segment runs twice)
        against walk_device_taped + backward_device on the full tape, with torch's peak allocation over each (the library's own workspaces, a few MB that
        do not grow with the ticks, are outside it).
    (d) with --baseline LIB (another build of the library in the package directory: the parent commit's): what existed must not pay for the feature -- the
        headline solve of bench.py through tools/ab_multi.sh, walk_device() and forward_sensitivity_device on a plain tape, both builds in turn in child
        processes started before this one touches the GPU.  README.md gives the in-call spread of such runs as about 0.3 %; a larger gap is said in the
        file.  A finding, not a gate: the exit status is 0 either way.
Writes its lines to --out (default profiles/r15_walk_mismatch_jvp.txt) as well."""
import argparse, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_walk_mismatch_jvp.txt"))
ap.add_argument("--ticks", type=int, default=24)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", default=None, help="file name of another build of the library in the package directory: part (d)")
ap.add_argument("--ab-reps", type=int, default=3)
ap.add_argument("--child", action="store_true", help="internal: time walk_device() and forward_sensitivity_device with the library CMPC_LIB names")
args = ap.parse_args()
SPREAD = 0.003
T, B, K, lines = args.ticks, args.batch, args.k, []


def say(s):
    print(s, flush=True)
    lines.append(s)


def start():
    rng = np.random.default_rng(5)
    return np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3)), rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.02, 0.02, (B, 3))


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / T, r


if args.child:
    import torch
    import cmpc_amd as cm
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    com0, dcom0, h0 = start()
    ro, ro_t = cm.rollout.WalkingRollout(cfg, B), cm.rollout.WalkingRollout(cfg, B)
    ds = torch.from_numpy(np.random.default_rng(2).normal(size=(B, K, 9))).cuda()
    ro.walk_device(8, com0, dcom0, h0)
    w = ro_t.walk_device_taped(T, com0, dcom0, h0)
    ro_t.forward_sensitivity_device(w, dir_state0=ds)
    walk, fwd = [], []
    for _ in range(args.repeats):
        walk.append(timed(torch, lambda: ro.walk_device(T, com0, dcom0, h0))[0])
        fwd.append(timed(torch, lambda: ro_t.forward_sensitivity_device(w, dir_state0=ds))[0])
    print("child", float(np.median(walk)), float(np.median(fwd)))
    sys.exit(0)

ab, abc = None, None
if args.baseline:      # (d) first: fresh child processes, this one has not opened the GPU yet
    libs = [args.baseline, "libcmpc_hip.so"]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "ab_multi.sh"), "config2", str(args.ab_reps)] + libs, cwd=ROOT, capture_output=True, text=True).stdout
    ab = {lib: [] for lib in libs}
    for ln in out.splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] in ab:
            ab[w[0]].append(float(w[3]))
    assert all(len(v) == args.ab_reps for v in ab.values()), out
    abc = {lib: ([], []) for lib in libs}
    for _ in range(args.ab_reps):
        for lib in libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--ticks", str(T), "--batch", str(B), "--k", str(K), "--repeats",
                                str(args.repeats)], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, CMPC_LIB=lib))
            assert o.returncode == 0, o.stderr[-2000:]
            for ln in o.stdout.splitlines():
                w = ln.split()
                if len(w) == 3 and w[0] == "child":
                    abc[lib][0].append(float(w[1]))
                    abc[lib][1].append(float(w[2]))
    assert all(len(v[0]) == args.ab_reps for v in abc.values()), abc

import torch
import cmpc_amd as cm

cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
fmt = lambda a: ", ".join(f"{x:.4f}" for x in a)
med = lambda a: float(np.median(a))
say(f"forward mode and the checkpointed reverse under a plant mismatch: N = {cfg.N}, B = {B}, {T} ticks, k = {K}, variants alternating, median of "
    f"{args.repeats} timed regions, ms per tick (whole call / ticks); {torch.cuda.get_device_name(0)}")
com0, dcom0, h0 = start()
rng = np.random.default_rng(7)
cu = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
mm = dict(hidden_wrench=cu(np.concatenate([rng.normal(0, 0.3, (T, B, 3)), rng.normal(0, 0.05, (T, B, 3))], -1)),
          state_noise=cu(np.concatenate([rng.normal(0, 3e-3, (T, B, 3)), rng.normal(0, 1e-2, (T, B, 3)), rng.normal(0, 2e-3, (T, B, 3))], -1)),
          force_gain=cu(rng.uniform(0.9, 1.1, B)), tick_first=0)
unit = dict(hidden_wrench=torch.zeros_like(mm["hidden_wrench"]), state_noise=torch.zeros_like(mm["state_noise"]), force_gain=torch.ones_like(mm["force_gain"]),
            tick_first=0)
ds = cu(np.random.default_rng(2).normal(size=(B, K, 9)), np.float64)
dmm = dict(dir_hidden_wrench=cu(rng.normal(size=(T, B, K, 6)), np.float64), dir_state_noise=cu(0.1 * rng.normal(size=(T, B, K, 9))),
           dir_force_gain=cu(rng.normal(size=(B, K)), np.float64))
gS = cu(np.random.default_rng(1).normal(size=(T + 1, B, 9)), np.float64)
ro_p, ro_u, ro_m = (cm.rollout.WalkingRollout(cfg, B) for _ in range(3))
w_p = ro_p.walk_device_taped(T, com0, dcom0, h0)
w_u = ro_u.walk_device_taped(T, com0, dcom0, h0, mismatch=unit)
w_m = ro_m.walk_device_taped(T, com0, dcom0, h0, mismatch=mm)
ro_c = {e: cm.rollout.WalkingRollout(cfg, B) for e in (4, 8)}
ro_f = cm.rollout.WalkingRollout(cfg, B)


def checkpointed(e):
    wc = ro_c[e].walk_device_checkpointed(T, com0, dcom0, h0, e, mismatch=mm, trace=False)
    return ro_c[e].backward_device_checkpointed_mismatch(wc, gS)


def full():
    w = ro_f.walk_device_taped(T, com0, dcom0, h0, mismatch=mm, trace=False)
    return ro_f.backward_device(w, gS)


variants = (("fwd_plain", lambda: ro_p.forward_sensitivity_device(w_p, dir_state0=ds)),
            ("fwd_unit", lambda: ro_u.forward_sensitivity_device_mismatch(w_u, dir_state0=ds)),
            ("fwd_all", lambda: ro_m.forward_sensitivity_device_mismatch(w_m, dir_state0=ds, **dmm)),
            ("rev_full", full), ("rev_every4", lambda: checkpointed(4)), ("rev_every8", lambda: checkpointed(8)))
for _, fn in variants:      # warm-up (module load, allocator, the workspaces of both walks)
    fn()
ms = {k: [] for k, _ in variants}
peak, last = {}, {}
for _ in range(args.repeats):
    for k, fn in variants:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t, last[k] = timed(torch, fn)
        ms[k].append(t)
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
m = {k: med(v) for k, v in ms.items()}
same = torch.equal(last["fwd_unit"]["states"], last["fwd_plain"]["states"])
say(f"(a) forward_sensitivity_device on the plain tape {m['fwd_plain']:.4f} ({fmt(ms['fwd_plain'])}) | forward_sensitivity_device_mismatch on the unit-mismatch "
    f"tape {m['fwd_unit']:.4f} ({fmt(ms['fwd_unit'])}) | unit / plain = {m['fwd_unit'] / m['fwd_plain']:.4f}, {1e3 * (m['fwd_unit'] - m['fwd_plain']):+.1f} us per "
    f"tick: the mismatched plant instantiation's own cost | the same state directions to the bit: {same}")
say(f"(b) all three parts set, all three direction groups given {m['fwd_all']:.4f} ({fmt(ms['fwd_all'])}) | all / plain = {m['fwd_all'] / m['fwd_plain']:.4f}, "
    f"{1e3 * (m['fwd_all'] - m['fwd_plain']):+.1f} us per tick | largest |d state_T| {float(last['fwd_all']['states'][-1].abs().max()):.3e}, flagged ticks "
    f"{int((last['fwd_all']['status'] != 0).sum())}")
bits = {e: all(torch.equal(last[f"rev_every{e}"][k], last["rev_full"][k]) for k in ("state0", "hidden_wrench", "state_noise", "force_gain", "models")) for e in (4, 8)}
say(f"(c) walk_device_taped + backward_device on the full tape {m['rev_full']:.4f} ({fmt(ms['rev_full'])}), peak {peak['rev_full']:.1f} MiB | "
    f"walk_device_checkpointed + backward_device_checkpointed_mismatch, every = 4: {m['rev_every4']:.4f} ({fmt(ms['rev_every4'])}), peak {peak['rev_every4']:.1f} MiB, "
    f"/ full = {m['rev_every4'] / m['rev_full']:.4f} | every = 8: {m['rev_every8']:.4f} ({fmt(ms['rev_every8'])}), peak {peak['rev_every8']:.1f} MiB, / full = "
    f"{m['rev_every8'] / m['rev_full']:.4f} | gradients bit-equal to the full tape's: every = 4 {bits[4]}, every = 8 {bits[8]}")
if ab:
    note = lambda r: f"{r:.4f} (" + ("inside" if abs(r - 1.0) <= SPREAD else "OUTSIDE: this build " + ("slower" if r > 1.0 else "faster") + " by more than") + \
        f" the in-call spread of {100 * SPREAD:.1f} %)"
    new, old = med(ab["libcmpc_hip.so"]), med(ab[args.baseline])
    say(f"(d) headline solve (bench.py config2 through tools/ab_multi.sh, {args.ab_reps} rounds), ms per step: {args.baseline} {old:.4f} "
        f"({fmt(ab[args.baseline])}) | this build {new:.4f} ({fmt(ab['libcmpc_hip.so'])}) | this build / baseline = {note(new / old)}")
    for i, what in ((0, "walk_device()"), (1, f"forward_sensitivity_device (plain tape, k = {K})")):
        new, old = med(abc["libcmpc_hip.so"][i]), med(abc[args.baseline][i])
        say(f"(d) {what}, child processes alternating, {args.ab_reps} rounds of the median of {args.repeats}, ms per tick: {args.baseline} {old:.4f} "
            f"({fmt(abc[args.baseline][i])}) | this build {new:.4f} ({fmt(abc['libcmpc_hip.so'][i])}) | this build / baseline = {note(new / old)}")
else:
    say("(d) not run (no --baseline)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
