"""Cost of the roll-out tick forwards (include/cmpc.h: cmpc_rollout_tick_jvp_device) beside the solution JVP it is built around
(cmpc_solution_jvp_rot_device at the same k, fed with the tick's own assembled directions) and beside the tick VJP, and of a whole forward sweep
(WalkingRollout.forward_sensitivity) beside the reverse sweep: wall time on torch's stream (HIP events, median of `reps`).
One tick: tick 8 (a swing tick) of the taped walking roll-out at B = 256, k = 1, 8, 16, every direction group given.  Sweep: the 60-tick walking roll-out
at B = 1024, taped, forward_sensitivity at k = 8 and backward(rot=True).
Usage: python tools/gpu_rollout_jvp_cost.py [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402
from tools.gpu_sensitivity_cost import _time  # noqa: E402


def _walk(B, ticks):
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    rng = np.random.default_rng(5)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0, h0 = rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3))
    push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    ro = cm.rollout.WalkingRollout(cfg, B, plan=cm.rollout.walking_plan(cfg, steps=10))
    return cfg, ro, (ticks, com0, dcom0, h0), dict(push=push, push_ticks=3, record="light", timing=False)


def _directions(cfg, B, k, M, seed=1):
    import torch
    L, N = cm.Layout(cfg.N), cfg.N
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda shape, dt, scale=1.0: torch.randn(shape, generator=g, device="cuda", dtype=dt) * scale
    f32, f64 = torch.float32, torch.float64
    return dict(dDirState=rnd((B, k, 9), f64), dDirPrevList=rnd((B, k, 2, M, 3), f64, 0.1), dDirPrevListRot=rnd((B, k, 2, M, 3), f64, 0.1),
                dDirPlan=rnd((B, k, 2, M, 3), f64, 0.1), dDirPlanRot=rnd((B, k, 2, M, 3), f64, 0.1), dDirWrench=rnd((B, k, N, 6), f32),
                dDirModel=rnd((B, k, 34), f64, 1e-3), dDirP=rnd((B, k, L.np), f32, 0.1))


def one_tick(reps, B=256, tick=8):
    import torch
    cfg, ro, args, kw = _walk(B, tick + 1)
    rec = ro.run(*args, tape=True, **kw)
    tk = rec["tape"]["ticks"][tick]
    s = ro.solver
    M = tk["list_t"].shape[2]
    g = torch.ones((B, 9), dtype=torch.float64, device="cuda")
    gl = torch.zeros((B, 2, M, 3), dtype=torch.float64, device="cuda")
    s.rollout_tick_vjp_device(tk["now"], tk, g, gl, rot=True, dGradListRotOut=gl)          # (workspaces allocated)
    t_vjp = _time(lambda: s.rollout_tick_vjp_device(tk["now"], tk, g, gl, rot=True, dGradListRotOut=gl), reps)
    t_solve_vjp = _time(lambda: s.solution_vjp_rot_device(tk["X"], tk["P"], tk["lam_g"], tk["X"]), reps)
    print(f"walking tick {tick} B={B} N={cfg.N}: tick VJP (rot) {t_vjp:.3f} ms, bare solution VJP (rot) {t_solve_vjp:.3f} ms", flush=True)
    for k in (1, 8, 16):
        d = _directions(cfg, B, k, M)
        r = s.rollout_tick_jvp_device(tk["now"], tk, k, rot=True, p_full=True, **d)      # (the workspace grown to k)
        flagged = int((r["sens"][:, 0] != 0).sum())
        t_tick = _time(lambda: s.rollout_tick_jvp_device(tk["now"], tk, k, **d), reps)
        t_bare = _time(lambda: s.solution_jvp_rot_device(tk["X"], tk["P"], tk["lam_g"], dDirP=r["p"], dDirModel=d["dDirModel"], dDirRot=r["rot"]), reps)
        print(f"  k={k:2d}: tick JVP {t_tick:.3f} ms, bare solution JVP (rot) {t_bare:.3f} ms: glue {t_tick - t_bare:+.3f} ms = "
              f"{(t_tick - t_bare) / t_bare * 100:.1f} % of the bare solution JVP;  tick JVP / tick VJP {t_tick / t_vjp:.2f};  flagged {flagged} of {B}  "
              "[each with the Python wrapper's output allocations]", flush=True)


def sweep(reps, B=1024, ticks=60, k=8):
    import torch
    cfg, ro, args, kw = _walk(B, ticks)
    rec = ro.run(*args, tape=True, **kw)
    tape = rec["tape"]
    M = tape["ticks"][0]["list_t"].shape[2]
    d = _directions(cfg, B, k, M)
    dirs = dict(dir_state0=d["dDirState"], dir_list0=d["dDirPrevList"], dir_list_rot0=d["dDirPrevListRot"], dir_plan=d["dDirPlan"], dir_plan_rot=d["dDirPlanRot"],
                dir_models=d["dDirModel"], dir_push=torch.ones((B, k, 3), dtype=torch.float32, device="cuda"))
    gS = torch.zeros((ticks + 1, B, 9), dtype=torch.float64, device="cuda")
    gS[ticks, :, 0:3] = 1.0
    fwd, bwd, jvp = [], [], []
    for _ in range(reps):
        fwd.append(float(np.sum(ro.run(*args, **kw)["tick_ms"])))
        for fn, acc in ((lambda: ro.backward(tape, gS, rot=True), bwd), (lambda: ro.forward_sensitivity(tape, **dirs), jvp)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    flagged = int((out["status"] != 0).sum())
    print(f"walking roll-out B={B} ticks={ticks}: forward {np.median(fwd):.1f} ms, reverse sweep (rot) {np.median(bwd):.1f} ms "
          f"({np.median(bwd) / np.median(fwd):.1f} x the forward), forward sweep k={k} {np.median(jvp):.1f} ms ({np.median(jvp) / np.median(fwd):.1f} x the forward, "
          f"{np.median(jvp) / np.median(bwd):.2f} x one reverse sweep, {np.median(jvp) / k / np.median(bwd):.3f} x per column); flagged (tick, problem) pairs "
          f"{flagged} of {ticks * B}; unconverged solves {int(np.sum(rec['unconverged']))}", flush=True)


if __name__ == "__main__":
    r = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    one_tick(r)
    sweep(r)
