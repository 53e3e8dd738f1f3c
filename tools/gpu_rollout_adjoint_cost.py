"""Cost of the roll-out tick in reverse (include/cmpc.h: cmpc_rollout_tick_vjp_device) beside the solution VJP it is built around
(cmpc_solution_vjp_model_device), and of a whole reverse sweep beside its forward roll-out: wall time on torch's stream (HIP events, median of `reps`).
One tick: the parameters of config 2 (B = 256) and config 3 (B = 4096) dressed as a first tick (two stance contacts per foot list).  Sweep: the
60-tick walking roll-out at B = 1024, taped, then WalkingRollout.backward.
Usage: python tools/gpu_rollout_adjoint_cost.py [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402
from tools.gpu_sensitivity_cost import _time  # noqa: E402


def one_tick(reps):
    import torch
    for name, (cfg, P, X0) in (("config2", cm.synthetic.config2_perturbed_com(256)), ("config3", cm.synthetic.config3_external_push(4096))):
        B, N = P.shape[0], cfg.N
        L = cm.Layout(N)
        s = cm.BatchSolver(cfg, B)
        s.set_multiplier_output()
        dev = torch.device("cuda")
        dP, dX0 = torch.from_numpy(P.astype(np.float32)).to(dev), torch.from_numpy(X0.astype(np.float32)).to(dev)
        dX, dI = s.solve_device(dP, dX0)
        lam = s.multipliers_device(dX, dP)
        M = 4
        lt = torch.zeros((B, 2, M, 2), dtype=torch.float64, device=dev)
        lt[:, :, 0, 1] = 1e9                                  # one contact per foot, active for ever
        ln = torch.ones((B, 2), dtype=torch.int32, device=dev)
        tape = dict(X=dX, P=dP, lam_g=lam, state=dP[:, L.p_com0:L.p_com0 + 9].contiguous(), info=dI, ok=None,
                    land=torch.full((B, 2), -1, dtype=torch.int32, device=dev), plan_t=None, plan_n=None, prev_t=None, prev_n=None, list_t=lt, list_n=ln,
                    step=cfg.sampling_time / 6, substeps=6, force_sample_time=False)
        g = torch.ones((B, 9), dtype=torch.float64, device=dev)
        gl = torch.zeros((B, 2, M, 3), dtype=torch.float64, device=dev)
        V = torch.ones((B, L.nx), dtype=torch.float32, device=dev)
        s.rollout_tick_vjp_device(0.0, tape, g, gl)          # (workspaces allocated)
        t_solve = _time(lambda: s.solve_device(dP, dX0, dX=dX, dInfo=dI), reps)
        t_vjp = _time(lambda: s.solution_vjp_model_device(dX, dP, lam, V), reps)
        t_tick = _time(lambda: s.rollout_tick_vjp_device(0.0, tape, g, gl), reps)
        t_plant = _time(lambda: s.plant_step_vjp_device(dX, dP, tape["state"], g), reps)
        t_list = _time(lambda: s.contacts_position_vjp_device(0.0, lt, ln, tape["land"], dGradListOut=gl, dGradP=dP, dGradX=V, phase=3), reps)
        print(f"{name} B={B} N={N}: solve {t_solve:.3f} ms, solution VJP (p + model) {t_vjp:.3f} ms, tick VJP {t_tick:.3f} ms "
              f"(glue {t_tick - t_vjp:+.3f} ms = {(t_tick - t_vjp) / t_tick * 100:.1f} % of the tick VJP); alone: plant VJP {t_plant:.3f} ms, "
              f"list VJP (both parts) {t_list:.3f} ms  [each with the Python wrapper's output allocations]", flush=True)


def sweep(reps, B=1024, ticks=60):
    import torch
    cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
    rng = np.random.default_rng(5)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0, h0 = rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3))
    push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    ro = cm.rollout.WalkingRollout(cfg, B, plan=cm.rollout.walking_plan(cfg, steps=10))
    fwd, fwd_taped, bwd = [], [], []
    gS = torch.zeros((ticks + 1, B, 9), dtype=torch.float64, device="cuda")
    gS[ticks, :, 0:3] = 1.0
    for _ in range(reps):
        rec = ro.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False)
        fwd.append(float(np.sum(rec["tick_ms"])))
        rec = ro.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False, tape=True)
        fwd_taped.append(float(np.sum(rec["tick_ms"])))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ro.backward(rec["tape"], gS)
        torch.cuda.synchronize()
        bwd.append((time.perf_counter() - t0) * 1e3)
    flagged = int((out["status"] != 0).sum())
    print(f"walking roll-out B={B} ticks={ticks}: forward {np.median(fwd):.1f} ms, forward taped {np.median(fwd_taped):.1f} ms, reverse sweep "
          f"{np.median(bwd):.1f} ms ({np.median(bwd) / np.median(fwd):.1f} x the forward); flagged (tick, problem) pairs {flagged} of {ticks * B}; "
          f"unconverged solves {int(np.sum(rec['unconverged']))}", flush=True)


if __name__ == "__main__":
    r = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    one_tick(r)
    sweep(r)
