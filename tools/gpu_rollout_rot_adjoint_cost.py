"""Cost of carrying the orientations through the roll-out tick in reverse: one rollout_tick_vjp_device(rot=True) call (cmpc_rollout_tick_vjp_rot_device)
beside rot=False (cmpc_rollout_tick_vjp_device) at B = 256, N = 20 -- the parameters of config 2 dressed as a first tick, as
tools/gpu_rollout_adjoint_cost.py does.  Wall time on torch's stream (HIP events), the two variants alternating in one process after a warm-up of both;
median and spread of `reps` calls each, with the Python wrapper's output allocations in both.
Usage: python tools/gpu_rollout_rot_adjoint_cost.py [reps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402


def main(reps=30):
    import torch
    cfg, P, X0 = cm.synthetic.config2_perturbed_com(256)
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
    calls = {False: lambda: s.rollout_tick_vjp_device(0.0, tape, g, gl), True: lambda: s.rollout_tick_vjp_device(0.0, tape, g, gl, dGradListRotOut=gl, rot=True)}
    for _ in range(3):
        for rot in (False, True):
            r = calls[rot]()
    torch.cuda.synchronize()
    assert (r["sens"][:, 0] == 0).all()
    ts = {False: [], True: []}
    for _ in range(reps):
        for rot in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            calls[rot]()
            b.record()
            torch.cuda.synchronize()
            ts[rot].append(a.elapsed_time(b))
    m = {k: float(np.median(v)) for k, v in ts.items()}
    for k, name in ((False, "rot=False"), (True, "rot=True ")):
        print(f"config2 B={B} N={N} tick VJP {name}: median {m[k]:.3f} ms  (min {min(ts[k]):.3f}, max {max(ts[k]):.3f}, {reps} calls, alternating)")
    print(f"rot=True / rot=False = {m[True] / m[False]:.4f}  ({m[True] - m[False]:+.3f} ms per call)", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
