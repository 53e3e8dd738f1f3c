"""Cost of the cotangent-column VJP (include/cmpc.h, cmpc_solution_vjp_cols_device) beside what it replaces: k calls of the single-column entry, and the
policy Jacobian (24 unit cotangents, all parameters) beside feedback_gain_device (9 JVP columns, the state block only).  Config 2 (B = 256, N = 20) and
config 3 (B = 4096, N = 20); HIP events on torch's stream, median of `reps` after a warm-up, the variants of a comparison alternating in one process.
Usage: python tools/gpu_vjp_cols_cost.py [reps] [out]        (out: default profiles/r15_vjp_cols.txt)
       python tools/gpu_vjp_cols_cost.py --single [reps]     (the single-column cmpc_solution_vjp_device and the k = 9 JVP alone, one line per configuration: for an
                                                              A/B of two builds of the library through CMPC_LIB, as tools/ab_multi.sh does for the solve)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402

KS = (1, 8, 24, 30)


def _alternate(fns, reps):
    """median wall time [ms] of each fn: one warm-up each, then reps rounds in which the variants take turns"""
    import torch
    ts = [[] for _ in fns]
    for r in range(reps + 1):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r > 0:
                ts[i].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in ts]


def _cases():
    return [("config2", cm.synthetic.config2_perturbed_com(256)), ("config3", cm.synthetic.config3_external_push(4096))]


def _solved(cfg, P, X0):
    import torch
    s = cm.BatchSolver(cfg, P.shape[0])
    s.set_multiplier_output()
    dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
    dX, dI = s.solve_device(dP, dX0)
    lam = s.multipliers_device(dX, dP)
    torch.cuda.synchronize()
    return s, dP, dX, lam


def single(reps):
    import torch
    for name, (cfg, P, X0) in _cases():
        s, dP, dX, lam = _solved(cfg, P, X0)
        V = torch.ones((P.shape[0], cm.Layout(cfg.N).nx), dtype=torch.float32, device=dP.device)
        out, sens = s.solution_vjp_device(dX, dP, lam, V)
        t, tj = _alternate([lambda: s.solution_vjp_device(dX, dP, lam, V, out=out, sens=sens), lambda: s.feedback_gain_device(dX, dP, lam)], reps)
        print(f"{os.environ.get('CMPC_LIB', 'libcmpc_hip.so')} {name} single-column vjp {t:.3f} ms, jvp k=9 (feedback gain) {tj:.3f} ms", flush=True)


def main(reps, path):
    import torch
    lines = []
    for name, (cfg, P, X0) in _cases():
        B, L = P.shape[0], cm.Layout(cfg.N)
        s, dP, dX, lam = _solved(cfg, P, X0)
        rng = np.random.default_rng(15)
        V = torch.from_numpy(rng.standard_normal((B, max(KS), L.nx)).astype(np.float32)).cuda()
        cols_p = [V[:, j].contiguous() for j in range(max(KS))]
        one = torch.empty((B, L.np), dtype=torch.float32, device=dP.device)
        sens = torch.empty((B, cm._capi.SENS), dtype=torch.float32, device=dP.device)
        row = [f"{name} B={B} N={cfg.N}:"]
        for k in KS:
            Vk = V[:, :k].contiguous()
            out = torch.empty((B, k, L.np), dtype=torch.float32, device=dP.device)

            def singles():
                for j in range(k):
                    s.solution_vjp_device(dX, dP, lam, cols_p[j], out=one, sens=sens)
            t_cols, t_single = _alternate([lambda: s.solution_vjp_cols_device(dX, dP, lam, Vk, out_p=out, sens=sens), singles], reps)
            row.append(f"k={k} cols {t_cols:.2f} ms, {k} single calls {t_single:.2f} ms ({t_single / t_cols:.2f} x)")
            del out, Vk
        t_pj, t_pjm, t_fg = _alternate([lambda: s.policy_jacobian_device(dX, dP, lam), lambda: s.policy_jacobian_device(dX, dP, lam, model=True, rot=True),
                                        lambda: s.feedback_gain_device(dX, dP, lam)], reps)
        _, _, _, sn = s.policy_jacobian_device(dX, dP, lam)
        sn = sn.cpu().numpy()
        row.append(f"policy Jacobian [24 x {L.np}] {t_pj:.2f} ms, with the model and rotation blocks {t_pjm:.2f} ms, feedback gain [24 x 9] {t_fg:.2f} ms; "
                   f"status != 0: {int((sn[:, 0] != 0).sum())}, residual max {sn[:, 1].max():.1e}")
        lines.append(" ".join(row[:1]) + " " + "; ".join(row[1:]))
        print(lines[-1], flush=True)
        del s, V, cols_p
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(f"tools/gpu_vjp_cols_cost.py: HIP events, median of {reps} after a warm-up, variants alternating in one process\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--single":
        single(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "r15_vjp_cols.txt"))
