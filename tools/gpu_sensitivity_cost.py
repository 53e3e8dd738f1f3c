"""Cost of the solution sensitivities (include/cmpc.h) beside the solve they differentiate: wall time of the kernels on torch's stream (HIP events,
median of `reps`), for the VJP and the JVP with k = 1 / 9 / 16, at config 2 (B = 256), config 3 (B = 4096) and config 5 (B = 8192, N = 30), and the
workspace bytes per problem.  Kernel-only times for the record come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
Usage: python tools/gpu_sensitivity_cost.py [reps]; python tools/gpu_sensitivity_cost.py --sweep (the accuracy sweep, see sweep())"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402


def _time(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main(reps=5):
    import torch
    cases = [("config2", cm.synthetic.config2_perturbed_com(256)), ("config3", cm.synthetic.config3_external_push(4096)),
             ("config5", cm.synthetic.config5_footstep_candidates(8192))]
    for name, (cfg, P, X0) in cases:
        B = P.shape[0]
        L = cm.Layout(cfg.N)
        s = cm.BatchSolver(cfg, B)
        s.set_multiplier_output()
        dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
        dX, dI = s.solve_device(dP, dX0)
        lam = s.multipliers_device(dX, dP)
        t_solve = _time(lambda: s.solve_device(dP, dX0, dX=dX, dInfo=dI), reps)
        V = torch.ones((B, L.nx), dtype=torch.float32, device=dP.device)
        _, sv = s.solution_vjp_device(dX, dP, lam, V)
        t_vjp = _time(lambda: s.solution_vjp_device(dX, dP, lam, V), reps)
        row = [f"{name} B={B} N={cfg.N}: solve {t_solve:.3f} ms, vjp {t_vjp:.3f} ms ({t_vjp / t_solve:.2f} x solve)"]
        for k in (1, 9, 16):
            D = torch.zeros((B, k, L.np), dtype=torch.float32, device=dP.device)
            for i in range(k):
                D[:, i, L.p_com0 + i % 9] = 1.0
            t = _time(lambda: s.solution_jvp_device(dX, dP, lam, D), reps)
            row.append(f"jvp k={k} {t:.3f} ms")
        sv = sv.cpu().numpy()
        row.append(f"workspace {s.workspace_bytes_per_problem()} B/problem; status != 0: {int((sv[:, 0] != 0).sum())}, "
                   f"problems with weakly active rows {int((sv[:, 2] > 0).sum())}, residual max {sv[:, 1].max():.1e}")
        print("; ".join(row), flush=True)


def _ref_gaps(args):
    """(kernel - sens_ref) of one problem: JVP of every column, relative to the column's largest entry; VJP relative to its largest entry"""
    name, N, X, P, lam, D, DX, V, GP = args
    from tests import sens_ref
    cfg = _cfg(name, N)
    S = sens_ref.Sens(cfg, X.astype(np.float64), P.astype(np.float64), lam.astype(np.float64))
    j = max(np.abs(DX[i] - S.jvp(D[i].astype(np.float64))).max() / max(np.abs(S.jvp(D[i].astype(np.float64))).max(), 1e-3) for i in range(D.shape[0]))
    gr = S.vjp(V.astype(np.float64))
    v = np.abs((GP - gr) * sens_ref.covered_mask(N)).max() / np.abs(gr).max()
    return j, v, S.weak


def _cfg(name, N):
    return {"config2": lambda: cm.synthetic.config2_perturbed_com(1)[0], "config3": lambda: cm.synthetic.config3_external_push(1)[0],
            "config5": lambda: cm.synthetic.config5_footstep_candidates(1)[0]}[name]()


def sweep(seeds=5, B=512, sample=3):
    """5 seeds x 512 problems per configuration: status, residual, weakly active rows (loaded / swing), the adjoint identity on the device outputs for
    every problem; the kernel against tests/sens_ref.py on `sample` problems per seed (JVP of all 13 columns, VJP)."""
    import torch
    from multiprocessing import Pool
    gens = [("config2", cm.synthetic.config2_perturbed_com, 700), ("config3", cm.synthetic.config3_external_push, 710),
            ("config5", cm.synthetic.config5_footstep_candidates, 720)]
    for name, gen, s0 in gens:
        acc = dict(status=0, resid=0.0, weak_problems=0, weak_swing_problems=0, adj=0.0, sigma=0.0)
        jobs = []
        for sd in range(s0, s0 + seeds):
            cfg, P, X0 = gen(B, seed=sd)
            L = cm.Layout(cfg.N)
            s = cm.BatchSolver(cfg, B)
            s.set_multiplier_output()
            dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
            dX, dI = s.solve_device(dP, dX0)
            lam = s.multipliers_device(dX, dP)
            rng = np.random.default_rng(sd)
            D = np.zeros((B, 13, L.np), np.float32)
            for i in range(9):
                D[:, i, L.p_com0 + i] = 1.0
            D[:, 9, L.p_comref + 3 * 5 + 2] = 1.0
            D[:, 10, L.p_href + 3 * 4 + 1] = 1.0
            D[:, 11, L.p_fext + 3 * 2] = 1.0
            from tests import sens_ref
            D[:, 12] = (rng.standard_normal((B, L.np)) * 1e-2 * sens_ref.covered_mask(cfg.N)).astype(np.float32)
            V = rng.standard_normal((B, L.nx)).astype(np.float32)
            DX, sj = s.solution_jvp_device(dX, dP, lam, torch.from_numpy(D).cuda())
            GP, sv = s.solution_vjp_device(dX, dP, lam, torch.from_numpy(V).cuda())
            torch.cuda.synchronize()
            X, Lm, I, DX, GP, sj, sv = (t.cpu().numpy() for t in (dX, lam, dI, DX, GP, sj, sv))
            ok = (I[:, 5] == 0)
            acc["status"] += int(((sj[:, 0] != 0) & ok).sum() + ((sv[:, 0] != 0) & ok).sum())
            acc["resid"] = max(acc["resid"], float(sj[ok, 1].max()), float(sv[ok, 1].max()))
            acc["weak_problems"] += int((sj[ok, 2] > 0).sum())
            acc["weak_swing_problems"] += int((sj[ok, 5] > 0).sum())
            acc["sigma"] = max(acc["sigma"], float(sj[ok, 3].max()))
            for b in np.nonzero(ok)[0]:
                lhs = float((V[b].astype(np.float64)[None] * DX[b].astype(np.float64)).sum())
                rhs = float(GP[b].astype(np.float64) @ D[b].astype(np.float64).sum(0))
                acc["adj"] = max(acc["adj"], abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-6))
            for b in np.nonzero(ok)[0][:sample]:
                jobs.append((name, cfg.N, X[b], P[b].astype(np.float32), Lm[b], D[b], DX[b], V[b], GP[b]))
            del s
        with Pool(16) as pool:
            res = pool.map(_ref_gaps, jobs)
        jv = max(r[0] for r in res)
        vv = max(r[1] for r in res)
        print(f"{name}: {seeds} seeds x {B}: nonzero sensitivity status {acc['status']}, residual max {acc['resid']:.1e}, "
              f"problems with weakly active rows of loaded feet {acc['weak_problems']}, with weak swing-foot rows {acc['weak_swing_problems']}, "
              f"largest Sigma {acc['sigma']:.1e}, adjoint identity max {acc['adj']:.1e}; kernel vs sens_ref on {len(res)} problems: "
              f"jvp {jv:.1e} vjp {vv:.1e}", flush=True)


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--sweep":
    sweep()


if __name__ == "__main__" and (len(sys.argv) < 2 or sys.argv[1] != "--sweep"):
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
