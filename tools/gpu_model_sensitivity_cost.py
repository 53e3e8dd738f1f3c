"""Cost of the model directions (include/cmpc.h: cmpc_solution_vjp_model_device, cmpc_solution_jvp_model_device, cmpc_model_value_gradient_device)
beside the solve and the p-only VJP: wall time on torch's stream (HIP events, median of `reps`) at config 2 (B = 256), config 3 (B = 4096) and
config 5 (B = 8192, N = 30).
Usage: python tools/gpu_model_sensitivity_cost.py [reps]; python tools/gpu_model_sensitivity_cost.py --sweep (the accuracy sweep, see sweep())"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402
from tools.gpu_sensitivity_cost import _cfg, _time  # noqa: E402

M = 34


def _dirs(cfg, B, L, rng):
    """[B, 14, 34] model directions (sens_model_ref.model_directions and a random one), [B, 14, n_p] p directions (only the last column)"""
    from tests import sens_model_ref as smr, sens_ref
    dm = np.zeros((B, 14, M))
    dm[:, :13] = np.stack([d for _, d in smr.model_directions(cfg)])
    dm[:, 13] = rng.standard_normal((B, M)) * 1e-2
    dp = np.zeros((B, 14, L.np), np.float32)
    dp[:, 13] = (rng.standard_normal((B, L.np)) * 1e-2 * sens_ref.covered_mask(cfg.N)).astype(np.float32)
    return dm, dp


def main(reps=3):
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
        t_vjp = _time(lambda: s.solution_vjp_device(dX, dP, lam, V), reps)
        t_vjpm = _time(lambda: s.solution_vjp_model_device(dX, dP, lam, V), reps)
        row = [f"{name} B={B} N={cfg.N}: solve {t_solve:.3f} ms, vjp p only {t_vjp:.3f} ms, vjp p + model {t_vjpm:.3f} ms "
               f"({(t_vjpm - t_vjp) / t_vjp * 100:+.1f} %)"]
        for k in (1, 13):
            Dm = torch.zeros((B, k, M), dtype=torch.float64, device=dP.device)
            for i in range(k):
                Dm[:, i, i % 10] = 1.0
            Dp = torch.zeros((B, k, L.np), dtype=torch.float32, device=dP.device)
            t_p = _time(lambda: s.solution_jvp_device(dX, dP, lam, Dp), reps)
            t_m = _time(lambda: s.solution_jvp_model_device(dX, dP, lam, None, Dm), reps)
            row.append(f"jvp k={k} p only {t_p:.3f} ms, model {t_m:.3f} ms ({(t_m - t_p) / t_p * 100:+.1f} %)")
        t_vg = _time(lambda: s.model_value_gradient_device(dX, dP, lam), reps)
        t_vp = _time(lambda: s.value_gradient_device(dX, dP, lam), reps)
        row.append(f"model value gradient {t_vg:.3f} ms (dV*/dp {t_vp:.3f} ms)")
        print("; ".join(row), flush=True)


def _ref_gaps(args):
    """(kernel - sens_model_ref) of one problem: JVP of every column relative to its largest entry, VJP per field group, dSens[6] relative"""
    name, N, X, P, lam, dm, dp, DX, V, GM, rj_k, rv_k = args
    from tests import sens_model_ref as smr
    cfg = _cfg(name, N)
    th = cm.config.model_row(cfg).astype(np.float32).astype(np.float64)
    MS = smr.ModelSens(cfg, X.astype(np.float64), P.astype(np.float64), lam.astype(np.float64), theta=th)
    j = 0.0
    for i in range(dm.shape[0]):
        r = MS.jvp(dm[i], dp[i].astype(np.float64) if i == dm.shape[0] - 1 else None)
        j = max(j, np.abs(DX[i] - r).max() / max(np.abs(r).max(), 1e-3))
    gr = MS.vjp(V.astype(np.float64))
    groups = {"friction": [0], "weights": list(range(1, 10)), "corners_left": list(range(10, 22)), "corners_right": list(range(22, 34))}
    g = {k: float(np.abs(GM[ix] - gr[ix]).max() / max(np.abs(gr[ix]).max(), 1e-12)) for k, ix in groups.items()}
    rj = max(MS.removed(dm[i]) for i in range(dm.shape[0]))
    rv = MS.removed_vjp()
    rel = max(abs(float(rj_k) - rj) / max(rj, 1e-6), abs(float(rv_k) - rv) / max(rv, 1e-6))
    return j, g, rel


def sweep(seeds=5, B=512, sample=3):
    """5 seeds x 512 problems per configuration: status, residual, dSens[6], the adjoint identity on the device outputs for every problem; the
    kernel against tests/sens_model_ref.py on `sample` problems per seed (JVP of the 14 columns, VJP per field group, dSens[6])."""
    import torch
    from multiprocessing import Pool
    gens = [("config2", cm.synthetic.config2_perturbed_com, 800), ("config3", cm.synthetic.config3_external_push, 810),
            ("config5", cm.synthetic.config5_footstep_candidates, 820)]
    for name, gen, s0 in gens:
        acc = dict(status=0, resid=0.0, adj=0.0, rel_jvp=0.0, rel_vjp=0.0)
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
            dm, dp = _dirs(cfg, B, L, rng)
            V = rng.standard_normal((B, L.nx)).astype(np.float32)
            DX, sj = s.solution_jvp_model_device(dX, dP, lam, torch.from_numpy(dp).cuda(), torch.from_numpy(dm).cuda())
            GM, _, sv = s.solution_vjp_model_device(dX, dP, lam, torch.from_numpy(V).cuda(), grad_p=False)
            torch.cuda.synchronize()
            X, Lm, I, DX, GM, sj, sv = (t.cpu().numpy() for t in (dX, lam, dI, DX, GM, sj, sv))
            ok = (I[:, 5] == 0)
            acc["status"] += int(((sj[:, 0] != 0) & ok).sum() + ((sv[:, 0] != 0) & ok).sum())
            acc["resid"] = max(acc["resid"], float(sj[ok, 1].max()), float(sv[ok, 1].max()))
            acc["rel_jvp"] = max(acc["rel_jvp"], float(sj[ok, 6].max()))
            acc["rel_vjp"] = max(acc["rel_vjp"], float(sv[ok, 6].max()))
            for b in np.nonzero(ok)[0]:
                lhs = sum(float(V[b].astype(np.float64) @ DX[b, j].astype(np.float64)) for j in range(13))
                rhs = float(GM[b] @ dm[b, :13].sum(0))
                acc["adj"] = max(acc["adj"], abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-6))
            for b in np.nonzero(ok)[0][:sample]:
                jobs.append((name, cfg.N, X[b], P[b].astype(np.float32), Lm[b], dm[b], dp[b], DX[b], V[b], GM[b], sj[b, 6], sv[b, 6]))
            del s
        with Pool(16) as pool:
            res = pool.map(_ref_gaps, jobs)
        jv = max(r[0] for r in res)
        gv = {k: max(r[1][k] for r in res) for k in res[0][1]}
        rel = max(r[2] for r in res)
        print(f"{name}: {seeds} seeds x {B}: nonzero status {acc['status']}, residual max {acc['resid']:.1e}, adjoint identity max {acc['adj']:.1e}, "
              f"dSens[6] max jvp {acc['rel_jvp']:.1e} vjp {acc['rel_vjp']:.1e}; kernel vs sens_model_ref on {len(res)} problems: jvp {jv:.1e}, vjp "
              + " ".join(f"{k} {v:.1e}" for k, v in gv.items()) + f", dSens[6] {rel:.1e}", flush=True)


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--sweep":
    sweep()


if __name__ == "__main__" and (len(sys.argv) < 2 or sys.argv[1] != "--sweep"):
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
