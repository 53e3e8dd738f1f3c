"""Cost of the rotation directions (include/cmpc.h: cmpc_solution_vjp_rot_device, cmpc_solution_jvp_rot_device,
cmpc_rotation_value_gradient_device, cmpc_contacts_rotation_vjp_device) beside the model entry points on the same problems: wall time on torch's
stream (HIP events, median of `reps`) at config 2 (B = 256), config 3 (B = 4096) and config 5 (B = 8192, N = 30).  The model entry points' lines are
printed whatever the library, so the same script run on an earlier build of the library (CMPC_LIB, as tools/ab_multi.sh) gives the numbers to
compare them with.
Usage: python tools/gpu_rot_sensitivity_cost.py [reps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402
from tools.gpu_sensitivity_cost import _time  # noqa: E402

M = 34


def main(reps=3):
    import torch
    cases = [("config2", cm.synthetic.config2_perturbed_com(256)), ("config3", cm.synthetic.config3_external_push(4096)),
             ("config5", cm.synthetic.config5_footstep_candidates(8192))]
    have_rot = hasattr(cm._capi.lib(), "cmpc_solution_jvp_rot_device")
    print(f"library {os.path.basename(cm._capi.LIB_PATH)}: rotation entry points {'present' if have_rot else 'absent'}", flush=True)
    for name, (cfg, P, X0) in cases:
        B, N = P.shape[0], cfg.N
        L = cm.Layout(N)
        s = cm.BatchSolver(cfg, B)
        s.set_multiplier_output()
        dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
        dX, dI = s.solve_device(dP, dX0)
        lam = s.multipliers_device(dX, dP)
        V = torch.ones((B, L.nx), dtype=torch.float32, device=dP.device)
        gM = torch.empty((B, M), dtype=torch.float64, device=dP.device)
        gP = torch.empty((B, L.np), dtype=torch.float32, device=dP.device)
        sens = torch.empty((B, cm._capi.SENS), dtype=torch.float32, device=dP.device)
        t_vm = _time(lambda: s.solution_vjp_model_device(dX, dP, lam, V, out_model=gM, out_p=gP, sens=sens), reps)
        row = [f"{name} B={B} N={N}: vjp p + model {t_vm:.3f} ms"]
        if have_rot:
            gR = torch.empty((B, 2, N, 3), dtype=torch.float64, device=dP.device)
            t_vr = _time(lambda: s.solution_vjp_rot_device(dX, dP, lam, V, out_rot=gR, out_model=gM, out_p=gP, sens=sens), reps)
            row.append(f"vjp p + model + rot {t_vr:.3f} ms ({(t_vr - t_vm) / t_vm * 100:+.1f} %)")
        for k in (1, 8):
            Dm = torch.zeros((B, k, M), dtype=torch.float64, device=dP.device)
            for i in range(k):
                Dm[:, i, i % 10] = 1.0
            out = torch.empty((B, k, L.nx), dtype=torch.float32, device=dP.device)
            t_m = _time(lambda: s.solution_jvp_model_device(dX, dP, lam, None, Dm, out=out, sens=sens), reps)
            row.append(f"jvp k={k} model {t_m:.3f} ms")
            if have_rot:
                Om = torch.zeros((B, k, 2, N, 3), dtype=torch.float64, device=dP.device)
                for i in range(k):
                    Om[:, i, i % 2, :, 2] = 1.0       # the yaw of one whole foot per column
                t_n = _time(lambda: s.solution_jvp_rot_device(dX, dP, lam, None, Dm, None, out=out, sens=sens), reps)
                t_r = _time(lambda: s.solution_jvp_rot_device(dX, dP, lam, None, None, Om, out=out, sens=sens), reps)
                t_b = _time(lambda: s.solution_jvp_rot_device(dX, dP, lam, None, Dm, Om, out=out, sens=sens), reps)
                row.append(f"rot entry, rot NULL {t_n:.3f} ms ({(t_n - t_m) / t_m * 100:+.1f} %), rot only {t_r:.3f} ms ({(t_r - t_m) / t_m * 100:+.1f} %), "
                           f"model + rot {t_b:.3f} ms ({(t_b - t_m) / t_m * 100:+.1f} %)")
        t_vg = _time(lambda: s.model_value_gradient_device(dX, dP, lam), reps)
        row.append(f"model value gradient {t_vg:.3f} ms")
        if have_rot:
            vg = torch.empty((B, 2, N, 3), dtype=torch.float64, device=dP.device)
            t_rg = _time(lambda: s.rotation_value_gradient_device(dX, dP, lam, out=vg), reps)
            Mx = 8
            lt = torch.zeros((B, 2, Mx, 2), dtype=torch.float64, device=dP.device)
            lt[:, :, :, 0] = torch.arange(Mx, device=dP.device) * 0.5 - 0.25
            lt[:, :, :, 1] = lt[:, :, :, 0] + 0.4
            ln = torch.full((B, 2), Mx, dtype=torch.int32, device=dP.device)
            t_ls = _time(lambda: s.contacts_rotation_vjp_device(0.0, lt, ln, vg), reps)
            row.append(f"rotation value gradient {t_rg:.3f} ms, list contraction (8 entries) {t_ls:.3f} ms")
        print("; ".join(row), flush=True)
        del s


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
