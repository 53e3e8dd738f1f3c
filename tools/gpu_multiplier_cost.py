"""Cost and accuracy of the multiplier output (include/cmpc.h, cmpc_set_multiplier_output).

1. Solve time with the output on and off (configs 2 and 3, B = 4096, same handle kind, kernel time from the handle's event pair, median of 20).
2. Time of the mapping, certificate and value-gradient kernels at B = 256 and 4096 (torch events, median of 50).
3. Worst KKT residuals of (returned x, exported lam) over 5 seeds x 512 problems of configs 2, 3 and 5 and of config 3 at N = 25 (runtime-N kernel),
   float64 on the host: the numbers behind the limits of tests/test_gpu_multipliers.py.

Usage: python tools/gpu_multiplier_cost.py [--out FILE]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd as cm  # noqa: E402
from tests.test_multipliers_cpu import host_kkt  # noqa: E402


def _med_ms(fn, n):
    import torch
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# multiplier output: cost and accuracy (MI355X)")
    for gen in ("config2_perturbed_com", "config3_external_push"):
        B = 4096
        cfg, P, X0 = getattr(cm.synthetic, gen)(B, seed=7)
        dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
        res = {}
        for on in (False, True, False, True):
            s = cm.BatchSolver(cfg, B)
            s.set_multiplier_output(on)
            dX, dI = s.solve_device(dP, dX0)
            torch.cuda.synchronize()
            t = []
            for _ in range(20):
                s.solve_device(dP, dX0, dX=dX, dInfo=dI)
                torch.cuda.synchronize()
                t.append(s.last_solve_ms())
            res.setdefault(on, []).append(float(np.median(t)))
            s.close()
        off, onm = min(res[False]), min(res[True])
        say(f"solve {gen} B={B}: output off {off:.3f} ms, on {onm:.3f} ms ({100 * (onm / off - 1):+.2f} %)  [runs off {res[False]}, on {res[True]}]")
    for B in (256, 4096):
        cfg, P, X0 = cm.synthetic.config3_external_push(B, seed=8)
        s = cm.BatchSolver(cfg, B)
        s.set_multiplier_output()
        dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
        dX, dI = s.solve_device(dP, dX0)
        lam = s.multipliers_device(dX, dP)
        cert = s.kkt_certificate_device(dX, dP, lam)
        gp = s.value_gradient_device(dX, dP, lam)
        torch.cuda.synchronize()
        with torch.cuda.stream(s.launch_stream):
            tm = _med_ms(lambda: s.multipliers_device(dX, dP, out=lam), 50)
            tc = _med_ms(lambda: s.kkt_certificate_device(dX, dP, lam, out=cert), 50)
            tg = _med_ms(lambda: s.value_gradient_device(dX, dP, lam, out=gp), 50)
        say(f"kernels config3 B={B}: multipliers {tm:.3f} ms, certificate {tc:.3f} ms, value gradient {tg:.3f} ms")
        s.close()
    for gen, N in (("config2_perturbed_com", 20), ("config3_external_push", 20), ("config5_footstep_candidates", 30), ("config3_external_push", 25)):
        worst = dict(stat=0.0, feas=0.0, compl=0.0, sign=0.0)
        dev = 0.0
        for seed in range(5):
            B = 512
            cfg, P, X0 = getattr(cm.synthetic, gen)(B, N=N, seed=200 + seed)
            P32 = P.astype(np.float32)
            s = cm.BatchSolver(cfg, B)
            s.set_multiplier_output()
            dP, dX0 = torch.from_numpy(P32).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
            dX, dI = s.solve_device(dP, dX0)
            lam = s.multipliers_device(dX, dP)
            cert = s.kkt_certificate_device(dX, dP, lam)
            torch.cuda.synchronize()
            X, info, L, C = (t.cpu().numpy() for t in (dX, dI, lam, cert))
            bad = int((info[:, 5] != 0).sum())
            for b in range(B):
                if info[b, 5] != 0:
                    continue
                k = host_kkt(cfg, X[b].astype(np.float64), P32[b].astype(np.float64), L[b].astype(np.float64))
                for f in worst:
                    worst[f] = max(worst[f], k[f])
                dev = max(dev, abs(C[b, 0] - k["stat"]))
            s.close()
            say(f"  {gen} N={N} seed {200 + seed}: not converged {bad}; running worst " + " ".join(f"{f} {v:.2e}" for f, v in worst.items()))
        say(f"KKT worst {gen} N={N} (5 x 512): " + " ".join(f"{f} {v:.2e}" for f, v in worst.items()) + f"; device-host stationarity {dev:.2e}")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
