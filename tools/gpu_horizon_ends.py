"""Developer probe (GPU box): the batches of tests/test_gpu_horizon_ends.py at the library's defaults, device and CPU model side by side, against
the float64 oracle converged to 1e-9.  One run, no thresholds:  python tools/gpu_horizon_ends.py [OUT]  (default profiles/horizon_ends.txt).

Per family, horizon and storage: iterations (mean, max), problems polished, problems with status != 0, problems outside parity.limits and the worst
error per quantity; under each batch the same figures of the CPU model of the shipped algorithm (oracle/ipm_ref.c, mix=True, the defaults of
cmpc_create).  Every number quoted in tests/test_gpu_horizon_ends.py, include/cmpc.h, INTEGRATION.md and DESIGN.md about these horizons is from
this file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cmpc_amd as cm  # noqa: E402
from tests.test_gpu_horizon_ends import ALL_BATCHES, LDS_NMAX, horizon  # noqa: E402
from tests.test_horizon_ends_cpu import model_solve, oracle_solve, outside_limits  # noqa: E402

KEYS = ("com", "force0", "forces", "dcom", "h", "pos")


def line(tag, B, info, over, worst, polished_at):
    return ("%-44s its mean %5.2f max %2d polished %3d status!=0 %3d outside %3d of %3d | " % (
        tag, info[:, 0].mean(), int(info[:, 0].max()), int(((info[:, 3] % 1000000) >= polished_at).sum()), int((info[:, 5] != 0).sum()), over, B)
        + " ".join("%s %.1e" % (k, worst[k]) for k in KEYS))


def main(out_path):
    lines = ["# tools/gpu_horizon_ends.py: device (MI355X) and CPU model (ipm_ref.c, mix) at the library's defaults against the float64 oracle (1e-9).",
             "# outside = problems with a quantity at or above tests/parity.limits (1e-4 relative; h 3e-5 absolute)."]
    for family, key in ALL_BATCHES:
        cfg, P32, X032, Xr = oracle_solve(family, key)
        N, B = cfg.N, P32.shape[0]
        name = "%s N=%d%s" % (family, N, " swing %d,%d" % key[1] if isinstance(key, tuple) else "")
        for storage in (("lds", "hbm") if horizon(key) <= LDS_NMAX else ("hbm",)):
            s = cm.BatchSolver(cfg, B, factors=storage)
            X, info, rc = s.solve_host(P32, X032)
            s.close()
            over, worst = outside_limits(N, P32, X.astype(np.float64), Xr)
            lines.append(line("device %s %s" % (name, storage), B, info, over, worst, 100000))
            print(lines[-1], flush=True)
        Xm, im = model_solve(cfg, P32, X032)
        over, worst = outside_limits(N, P32, Xm.astype(np.float64), Xr)
        lines.append(line("model  %s" % name, B, im, over, worst, 100))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "horizon_ends.txt"))
