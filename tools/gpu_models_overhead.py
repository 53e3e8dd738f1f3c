"""Developer tool (GPU box): what per-problem models cost the solve.  Config 3 (B = 4096, N = 20) solved K times on a handle without a model table,
then K times with a table set (cmpc_set_models) whose every row is the handle's own model -- the same records, so the same iterations and the same
bits; only the prologue reads problem b's record instead of the shared one.  Run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/gpu_models_overhead.py
and compare the cmpc_solve_kernel durations of the two halves (the script prints its own event-timed means too, alternating A and B)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(K=20, rounds=3):
    import torch

    import cmpc_amd as cm
    cfg, P, X0 = cm.synthetic.config3_external_push(4096)
    B = P.shape[0]
    dP, dX0 = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda()
    plain = cm.BatchSolver(cfg, B)
    table = cm.BatchSolver(cfg, B)
    table.set_models([cfg] * B)
    out = {}
    for name, s in (("unset", plain), ("set", table)):
        out[name] = s.solve_device(dP, dX0)
    torch.cuda.synchronize()
    same = torch.equal(out["unset"][0], out["set"][0]) and torch.equal(out["unset"][1][:, :6], out["set"][1][:, :6])
    ms = {"unset": [], "set": []}
    for _ in range(rounds):
        for name, s in (("unset", plain), ("set", table)):
            for _ in range(K):
                s.solve_device(dP, dX0, dX=out[name][0], dInfo=out[name][1])
                torch.cuda.synchronize()
                ms[name].append(s.last_solve_ms())
    for name in ms:
        a = np.asarray(ms[name])
        print(f"{name:6s} solve ms: median {np.median(a):.4f} mean {a.mean():.4f} min {a.min():.4f} (n = {a.size})")
    print(f"set / unset (medians): {np.median(ms['set']) / np.median(ms['unset']):.5f}; outputs bit-identical: {same}")


if __name__ == "__main__":
    main()
