#!/usr/bin/env python
"""Benchmark of the hot path: batched centroidal-MPC solves (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

N > 1: this script starts its own N ranks (one per GPU, `python -m torch.distributed.run` as a child process,
BEFORE anything in this process touches the GPU) unless it is already running as a rank of such a launch
(RANK/WORLD_SIZE in the environment: the driver's own `torch.distributed.run ... bench.py --gpus N`).
A step = one batched solve of the workload on every GPU, inputs resident in HBM, followed for N > 1 by the
RCCL all-gather of the compact solutions.  Rank 0 prints ONE JSON line.

Workloads (BASELINE.json configs):
    config2  B=256 per GPU, perturbed-CoM standing problems, horizon 20       (the headline `value`; weak scaling)
    config3  B=4096 per GPU, swing phase + external pushes, step adjustment   (secondary; weak)
    config4  65536 Monte-Carlo problems in total (config-3 generator, seed 2), contiguous shards of 65536/N
             problems per GPU (8 x 8192 at N=8)                              (secondary; STRONG scaling)
    config5  B=8192 per GPU, yawed footstep candidates, horizon 30            (secondary; weak)
plus the single-problem (B=1) solve latency the metric names, and
    rollout  B=1024 per GPU, 60 ticks of the warm-started receding-horizon walking roll-out (the reference's operating mode:
             is_warm_start_enabled true, ergoCubGazeboV1/centroidal_mpc.ini:9; CentroidalMPCBlock.cpp:586-631 + the plant of
             WholeBodyQPBlock.cpp:1083-1150): seven launches per tick, everything resident in HBM            (secondary; weak)
    inflight two independent config-2 batches in flight on two streams (two handles): a batch is as slow as its slowest problem, and the CUs its early
             finishers release start the other batch -- what a Monte-Carlo campaign of many batches gets; NOT the headline, whose steps run one at a time
             as the ticks of a receding horizon must                                                          (secondary; N = 1 only)
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# canonical algorithmic work: F_iter(N) = 4.25e5 * N flop per interior-point iteration
F_ITER_PER_STAGE = 4.25e5
PEAK_F32_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense f32-input MFMA peak = f32 vector peak
CONFIG4_TOTAL = 65536


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="problems per GPU of the primary workload (0: its BASELINE size)")
    ap.add_argument("--workload", default="config2", choices=["config2", "config3", "config4", "config5"])
    ap.add_argument("--secondary", default="config3,config5,config4,latency,rollout,inflight",
                    help="comma list of extra workloads reported under `secondary` ('' or 'none': skip)")
    ap.add_argument("--secondary-steps", type=int, default=5)
    ap.add_argument("--cpu-sample", type=int, default=6144)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-collective", action="store_true",
                    help="run the all-gather path with one rank too (rehearsal on a single GPU)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="rehearsal only: more ranks than GPUs, ranks share the devices round-robin and the collective runs on "
                         "gloo (RCCL refuses two ranks on one device); the line is marked `rehearsal`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, rank 0 writes what the last timed step of the primary workload returned as DIR/<name>.npy "
                         "(see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def launch_ranks(args):
    """Parent of an N > 1 run that was started as plain `python bench.py --gpus N`: starts the ranks as a child
    process and exits with its code.  Nothing here initialises the GPU (device_count() does not, on this image)."""
    import torch
    ndev = torch.cuda.device_count()
    if ndev < 1:
        sys.exit("bench.py: no GPU visible (this benchmark has no CPU path)")
    if args.gpus > ndev and not args.share_gpu:
        sys.exit(f"bench.py: --gpus {args.gpus} but only {ndev} GPU(s) are visible; run on a node with {args.gpus} GPUs "
                 f"(or add --share-gpu for a functional rehearsal with the ranks sharing the device)")
    if args.share_gpu and args.gpus > 6:
        sys.exit("bench.py: --share-gpu is limited to 6 ranks per device")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "2")
    sys.exit(subprocess.call(cmd, env=env))


# ------------------------------------------------------------------------------------------------------------
def make_workload(cm, name, rank, world, batch=0):
    """-> (cfg, P32, X032, scaling, description).  Each rank builds only its own problems."""
    if name == "config2":
        B = batch or 256
        cfg, P, X0 = cm.synthetic.config2_perturbed_com(B, seed=0 + 1000 * rank)
        return cfg, P, X0, "weak", f"config2: batch={B}/GPU perturbed-CoM standing problems"
    if name == "config3":
        B = batch or 4096
        cfg, P, X0 = cm.synthetic.config3_external_push(B, seed=1 + 1000 * rank)
        return cfg, P, X0, "weak", f"config3: batch={B}/GPU swing phase + external pushes (+-50 N), step adjustment on"
    if name == "config4":
        total = batch * world if batch else CONFIG4_TOTAL
        lo, hi = cm.distributed.shard_bounds(total, world, rank)
        cfg, P, X0 = cm.synthetic.config4_monte_carlo(total, shard=(lo, hi))
        return cfg, P, X0, "strong", (f"config4: {total} Monte-Carlo disturbances (config-3 generator, seed 2), contiguous shards of "
                                      f"{hi - lo} per GPU")
    if name == "config5":
        B = batch or 8192
        cfg, P, X0 = cm.synthetic.config5_footstep_candidates(B, seed=3 + 1000 * rank)
        return cfg, P, X0, "weak", f"config5: batch={B}/GPU yawed footstep candidates, horizon 30"
    raise ValueError(name)


class Runner:
    def __init__(self, args):
        import torch
        import cmpc_amd as cm
        self.torch, self.cm, self.args = torch, cm, args
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        ndev = torch.cuda.device_count()
        if ndev < 1:
            sys.exit("bench.py: no GPU visible (this benchmark has no CPU path)")
        if self.world != args.gpus:
            sys.exit(f"bench.py: launched with WORLD_SIZE={self.world} but --gpus {args.gpus}; they must agree")
        if self.world > ndev and not args.share_gpu:
            sys.exit(f"bench.py: {self.world} ranks but {ndev} GPU(s); add --share-gpu for a rehearsal")
        self.devidx = self.local_rank % ndev
        torch.cuda.set_device(self.devidx)
        self.dev = torch.device("cuda", self.devidx)
        self.coll = self.world > 1 or args.force_collective
        self.backend = None
        if self.coll:
            import torch.distributed as dist
            self.dist = dist
            self.backend = "gloo" if (args.share_gpu and self.world > ndev) else "nccl"
            if "RANK" not in os.environ:  # --force-collective with a single, unlaunched rank
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", "29533")
                os.environ["RANK"], os.environ["WORLD_SIZE"] = "0", "1"
            if self.backend == "nccl":
                dist.init_process_group("nccl", device_id=self.dev)
            else:
                dist.init_process_group("gloo")

    def barrier(self):
        if self.coll:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def max_over_ranks(self, v):
        if self.world == 1:
            return v
        t = self.torch.tensor([v], dtype=self.torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather_floats(self, vals):
        """list of python floats per rank -> [world][len] on every rank"""
        if self.world == 1:
            return [list(vals)]
        t = self.torch.tensor(vals, dtype=self.torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        out = [self.torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        return [o.cpu().tolist() for o in out]

    def _timed(self, solver, step, gather, steps, warmup, dP, dX0, dX, dInfo):
        """warm-up steps, then the timed region; returns (elapsed seconds: max over ranks, launch durations in ms, all-gather ms or None)"""
        torch = self.torch
        for _ in range(warmup):
            step()
        # Launch duration by HIP events on the stream the kernel is launched on.  An event record is a barrier packet on the stream: four per step (the
        # library's own pair, cmpc_last_solve_ms, and a pair here) left 36 us between back-to-back launches of the 0.85 ms kernel (rocprofv3 kernel trace,
        # tools/gpu_launch_gaps.sh).  So the library's pair is switched off for the timed region (cmpc_set_timing), and without a collective between the
        # launches ONE pair brackets all of them: launch duration = that / steps (it includes the dispatch gap between launches).  With a collective
        # between the launches every launch keeps a pair of its own.
        solver.set_timing(False)
        ks = solver.launch_stream
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps if self.coll else 2)]
        self.barrier()
        t0 = time.perf_counter()
        if self.coll:
            for i in range(steps):
                ev[2 * i].record(ks)
                solver.solve_device(dP, dX0, dX, dInfo)
                ev[2 * i + 1].record(ks)
                gather()
        else:
            ev[0].record(ks)
            for i in range(steps):
                solver.solve_device(dP, dX0, dX, dInfo)
            ev[1].record(ks)
        self.barrier()
        elapsed = self.max_over_ranks(time.perf_counter() - t0)
        solver.set_timing(True)
        kern_ms = np.array([ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(steps)]) if self.coll else np.array([ev[0].elapsed_time(ev[1]) / steps])
        ag_ms = None
        if self.coll:  # packing + collective alone, for the record
            self.barrier()
            t1 = time.perf_counter()
            for _ in range(10):
                gather()
            self.barrier()
            ag_ms = self.max_over_ranks((time.perf_counter() - t1) / 10 * 1e3)
        return elapsed, kern_ms, ag_ms

    def run(self, name, steps, warmup, batch=0):
        """Times `steps` steps of one workload; returns (measurement dict on every rank, host-side problem data)."""
        torch, cm = self.torch, self.cm
        cfg, P, X0, scaling, desc = make_workload(cm, name, self.rank, self.world, batch)
        P32, X032 = P.astype(np.float32), X0.astype(np.float32)
        del P, X0
        B = P32.shape[0]
        solver = cm.BatchSolver(cfg, B, device=self.devidx)
        dP, dX0 = torch.from_numpy(P32).to(self.dev), torch.from_numpy(X032).to(self.dev)
        dX = torch.empty_like(dX0)
        dInfo = torch.empty((B, 8), dtype=torch.float32, device=self.dev)
        # N > 1: one kernel packs the compact record of every problem, one all-gather shares it (preallocated buffers)
        W = 3 * (cfg.N + 1) + 38
        counts = [int(c) for c in np.array(self.gather_floats([float(B)]))[:, 0]]
        equal = len(set(counts)) == 1
        cbuf = torch.empty((B, W), dtype=torch.float32, device=self.dev) if self.coll else None
        gbuf = torch.empty((sum(counts), W), dtype=torch.float32, device=self.dev) if self.coll else None

        def gather():
            local = solver.compact_output_device(dX, dInfo, cbuf)
            return cm.distributed.all_gather_solutions(local, self.world, out=gbuf, force=True, counts=None if equal else counts)

        def step():
            solver.solve_device(dP, dX0, dX, dInfo)
            return gather() if self.coll else None

        # everything from here to the end of the timed region is queued on the solver's launch stream (torch's current stream inside this block): the solve, the
        # packing kernel and the collective follow each other in stream order, with no cross-stream event dependency between them
        ks = solver.launch_stream       # the HIP stream the solve kernel is launched on
        ks.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(ks):
            m_ = self._timed(solver, step, gather, steps, warmup, dP, dX0, dX, dInfo)
        torch.cuda.current_stream(self.dev).wait_stream(ks)
        elapsed, kern_ms, ag_ms = m_
        info = dInfo.cpu().numpy()
        iters = info[:, 0]
        giveups = float(np.floor(info[:, 3] / 1e6).sum())    # info[3] carries 1e6 per give-up at a hand-off word of the streaming stage (include/cmpc.h)
        per_rank = self.gather_floats([float(kern_ms.mean()), float(iters.sum()), float(iters.max()), float((info[:, 5] == 0).sum()), float(B), giveups])
        pr = np.array(per_rank)
        total_B = int(pr[:, 4].sum())
        flop_per_launch = float(iters.sum()) * F_ITER_PER_STAGE * cfg.N     # this rank's launch
        achieved = flop_per_launch / (kern_ms.mean() * 1e-3) / 1e12
        m = {
            "workload": f"{desc}, ergoCubGazeboV1 parameters, horizon={cfg.N}, dt={cfg.sampling_time}, cold start, converged to 1e-6",
            "value": round(total_B * steps / elapsed, 1), "unit": "solves/s", "scaling": scaling,
            "ms_per_step": round(elapsed / steps * 1e3, 4), "steps": steps,
            "batch_per_gpu": B, "batch_total": total_B, "horizon": cfg.N,
            "iterations_mean": round(float(pr[:, 1].sum() / total_B), 2), "iterations_max": int(pr[:, 2].max()),
            "converged_fraction": round(float(pr[:, 3].sum() / total_B), 6),
            "sync_giveups": int(pr[:, 5].sum()),
            "kernel_ms_per_rank": [round(v, 4) for v in pr[:, 0].tolist()],
            "roofline": {"bound": "mfma", "achieved": round(achieved, 4), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(achieved / PEAK_F32_TFLOPS, 5), "traffic": None,
                         "kernel": "cmpc_solve_kernel", "kernel_ms_avg": round(float(kern_ms.mean()), 4),
                         "algorithmic_flop_per_launch": flop_per_launch,
                         "algorithmic_hbm_bytes_per_launch": 4 * B * (cm.Layout(cfg.N).np + 2 * cm.Layout(cfg.N).nx + 8)},
        }
        if ag_ms is not None:
            m["allgather_ms"] = round(ag_ms, 4)
        # gbuf: the all-gathered compact records of the last step (the all-gather timing loop above re-gathers the same dX, dInfo)
        data = dict(cfg=cfg, P32=P32, X032=X032, X=dX.cpu().numpy(), info=info, kern_ms=kern_ms,
                    gathered=gbuf.cpu().numpy() if self.coll else None)
        del solver, dP, dX0, dX, dInfo, cbuf, gbuf
        torch.cuda.empty_cache()
        return m, data

    def latency(self, n=64):
        """The metric's second half: solve latency of ONE problem (B=1, one workgroup), p50 over n different config-2
        problems, HIP events on the launch stream."""
        torch, cm = self.torch, self.cm
        cfg, P, X0 = cm.synthetic.config2_perturbed_com(n, seed=7)
        dP, dX0 = torch.from_numpy(P.astype(np.float32)).to(self.dev), torch.from_numpy(X0.astype(np.float32)).to(self.dev)
        solver = cm.BatchSolver(cfg, 1, device=self.devidx)
        dX = torch.empty((1, dX0.shape[1]), dtype=torch.float32, device=self.dev)
        dInfo = torch.empty((1, 8), dtype=torch.float32, device=self.dev)
        ks = solver.launch_stream
        solver.set_timing(False)        # (the event pair of this loop is the measurement; the library's own pair would sit inside it)
        torch.cuda.synchronize()
        ms, its = [], []
        with torch.cuda.stream(ks):
            for i in range(3):
                solver.solve_device(dP[i:i + 1], dX0[i:i + 1], dX, dInfo)
            torch.cuda.synchronize()
            for i in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ks)
                solver.solve_device(dP[i:i + 1], dX0[i:i + 1], dX, dInfo)
                e1.record(ks)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
                its.append(float(dInfo[0, 0].item()))
        ms = np.array(ms)
        return {"workload": f"B=1: one config-2 problem per launch, {n} different problems", "p50_ms": round(float(np.median(ms)), 4),
                "p90_ms": round(float(np.quantile(ms, 0.9)), 4), "iterations_mean": round(float(np.mean(its)), 2),
                "ms_per_iteration": round(float(ms.sum() / np.sum(its)), 4)}


    def in_flight(self, nfl=2, steps=40):
        """Independent config-2 batches, `nfl` of them in flight: one handle and one stream each, launches issued round-robin.  Same kernel, same batch as the
        headline; only the order of issue differs."""
        torch, cm = self.torch, self.cm
        cfg, P, X0 = cm.synthetic.config2_perturbed_com(256, seed=0)
        dP, dX0 = torch.from_numpy(P.astype(np.float32)).to(self.dev), torch.from_numpy(X0.astype(np.float32)).to(self.dev)
        solvers = [cm.BatchSolver(cfg, 256, device=self.devidx) for _ in range(nfl)]
        outs = [(torch.empty_like(dX0), torch.empty((256, 8), dtype=torch.float32, device=self.dev)) for _ in range(nfl)]
        raw = [s.launch_stream.cuda_stream for s in solvers]
        for s in solvers:
            s.set_timing(False)

        def run(k):
            for i in range(k):
                j = i % nfl
                solvers[j].solve_device(dP, dX0, outs[j][0], outs[j][1], stream=raw[j])
        torch.cuda.synchronize()
        run(2 * nfl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = all(bool((o[1][:, 5] == 0).all().item()) for o in outs)
        same = all(bool(torch.equal(o[0], outs[0][0])) for o in outs[1:])
        for s in solvers:
            s.close()
        return {"workload": f"config2 (B=256, horizon 20), {nfl} independent batches in flight on {nfl} streams, {steps} launches",
                "value": round(256 * steps / dt, 1), "unit": "solves/s", "ms_per_batch": round(dt / steps * 1e3, 4), "batches_in_flight": nfl,
                "all_converged": ok, "batches_bit_identical": same}

    def rollout(self, B=1024, ticks=60):
        """The reference's operating mode, timed end to end: every tick = merge the planner's footsteps with the MPC-adjusted current
        contact, sample the list, write the measured state, shift the previous solution, solve (warm), adjust the next footstep,
        integrate the plant -- seven launches, then the host reads the status word (as the reference reads advance()'s bool).
        Same discipline as run(): barrier + synchronize on both sides of the timed region, max over ranks."""
        torch, cm = self.torch, self.cm
        cfg = cm.config.ergocub_gazebo_v1(20, 0.06)
        rng = np.random.default_rng(9 + 1000 * self.rank)
        com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
        dcom0 = rng.uniform(-0.05, 0.05, (B, 3)); h0 = rng.uniform(-0.02, 0.02, (B, 3))
        push = np.zeros((B, 3)); push[:, :2] = rng.uniform(-30.0, 30.0, (B, 2)) / cm.synthetic.ROBOT_MASS
        ro = cm.rollout.WalkingRollout(cfg, B, plan=cm.rollout.walking_plan(cfg, steps=6), device=self.devidx)
        ro.run(2, com0, dcom0, h0, push=push, push_ticks=3, record="light")        # untimed warm-up
        self.barrier()
        t0 = time.perf_counter()
        rec = ro.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="light", timing=False)
        self.barrier()
        elapsed = self.max_over_ranks(time.perf_counter() - t0)
        if "aborted_tick" in rec:
            ro.solver.close()
            return {"workload": f"warm-started receding-horizon walking roll-out: batch={B}/GPU x {ticks} ticks", "failed": True,
                    "aborted_tick": int(rec["aborted_tick"]), "why": "the merge of the planner's and the MPC's contact lists failed (updateContactPhaseList returned false): "
                                                                      "the reference aborts the tick there, CentroidalMPCBlock.cpp:603-607"}
        ms = np.array(rec["tick_ms"])
        pr = np.array(self.gather_floats([float(np.sum(rec["unconverged"])), float(np.max(rec["iterations_max"])), float(np.mean(rec["iterations_mean"])),
                                          float(ms.max()), float(np.median(ms)), float(np.percentile(ms, 99))]))
        ro.solver.close()
        return {"workload": f"warm-started receding-horizon walking roll-out: batch={B}/GPU x {ticks} ticks (3.6 s, six steps, pushes +-30 N for the "
                            f"first 3 ticks), horizon 20, one call of the C ABI per warm tick (cmpc_rollout_tick_device: merge, sample, setState, shift | solve | adjust, plant as three launches), all in HBM",
                "value": round(self.world * B * ticks / elapsed, 1), "unit": "solves/s", "scaling": "weak",
                "ticks_per_s": round(ticks / elapsed, 1), "ticks": ticks, "batch_per_gpu": B,
                "tick_latency_ms": {"p50": round(float(np.median(pr[:, 4])), 3), "p99": round(float(pr[:, 5].max()), 3), "max": round(float(pr[:, 3].max()), 3),
                                    "what": "wall clock of one tick on one rank: the tick call (references from the planner trajectory inside it) and the wait for the stream"},
                "iterations_mean_per_tick": round(float(pr[:, 2].mean()), 2), "iterations_max": int(pr[:, 1].max()),
                "iterations_mean_first_ticks": [round(v, 2) for v in rec["iterations_mean"][:20]],
                "iterations_max_by_tick": rec["iterations_max"],
                "unconverged": int(pr[:, 0].sum()), "merge_ok": bool(all(rec["merge_ok"])),
                "warm_policy": "warm-started pass budget 14 iterations, then the problem starts again from the cold start inside the launch"}


DUMP_LIMIT = 64 << 20     # bytes, all files of --dump-outputs together


def dump_outputs(out_dir, data):
    """--dump-outputs: what the timed path returned in its last timed step (every step solves the same problems from the same cold
    start), float32, rank 0's problems:
        x.npy         [B, nx]      the solutions
        info.npy      [B, 7]       the info words (include/cmpc.h) without word 6, solve_cycles: a shader-clock count, not a result
        gathered.npy  [sum B, W]   collective runs only: the compact records every rank received from the all-gather
    The inputs are seeded (make_workload), so the same arguments give the same problems on every run.  Above DUMP_LIMIT in all,
    every array keeps the same seeded sample of its rows, and <name>_rows.npy (float64) holds their indices."""
    arrays = {"x": data["X"], "info": np.delete(data["info"], 6, axis=1)}
    if data.get("gathered") is not None:
        arrays["gathered"] = data["gathered"]
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT - (64 << 10):   # headroom for the .npy headers
        frac = (DUMP_LIMIT - (64 << 10)) / sum(a.nbytes + 8 * a.shape[0] for a in arrays.values())
        for name in list(arrays):
            a = arrays[name]
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], max(1, int(a.shape[0] * frac)), replace=False))
            arrays[name] = a[rows]
            arrays[f"{name}_rows"] = rows.astype(np.float64)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a))


# ---- the CPU leg: the only place the oracle (test infrastructure) is used, as baseline and as checker ------------
def cpu_baseline(cfg, P32, X032, tol, mu_min, sample):
    """oracle/ipm_ref.c (float64 port of the same algorithm) on the host cores, OpenMP over a bounded sample of the
    same workload.  This is the CPU restatement baseline, NOT IPOPT+MUMPS (absent from the image)."""
    from oracle import oracle_lib as ol, problem_nlp
    # the box's CPU share for one GPU is 16 cores; never more threads than the affinity mask allows
    cores = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    oc = problem_nlp.oracle_cfg(cfg)
    reps = int(np.ceil(sample / P32.shape[0]))
    P = np.tile(P32.astype(np.float64), (reps, 1))[:sample]
    X0 = np.tile(X032.astype(np.float64), (reps, 1))[:sample]
    ol.ref_solve_batch(oc, P[:cores], X0[:cores], ol.ipm_opts(tol=tol, mu_min=mu_min, max_iter=60), nthreads=cores)
    t = time.perf_counter()
    _, info = ol.ref_solve_batch(oc, P, X0, ol.ipm_opts(tol=tol, mu_min=mu_min, max_iter=60), nthreads=cores)
    dt = time.perf_counter() - t
    # single-thread latency of one solve (p50 over 32 problems)
    lat = []
    for b in range(min(32, P.shape[0])):
        t1 = time.perf_counter()
        ol.ref_solve_batch(oc, P[b:b + 1], X0[b:b + 1], ol.ipm_opts(tol=tol, mu_min=mu_min, max_iter=60), nthreads=1)
        lat.append((time.perf_counter() - t1) * 1e3)
    return {"value": round(sample / dt, 1), "unit": "solves/s", "cores": cores, "kind": "port",
            "label": "CPU restatement baseline (oracle/ipm_ref.c, float64 Riccati interior point, same tolerances; its final extrapolation "
                     "step is not counted in its iteration figure), not IPOPT+MUMPS",
            "p50_solve_latency_ms_1thread": round(float(np.median(lat)), 3),
            "sample": f"{sample} problems of the same workload, float64, OpenMP x{cores}, {dt:.1f} s wall, "
                      f"{int((info[:, 5] == 0).sum())}/{sample} converged, mean {info[:, 0].mean():.1f} iterations"}


def parity_sample(data, n=64):
    """Worst relative error of the GPU result on the first n problems against the float64 oracle converged to 1e-9
    (checker only; part of the CPU leg)."""
    from oracle import oracle_lib as ol, problem_nlp
    from tests import parity
    cfg = data["cfg"]
    n = min(n, data["P32"].shape[0])
    cores = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    Xr, infr = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), data["P32"][:n].astype(np.float64), data["X032"][:n].astype(np.float64),
                                  ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=cores)
    worst = {}
    for b in range(n):
        if infr[b, 5] != 0:
            continue
        for k, v in parity.errors(cfg.N, data["P32"][b], data["X"][b], Xr[b]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return {"problems": n, "oracle_converged": int((infr[:, 5] == 0).sum()),
            "worst_rel_err": {k: float(f"{v:.3g}") for k, v in worst.items()},
            "note": "com/force0/forces/dcom relative (max-norm), pos/h absolute; tolerance 1e-4 on com and forces"}


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        launch_ranks(args)      # does not return
    R = Runner(args)
    sec_names = [s for s in args.secondary.split(",") if s and s != "none" and s != args.workload]
    m, data = R.run(args.workload, args.steps, args.warmup, args.batch)
    if args.dump_outputs and R.rank == 0:
        dump_outputs(args.dump_outputs, data)
    secondary = {}
    sec_data = {}
    for s in sec_names:
        if s == "latency":
            if R.rank == 0:
                secondary["single_problem_latency"] = R.latency()
            continue
        if s == "rollout":
            secondary["rollout"] = R.rollout()
            continue
        if s == "inflight":
            if R.world == 1:
                secondary["two_batches_in_flight"] = R.in_flight()
            continue
        sm, sd = R.run(s, args.secondary_steps, 2)
        secondary[s] = sm
        if R.rank == 0 and R.world == 1 and not args.no_cpu_baseline:
            sec_data[s] = {k: (v[:64] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in sd.items()}
        del sd

    if R.rank == 0:
        # secondaries: HBM bytes per launch from the committed PMC passes of the same workload, where one exists
        for wl, sm in secondary.items():
            import glob
            fns = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_summary_{wl}.json")))
            fn = fns[-1] if fns else ""
            if isinstance(sm, dict) and "roofline" in sm and fn and R.world == 1:
                try:
                    pm = json.load(open(fn))
                    if abs(pm.get("algorithmic_bytes_per_launch", 0) - sm["roofline"]["algorithmic_hbm_bytes_per_launch"]) < 1:
                        sm["roofline"]["traffic"] = pm["hbm_bytes_per_launch"]
                        sm["roofline"]["hbm_GBps"] = round(pm["hbm_bytes_per_launch"] / (sm["roofline"]["kernel_ms_avg"] * 1e-3) / 1e9, 1)
                        sm["roofline"]["valu_active_over_wave_cycles"] = round(pm["derived"]["valu_active_over_wave_cycles"], 3)
                        sm["roofline"]["traffic_source"] = f"{os.path.relpath(fn, ROOT)} (committed rocprofv3 --pmc passes; not measured in this run)"
                        sm["roofline"]["traffic_note"] = ("HBM-factor variant: per-stage factor records, slacks and multipliers stream through L2/HBM "
                                                          "(three workgroups per CU); not re-reads of the inputs")
                except Exception:
                    pass
        traffic, tsrc = None, None   # HBM bytes per launch from the committed PMC passes (profiles/), same command
        try:
            import glob
            pm = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.json")))
            if pm and args.workload == "config2" and m["batch_per_gpu"] == 256:
                pmj = json.load(open(pm[-1]))
                traffic = pmj["hbm_bytes_per_launch"]
                tsrc = os.path.relpath(pm[-1], ROOT)
                # HBM GB/s (tiny: the state lives in LDS) and VALU busy, from the same committed counter passes
                m["roofline"]["hbm_GBps"] = round(traffic / (m["roofline"]["kernel_ms_avg"] * 1e-3) / 1e9, 2)
                m["roofline"]["valu_active_over_wave_cycles"] = round(pmj["derived"]["valu_active_over_wave_cycles"], 3)
            # north_star's "MFMA%" and the share of wave-cycles spent parked, from the committed wait-attribution passes of the same command
            pw = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_wait_config2.json")))
            if pw and args.workload == "config2" and m["batch_per_gpu"] == 256:
                pwj = json.load(open(pw[-1]))["derived"]
                m["roofline"]["mfma_busy_frac"] = round(pwj["mfma_pipe_quadcycles_over_wave_cycles"], 4)
                m["roofline"]["mfma_share_of_valu_instructions"] = round(pwj["mfma_share_of_valu_instructions"], 4)
                m["roofline"]["wait_any_frac"] = round(pwj["wait_any_share"], 3)
                m["roofline"]["counters_source"] = f"{os.path.relpath(pw[-1], ROOT)} (committed rocprofv3 --pmc passes of this command; not measured in this run)"
        except Exception:
            traffic = None
        m["roofline"]["traffic"] = traffic
        m["roofline"]["traffic_source"] = (f"{tsrc} (rocprofv3 --pmc passes of this command, committed; not measured in this run)"
                                           if tsrc else None)
        m["roofline"]["note"] = ("peak = dense f32-input MFMA = f32 vector rate, 157.3 TFLOP/s (MI355X_MICROARCH.md); the matrix pipe carries the trailing updates of the fused "
                                 "factorisation (v_mfma_f32_4x4x1, every variant) and the stage's Schur-complement product Z^T Z (v_mfma_f32_16x16x4, resident variants), the "
                                 "rest is f32/f64 VALU; what binds in practice is instruction issue of single waves (4 cycles per instruction of any kind); flop = executed IP "
                                 "iterations x 4.25e5*N (SURVEY 8d canonical count); HBM traffic is ~11 KB/solve")
        out = {
            "metric": "centroidal-MPC solves/sec (batch, horizon=20)",
            "value": m["value"], "unit": "solves/s",
            "n_gpus": R.world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": m["ms_per_step"],
            "higher_is_better": True, "scaling": m["scaling"], "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": m["workload"], "batch_per_gpu": m["batch_per_gpu"], "batch_total": m["batch_total"],
                       "horizon": m["horizon"], "precision": "f32 storage+factorisation, f64 residuals"},
            "p50_solve_latency_ms": round(float(np.median(data["kern_ms"])), 4),   # (of the whole batch's launch; without a collective: the region's mean, see run())
            "iterations_mean": m["iterations_mean"], "iterations_max": m["iterations_max"],
            "converged_fraction": m["converged_fraction"],
            "sync_giveups": m["sync_giveups"],
            "kernel_ms_per_rank": m["kernel_ms_per_rank"],
            "roofline": m["roofline"],
        }
        if R.coll:
            out["ranks"] = R.world
            out["collective_backend"] = "rccl" if R.backend == "nccl" else R.backend
            out["allgather_ms"] = m.get("allgather_ms")
        if args.share_gpu and R.backend == "gloo":
            out["rehearsal"] = f"{R.world} ranks sharing {R.torch.cuda.device_count()} GPU(s), gloo collective: functional check, not a scaling number"
        if R.world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(data["cfg"], data["P32"], data["X032"], 1e-6, 5e-8, args.cpu_sample)
            out["parity_sample"] = parity_sample(data)
            for s, sd in sec_data.items():
                secondary[s]["parity_sample"] = parity_sample(sd)
        if secondary:
            out["secondary"] = secondary
        print(json.dumps(out), flush=True)
    if R.coll:
        R.barrier()
        R.dist.destroy_process_group()


if __name__ == "__main__":
    main()
