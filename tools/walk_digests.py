"""GPU box: a SHA-256 of every tensor that a fixed list of tiny device walks returns (WalkingRollout's public methods only), per case and per key --
the evidence that a change to the Python roll-out layer left every walk's bits alone.  The device walks are deterministic between handles of the same
batch size and factor storage, so two trees either print the same digests or compute something different.
    python tools/walk_digests.py --commit HASH --out tests/golden/walk_digests.json     (on the tree that is the reference: copy this file into it)
    python tools/walk_digests.py --check tests/golden/walk_digests.json                 (on any later tree: exit 1 and the keys that differ)
tests/test_gpu_walk_digests.py is the second form as a test.  The cases: N = 10, dt = 0.06, the ergoCubGazeboV1 weights, B = 8 and 14 ticks for the plain
walks (tests/test_gpu_walk_snapshot.py's starts, push and replan at tick 7), Q = 5 trials of 4 ticks through B = 2 slots in 12 ticks for the refill walks.
Word 6 of every info row is the solve's clock count and is left out, as tests/test_gpu_walk_snapshot.py's _same_walk leaves it out.
--set grads is a second case list on the same shapes (grad_cases: the device derivatives, the host-stepped ones, the autograd wrappers), recorded in
tests/golden/walk_grad_digests.json and held by tests/test_gpu_walk_grad_digests.py."""
import argparse, hashlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T = 8, 14
RB, Q, TT, RT = 2, 5, 4, 12


def digest(value, key="", out=None):
    """{dotted key: SHA-256 of the tensor's bytes (shape and dtype in front), or the value itself for a number, a string or None}, through dicts, lists and
    tuples; callables, ctypes structs and keys that start with "_" (keep-alives) are left out"""
    import torch
    out = {} if out is None else out
    if isinstance(value, torch.Tensor):
        a = np.ascontiguousarray(value.detach().cpu().numpy())
        if key.split(".")[-1] == "info" and a.shape[-1] == 8:      # (word 6 is the clock)
            a = np.ascontiguousarray(np.delete(a, 6, axis=-1))
        out[key] = hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()
    elif isinstance(value, np.ndarray):
        out[key] = hashlib.sha256(f"{value.dtype}{value.shape}".encode() + np.ascontiguousarray(value).tobytes()).hexdigest()
    elif isinstance(value, dict):
        for k in sorted(value, key=str):
            if not str(k).startswith("_"):
                digest(value[k], f"{key}.{k}" if key else str(k), out)
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            digest(v, f"{key}.{i}", out)
    elif value is None or isinstance(value, (bool, int, float, str)):
        out[key] = repr(value)
    return out


def cases():
    """-> {case: the walk's dict}, every walk on a roll-out of its own"""
    import torch
    import cmpc_amd as cm
    from tests.test_gpu_walk_record import _start
    from tests.test_gpu_walk_refill_plans import _plans
    from tests.test_gpu_walk_refill_trials import _trial_mismatch, _trial_models
    from tests.test_gpu_walk_snapshot import _walk_case
    from tests.test_gpu_walk_tape import _cfg
    cfg = _cfg()
    new = lambda batch=B: cm.rollout.WalkingRollout(cfg, batch)
    out = {}

    def plain(case, **more):
        com0, dcom0, h0, kw, replan = _walk_case(case)
        ro = new()
        return ro, (T, com0, dcom0, h0), dict(kw, replan=replan(ro), **more)
    ro, a, kw = plain("benign")
    out["walk"] = ro.walk_device(*a, **kw)
    for case in ("ends3", "nan"):
        ro, a, kw = plain(case, skip_ended=True)
        out[f"walk_skip_ended_{case}"] = ro.walk_device(*a, **kw)
    ro, a, kw = plain("benign")
    mm = dict(_trial_mismatch(B, 6, 5, 1, seed=3), tick_first=2)
    out["walk_taped_mismatch"] = ro.walk_device_taped(*a, mismatch=mm, **kw)
    ro, a, kw = plain("benign")
    w = out["walk_checkpointed"] = ro.walk_device_checkpointed(*a, 5, **kw)
    out["walk_resume"] = new().walk_resume_device(w["checkpoints"][5], T - 5, index=np.array([2, 2, 2, 2, 5, 5, 5, 5], np.int32), replan=kw["replan"],
                                                  taped=True)
    ro, a, kw = plain("benign")
    ro.set_limits()
    out["walk_limits"] = ro.walk_device(*a, **kw)

    com0, dcom0, h0, push = _start(Q)
    start, pushed = (RT, TT, com0, dcom0, h0), dict(push=push, push_ticks=2)
    models, hidden = _trial_models(Q), dict(hidden_wrench=_trial_mismatch(Q, 3, 2, 1, seed=4)["hidden_wrench"])
    out["refill"] = new(RB).walk_device_refill(*start, **pushed)
    out["refill_trials"] = new(RB).walk_device_refill_trials(*start, models=models, mismatch=hidden, **pushed)
    out["refill_taped"] = new(RB).walk_device_refill_taped(*start, models=models, mismatch=_trial_mismatch(Q, 3, 2, 1, seed=5), **pushed)
    out["refill_from_snapshot"] = new(RB).walk_device_refill_from_snapshot(w["checkpoints"][5], RT, TT, np.array([0, 3, 3, 7, 1], np.int32), models=models,
                                                                           mismatch=hidden, **pushed)
    plans, plan_of = _plans(cfg), np.array([0, 1, 2, 1, 0], np.int32)
    for taped in (False, True):
        ro = new(RB)
        out["refill_plans_taped" if taped else "refill_plans"] = ro.walk_device_refill_plans(
            *start, plans, plan_of, references=ro.plan_references(plans, TT), models=models, mismatch=hidden, taped=taped, **pushed)
    ro = new(RB)
    ro.set_limits()
    out["refill_limits"] = ro.walk_device_refill_trials(*start, mismatch=hidden, **pushed)
    torch.cuda.synchronize()
    for name in [k for k in out if k.startswith("refill")]:      # (the per-trial trace rows: one index_select each out of the slot-major trace)
        trials = dict(out[name]["trials"])
        trials["trace_of"] = [trials["trace"](q) for q in range(Q)]
        out[name] = dict(out[name], trials=trials)
    return out


def grad_cases():
    """-> {case: a dict of derivative outputs}: the second case list (--set grads; tests/golden/walk_grad_digests.json, tests/test_gpu_walk_grad_digests.py) --
    the device derivatives, the host-stepped ones and the autograd wrappers on the shapes above, k = 2 columns in forward mode.  Seeds and directions
    come from one numpy generator; every state seed has a NaN behind the end of problem 3, which the ends3 cases end at tick 7.  Every key agreed
    between two recordings on the parent tree: no key is left out besides word 6 of info."""
    import torch
    import cmpc_amd as cm
    from tests.test_gpu_walk_record import _start
    from tests.test_gpu_walk_refill_trials import _trial_mismatch, _trial_models
    from tests.test_gpu_walk_snapshot import _walk_case
    from tests.test_gpu_walk_tape import _cfg
    cfg, rng, K = _cfg(), np.random.default_rng(2024), 2
    dev = torch.device("cuda", 0)
    new = lambda batch=B, **kw: cm.rollout.WalkingRollout(cfg, batch, **kw)
    out = {}

    def plain(case, **more):
        com0, dcom0, h0, kw, replan = _walk_case(case)
        ro = new()
        return ro, (T, com0, dcom0, h0), dict(kw, replan=replan(ro), **more)

    def seeds(ticks, batch, nx, nan=True):
        gS, gX = rng.normal(size=(ticks + 1, batch, 9)), rng.normal(size=(ticks, batch, nx)).astype(np.float32)
        if nan:
            gS[9:, 3] = np.nan
        return gS, gX
    d = lambda *shape, dtype=np.float64: rng.normal(size=shape).astype(dtype)

    # on a taped mismatch walk that ends problem 3 at tick 7, the limits' measures traced
    ro, a, kw = plain("ends3")
    ro.set_limits()
    nx, M = ro.L.nx, ro.M
    w = ro.walk_device_taped(*a, mismatch=dict(_trial_mismatch(B, 6, 5, 1, seed=3), tick_first=2), **kw)
    gS, gX = seeds(T, B, nx)
    n_ref = w["tape"]["references"]["knots"]
    out["backward_device"] = ro.backward_device(w, gS, gX)
    out["backward_device_rot"] = ro.backward_device_rot(w, gS, gX)
    out["backward_device_refs"] = ro.backward_device_refs(w, gS, gX, rot=True)
    out["backward_device_measures"] = ro.backward_device_measures(w, d(T, B, 4), gS, gX, refs=True)
    dirs = dict(dir_state0=d(B, K, 9), dir_plan=d(B, K, 2, M, 3), dir_models=1e-3 * d(B, K, 34))
    out["forward_refs"] = ro.forward_sensitivity_device_mismatch(w, dir_ref_com=d(B, K, n_ref, 3), dir_ref_h=d(B, K, n_ref, 3), **dirs)
    out["forward_mismatch"] = ro.forward_sensitivity_device_mismatch(w, dir_hidden_wrench=d(T, B, K, 6), dir_state_noise=d(T, B, K, 9, dtype=np.float32),
                                                                    dir_force_gain=d(B, K), solutions=True, **dirs)
    # on tapes without a mismatch: the plain forward mode, the references' and the measures'
    ro, a, kw = plain("ends3")
    ro.set_limits()
    w = ro.walk_device_taped(*a, **kw)
    out["forward_device"] = ro.forward_sensitivity_device(w, dir_push=d(B, K, 3, dtype=np.float32), dir_plan_rot=d(B, K, 2, M, 3), solutions=True)
    out["forward_device_refs"] = ro.forward_sensitivity_device_refs(w, dir_ref_com=d(B, K, n_ref, 3), dir_state0=d(B, K, 9))
    out["forward_device_measures"] = ro.forward_sensitivity_device_measures(w, dir_state0=d(B, K, 9), dir_models=1e-3 * d(B, K, 34))
    # checkpointed, every = 5: the plain walk's reverse, and under a mismatch
    for name, mm in (("checkpointed", None), ("checkpointed_mismatch", dict(_trial_mismatch(B, 6, 5, 1, seed=3), tick_first=2))):
        ro, a, kw = plain("ends3")
        w = ro.walk_device_checkpointed(*a, 5, **(kw if mm is None else dict(kw, mismatch=mm)))
        back = ro.backward_device_checkpointed if mm is None else ro.backward_device_checkpointed_mismatch
        out[f"backward_{name}"] = back(w, gS, gX, rot=True)
    # sensed: a tape with delay 1 and noise, then snapshots and a resume
    ro, a, kw = plain("benign")
    kw.pop("push"), kw.pop("push_ticks")
    hidden = dict(hidden_wrench=_trial_mismatch(B, 6, 5, 1, seed=6)["hidden_wrench"], tick_first=2)
    sensor = lambda r: r.wrench_sensor(delay=1, hold_knots=2, deadband=0.1, noise=0.05 * np.random.default_rng(7).normal(size=(T, B, 6)).astype(np.float32))
    w = ro.walk_device_sensed(*a, hidden, sensor(ro), tape=True, **kw)
    gS2, gX2 = seeds(T, B, nx, nan=False)
    out["walk_sensed_taped"] = {k: v for k, v in w.items() if k != "tape"}
    out["backward_sensed"] = ro.backward_device_sensed(w, gS2, gX2)
    out["forward_sensed"] = ro.forward_sensitivity_device_sensed(w, K, dir_hidden_wrench=d(6, B, K, 6), dir_sensor_noise=d(T, B, K, 6), dir_state0=d(B, K, 9))
    ro, a, kw = plain("benign")
    kw.pop("push"), kw.pop("push_ticks")
    w = out["walk_sensed_every"] = ro.walk_device_sensed(*a, hidden, sensor(ro), every=5, **kw)
    ro2 = new()
    out["walk_resume_sensed"] = ro2.walk_resume_device_sensed(w["checkpoints"][5], T - 5, hidden, sensor(ro2), replan=kw["replan"])
    # refill: the taped walk, one regrouped view, every trial's gradient
    com0, dcom0, h0, push = _start(Q)
    ro = new(RB)
    w = ro.walk_device_refill_taped(RT, TT, com0, dcom0, h0, models=_trial_models(Q), mismatch=_trial_mismatch(Q, 3, 2, 1, seed=5), push=push, push_ticks=2)
    out["refill_trial_walk"] = ro.refill_trial_walk(w, [3, 1])
    gS3, gX3 = seeds(TT, Q, nx, nan=False)
    out["backward_refill"] = ro.backward_device_refill(w, gS3, gX3)
    # the host-stepped path, 4 ticks
    com0, dcom0, h0, push = _start(B)
    ro = new()
    tape = ro.run(4, com0, dcom0, h0, push=push, push_ticks=3, record="light", tape=True)["tape"]
    gS4, gX4 = seeds(4, B, nx, nan=False)
    out["host_backward"] = ro.backward(tape, gS4, gX4, rot=True)
    out["host_forward"] = ro.forward_sensitivity(tape, dir_state0=d(B, K, 9), dir_push=d(B, K, 3, dtype=np.float32), dir_plan_rot=d(B, K, 2, M, 3), solutions=True)

    # the autograd wrappers: outputs and every .grad of a sum of what they return, weighted by fixed numbers
    def leaves(**arrays):
        return {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in arrays.items()}

    def graded(result, inputs, weights):
        results = result if isinstance(result, tuple) else (result,)
        sum((torch.nan_to_num(r.to(torch.float64)) * torch.from_numpy(wt).to(dev)).sum() for r, wt in zip(results, weights)).backward()
        return dict(out=[r.detach() for r in results], grad={k: v.grad for k, v in inputs.items()})
    com0, dcom0, h0, kw, replan = _walk_case("ends3")
    s0, pushv = np.concatenate([com0, dcom0, h0], 1).astype(np.float32), kw["push"].astype(np.float32)
    mm = _trial_mismatch(B, 6, 5, 1, seed=3)
    wS, wM = d(T + 1, B, 9), d(T, B, 4)
    wS[9:, 3] = wM[9:, 3] = np.nan      # (cotangents behind problem 3's end: the fold sums them into its own row, the measures' are not read)
    basic = lambda: leaves(state0=s0, push=pushv, models=cm.config.model_array([cfg] * B))
    ro, inp = new(), dict(basic(), **leaves(plan_rot=0.05 * d(B, 2, M, 3)))
    out["differentiable_host"] = graded(cm.rollout_differentiable(ro, 4, push_ticks=3, **inp), inp, (wS[:5],))
    ro, inp = new(), dict(basic(), **leaves(plan_rot=0.05 * d(B, 2, M, 3), ref_com=0.01 * d(B, n_ref, 3), hidden_wrench=mm["hidden_wrench"],
                                            state_noise=mm["state_noise"], force_gain=mm["force_gain"]))
    out["differentiable_device"] = graded(cm.rollout_differentiable(ro, T, push_ticks=3, device_walk=True, replan=replan(ro), **inp), inp, (wS,))
    for name, fn in (("checkpointed", cm.rollout_differentiable_checkpointed), ("checkpointed_mismatch", cm.rollout_differentiable_checkpointed_mismatch)):
        more = leaves(hidden_wrench=mm["hidden_wrench"], force_gain=mm["force_gain"]) if name.endswith("mismatch") else {}
        ro, inp = new(), dict(basic(), **more)
        out[f"differentiable_{name}"] = graded(fn(ro, T, every=5, push_ticks=3, replan=replan(ro), **inp), inp, (wS,))
    ro, inp = new(), dict(basic(), **leaves(ref_h=0.01 * d(B, n_ref, 3), state_noise=mm["state_noise"]))
    out["differentiable_measures"] = graded(cm.rollout_differentiable_measures(ro, T, push_ticks=3, replan=replan(ro), **inp), inp, (wS, wM))
    # forward mode through the device wrapper, one tangent
    import torch.autograd.forward_ad as fwd
    ro = new()
    with fwd.dual_level():
        dual = fwd.make_dual(torch.from_numpy(s0).to(dev), torch.from_numpy(d(B, 9, dtype=np.float32)).to(dev))
        states = cm.rollout_differentiable(ro, T, dual, torch.from_numpy(pushv).to(dev), push_ticks=3, device_walk=True, replan=replan(ro))
        primal, tangent = fwd.unpack_dual(states)
        out["differentiable_device_forward_ad"] = dict(primal=primal.detach(), tangent=tangent.detach(), last_forward=ro.last_forward)
    torch.cuda.synchronize()
    return out


def compute(which="walks"):
    """-> {case: {key: digest}}"""
    return {name: digest(w) for name, w in (grad_cases() if which == "grads" else cases()).items()}


def differences(got, want):
    """the lines that say where two {case: {key: digest}} differ: keys missing, keys added, digests that differ"""
    lines = []
    for case in sorted(set(got) | set(want)):
        g, w = got.get(case), want.get(case)
        if g is None or w is None:
            lines.append(f"{case}: {'missing' if g is None else 'not in the reference'}")
            continue
        for k in sorted(set(g) | set(w)):
            if k not in g or k not in w:
                lines.append(f"{case}: {k}: {'missing' if k not in g else 'not in the reference'}")
            elif g[k] != w[k]:
                lines.append(f"{case}: {k}: differs")
    return lines


if __name__ == "__main__":
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown", help="the commit of the tree the digests are taken on (recorded in the file)")
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--check", default=None, help="compare with this file instead of writing one: exit 1 where a key differs")
    ap.add_argument("--set", default="walks", choices=("walks", "grads"), help="the case list: the walks (the default), or the derivatives and wrappers")
    args = ap.parse_args()
    doc = dict(tool="tools/walk_digests.py", commit=args.commit, rocm=torch.version.hip, torch=torch.__version__,
               device=torch.cuda.get_device_name(0), cases=compute(args.set))
    if args.set != "walks":
        doc["set"] = args.set
    if args.check:
        with open(args.check) as f:
            lines = differences(doc["cases"], json.load(f)["cases"])
        print("\n".join(lines) if lines else f"walk_digests: {sum(len(c) for c in doc['cases'].values())} keys equal to {args.check}")
        sys.exit(1 if lines else 0)
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
