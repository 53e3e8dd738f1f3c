"""GPU box: a SHA-256 of every tensor that a fixed list of tiny device walks returns (WalkingRollout's public methods only), per case and per key --
the evidence that a change to the Python roll-out layer left every walk's bits alone.  The device walks are deterministic between handles of the same
batch size and factor storage, so two trees either print the same digests or compute something different.
    python tools/walk_digests.py --commit HASH --out tests/golden/walk_digests.json     (on the tree that is the reference: copy this file into it)
    python tools/walk_digests.py --check tests/golden/walk_digests.json                 (on any later tree: exit 1 and the keys that differ)
tests/test_gpu_walk_digests.py is the second form as a test.  The cases: N = 10, dt = 0.06, the ergoCubGazeboV1 weights, B = 8 and 14 ticks for the plain
walks (tests/test_gpu_walk_snapshot.py's starts, push and replan at tick 7), Q = 5 trials of 4 ticks through B = 2 slots in 12 ticks for the refill walks.
Word 6 of every info row is the solve's clock count and is left out, as tests/test_gpu_walk_snapshot.py's _same_walk leaves it out."""
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


def compute():
    """-> {case: {key: digest}}"""
    return {name: digest(w) for name, w in cases().items()}


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
    args = ap.parse_args()
    doc = dict(tool="tools/walk_digests.py", commit=args.commit, rocm=torch.version.hip, torch=torch.__version__,
               device=torch.cuda.get_device_name(0), cases=compute())
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
