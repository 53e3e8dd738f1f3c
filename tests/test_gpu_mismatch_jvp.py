"""GPU: the plant-model mismatch FORWARDS and the checkpointed reverse under a mismatch (include/cmpc.h, "the mismatch FORWARDS"; DESIGN.md 7f, "Mismatch,
forwards").  The plant kernel's mismatched instantiation against the float64 restatement tests/mismatch_jvp_ref.py and, by the adjoint identity, against
cmpc_plant_step_vjp_mismatch_device; the tick against the restated tick at the contact changes of the 18-tick scene of tests/test_gpu_mismatch_long.py; the
walk against the ticks chained by hand and against its own segments, to the bit; the forward walk against backward_device by the adjoint identity over all
18 rows, all groups at once and each mismatch group alone; the plain forward walk on the same tape, which must NOT satisfy it; an ending in single support;
off against the entries that existed; the checkpointed reverse against the full tape, to the bit; no host read.
N = 10, dt = 0.06, the ergoCubGazeboV1 weights.  Every tolerance is one the project already states: F64, ADJ, REF of tests/test_gpu_rollout_adjoint.py."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import mismatch_jvp_ref as mj
from tests import rollout_adjoint_ref as rar
from tests import sens_rot_ref as srr
from tests.test_gpu_mismatch import NEW, _cu, _h, _host_tape, _rows, _tick_tape
from tests.test_gpu_mismatch_long import B, N, T, _cfg, _mm18
from tests.test_gpu_rollout_adjoint import ADJ, F64, REF, ULP32, _plant_inputs, _rel
from tests.test_gpu_rollout_jvp import _tick_directions
from tests.test_gpu_walk_record import _start
from tests.test_gpu_walk_rot_tape import ROT
from tests.test_gpu_walk_tape import GRADS, _same_bits

pytestmark = pytest.mark.gpu

KEYS = ("states", "list", "list_rot", "X", "status", "removed")
WALK_ADJ = T * ADJ      # tests/test_gpu_walk_jvp.py holds five chained ticks to 5 x ADJ; here 18 are chained


# ---- 1. the plant kernel ----
def test_plant_kernel_matches_the_restatement_and_is_the_transpose_of_the_vjp_kernel():
    """cmpc_plant_step_jvp_mismatch_cols_device at B = 33, k = 9 (297 lanes: a second workgroup; k past the solve's chunk of eight), per-problem models, one
    foot of every third problem gated off (the others in double support), gains in [0.9, 1.1] and one gain = 0, hidden rows given and NULL: against
    mismatch_jvp_ref.plant_jvp within F64 (double arithmetic on the same float32 inputs); against cmpc_plant_step_vjp_mismatch_device by <g, J d> =
    <J^T g, d>, within F64 of the summed magnitudes plus one float32 rounding of the two float32 outputs' terms; column j is a k = 1 call to the bit; all
    four new pointers NULL is cmpc_plant_step_jvp_cols_device to the bit."""
    import torch
    cfg = _cfg()
    L, nb, k, step, nsub = cm.Layout(N), 33, 9, 0.01, 6
    X, P, state, models = _plant_inputs(cfg, nb, 12)
    rng = np.random.default_rng(14)
    gain = rng.uniform(0.9, 1.1, nb).astype(np.float32)
    gain[4] = 0.0
    hidden = np.concatenate([rng.normal(0, 0.5, (nb, 3)), rng.normal(0, 0.1, (nb, 3))], 1).astype(np.float32)
    d = dict(state=rng.normal(size=(nb, k, 9)), x=rng.normal(size=(nb, k, L.nx)).astype(np.float32), p=rng.normal(size=(nb, k, L.np)).astype(np.float32),
             model=rng.normal(size=(nb, k, 34)), rot0=rng.normal(size=(nb, k, 2, 3)), hidden=rng.normal(size=(nb, k, 6)), gain=rng.normal(size=(nb, k)))
    g = rng.normal(size=(nb, 9))
    s = cm.BatchSolver(cfg, nb)
    s.set_models(models)
    dX, dP, dS = _cu(X), _cu(P), _cu(state)
    dd = {name: _cu(a) for name, a in d.items()}
    call = lambda sel=slice(None), **kw: s.plant_step_jvp_mismatch_cols_device(
        dX, dP, dS, dd["state"][:, sel].contiguous(), dd["x"][:, sel].contiguous(), dd["p"][:, sel].contiguous(), dd["model"][:, sel].contiguous(),
        dd["rot0"][:, sel].contiguous(), step=step, substeps=nsub, **kw)
    mm = lambda sel=slice(None), hid=True: dict(hidden_wrench=_cu(hidden) if hid else None, force_gain=_cu(gain), dDirHidden=dd["hidden"][:, sel].contiguous(),
                                                dDirGain=dd["gain"][:, sel].contiguous())
    out = call(**mm())
    out_nohid = call(**mm(hid=False))
    v = s.plant_step_vjp_mismatch_device(dX, dP, dS, _cu(g), step=step, substeps=nsub, hidden_wrench=_cu(hidden), force_gain=_cu(gain), grad_rot=True)
    cols = [call(slice(j, j + 1), **mm(slice(j, j + 1))) for j in range(k)]
    null = call()
    plain = s.plant_step_jvp_cols_device(dX, dP, dS, dd["state"], dd["x"], dd["p"], dd["model"], dd["rot0"], step=step, substeps=nsub)
    torch.cuda.synchronize()
    got, got_nohid = _h(out), _h(out_nohid)
    v = {name: _h(a).astype(np.float64) for name, a in v.items()}
    grav = float(np.float32(rar.GRAVITY))
    worst = dict(jvp=0.0, jvp_no_hidden=0.0, adjoint=0.0)
    for b in range(nb):
        corners = models[b, 10:].astype(np.float32).astype(np.float64)
        args = (L, corners, X[b], P[b], state[b], float(np.float32(step)), nsub)
        for j in range(k):
            dirs = (d["state"][b, j], d["x"][b, j], d["p"][b, j], d["model"][b, j], d["rot0"][b, j])
            ref = mj.plant_jvp(*args, *dirs, hidden[b], float(gain[b]), d["hidden"][b, j], d["gain"][b, j], gravity=grav)
            worst["jvp"] = max(worst["jvp"], _rel(got[b, j], ref))
            ref = mj.plant_jvp(*args, *dirs, None, float(gain[b]), d["hidden"][b, j], d["gain"][b, j], gravity=grav)
            worst["jvp_no_hidden"] = max(worst["jvp_no_hidden"], _rel(got_nohid[b, j], ref))
            lhs = g[b] @ got[b, j]
            f32_terms = [v["x"][b] * d["x"][b, j], v["p"][b] * d["p"][b, j]]
            f64_terms = [v["state"][b] * d["state"][b, j], v["model"][b] * d["model"][b, j], v["rot0"][b] * d["rot0"][b, j], v["hidden"][b] * d["hidden"][b, j],
                         np.array([v["gain"][b] * d["gain"][b, j]])]
            rhs = sum(float(t.sum()) for t in f32_terms + f64_terms)
            mag32 = sum(float(np.abs(t).sum()) for t in f32_terms)
            tol = F64 * (mag32 + sum(float(np.abs(t).sum()) for t in f64_terms) + float(np.abs(g[b] * got[b, j]).sum())) + ULP32 * mag32
            worst["adjoint"] = max(worst["adjoint"], abs(lhs - rhs) / tol)
            assert abs(lhs - rhs) <= tol, (b, j, lhs, rhs, tol)
    print(f"\nmismatched plant JVP kernel, B = {nb}, k = {k}: against the restatement {worst['jvp']:.2e}, hidden NULL {worst['jvp_no_hidden']:.2e} (bound {F64:.0e}); "
          f"adjoint identity against the VJP kernel, worst |lhs - rhs| / (F64 glue + one float32 rounding) = {worst['adjoint']:.2f} (bound 1)")
    assert worst["jvp"] <= F64 and worst["jvp_no_hidden"] <= F64
    assert not np.array_equal(got, got_nohid) and np.abs(v["hidden"]).max() > 0 and np.abs(v["gain"]).max() > 0
    gated = [b for b in range(nb) if (P[b, [L.p_gam[0], L.p_gam[1]]] < 0.5).any()]
    assert len(gated) == nb // 3 and gain[4] == 0.0 and 4 not in gated      # a foot off, double support and gain = 0 are among the problems
    for j in range(k):
        _same_bits(cols[j][:, 0], out[:, j], f"column {j} against a k = 1 call")
    _same_bits(null, plain, "all four pointers NULL against cmpc_plant_step_jvp_cols_device")
    assert not np.array_equal(_h(null), got)


# ---- the 18-tick scene ----
@pytest.fixture(scope="module")
def walk18():
    """tests/test_gpu_mismatch_long.py's scene: 18 ticks under _mm18(), taped -- lift-off at tick 6, touchdown with step adjustment at 14, second lift at
    16 -- with its reverse under random seeds, and the direction columns the tests share"""
    import torch
    cfg = _cfg()
    start = _start(B)[:3]
    mm = _mm18()
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(T, *start, mismatch=mm)
    rng = np.random.default_rng(41)
    gS, gX = rng.normal(size=(T + 1, B, 9)), (1e-2 * rng.normal(size=(T, B, ro.L.nx))).astype(np.float32)
    got = ro.backward_device(w, gS, gX)
    torch.cuda.synchronize()
    assert (_h(w["end_tick"]) == -1).all()
    land = _h(w["land"])
    assert land[4, 0, 0] == N and land[13, 0, 0] == 1, land[:, 0, 0]
    return dict(cfg=cfg, start=start, mm=mm, ro=ro, w=w, gS=gS, gX=gX, got=got)


def _walk_dirs(cfg, M, k, seed, rot=False):
    """k random columns of the direction groups of forward_sensitivity_device_mismatch, as its keyword arguments"""
    rng = np.random.default_rng(seed)
    t = _tick_directions(rng, cfg, B, k, M)
    d = dict(dir_state0=t["state"], dir_list0=t["list"], dir_plan=t["plan"], dir_push=rng.normal(size=(B, k, 3)).astype(np.float32), dir_models=t["model"],
             dir_wrench=rng.normal(size=(T, B, k, N, 6)).astype(np.float32),
             dir_hidden_wrench=rng.normal(size=(T, B, k, 6)), dir_state_noise=(0.1 * rng.normal(size=(T, B, k, 9))).astype(np.float32),
             dir_force_gain=rng.normal(size=(B, k)))
    if rot:
        d.update(dir_list_rot0=t["list_rot"], dir_plan_rot=t["plan_rot"])
    return d


# ---- 2. the tick ----
def test_tick_jvp_at_the_contact_changes(walk18):
    """cmpc_rollout_tick_jvp_mismatch_device on ticks 6 (lift-off), 14 (touchdown and adjustment), 16 (the second lift, outside the noise schedule) and 17
    (outside both) against mismatch_jvp_ref.tick_jvp fed with the tape's own float32 (x, p, lam_g), problems 0 and 5, k = 4: column 0 every group at once,
    column 1 only dDirNoise, column 2 only dDirHidden, column 3 only dDirGain; every output group of every column within REF, relative to the group's
    largest entry.  With nothing of a mismatch given the entry is cmpc_rollout_tick_jvp_device to the bit."""
    import torch
    cfg, mm, tape, s = walk18["cfg"], walk18["mm"], walk18["w"]["tape"], walk18["ro"].solver
    M, k = tape["list_t"].shape[3], 4
    rng = np.random.default_rng(43)
    gain = _cu(mm["force_gain"])
    names = ("all", "noise", "hidden", "gain")
    worst = {n_: 0.0 for n_ in names}
    for i in (6, 14, 16, 17):
        tk, hid, now = _tick_tape(tape, i), _rows(mm, i), i * cfg.sampling_time
        d = _tick_directions(rng, cfg, B, k, M)
        base = {g: d[g].copy() for g in ("state", "list", "plan", "wrench", "model")}
        for g in base:
            base[g][:, 1:] = 0
        dm = dict(hidden=rng.normal(size=(B, k, 6)), noise=(0.1 * rng.normal(size=(B, k, 9))).astype(np.float32), gain=rng.normal(size=(B, k)))
        for g, cols in (("hidden", (0, 2)), ("noise", (0, 1)), ("gain", (0, 3))):
            keep = np.zeros(k, bool)
            keep[list(cols)] = True
            dm[g][:, ~keep] = 0
        r = s.rollout_tick_jvp_mismatch_device(now, tk, k, hidden_wrench=None if hid is None else _cu(hid), force_gain=gain, dDirHidden=_cu(dm["hidden"]),
                                               dDirNoise=_cu(dm["noise"]), dDirGain=_cu(dm["gain"]), dDirState=_cu(base["state"]),
                                               dDirPrevList=_cu(base["list"]), dDirPlan=_cu(base["plan"]), dDirWrench=_cu(base["wrench"]),
                                               dDirModel=_cu(base["model"]), x=True, p_full=True)
        torch.cuda.synchronize()
        assert (_h(r["sens"])[:, 0] == 0).all(), _h(r["sens"])[:, 0]
        got = {g: _h(r[g]) for g in ("state", "list", "x", "p")}
        for b in (0, 5):
            tp = _host_tape(tk, b, None if hid is None else hid[b], float(mm["force_gain"][b]))
            RS = srr.RotSens(cfg, tp["X"], tp["P"], tp["lam_g"])
            for j, name in enumerate(names):
                ref = mj.tick_jvp(cfg, tp, now, base["state"][b, j], base["list"][b, j], None, base["plan"][b, j], None, base["wrench"][b, j], base["model"][b, j],
                                  None, dm["hidden"][b, j], dm["noise"][b, j], dm["gain"][b, j], RS=RS)
                assert ref["status"] == 0
                gaps = {g: _rel(got[g][b, j], ref[g]) for g in got if np.abs(ref[g]).max() > 0}
                for g in got:
                    if g not in gaps:      # a group this direction does not reach: exact zeros on both sides
                        assert not got[g][b, j].any(), (i, b, name, g)
                print(f"tick {i} problem {b} direction {name}: " + " ".join(f"{g} {v_:.1e}" for g, v_ in gaps.items()))
                worst[name] = max(worst[name], max(gaps.values()))
                assert np.abs(got["state"][b, j]).max() > 0, (i, b, name)
                if name in ("hidden", "gain"):      # the plant's alone: nothing of them reaches the solve
                    assert not got["x"][b, j].any() and not got["p"][b, j].any()
                if name == "noise":                 # the solve's alone: it sits on the com0 / dcom0 / h0 rows of the p direction, one float32 add to zero
                    L = cm.Layout(N)
                    np.testing.assert_array_equal(got["p"][b, j, L.p_com0:L.p_com0 + 9], dm["noise"][b, j])
    print("mismatch tick JVP at the contact changes, worst per direction group: " + " ".join(f"{n_} {v_:.2e}" for n_, v_ in worst.items()) + f" (bound {REF:.0e})")
    assert max(worst.values()) <= REF, worst
    # nothing of a mismatch: the entry that existed, bit for bit
    tk = _tick_tape(tape, 14)
    dirs = dict(dDirState=_cu(d["state"]), dDirPrevList=_cu(d["list"]), dDirPrevListRot=_cu(d["list_rot"]), dDirPlan=_cu(d["plan"]), dDirPlanRot=_cu(d["plan_rot"]),
                dDirWrench=_cu(d["wrench"]), dDirModel=_cu(d["model"]), dDirP=_cu(d["p"]), x=True, rot=True, p_full=True)
    old = s.rollout_tick_jvp_device(14 * cfg.sampling_time, tk, k, **dirs)
    new = s.rollout_tick_jvp_mismatch_device(14 * cfg.sampling_time, tk, k, **dirs)
    torch.cuda.synchronize()
    for g in old:
        _same_bits(new[g], old[g], f"nothing of a mismatch: {g}")


# ---- 3. walk = ticks ----
def _walk_call(ro, w, d, k, segments, mismatch=True):
    """cmpc_rollout_walk_jvp_mismatch_device (mismatch=False: cmpc_rollout_walk_jvp_device) over the given (tick0, ticks) segments of w's tape on shared
    arrays, as forward_sensitivity_device_mismatch lays them out -> dict of KEYS"""
    import torch
    tape, s, M, dev = w["tape"], ro.solver, ro.M, ro.dev
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    opt = lambda name: None if d.get(name) is None else _cu(d[name])
    out = dict(states=z((T + 1, B, k, 9)), status=z((T, B), torch.int32), removed=z((T, B), torch.float32), X=z((T, B, k, ro.L.nx), torch.float32))
    out["states"][0] = _cu(d["dir_state0"])
    rot = d.get("dir_list_rot0") is not None
    out["list"] = _cu(d["dir_list0"]).clone() if d.get("dir_list0") is not None else z((B, k, 2, M, 3))
    out["list_rot"] = _cu(d["dir_list_rot0"]).clone() if rot else None
    walk, kw = s.rollout_walk_jvp_device, {}
    if mismatch:
        walk = s.rollout_walk_jvp_mismatch_device
        kw = dict(mismatch=tape.get("mismatch"), dir_hidden=opt("dir_hidden_wrench"), dir_noise=opt("dir_state_noise"), dir_gain=opt("dir_force_gain"))
    with torch.cuda.stream(s.launch_stream):
        for t0, n in segments:
            walk(t0, n, tape, t0, w["end_tick"], k, out["states"], out["list"], out["status"], carry_list_rot=out["list_rot"], dir_plan=opt("dir_plan"),
                 dir_plan_rot=opt("dir_plan_rot"), dir_wrench=opt("dir_wrench"), dir_model=opt("dir_models"), dir_x=out["X"], removed=out["removed"], **kw)
    torch.cuda.synchronize()
    if not rot:
        out["list_rot"] = z((B, k, 2, M, 3))
    return out


def test_walk_is_the_ticks_and_its_segments(walk18):
    """one call of cmpc_rollout_walk_jvp_mismatch_device over the 18 rows (k = 2, every group, orientations carried) against
    cmpc_rollout_tick_jvp_mismatch_device chained by hand, row by row with that tick's hidden row and the tape row's directions; against the segments
    0 .. 6 + 7 .. 15 + 16 .. 17 (two odd lengths: the carry copy out of the workspace); and against forward_sensitivity_device_mismatch: to the bit"""
    import torch
    cfg, mm, ro, w = walk18["cfg"], walk18["mm"], walk18["ro"], walk18["w"]
    tape, s, k = w["tape"], ro.solver, 2
    d = _walk_dirs(cfg, ro.M, k, 44, rot=True)
    d.pop("dir_push")
    one = _walk_call(ro, w, d, k, [(0, T)])
    three = _walk_call(ro, w, d, k, [(0, 7), (7, 9), (16, 2)])
    for key in KEYS:
        _same_bits(three[key], one[key], f"three segments against one call: {key}")
    api = ro.forward_sensitivity_device_mismatch(w, solutions=True, **d)
    torch.cuda.synchronize()
    for key in KEYS:
        _same_bits(api[key], one[key], f"forward_sensitivity_device_mismatch against the call: {key}")
    # by hand (nothing ended: every gate step between two ticks is the identity selection)
    gain = _cu(mm["force_gain"])
    ds, dl, dlr = _cu(d["dir_state0"]), _cu(d["dir_list0"]), _cu(d["dir_list_rot0"])
    hand = dict(states=[ds], X=[], status=[])
    with torch.cuda.stream(s.launch_stream):
        for i in range(T):
            hid = _rows(mm, i)
            r = s.rollout_tick_jvp_mismatch_device(i * cfg.sampling_time, _tick_tape(tape, i), k, hidden_wrench=None if hid is None else _cu(hid), force_gain=gain,
                                                   dDirHidden=_cu(d["dir_hidden_wrench"][i]), dDirNoise=_cu(d["dir_state_noise"][i]),
                                                   dDirGain=_cu(d["dir_force_gain"]), dDirState=ds, dDirPrevList=dl, dDirPrevListRot=dlr,
                                                   dDirPlan=_cu(d["dir_plan"]), dDirPlanRot=_cu(d["dir_plan_rot"]), dDirWrench=_cu(d["dir_wrench"][i]),
                                                   dDirModel=_cu(d["dir_models"]), x=True)
            ds, dl, dlr = r["state"], r["list"], r["list_rot"]
            hand["states"].append(ds)
            hand["X"].append(r["x"])
            hand["status"].append(r["sens"][:, 0].to(torch.int32))
    torch.cuda.synchronize()
    _same_bits(torch.stack(hand["states"]), one["states"], "ticks by hand: states")
    _same_bits(torch.stack(hand["X"]), one["X"], "ticks by hand: X")
    _same_bits(torch.stack(hand["status"]), one["status"], "ticks by hand: status")
    _same_bits(dl, one["list"], "ticks by hand: list")
    _same_bits(dlr, one["list_rot"], "ticks by hand: list_rot")
    assert (_h(one["status"]) == 0).all() and np.isfinite(_h(one["states"])).all() and np.abs(_h(one["states"])[-1]).max() > 0


# ---- 4. / 5. the adjoint identity over the whole walk ----
def _identity_gaps(v, f, pairs):
    """per problem and column: sum over all rows of <gS, dS> + <gX, dX> against the contraction of the reverse walk's keys with their directions
    -> (the worst relative gap, the smallest |right-hand side|, the per-(problem, column) gaps)"""
    gS, gX, r = v["gS"], v["gX"], v["got"]
    fs, fx = _h(f["states"]), _h(f["X"]).astype(np.float64)
    rh = {name: _h(r[name]).astype(np.float64) for name, _, _ in pairs}
    k = fs.shape[2]
    gaps, smallest = np.zeros((B, k)), np.inf
    for b in range(B):
        for j in range(k):
            lhs = float((gS[:, b] * fs[:, b, j]).sum() + (gX[:, b].astype(np.float64) * fx[:, b, j]).sum())
            terms = {name: float((rh[name][:, b] * dd[:, b, j]).sum()) if rows else float((rh[name][b] * dd[b, j]).sum()) for name, dd, rows in pairs}
            rhs = sum(terms.values())
            gaps[b, j] = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)
            smallest = min(smallest, abs(rhs))
            print(f"problem {b} column {j}: forward {lhs:.9e}  reverse {rhs:.9e}  gap {gaps[b, j]:.2e}  terms " + " ".join(f"{n_} {t:.1e}" for n_, t in terms.items()))
    return float(gaps.max()), smallest, gaps


def test_forward_and_reverse_are_adjoint_on_the_device_under_the_mismatch(walk18):
    """forward_sensitivity_device_mismatch (k = 2, solutions) against backward_device on the same 18-tick mismatch tape, random grad_states / grad_X: per
    problem and column the sum over all rows of <gS, dS> + <gX, dX> equals the contraction of state0, list0, plan, push, models AND hidden_wrench,
    state_noise, force_gain with their directions, relative gap <= 18 x ADJ (18 chained ticks; tests/test_gpu_walk_jvp.py: 5 x ADJ for five).  Three more
    runs with the directions of one mismatch group alone, so that a missing term cannot hide behind the others: each right-hand side non-zero."""
    import torch
    v = walk18
    cfg, ro, w = v["cfg"], v["ro"], v["w"]
    d = _walk_dirs(cfg, ro.M, 2, 45)
    d.pop("dir_wrench")
    f = ro.forward_sensitivity_device_mismatch(w, solutions=True, **d)
    torch.cuda.synchronize()
    assert (_h(f["status"]) == 0).all() and (_h(v["got"]["status"]) == 0).all()
    new = (("hidden_wrench", d["dir_hidden_wrench"], True), ("state_noise", d["dir_state_noise"].astype(np.float64), True),
           ("force_gain", d["dir_force_gain"], False))
    pairs = (("state0", d["dir_state0"], False), ("list0", d["dir_list0"], False), ("plan", d["dir_plan"], False),
             ("push", d["dir_push"].astype(np.float64), False), ("models", d["dir_models"], False)) + new
    worst, _, _ = _identity_gaps(v, f, pairs)
    print(f"forward walk against reverse walk under the mismatch over {T} ticks, all groups, worst gap over {B} problems x 2 columns: {worst:.2e} "
          f"(bound {WALK_ADJ:.1e})")
    assert worst <= WALK_ADJ
    for pair, arg in zip(new, ("dir_hidden_wrench", "dir_state_noise", "dir_force_gain")):
        f1 = ro.forward_sensitivity_device_mismatch(w, solutions=True, **{arg: d[arg]})
        torch.cuda.synchronize()
        one, smallest, _ = _identity_gaps(v, f1, (pair,))
        print(f"... {pair[0]} alone: worst gap {one:.2e} (bound {WALK_ADJ:.1e}), smallest |right-hand side| {smallest:.2e}")
        assert one <= WALK_ADJ and smallest > 0
        worst = max(worst, one)
    print(f"worst gap of the four runs: {worst:.2e}")


def test_the_refusal_was_right(walk18):
    """the plain cmpc_rollout_walk_jvp_device on the mismatch tape, a state0 direction alone: its partials are the plant's at the MPC's forces and wrench, and
    the identity with backward_device fails -- the worst gap exceeds the bound the mismatched entry meets on the same directions"""
    v = walk18
    cfg, ro, w = v["cfg"], v["ro"], v["w"]
    d = dict(dir_state0=_walk_dirs(cfg, ro.M, 2, 46)["dir_state0"])
    pairs = (("state0", d["dir_state0"], False),)
    right, _, _ = _identity_gaps(v, _walk_call(ro, w, d, 2, [(0, T)]), pairs)
    wrong, _, gaps = _identity_gaps(v, _walk_call(ro, w, d, 2, [(0, T)], mismatch=False), pairs)
    print(f"state0 direction alone: the mismatched forward walk {right:.2e}, the plain forward walk on the same tape {wrong:.2e} (bound {WALK_ADJ:.1e}); "
          f"{int((gaps > WALK_ADJ).sum())} of {gaps.size} (problem, column) pairs of the plain walk miss it")
    assert right <= WALK_ADJ < wrong


# ---- 6. an ending ----
@pytest.mark.parametrize("skip_ended", [False, True])
def test_an_ending_in_single_support(walk18, skip_ended):
    """NaN in problem 3's hidden row of tick 8 (the left foot in the air) ends it alone; its rows 8 .. of the hidden-wrench and noise directions are NaN.
    The seven others are bit-equal to the walk without the NaN; problem 3's state rows 0 .. 8 and solution rows 0 .. 7 are the 8-tick walk's, everything
    behind is exactly zero with status 6, and nothing is non-finite.  The gain's direction is [B, k] without a row axis, so in ONE call NaN there would reach
    ticks 0 .. 7 as well; it is held through the tick entry chained by hand over the same tape, which hands the directions over tick by tick: problem 3's
    gain direction is NaN from tick 8 on (with the hidden and noise rows), its dOk word is the gate's 0 from there on, and every state and solution row
    equals the one call's to the bit -- the plant kernel's ok branch reads no direction of an ended problem."""
    import torch
    cfg, mm, ref_w, ro_ref = walk18["cfg"], walk18["mm"], walk18["w"], walk18["ro"]
    bad = dict(mm, hidden_wrench=mm["hidden_wrench"].copy())
    bad["hidden_wrench"][8 - mm["tick_first"], 3, 1] = np.nan
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(T, *walk18["start"], mismatch=bad, skip_ended=skip_ended)
    ro8 = cm.rollout.WalkingRollout(cfg, B)
    eight = ro8.walk_device_taped(8, *walk18["start"], mismatch=mm, skip_ended=skip_ended)
    d = _walk_dirs(cfg, ro.M, 2, 47)
    d.pop("dir_wrench"); d.pop("dir_push")
    d_nan = dict(d, dir_hidden_wrench=d["dir_hidden_wrench"].copy(), dir_state_noise=d["dir_state_noise"].copy())
    d_nan["dir_hidden_wrench"][8:, 3] = np.nan
    d_nan["dir_state_noise"][8:, 3] = np.nan
    d8 = dict(d, dir_hidden_wrench=d["dir_hidden_wrench"][:8], dir_state_noise=d["dir_state_noise"][:8])
    f = ro.forward_sensitivity_device_mismatch(w, solutions=True, **d_nan)
    want = ro_ref.forward_sensitivity_device_mismatch(ref_w, solutions=True, **d)
    short = ro8.forward_sensitivity_device_mismatch(eight, solutions=True, **d8)
    torch.cuda.synchronize()
    assert _h(w["end_tick"]).tolist() == [-1, -1, -1, 8, -1, -1, -1, -1] and int(w["end_code"][3]) == 5 and (_h(eight["end_tick"]) == -1).all()
    f, want, short = ({key: _h(r[key]) for key in KEYS} for r in (f, want, short))
    others = [0, 1, 2, 4, 5, 6, 7]
    for key in KEYS:
        assert np.isfinite(f[key]).all(), key
        ax = 0 if key in ("list", "list_rot") else 1
        _same_bits(np.take(f[key], others, axis=ax), np.take(want[key], others, axis=ax), f"the others: {key}")
    _same_bits(f["states"][:9, 3], short["states"][:, 3], "problem 3: states 0 .. 8")
    _same_bits(f["X"][:8, 3], short["X"][:, 3], "problem 3: solutions 0 .. 7")
    assert not f["states"][9:, 3].any() and not f["X"][8:, 3].any() and not f["list"][3].any() and not f["list_rot"][3].any()
    assert f["status"][:, 3].tolist() == [0] * 8 + [6] * 10 and not f["removed"][8:, 3].any()
    assert np.abs(f["states"][8, 3]).max() > 0
    # the gain direction too: the tick entry chained by hand, all three mismatch directions of problem 3 NaN from tick 8 on
    tape, s, k = w["tape"], ro.solver, 2
    gain = _cu(mm["force_gain"])
    dg_nan = d["dir_force_gain"].copy()
    dg_nan[3] = np.nan
    ds, dl = _cu(d["dir_state0"]), _cu(d["dir_list0"])
    hand = dict(states=[ds], X=[])
    with torch.cuda.stream(s.launch_stream):
        for i in range(T):
            tk, hid = _tick_tape(tape, i), _rows(bad, i)
            if i >= 8:      # (what the gate's PRE part feeds the tick for a problem that ended at tick 8)
                tk["ok"] = tk["ok"].clone()
                tk["ok"][3] = 0
            r = s.rollout_tick_jvp_mismatch_device(i * cfg.sampling_time, tk, k, hidden_wrench=None if hid is None else _cu(hid), force_gain=gain,
                                                   dDirHidden=_cu(d_nan["dir_hidden_wrench"][i]), dDirNoise=_cu(d_nan["dir_state_noise"][i]),
                                                   dDirGain=_cu(dg_nan if i >= 8 else d["dir_force_gain"]), dDirState=ds, dDirPrevList=dl,
                                                   dDirPlan=_cu(d["dir_plan"]), dDirModel=_cu(d["dir_models"]), x=True)
            ds, dl = r["state"], r["list"]
            hand["states"].append(ds)
            hand["X"].append(r["x"])
    torch.cuda.synchronize()
    _same_bits(torch.stack(hand["states"]), f["states"], "ticks by hand, the gain direction NaN behind the end: states")
    _same_bits(torch.stack(hand["X"]), f["X"], "ticks by hand, the gain direction NaN behind the end: X")
    _same_bits(dl, f["list"], "ticks by hand, the gain direction NaN behind the end: list")


# ---- 7. off is off ----
def test_off_is_off(walk18):
    """a tape without a mismatch: every key of forward_sensitivity_device_mismatch without the three directions is forward_sensitivity_device's and
    forward_sensitivity_device_refs', to the bit"""
    import torch
    cfg = walk18["cfg"]
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(8, *walk18["start"])
    d = {key: a[:8] if key == "dir_wrench" else a for key, a in _walk_dirs(cfg, ro.M, 2, 48, rot=True).items()
         if key not in ("dir_hidden_wrench", "dir_state_noise", "dir_force_gain", "dir_push")}
    n_ref = w["tape"]["references"]["knots"]
    drc = np.random.default_rng(49).normal(size=(B, 2, n_ref, 3)) * 0.01
    old = ro.forward_sensitivity_device(w, solutions=True, **d)
    new = ro.forward_sensitivity_device_mismatch(w, solutions=True, **d)
    old_refs = ro.forward_sensitivity_device_refs(w, dir_ref_com=drc, solutions=True, **d)
    new_refs = ro.forward_sensitivity_device_mismatch(w, dir_ref_com=drc, solutions=True, **d)
    torch.cuda.synchronize()
    assert "mismatch" not in w["tape"] and set(new) == set(old)
    for key in KEYS:
        _same_bits(new[key], old[key], f"off: {key}")
        _same_bits(new_refs[key], old_refs[key], f"off, with reference directions: {key}")
    assert not np.array_equal(_h(old["states"]), _h(old_refs["states"]))


# ---- 7b. argument errors on a live handle ----
def test_c_entries_refuse_bad_arguments_on_a_live_handle(walk18):
    """k < 1 in each of the three entries, and tick0 < 0, a schedule without rows and a negative count in the walk, on a live handle with real, large enough
    arrays: CMPC_ERR_ARG with the entry's own name and its reason in cmpc_last_error, and not one output word written (tests/test_mismatch_jvp_cpu.py can
    only reach the handle check)"""
    import ctypes as C
    import torch
    ro, w = walk18["ro"], walk18["w"]
    s, tape, M = ro.solver, w["tape"], ro.M
    lib, h, L = s._lib, s._h, ro.L
    z = lambda shape, dt=torch.float64: torch.full(shape, 7, dtype=dt, device=ro.dev)
    states, carry, status = z((T + 1, B, 1, 9)), z((B, 1, 2, M, 3)), z((T, B), torch.int32)
    dh, dn, dg = z((T, B, 1, 6)), z((T, B, 1, 9), torch.float32), z((B, 1))
    wd = cm._capi.CmpcWalkDirs(states.data_ptr(), carry.data_ptr(), None, None, None, None, None, None, None, status.data_ptr(), None)
    md = cm._capi.CmpcWalkDirsMismatch(dh.data_ptr(), dn.data_ptr(), dg.data_ptr())
    good = tape["mismatch"]["_c"]
    hid = tape["mismatch"]["hidden_wrench"].data_ptr()
    walk = lambda tick0, k, m: lib.cmpc_rollout_walk_jvp_mismatch_device(h, M, tick0, T, tape["_c"], 0, None, k, C.byref(wd), C.byref(m), C.byref(md), None)
    name = "cmpc_rollout_walk_jvp_mismatch_device"
    for k in (0, -1):
        assert walk(0, k, good) == -1 and name in s.last_error and "k >= 1" in s.last_error, s.last_error
    assert walk(-1, 1, good) == -1 and name in s.last_error and "bad argument" in s.last_error, s.last_error
    for m in (cm._capi.CmpcPlantMismatch(0, hid, 0, None, 0, None), cm._capi.CmpcPlantMismatch(0, hid, -2, None, 0, None)):
        assert walk(0, 1, m) == -1 and name in s.last_error and "bad mismatch" in s.last_error, s.last_error
    # the tick and the plant: k < 1
    tk = _tick_tape(tape, 3)
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    ct = cm._capi.CmpcTickTape(tk["X"].data_ptr(), tk["P"].data_ptr(), tk["lam_g"].data_ptr(), tk["state"].data_ptr(), tk["info"].data_ptr(), tk["ok"].data_ptr(),
                               tk["land"].data_ptr(), tk["plan_t"].data_ptr(), tk["plan_n"].data_ptr(), tk["prev_t"].data_ptr(), tk["prev_n"].data_ptr(),
                               tk["list_t"].data_ptr(), tk["list_n"].data_ptr(), float(tk["step"]), int(tk["substeps"]), 1 if tk["force_sample_time"] else 0)
    out_state, out_list, sens = z((B, 1, 9)), z((B, 1, 2, M, 3)), z((B, cm._capi.SENS), f32)
    dout = cm._capi.CmpcTickDirsOut(out_state.data_ptr(), out_list.data_ptr(), None, None, None, None)
    tmd = cm._capi.CmpcTickDirsMismatch(dh[3].data_ptr(), dn[3].data_ptr(), dg.data_ptr())
    for k in (0, -1):
        assert lib.cmpc_rollout_tick_jvp_mismatch_device(h, M, 0.18, C.byref(ct), k, None, C.byref(dout), sens.data_ptr(), None, None, C.byref(tmd), None) == -1
        assert "cmpc_rollout_tick_jvp_mismatch_device" in s.last_error and "null argument" in s.last_error, s.last_error
        assert lib.cmpc_plant_step_jvp_mismatch_cols_device(h, tk["X"].data_ptr(), tk["P"].data_ptr(), tk["state"].data_ptr(), 0.01, 6, k, states[0].data_ptr(),
                                                            None, None, None, None, None, None, dh[3].data_ptr(), dg.data_ptr(), out_state.data_ptr(), None) == -1
        assert "cmpc_plant_step_jvp_mismatch_cols_device" in s.last_error and "bad argument" in s.last_error, s.last_error
    torch.cuda.synchronize()
    for a in (states, carry, status, out_state, out_list, sens):      # nothing was queued: every output still holds its fill
        assert bool((a == 7).all())


# ---- 8. the checkpointed reverse ----
@pytest.mark.parametrize("case", ["plain", "ending", "rot"])
@pytest.mark.parametrize("every", [4, 7])
def test_checkpointed_reverse_is_the_full_tape_reverse(walk18, every, case):
    """backward_device_checkpointed_mismatch on walk_device_checkpointed(18, every, mismatch=_mm18()) -- every = 4: segments 4, 4, 4, 4, 2; every = 7:
    segments 7, 7, 4 -- against backward_device on the full tape: every key to the bit, force_gain, which the segments add to last first, among them, and
    tape_rows_peak == every + 1.  Again with problem 3 ended at tick 8 by a NaN push (NaN seeds behind its end), and with rot=True against
    backward_device_rot."""
    import torch
    cfg, mm, gS, gX = walk18["cfg"], walk18["mm"], walk18["gS"], walk18["gX"]
    if case == "ending":
        mm = dict(mm, hidden_wrench=mm["hidden_wrench"].copy())
        mm["hidden_wrench"][8 - mm["tick_first"], 3, 1] = np.nan
        gS = gS.copy()
        gS[9:, 3] = np.nan
    if case == "plain":
        full, want = walk18["w"], walk18["got"]
    else:
        ro_f = cm.rollout.WalkingRollout(cfg, B)
        full = ro_f.walk_device_taped(T, *walk18["start"], mismatch=mm)
        want = ro_f.backward_device_rot(full, gS, gX) if case == "rot" else ro_f.backward_device(full, gS, gX)
    ro = cm.rollout.WalkingRollout(cfg, B)
    wc = ro.walk_device_checkpointed(T, *walk18["start"], every, mismatch=mm)
    got = ro.backward_device_checkpointed_mismatch(wc, gS, gX, rot=case == "rot")
    torch.cuda.synchronize()
    assert sorted(wc["checkpoints"]) == list(range(every, T, every)) and got["tape_rows_peak"] == every + 1
    assert _h(wc["end_tick"]).tolist() == _h(full["end_tick"]).tolist() == ([-1, -1, -1, 8, -1, -1, -1, -1] if case == "ending" else [-1] * B)
    keys = GRADS + NEW + (ROT if case == "rot" else ())
    assert set(keys) <= set(got) and set(got) - {"tape_rows_peak"} == set(want)
    for key in keys:
        assert np.isfinite(_h(got[key])).all(), key
        _same_bits(got[key], want[key], f"every = {every}, {case}: {key}")
    for key in NEW:
        assert np.abs(_h(got[key])).max() > 0, key
    if case == "ending":
        assert not _h(got["hidden_wrench"])[8:, 3].any() and _h(got["status"])[:, 3].tolist() == [0] * 8 + [6] * 10
    with pytest.raises(NotImplementedError):      # the pinned refusal stays
        ro.backward_device_checkpointed(wc, gS)


def test_autograd_through_the_checkpointed_mismatch():
    """rollout_differentiable_checkpointed_mismatch against rollout_differentiable(device_walk=True, hidden_wrench=, state_noise=, force_gain=): the states
    and the .grad of state0, hidden_wrench, state_noise and force_gain, to the bit"""
    import torch
    from tests.test_gpu_mismatch import _mismatch
    cfg = _cfg()
    nb, ticks = 4, 6
    com0, dcom0, h0, _ = _start(nb, seed=3)
    s0 = np.concatenate([com0, dcom0, h0], 1).astype(np.float32)
    mm = _mismatch(nb, hidden_ticks=4, noise_ticks=3, tick_first=0)
    target = torch.tensor([0.05, 0.02, 0.7], dtype=torch.float64, device="cuda")

    def grads(fn):
        ro = cm.rollout.WalkingRollout(cfg, nb)
        S = _cu(s0).requires_grad_(True)
        H, Z, G = (_cu(mm[key]).requires_grad_(True) for key in ("hidden_wrench", "state_noise", "force_gain"))
        states = fn(ro, S, H, Z, G)
        (((states[-1, :, 0:3].to(torch.float64) - target) ** 2).sum() + states[3, :, 6:9].to(torch.float64).sum()).backward()
        torch.cuda.synchronize()
        return ro, states.detach(), S.grad, H.grad, Z.grad, G.grad
    a = grads(lambda ro, S, H, Z, G: cm.rollout_differentiable(ro, ticks, S, device_walk=True, hidden_wrench=H, state_noise=Z, force_gain=G))
    b = grads(lambda ro, S, H, Z, G: cm.rollout_differentiable_checkpointed_mismatch(ro, ticks, S, 4, hidden_wrench=H, state_noise=Z, force_gain=G))
    for name, x, y in zip(("states", "state0.grad", "hidden_wrench.grad", "state_noise.grad", "force_gain.grad"), a[1:], b[1:]):
        _same_bits(y, x, name)
        assert float(x.abs().max()) > 0, name
    assert b[0].last_backward["tape_rows_peak"] <= 5 and "checkpoints" in b[0].last_walk and "tape" not in b[0].last_walk
    assert tuple(b[3].shape) == (4, nb, 6) and tuple(b[4].shape) == (3, nb, 9)


# ---- 9. no host read ----
def test_nothing_is_read_back(walk18):
    """forward_sensitivity_device_mismatch and backward_device_checkpointed_mismatch under torch's sync debug mode, after a first call of each has allocated
    the workspaces; the results are the first call's, to the bit"""
    import torch
    cfg, mm = walk18["cfg"], walk18["mm"]
    ro = cm.rollout.WalkingRollout(cfg, B)
    w = ro.walk_device_taped(T, *walk18["start"], mismatch=mm)
    wc = ro.walk_device_checkpointed(T, *walk18["start"], 7, mismatch=mm)
    d = {key: _cu(a) for key, a in _walk_dirs(cfg, ro.M, 2, 50, rot=True).items() if key != "dir_push"}
    gS, gX = _cu(walk18["gS"]), _cu(walk18["gX"])
    f0 = ro.forward_sensitivity_device_mismatch(w, solutions=True, **d)
    r0 = ro.backward_device_checkpointed_mismatch(wc, gS, gX)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        f = ro.forward_sensitivity_device_mismatch(w, solutions=True, **d)
        r = ro.backward_device_checkpointed_mismatch(wc, gS, gX)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for key in KEYS:
        _same_bits(f[key], f0[key], key)
    for key in GRADS + NEW:
        _same_bits(r[key], r0[key], key)
        _same_bits(r[key], walk18["got"][key], f"against the full tape: {key}")
