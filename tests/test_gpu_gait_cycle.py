"""GPU: the solver held to the float64 oracle at every phase of the gait cycle (synthetic.gait_cycle: each phase of one period of the roll-out's walk
as the horizon's first stage, 4 aligned + 4 displaced problems per phase) -- a foot in the air at stage 0, landings and lift-offs at the first and
last stage, both feet swinging inside one horizon: the contact patterns the per-stage free-offset mask, the landing-offset pivot blocks, the restart
logic and the subset rule branch on.  Cold parity per phase, independence of batch position and size, the warm chain across lift-off and landing, the
roll-out's own ticks, the exported multipliers and the solution sensitivities.  tests/test_gait_cycle_cpu.py holds the oracle itself to the generic
solver on these patterns.  Every limit is imported from where the project states it (tests/parity.py, test_gpu_multipliers.py,
test_gpu_sensitivity.py); measured tables: profiles/gait_cycle_accuracy.txt."""
import numpy as np
import pytest

import cmpc_amd as cm
from oracle import oracle_lib as ol, problem_nlp
from tests import parity, sens_ref
from tests.test_gait_cycle_cpu import SEED, gamma

pytestmark = pytest.mark.gpu

PER_FAMILY = 4
FAMILIES = ("aligned", "displaced")
INFO_KEEP = [0, 1, 2, 3, 4, 5, 7]        # (info[6] is the shader-clock word)
_batches = {}


def _oracle(cfg, P32, X032):
    Xr, info = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64),
                                  ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=16)
    return Xr, info


def _batch(N, dt):
    """-> (cfg, P32, X032, phase, family, Xref): rows of the aligned family first, then the displaced one (another seed: the phases in double
    support would otherwise hold every problem twice); the oracle's cold float64 solve of the float32 inputs, computed once per horizon."""
    if (N, dt) not in _batches:
        cfg = cm.config.ergocub_gazebo_v1(N, dt)
        parts = [cm.synthetic.gait_cycle(cfg, PER_FAMILY, SEED + 100 * f + N, displaced=bool(f)) for f in range(2)]
        P32 = np.concatenate([p[1] for p in parts]).astype(np.float32)
        X032 = np.concatenate([p[2] for p in parts]).astype(np.float32)
        phase = np.concatenate([p[3] for p in parts])
        family = np.repeat(np.arange(2), parts[0][1].shape[0])
        Xr, info = _oracle(cfg, P32, X032)
        assert (info[:, 5] == 0).all(), (phase[info[:, 5] != 0], family[info[:, 5] != 0])
        for a in (P32, X032, phase, family, Xr):
            a.setflags(write=False)
        _batches[(N, dt)] = (cfg, P32, X032, phase, family, Xr)
    return _batches[(N, dt)]


def _pattern(N, p):
    g = gamma(N, p[None])[0]
    return " ".join("".join("1" if v else "0" for v in g[c]) for c in range(2))


def _phase_table(N, P32, X, Xr, phase, family, info, label):
    """Worst errors per (phase, family), printed; -> [((phase, family name), worst)]"""
    rows = []
    print(f"\n{label}: worst error against the float64 oracle per phase and family (limits {parity.limits(N)})")
    print("phase family    Gamma left / right" + " " * max(0, 2 * N - 17) + "  iters  com      dcom     h        pos      force0   forces")
    for s in range(int(phase.max()) + 1):
        for f, name in enumerate(FAMILIES):
            sel = np.nonzero((phase == s) & (family == f))[0]
            w = parity.worst_errors(N, P32[sel], X[sel], Xr[sel])
            rows.append(((s, name), w))
            it = info[sel, 0].astype(int)
            print(f"{s:5d} {name:9s} {_pattern(N, P32[sel[0]])}  {it.min():2d}-{it.max():2d}  "
                  + " ".join(f"{w[k]:.2e}" for k in ("com", "dcom", "h", "pos", "force0", "forces")))
    lim = parity.limits(N)
    overall = {k: max(w[k] for _, w in rows) for k in lim}
    print(f"{label}: worst of all phases " + " ".join(f"{k} {v:.2e} ({lim[k] / max(v, 1e-300):.1f}x inside)" for k, v in overall.items()))
    return rows


def _assert_rows_within(N, rows, label):
    bad = []
    for key, w in rows:
        try:
            parity.assert_within(N, w)
        except AssertionError as e:
            bad.append((key, str(e)))
    assert not bad, (label, bad)


def _device_solve(s, P32, X032, warm=False):
    import torch
    dX, dI = s.solve_device(torch.from_numpy(np.array(P32)).cuda(), torch.from_numpy(np.array(X032)).cuda(), warm=warm)
    torch.cuda.synchronize()
    return dX.cpu().numpy(), dI.cpu().numpy()


# the (horizon, variant) pairs the suite already instantiates: compile-time horizons 10, 13 and 20 and the run-time-N kernel (17) of the resident
# variant; the N = 20 and N = 30 instantiations, the run-time-N kernel (13) and the HBM-slack form of it (25) of the HBM-factor variant
VARIANTS = [(10, 0.1, "lds"), (13, 0.1, "lds"), (17, 0.06, "lds"), (20, 0.06, "lds"), (20, 0.06, "hbm"), (13, 0.1, "hbm"), (25, 0.06, "hbm"),
            (30, 0.06, "hbm")]


@pytest.mark.parametrize("N,dt,factors", VARIANTS)
def test_cold_parity_at_every_phase(N, dt, factors):
    """Every problem of every phase converges (status 0, never 3: the generator stays inside the supported subset), no wave gave up at a hand-off
    word, and every quantity at every knot is within parity.limits of the oracle -- per phase and family, so that a failure names them."""
    cfg, P32, X032, phase, family, Xr = _batch(N, dt)
    s = cm.BatchSolver(cfg, P32.shape[0], factors=factors)
    X, info = _device_solve(s, P32, X032)
    s.close()
    rows = _phase_table(N, P32, X, Xr, phase, family, info, f"cold N = {N} {factors}")
    bad = np.nonzero(info[:, 5] != 0)[0]
    assert bad.size == 0, [(int(phase[b]), FAMILIES[family[b]], info[b, 5]) for b in bad]
    parity.assert_no_sync_giveups(info)
    _assert_rows_within(N, rows, f"N = {N} {factors}")


@pytest.mark.parametrize("N,dt,factors", [(13, 0.1, "lds"), (20, 0.06, "lds"), (20, 0.06, "hbm"), (30, 0.06, "hbm")])
def test_a_phase_does_not_depend_on_its_neighbours(N, dt, factors):
    """The batch with its phases permuted gives every problem the same bits, x and info alike; one problem of every phase solved alone on a B = 1
    handle gives the bits it has inside the batch."""
    cfg, P32, X032, phase, family, _ = _batch(N, dt)
    B = P32.shape[0]
    s = cm.BatchSolver(cfg, B, factors=factors)
    X, info = _device_solve(s, P32, X032)
    perm = np.random.default_rng(N).permutation(B)
    Xp, infop = _device_solve(s, P32[perm], X032[perm])
    s.close()
    np.testing.assert_array_equal(Xp, X[perm])
    np.testing.assert_array_equal(infop[:, INFO_KEEP], info[perm][:, INFO_KEEP])
    s1 = cm.BatchSolver(cfg, 1, factors=factors)
    for ph in range(int(phase.max()) + 1):
        b = int(np.nonzero((phase == ph) & (family == 1))[0][ph % PER_FAMILY])
        X1, info1 = _device_solve(s1, P32[b:b + 1], X032[b:b + 1])
        assert np.array_equal(X1[0], X[b]) and np.array_equal(info1[0, INFO_KEEP], info[b, INFO_KEEP]), (ph, info1[0], info[b])
    s1.close()


@pytest.mark.parametrize("N,dt,factors", [(20, 0.06, "lds"), (20, 0.06, "hbm"), (30, 0.06, "hbm")])
def test_warm_chain_across_lift_off_and_landing(N, dt, factors):
    """Problem (s + 1, j) warm-started from the solution of problem (s, j) shifted by one knot (the library's shift, solve_device(warm=True), the
    default warm policy): the previous tick's solution of another state, with the contact pattern one stage on -- across every lift-off and landing
    of the cycle.  (Phase 0 has no predecessor in the batch: it starts from its own shifted solution.)  Every solve has status 0 and is within
    parity.limits of the oracle's cold float64 solve of the same P."""
    import torch
    cfg, P32, X032, phase, family, Xr = _batch(N, dt)
    B = P32.shape[0]
    s = cm.BatchSolver(cfg, B, factors=factors)
    dP = torch.from_numpy(np.array(P32)).cuda()
    dX, dI = s.solve_device(dP, torch.from_numpy(np.array(X032)).cuda())
    dShift = torch.empty_like(dX)
    s.shift_solution_device(dX, dShift)
    torch.cuda.synchronize()
    cold = dI.cpu().numpy()
    assert (cold[:, 5] == 0).all()
    src = np.arange(B)
    later = phase > 0
    src[later] -= PER_FAMILY            # (row b is problem (phase, j) of its family: row b - PER_FAMILY is problem (phase - 1, j))
    assert (phase[src[later]] == phase[later] - 1).all() and (family[src] == family).all()
    dX0 = dShift[torch.from_numpy(src).cuda()].contiguous()
    dXw, dIw = s.solve_device(dP, dX0, warm=True)
    torch.cuda.synchronize()
    Xw, info = dXw.cpu().numpy(), dIw.cpu().numpy()
    s.close()
    rows = _phase_table(N, P32, Xw, Xr, phase, family, info, f"warm chain N = {N} {factors}")
    restarted = (info[:, 3].astype(np.int64) // 10000) % 10
    print(f"warm chain N = {N} {factors}: iterations per phase, warm (cold), mean over the phase's 8 problems; [restarted from the cold start]")
    for ph in range(int(phase.max()) + 1):
        sel = phase == ph
        print(f"  phase {ph:2d}: {info[sel, 0].mean():5.2f} ({cold[sel, 0].mean():5.2f}) max {int(info[sel, 0].max()):2d} ({int(cold[sel, 0].max()):2d})"
              f" [{int((restarted[sel] > 0).sum())}]")
    bad = np.nonzero(info[:, 5] != 0)[0]
    assert bad.size == 0, [(int(phase[b]), FAMILIES[family[b]], info[b]) for b in bad]
    parity.assert_no_sync_giveups(info)
    _assert_rows_within(N, rows, f"warm chain N = {N} {factors}")


def test_the_rollouts_own_ticks_match_the_oracle():
    """The warm, merged and adjusted operating mode: a 22-tick walking roll-out on the native tick with pushes, taped.  Every tick's own P (the
    merged and sampled lists with the adjusted landing positions, the plant's state) is solved by the oracle in float64 from the cold start, and the
    tick's X -- warm-started from the previous tick's shifted solution -- is held to it within parity.limits, tick by tick."""
    N, B, ticks = 20, 16, 22
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    rng = np.random.default_rng(21)
    com0 = np.array([0.0, 0.0, 0.7]) + rng.uniform(-0.01, 0.01, (B, 3))
    dcom0 = rng.uniform(-0.05, 0.05, (B, 3))
    h0 = rng.uniform(-0.02, 0.02, (B, 3))
    push = np.zeros((B, 3))
    push[:, :2] = rng.uniform(-20.0, 20.0, (B, 2)) / cm.synthetic.ROBOT_MASS
    ro = cm.rollout.WalkingRollout(cfg, B)
    assert ro.native_tick
    rec = ro.run(ticks, com0, dcom0, h0, push=push, push_ticks=3, record="light", tape=True)
    tape = rec["tape"]["ticks"]
    assert len(tape) == ticks and all(rec["merge_ok"])
    P = np.stack([tk["P"].cpu().numpy() for tk in tape])          # [ticks, B, n_p]
    X = np.stack([tk["X"].cpu().numpy() for tk in tape])
    info = np.stack([tk["info"].cpu().numpy() for tk in tape])
    ro.solver.close()
    P64 = P.reshape(ticks * B, -1).astype(np.float64)
    Xr, infr = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P64, cm.layout.cold_start(N, P64), ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=16)
    Xr, infr = Xr.reshape(ticks, B, -1), infr.reshape(ticks, B, -1)
    air0 = [int((~gamma(N, P[i])[:, :, 0]).any(1).sum()) for i in range(ticks)]
    print(f"\nroll-out N = {N}, B = {B}: per tick, worst error against the oracle's cold solve of the tick's own P")
    print("tick  air@0  Gamma left / right (problem 0)" + " " * 8 + "  iters  com      dcom     h        pos      force0   forces")
    rows = []
    for i in range(ticks):
        w = parity.worst_errors(N, P[i], X[i], Xr[i])
        rows.append(((i, "tick"), w))
        it = info[i][:, 0].astype(int)
        print(f"{i:4d}  {air0[i]:5d}  {_pattern(N, P[i, 0])}  {it.min():2d}-{it.max():2d}  "
              + " ".join(f"{w[k]:.2e}" for k in ("com", "dcom", "h", "pos", "force0", "forces")))
    assert sum(a > 0 for a in air0) >= ticks // 2          # (a foot is in the air at stage 0 in most ticks of a walk)
    # the two sides agree on what is solvable: where the device reports a solution the oracle has one (status 0, and never 3)
    dev_ok = info[:, :, 5] == 0
    assert (infr[:, :, 5][dev_ok] == 0).all() and not (infr[:, :, 5] == 3).any(), infr[:, :, 5]
    assert dev_ok.all(), np.argwhere(~dev_ok)
    _assert_rows_within(N, rows, "roll-out ticks")


@pytest.mark.parametrize("N,dt,factors", [(20, 0.06, "lds"), (20, 0.06, "hbm"), (30, 0.06, "hbm")])
def test_exported_multipliers_certify_every_phase(N, dt, factors):
    """The batches of the cold parity test: (returned x, exported lam_g) is a KKT point of the reference NLP at every phase, with the assertions and
    limits of test_exported_multipliers_certify_fresh_seeds (its helpers)."""
    from tests.test_gpu_multipliers import _kkt_all, _solve
    cfg, P32, X032, phase, family, _ = _batch(N, dt)
    s, X, info, lam, cert = _solve(cfg, np.array(P32), np.array(X032), factors=factors)
    _kkt_all(cfg, P32, X, info, lam, cert, f"gait cycle N = {N} {factors}")
    s.close()


@pytest.mark.parametrize("N,dt,factors", [(20, 0.06, "lds"), (20, 0.06, "hbm"), (30, 0.06, "hbm")])
def test_sensitivities_at_every_phase(N, dt, factors):
    """One displaced problem per phase: the JVP over the eight generic directions of sens_ref.directions, unit directions on x and y of the currentPos
    of the foot in the air at stage 0 (zero columns in the double-support phases) and one random covered direction, and the VJP of a random v, against
    sens_ref.Sens at the device's own (x, p, lam_g), and the adjoint identity on the device outputs.  The VJP's dense reference costs one oracle
    evaluation per entry of p: it is taken on the state, currentPos and 24 random covered entries, relative to the largest covered entry of the vector
    (read from the device's own output where that is larger than the entries taken: the adjoint identity holds the rest of it)."""
    import torch
    from tests.test_gpu_sensitivity import ADJ, REF, RESID, _dirs, _solve
    cfg, P32, X032, phase, family, _ = _batch(N, dt)
    L = cm.Layout(N)
    periods = int(phase.max()) + 1
    probe = np.array([np.nonzero((phase == ph) & (family == 1))[0][ph % PER_FAMILY] for ph in range(periods)])
    Pp, Xp0 = np.array(P32[probe]), np.array(X032[probe])
    B = len(probe)
    s, dP, dX, dI, lam = _solve(cfg, Pp, Xp0, factors=factors)
    X, Lm, info = dX.cpu().numpy(), lam.cpu().numpy(), dI.cpu().numpy()
    assert (info[:, 5] == 0).all(), info[:, 5]
    rng = np.random.default_rng(9)
    cov = sens_ref.covered_mask(N)
    k = 11
    dirs = np.zeros((B, k, L.np), np.float32)
    dirs[:, :8] = _dirs(cfg, Pp[0], Lm[0])[:8]
    G0 = gamma(N, Pp)[:, :, 0]
    for b in range(B):
        for c in range(2):
            if not G0[b, c]:
                dirs[b, 8, L.p_cur[c]] = 1.0
                dirs[b, 9, L.p_cur[c] + 1] = 1.0
    dirs[:, 10] = (rng.standard_normal((B, L.np)) * 1e-2 * cov).astype(np.float32)
    V = rng.standard_normal((B, L.nx)).astype(np.float32)
    dDX, sj = s.solution_jvp_device(dX, dP, lam, torch.from_numpy(dirs).cuda())
    dGP, sv = s.solution_vjp_device(dX, dP, lam, torch.from_numpy(V).cuda())
    torch.cuda.synchronize()
    DX, GP, sj, sv = dDX.cpu().numpy(), dGP.cpu().numpy(), sj.cpu().numpy(), sv.cpu().numpy()
    s.close()
    assert (sj[:, 0] == 0).all() and (sv[:, 0] == 0).all(), (sj[:, 0], sv[:, 0])
    print(f"\nsensitivities N = {N} {factors}: residual jvp {sj[:, 1].max():.1e} vjp {sv[:, 1].max():.1e}, weak rows max {sj[:, 2].max():.0f}, "
          f"largest Sigma {sj[:, 3].max():.1e}")
    assert sj[:, 1].max() < RESID and sv[:, 1].max() < RESID
    fixed = np.concatenate([np.arange(L.p_com0, L.p_com0 + 9)] + [np.arange(L.p_cur[c], L.p_cur[c] + 3) for c in range(2)])
    print("phase  jvp      (currentPos) vjp      adjoint")
    worst = dict(jvp=0.0, vjp=0.0, adj=0.0)
    for b in range(B):
        S = sens_ref.Sens(cfg, X[b].astype(np.float64), Pp[b].astype(np.float64), Lm[b].astype(np.float64))
        e = np.zeros(k)
        for j in range(k):
            if not dirs[b, j].any():
                assert not DX[b, j].any()
                continue
            r = S.jvp(dirs[b, j].astype(np.float64))
            e[j] = np.abs(DX[b, j] - r).max() / max(np.abs(r).max(), 1e-3)
        idx = np.unique(np.concatenate([fixed, rng.choice(np.nonzero(cov)[0], 24, replace=False)]))
        gr = S.vjp(V[b].astype(np.float64), idx=idx)
        ev = np.abs(GP[b][idx] - gr[idx]).max() / max(np.abs(gr[idx]).max(), np.abs(GP[b] * cov).max())
        u = dirs[b].astype(np.float64).sum(0)
        lhs = float(V[b].astype(np.float64) @ DX[b].astype(np.float64).sum(0))
        rhs = float(GP[b].astype(np.float64) @ u)
        ea = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-6)
        print(f"{b:5d}  {e.max():.1e}  {e[8:10].max():.1e}      {ev:.1e}  {ea:.1e}")
        worst = dict(jvp=max(worst["jvp"], e.max()), vjp=max(worst["vjp"], ev), adj=max(worst["adj"], ea))
    print(" ".join(f"{a} {v:.1e}" for a, v in worst.items()))
    assert worst["jvp"] <= REF and worst["vjp"] <= REF and worst["adj"] <= ADJ, worst
