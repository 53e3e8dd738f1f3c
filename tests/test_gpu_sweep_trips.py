"""GPU tests of the forward sweep's stage loop (csrc/cmpc_solver.hip: forward_sweep) at the smallest shapes where a rotated or re-pipelined
loop can go wrong.  The sweep takes four stages per trip, addresses their operands as pointer + immediate and bumps the pointers at the trip's
end; what is left runs a stage at a time.  So: resident horizons 10 (two trips + two remainder stages), 13 (three + one) and 22 (five + two),
the runtime-N variant at N = 17 (no instantiation of its own), and the HBM-factor variant (two stages per trip, operands fetched a stage ahead)
at N = 20 and N = 30.  B = 4 standing and B = 4 push problems each: every solve converges, no wave of the streaming stage gives up, and the
result lies within tests/parity.assert_within of the float64 oracle.  A converged solve ends in phase_finish, whose tail polish enters the
sweep at stage k0 = N - tail_stages > 0: info[:, 3] says where it ran, and it must have run somewhere in this set."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity

pytestmark = pytest.mark.gpu

B = 4
GENERATORS = {"standing": lambda N: cm.synthetic.config2_perturbed_com(B, N=N, seed=7),
              "push": lambda N: cm.synthetic.config3_external_push(B, N=N, seed=8)}
# (variant, horizon, factor storage)
VARIANTS = [("resident", 10, "lds"), ("resident", 13, "lds"), ("resident", 22, "lds"), ("runtime-N", 17, "lds"), ("hbm-factor", 20, "hbm"), ("hbm-factor", 30, "hbm")]
CASES = [(v, N, f, kind) for (v, N, f) in VARIANTS for kind in GENERATORS]

_solved = {}


def _solve(N, factors, kind):
    """One solve and one oracle solve per case, shared by the tests below and left unchanged."""
    key = (N, factors, kind)
    if key not in _solved:
        from oracle import oracle_lib as ol, problem_nlp
        cfg, P, X0 = GENERATORS[kind](N)
        assert cfg.N == N
        P32, X032 = P.astype(np.float32), X0.astype(np.float32)
        s = cm.BatchSolver(cfg, B, factors=factors)
        X, info, rc = s.solve_host(P32, X032)
        err = s.last_error
        s.close()
        Xr, infr = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64), ol.ipm_opts(tol=1e-9, mu_min=1e-10))
        assert (infr[:, 5] == 0).all(), infr[:, 5]
        _solved[key] = (cfg, P32, X, info, rc, err, Xr)
    return _solved[key]


@pytest.mark.parametrize("variant,N,factors,kind", CASES, ids=["%s-N%d-%s" % (v, N, k) for (v, N, f, k) in CASES])
def test_sweep_trips_and_remainder_match_the_oracle(variant, N, factors, kind):
    cfg, P32, X, info, rc, err, Xr = _solve(N, factors, kind)
    print(variant, N, kind, "iterations", info[:, 0].astype(int).tolist(), "info[3]", info[:, 3].astype(int).tolist())
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], err)
    parity.assert_no_sync_giveups(info)
    worst = parity.worst_errors(N, P32, X, Xr)
    print("   worst", worst)
    parity.assert_within(N, worst)


def test_the_tail_polish_entered_the_sweep_past_stage_zero():
    """info[:, 3] carries 100000 where the tail polish ran (include/cmpc.h): the sweep's entry at k0 > 0, with the pointers of stage k0 and a
    trip count of its own.  Whether a problem triggers it at the default threshold is the problem's business (printed per case); the solve below with the
    trigger at its floor takes it."""
    polished = {}
    for (v, N, f, kind) in CASES:
        info = _solve(N, f, kind)[3]
        polished[(v, N, kind)] = int(((info[:, 3] % 1000000) >= 100000).sum())
    print("polished problems per case at the default trigger:", polished)
    _forced_tail_polish()


def _forced_tail_polish():
    """The same entry with the trigger at its floor, so that it is taken whatever the problems do: N = 13, k0 = 10 -- the sweep starts with the pointers of
    stage 10, runs no whole trip and three remainder stages."""
    from oracle import oracle_lib as ol, problem_nlp
    N = 13
    cfg, P, X0 = GENERATORS["push"](N)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B, factors="lds", tail_trigger=1e-12)
    X, info, rc = s.solve_host(P32, X032)
    err = s.last_error
    s.close()
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], err)
    parity.assert_no_sync_giveups(info)
    assert ((info[:, 3] % 1000000) >= 100000).any(), info[:, 3]
    Xr, infr = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64), ol.ipm_opts(tol=1e-9, mu_min=1e-10))
    assert (infr[:, 5] == 0).all()
    parity.assert_within(N, parity.worst_errors(N, P32, X, Xr))
