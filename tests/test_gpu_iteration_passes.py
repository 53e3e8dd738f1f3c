"""GPU tests of the passes of an iteration beside the forward sweeps (csrc/cmpc_solver.hip: delta_sweep, phase_residuals, phase_affine_post, phase_final_post) at the
smallest shapes where their lean forms can go wrong.

The corrector sweep takes four stages per trip from the last stage down, addresses a trip's operands as pointer + immediate, moves the pointers once per trip and reads
its operands through pointers blended by lane role; the stages that do not fill a trip run first, one at a time.  The residual pass hands the light dynamics defects to
whole waves, a kind each.  So: B = 4 problems of config3_external_push (friction rows active, a swing phase, free landing offsets) at the resident horizons 10, 13 and
20 -- remainders of 2, 1 and 0 stages -- at the runtime horizon 11 (a stage per trip, the unblended sweep), and at N = 20 through the HBM-factor storage as well (the
form both passes kept).  Every case is held to the float64 oracle with tests/parity.assert_within; the HBM-factor run must take the iterations of the resident run;
and one problem solved twice must give the same bits."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity

pytestmark = pytest.mark.gpu

B = 4
SEED = 8
# (horizon, factor storage)
CASES = [(10, "lds"), (13, "lds"), (20, "lds"), (11, "lds"), (20, "hbm")]

_solved = {}


def _solve(N, factors):
    """One solve and one oracle solve per case, shared by the tests below and left unchanged."""
    key = (N, factors)
    if key not in _solved:
        from oracle import oracle_lib as ol, problem_nlp
        cfg, P, X0 = cm.synthetic.config3_external_push(B, N=N, seed=SEED)
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


@pytest.mark.parametrize("N,factors", CASES, ids=["N%d-%s" % c for c in CASES])
def test_iteration_passes_match_the_oracle(N, factors):
    cfg, P32, X, info, rc, err, Xr = _solve(N, factors)
    print(N, factors, "iterations", info[:, 0].astype(int).tolist())
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], err)
    parity.assert_no_sync_giveups(info)
    worst = parity.worst_errors(N, P32, X, Xr)
    print("   worst", worst)
    parity.assert_within(N, worst)


def test_the_problems_exercise_friction_rows_and_free_landing_offsets():
    """What the shapes are chosen for: a swing phase inside the horizon (Gamma = 0 somewhere: its landing offsets are free, the corrector sweep's offset role and the
    box rows of the passes are in use) and a push that loads the friction rows."""
    for (N, factors) in CASES:
        cfg, P32 = _solve(N, factors)[:2]
        L = cm.Layout(N)
        gam = np.stack([P32[:, L.p_gam[c]:L.p_gam[c] + N] for c in range(2)])
        assert (gam < 0.5).any() and (gam > 0.5).any(), (N, gam)


def test_hbm_factor_run_takes_the_iterations_of_the_resident_run():
    lds, hbm = _solve(20, "lds"), _solve(20, "hbm")
    print("iterations resident", lds[3][:, 0].astype(int).tolist(), "HBM-factor", hbm[3][:, 0].astype(int).tolist())
    assert (lds[3][:, 0] == hbm[3][:, 0]).all(), (lds[3][:, 0], hbm[3][:, 0])


def test_one_problem_solved_twice_gives_the_same_bits():
    cfg, P, X0 = cm.synthetic.config3_external_push(1, N=20, seed=SEED)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, 1)
    X1, info1, rc1 = s.solve_host(P32, X032)
    X2, info2, rc2 = s.solve_host(P32, X032)
    s.close()
    assert rc1 == 0 and rc2 == 0 and info1[0, 5] == 0, (rc1, rc2, info1)
    assert X1.tobytes() == X2.tobytes()
    assert info1[:, :6].tobytes() == info2[:, :6].tobytes(), (info1, info2)   # (iterations, residuals, status; word 6 is a cycle count)
