"""GPU tests of the pass behind the last forward sweep of an iteration (csrc/cmpc_solver.hip: phase_final_post) in its resident form: the costate scans split by axis
over three waves (costate_scan_axis), the rows on the other five, every block reduction of the three fused passes behind one barrier.

The costates act on the iterate only through the exact-Hessian term, so the handles must have it on; the foot scans weigh by Gamma, so the problems need a swing phase
inside the horizon (Gamma = 0 and Gamma = 1) and free landing offsets (box rows in use): B = 4 problems of config3_external_push.  Horizons: 10, 13, 20, 22 resident
(2, 3, 3 and 4 row slots per thread; 22 is the largest LDS image), 11 on the runtime-N path and 20 through the HBM-factor storage (both keep the one-wave scan and the
two-barrier reductions).  Every case is held to the float64 oracle; the HBM-factor run must take the iterations of the resident run; the exported costates (the same
scan, at the returned iterate) must certify the returned x within the limits of tests/test_gpu_multipliers.py; one problem solved twice gives the same bits, and a
permutation of the problems the permuted bits."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity
from tests.test_gpu_multipliers import _kkt_all, _solve as _solve_with_multipliers

pytestmark = pytest.mark.gpu

B = 4
SEED = 8
# (horizon, factor storage)
CASES = [(10, "lds"), (13, "lds"), (20, "lds"), (22, "lds"), (11, "lds"), (20, "hbm")]

_solved = {}


def _problems(N):
    cfg, P, X0 = cm.synthetic.config3_external_push(B, N=N, seed=SEED)
    assert cfg.N == N
    return cfg, P.astype(np.float32), X0.astype(np.float32)


def _solve(N, factors):
    """One solve and one oracle solve per case, shared by the tests below and left unchanged."""
    key = (N, factors)
    if key not in _solved:
        from oracle import oracle_lib as ol, problem_nlp
        cfg, P32, X032 = _problems(N)
        s = cm.BatchSolver(cfg, B, factors=factors)
        assert s._ccfg.exact_hessian == 1          # (the costates reach the iterate through this term only)
        assert s.factor_storage == factors
        X, info, rc = s.solve_host(P32, X032)
        err = s.last_error
        s.close()
        Xr, infr = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64), ol.ipm_opts(tol=1e-9, mu_min=1e-10))
        assert (infr[:, 5] == 0).all(), infr[:, 5]
        _solved[key] = (cfg, P32, X032, X, info, rc, err, Xr)
    return _solved[key]


@pytest.mark.parametrize("N,factors", CASES, ids=["N%d-%s" % c for c in CASES])
def test_final_post_matches_the_oracle(N, factors):
    cfg, P32, X032, X, info, rc, err, Xr = _solve(N, factors)
    print(N, factors, "iterations", info[:, 0].astype(int).tolist())
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], err)
    parity.assert_no_sync_giveups(info)
    worst = parity.worst_errors(N, P32, X, Xr)
    print("   worst", worst)
    parity.assert_within(N, worst)


def test_the_problems_have_a_swing_phase_and_free_landing_offsets():
    """Gamma = 0 and Gamma = 1 inside the horizon: the foot scans run with both weights, and the box rows of a free landing offset are in use."""
    for (N, factors) in CASES:
        P32 = _solve(N, factors)[1]
        L = cm.Layout(N)
        gam = np.stack([P32[:, L.p_gam[c]:L.p_gam[c] + N] for c in range(2)])
        assert (gam < 0.5).any() and (gam > 0.5).any(), (N, gam)


def test_hbm_factor_run_takes_the_iterations_of_the_resident_run():
    lds, hbm = _solve(20, "lds"), _solve(20, "hbm")
    print("iterations resident", lds[4][:, 0].astype(int).tolist(), "HBM-factor", hbm[4][:, 0].astype(int).tolist())
    assert (lds[4][:, 0] == hbm[4][:, 0]).all(), (lds[4][:, 0], hbm[4][:, 0])


@pytest.mark.parametrize("N,factors", CASES, ids=["N%d-%s" % c for c in CASES])
def test_exported_costates_certify_the_returned_x(N, factors):
    """multipliers_device + kkt_certificate_device on a solve with the dual record on: the limits of tests/test_gpu_multipliers.py."""
    cfg, P32, X032 = _problems(N)
    s, X, info, lam, cert = _solve_with_multipliers(cfg, P32, X032, factors=factors)
    _kkt_all(cfg, P32, X, info, lam, cert, f"final post N={N} {factors}")
    s.close()


@pytest.mark.parametrize("N", [20, 22])
def test_solved_twice_and_permuted_gives_the_same_bits(N):
    cfg, P32, X032, X, info = _solve(N, "lds")[:5]
    perm = np.array([2, 0, 3, 1])
    s = cm.BatchSolver(cfg, B, factors="lds")
    X2, info2, rc2 = s.solve_host(P32, X032)
    Xp, infop, rcp = s.solve_host(np.ascontiguousarray(P32[perm]), np.ascontiguousarray(X032[perm]))
    s.close()
    assert rc2 == 0 and rcp == 0
    assert X.tobytes() == X2.tobytes()
    assert info[:, :6].tobytes() == info2[:, :6].tobytes(), (info, info2)   # (iterations, residuals, status; word 6 is a cycle count)
    assert X[perm].tobytes() == Xp.tobytes()
    assert info[perm][:, :6].tobytes() == infop[:, :6].tobytes(), (info[perm], infop)
