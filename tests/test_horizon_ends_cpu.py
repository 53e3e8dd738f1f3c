"""No GPU: what tests/test_gpu_horizon_ends.py rests on.  Its batches solve on the float64 oracle, lie inside the supported NLP subset and have the
Gamma patterns it states; the host tables (cmpc_dims, cmpc_nlp_sparsity) agree with the oracle's Jacobian and Hessian structure at both ends of the
horizon range; and the CPU model of the shipped algorithm (oracle/ipm_ref.c with mix=True at the library's defaults) is run over the standing
batches and printed, as the record of what the model predicts next to the device's figures (profiles/horizon_ends.txt)."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity
from tests.test_gpu_horizon_ends import ALL_BATCHES, PUSH_LONG_SWING, PUSH_SHORT_GAMMA, STANDING_SHORT, batch, horizon

_cache = {}


def oracle_solve(family, key):
    """-> (cfg, P32, X032, Xr): the float64 oracle converged to 1e-9 on the batch's float32 inputs; asserts that it converged on every problem."""
    if (family, key) not in _cache:
        from oracle import oracle_lib as ol, problem_nlp
        cfg, P, X0 = batch(family, key)
        P32, X032 = P.astype(np.float32), X0.astype(np.float32)
        Xr, info = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64), ol.ipm_opts(tol=1e-9, mu_min=1e-10),
                                      nthreads=16)
        assert (info[:, 5] == 0).all(), (family, key, info[:, 5])
        _cache[(family, key)] = (cfg, P32, X032, Xr)
    return _cache[(family, key)]


def model_solve(cfg, P32, X032):
    """The CPU model of the device algorithm at cmpc_create's defaults: float32 storage / float64 residuals (mix), tolerance cmpc_default_tolerance(N): 1e-6 for
    N = 4 .. 20, 3e-7 beyond and for N <= 3, barrier floor 5e-8, 40 iterations, final extrapolation, tail polish of 3 stages (off where tail_stages >= horizon).  -> (X, info)"""
    from oracle import oracle_lib as ol, problem_nlp
    N = cfg.N
    opts = ol.ipm_opts(tol=cm._capi.lib().cmpc_default_tolerance(N), mu_min=5e-8, max_iter=40, tail_stages=3 if N > 3 else 0)
    return ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64), opts, mix=True, nthreads=16)


def outside_limits(N, P32, X, Xr):
    """-> (number of problems with a quantity at or above parity.limits, worst error per quantity)"""
    lim = parity.limits(N)
    over = sum(any(not e[k] < lim[k] for k in lim) for e in (parity.errors(N, P32[b], X[b], Xr[b]) for b in range(P32.shape[0])))
    return over, parity.worst_errors(N, P32, X, Xr)


@pytest.mark.parametrize("family,key", ALL_BATCHES, ids=["%s-%s" % (f, k) for f, k in ALL_BATCHES])
def test_batches_solve_on_the_oracle_inside_the_subset(family, key):
    cfg, P32, X032, Xr = oracle_solve(family, key)
    N = horizon(key)
    assert cfg.N == N and P32.shape[0] == (256 if family.endswith("short") else 16)
    assert np.isfinite(Xr).all()
    assert not any(parity.outside_subset(N, P32[b]) for b in range(P32.shape[0]))


def test_gamma_patterns_of_the_push_batches():
    for key, pattern in PUSH_SHORT_GAMMA.items():
        cfg, P32, _, _ = oracle_solve("push_short", key)
        L = cm.Layout(cfg.N)
        for b in (0, 255):
            assert P32[b, L.p_gam[0]:L.p_gam[0] + cfg.N].astype(int).tolist() == pattern, key
            assert (P32[b, L.p_gam[1]:L.p_gam[1] + cfg.N] == 1).all()
    for N, (start, length) in PUSH_LONG_SWING.items():
        cfg, P32, _, _ = oracle_solve("push_long", N)
        L = cm.Layout(N)
        assert P32[0, L.p_gam[0]:L.p_gam[0] + N].astype(int).tolist() == [1] * start + [0] * length + [1] * (N - start - length)
    # the candidate schedules at N = 40 land more often inside the horizon than any other tested problem does (N = 30: at most 4)
    cfg, P32, _, _ = oracle_solve("candidates", 40)
    most = max(sum(len(parity.landing_stages(40, P32[b], c)) for c in range(2)) for b in range(16))
    _, P30, _ = cm.synthetic.config5_footstep_candidates(256, seed=3)
    most30 = max(sum(len(parity.landing_stages(30, P30[b].astype(np.float32), c)) for c in range(2)) for b in range(256))
    print("landings per horizon: N = 40", most, "N = 30 (256 problems)", most30)
    assert most > most30


@pytest.mark.parametrize("N", [2, 3, 4, 5, 9, 31, 40])
def test_host_tables_agree_with_the_oracles_structure(N):
    """cmpc_dims and cmpc_nlp_sparsity against the (row, col) structure oracle/nlp_ref.c writes: the same counts, no entry twice, the same sets."""
    from oracle import oracle_lib as ol, problem_nlp
    lib = cm._capi.lib()
    v = [C.c_int() for _ in range(5)]
    assert lib.cmpc_dims(N, *[C.byref(a) for a in v]) == 0
    nx, npar, ng, nnzj, nnzh = [a.value for a in v]
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    oc = problem_nlp.oracle_cfg(cfg)
    assert ol.dims(oc) == (nx, npar, ng, nnzj, nnzh)
    L = cm.Layout(N)
    assert (L.nx, L.np, L.ng) == (nx, npar, ng)
    jr = np.full(nnzj, -1, np.int32); jc = np.full(nnzj, -1, np.int32); hr = np.full(nnzh, -1, np.int32); hc = np.full(nnzh, -1, np.int32)
    assert lib.cmpc_nlp_sparsity(N, jr.ctypes.data, jc.ctypes.data, hr.ctypes.data, hc.ctypes.data) == 0
    rng = np.random.default_rng(N)
    x, p = rng.normal(size=nx), rng.normal(size=npar)
    r, c, _ = ol.nlp_jac(oc, x, p)
    mine, theirs = list(zip(jr.tolist(), jc.tolist())), list(zip(r.tolist(), c.tolist()))
    assert len(set(mine)) == nnzj and len(set(theirs)) == nnzj and set(mine) == set(theirs)
    assert jr.min() >= 0 and jr.max() < ng and jc.min() >= 0 and jc.max() < nx and (np.diff(jc) >= 0).all()
    r, c, _ = ol.nlp_hess(oc, x, p, 1.0, rng.normal(size=ng))
    mine, theirs = list(zip(hr.tolist(), hc.tolist())), list(zip(r.tolist(), c.tolist()))
    assert len(set(mine)) == nnzh and len(set(theirs)) == nnzh and set(mine) == set(theirs)
    assert hr.min() >= 0 and max(hr.max(), hc.max()) < nx and (np.diff(hc) >= 0).all()


def test_dims_refuses_what_create_refuses():
    """Neither needs a device for it: the range is checked first."""
    lib = cm._capi.lib()
    for N in (-1, 0, 1, 41, 1000):
        v = [C.c_int(-7) for _ in range(5)]
        assert lib.cmpc_dims(N, *[C.byref(a) for a in v]) == -1 and [a.value for a in v] == [-7] * 5
        assert b"[2, 40]" in lib.cmpc_last_error(None)
        ccfg = cm.solver._c_config(cm.config.ergocub_gazebo_v1(20, 0.06))
        ccfg.horizon = N
        h = C.c_void_p()
        assert lib.cmpc_create(C.byref(ccfg), 4, 0, C.byref(h)) == -1 and not h.value
        assert b"cmpc_create" in lib.cmpc_last_error(None) and b"[2, 40]" in lib.cmpc_last_error(None)
    for N in (2, 40):
        assert lib.cmpc_dims(N, None, None, None, None, None) == 0


def test_cpu_model_sweep_of_the_standing_batches():
    """The record of what the CPU model of the shipped algorithm predicts at the library's defaults (run with -s to read it): per horizon, the
    problems outside parity.limits and the worst errors.  Asserts only that the oracle converged and that the model returns status 0 throughout:
    the misses it prints are answers reported as converged."""
    print()
    for N in STANDING_SHORT:
        cfg, P32, X032, Xr = oracle_solve("standing_short", N)
        Xm, im = model_solve(cfg, P32, X032)
        over, worst = outside_limits(N, P32, Xm.astype(np.float64), Xr)
        print("model standing N %2d: outside limits %3d of %d, iterations mean %.2f max %d, " % (N, over, P32.shape[0], im[:, 0].mean(), im[:, 0].max())
              + " ".join("%s %.1e" % kv for kv in worst.items()))
        assert (im[:, 5] == 0).all(), (N, im[:, 5])
