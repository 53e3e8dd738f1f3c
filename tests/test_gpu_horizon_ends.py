"""GPU: every class of horizon cmpc_create accepts (2 .. CMPC_NMAX = 40), held to the float64 oracle and to the project's existing limits.

The other GPU files run horizons 10 .. 30.  Here: the smallest horizon (N = 2: sq_init builds the descriptors of stages 1 and 0, the consumers'
"stage after next" never exists, the warm shift repeats knot 1); the tail polish switched off (N <= 3: tail_stages >= horizon) and covering every
stage but the first (N = 4, k0 = 1); the largest resident image without an instantiation of its own (N = 21); the first horizon whose resident
image exceeds 160 KiB, where a factors="lds" request is served by the HBM-factor variant (N = 23); and the horizons above 30 (31, 35, 40), which
run the run-time-N HBM-factor variant with slacks and multipliers in HBM, 41 lanes in the lane-per-stage scans and the largest scratch stride.

Every limit is an existing one, imported from where it lives (tests/parity.py, test_gpu_multipliers.py, test_gpu_sensitivity.py,
test_gpu_nlp_eval.py).  The batches below are held by tests/test_horizon_ends_cpu.py: the oracle solves every problem, every problem is inside
the supported subset, the Gamma patterns are the stated ones.  Device and CPU-model figures per cell: profiles/horizon_ends.txt
(tools/gpu_horizon_ends.py)."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity

pytestmark = pytest.mark.gpu

# ---- the batches: (family, key) -> (cfg, P, X0).  key = N, or (N, swing) where a horizon has two push batches ----
PUSH_SHORT_SWING = {2: (1, 1), 3: (1, 1), 4: (1, 2), 7: (2, 3)}
PUSH_SHORT = [(2, (1, 1)), (2, (0, 1)), (3, (1, 1)), (4, (1, 2)), (7, (2, 3))]   # N = 2, swing (0, 1): the foot is in the air at stage 0 and lands at stage 1
PUSH_SHORT_GAMMA = {(2, (1, 1)): [1, 0], (2, (0, 1)): [0, 1], (3, (1, 1)): [1, 0, 1], (4, (1, 2)): [1, 0, 0, 1], (7, (2, 3)): [1, 1, 0, 0, 0, 1, 1]}
PUSH_LONG_SWING = {21: (7, 7), 23: (7, 8), 31: (10, 10), 35: (12, 12), 40: (13, 13)}
STANDING_SHORT = [2, 3, 4, 7, 10, 12, 13, 20]
STANDING_LONG = [21, 23, 31, 35, 40]
CANDIDATES = [31, 35, 40]
LDS_NMAX = 22   # the largest horizon whose resident image fits 160 KiB (tests/test_host_logic.py)


def batch(family, key):
    if family == "push_short":
        N, swing = key
        cfg = cm.config.ergocub_gazebo_v1(N, 0.1)
        return (cfg,) + tuple(cm.synthetic.walking_push(cfg, 256, 30.0, min(2, N), 700 + N, swing=swing)[1:])
    if family == "push_long":
        cfg = cm.config.ergocub_gazebo_v1(key, 0.06)
        return (cfg,) + tuple(cm.synthetic.walking_push(cfg, 16, 30.0, 2, 31 + key, swing=PUSH_LONG_SWING[key])[1:])
    if family == "standing_short":
        return cm.synthetic.config2_perturbed_com(256, N=key, seed=900 + key)
    if family == "standing_long":
        return cm.synthetic.config2_perturbed_com(16, N=key, seed=7)
    if family == "candidates":
        return cm.synthetic.config5_footstep_candidates(16, N=key, seed=3 + key)
    raise ValueError(family)


def horizon(key):
    return key[0] if isinstance(key, tuple) else key


ALL_BATCHES = ([("push_short", k) for k in PUSH_SHORT] + [("push_long", N) for N in PUSH_LONG_SWING] + [("standing_short", N) for N in STANDING_SHORT]
               + [("standing_long", N) for N in STANDING_LONG] + [("candidates", N) for N in CANDIDATES])
# "lds" where the resident image fits, "hbm" everywhere
CELLS = [(f, k, st) for (f, k) in ALL_BATCHES for st in (("lds", "hbm") if horizon(k) <= LDS_NMAX else ("hbm",))]


def cell_id(cell):
    f, k, st = cell[:3]
    return "%s-N%d%s-%s" % (f, horizon(k), "-swing%d_%d" % k[1] if isinstance(k, tuple) else "", st)


# Cells where the device returns status 0 outside parity.limits (standing family, N <= 13 only: the one place where the CPU model of the shipped
# algorithm, oracle/ipm_ref.c with mix=True at the library's defaults, itself leaves the limits -- a weakly active friction row of the first
# stages left at its sqrt(mu_min / curvature) bias).  (family, key, storage) -> measured figures, from profiles/horizon_ends.txt.
_WHERE = "; profiles/horizon_ends.txt"
OUTSIDE_LIMITS = {
    ("standing_short", 2, "lds"): "57 of 256 outside, force0 3.1e-1 dcom 5.7e-1 (31 problems status 1)" + _WHERE,
    ("standing_short", 2, "hbm"): "59 of 256 outside, force0 3.1e-1 dcom 5.7e-1 (31 problems status 1)" + _WHERE,
    ("standing_short", 3, "lds"): "60 of 256 outside, force0 1.9e-2 dcom 5.1e-2 (30 problems status 1)" + _WHERE,
    ("standing_short", 3, "hbm"): "63 of 256 outside, force0 1.9e-2 dcom 5.0e-2 (30 problems status 1)" + _WHERE,
    ("standing_short", 4, "lds"): "99 of 256 outside, force0 3.3e-3 dcom 9.5e-3" + _WHERE,
    ("standing_short", 4, "hbm"): "101 of 256 outside, force0 3.3e-3 dcom 9.5e-3" + _WHERE,
    ("standing_short", 7, "lds"): "21 of 256 outside, dcom 5.9e-4" + _WHERE,
    ("standing_short", 7, "hbm"): "18 of 256 outside, force0 2.5e-4 dcom 1.7e-3" + _WHERE,
    ("standing_short", 10, "lds"): "2 of 256 outside, dcom 1.7e-4" + _WHERE,
    ("standing_short", 10, "hbm"): "4 of 256 outside, dcom 2.7e-4" + _WHERE,
    ("standing_short", 13, "lds"): "1 of 256 outside, dcom 3.3e-4" + _WHERE,
    ("standing_short", 13, "hbm"): "1 of 256 outside, dcom 3.3e-4" + _WHERE,
}
# The standing cells at N = 2 and N = 3 also leave problems at status 1: the kernel asks, beyond the model's residual test, for a Newton step below the
# step tolerance, and with a weakly active friction row at the barrier floor the step of these problems contracts too slowly for 40 iterations
# (measured at tolerance 1e-6: 80 iterations converge all at N = 3 and all but 10 at N = 2; the model, without that test, returns status 0 up to 4e-2 off).
NOT_CONVERGED = {
    ("standing_short", 2, "lds"): "31 of 256 at status 1 after 40 iterations (mean 15.6)" + _WHERE, ("standing_short", 2, "hbm"): "31 of 256 at status 1 after 40 iterations (mean 15.6)" + _WHERE,
    ("standing_short", 3, "lds"): "30 of 256 at status 1 after 40 iterations (mean 16.5)" + _WHERE, ("standing_short", 3, "hbm"): "30 of 256 at status 1 after 40 iterations (mean 16.6)" + _WHERE,
}

_batches, _oracle, _solved = {}, {}, {}


def _batch32(family, key):
    if (family, key) not in _batches:
        cfg, P, X0 = batch(family, key)
        assert cfg.N == horizon(key)
        _batches[(family, key)] = (cfg, P.astype(np.float32), X0.astype(np.float32))
    return _batches[(family, key)]


def oracle(family, key):
    """The float64 oracle's solution of a batch: computed once, shared, left unchanged."""
    if (family, key) not in _oracle:
        from oracle import oracle_lib as ol, problem_nlp
        cfg, P32, X032 = _batch32(family, key)
        Xr, info = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64), ol.ipm_opts(tol=1e-9, mu_min=1e-10),
                                      nthreads=16)
        assert (info[:, 5] == 0).all(), info[:, 5]
        _oracle[(family, key)] = Xr
    return _oracle[(family, key)]


def _solve(family, key, storage):
    """One cold solve per cell at the library's defaults, shared by the tests below."""
    if (family, key, storage) not in _solved:
        cfg, P32, X032 = _batch32(family, key)
        s = cm.BatchSolver(cfg, P32.shape[0], factors=storage)
        used = s.factor_storage
        X, info, rc = s.solve_host(P32, X032)
        err = s.last_error
        s.close()
        _solved[(family, key, storage)] = (X, info, rc, err, used)
    return _solved[(family, key, storage)]


def _report(tag, N, info, worst):
    print(f"\n{tag}: iterations mean {info[:, 0].mean():.2f} max {int(info[:, 0].max())} polished {int(((info[:, 3] % 1000000) >= 100000).sum())} "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- a. the solver against the oracle ----
def _cells(expected_failures):
    return [pytest.param(c, marks=pytest.mark.xfail(strict=True, reason=expected_failures[c])) if c in expected_failures else c for c in CELLS]


@pytest.mark.parametrize("cell", _cells(NOT_CONVERGED), ids=cell_id)
def test_every_problem_converges_in_the_requested_variant(cell):
    family, key, storage = cell
    X, info, rc, err, used = _solve(family, key, storage)
    assert used == storage
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], err)
    parity.assert_no_sync_giveups(info)
    assert np.isfinite(X).all()


@pytest.mark.parametrize("cell", _cells(OUTSIDE_LIMITS), ids=cell_id)
def test_solution_within_limits_of_the_oracle(cell):
    """All problems of the batch (256 at the short horizons, 16 at the long ones) within parity.limits of ref_solve_batch(tol=1e-9, mu_min=1e-10)."""
    family, key, storage = cell
    cfg, P32, X032 = _batch32(family, key)
    X, info, rc, err, used = _solve(family, key, storage)
    N = cfg.N
    worst = parity.worst_errors(N, P32, X, oracle(family, key))
    _report(cell_id(cell), N, info, worst)
    parity.assert_within(N, worst)


@pytest.mark.parametrize("cell", [c for c in CELLS if horizon(c[1]) in (2, 40)], ids=cell_id)
def test_permuted_batch_solves_bit_identically(cell):
    family, key, storage = cell
    cfg, P32, X032 = _batch32(family, key)
    X, info, rc, err, used = _solve(family, key, storage)
    perm = np.random.default_rng(2 + cfg.N).permutation(P32.shape[0])
    assert (perm != np.arange(P32.shape[0])).any()
    s = cm.BatchSolver(cfg, P32.shape[0], factors=storage)
    Xp, infop, rcp = s.solve_host(P32[perm], X032[perm])
    s.close()
    assert rcp == rc
    np.testing.assert_array_equal(Xp, X[perm])
    np.testing.assert_array_equal(infop[:, :6], info[perm][:, :6])   # (all but the shader-clock word and the last step)


# ---- b. the storage boundary ----
def test_largest_uninstantiated_resident_image_and_the_first_that_does_not_fit():
    """N = 21 with factors="lds" at B = 16 runs resident (156 420 bytes); N = 23 with the same request runs the HBM-factor variant (its resident
    image, 167 116 bytes, exceeds 160 KiB), and says so through cmpc_factor_storage.  Both match the oracle."""
    lib = cm._capi.lib()
    lib.cmpc_solver_lds_bytes.restype = C.c_size_t
    lib.cmpc_solver_lds_bytes.argtypes = [C.c_int, C.c_int]
    assert lib.cmpc_solver_lds_bytes(21, 0) <= 160 * 1024 < lib.cmpc_solver_lds_bytes(23, 0)
    assert lib.cmpc_solver_lds_bytes(23, 1) <= 160 * 1024
    assert _solve("push_long", 21, "lds")[4] == "lds"
    cfg, P32, X032 = _batch32("push_long", 23)
    s = cm.BatchSolver(cfg, 16, factors="lds")
    assert s.factor_storage == "hbm"
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], s.last_error)
    s.close()
    parity.assert_no_sync_giveups(info)
    parity.assert_within(23, parity.worst_errors(23, P32, X, oracle("push_long", 23)))
    np.testing.assert_array_equal(X, _solve("push_long", 23, "hbm")[0])      # (the same variant as an "hbm" request: bit-identical)
    X21, info21 = _solve("push_long", 21, "lds")[:2]
    assert (info21[:, 5] == 0).all()
    parity.assert_within(21, parity.worst_errors(21, _batch32("push_long", 21)[1], X21, oracle("push_long", 21)))


# ---- c. the edges of the tail polish ----
@pytest.mark.parametrize("storage", ["lds", "hbm"])
def test_polish_covering_every_stage_but_the_first(storage):
    """N = 4, tail_stages 3: with the trigger at its floor the polish takes the sweep's entry at k0 = 1 (info[:, 3] carries its mark) and the result
    matches the oracle, as in test_gpu_sweep_trips._forced_tail_polish at N = 13."""
    key = (4, PUSH_SHORT_SWING[4])
    cfg, P32, X032 = _batch32("push_short", key)
    s = cm.BatchSolver(cfg, P32.shape[0], factors=storage, tail_trigger=1e-12)
    X, info, rc = s.solve_host(P32, X032)
    err = s.last_error
    s.close()
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], err)
    parity.assert_no_sync_giveups(info)
    assert ((info[:, 3] % 1000000) >= 100000).any(), info[:, 3]
    worst = parity.worst_errors(4, P32, X, oracle("push_short", key))
    _report("forced polish N=4 " + storage, 4, info, worst)
    parity.assert_within(4, worst)


@pytest.mark.parametrize("storage", ["lds", "hbm"])
def test_polish_is_off_at_three_stages(storage):
    """N = 3: tail_stages >= horizon switches the polish off in cmpc_create, so the trigger at its floor changes nothing -- no mark, and bit for bit
    the solve at the default trigger."""
    key = (3, PUSH_SHORT_SWING[3])
    cfg, P32, X032 = _batch32("push_short", key)
    s = cm.BatchSolver(cfg, P32.shape[0], factors=storage, tail_trigger=1e-12)
    X, info, rc = s.solve_host(P32, X032)
    s.close()
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5])
    assert ((info[:, 3] % 1000000) < 100000).all(), info[:, 3]
    np.testing.assert_array_equal(X, _solve("push_short", key, storage)[0])
    parity.assert_within(3, parity.worst_errors(3, P32, X, oracle("push_short", key)))


# ---- d. the warm path ----
def shift_ref(N, X):
    """cmpc_shift_solution_device restated: every block of x moves one knot towards the present and repeats its last knot."""
    L = cm.Layout(N)
    out = np.empty_like(X)
    blocks = [(L.com, N + 1), (L.dcom, N + 1), (L.h, N + 1)]
    for c in range(2):
        blocks += [(L.pos[c], N + 1), (L.vel[c], N)] + [(L.f[c][j], N) for j in range(4)]
    assert sum(3 * n for _, n in blocks) == L.nx
    for o, n in blocks:
        a = X[:, o:o + 3 * n].reshape(-1, n, 3)
        out[:, o:o + 3 * n] = np.concatenate([a[:, 1:], a[:, -1:]], axis=1).reshape(-1, 3 * n)
    return out


@pytest.mark.parametrize("cell", [("push_short", (2, (1, 1)), "lds"), ("push_short", (2, (1, 1)), "hbm"), ("push_long", 40, "hbm")], ids=cell_id)
def test_warm_shift_and_warm_solve(cell):
    """The warm shift against its numpy restatement (bit for bit: it only copies), and a warm solve of the same problems from the shifted solution,
    held to the oracle like the cold one."""
    import torch
    family, key, storage = cell
    cfg, P32, X032 = _batch32(family, key)
    N, B = cfg.N, P32.shape[0]
    X = _solve(family, key, storage)[0]
    s = cm.BatchSolver(cfg, B, factors=storage)
    dX0 = torch.full((B, cm.Layout(N).nx), float("nan"), dtype=torch.float32, device="cuda")
    s.shift_solution_device(torch.from_numpy(X).cuda(), dX0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dX0.cpu().numpy(), shift_ref(N, X))
    dXw, dIw = s.solve_device(torch.from_numpy(P32).cuda(), dX0, warm=True)
    torch.cuda.synchronize()
    Xw, infow = dXw.cpu().numpy(), dIw.cpu().numpy()
    s.close()
    assert (infow[:, 5] == 0).all(), infow[:, 5]
    parity.assert_no_sync_giveups(infow)
    worst = parity.worst_errors(N, P32, Xw, oracle(family, key))
    _report("warm " + cell_id(cell), N, infow, worst)
    parity.assert_within(N, worst)


# ---- e. the NLP callbacks ----
NLP_BATCHES = [("push_short", (2, (1, 1))), ("push_short", (2, (0, 1))), ("push_short", (3, (1, 1))), ("push_long", 40), ("candidates", 40)]


@pytest.mark.parametrize("family,key", NLP_BATCHES, ids=[cell_id((f, k, "nlp")) for f, k in NLP_BATCHES])
def test_nlp_callbacks_match_the_oracle(family, key):
    """f, g, grad f, jac, hess and cmpc_eval_nlp_grad_device against oracle/nlp_ref.c (1e-5 relative), as test_gpu_nlp_eval.py does at N = 20 / 30."""
    from tests.test_gpu_nlp_eval import check_callbacks_against_oracle, check_nlp_grad_against_oracle
    cfg, P32, X032 = _batch32(family, key)
    check_callbacks_against_oracle(cfg, P32[:4], X032[:4])
    check_nlp_grad_against_oracle(cfg, P32[:4], X032[:4])


# ---- f. the multipliers ----
MULT_CELLS = [("push_short", (2, (1, 1)), "lds"), ("push_short", (2, (0, 1)), "lds"), ("push_short", (3, (1, 1)), "lds"), ("push_short", (4, (1, 2)), "lds"),
              ("push_long", 21, "hbm"), ("push_long", 40, "hbm")]


@pytest.mark.parametrize("cell", MULT_CELLS, ids=cell_id)
def test_exported_multipliers_certify_the_returned_x(cell):
    """(x, lam) of the device record is a KKT point of the reference NLP, on the host in float64 and by the device certificate: STAT, FEAS, COMPL and
    SIGN of test_gpu_multipliers.py.  64 problems of the short batches, all 16 of the long ones."""
    from tests.test_gpu_multipliers import _kkt_all, _solve as solve_with_multipliers
    family, key, storage = cell
    cfg, P32, X032 = _batch32(family, key)
    s, X, info, lam, cert = solve_with_multipliers(cfg, P32[:64], X032[:64], factors=storage)
    assert s.factor_storage == storage
    _kkt_all(cfg, P32[:64], X, info, lam, cert, cell_id(cell))
    s.close()


# ---- g. the sensitivities ----
SENS_CELLS = [("push_short", (2, (1, 1)), "lds"), ("push_short", (2, (1, 1)), "hbm"), ("push_short", (3, (1, 1)), "lds"), ("push_short", (3, (1, 1)), "hbm"),
              ("push_long", 40, "hbm")]


@pytest.mark.parametrize("cell", SENS_CELLS, ids=cell_id)
def test_sensitivities_match_sens_ref_and_adjoint(cell):
    """The body of test_gpu_sensitivity.test_kernel_matches_sens_ref_and_adjoint (JVP with k = 9, VJP, adjoint identity; its REF, ADJ and RESID; problems
    0, 1 and B - 1 against sens_ref) on the first 16 rows of the push batch."""
    from tests.test_gpu_sensitivity import check_sens_ref_and_adjoint
    family, key, storage = cell
    cfg, P32, X032 = _batch32(family, key)
    check_sens_ref_and_adjoint(cfg, P32[:16], X032[:16], storage, cell_id(cell))


# ---- h. the range ----
def test_horizons_outside_the_range_are_refused_by_create_and_dims():
    lib = cm._capi.lib()
    for N in (1, 41):
        ccfg = cm.solver._c_config(cm.config.ergocub_gazebo_v1(N, 0.06))
        h = C.c_void_p()
        assert lib.cmpc_create(C.byref(ccfg), 4, 0, C.byref(h)) == -1 and not h.value
        assert b"[2, 40]" in lib.cmpc_last_error(None), lib.cmpc_last_error(None)
        v = [C.c_int(-7) for _ in range(5)]
        assert lib.cmpc_dims(N, *[C.byref(a) for a in v]) == -1
        assert b"cmpc_dims" in lib.cmpc_last_error(None) and b"[2, 40]" in lib.cmpc_last_error(None)
        assert [a.value for a in v] == [-7] * 5
    for N in (2, 40):
        v = [C.c_int() for _ in range(5)]
        assert lib.cmpc_dims(N, *[C.byref(a) for a in v]) == 0
        assert [a.value for a in v] == [45 * N + 15, 50 * N + 27, 53 * N + 15, 243 * N + 15, 348 * N - 36]
        L = cm.Layout(N)
        assert (L.nx, L.np, L.ng) == (v[0].value, v[1].value, v[2].value)
