"""GPU parity tests (run with -m gpu on an MI355X): the HIP solver through the C ABI against
(a) the committed float64 goldens, (b) the float64 oracle on freshly seeded batches, and
(c) size-independent properties at BASELINE.json's full batch sizes.

Tolerance (north_star): <= 1e-4 relative on the CoM trajectory and the contact forces (forces
modulo the internal-force direction the NLP leaves undetermined, see tests/parity.py); foot
positions <= 1e-4 m.  The arithmetic is float32 storage / float64 residuals."""
import os

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity

pytestmark = pytest.mark.gpu
TOL = 1e-4

CASES = {"known_answer_n12": lambda: cm.synthetic.standing_known_answer(),
         "cfg1": lambda: cm.synthetic.config1_plumbing(),
         "cfg2": lambda: cm.synthetic.config2_perturbed_com(8),
         "cfg3": lambda: cm.synthetic.config3_external_push(8),
         "cfg5": lambda: cm.synthetic.config5_footstep_candidates(4)}


def _oracle(cfg, P32, X032, nthreads=16):
    from oracle import oracle_lib as ol, problem_nlp
    Xr, info = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64),
                                  ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=nthreads)
    assert (info[:, 5] == 0).all()
    return Xr


def _worst(cfg, P32, X, Xr):
    return parity.worst_errors(cfg.N, P32, X, Xr)


def test_hip_library_is_loaded():
    lib = cm._capi.lib()
    assert os.path.basename(lib._name) == "libcmpc_hip.so"


@pytest.mark.parametrize("name", list(CASES))
def test_matches_golden(name, golden_dir):
    d = np.load(os.path.join(golden_dir, f"argmin_{name}.npz"))
    cfg = CASES[name]()[0]
    B = d["P"].shape[0]
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(d["P"], d["X0"])
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], s.last_error)
    for b in range(B):
        e = parity.errors(cfg.N, d["P"][b], X[b], d["x_star"][b])
        assert e["com"] < TOL and e["force0"] < TOL and e["forces"] < TOL and e["pos"] < TOL, (b, e)
    s.close()


@pytest.mark.parametrize("name,which", [(n, w) for n in ("walk", "yaw", "push", "ssend", "stand", "gait") for w in ("tmp", "jit")])
def test_matches_argmin_computed_on_the_reference_code(name, which, golden_dir):
    """N = 12, dt = 0.1 goldens solved on the reference's own compiled NLP functions (swing + push, yawed footsteps; both
    baked weight sets; tests/golden/make_argmin_ref_golden.py), every knot of every quantity."""
    d = np.load(os.path.join(golden_dir, f"argmin_ref_{name}_{which}.npz"))
    cfg = cm.config.generated_code_weights(which, 12, 0.1)
    B = d["P"].shape[0]
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(d["P"], d["X0"])
    assert rc == 0 and (info[:, 5] == 0).all(), (rc, info[:, 5], s.last_error)
    parity.assert_within(cfg.N, parity.worst_errors(cfg.N, d["P"], X, d["x_star"]))
    s.close()


def test_known_answer_objective():
    """f* = 8.16487469 for the standing problem (float32 inputs: 8.1648620)."""
    from oracle import oracle_lib as ol, problem_nlp
    cfg, P, X0 = cm.synthetic.standing_known_answer()
    s = cm.BatchSolver(cfg, 1)
    X, info, rc = s.solve_host(P, X0)
    assert rc == 0
    f, _ = ol.nlp_fg(problem_nlp.oracle_cfg(cfg), X[0].astype(np.float64), P[0].astype(np.float32).astype(np.float64))
    assert abs(f - 8.1648620) < 2e-5


@pytest.mark.parametrize("gen,B", [(cm.synthetic.config2_perturbed_com, 256), (cm.synthetic.config3_external_push, 256)])
def test_batch_matches_oracle(gen, B):
    cfg, P, X0 = gen(B)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0, s.last_error
    Xr = _oracle(cfg, P32, X032)
    worst = _worst(cfg, P32, X, Xr)
    parity.assert_within(cfg.N, worst)


@pytest.mark.parametrize("gen,seed", [(cm.synthetic.config2_perturbed_com, 20261), (cm.synthetic.config3_external_push, 20262),
                                      (cm.synthetic.config5_footstep_candidates, 20263)])
def test_unseen_seed_matches_oracle(gen, seed):
    """Seeds that were never used while tuning the termination heuristics (0/1/3/11 were): all-knot forces and the
    CoM velocity included."""
    B = 128
    cfg, P, X0 = gen(B, seed=seed)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0, s.last_error
    worst = _worst(cfg, P32, X, _oracle(cfg, P32, X032))
    parity.assert_within(cfg.N, worst)


def test_config4_shard_of_8192():
    """BASELINE config 4: 65536 Monte-Carlo problems (config-3 generator, seed 2) sharded 8 x 8192.  One rank's shard
    on one GPU: every problem converges and satisfies the NLP's constraints (oracle's g), the solve is invariant under
    a permutation of the batch, and 64 sampled problems match the float64 oracle."""
    from oracle import oracle_lib as ol, problem_nlp
    lo, hi = cm.distributed.shard_bounds(65536, 8, 5)
    assert hi - lo == 8192
    cfg, P, X0 = cm.synthetic.config4_monte_carlo(65536, shard=(lo, hi))
    B = hi - lo
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0 and (info[:, 5] == 0).all(), s.last_error
    parity.assert_no_sync_giveups(info)
    perm = np.random.default_rng(4).permutation(B)
    Xp, _, _ = s.solve_host(P32[perm], X032[perm])
    np.testing.assert_array_equal(Xp, X[perm])
    oc = problem_nlp.oracle_cfg(cfg)
    N = cfg.N
    sample = np.arange(0, B, 128)
    for b in sample:
        _, g = ol.nlp_fg(oc, X[b].astype(np.float64), P32[b].astype(np.float64))
        lb, ub = problem_nlp.bounds(cfg, P32[b].astype(np.float64))
        assert np.abs(g[15:15 + 15 * N]).max() < 2e-6
        assert (g <= ub + 2e-6).all() and (g >= lb - 2e-6).all()
    Xr = _oracle(cfg, P32[sample], X032[sample])
    worst = _worst(cfg, P32[sample], X[sample], Xr)
    parity.assert_within(cfg.N, worst)


@pytest.mark.parametrize("N,dt,B", [(13, 0.1, 16), (15, 0.1, 16), (22, 0.06, 16), (17, 0.06, 16), (10, 0.1, 16), (12, 0.1, 16),
                                    (13, 0.1, 400), (22, 0.06, 400), (10, 0.1, 400), (12, 0.1, 400), (15, 0.1, 400), (17, 0.06, 400), (25, 0.06, 400)])
def test_every_shipped_horizon(N, dt, B):
    """The horizons of the robots the reference ships configurations for (ergoCubSN000: 13, iCubGazeboV3: 15, ergoCubSN001: 22;
    SURVEY 8a-1; iCub plumbing config: 10; ergoCubGazeboV1_1: 12) are compile-time instantiations of the resident kernel; 17 takes the
    run-time-N variant; B = 400 > #CU takes the HBM-factor variant with run-time N (every horizon but 20 and 30, which have their own
    instantiations; 25 has its slacks and multipliers in HBM).  Walking problems with pushes, against the oracle."""
    cfg = cm.config.ergocub_gazebo_v1(N, dt)
    assert cm.synthetic.config3_external_push(2, N=N)[0].N == N
    # config3's schedule at this sampling time: swing from knot N // 3 for N // 3 knots, 30 N pushes over two stages
    _, P, X0 = cm.synthetic.walking_push(cfg, B, 30.0, 2, 31 + N)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0 and (info[:, 5] == 0).all(), s.last_error
    sample = np.arange(0, B, max(1, B // 16))
    parity.assert_within(N, _worst(cfg, P32[sample], X[sample], _oracle(cfg, P32[sample], X032[sample])))


def test_device_and_host_entry_points_agree():
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(64)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, 64)
    Xh, infoh, rc = s.solve_host(P32, X032)
    dX, dI = s.solve_device(torch.from_numpy(P32).cuda(), torch.from_numpy(X032).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dX.cpu().numpy(), Xh)  # same kernel, same inputs: bit-identical
    assert s.last_solve_ms() > 0
    # launched from a non-default current stream the call goes straight onto that stream (no side stream, no event dependencies): same answer, in stream order
    # with the torch ops around it; cmpc_set_timing(0) stops the event pair around the launch and cmpc_last_solve_ms says so
    s.set_timing(False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dP2 = torch.from_numpy(P32).cuda(non_blocking=False) * 1.0     # (a torch op on the side stream in front of the solve)
        dX2, dI2 = s.solve_device(dP2, torch.from_numpy(X032).cuda())
        twice = dX2 * 2.0                                               # (and one behind it)
    side.synchronize()
    np.testing.assert_array_equal(dX2.cpu().numpy(), Xh)
    np.testing.assert_array_equal(twice.cpu().numpy(), 2.0 * Xh)
    assert s.last_solve_ms() < 0
    s.set_timing(True)
    s.solve_device(torch.from_numpy(P32).cuda(), torch.from_numpy(X032).cuda())
    assert s.last_solve_ms() > 0


def test_full_size_properties_config3():
    """B = 4096 (config 3): every problem converges, satisfies the NLP's constraints, batch order is
    irrelevant (problem b of a permuted batch == permuted problem), and duplicates agree bitwise."""
    from oracle import oracle_lib as ol, problem_nlp
    B = 4096
    cfg, P, X0 = cm.synthetic.config3_external_push(B)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0 and (info[:, 5] == 0).all(), s.last_error
    parity.assert_no_sync_giveups(info)
    # the first 256 of them through the resident variant (one problem per compute unit: the streaming backward stage and its hand-off words)
    sr = cm.BatchSolver(cfg, 256, factors="lds")
    Xr, infor, rcr = sr.solve_host(P32[:256], X032[:256])
    assert rcr == 0 and (infor[:, 5] == 0).all(), sr.last_error
    parity.assert_no_sync_giveups(infor)
    sr.close()
    perm = np.random.default_rng(0).permutation(B)
    Xp, _, _ = s.solve_host(P32[perm], X032[perm])
    np.testing.assert_array_equal(Xp, X[perm])
    # feasibility of a sample with the oracle's g(x): dynamics rows ~0, friction rows <= 0
    oc = problem_nlp.oracle_cfg(cfg)
    N = cfg.N
    for b in range(0, B, 512):
        _, g = ol.nlp_fg(oc, X[b].astype(np.float64), P32[b].astype(np.float64))
        lb, ub = problem_nlp.bounds(cfg, P32[b].astype(np.float64))
        assert np.abs(g[15:15 + 15 * N]).max() < 2e-6          # dynamics
        assert (g <= ub + 2e-6).all() and (g >= lb - 2e-6).all()


def test_step_adjustment_is_active_in_config3():
    cfg, P, X0 = cm.synthetic.config3_external_push(32)
    mpc = cm.CentroidalMPC(batch=32)
    assert mpc.initialize(cfg)
    L = cm.Layout(cfg.N)
    s = cm.BatchSolver(cfg, 32)
    X, info, rc = s.solve_host(P, X0)
    assert rc == 0
    land = L.x_pos(X, 0)[:, 14, :]     # left foot lands at knot 14 (Gamma = 1x6, 0x8, 1x6)
    nominal = np.array([0.1, 0.08, 0.0])
    d = land - nominal
    assert (np.abs(d[:, 0]) <= 0.01 + 1e-5).all() and (d[:, 1] >= -1e-5).all() and (d[:, 1] <= 0.05 + 1e-5).all()
    assert np.abs(d[:, :2]).max() > 5e-5   # pushes move the footstep (w_pos = 2e3 keeps it within ~0.1 mm)
    assert np.abs(d[:, 2]).max() < 1e-6    # z is an equality row (lower == upper == 0)


def test_class_surface_round_trip():
    """setState / setReferenceTrajectory / setContactPhaseList / advance / getOutput, as
    CentroidalMPCBlock.cpp:407-622 drives them, reproduce the tensor-level solve."""
    cfg, P, X0 = cm.synthetic.config3_external_push(16)
    N, L = cfg.N, cm.Layout(cfg.N)
    from cmpc_amd.synthetic import _walking_lists
    mpc = cm.CentroidalMPC(batch=16)
    assert mpc.initialize(cfg), mpc.last_error
    st = P[:, L.p_com0:L.p_com0 + 9]
    wrench = np.zeros((16, N, 6), np.float32)
    wrench[:, :, :3] = P[:, L.p_fext:L.p_fext + 3 * N].reshape(16, N, 3)
    assert mpc.set_state(st[:, 0:3], st[:, 3:6], st[:, 6:9], wrench)
    assert mpc.set_reference_trajectory(P[:, L.p_comref:L.p_comref + 3 * (N + 1)], P[:, L.p_href:L.p_href + 3 * (N + 1)])
    assert mpc.set_contact_phase_list(_walking_lists(cfg, 6, 8))
    assert mpc.advance(), mpc.last_error
    assert mpc.is_output_valid()
    out = mpc.get_output()
    s = cm.BatchSolver(cfg, 16)
    X, info, rc = s.solve_host(P, X0)
    np.testing.assert_allclose(out.forces, L.first_forces(X), rtol=0, atol=2e-5)
    assert (out.next_knots[:, 0] == 14).all() and (out.next_knots[:, 1] == -1).all()
    np.testing.assert_allclose(out.next_positions[:, 0], L.x_pos(X, 0)[:, 14], atol=2e-6)
    # warm start (previous solution shifted by one knot, is_warm_start_enabled) reaches the same optimum
    X_cold, _ = mpc.get_solution()
    assert mpc.set_initial_guess(None, shift_previous=True) and mpc.advance()
    X_warm, info_warm = mpc.get_solution()
    assert (info_warm[:, 5] == 0).all()
    for b in range(16):
        e = parity.errors(cfg.N, P[b], X_warm[b], X_cold[b])
        assert e["com"] < TOL and e["force0"] < TOL, e


def test_error_paths_return_false_like_the_reference():
    mpc = cm.CentroidalMPC(batch=2)
    assert not mpc.advance() and "initialize" in mpc.last_error
    cfg = cm.config.ergocub_gazebo_v1()
    assert mpc.initialize(cfg)
    bad = dict(R=np.zeros((2, 2, cfg.N, 3, 3)), upper=np.zeros((2, 2, cfg.N, 3)), lower=np.ones((2, 2, cfg.N, 3)),
               enabled=np.ones((2, 2, cfg.N)), nominal=np.zeros((2, 2, cfg.N + 1, 3)), current=np.zeros((2, 2, 3)))
    assert not mpc.set_contact_phase_list(bad) and "upper < lower" in mpc.last_error


def test_long_horizon_uses_global_factor_storage():
    """N = 30 (config 5) does not fit the 160 KiB LDS image; factors go to HBM scratch."""
    cfg, P, X0 = cm.synthetic.config5_footstep_candidates(64)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, 64)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0, s.last_error
    Xr = _oracle(cfg, P32, X032)
    worst = _worst(cfg, P32, X, Xr)
    parity.assert_within(cfg.N, worst)


@pytest.mark.parametrize("factors", ["lds", "hbm"])
def test_solve_does_not_depend_on_stale_lds(factors, monkeypatch):
    """LDS arrives uninitialised: poison every CU's LDS with NaNs (test hook of the C ABI), then solve more
    problems than there are CUs so that later workgroups also inherit an earlier workgroup's image.  Results must
    be bit-identical to an unpoisoned solve and all converged.  (Regression: entries read under a zero weight.)"""
    B = 768
    cfg, P, X0 = cm.synthetic.config3_external_push(B, seed=11)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B, factors=factors)
    X1, info1, rc1 = s.solve_host(P32, X032)
    assert rc1 == 0 and (info1[:, 5] == 0).all(), s.last_error
    assert s._lib.cmpc_test_poison_lds(s._h) == 0
    X2, info2, rc2 = s.solve_host(P32, X032)
    assert rc2 == 0 and (info2[:, 5] == 0).all(), s.last_error
    np.testing.assert_array_equal(X1, X2)
    np.testing.assert_array_equal(info1[:, 0], info2[:, 0])


def test_fixed_initial_barrier_parameter_still_available(golden_dir):
    """cmpc_config.mu_init > 0 pins the initial barrier parameter (default: per problem from its initial
    infeasibility); both reach the same optimum."""
    cfg, P, X0 = cm.synthetic.config3_external_push(8)
    d = np.load(os.path.join(golden_dir, "argmin_cfg3.npz"))
    for kw in ({}, {"mu_init": 0.1}, {"mu_init": 0.5}):
        s = cm.BatchSolver(cfg, 8, **kw)
        X, info, rc = s.solve_host(d["P"].astype(np.float32), d["X0"].astype(np.float32))
        assert rc == 0 and (info[:, 5] == 0).all(), (kw, s.last_error)
        for b in range(8):
            e = parity.errors(cfg.N, d["P"][b], X[b], d["x_star"][b])
            assert e["com"] < TOL and e["force0"] < TOL and e["pos"] < TOL, (kw, b, e)
        s.close()


def test_compact_output_kernel_matches_the_torch_restatement():
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(64)
    s = cm.BatchSolver(cfg, 64)
    dX, dInfo = s.solve_device(torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(X0.astype(np.float32)).cuda())
    cols = torch.from_numpy(cm.distributed.compact_columns(cfg.N)).cuda()
    ref = cm.distributed.compact_output(dX, dInfo, cols)
    out = s.compact_output_device(dX, dInfo)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape)
    np.testing.assert_array_equal(out.cpu().numpy(), ref.cpu().numpy())


def test_iteration_budget_exhausted_is_reported_per_problem():
    """ipopt_max_iteration too small: the reference's advance() returns false (CentroidalMPCBlock.cpp:615-619); here every
    problem reports status 1 with its last iterate (finite), and the batch call says CMPC_ERR_NOT_CONVERGED."""
    cfg, P, X0 = cm.synthetic.config3_external_push(32)
    s = cm.BatchSolver(cfg, 32, max_iterations=2)
    X, info, rc = s.solve_host(P.astype(np.float32), X0.astype(np.float32))
    assert rc == -3 and "converge" in s.last_error
    assert (info[:, 5] == 1).all() and (info[:, 0] == 2).all()
    assert np.isfinite(X).all()


@pytest.mark.parametrize("B", [5, 1024])
def test_a_poisoned_problem_does_not_touch_its_neighbours(B):
    """One problem of the batch gets NaN parameters (resident variant at B = 5, HBM-factor variant at B = 1024): it must
    come back flagged (status != 0) without hanging the kernel, and every other problem bit-identical to a clean solve."""
    cfg, P, X0 = cm.synthetic.config3_external_push(B, seed=21)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X1, info1, rc1 = s.solve_host(P32, X032)
    assert rc1 == 0 and (info1[:, 5] == 0).all()
    bad = B // 2
    Pb = P32.copy()
    Pb[bad, :] = np.nan
    X2, info2, rc2 = s.solve_host(Pb, X032)
    assert rc2 == -3
    assert info2[bad, 5] != 0
    keep = np.arange(B) != bad
    assert (info2[keep, 5] == 0).all()
    np.testing.assert_array_equal(X1[keep], X2[keep])
    np.testing.assert_array_equal(info1[keep, 0], info2[keep, 0])


@pytest.mark.parametrize("N", [13, 20])
def test_hbm_factor_and_resident_variants_agree(N, monkeypatch):
    """The same problems through the resident variant (factor records in LDS) and the HBM-factor variant (records written to
    and read back from global scratch): both converge, to the same point.  Regression for the record stores: 16-byte buffer
    stores with an SGPR stage offset delivered single wrong dwords in some builds (N = 13, this seed: 5 of 8 problems lost)."""
    cfg, P, X0 = cm.synthetic.config3_external_push(32, N=N, seed=44)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    out = {}
    for factors in ("lds", "hbm"):
        s = cm.BatchSolver(cfg, 32, factors=factors)
        X, info, rc = s.solve_host(P32, X032)
        assert rc == 0 and (info[:, 5] == 0).all(), (factors, s.last_error)
        out[factors] = (X, info)
        s.close()
    # (the resident variants assemble a stage in the square-root form, the HBM-factor variants through the value function: the same optimum -- checked
    #  below -- by different float32 algebra, and the lagged termination test may then fire an iteration apart on a borderline problem)
    # Recorded exception (round 4, profiles/r04_experiments_not_kept.txt item 24): problem 8 of this very set at N = 20 sits on a nearly degenerate friction row.
    # Its traces in the two variants agree to four digits up to iteration 5; at iteration 6, at the barrier floor, the rounding of the float32 costates (serial
    # recursion -> scans) decides whether a multiplier of ~1e-9 blocks the dual step (ad = 0.74 instead of 1), and the resident variant then needs 11 iterations
    # where the HBM-factor variant needs 8.  511 of 512 + 63 of 64 problems of the probe (tools/gpu_variant_iters.py) are iteration-for-iteration identical in
    # both variants and both costate forms.  So: within one iteration on all problems but at most one, which must still be within three.
    diff = np.abs(out["lds"][1][:, 0] - out["hbm"][1][:, 0])
    assert (diff <= 1).sum() >= 31 and diff.max() <= 3, (out["lds"][1][:, 0], out["hbm"][1][:, 0])
    for b in range(32):
        e = parity.errors(cfg.N, P32[b], out["hbm"][0][b], out["lds"][0][b])
        assert e["com"] < 2e-5 and e["forces"] < 5e-5 and e["pos"] < 2e-5, (b, e)


@pytest.mark.parametrize("gen", ["push_recovery_n12", "walking_push_n12", "yawed_steps_n12"])
def test_streaming_stage_matches_the_value_function_stage_on_stepping_problems(gen, monkeypatch):
    """Problems with free landing offsets (pivot blocks 8 and 9 of the stage Hessian are factorised, a foot at a time) through both backward stages: the
    streaming square-root stage of the resident variants (N = 12 instantiation) and the value-function stage of the HBM-factor variants.  Same optimum, iteration
    counts within two.  (A wrong descriptor set in the streaming stage showed here first: 9 -> 12..40 iterations on these very problems.)"""
    cfg, P, X0 = getattr(cm.synthetic, gen)("tmp")
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    out = {}
    for factors in ("lds", "hbm"):
        s = cm.BatchSolver(cfg, P32.shape[0], factors=factors)
        X, info, rc = s.solve_host(P32, X032)
        assert rc == 0 and (info[:, 5] == 0).all(), (factors, info[:, 5], s.last_error)
        out[factors] = (X, info)
        s.close()
    assert np.abs(out["lds"][1][:, 0] - out["hbm"][1][:, 0]).max() <= 1, (out["lds"][1][:, 0], out["hbm"][1][:, 0])
    for b in range(P32.shape[0]):
        e = parity.errors(cfg.N, P32[b], out["hbm"][0][b], out["lds"][0][b])
        assert e["com"] < 3e-5 and e["forces"] < 1e-4 and e["pos"] < 3e-5, (b, e)


@pytest.mark.parametrize("B", [5, 1024])
@pytest.mark.parametrize("where", ["com_ref", "f_ext", "x0"])
def test_a_single_nan_is_reported_not_returned_as_converged(B, where):
    """A NaN that reaches only the right-hand side (one entry of the CoM reference, of the external force, or of the
    initial guess) leaves the first factorisation intact: every step becomes NaN, and a termination test built on fmaxf
    would read the residuals as zero.  The reference's IPOPT stops with 'invalid number' and advance() returns false
    (CentroidalMPCBlock.cpp:615-619): status != 0, rc = CMPC_ERR_NOT_CONVERGED, the neighbours untouched."""
    cfg, P, X0 = cm.synthetic.config3_external_push(B, seed=23)
    L = cm.Layout(cfg.N)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X1, info1, rc1 = s.solve_host(P32, X032)
    assert rc1 == 0
    bad = B // 3
    Pb, Xb = P32.copy(), X032.copy()
    if where == "com_ref":
        Pb[bad, L.p_comref + 3 * 7 + 1] = np.nan
    elif where == "f_ext":
        Pb[bad, L.p_fext + 3 * 2] = np.nan
    else:
        Xb[bad, L.f[1][2] + 3 * 5 + 2] = np.nan
    X2, info2, rc2 = s.solve_host(Pb, Xb)
    assert rc2 == -3
    assert info2[bad, 5] != 0, info2[bad]
    assert info2[bad, 0] <= 3                      # stopped at once, not after the iteration budget
    keep = np.arange(B) != bad
    assert (info2[keep, 5] == 0).all()
    np.testing.assert_array_equal(X1[keep], X2[keep])


def test_full_size_properties_config5():
    """BASELINE config 5 at its full size (B = 8192, N = 30; 1.16 GB of factor scratch): every problem converges and satisfies
    the NLP's constraints, the solve is invariant under a permutation of the batch, and 64 sampled problems match the float64
    oracle at north_star's tolerance on every quantity at every knot (mirrors test_config4_shard_of_8192)."""
    from oracle import oracle_lib as ol, problem_nlp
    B = 8192
    cfg, P, X0 = cm.synthetic.config5_footstep_candidates(B)
    assert cfg.N == 30
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0 and (info[:, 5] == 0).all(), s.last_error
    parity.assert_no_sync_giveups(info)
    perm = np.random.default_rng(6).permutation(B)
    Xp, _, _ = s.solve_host(P32[perm], X032[perm])
    np.testing.assert_array_equal(Xp, X[perm])
    oc = problem_nlp.oracle_cfg(cfg)
    N = cfg.N
    sample = np.arange(0, B, 128)
    for b in sample:
        _, g = ol.nlp_fg(oc, X[b].astype(np.float64), P32[b].astype(np.float64))
        lb, ub = problem_nlp.bounds(cfg, P32[b].astype(np.float64))
        assert np.abs(g[15:15 + 15 * N]).max() < 2e-6
        assert (g <= ub + 2e-6).all() and (g >= lb - 2e-6).all()
    worst = _worst(cfg, P32[sample], X[sample], _oracle(cfg, P32[sample], X032[sample]))
    parity.assert_within(cfg.N, worst)
    # the tail polish ran where the extrapolation step of the last stages was large, and only there
    polished = info[:, 3] >= 100000
    assert 0 < polished.sum() < B
    s.close()


def test_failed_scratch_allocation_is_an_error_not_a_crash():
    """cmpc_create with a batch whose factor scratch cannot be allocated (N = 30: 141 KB per problem; 3 000 000 problems = 423 GB
    against 288 GB of HBM) returns CMPC_ERR_HIP with the handle released (csrc/cmpc_api.hip: HIPCHK_CREATE -> cmpc_destroy), and
    the library keeps working."""
    import ctypes as C
    cfg = cm.config.ergocub_gazebo_v1(30, 0.06)
    lib = cm._capi.lib()
    ccfg = cm.solver._c_config(cfg)
    h = C.c_void_p()
    rc = lib.cmpc_create(C.byref(ccfg), 3_000_000, 0, C.byref(h))
    assert rc == -2 and not h.value, rc
    assert b"hipMalloc" in lib.cmpc_last_error(None)
    _, P, X0 = cm.synthetic.config5_footstep_candidates(8)
    s = cm.BatchSolver(cfg, 8)
    X, info, rc = s.solve_host(P.astype(np.float32), X0.astype(np.float32))
    assert rc == 0 and (info[:, 5] == 0).all()


def test_tail_polish_only_moves_the_tail(monkeypatch):
    """cmpc_config.tail_stages: problems whose tail is not polished are bit-identical with and without it; where it ran, the
    stages before the tail barely move and the last knots move towards the oracle."""
    B = 256
    cfg, P, X0 = cm.synthetic.config5_footstep_candidates(B, seed=77)
    N, L = cfg.N, cm.Layout(cfg.N)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s0 = cm.BatchSolver(cfg, B, tail_stages=0)
    Xa, infa, rc = s0.solve_host(P32, X032)
    assert rc == 0
    s1 = cm.BatchSolver(cfg, B)
    Xb, infb, rc = s1.solve_host(P32, X032)
    assert rc == 0
    polished = infb[:, 3] >= 100000
    assert polished.any() and (infa[:, 3] < 100000).all()
    np.testing.assert_array_equal(infa[:, 0], infb[:, 0])                # the polish is not counted as an iteration
    np.testing.assert_array_equal(Xa[~polished], Xb[~polished])
    # the stages before the tail take the same extrapolation step, at a step length limited by their own rows only: (nearly) the same numbers
    k0 = N - 3
    for c in range(2):
        for j in range(4):
            assert np.abs(L.x_force(Xa, c, j)[:, :k0] - L.x_force(Xb, c, j)[:, :k0]).max() < 1e-3
    assert np.abs(L.x_com(Xa)[:, :k0 + 1] - L.x_com(Xb)[:, :k0 + 1]).max() < 1e-5
    Xr = _oracle(cfg, P32[polished], X032[polished])
    wa, wb = _worst(cfg, P32[polished], Xa[polished], Xr), _worst(cfg, P32[polished], Xb[polished], Xr)
    # the polish is about the FORCES of the last knots (unloaded corners at the apex of their friction pyramid); the CoM velocity it leaves where the
    # tolerance put it: since the default tolerance beyond N = 20 is 3e-7 that is 3..5e-5 with and without the polish (it used to improve with it at 1e-6)
    assert wb["forces"] < wa["forces"] and wb["dcom"] < max(wa["dcom"], 0.6 * parity.TOL), (wa, wb)


@pytest.mark.parametrize("B", [5, 1024])
def test_problems_outside_the_supported_subset_are_flagged_not_solved(B):
    """include/cmpc.h states the NLP subset the kernel supports.  A raw P through cmpc_solve_device with one problem per violation (Gamma = 0.5 at
    one stage; a foot held 5 cm outside its box; a nominal position moved by 2 cm inside a stance phase): each comes back at once with status 3,
    no iteration and a finite x; every other problem bit-identical, in x and in iterations, to a clean solve (resident variant at B = 5,
    HBM-factor variant at B = 1024)."""
    import torch
    cfg, P, X0 = cm.synthetic.config3_external_push(B, seed=23)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    dX1, dI1 = s.solve_device(torch.from_numpy(P32).cuda(), torch.from_numpy(X032).cuda())
    torch.cuda.synchronize()
    X1, info1 = dX1.cpu().numpy(), dI1.cpu().numpy()
    assert (info1[:, 5] == 0).all()
    bad = {"gamma": 0, "held": B // 2, "nominal": B - 1}
    Pb = P32.copy()
    for which, b in bad.items():
        Pb[b] = parity.break_subset(cfg.N, P32[b], which)
    dX2, dI2 = s.solve_device(torch.from_numpy(Pb).cuda(), torch.from_numpy(X032).cuda())
    torch.cuda.synchronize()
    X2, info2 = dX2.cpu().numpy(), dI2.cpu().numpy()
    rows = list(bad.values())
    assert (info2[rows, 5] == 3).all() and (info2[rows, 0] <= 1).all(), info2[rows]
    assert np.isfinite(X2[rows]).all()
    keep = np.setdiff1d(np.arange(B), rows)
    assert (info2[keep, 5] == 0).all()
    np.testing.assert_array_equal(X2[keep], X1[keep])
    np.testing.assert_array_equal(info2[keep, 0], info1[keep, 0])
    # the host entry point says so: CMPC_ERR_NOT_CONVERGED, and the error text names status 3
    _, info3, rc = s.solve_host(Pb, X032)
    assert rc == -3 and "status 3" in s.last_error and "outside the supported NLP subset" in s.last_error, s.last_error
    np.testing.assert_array_equal(info3[:, 5], info2[:, 5])
    s.close()
