"""Shipped-robot parity matrix (run with -m gpu on an MI355X): every robot the reference ships a centroidal_mpc.ini for
(tests/golden/ini/), solved at its own horizon, sampling time, weights, corners, friction and bounding boxes, against the float64 oracle.

The other GPU parity tests use ergoCubGazeboV1's weights, where w_pos = 2e3 keeps a pushed landing within ~0.2 mm of its nominal position:
no footstep bounding-box row is ever active there.  The shipped robots' softer w_pos (50 / 200) with 150 N pushes, and the yawed candidate
schedules of config 5, put landings on a face of the box, so the q-bound rows, their slacks and multipliers are active at the optimum.  The
tests count those faces on the oracle's solutions and require the GPU landing on the same faces."""
import os

import numpy as np
import pytest

import cmpc_amd as cm
from tests import parity

pytestmark = pytest.mark.gpu

ROBOTS = ["ergoCubGazeboV1", "ergoCubGazeboV1_1", "ergoCubSN000", "ergoCubSN001", "iCubGazeboV3"]
SEED = 7
# fewest problems of the 64 of the push family whose oracle landing sits on a box face (measured at seed 7: 31 / 14 / 11)
MIN_FACES = {"ergoCubSN000": 16, "ergoCubSN001": 8, "iCubGazeboV3": 8}


def _cfg(robot, golden_dir):
    return cm.config.from_ini(open(os.path.join(golden_dir, "ini", f"{robot}.ini")).read())


def _family(cfg, family, B):
    if family == "push":
        return cm.synthetic.walking_push(cfg, B, 150.0, 3, SEED)
    return cm.synthetic.footstep_candidates(cfg, B, SEED)


def _oracle(cfg, P32, X032):
    from oracle import oracle_lib as ol, problem_nlp
    Xr, info = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P32.astype(np.float64), X032.astype(np.float64),
                                  ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=16)
    assert (info[:, 5] == 0).all()
    return Xr


# Open findings of this matrix, narrowed to the exact problems and quantities (every other assertion of these cases still holds):
# - iCubGazeboV3 has no force-symmetry cost.  Its corner forces are determined only through the friction rows of unloaded corners (a
#   redistribution with zero net wrench is blocked by them, so the two float64 solvers agree with each other to 1e-5), and the kernel,
#   stopping at its default tolerance, returns corner forces 3e-2 (relative) away from the float64 optimum; on the yawed schedules the CoM
#   velocity follows (7e-4) and the landings sit up to ~5e-5 m off the oracle's box faces.  A tighter tolerance does not converge within the
#   iteration budget in float32.  For this robot the matrix holds CoM, footsteps (1e-4) and the box faces at the footstep limit; forces, CoM
#   velocity, angular momentum and the 1e-5 face test at full strength are test_icub_parity_at_full_strength, a strict expected failure.
# - Problems that do not converge (the status of each is pinned, so a fix -- or a new failure -- shows as a failed test):
KNOWN_UNCONVERGED = {("iCubGazeboV3", "yaw", "lds", 64): {37: 2}, ("iCubGazeboV3", "yaw", "hbm", 64): {53: 1},
                     ("ergoCubSN000", "push", "auto", 400): {116: 1}}
# - One landing lies more than 1e-5 m off the oracle's box face, held at the footstep limit only (problem index in its batch):
KNOWN_FACE_GAP = {("ergoCubSN000", 400): {65}}
# - The float64 oracle itself fails on iCubGazeboV3 push problems 114, 160 and 387 of 400: the B = 400 sample (5, 15, ..., 395) avoids them.
OPEN = {"iCubGazeboV3": ("force0", "forces", "dcom", "h")}


def _solve(robot, cfg, family, B, factors):
    _, P, X0 = _family(cfg, family, B)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B, factors=factors)
    X, info, rc = s.solve_host(P32, X032)
    s.close()
    parity.assert_no_sync_giveups(info)
    known = KNOWN_UNCONVERGED.get((robot, family, factors or "auto", B), {})
    bad = {int(b): int(info[b, 5]) for b in np.where(info[:, 5] != 0)[0]}
    assert bad == known, (bad, known)
    assert (rc == 0) == (not known), rc
    ok = np.setdiff1d(np.arange(B), list(known))
    return P32, X032, X, info, ok


def _check(robot, cfg, family, P32, X, info, Xr, tag, full=False, face_gap=()):
    N = cfg.N
    worst = parity.worst_errors(N, P32, X, Xr)
    faces = [parity.box_faces(N, P32[b], Xr[b]) for b in range(P32.shape[0])]
    n_face = sum(1 for f in faces if f)
    print(f"\nROBOT {robot} N={N} {family} {tag}: faces {n_face}/{P32.shape[0]} iters max {int(info[:, 0].max())} "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    lim = parity.limits(N)
    face_tol = 1e-5
    if robot in OPEN and not full:
        worst = {k: v for k, v in worst.items() if k not in OPEN[robot]}
        face_tol = lim["pos"]
    bad = {k: (worst[k], lim[k]) for k in worst if not worst[k] < lim[k]}
    assert not bad, (bad, worst)
    # the GPU landing sits on every face the oracle's landing sits on: within 1e-5 m (float32 storage, barrier floor 5e-8) for a landing inside
    # the horizon; a foot still in the air at the end of the horizon (row N - 1) is held by w_pos alone, and there the foot-position limit applies
    for b, f in enumerate(faces):
        if f:
            near = parity.box_faces(N, P32[b], X[b], tol=lim["pos"] if b in face_gap else face_tol) | {r for r in parity.box_faces(N, P32[b], X[b], tol=lim["pos"]) if r[1] == N - 1}
            missing = f - near
            assert not missing, (b, sorted(f), sorted(missing))
    return n_face


@pytest.mark.parametrize("factors", ["lds", "hbm"])
@pytest.mark.parametrize("family", ["push", "yaw"])
@pytest.mark.parametrize("robot", ROBOTS)
def test_shipped_robot_matches_oracle(robot, family, factors, golden_dir):
    B = 64
    cfg = _cfg(robot, golden_dir)
    P32, X032, X, info, ok = _solve(robot, cfg, family, B, factors)
    n_face = _check(robot, cfg, family, P32[ok], X[ok], info[ok], _oracle(cfg, P32[ok], X032[ok]), factors)
    if family == "push" and robot in MIN_FACES:
        assert n_face >= MIN_FACES[robot], n_face
    if family == "yaw":
        assert n_face >= B // 2, n_face


@pytest.mark.parametrize("robot", ROBOTS)
def test_shipped_robot_default_variant_at_400(robot, golden_dir):
    """B = 400 > #CU with the default factor storage: the run-time-N HBM-factor variant for every horizon but 20 (its own instantiation).
    A sample of 40 problems against the oracle."""
    B = 400
    cfg = _cfg(robot, golden_dir)
    P32, X032, X, info, ok = _solve(robot, cfg, "push", B, None)
    sample = np.setdiff1d(np.arange(5, B, 10), np.setdiff1d(np.arange(B), ok))
    gap = {i for i, b in enumerate(sample) if b in KNOWN_FACE_GAP.get((robot, B), ())}
    _check(robot, cfg, "push", P32[sample], X[sample], info[sample], _oracle(cfg, P32[sample], X032[sample]), "auto B=400", face_gap=gap)


@pytest.mark.xfail(strict=True, reason="iCubGazeboV3 (no force-symmetry cost): corner forces 3e-2 from the float64 optimum")
@pytest.mark.parametrize("factors", ["lds", "hbm"])
@pytest.mark.parametrize("family", ["push", "yaw"])
def test_icub_parity_at_full_strength(family, factors, golden_dir):
    cfg = _cfg("iCubGazeboV3", golden_dir)
    P32, X032, X, info, ok = _solve("iCubGazeboV3", cfg, family, 64, factors)
    _check("iCubGazeboV3", cfg, family, P32[ok], X[ok], info[ok], _oracle(cfg, P32[ok], X032[ok]), factors, full=True)


@pytest.mark.parametrize("robot,N", [("ergoCubSN001", None), ("ergoCubGazeboV1", 30)])
def test_facade_config_matches_oracle(robot, N, golden_dir):
    """The cmpc_config the C++ facade and solver.py build from the ini file (tests/test_facade_config_cpu.py pins that they agree): the shipped
    ipopt_tolerance (1e-2 / 1e-4) is looser than the library default, so it is passed as 0 and cmpc_create applies 3e-7 beyond N = 20.  At N = 22
    (ergoCubSN001) and N = 30 (ergoCubGazeboV1's weights) the box-face family then meets north_star's tolerance on every quantity."""
    cfg = _cfg(robot, golden_dir)
    if N is not None:
        cfg.horizon_steps = N
    assert cfg.N > 20
    ccfg = cm.solver._c_config(cfg)
    assert ccfg.tolerance == 0.0
    B = 64
    _, P, X0 = _family(cfg, "push", B)
    P32, X032 = P.astype(np.float32), X0.astype(np.float32)
    s = cm.BatchSolver(cfg, B)
    X, info, rc = s.solve_host(P32, X032)
    assert rc == 0 and (info[:, 5] == 0).all(), (info[:, 5], s.last_error)
    s.close()
    _check(robot, cfg, "push", P32, X, info, _oracle(cfg, P32, X032), f"facade N={cfg.N}")
