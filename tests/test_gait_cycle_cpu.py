"""CPU: the gait-cycle generator (synthetic.gait_cycle) -- every phase of one period of the roll-out's walk as the horizon's first stage -- holds the
contact patterns the receding-horizon product meets, stays inside the supported NLP subset, and is solved by the float64 oracle (ipm_ref.c), which is
held here to the stage-agnostic generic solver on those patterns.  tests/test_gpu_gait_cycle.py holds the HIP kernels to that oracle."""
import numpy as np
import pytest

import cmpc_amd as cm
from oracle import ipm_generic, oracle_lib as ol, problem_nlp
from tests import parity

SEED = 7300
HORIZONS = [(10, 0.1), (12, 0.1), (13, 0.1), (15, 0.1), (17, 0.06), (20, 0.06), (22, 0.06), (25, 0.06), (30, 0.06)]


def gamma(N, P):
    """-> [B, 2, N] bool"""
    L = cm.Layout(N)
    return np.stack([P[:, L.p_gam[c]:L.p_gam[c] + N] > 0.5 for c in range(2)], 1)


def swing_phases(g):
    """number of maximal runs of swing stages in one foot's Gamma"""
    air = ~np.asarray(g, bool)
    return int(air[0]) + int((air[1:] & ~air[:-1]).sum())


def edge_phases(N, P):
    """Rows of a per_phase = 1 batch whose phase starts with a foot in the air or has a landing or lift-off at stage 1, N - 2 or N - 1 (the stages at
    which a swing phase enters or leaves the horizon), plus every third of the remaining phases."""
    G = gamma(N, P)
    edge, rest = [], []
    for b in range(P.shape[0]):
        change = G[b, :, 1:] != G[b, :, :-1]                  # change[c, k - 1]: a landing or a lift-off at stage k
        if (~G[b, :, 0]).any() or change[:, [0, N - 3, N - 2]].any():
            edge.append(b)
        else:
            rest.append(b)
    return sorted(edge + rest[::3])


def test_one_period_holds_the_patterns_of_the_receding_horizon():
    """Census of Gamma over one period at dt = 0.06 (fails if the generator stops producing them): a foot in the air at stage 0, a landing at stage 1,
    a lift-off at stage 1, a swing phase entering at the last stage, a landing at the last stage, both feet with a swing phase inside one horizon
    (N = 20); a foot with two swing phases in one horizon (N = 30).  Problem b is at phase b // per_phase, displaced or not."""
    for N in (20, 30):
        cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
        _, P, X0, phase = cm.synthetic.gait_cycle(cfg, 2, SEED)
        _, Pd, _, phased = cm.synthetic.gait_cycle(cfg, 2, SEED, displaced=True)
        assert P.shape[0] == 40 and (phase == np.arange(40) // 2).all() and (phased == phase).all()
        G = gamma(N, P)
        feet = G.reshape(-1, N)
        assert (~feet[:, 0]).any()                                            # a foot with Gamma_0 = 0
        assert (~feet[:, 0] & feet[:, 1]).any()                               # 0, 1, ...
        assert (feet[:, 0] & ~feet[:, 1]).any()                               # 1, 0, ...
        assert (feet[:, N - 2] & ~feet[:, N - 1]).any()                       # ..., 1, 0
        assert (~feet[:, N - 2] & feet[:, N - 1]).any()                       # ..., 0, 1
        assert ((~G[:, 0]).any(1) & (~G[:, 1]).any(1)).any()                  # both feet swing inside one horizon
        if N == 30:
            assert max(swing_phases(g) for g in feet) == 2
        # every phase of the period is its own pattern, and the yawed footsteps give R != I
        assert len({G[b].tobytes() for b in range(0, 40, 2)}) == 20
        L = cm.Layout(N)
        assert np.abs(P[:, L.p_R[0] + 1]).min() > 1e-3
        # displaced: nothing but the currentPos of the feet in the air at stage 0 differs, inside 0.8 x the box in the foot frame
        diff = P != Pd
        for c in range(2):
            cur = slice(L.p_cur[c], L.p_cur[c] + 3)
            air = ~G[:, c, 0]
            assert diff[air][:, cur][:, :2].all() and not diff[~air][:, cur].any()
            diff[:, cur] = False
            cc = cfg.contacts[c]
            for b in np.nonzero(air)[0]:
                R = Pd[b, L.p_R[c]:L.p_R[c] + 9].reshape(3, 3).T
                d = R.T @ (Pd[b, cur] - Pd[b, L.p_nom[c]:L.p_nom[c] + 3])
                assert (d >= 0.8 * np.asarray(cc.bounding_box_lower_limit) - 1e-12).all() and (d <= 0.8 * np.asarray(cc.bounding_box_upper_limit) + 1e-12).all()
                assert abs(d[2]) < 1e-12
        assert not diff.any()


@pytest.mark.parametrize("displaced", [False, True], ids=["aligned", "displaced"])
@pytest.mark.parametrize("N,dt", HORIZONS)
def test_every_phase_is_inside_the_subset_and_the_oracle_solves_it(N, dt, displaced):
    cfg = cm.config.ergocub_gazebo_v1(N, dt)
    _, P, X0, phase = cm.synthetic.gait_cycle(cfg, 4, SEED + N, displaced=displaced)
    assert P.shape[0] == 4 * (12 if dt == 0.1 else 20)
    P, X0 = P.astype(np.float32).astype(np.float64), X0.astype(np.float32).astype(np.float64)
    outside = [b for b in range(P.shape[0]) if parity.outside_subset(N, P[b])]
    assert not outside, phase[outside]
    _, info = ol.ref_solve_batch(problem_nlp.oracle_cfg(cfg), P, X0, ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=4)
    assert (info[:, 5] == 0).all(), (phase[info[:, 5] != 0], info[info[:, 5] != 0])


GENERIC_TOL = 1e-10


@pytest.mark.parametrize("N", [20, 30])
def test_structured_solver_equals_the_independent_solver_on_the_gait_cycle(N):
    """ipm_ref.c against the stage-agnostic generic solver on the displaced family, one problem of every phase edge_phases names (19 of the 20 phases
    at either horizon).  Limits: those of test_structured_solver_equals_the_independent_solver_on_fresh_problems.  Options: between that test's
    (tol 1e-9, mu_min 1e-10: force0 reaches 2.0e-6 on one N = 20 phase, above its 1e-6) and tol 1e-11, mu_min 1e-12 (one N = 30 generic solve runs out of
    600 iterations): both solvers at tol GENERIC_TOL = 1e-10, the oracle's barrier floor at 1e-11 (the generic solver's floor is tol / 10 too).
    Every compared problem has status 0 in both solvers there (the generic solver in at most 51 iterations).  Measured worst (printed):
    N = 20: com 2.6e-9, dcom 6.8e-9, force0 5.6e-7, forces 4.8e-7, pos 2.0e-7; N = 30: com 2.7e-9, dcom 7.0e-9, force0 5.7e-7, forces 4.4e-7,
    pos 1.6e-7."""
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    _, P, X0, phase = cm.synthetic.gait_cycle(cfg, 1, SEED + N, displaced=True)
    P, X0 = P.astype(np.float32).astype(np.float64), X0.astype(np.float32).astype(np.float64)
    oc = problem_nlp.oracle_cfg(cfg)
    Xs, info = ol.ref_solve_batch(oc, P, X0, ol.ipm_opts(tol=GENERIC_TOL, mu_min=GENERIC_TOL / 10, max_iter=100), nthreads=4)
    assert (info[:, 5] == 0).all(), phase[info[:, 5] != 0]
    sel = edge_phases(N, P)
    assert len(sel) >= 17
    worst = dict(com=0.0, dcom=0.0, force0=0.0, forces=0.0, pos=0.0)
    for b in sel:
        lb, ub = problem_nlp.bounds(cfg, P[b])
        r = ipm_generic.solve(oc, P[b], lb, ub, X0[b], tol=GENERIC_TOL, max_iter=600)
        assert r["status"] == 0, (b, r["iters"], r["kkt"])
        e = parity.errors(N, P[b], Xs[b], r["x"])
        for k in worst:
            worst[k] = max(worst[k], e[k])
        assert e["com"] < 1e-6 and e["dcom"] < 1e-5 and e["force0"] < 1e-6 and e["forces"] < 2e-5 and e["pos"] < 5e-6, (b, e)
    print(f"\nN = {N}: {len(sel)} phases, worst " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
