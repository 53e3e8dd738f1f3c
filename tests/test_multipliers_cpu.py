"""Host restatement (float64) of the multiplier interface of include/cmpc.h: the map from the solver's dual record (costates of its stage form, multipliers
of its friction and landing-offset rows) onto the reference NLP's lam_g, the KKT certificate's fields, and the gradient of the optimal cost.  Held here to
the goldens' lam_g (IPOPT's sign convention, certified by tests/golden/make_argmin_ref_golden.py) and to central finite differences of the float64 oracle's
optimal cost.  No GPU: tests/test_gpu_multipliers.py holds the device kernels to these functions."""
import os

import numpy as np
import pytest

import cmpc_amd as cm

NS, NI = 15, 44


def _ol():
    from oracle import oracle_lib as ol, problem_nlp
    return ol, problem_nlp


def _gam(N, p, c):
    L = cm.Layout(N)
    o = c * (19 * N + 6) + 15 * N
    return p[o:o + N]


def rows(N):
    """offsets of the row blocks of g (GLay of cmpc_nlp_eval.hip)"""
    o = {"init": 0, "com": 15, "dcom": 15 + 3 * N, "h": 15 + 6 * N, "pos": [15 + 9 * N, 15 + 12 * N]}
    b = 15 + 15 * N
    o["bbox"], o["fric"] = [], []
    for c in range(2):
        o["bbox"].append(b); b += 3 * N
        o["fric"].append(b); b += 16 * N
    return o


def _R(N, p, c, k):
    o = c * (19 * N + 6) + 9 * k
    return p[o:o + 9].reshape(3, 3).T        # vec(R) column-major


def _box(N, p, c):
    o = c * (19 * N + 6)
    return p[o + 12 * N:o + 15 * N].reshape(N, 3), p[o + 9 * N:o + 12 * N].reshape(N, 3)   # lower, upper


def record_from_lam(cfg, x, p, lam):
    """the dual record a solver of the stage form holds at a KKT point (x, lam) of the reference NLP: costates lam_s[N+1][15] of
    L_s = f + sum lam_{k+1}^T (phi_k - s_{k+1}) and multipliers z[N][44] (32 friction rows, 6 upper and 6 lower offset rows).  The stage form has no
    box row in stance, so its costates are those of the convention: friction and free swing box rows as given, every other row from stationarity in the
    states, knot N down to 1 -- the solver's costate recursion, through nlp_grad."""
    ol, problem_nlp = _ol()
    oc = problem_nlp.oracle_cfg(cfg)
    N = cfg.N
    o = rows(N)
    lm = lam.copy()
    lm[:15 + 15 * N] = 0
    for c in range(2):
        lo, up = _box(N, p, c)
        for k in range(N):
            for i in range(3):
                if _gam(N, p, c)[k] >= 0.5 or not np.float32(up[k, i]) - np.float32(lo[k, i]) > np.float32(1e-9):
                    lm[o["bbox"][c] + 3 * k + i] = 0
    S = np.zeros((N + 1, NS))
    Z = np.zeros((N, NI))
    for j in range(N, 0, -1):
        k = j - 1
        gx, _ = ol.nlp_grad(oc, x, p, 1.0, lm)       # (the rows of stage k are still zero)
        for blk, key in enumerate(("com", "dcom", "h")):
            lm[o[key] + 3 * k:o[key] + 3 * k + 3] = -gx[3 * (N + 1) * blk + 3 * j:3 * (N + 1) * blk + 3 * j + 3]
            S[j, 3 * blk:3 * blk + 3] = -lm[o[key] + 3 * k:o[key] + 3 * k + 3]
        for c in range(2):
            op = 9 * (N + 1) + c * (18 * N + 3) + 3 * j
            if _gam(N, p, c)[k] >= 0.5:
                lm[o["pos"][c] + 3 * k:o["pos"][c] + 3 * k + 3] = -gx[op:op + 3]
                S[j, 9 + 3 * c:12 + 3 * c] = gx[op:op + 3]
            else:   # swing: R lam_bbox = -(the rest of the gradient) -- which also folds the shares of the stance duplicates onto the landing row
                R = _R(N, p, c, k)
                lb = lm[o["bbox"][c] + 3 * k:o["bbox"][c] + 3 * k + 3]
                lm[o["bbox"][c] + 3 * k:o["bbox"][c] + 3 * k + 3] = -(R.T @ gx[op:op + 3]) + lb
                S[j, 9 + 3 * c:12 + 3 * c] = -(R @ lm[o["bbox"][c] + 3 * k:o["bbox"][c] + 3 * k + 3])
            lb = lm[o["bbox"][c] + 3 * k:o["bbox"][c] + 3 * k + 3]
            Z[k, 16 * c:16 * c + 16] = lm[o["fric"][c] + 16 * k:o["fric"][c] + 16 * k + 16]
            Z[k, 32 + 3 * c:35 + 3 * c] = np.maximum(lb, 0)
            Z[k, 38 + 3 * c:41 + 3 * c] = np.maximum(-lb, 0)
    return S, Z


def map_record(cfg, x, p, S, Z):
    """cmpc_get_multipliers_device, restated: record -> lam_g (include/cmpc.h, row by row)"""
    ol, problem_nlp = _ol()
    N = cfg.N
    o = rows(N)
    lam = np.zeros(53 * N + 15)
    for k in range(N):
        for blk, key in enumerate(("com", "dcom", "h")):
            lam[o[key] + 3 * k:o[key] + 3 * k + 3] = -S[k + 1, 3 * blk:3 * blk + 3]
        for c in range(2):
            stance = _gam(N, p, c)[k] >= 0.5
            if stance:
                lam[o["pos"][c] + 3 * k:o["pos"][c] + 3 * k + 3] = -S[k + 1, 9 + 3 * c:12 + 3 * c]
            else:
                lo, up = _box(N, p, c)
                for i in range(3):
                    if np.float32(up[k, i]) - np.float32(lo[k, i]) > np.float32(1e-9):
                        v = Z[k, 32 + 3 * c + i] - Z[k, 38 + 3 * c + i]
                    else:
                        v = -(_R(N, p, c, k)[:, i] @ S[k + 1, 9 + 3 * c:12 + 3 * c])
                    lam[o["bbox"][c] + 3 * k + i] = v
            lam[o["fric"][c] + 16 * k:o["fric"][c] + 16 * k + 16] = Z[k, 16 * c:16 * c + 16]
    # initial-condition rows from stationarity at the stage-0 columns (nlp_grad with the init rows at zero)
    gx, _ = ol.nlp_grad(problem_nlp.oracle_cfg(cfg), x, p, 1.0, lam)
    L = cm.Layout(N)
    cols = [3 * (N + 1) * (i // 3) + i % 3 for i in range(9)] + [9 * (N + 1) + c * (18 * N + 3) + a for c in range(2) for a in range(3)]
    lam[:15] = -gx[cols]
    assert L.ng == lam.size
    return lam


def host_kkt(cfg, x, p, lam):
    """the fields of cmpc_kkt_certificate_device in float64 (kkt_report of tests/golden/make_argmin_ref_golden.py)"""
    ol, problem_nlp = _ol()
    oc = problem_nlp.oracle_cfg(cfg)
    lb, ub = problem_nlp.bounds(cfg, p)
    f, g = ol.nlp_fg(oc, x, p)
    gx, _ = ol.nlp_grad(oc, x, p, 1.0, lam)
    scale = max(1.0, np.abs(lam).max())
    ineq = ub - lb > 1e-12
    dist = np.minimum(g - lb, ub - g)
    up = np.where(lb < -1e19, True, np.where(ub > 1e19, False, (ub - g) < (g - lb)))
    wrong = np.where(up, -lam, lam)
    return dict(stat=np.abs(gx).max() / scale, feas=max(np.maximum(lb - g, 0).max(), np.maximum(g - ub, 0).max()),
                compl=np.abs(lam[ineq] * dist[ineq]).max() / scale, sign=max(wrong[ineq].max(), 0.0) / scale, f=f, scale=scale,
                stat_abs=np.abs(gx).max())


def value_gradient(cfg, x, p, lam):
    """dV*/dp = grad_p L(x, lam) + the bound-only parameters' terms (cmpc_value_gradient_device)"""
    ol, problem_nlp = _ol()
    N = cfg.N
    _, gp = ol.nlp_grad(problem_nlp.oracle_cfg(cfg), x, p, 1.0, lam)
    gp = gp.copy()
    o = rows(N)
    per = 19 * N + 6
    gp[2 * per:2 * per + 9] = -lam[:9]
    for c in range(2):
        lb = lam[o["bbox"][c]:o["bbox"][c] + 3 * N]
        gp[c * per + 9 * N:c * per + 12 * N] = -np.maximum(lb, 0)
        gp[c * per + 12 * N:c * per + 15 * N] = -np.minimum(lb, 0)
        gp[c * per + 19 * N + 3:c * per + 19 * N + 6] = -lam[9 + 3 * c:12 + 3 * c]
    return gp


def unique_rows(N):
    """rows whose multiplier is unique at a KKT point: the initial-condition rows of com, dcom, h and the com / dcom / h dynamics.  Not the feet's
    initial-condition rows: a foot in stance from stage 0 has box rows R^T (pos_k+1 - nom) that the dynamics make duplicates of its initial row, and the
    goldens spread thousands on them where the convention puts everything on the foot's position rows (argmin_ref_walk_tmp, problem 0: 3.5e3)."""
    return np.concatenate([np.arange(0, 9), np.arange(15, 15 + 9 * N)])


def zero_rows(N, p):
    """rows the convention sets to exactly 0: g_pos of swing stages, g_bbox of stance stages"""
    o = rows(N)
    z = []
    for c in range(2):
        g = _gam(N, p, c)
        for k in range(N):
            base = o["pos"][c] if g[k] < 0.5 else o["bbox"][c]
            z += [base + 3 * k + i for i in range(3)]
    return np.array(z)


GOLDEN_REF = [(n, w) for n in ("walk", "yaw", "push", "ssend", "stand") for w in ("tmp", "jit")]


def golden_cfg(name, which=None):
    if which is not None:
        return cm.config.generated_code_weights(which, 12, 0.1)
    return {"cfg1": cm.synthetic.config1_plumbing, "cfg2": lambda: cm.synthetic.config2_perturbed_com(8),
            "cfg3": lambda: cm.synthetic.config3_external_push(8), "cfg5": lambda: cm.synthetic.config5_footstep_candidates(4)}[name]()[0]


@pytest.mark.parametrize("name,which", GOLDEN_REF + [(n, None) for n in ("cfg2", "cfg3", "cfg5")])
def test_row_mapping_reproduces_the_goldens_multipliers(name, which, golden_dir):
    """record_from_lam -> map_record at the goldens' (x*, lam*): the unique rows come back (the init rows through stationarity, nlp_grad), the
    convention's rows are exactly 0, and the mapped lam_g is a KKT point of the reference NLP as good as the golden's own."""
    d = np.load(os.path.join(golden_dir, f"argmin_ref_{name}_{which}.npz" if which else f"argmin_{name}.npz"))
    cfg = golden_cfg(name, which)
    N = cfg.N
    worst = dict(unique=0.0, stat=0.0, compl=0.0, sign=0.0)
    for b in range(d["P"].shape[0]):
        x, p, lam = (d[k][b].astype(np.float64) for k in ("x_star", "P", "lam_g"))
        S, Z = record_from_lam(cfg, x, p, lam)
        lm = map_record(cfg, x, p, S, Z)
        u = unique_rows(N)
        assert (lm[zero_rows(N, p)] == 0).all()
        k1 = host_kkt(cfg, x, p, lm)
        # (unique rows relative to their own largest entry: the goldens' duplicate box rows carry thousands, which must not loosen this)
        worst["unique"] = max(worst["unique"], np.abs(lm[u] - lam[u]).max() / max(1.0, np.abs(lam[u]).max()))
        for f in ("stat", "compl", "sign"):
            worst[f] = max(worst[f], k1[f])
    print(f"\n{name} {which}: " + " ".join(f"{f} {v:.1e}" for f, v in worst.items()))
    # measured worst over the 13 goldens: unique rows 3.1e-11 (cfg2), stationarity 1.1e-9 (yaw tmp), complementarity 1.5e-11 (stand), sign 7.2e-16
    # (yaw jit).  The goldens' own certificate: stationarity < 1e-7, complementarity < 1e-6 (tests/golden/make_argmin_ref_golden.py)
    assert worst["unique"] <= 1e-9 and worst["stat"] <= 1e-8 and worst["compl"] <= 1e-9 and worst["sign"] <= 1e-12, worst


def _active_box_entries(cfg, p, lam):
    """the most strongly active upper and lower bound (|lam| > 0.05) of a free landing-offset component in a swing stage, each with the same bound of
    the stance stages behind it, which subset rule 3 keeps bit-equal to it (one parameter of the NLP: perturbed together)"""
    N = cfg.N
    per, o = 19 * N + 6, rows(N)
    out = []
    for side in ("upper", "lower"):
        best = None
        for c in range(2):
            lo, up = _box(N, p, c)
            g = _gam(N, p, c)
            for k in range(N):
                for i in range(3):
                    v = lam[o["bbox"][c] + 3 * k + i]
                    if g[k] < 0.5 and up[k, i] - lo[k, i] > 1e-6 and (v > 0.05 if side == "upper" else v < -0.05):
                        if best is None or abs(v) > best[0]:
                            best = (abs(v), c, k, i)
        if best is not None:
            _, c, k, i = best
            g = _gam(N, p, c)
            q0 = c * per + (9 * N if side == "upper" else 12 * N) + 3 * k + i
            qs = [q0]
            while k + len(qs) < N and g[k + len(qs)] >= 0.5:
                assert p[q0 + 3 * len(qs)] == p[q0]
                qs.append(q0 + 3 * len(qs))
            out.append((side, qs))
    return out


def _current_entries(cfg, p, h):
    """currentPos components whose perturbation by +-h keeps every stance-from-stage-0 box row inside its bounds (subset rule 2)"""
    N = cfg.N
    per = 19 * N + 6
    out = []
    for c in range(2):
        lo, up = _box(N, p, c)
        g = _gam(N, p, c)
        cur, nom = p[c * per + 19 * N + 3:c * per + 19 * N + 6], p[c * per + 16 * N:c * per + 19 * N + 3].reshape(N + 1, 3)
        for a in range(3):
            ok = True
            for k in range(N):
                if g[k] < 0.5:
                    break
                for sgn in (1, -1):
                    v = _R(N, p, c, k).T @ (cur + sgn * h * np.eye(3)[a] - nom[k + 1])
                    ok &= bool(((v >= lo[k] - 1e-6) & (v <= up[k] + 1e-6)).all())
            if ok:
                out.append(("currentPos", [c * per + 19 * N + 3 + a]))
    return out


# (golden, problems, the bound-only kinds the case must reach)
FD_CASES = [("cfg2", None, (0, 1), {"currentPos"}), ("cfg5", None, (0, 2), {"lower", "currentPos"}), ("yaw", "tmp", (4, 13), {"upper", "lower"})]


@pytest.mark.parametrize("name,which,problems,kinds", FD_CASES)
def test_value_gradient_matches_finite_differences_of_the_oracle(name, which, problems, kinds, golden_dir):
    """dV*/dp of the host formula at the golden's (x*, lam* in the convention) against central differences of V*(p) = f(x*(p), p) from the float64
    oracle solve (tolerance 1e-9): com0, dcom0, h0, a comRef and an hRef entry, a nominalPos entry, an fExt entry; the most active upper and lower box
    entry of a swing stage (with its stance duplicates); the currentPos entries that stay inside the supported subset.  Each case must reach the
    bound-only kinds it names (over the three: upper, lower, currentPos).  (Weakly active box rows, |lam| ~ 1e-3 with the bound binding on one side only, are
    kinks of V*: no central difference measures their one-sided slopes -- hence |lam| > 0.05.)"""
    ol, problem_nlp = _ol()
    d = np.load(os.path.join(golden_dir, f"argmin_ref_{name}_{which}.npz" if which else f"argmin_{name}.npz"))
    cfg = golden_cfg(name, which)
    N = cfg.N
    oc = problem_nlp.oracle_cfg(cfg)
    per = 19 * N + 6
    worst = {}
    for b in problems:
        x, p, lam = (d[k][b].astype(np.float64) for k in ("x_star", "P", "lam_g"))
        lam = map_record(cfg, x, p, *record_from_lam(cfg, x, p, lam))   # (the convention: the golden spreads some multipliers over duplicate rows)
        gp = value_gradient(cfg, x, p, lam)
        t0 = 2 * per
        params = [("com0", [t0 + 0]), ("com0", [t0 + 2]), ("dcom0", [t0 + 3]), ("dcom0", [t0 + 5]), ("h0", [t0 + 7]), ("comRef", [t0 + 9 + 3 * 5 + 2]),
                  ("hRef", [t0 + 9 + 3 * (N + 1) + 3 * 4 + 1]), ("fExt", [t0 + 9 + 6 * (N + 1) + 3 * 2]), ("nominalPos", [16 * N + 1])]
        params += _active_box_entries(cfg, p, lam) + _current_entries(cfg, p, 1e-4)
        X0 = np.repeat(x[None], 2, 0)
        for kind, q in params:
            h = 1e-4 * max(1.0, abs(p[q[0]]))
            Pp = np.repeat(p[None], 2, 0)
            Pp[0, q] += h
            Pp[1, q] -= h
            Xs, info = ol.ref_solve_batch(oc, Pp, X0, ol.ipm_opts(tol=1e-9, mu_min=1e-10), nthreads=2)
            assert (info[:, 5] == 0).all(), (name, b, kind, q, info[:, 5])
            V = [ol.nlp_fg(oc, Xs[i], Pp[i])[0] for i in range(2)]
            fd = (V[0] - V[1]) / (2 * h)
            an = gp[q].sum()
            gap = abs(fd - an) / max(1.0, abs(an))
            worst[kind] = max(worst.get(kind, 0.0), gap)
            # measured worst: 1.1e-6 (lower, cfg5 problem 2; upper, yaw 4), 4.3e-7 (currentPos, cfg2), 7.3e-8 (the others)
            assert gap <= 1e-5, (name, b, kind, q, fd, an)
    print(f"\n{name} {which}: FD gap " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert kinds <= set(worst), (kinds, worst)
