"""Float64 dense restatement of the solution sensitivities of include/cmpc.h (cmpc_solution_jvp_device / cmpc_solution_vjp_device), built on the
oracle's nlp_grad / nlp_jac / nlp_hess and problem_nlp.bounds.  One problem at a time, the full x layout minus the stance vel columns, the symmetric
system of the header solved densely:

    [ W    J_E^T ] [ dx    ]      [ d_p(grad_x L) dp + sum_I J_i^T Sigma_i (d_p g_i dp - db_i) ]
    [ J_E  0     ] [ dlam_E] = -  [ d_p g_E dp - db_E                                          ]

Every covered parameter enters grad_x L, g and the bounds linearly, so the p-derivatives are differences of the oracle's functions at p + dp and p
(exact up to rounding).  Test infrastructure: no GPU; tests/test_sensitivity_cpu.py holds it to finite differences of the float64 oracle and
tests/test_gpu_sensitivity.py holds the device kernels to it."""
import numpy as np

import cmpc_amd as cm

S_MIN = 5e-8      # CMPC_SENS_SMIN
WEAK = 1e-3       # CMPC_SENS_WEAK


def _ol():
    from oracle import oracle_lib as ol, problem_nlp
    return ol, problem_nlp


def covered_mask(N):
    """1 on the parameters the map covers (com0, dcom0, h0, currentPos, comRef, hRef, nominalPos, box upper / lower, fExt, tauExt), 0 on R, Gamma"""
    L = cm.Layout(N)
    m = np.ones(L.np)
    for c in range(2):
        m[L.p_R[c]:L.p_R[c] + 9 * N] = 0
        m[L.p_gam[c]:L.p_gam[c] + N] = 0
    return m


class Sens:
    """the factorised system of one problem at (x, p, lam_g); s_min: the slack floor"""

    def __init__(self, cfg, x, p, lam, s_min=S_MIN):
        ol, problem_nlp = _ol()
        self.cfg, self.N = cfg, cfg.N
        N = self.N
        self.oc = problem_nlp.oracle_cfg(cfg)
        self.x, self.p, self.lam = (np.asarray(a, np.float64) for a in (x, p, lam))
        L = self.L = cm.Layout(N)
        nx, ng = L.nx, 53 * N + 15
        gam = [self.p[L.p_gam[c]:L.p_gam[c] + N] for c in range(2)]
        # kept columns: everything but the vel of stance stages
        keep = np.ones(nx, bool)
        for c in range(2):
            for k in range(N):
                if gam[c][k] >= 0.5:
                    keep[L.vel[c] + 3 * k:L.vel[c] + 3 * k + 3] = False
        self.keep = np.nonzero(keep)[0]
        # rows
        o_box = [15 + 15 * N + c * 19 * N for c in range(2)]
        o_fric = [o_box[c] + 3 * N for c in range(2)]
        eq = list(range(15 + 15 * N))
        self.fric = np.concatenate([np.arange(o_fric[c], o_fric[c] + 16 * N) for c in range(2)])
        free = []
        for c in range(2):
            lo = self.p[L.p_lo[c]:L.p_lo[c] + 3 * N]
            up = self.p[L.p_up[c]:L.p_up[c] + 3 * N]
            for k in range(N):
                if gam[c][k] >= 0.5:
                    continue
                for i in range(3):
                    r = o_box[c] + 3 * k + i
                    if np.float32(up[3 * k + i]) - np.float32(lo[3 * k + i]) > np.float32(1e-9):
                        free.append(r)
                    else:
                        eq.append(r)
        self.eq, self.free = np.array(eq), np.array(free, int)
        self.fixed = np.array([r for r in eq if r >= 15 + 15 * N], int)
        # g, bounds, J, Hessian of L
        _, self.g = ol.nlp_fg(self.oc, self.x, self.p)
        self.lb, self.ub = problem_nlp.bounds(cfg, self.p)
        jr, jc, jv = ol.nlp_jac(self.oc, self.x, self.p)
        J = np.zeros((ng, nx))
        np.add.at(J, (jr, jc), jv)
        hr, hc, hv = ol.nlp_hess(self.oc, self.x, self.p, 1.0, self.lam)
        H = np.zeros((nx, nx))
        np.add.at(H, (hr, hc), hv)
        if not (np.any(hr < hc) and np.any(hr > hc)):      # one triangle stored
            H = H + H.T - np.diag(np.diag(H))
        self.J = J
        # Sigma of every inequality side
        lam = self.lam
        zf = np.maximum(lam[self.fric], 0)
        sf = -self.g[self.fric]
        self.sig_f = zf / np.maximum(sf, s_min)
        zU, zL = np.maximum(lam[self.free], 0), np.maximum(-lam[self.free], 0)
        sU, sL = self.ub[self.free] - self.g[self.free], self.g[self.free] - self.lb[self.free]
        self.sig_u, self.sig_l = zU / np.maximum(sU, s_min), zL / np.maximum(sL, s_min)
        # weakly active rows: friction rows of loaded feet (stance stages) and box sides; those of swing feet apart (include/cmpc.h, dSens[5])
        stance = np.concatenate([np.repeat(gam[c] >= 0.5, 16) for c in range(2)])
        wf = (zf < WEAK) & (sf < WEAK)
        self.weak = int(np.sum(wf & stance) + np.sum((zU < WEAK) & (sU < WEAK)) + np.sum((zL < WEAK) & (sL < WEAK)))
        self.weak_swing = int(np.sum(wf & ~stance))
        self.sigmax = float(max(self.sig_f.max(initial=0), self.sig_u.max(initial=0), self.sig_l.max(initial=0)))
        W = H.copy()
        Jf, Jb = J[self.fric], J[self.free]
        self.JfT, self.JbT = np.ascontiguousarray(Jf.T), np.ascontiguousarray(Jb.T)   # (rhs runs once per parameter in vjp: not sliced out of J every call)
        W += Jf.T @ (self.sig_f[:, None] * Jf) + Jb.T @ ((self.sig_u + self.sig_l)[:, None] * Jb)
        JE = J[self.eq][:, self.keep]
        nk, ne = self.keep.size, self.eq.size
        K = np.zeros((nk + ne, nk + ne))
        K[:nk, :nk] = W[np.ix_(self.keep, self.keep)]
        K[:nk, nk:] = JE.T
        K[nk:, :nk] = JE
        self.K = K
        self.nk = nk
        from tests import parity
        self.n = parity._internal_force_direction(L, self.p)
        self.gx0, _ = ol.nlp_grad(self.oc, self.x, self.p, 1.0, self.lam)

    def rhs(self, dp):
        """r(dp) of the system (without the leading minus), kept columns then E rows"""
        ol, problem_nlp = _ol()
        dp = np.asarray(dp, np.float64) * covered_mask(self.N)
        p1 = self.p + dp
        gx1, _ = ol.nlp_grad(self.oc, self.x, p1, 1.0, self.lam)
        _, g1 = ol.nlp_fg(self.oc, self.x, p1)
        lb1, ub1 = problem_nlp.bounds(self.cfg, p1)
        dg, dlb, dub = g1 - self.g, lb1 - self.lb, ub1 - self.ub
        rx = gx1 - self.gx0
        rx = rx + self.JfT @ (self.sig_f * dg[self.fric])
        rx = rx + self.JbT @ (self.sig_u * (dg[self.free] - dub[self.free]) + self.sig_l * (dg[self.free] - dlb[self.free]))
        db = 0.5 * (dlb + dub)
        rE = dg[self.eq] - db[self.eq]
        return np.concatenate([rx[self.keep], rE])

    def _solve(self, b):
        """dense solve with one step of iterative refinement (b a vector or a matrix of columns); K is factorised once"""
        from scipy.linalg import lu_factor, lu_solve
        if getattr(self, "_lu", None) is None:
            self._lu = lu_factor(self.K)
        y = lu_solve(self._lu, b)
        return y + lu_solve(self._lu, b - self.K @ y)

    def _full(self, d):
        out = np.zeros(self.L.nx)
        out[self.keep] = d[:self.nk]
        return out

    def jvp(self, dp):
        dx = self._full(self._solve(-self.rhs(dp)))
        if self.n is not None:
            dx = dx - self.n * (self.n @ dx)
        return dx

    def vjp(self, v, idx=None):
        """idx: the entries of p to compute (the others stay 0); None: every covered one"""
        v = np.asarray(v, np.float64)
        if self.n is not None:
            v = v - self.n * (self.n @ v)
        w = self._solve(np.concatenate([v[self.keep], np.zeros(self.eq.size)]))
        m = covered_mask(self.N)
        out = np.zeros(self.L.np)
        for j in (np.nonzero(m)[0] if idx is None else [j for j in idx if m[j]]):
            e = np.zeros(self.L.np)
            e[j] = 1.0
            out[j] = -w @ self.rhs(e)
        return out


def directions(cfg, p, lam):
    """[(name, dp)]: unit perturbations of com0, dcom0, h0, comRef, hRef, fExt, tauExt, a nominalPos group (a swing landing's nominal with the
    stance knots behind it), the most active upper and lower swing box groups, and the currentPos entries that stay in the subset"""
    from tests.test_multipliers_cpu import _active_box_entries, _current_entries
    N = cfg.N
    L = cm.Layout(N)
    out = []

    def unit(idx):
        d = np.zeros(L.np)
        d[idx] = 1.0
        return d
    out += [("com0", unit([L.p_com0 + 0])), ("com0", unit([L.p_com0 + 2])), ("dcom0", unit([L.p_dcom0 + 1])), ("h0", unit([L.p_h0 + 0])),
            ("comRef", unit([L.p_comref + 3 * 5 + 2])), ("hRef", unit([L.p_href + 3 * 4 + 1])), ("fExt", unit([L.p_fext + 3 * 2])),
            ("tauExt", unit([L.p_text + 3 * 1 + 1]))]
    # a nominalPos group: the knot after foot c's first swing stage with the stance knots that repeat it (rule 3), else one knot
    for c in range(2):
        gam = p[L.p_gam[c]:L.p_gam[c] + N]
        sw = [k for k in range(N) if gam[k] < 0.5]
        if sw:
            k = sw[-1] if sw[-1] + 1 < N else sw[0]
            idx = [L.p_nom[c] + 3 * (k + 1)]
            j = k + 1
            while j < N and gam[j] >= 0.5:
                idx.append(L.p_nom[c] + 3 * (j + 1))
                j += 1
            out.append(("nominalPos", unit(idx)))
            break
    else:
        out.append(("nominalPos", unit([L.p_nom[0] + 3 * 3])))
    for side, qs in _active_box_entries(cfg, p, lam):
        out.append((side, unit(qs)))
    out += [(kind, unit(q)) for kind, q in _current_entries(cfg, p, 1e-4)]
    return out
