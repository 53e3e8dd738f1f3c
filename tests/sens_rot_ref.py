"""Float64 dense restatement of the rotation directions of include/cmpc.h (cmpc_solution_jvp_rot_device, cmpc_solution_vjp_rot_device,
cmpc_rotation_value_gradient_device, cmpc_contacts_rotation_vjp_device), composed on top of tests/sens_ref.Sens and tests/sens_model_ref.ModelSens
(the same system, Sigma, rows and solve):

    r_x = d_omega(grad_x L) omega + sum_I J_i^T Sigma_i d_omega g_i omega,     r_E = d_omega g_E omega

omega[2][N][3] moves the rotation of foot c at stage k along dR = R [omega_{c,k}]x (the right, body-frame tangent), R the matrix as stored in p.
Every term of the NLP is linear in the entries of R, so the omega-derivatives are central differences of the oracle's nlp_grad / nlp_fg along
dp_R = vec(R [omega]x) (exact up to rounding).  No bound depends on R.  In double support over the whole horizon the right-hand side loses its
component along the internal-force direction n before the solve; the removed relative size |n^T r_x| / |r_x| is what the kernel reports in dSens[6].

Stiff rows.  A rotation moves the box rows of swing stages, R^T (pos - nominalPos), directly.  Where such a row is active its Sigma is z / s_min (3e8
at the default floor) and the condensed right-hand side J_i^T Sigma_i d g_i reaches 1e5 .. 1e7, which the solution cancels to order one: in float64
<v, J u> and <J^T v, u> then agree to 1e-9 only, whatever the solver.  The rows with Sigma above STIFF are therefore kept out of the condensation:
with t_i = Sigma_i (J_i dx + d g_i) as an unknown of its own,

    [ W'   J_E^T  J_T^T      ] [ dx     ]      [ r_x' ]         W', r_x': W and r_x without the rows T
    [ J_E  0      0          ] [ dlam_E ] = -  [ r_E  ]
    [ J_T  0      -Sigma_T^-1] [ t      ]      [ dg_T ]

is the same linear system (eliminate t), and nothing in it is large.  Test infrastructure: no GPU."""
import numpy as np

import cmpc_amd as cm
from tests import sens_model_ref as smr
from tests import sens_ref

STIFF = 1e3   # rows with a larger Sigma stay out of the condensation (see above)


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def expm(w):
    """Rodrigues: exp([w]x)"""
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    if t < 1e-300:
        return np.eye(3)
    K = skew(w / t)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def stage_R(L, p, c, k):
    """R_{c,k} as stored in p (column-major 3x3 at p_R[c] + 9 k)"""
    return np.asarray(p[L.p_R[c] + 9 * k:L.p_R[c] + 9 * k + 9], np.float64).reshape(3, 3).T


def dp_rot(N, p, omega):
    """the direction of p that moves every R_{c,k} along R [omega_{c,k}]x"""
    L = cm.Layout(N)
    omega = np.asarray(omega, np.float64).reshape(2, N, 3)
    dp = np.zeros(L.np)
    for c in range(2):
        for k in range(N):
            if omega[c, k].any():
                dp[L.p_R[c] + 9 * k:L.p_R[c] + 9 * k + 9] = (stage_R(L, p, c, k) @ skew(omega[c, k])).T.reshape(9)
    return dp


def p_rotated(N, p, omega, dtype=np.float64):
    """p with every R_{c,k} replaced by R_{c,k} exp([omega_{c,k}]x)"""
    L = cm.Layout(N)
    omega = np.asarray(omega, np.float64).reshape(2, N, 3)
    out = np.array(p, dtype)
    for c in range(2):
        for k in range(N):
            if omega[c, k].any():
                out[L.p_R[c] + 9 * k:L.p_R[c] + 9 * k + 9] = (stage_R(L, p, c, k) @ expm(omega[c, k])).T.reshape(9)
    return out


def groups(N, p):
    """[(c, [stages])]: per foot, the maximal runs of consecutive stages with the same stored R (a landing's swing stages and the stance stages that
    repeat them: subset rule 3)"""
    L = cm.Layout(N)
    out = []
    for c in range(2):
        run = [0]
        for k in range(1, N):
            if np.array_equal(p[L.p_R[c] + 9 * k:L.p_R[c] + 9 * k + 9], p[L.p_R[c] + 9 * (k - 1):L.p_R[c] + 9 * k]):
                run.append(k)
            else:
                out.append((c, run))
                run = [k]
        out.append((c, run))
    return out


def rot_directions(N, p):
    """[(name, omega[2][N][3], has_swing)]: for each foot, each group of stages with equal R along e_z and along a general unit axis, and the whole
    foot along both"""
    L = cm.Layout(N)
    gen = np.array([0.36, -0.48, 0.8])
    out = []
    gs = groups(N, p)
    for c, ks in gs + [(c, list(range(N))) for c in range(2) if (c, list(range(N))) not in gs]:
        swing = bool(np.any(p[L.p_gam[c] + np.array(ks)] < 0.5))
        for nm, w in (("z", np.array([0.0, 0.0, 1.0])), ("gen", gen)):
            om = np.zeros((2, N, 3))
            om[c, ks] = w
            out.append((f"foot{c}[{ks[0]}..{ks[-1]}]{nm}", om, swing))
    return out


class RotSens:
    """the rotation directions of one problem at (x, p, lam_g) (and model theta: default cfg's own)"""

    def __init__(self, cfg, x, p, lam, theta=None, s_min=sens_ref.S_MIN):
        self.MS = smr.ModelSens(cfg, x, p, lam, theta=theta, s_min=s_min)
        self.S = self.MS.S
        self.n, self.N = self.S.n, cfg.N

    def _diff(self, omega):
        from oracle import oracle_lib as ol
        S = self.S
        om = np.asarray(omega, np.float64)
        h = 1.0 / max(np.abs(om).max(), 1e-300)   # (a rotation of order one: exact for a linear function, least cancellation)
        dp = dp_rot(self.N, S.p, h * om)
        gx1, _ = ol.nlp_grad(S.oc, S.x, S.p + dp, 1.0, S.lam)
        gx0, _ = ol.nlp_grad(S.oc, S.x, S.p - dp, 1.0, S.lam)
        _, g1 = ol.nlp_fg(S.oc, S.x, S.p + dp)
        _, g0 = ol.nlp_fg(S.oc, S.x, S.p - dp)
        return (g1 - g0) / (2 * h), (gx1 - gx0) / (2 * h)

    def _stiff(self):
        """(rows T, Sigma_T, the factorised un-condensed system), built once"""
        if getattr(self, "_aug", None) is None:
            from scipy.linalg import lu_factor
            S = self.S
            rows = np.concatenate([S.fric, S.free])
            sig = np.concatenate([S.sig_f, S.sig_u + S.sig_l])
            T = sig > STIFF
            JT = S.J[rows[T]][:, S.keep]
            n0, nt = S.K.shape[0], int(T.sum())
            K = np.zeros((n0 + nt, n0 + nt))
            K[:n0, :n0] = S.K
            K[:S.nk, :S.nk] -= JT.T @ (sig[T][:, None] * JT)
            K[:S.nk, n0:] = JT.T
            K[n0:, :S.nk] = JT
            K[n0:, n0:] = -np.diag(1.0 / sig[T])
            self._aug = (rows[T], sig[T], K, lu_factor(K))
        return self._aug

    def _solve(self, b, bT=None):
        """the solve of sens_ref.Sens for the condensed right-hand side b plus J_T^T Sigma_T bT, through the un-condensed system"""
        from scipy.linalg import lu_solve
        _, _, K, lu = self._stiff()
        rhs = np.concatenate([b, np.zeros(K.shape[0] - b.size) if bT is None else bT])
        y = lu_solve(lu, rhs)
        y = y + lu_solve(lu, rhs - K @ y)
        return y

    def rhs_parts(self, omega, split=False):
        """(r_x in the full x layout, r_E) of a rotation direction, before the projection; split: the rows T's share J_T^T Sigma_T dg_T is left
        out of r_x and dg_T is returned as well"""
        S = self.S
        dg, rx = self._diff(omega)
        sf, sb = S.sig_f.copy(), S.sig_u + S.sig_l
        if split:
            sf[sf > STIFF] = 0.0
            sb[sb > STIFF] = 0.0
        rx = rx + S.J[S.fric].T @ (sf * dg[S.fric])
        rx = rx + S.J[S.free].T @ (sb * dg[S.free])
        return (rx, dg[S.eq], dg[self._stiff()[0]]) if split else (rx, dg[S.eq])

    def removed(self, omega):
        """|n^T r_x| / |r_x| of a rotation direction (0 without the internal-force direction)"""
        if self.n is None:
            return 0.0
        rx, _ = self.rhs_parts(omega)
        nr = np.linalg.norm(rx[self.S.keep])
        return float(abs(self.n @ rx) / nr) if nr > 0 else 0.0

    def rhs(self, omega):
        """(r(omega) of the system without the rows T's share, kept columns then E rows, with no component of the whole r_x along n;  dg_T)"""
        rx, rE, dgT = self.rhs_parts(omega, split=True)
        if self.n is not None:
            rx = rx - self.n * (self.n @ self.rhs_parts(omega)[0])
        return np.concatenate([rx[self.S.keep], rE]), dgT

    def jvp(self, omega, dtheta=None, dp=None):
        S = self.S
        b, dgT = self.rhs(omega)
        if dtheta is not None:
            b = b + self.MS.rhs(dtheta)
        if dp is not None:
            b = b + S.rhs(dp)
        dx = S._full(self._solve(-b, -dgT))
        if self.n is not None:
            dx = dx - self.n * (self.n @ dx)
        return dx

    def _units(self):
        for c in range(2):
            for k in range(self.N):
                for a in range(3):
                    om = np.zeros((2, self.N, 3))
                    om[c, k, a] = 1.0
                    yield (c, k, a), om

    def vjp(self, v):
        """dl/domega [2][N][3] = -w^T r_omega, w the solution of [v; 0] with v's component along n removed"""
        S = self.S
        v = np.asarray(v, np.float64)
        if self.n is not None:
            v = v - self.n * (self.n @ v)
        w = self._solve(np.concatenate([v[S.keep], np.zeros(S.eq.size)]))
        n0 = S.K.shape[0]
        out = np.zeros((2, self.N, 3))
        for i, om in self._units():
            b, dgT = self.rhs(om)
            out[i] = -(w[:n0] @ b + w[n0:] @ dgT)
        return out

    def removed_vjp(self):
        """dSens[6] of the VJP's rotation part: the largest removed relative size over the 6 N entries"""
        return max(self.removed(om) for _, om in self._units()) if self.n is not None else 0.0

    def value_gradient(self):
        """dV*/domega [2][N][3] = lam^T d_omega g at (x, lam) (f does not depend on R)"""
        out = np.zeros((2, self.N, 3))
        for i, om in self._units():
            dg, _ = self._diff(om)
            out[i] = self.S.lam @ dg
        return out


def stage_owner(N, dt, now, t, n):
    """cmpc_contacts_sample's owner of every stage for one foot's list t[n][2] (activation, deactivation): the active contact, else the next, else
    the last; -1 when the list is empty"""
    own = np.full(N, -1)
    for k in range(N):
        tk = now + k * dt + cm.contacts.TIME_EPS
        act = [m for m in range(n) if t[m, 0] <= tk < t[m, 1]]
        nxt = [m for m in range(n) if t[m, 0] > tk]
        own[k] = act[0] if act else nxt[0] if nxt else n - 1
    return own


def list_sum(g_rot, owners, n, max_contacts):
    """per-stage -> per-list-entry, one foot: out[m] = the sum over the stages k that entry m owns of g_rot[k], in stage order; entries at or beyond
    n carry none; a foot that sampling would not sample (n == 0 or n > max_contacts) gets zeros"""
    out = np.zeros((max_contacts, 3))
    if n < 1 or n > max_contacts:
        return out
    for k, m in enumerate(owners):
        if 0 <= m < n:
            out[m] += g_rot[k]
    return out
