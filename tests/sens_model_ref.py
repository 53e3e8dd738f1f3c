"""Float64 dense restatement of the model directions of include/cmpc.h (cmpc_solution_jvp_model_device, cmpc_solution_vjp_model_device,
cmpc_model_value_gradient_device), composed on top of tests/sens_ref.Sens (the same system, Sigma, rows and solve):

    r_x = d_theta(grad_x L) dtheta + sum_I J_i^T Sigma_i d_theta g_i dtheta,     r_E = d_theta g_E dtheta

theta is the 34 doubles of cmpc_model in its field order.  Every field enters grad_x L and g at most quadratically (com_weight[2] through
w_z(k)^2, the rest linearly), so the theta-derivatives are central differences of the oracle's nlp_grad / nlp_fg at theta +- dtheta (exact up to
rounding).  In double support over the whole horizon the right-hand side loses its component along the internal-force direction n before the solve;
the removed relative size |n^T r_x| / |r_x| is what the kernel reports in dSens[6].  Test infrastructure: no GPU."""
import copy

import numpy as np

import cmpc_amd as cm
from tests import sens_ref

M = 34   # CMPC_MODEL_DOUBLES
FIELDS = (["friction", "com_weight_x", "com_weight_y", "com_weight_z", "angular_momentum", "contact_position", "force_rate_x", "force_rate_y",
           "force_rate_z", "symmetry"] + [f"corner_{c}{j}{'xyz'[b]}" for c in range(2) for j in range(4) for b in range(3)])


def corner_index(c, j, b):
    return 10 + 12 * c + 3 * j + b


def theta_of(cfg):
    """the 34 doubles of a configuration's model (config.model_row)"""
    return cm.config.model_row(cfg)


def nlp_cfg(cfg, theta):
    """the oracle's NlpCfg of configuration cfg (horizon, sampling time) with model theta"""
    from oracle import oracle_lib as ol
    th = np.asarray(theta, np.float64)
    return ol.make_cfg(cfg.N, cfg.sampling_time, mu=th[0], w_com=th[1:4], w_h=th[4], w_pos=th[5], w_rate=th[6:9], w_sym=th[9],
                       corners=th[10:34].reshape(2, 4, 3))


def cfg_with_model(cfg, theta):
    """a copy of cfg whose model fields are theta (sens_ref.Sens builds its oracle configuration from the package configuration)"""
    th = np.asarray(theta, np.float64)
    out = copy.deepcopy(cfg)
    out.static_friction_coefficient = float(th[0])
    out.com_weight = tuple(float(v) for v in th[1:4])
    out.angular_momentum_weight, out.contact_position_weight = float(th[4]), float(th[5])
    out.force_rate_of_change_weight = tuple(float(v) for v in th[6:9])
    out.contact_force_symmetry_weight = float(th[9])
    for c in range(2):
        out.contacts[c].corners = [tuple(float(v) for v in th[10 + 12 * c + 3 * j:13 + 12 * c + 3 * j]) for j in range(4)]
    return out


class ModelSens:
    """the model directions of one problem at (x, p, lam_g) and model theta (default: cfg's own)"""

    def __init__(self, cfg, x, p, lam, theta=None, s_min=sens_ref.S_MIN):
        self.theta = theta_of(cfg) if theta is None else np.asarray(theta, np.float64)
        self.cfg = cfg_with_model(cfg, self.theta)
        self.S = sens_ref.Sens(self.cfg, x, p, lam, s_min=s_min)
        self.n = self.S.n

    def _eval(self, theta):
        from oracle import oracle_lib as ol
        S = self.S
        oc = nlp_cfg(self.cfg, theta)
        gx, _ = ol.nlp_grad(oc, S.x, S.p, 1.0, S.lam)
        f, g = ol.nlp_fg(oc, S.x, S.p)
        return f, g, gx

    def _diff(self, dtheta):
        d = np.asarray(dtheta, np.float64)
        h = 1.0 / max(np.abs(d).max(), 1e-300)   # (a step of order one in the largest field: exact for quadratics, least cancellation)
        f1, g1, gx1 = self._eval(self.theta + h * d)
        f0, g0, gx0 = self._eval(self.theta - h * d)
        return (f1 - f0) / (2 * h), (g1 - g0) / (2 * h), (gx1 - gx0) / (2 * h)

    def rhs_parts(self, dtheta):
        """(r_x in the full x layout, r_E) of a model direction, before the projection"""
        S = self.S
        _, dg, rx = self._diff(dtheta)
        rx = rx + S.J[S.fric].T @ (S.sig_f * dg[S.fric])
        rx = rx + S.J[S.free].T @ ((S.sig_u + S.sig_l) * dg[S.free])   # (no model field enters the box rows: zero)
        return rx, dg[S.eq]

    def removed(self, dtheta):
        """|n^T r_x| / |r_x| of a model direction (0 without the internal-force direction)"""
        if self.n is None:
            return 0.0
        rx, _ = self.rhs_parts(dtheta)
        nr = np.linalg.norm(rx[self.S.keep])
        return float(abs(self.n @ rx) / nr) if nr > 0 else 0.0

    def rhs(self, dtheta):
        """r(dtheta) of the system (kept columns then E rows), with no component along n"""
        rx, rE = self.rhs_parts(dtheta)
        if self.n is not None:
            rx = rx - self.n * (self.n @ rx)
        return np.concatenate([rx[self.S.keep], rE])

    def jvp(self, dtheta, dp=None):
        S = self.S
        b = self.rhs(dtheta)
        if dp is not None:
            b = b + S.rhs(dp)
        dx = S._full(S._solve(-b))
        if self.n is not None:
            dx = dx - self.n * (self.n @ dx)
        return dx

    def vjp(self, v):
        """dl/dtheta [34] = -w^T r_theta, w the solution of [v; 0] with v's component along n removed"""
        S = self.S
        v = np.asarray(v, np.float64)
        if self.n is not None:
            v = v - self.n * (self.n @ v)
        w = S._solve(np.concatenate([v[S.keep], np.zeros(S.eq.size)]))
        return np.array([-w @ self.rhs(np.eye(M)[t]) for t in range(M)])

    def removed_vjp(self):
        """dSens[6] of the VJP: the largest removed relative size over the 34 fields"""
        return max(self.removed(np.eye(M)[t]) for t in range(M))

    def value_gradient(self):
        """dV*/dtheta [34] = d_theta f + lam^T d_theta g at (x, lam)"""
        out = np.zeros(M)
        for t in range(M):
            df, dg, _ = self._diff(np.eye(M)[t])
            out[t] = df + self.S.lam @ dg
        return out


def model_directions(cfg):
    """[(name, dtheta)]: one unit direction per field group -- friction, each weight, one corner of each foot (axis x), and a mirrored corner pair
    (left corner 0 and the right corner nearest to its mirror image y -> -y) moved identically (axis x, both feet)"""
    out = [(FIELDS[t], np.eye(M)[t]) for t in range(10)]
    out.append(("corner_left", np.eye(M)[corner_index(0, 0, 0)]))
    out.append(("corner_right", np.eye(M)[corner_index(1, 0, 0)]))
    th = theta_of(cfg)
    c0 = th[10:13] * np.array([1.0, -1.0, 1.0])
    jm = int(np.argmin([np.linalg.norm(th[corner_index(1, j, 0):corner_index(1, j, 0) + 3] - c0) for j in range(4)]))
    d = np.zeros(M)
    d[corner_index(0, 0, 0)] = d[corner_index(1, jm, 0)] = 1.0
    out.append(("corner_mirrored", d / np.linalg.norm(d)))
    return out
