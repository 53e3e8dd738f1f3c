"""Batch counterpart of the reference's CentroidalMPC class on top of BatchSolver (solver.py), and what its getOutput() exposes."""
from __future__ import annotations

from typing import TYPE_CHECKING, Optional

import numpy as np

from . import _capi
from .config import CentroidalMPCConfig, from_ini
from .contacts import pack_lists, sample_schedule_batch
from .layout import Layout

if TYPE_CHECKING:   # (solver.py imports this module: the class itself is imported where it is used, in initialize)
    from .solver import BatchSolver

class CentroidalMPCOutput:
    """What getOutput() exposes downstream (WholeBodyQPBlock.cpp:824-829, 1319-1335): per contact
    the first-knot corner forces (world frame, mass-normalised) and pose, plus the step-adjusted
    next landing position (CentroidalMPCBlock.cpp:598, 626)."""

    def __init__(self, names, forces0, pos0, next_pos, next_knot):
        self.contact_names = names
        self.forces = forces0        # [B,2,4,3]
        self.positions = pos0        # [B,2,3]
        self.next_positions = next_pos  # [B,2,3]
        self.next_knots = next_knot  # [B,2]


class CentroidalMPC:
    """Batch counterpart of BipedalLocomotion::ReducedModelControllers::CentroidalMPC."""

    def __init__(self, batch: int = 1, device: int = 0):
        self._batch = batch
        self._device = device
        self._solver: Optional[BatchSolver] = None
        self._out: Optional[CentroidalMPCOutput] = None
        self.last_error = ""
        self._valid = False
        self._now = 0.0

    # -- initialize(handler): handler = CentroidalMPCConfig, ini text, or dict of options
    def initialize(self, handler, **solver_opts) -> bool:
        try:
            from .solver import BatchSolver
            cfg = from_ini(handler) if isinstance(handler, str) else handler
            if not isinstance(cfg, CentroidalMPCConfig):
                raise TypeError("initialize() needs a CentroidalMPCConfig or the text of a centroidal_mpc.ini")
            self.cfg = cfg
            self._now = 0.0
            self._solver = BatchSolver(cfg, self._batch, self._device, **solver_opts)
            self._lib = self._solver._lib
            self._h = self._solver._h
            return True
        except Exception as e:  # mirrors the reference: log + return false
            self.last_error = str(e)
            return False

    def _ok(self, rc) -> bool:
        if rc != 0:
            self.last_error = self._solver.last_error
            return False
        return True

    def _need_init(self) -> bool:
        if self._solver is None:
            self.last_error = "initialize() has not been called"
            return False
        return True

    def set_state(self, com, dcom, angular_momentum, external_wrench=None) -> bool:
        """com, dcom, angular_momentum: [B,3]; external_wrench [B,6] (the measured wrench: enters the first knot only, like
        the C++ facade -- BLF's own rule is not visible from the reference tree, parity unpinned) or [B,N,6] (per knot) or
        None.  h and the wrench are mass-normalised (CentroidalMPCBlock.cpp:403-410)."""
        if not self._need_init():
            return False
        B, N = self._batch, self.cfg.N
        st = np.concatenate([np.reshape(com, (B, 3)), np.reshape(dcom, (B, 3)), np.reshape(angular_momentum, (B, 3))], 1)
        st = np.ascontiguousarray(st, np.float32)
        w = None
        if external_wrench is not None:
            w = np.asarray(external_wrench, np.float32)
            if w.ndim == 2:
                w0 = w
                w = np.zeros((B, N, 6), np.float32)
                w[:, 0, :] = w0
            w = np.ascontiguousarray(w.reshape(B, N, 6))
        return self._ok(self._lib.cmpc_set_state(self._h, st.ctypes.data, w.ctypes.data if w is not None else None))

    def set_reference_trajectory(self, com, angular_momentum) -> bool:
        """com, angular_momentum: [B,N+1,3] (the reference passes N+1 knots, CentroidalMPCBlock.cpp:230-235)."""
        if not self._need_init():
            return False
        B, N = self._batch, self.cfg.N
        c = np.ascontiguousarray(np.reshape(com, (B, N + 1, 3)), np.float32)
        h = np.ascontiguousarray(np.reshape(angular_momentum, (B, N + 1, 3)), np.float32)
        return self._ok(self._lib.cmpc_set_reference(self._h, c.ctypes.data, h.ctypes.data))

    def set_reference_from_planner(self, com_in, h_in, in_dt: float, t_offset: float, robot_mass: float,
                                   com_height: float = 0.7) -> bool:
        """Planner trajectories [B,M,3] every in_dt seconds -> MPC knots (CentroidalMPCBlock.cpp:525-577): angular
        momentum divided by the mass, CoM height forced to com_height (NaN keeps the planner's)."""
        if not self._need_init():
            return False
        B = self._batch
        c = np.ascontiguousarray(np.reshape(com_in, (B, -1, 3)), np.float32)
        h = np.ascontiguousarray(np.reshape(h_in, (B, -1, 3)), np.float32)
        return self._ok(self._lib.cmpc_set_reference_from_planner(self._h, c.ctypes.data, h.ctypes.data, c.shape[1], float(in_dt),
                                                                  float(t_offset), float(robot_mass), float(com_height)))

    def set_contact_phase_list(self, lists, t0: Optional[float] = None) -> bool:
        """lists: one dict {contact_name: [PlannedContact,...]} for every problem of the batch (or a single dict shared
        by all), with absolute times; or the packed arrays (t, pose, n) of contacts.pack_lists; or a dict of ready
        tensors with keys R, upper, lower, enabled, nominal, current.  Lists are sampled at the knots now + k dt, where
        `now` is the class's own clock: zero at initialize(), + dt per successful advance() -- the reference's caller
        never passes the time, it advances its own clock the same way (CentroidalMPCBlock.cpp:631).  t0 overrides it."""
        if not self._need_init():
            return False
        B = self._batch
        now = self._now if t0 is None else float(t0)
        try:
            if isinstance(lists, dict) and "R" in lists:
                t = lists
            else:
                if isinstance(lists, tuple):
                    packed = lists
                elif isinstance(lists, dict):
                    packed = pack_lists(self.cfg, [lists])
                else:
                    packed = pack_lists(self.cfg, list(lists))
                t, land = sample_schedule_batch(self.cfg, *packed, now)     # vectorised over the batch
                if packed[0].shape[0] == 1 and B > 1:
                    t = {k: np.broadcast_to(v, (B,) + v.shape[1:]) for k, v in t.items()}
                self._lists = packed
            self._sched = t
            a = {k: np.ascontiguousarray(t[k], np.float32) for k in ("R", "upper", "lower", "enabled", "nominal", "current")}
        except Exception as e:
            self.last_error = str(e)
            return False
        return self._ok(self._lib.cmpc_set_contacts(self._h, a["R"].ctypes.data, a["upper"].ctypes.data, a["lower"].ctypes.data,
                                                    a["enabled"].ctypes.data, a["nominal"].ctypes.data, a["current"].ctypes.data))

    def set_initial_guess(self, x0=None, shift_previous=False) -> bool:
        if not self._need_init():
            return False
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, np.float32)
        return self._ok(self._lib.cmpc_set_initial_guess(self._h, x0.ctypes.data if x0 is not None else None, int(shift_previous)))

    def advance(self) -> bool:
        if not self._need_init():
            return False
        self._valid = False
        rc = self._lib.cmpc_advance(self._h)
        if rc != 0:
            self.last_error = self._solver.last_error
            return False
        B = self._batch
        f0 = np.empty((B, 2, 4, 3), np.float32)
        p0 = np.empty((B, 2, 3), np.float32)
        pn = np.empty((B, 2, 3), np.float32)
        kn = np.empty((B, 2), np.int32)
        if not self._ok(self._lib.cmpc_get_output(self._h, f0.ctypes.data, p0.ctypes.data, pn.ctypes.data, kn.ctypes.data)):
            return False
        self._out = CentroidalMPCOutput([c.contact_name for c in self.cfg.contacts], f0, p0, pn, kn)
        self._now += self.cfg.sampling_time
        self._valid = True
        return True

    def get_output(self) -> CentroidalMPCOutput:
        return self._out

    def is_output_valid(self) -> bool:
        return self._valid

    def set_multiplier_output(self, enabled: bool = True) -> bool:
        """Keep the dual record of every later advance() (cmpc_set_multiplier_output), for get_multipliers()."""
        if not self._need_init():
            return False
        return self._ok(self._lib.cmpc_set_multiplier_output(self._h, 1 if enabled else 0))

    def get_multipliers(self):
        """lam_g[B, n_g] of the last advance() (cmpc_get_multipliers; the multiplier output must be on), or None."""
        L = Layout(self.cfg.N)
        lam = np.empty((self._batch, L.ng), np.float32)
        if not self._ok(self._lib.cmpc_get_multipliers(self._h, lam.ctypes.data)):
            return None
        return lam

    def get_feedback_gain(self):
        """d(first-knot corner forces)/d(com0, dcom0, h0) [B, 24, 9] of the last advance() (BatchSolver.feedback_gain_device at its solution, its
        parameters and its multipliers), or None.  Needs the multiplier output on before advance() (set_multiplier_output); a problem whose
        sensitivity status is not 0 gets a zero gain (get_feedback_gain_info() returns the [B, CMPC_SENS] words)."""
        import torch
        if not self._need_init():
            return None
        X, _ = self.get_solution()
        lam = self.get_multipliers()
        if X is None or lam is None:
            return None
        L = Layout(self.cfg.N)
        P = np.empty((self._batch, L.np), np.float32)
        if not self._ok(self._lib.cmpc_get_parameters(self._h, P.ctypes.data)):
            return None
        dev = torch.device("cuda", self._device)
        gain, sens = self._solver.feedback_gain_device(*(torch.from_numpy(a).to(dev) for a in (X, P, lam)))
        self._gain_sens = sens.cpu().numpy()
        return gain.cpu().numpy()

    def get_feedback_gain_info(self):
        return getattr(self, "_gain_sens", None)

    def get_solution(self):
        L = Layout(self.cfg.N)
        X = np.empty((self._batch, L.nx), np.float32)
        info = np.empty((self._batch, _capi.INFO), np.float32)
        if not self._ok(self._lib.cmpc_get_solution(self._h, X.ctypes.data, info.ctypes.data)):
            return None, None
        return X, info

