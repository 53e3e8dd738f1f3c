"""Host-side mirror of the reference's CentroidalMPC surface for a batch of problems.

Reference interface (BipedalLocomotion::ReducedModelControllers::CentroidalMPC, used at
src/centroidal-mpc-walking/src/CentroidalMPCBlock.cpp:144,407,579,609,615,622):
    initialize / setState / setReferenceTrajectory / setContactPhaseList / advance / getOutput
Every mutator returns bool like the reference's (False => the caller logs and aborts the tick,
CentroidalMPCBlock.cpp:609-619); `last_error` holds the text.  All compute happens in
libcmpc_hip.so (hand-written gfx950 kernels) through the C ABI of include/cmpc.h.

The Python side is laid out like the C ABI's three files: a method lives in the module named after the file that defines the cmpc_* symbol it calls --
solver.py (csrc/cmpc_api.hip), solver_rollout.py (cmpc_api_rollout.hip), solver_walk_grad.py (cmpc_api_walk_grad.hip); the facade class is in facade.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _args, _capi
from ._args import _upload, opt_ptr, ptr  # noqa: F401  (_upload: reached as solver._upload by rollout.py)
from .config import GRAVITY, CentroidalMPCConfig, model_array
from .facade import CentroidalMPC, CentroidalMPCOutput  # noqa: F401
from .layout import Layout
from .solver_rollout import RolloutCalls
from .solver_walk_grad import WalkGradCalls


def _c_config(cfg: CentroidalMPCConfig, tolerance=None, mu_min=None, max_iterations=None,
              exact_hessian=True, final_extrapolation=True, step_tolerance=None, mu_init=None,
              tail_stages=3, tail_iterations=2, tail_trigger=2e-5, factors=None) -> _capi.CmpcConfig:
    c = _capi.CmpcConfig()
    c.horizon = cfg.N
    c.sampling_time = cfg.sampling_time
    c.friction_coefficient = cfg.static_friction_coefficient
    c.gravity = GRAVITY
    c.com_weight[:] = cfg.com_weight
    c.angular_momentum_weight = cfg.angular_momentum_weight
    c.contact_position_weight = cfg.contact_position_weight
    c.force_rate_of_change_weight[:] = cfg.force_rate_of_change_weight
    c.contact_force_symmetry_weight = cfg.contact_force_symmetry_weight
    c.corners[:] = np.asarray([cc.corners for cc in cfg.contacts], np.float64).reshape(-1)
    c.max_iterations = max_iterations or cfg.ipopt_max_iteration
    # the reference's ipopt_tolerance (1e-4 / 1e-2) is looser than the parity target; the GPU
    # solver always converges at least to 1e-6 so that its answer is reproducible to 1e-4
    # (0: the library's default -- 1e-6 for N = 4 .. 20, 3e-7 beyond and for N <= 3; step tolerance and barrier floor follow it)
    # (the ini value only when it is tighter than that default, as in the C++ facade)
    if tolerance is None:
        tolerance = cfg.ipopt_tolerance if 0 < cfg.ipopt_tolerance < _capi.lib().cmpc_default_tolerance(cfg.N) else 0.0
    c.tolerance = tolerance
    c.step_tolerance = step_tolerance if step_tolerance is not None else 0.0
    c.mu_init = mu_init if mu_init is not None else 0.0   # <= 0: per problem, from its initial infeasibility
    c.mu_min = mu_min if mu_min is not None else 0.0
    c.exact_hessian = int(exact_hessian)
    c.final_extrapolation = int(final_extrapolation)
    # tail polish (include/cmpc.h): the last stages re-solved when their extrapolation step is large
    c.tail_stages, c.tail_iterations, c.tail_trigger = int(tail_stages), int(tail_iterations), float(tail_trigger)
    c.factor_storage = _capi.FACTORS[factors]   # None / "auto": by batch size and horizon; "lds" / "hbm": the resident / the HBM-factor variant
    return c


def _model_array(models, batch) -> np.ndarray:
    """[B, 34] float64 C-contiguous host array from B configurations or an array of model rows"""
    if isinstance(models, (list, tuple)) and models and isinstance(models[0], CentroidalMPCConfig):
        a = model_array(models)
    else:
        a = np.ascontiguousarray(models.cpu().numpy() if hasattr(models, "cpu") else models, np.float64)
    if a.shape != (batch, _capi.MODEL_DOUBLES):
        raise ValueError(f"models: expected shape ({batch}, {_capi.MODEL_DOUBLES}), got {a.shape}")
    return a


class BatchSolver(RolloutCalls, WalkGradCalls):
    """Thin RAII wrapper of a cmpc_handle: device-resident batched solve.  The entries of csrc/cmpc_api.hip are here, those of cmpc_api_rollout.hip
    and cmpc_api_walk_grad.hip in the two base classes (solver_rollout.py, solver_walk_grad.py)."""

    def __init__(self, cfg: CentroidalMPCConfig, batch: int, device: int = 0, **opts):
        self.cfg = cfg
        self.layout = Layout(cfg.N)
        self.batch = batch
        self._device_index = device
        self._lib = _capi.lib()
        self._ccfg = _c_config(cfg, **opts)
        h = C.c_void_p()
        rc = self._lib.cmpc_create(C.byref(self._ccfg), batch, device, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"cmpc_create failed ({rc}): {self._lib.cmpc_last_error(None).decode()}")
        self._h = h
        self._stream = None  # torch.cuda.Stream the kernels are launched on (created lazily)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cmpc_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def last_error(self) -> str:
        return self._lib.cmpc_last_error(self._h).decode()

    @property
    def factor_storage(self) -> str:
        """"lds" / "hbm": the storage the handle's kernel variant uses (an "lds" request that does not fit is served from HBM)"""
        return {1: "lds", 2: "hbm"}[self._lib.cmpc_factor_storage(self._h)]

    def solve_device(self, dP, dX0, dX=None, dInfo=None, stream=None, warm=False):
        """torch CUDA tensors float32: P[B,np], X0[B,nx] -> X[B,nx], info[B,8].  Launches on
        torch's current stream unless `stream` (a raw hipStream_t) is given; asynchronous.
        warm: dX0 is the previous solution shifted by one knot (shift_solution_device) -> cmpc_solve_device_warm."""
        import torch
        L = self.layout
        pp, px0 = ptr(dP, torch.float32, (self.batch, L.np), "dP", True), ptr(dX0, torch.float32, (self.batch, L.nx), "dX0", True)
        if dX is None:
            dX = torch.empty_like(dX0)
        if dInfo is None:
            dInfo = torch.empty((self.batch, _capi.INFO), dtype=torch.float32, device=dP.device)
        fn = self._lib.cmpc_solve_device_warm if warm else self._lib.cmpc_solve_device
        h, px, pi = self._h, dX.data_ptr(), dInfo.data_ptr()
        if stream is None:
            self._launch(dP.device, lambda st: fn(h, pp, px0, px, pi, st), "cmpc_solve_device")
        elif (rc := fn(h, pp, px0, px, pi, stream)) != 0:
            raise RuntimeError(f"cmpc_solve_device failed ({rc}): {self.last_error}")
        return dX, dInfo

    def _stream_pair(self, dev):
        """(raw hipStream_t to launch on, torch stream to join back into or None).  Torch's current stream itself when it is not the default stream -- no
        cross-stream dependency at all; run a loop of device calls under `with torch.cuda.stream(solver.launch_stream):` to get that.  The default stream's
        handle is 0, which the C ABI reads as "the handle's own stream": there the call goes to a side stream ordered after the default stream and joined
        back into it -- two event dependencies per call, measured at 24 us of idle GPU per solve between back-to-back launches (tools/gpu_enqueue_probe.py)."""
        import torch
        cur = torch.cuda.current_stream(dev)
        if cur.cuda_stream != 0:
            return cur.cuda_stream, None
        if self._stream is None:
            self._stream = torch.cuda.Stream(dev)
        self._stream.wait_stream(cur)
        return self._stream.cuda_stream, cur

    def _launch(self, dev, fn, name=None):
        """runs fn(raw_stream) on torch's current stream (the default stream: on the solver's side stream, ordered after it and joined back; _stream_pair);
        the one place that takes the stream pair, calls, raises and joins back.  name: the C symbol, for the error text"""
        st, cur = self._stream_pair(dev)
        rc = fn(st)
        if rc != 0:
            if name is not None:
                raise RuntimeError(f"{name} failed ({rc}): {self.last_error}")
            raise RuntimeError(f"libcmpc_hip call failed ({rc}): {self.last_error}")
        if cur is not None:
            cur.wait_stream(self._stream)

    _opt = staticmethod(ptr)   # (data_ptr of an optional CUDA tensor (None -> NULL), checked: the spelling this class has always used)

    def _dev(self, device=None):
        """`device`, or the handle's own"""
        import torch
        return torch.device("cuda", self._device_index) if device is None else device

    def _box_arrays(self):
        """(upper, lower) limits of the contacts' bounding boxes as host float32 arrays, built once and kept in _box for the launches that read them"""
        if getattr(self, "_box", None) is None:
            self._box = (np.ascontiguousarray([c.bounding_box_upper_limit for c in self.cfg.contacts], np.float32),
                         np.ascontiguousarray([c.bounding_box_lower_limit for c in self.cfg.contacts], np.float32))
        return self._box

    @property
    def launch_stream(self):
        """torch.cuda.Stream the solve kernel runs on (record timing events here)."""
        import torch
        if self._stream is None:
            self._stream = torch.cuda.Stream(self._dev())
        return self._stream

    def solve_host(self, P: np.ndarray, X0: np.ndarray):
        """numpy float32 in/out through the PCIe-inclusive entry point.  Returns (X, info, rc)."""
        L = self.layout
        P = np.ascontiguousarray(P, np.float32)
        X0 = np.ascontiguousarray(X0, np.float32)
        if P.shape != (self.batch, L.np) or X0.shape != (self.batch, L.nx):
            raise AssertionError(f"solve_host: expected P {(self.batch, L.np)} and X0 {(self.batch, L.nx)}")
        X = np.empty_like(X0)
        info = np.empty((self.batch, _capi.INFO), np.float32)
        rc = self._lib.cmpc_solve(self._h, P.ctypes.data, X0.ctypes.data, X.ctypes.data, info.ctypes.data)
        if rc not in (0, -3):
            raise RuntimeError(f"cmpc_solve failed ({rc}): {self.last_error}")
        return X, info, rc

    def set_models(self, models):
        """cmpc_set_models: per-problem models (include/cmpc.h) -- a list of B CentroidalMPCConfig (only their model fields are read: friction,
        weights, corners), or an array [B, 34] float64 in cmpc_model's order (config.model_array); None: back to the handle's configuration.
        Checked on the host: a row that breaks the model rule raises ValueError naming its index and field, and the previous table stays."""
        if models is None:
            rc = self._lib.cmpc_set_models(self._h, None)
        else:
            a = _model_array(models, self.batch)
            rc = self._lib.cmpc_set_models(self._h, a.ctypes.data)
            if rc == -1:
                raise ValueError(self.last_error)
        if rc != 0:
            raise RuntimeError(f"cmpc_set_models failed ({rc}): {self.last_error}")

    def set_models_device(self, models, ok=None):
        """cmpc_set_models_device: models a [B, 34] float64 CUDA tensor (cmpc_model's order), the records derived by a kernel on torch's current
        stream.  A row that breaks the model rule is not an error: ok[b] = 0 (int32 [B], returned) and that problem's solves return status 3."""
        import torch
        pm = ptr(models, torch.float64, (self.batch, _capi.MODEL_DOUBLES), "models", True)
        ok = _args.out(ok, torch.int32, (self.batch,), "ok", models.device)
        self._launch(models.device, lambda st: self._lib.cmpc_set_models_device(self._h, pm, ok.data_ptr(), st))
        return ok

    def set_warm_policy(self, warm_budget: int = 0, restart_in_kernel: bool = True):
        """cmpc_set_warm_policy: iteration budget of a warm-started pass (0: max_iterations) and whether a warm start that does not
        converge is started again from the cold start inside the launch (True) or returned with status 1 (False)."""
        rc = self._lib.cmpc_set_warm_policy(self._h, int(warm_budget), 1 if restart_in_kernel else 0)
        if rc != 0:
            raise RuntimeError(f"cmpc_set_warm_policy failed ({rc}): {self.last_error}")

    def set_ended_device(self, end_tick=None):
        """cmpc_set_ended_device: end_tick an int32 CUDA tensor [B] in the convention of a walk record's end_tick (-1 walking, >= 0 ended), read on the
        device by every later solve, tick and cold start on this handle when it runs: a problem whose word is >= 0 is left out of those launches and none
        of its data is written (include/cmpc.h).  None: off (the default).  The tensor is referenced from here while it is set; launches already queued
        keep the pointer they were queued with, so a caller who clears the setting keeps the tensor alive until they have run."""
        if not hasattr(self._lib, "cmpc_set_ended_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_set_ended_device")
        import torch
        rc = self._lib.cmpc_set_ended_device(self._h, ptr(end_tick, torch.int32, (self.batch,), "end_tick"))
        if rc != 0:
            raise RuntimeError(f"cmpc_set_ended_device failed ({rc}): {self.last_error}")
        self._ended = end_tick

    def set_walk_limits(self, height=(None, None), reach_max=None, margin_min=None, track_max=None, measures=None, extremes=None, off=False):
        """cmpc_set_walk_limits: the physical limits every later record launch of this handle evaluates (tick codes 6..9, include/cmpc.h) -- height =
        (min, max), reach_max, margin_min, track_max, None or NaN: that limit is off -- with measures, a float32 CUDA tensor [rows, B, 4] or None (the
        per-tick trace of height, reach, margin, track), and extremes, a float32 CUDA tensor [B, 5] or None (walk_extremes_init_device sets it up).
        off=True: the setting is cleared (the default state).  The tensors are referenced from here while the setting holds; launches already queued
        keep the pointers they were queued with."""
        if not hasattr(self._lib, "cmpc_set_walk_limits"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_set_walk_limits")
        if off:
            rc = self._lib.cmpc_set_walk_limits(self._h, None)
            self._walk_limits = None
        else:
            import torch
            nan = lambda v: float("nan") if v is None else float(v)
            pm = ptr(measures, torch.float32, (None, self.batch, _capi.WALK_MEASURES), "measures")
            pe = ptr(extremes, torch.float32, (self.batch, _capi.WALK_EXTREMES), "extremes")
            lim = _capi.CmpcWalkLimits(nan(height[0]), nan(height[1]), nan(reach_max), nan(margin_min), nan(track_max),
                                       pm, int(measures.shape[0]) if measures is not None else 0, pe)
            rc = self._lib.cmpc_set_walk_limits(self._h, C.byref(lim))
            if rc == 0:
                self._walk_limits = (measures, extremes)
        if rc != 0:
            raise RuntimeError(f"cmpc_set_walk_limits failed ({rc}): {self.last_error}")

    def last_solve_ms(self) -> float:
        return float(self._lib.cmpc_last_solve_ms(self._h))

    def set_timing(self, enabled: bool = True):
        """cmpc_set_timing: record (default) or not the event pair around every solve launch that last_solve_ms() reads."""
        if hasattr(self._lib, "cmpc_set_timing"):
            self._lib.cmpc_set_timing(self._h, 1 if enabled else 0)

    def compact_output_device(self, dX, dInfo, out=None):
        """[B, 3(N+1) + 38] compact record of every problem (what distributed.compact_output builds with torch ops), by
        one kernel on the solver's stream; torch CUDA tensors."""
        import torch
        W = 3 * (self.cfg.N + 1) + 38
        out = _args.out(out, torch.float32, (self.batch, W), "out", dX.device)
        self._launch(dX.device, lambda st: self._lib.cmpc_compact_output_device(self._h, dX.data_ptr(), dInfo.data_ptr(), out.data_ptr(), st),
                     "cmpc_compact_output_device")
        return out

    # ---- multipliers of the reference NLP, KKT certificate, gradient of the optimal cost (include/cmpc.h) ----
    def set_multiplier_output(self, enabled: bool = True):
        """cmpc_set_multiplier_output: every later solve on this handle also keeps its dual record (what multipliers_device maps)."""
        rc = self._lib.cmpc_set_multiplier_output(self._h, 1 if enabled else 0)
        if rc != 0:
            raise RuntimeError(f"cmpc_set_multiplier_output failed ({rc}): {self.last_error}")

    def _nlp_point(self, dX, dP, dLamG, lam=True):
        """the checked pointers of a point (x, p, lam_g) of the reference NLP; lam=False: the call takes no lam_g"""
        import torch
        L, B = self.layout, self.batch
        return (ptr(dX, torch.float32, (B, L.nx), "dX", True), ptr(dP, torch.float32, (B, L.np), "dP", True),
                ptr(dLamG, torch.float32, (B, L.ng), "dLamG", lam))

    def _nlp_out(self, dX, dP, dLamG, out, width, fn, name, what="out", lam=True):
        """check the point, allocate or check `out` [B, width] float32, launch fn(x, p, lam_g, out, stream) -- pointers -- as the C symbol `name`"""
        import torch
        point = self._nlp_point(dX, dP, dLamG, lam)
        out = _args.out(out, torch.float32, (self.batch, width), what, dX.device)
        self._launch(dX.device, lambda st: fn(*point, out.data_ptr(), st), name)
        return out

    def multipliers_device(self, dX, dP, out=None):
        """lam_g[B, n_g] of the last solve (dX, dP: its solution and parameters) in the reference's row order and IPOPT's sign convention."""
        return self._nlp_out(dX, dP, None, out, self.layout.ng, lambda x, p, _, o, st: self._lib.cmpc_get_multipliers_device(self._h, x, p, o, st),
                             "cmpc_get_multipliers_device", lam=False)

    def kkt_certificate_device(self, dX, dP, dLamG, out=None):
        """[B, CMPC_CERT] KKT certificate of the reference NLP at (x, lam_g): stationarity, primal infeasibility, complementarity, sign violation,
        f, status, scale, unscaled stationarity (include/cmpc.h)."""
        return self._nlp_out(dX, dP, dLamG, out, _capi.CERT, lambda *a: self._lib.cmpc_kkt_certificate_device(self._h, *a), "cmpc_kkt_certificate_device")

    def value_gradient_device(self, dX, dP, dLamG, out=None):
        """dV*/dp [B, n_p] at a KKT point (x*, lam*): grad_p L plus the terms of the parameters that only enter the bounds."""
        return self._nlp_out(dX, dP, dLamG, out, self.layout.np, lambda *a: self._lib.cmpc_value_gradient_device(self._h, *a), "cmpc_value_gradient_device")

    # ---- solution sensitivities dx*/dp (include/cmpc.h) ----
    def _directions(self, dirs, msg):
        """the direction check of the solution_jvp_* family: dirs = (tensor or None, dtype, tail, name), each [B, k, *tail] with k >= 1, one k among
        those given (none given, or two values of k: AssertionError(msg)) -> (k, their pointers)"""
        for t, _, tail, name in dirs:
            if t is not None and (t.dim() < 2 or t.shape[1] < 1):
                raise AssertionError(f"{name}: expected [B, k >= 1, {tail}]")
        ks = {int(t.shape[1]) for t, _, _, _ in dirs if t is not None}
        if len(ks) != 1:
            raise AssertionError(msg)
        k = ks.pop()
        return k, [ptr(t, dt, (self.batch, k) + tail, name) for t, dt, tail, name in dirs]

    def _grad_outs(self, outs, lead, dev):
        """the output check of the solution_vjp_* family: outs = (wanted, tensor or None, dtype, tail, name) -> the tensors [*lead, *tail], made when
        wanted and None, checked when given, None when neither"""
        return [_args.out(t, dt, lead + tail, name, dev) if want or t is not None else None for want, t, dt, tail, name in outs]

    def solution_jvp_device(self, dX, dP, dLamG, dDirP, out=None, sens=None):
        """dx*/dp applied to k directions: dDirP[B, k, n_p] -> (dDX[B, k, n_x], sens[B, CMPC_SENS]) at the returned point (x, p, lam_g) of a solve.
        sens = (status 0 ok / 1 non-positive pivot / 2 not finite / 3 outside the subset, relative residual, weakly active rows, largest Sigma, ...);
        a flagged problem's outputs are zero."""
        import torch
        L = self.layout
        k, (pd,) = self._directions(((dDirP, torch.float32, (L.np,), "dDirP"),), "solution_jvp_device: no direction")
        out = _args.out(out, torch.float32, (self.batch, k, L.nx), "out", dX.device)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda x, p, l, o, st: self._lib.cmpc_solution_jvp_device(self._h, x, p, l, pd, k, out.data_ptr(), o, st),
                             "cmpc_solution_jvp_device", "sens")
        return out, sens

    def solution_vjp_device(self, dX, dP, dLamG, dGradX, out=None, sens=None):
        """(dx*/dp)^T v: dGradX[B, n_x] = dl/dx -> (dl/dp [B, n_p], sens[B, CMPC_SENS])."""
        import torch
        L = self.layout
        pg = ptr(dGradX, torch.float32, (self.batch, L.nx), "dGradX", True)
        out, = self._grad_outs(((True, out, torch.float32, (L.np,), "out"),), (self.batch,), dX.device)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda x, p, l, o, st: self._lib.cmpc_solution_vjp_device(self._h, x, p, l, pg, out.data_ptr(), o, st),
                             "cmpc_solution_vjp_device", "sens")
        return out, sens

    def feedback_gain_device(self, dX, dP, dLamG):
        """The linearised MPC policy: d(first-knot corner forces)/d(com0, dcom0, h0) -> (gain[B, 24, 9], sens[B, CMPC_SENS]); rows in the
        order of Layout.first_forces (contact, corner, axis), columns com0 xyz, dcom0 xyz, h0 xyz.  One JVP with 9 directions."""
        import torch
        L = self.layout
        dirs = torch.zeros((self.batch, 9, L.np), dtype=torch.float32, device=dX.device)
        for i in range(9):
            dirs[:, i, L.p_com0 + i] = 1.0
        dDX, sens = self.solution_jvp_device(dX, dP, dLamG, dirs)
        idx = torch.as_tensor(np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)]), device=dX.device)
        return dDX[:, :, idx].transpose(1, 2).contiguous(), sens

    # ---- derivatives with respect to the per-problem model (include/cmpc.h, "model directions") ----
    def solution_jvp_model_device(self, dX, dP, dLamG, dDirP=None, dDirModel=None, out=None, sens=None):
        """dx*/d(p, theta) applied to k directions: dDirP[B, k, n_p] float32 and dDirModel[B, k, 34] float64 in cmpc_model's order (either may be
        None: zero) -> (dDX[B, k, n_x], sens[B, CMPC_SENS]).  sens[:, 6]: the relative component of the model right-hand sides along the
        internal-force direction that was removed (largest over the k columns).  dDirModel None gives solution_jvp_device's result bit for bit."""
        import torch
        L = self.layout
        if dDirP is None and dDirModel is None:
            raise AssertionError("solution_jvp_model_device: no direction")
        k, (pp, pm) = self._directions(((dDirP, torch.float32, (L.np,), "dDirP"), (dDirModel, torch.float64, (_capi.MODEL_DOUBLES,), "dDirModel")),
                                       "solution_jvp_model_device: directions of different k")
        out = _args.out(out, torch.float32, (self.batch, k, L.nx), "out", dX.device)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda x, p, l, o, st: self._lib.cmpc_solution_jvp_model_device(self._h, x, p, l, pp, pm, k, out.data_ptr(), o, st),
                             "cmpc_solution_jvp_model_device", "sens")
        return out, sens

    def solution_vjp_model_device(self, dX, dP, dLamG, dGradX, out_model=None, out_p=None, sens=None, grad_p=True):
        """(dx*/d(p, theta))^T v from one adjoint solve: dGradX[B, n_x] = dl/dx -> (dl/dtheta [B, 34] float64, dl/dp [B, n_p] float32 or None
        when grad_p is False, sens[B, CMPC_SENS]).  dl/dp equals solution_vjp_device's bit for bit; sens[:, 6]: the largest relative component
        along the internal-force direction over the 34 fields."""
        import torch
        L = self.layout
        pg = ptr(dGradX, torch.float32, (self.batch, L.nx), "dGradX", True)
        out_model, out_p = self._grad_outs(((True, out_model, torch.float64, (_capi.MODEL_DOUBLES,), "out_model"),
                                            (grad_p, out_p, torch.float32, (L.np,), "out_p")), (self.batch,), dX.device)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda x, p, l, o, st: self._lib.cmpc_solution_vjp_model_device(self._h, x, p, l, pg, opt_ptr(out_p), out_model.data_ptr(), o, st),
                             "cmpc_solution_vjp_model_device", "sens")
        return out_model, out_p, sens

    def model_value_gradient_device(self, dX, dP, dLamG, out=None):
        """dV*/dtheta [B, 34] float64 at a KKT point (x*, lam*): d_theta f + lam^T d_theta g, at each problem's own model (zeros for a row whose model
        broke the model rule).  At a double-support point the corner entries depend on the internal force the solve returned (include/cmpc.h)."""
        import torch
        point = self._nlp_point(dX, dP, dLamG)
        out = _args.out(out, torch.float64, (self.batch, _capi.MODEL_DOUBLES), "out", dX.device)
        self._launch(dX.device, lambda st: self._lib.cmpc_model_value_gradient_device(self._h, *point, out.data_ptr(), st))
        return out

    # ---- derivatives with respect to the stage rotations (include/cmpc.h, "rotation directions") ----
    def solution_jvp_rot_device(self, dX, dP, dLamG, dDirP=None, dDirModel=None, dDirRot=None, out=None, sens=None):
        """dx*/d(p, theta, omega) applied to k directions: dDirP[B, k, n_p] float32, dDirModel[B, k, 34] float64 and dDirRot[B, k, 2, N, 3] float64
        (omega moves R_{c,k} along R [omega]x; any may be None: zero) -> (dDX[B, k, n_x], sens[B, CMPC_SENS]).  sens[:, 6]: the largest relative
        component of the model and rotation right-hand sides along the internal-force direction that was removed.  dDirRot None gives
        solution_jvp_model_device's result bit for bit."""
        import torch
        L = self.layout
        k, (pp, pm, pr) = self._directions(((dDirP, torch.float32, (L.np,), "dDirP"), (dDirModel, torch.float64, (_capi.MODEL_DOUBLES,), "dDirModel"),
                                            (dDirRot, torch.float64, (2, L.N, 3), "dDirRot")),
                                           "solution_jvp_rot_device: no direction, or directions of different k")
        out = _args.out(out, torch.float32, (self.batch, k, L.nx), "out", dX.device)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda x, p, l, o, st: self._lib.cmpc_solution_jvp_rot_device(self._h, x, p, l, pp, pm, pr, k, out.data_ptr(), o, st),
                             "cmpc_solution_jvp_rot_device", "sens")
        return out, sens

    def solution_vjp_rot_device(self, dX, dP, dLamG, dGradX, out_rot=None, out_model=None, out_p=None, sens=None, grad_p=True, grad_model=True):
        """(dx*/d(p, theta, omega))^T v from one adjoint solve: dGradX[B, n_x] = dl/dx -> (dl/domega [B, 2, N, 3] float64, dl/dtheta [B, 34]
        float64 or None, dl/dp [B, n_p] float32 or None, sens[B, CMPC_SENS]).  dl/dp and dl/dtheta equal solution_vjp_model_device's bit for bit."""
        import torch
        L = self.layout
        pg = ptr(dGradX, torch.float32, (self.batch, L.nx), "dGradX", True)
        out_rot, out_model, out_p = self._grad_outs(((True, out_rot, torch.float64, (2, L.N, 3), "out_rot"),
                                                     (grad_model, out_model, torch.float64, (_capi.MODEL_DOUBLES,), "out_model"),
                                                     (grad_p, out_p, torch.float32, (L.np,), "out_p")), (self.batch,), dX.device)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS, lambda x, p, l, o, st: self._lib.cmpc_solution_vjp_rot_device(
            self._h, x, p, l, pg, opt_ptr(out_p), opt_ptr(out_model), out_rot.data_ptr(), o, st), "cmpc_solution_vjp_rot_device", "sens")
        return out_rot, out_model, out_p, sens

    # ---- cotangent columns: k VJPs behind one factorisation per problem (include/cmpc.h, "Cotangent columns") ----
    def solution_vjp_cols_device(self, dX, dP, dLamG, dGradX, grad_p=True, grad_model=False, grad_rot=False, out_p=None, out_model=None, out_rot=None,
                                 sens=None):
        """(dx*/d(p, theta, omega))^T applied to k cotangents from one factorisation: dGradX[B, k, n_x] float32 -> (dl/dp [B, k, n_p] float32,
        dl/dtheta [B, k, 34] float64, dl/domega [B, k, 2, N, 3] float64, sens[B, CMPC_SENS]); an output that was not requested is None.  Column j
        equals solution_vjp_rot_device on dGradX[:, j] bit for bit.  sens is one row per problem: sens[:, 1] the largest residual over the columns,
        sens[:, 6] the largest removed component over columns and fields; a non-finite entry in any column flags the whole problem (status 2, zeros
        in every column)."""
        import torch
        L = self.layout
        if not (grad_p or grad_model or grad_rot):
            raise AssertionError("solution_vjp_cols_device: no output requested")
        if dGradX.dim() != 3:
            raise AssertionError("solution_vjp_cols_device: dGradX is [B, k, n_x]")
        if dGradX.dtype != torch.float32:
            raise AssertionError("solution_vjp_cols_device: dGradX is float32")
        k = int(dGradX.shape[1])
        pg = ptr(dGradX, torch.float32, (self.batch, k, L.nx), "dGradX")
        if k < 1:
            raise AssertionError("solution_vjp_cols_device: dGradX is [B, k >= 1, n_x]")
        outs = self._grad_outs(((grad_p, out_p if grad_p else None, torch.float32, (L.np,), "out_p"),        # (an output that was not requested is not used)
                                (grad_model, out_model if grad_model else None, torch.float64, (_capi.MODEL_DOUBLES,), "out_model"),
                                (grad_rot, out_rot if grad_rot else None, torch.float64, (2, L.N, 3), "out_rot")), (self.batch, k), dX.device)
        pp, pm, pr = (opt_ptr(t) for t in outs)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda x, p, l, o, st: self._lib.cmpc_solution_vjp_cols_device(self._h, x, p, l, pg, k, pp, pm, pr, o, st),
                             "cmpc_solution_vjp_cols_device", "sens")
        return outs[0], outs[1], outs[2], sens

    def policy_jacobian_device(self, dX, dP, dLamG, rows=None, model=False, rot=False):
        """Rows of dx*/d(p, theta, omega): rows = indices into x (default: the 24 first-knot corner forces, in feedback_gain_device's row order,
        that of Layout.first_forces) -> (J_p[B, len(rows), n_p] float32, J_model[B, len(rows), 34] float64 or None, J_rot[B, len(rows), 2, N, 3]
        float64 or None, sens[B, CMPC_SENS]).  One unit cotangent per row through one solution_vjp_cols_device call: one factorisation per problem,
        the rows in chunks of 8.  The derivatives are in the barrier form of DESIGN.md 7c, weakly active rows included; in double support the unit
        cotangents lose their component along the internal-force direction, as every cotangent does."""
        import torch
        L = self.layout
        if rows is None:
            rows = np.concatenate([np.arange(L.f[c][j], L.f[c][j] + 3) for c in range(2) for j in range(4)])
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if not (rows.size >= 1 and rows.min() >= 0 and rows.max() < L.nx):
            raise AssertionError("policy_jacobian_device: rows index x")
        V = torch.zeros((self.batch, rows.size, L.nx), dtype=torch.float32, device=dX.device)
        V[:, torch.arange(rows.size, device=dX.device), torch.as_tensor(rows, device=dX.device)] = 1.0
        return self.solution_vjp_cols_device(dX, dP, dLamG, V, grad_p=True, grad_model=model, grad_rot=rot)

    def rotation_value_gradient_device(self, dX, dP, dLamG, out=None):
        """dV*/domega [B, 2, N, 3] float64 at a KKT point (x*, lam*): lam^T d_omega g (the cost does not depend on R).  At a double-support point
        the entries depend on the internal force the solve returned (include/cmpc.h)."""
        import torch
        point = self._nlp_point(dX, dP, dLamG)
        out = _args.out(out, torch.float64, (self.batch, 2, self.layout.N, 3), "out", dX.device)
        self._launch(dX.device, lambda st: self._lib.cmpc_rotation_value_gradient_device(self._h, *point, out.data_ptr(), st))
        return out

    def contacts_rotation_vjp_device(self, now, list_t, list_n, dGradRot, out=None):
        """Per-stage -> per-list-entry (cmpc_contacts_rotation_vjp_device): list_t[B,2,M,2] float64 / list_n[B,2] int32 = the sampled lists,
        dGradRot[B,2,N,3] float64 -> dGradListRot[B,2,M,3] float64: entry m receives the sum of dGradRot over the stages it owns, in the body-frame
        tangent of its quaternion (q <- q (x) exp(omega / 2))."""
        import torch
        L, B, M, dev = self.layout, self.batch, list_t.shape[2], list_t.device
        out = _args.out(out, torch.float64, (B, 2, M, 3), "out", dev)
        args = (ptr(list_t, torch.float64, (B, 2, M, 2), "list_t", True), self._opt(list_n, torch.int32, (B, 2), "list_n"),
                self._opt(dGradRot, torch.float64, (B, 2, L.N, 3), "dGradRot"), out.data_ptr())
        self._launch(dev, lambda st: self._lib.cmpc_contacts_rotation_vjp_device(self._h, M, float(now), *args, st))
        return out

    def workspace_bytes_per_problem(self) -> int:
        """bytes of the sensitivity workspace per problem (cmpc_sensitivity_workspace_bytes)"""
        return int(self._lib.cmpc_sensitivity_workspace_bytes(self.layout.N))

    def plant_step_device(self, dX, dP, dState, dStateOut=None, dZmp=None, step=0.01, substeps=6,
                          zmp_half_x=0.08, zmp_half_y=0.03):
        """Closed-loop plant between two MPC ticks (WholeBodyQPBlock.cpp:805-873, 1083-1084, 1150): RK4 of the
        centroidal dynamics under the first-knot forces; torch CUDA tensors; returns (state[B,9], zmp[B,2])."""
        import torch
        if dStateOut is None:
            dStateOut = torch.empty_like(dState)
        if dZmp is None:
            dZmp = torch.empty((self.batch, 2), dtype=torch.float32, device=dState.device)
        self._launch(dState.device, lambda st: self._lib.cmpc_plant_step_device(
            self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), dStateOut.data_ptr(), dZmp.data_ptr(), float(step), int(substeps), float(zmp_half_x),
            float(zmp_half_y), st), "cmpc_plant_step_device")
        return dStateOut, dZmp

    # ---- plant-model mismatch (include/cmpc.h, "plant-model mismatch on the device walk"; DESIGN.md 7f, "Mismatch") ----
    def plant_step_mismatch_device(self, dX, dP, dState, dStateOut=None, dZmp=None, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03,
                                   hidden_wrench=None, force_gain=None):
        """cmpc_plant_step_mismatch_device: plant_step_device under one tick's hidden wrench hidden_wrench[B, 6] and the force gain force_gain[B] (float32
        CUDA tensors; None: not applied -- both None is plant_step_device bit for bit); returns (state[B,9], zmp[B,2])."""
        import torch
        B = self.batch
        if dStateOut is None:
            dStateOut = torch.empty_like(dState)
        if dZmp is None:
            dZmp = torch.empty((B, 2), dtype=torch.float32, device=dState.device)
        ph, pg = self._opt(hidden_wrench, torch.float32, (B, 6), "hidden_wrench"), self._opt(force_gain, torch.float32, (B,), "force_gain")
        self._launch(dState.device, lambda st: self._lib.cmpc_plant_step_mismatch_device(
            self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), dStateOut.data_ptr(), dZmp.data_ptr(), float(step), int(substeps), float(zmp_half_x),
            float(zmp_half_y), ph, pg, st))
        return dStateOut, dZmp

    def plant_step_vjp_mismatch_device(self, dX, dP, dState, dGradStateOut, step=0.01, substeps=6, hidden_wrench=None, force_gain=None, grad_rot=False):
        """cmpc_plant_step_vjp_mismatch_device: plant_step_vjp_device at the mismatched plant (hidden_wrench[B, 6], force_gain[B] float32 or None) ->
        dict(state[B,9] f64, x[B,n_x] f32, p[B,n_p] f32, model[B,34] f64, rot0[B,2,3] f64 or None, hidden[B,6] f64, gain[B] f64)."""
        import torch
        L, B, dev = self.layout, self.batch, dX.device
        f32, f64 = torch.float32, torch.float64
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(state=e((B, 9), f64), x=e((B, L.nx), f32), p=e((B, L.np), f32), model=e((B, _capi.MODEL_DOUBLES), f64),
                   rot0=e((B, 2, 3), f64) if grad_rot else None, hidden=e((B, 6), f64), gain=e((B,), f64))
        pg = self._opt(dGradStateOut, f64, (B, 9), "dGradStateOut")
        ph, pk = self._opt(hidden_wrench, f32, (B, 6), "hidden_wrench"), self._opt(force_gain, f32, (B,), "force_gain")
        self._launch(dev, lambda st: self._lib.cmpc_plant_step_vjp_mismatch_device(
            self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step), int(substeps), pg, out["state"].data_ptr(), out["x"].data_ptr(),
            out["p"].data_ptr(), out["model"].data_ptr(), out["rot0"].data_ptr() if grad_rot else None, ph, pk, out["hidden"].data_ptr(),
            out["gain"].data_ptr(), st))
        return out

    # ---- plant-step derivatives and the list path of a tick in reverse (include/cmpc.h, "plant-step derivatives") ----
    def plant_step_jvp_device(self, dX, dP, dState, dDirState, dDirX=None, dDirP=None, dDirModel=None, step=0.01, substeps=6, out=None, dDirRot0=None):
        """d(plant step) applied to one direction per problem: dDirState[B, 9] float64, dDirX[B, n_x] / dDirP[B, n_p] float32, dDirModel[B, 34]
        float64 and dDirRot0[B, 2, 3] float64 (the knot-0 rotations, dR = R [omega]x; cmpc_plant_step_jvp_rot_device) (None: zero) -> d state'[B, 9]
        float64.  What is and is not differentiated: include/cmpc.h."""
        import torch
        L, B = self.layout, self.batch
        out = _args.out(out, torch.float64, (B, 9), "out", dX.device)
        ps = self._opt(dDirState, torch.float64, (B, 9), "dDirState")
        px, pp = self._opt(dDirX, torch.float32, (B, L.nx), "dDirX"), self._opt(dDirP, torch.float32, (B, L.np), "dDirP")
        pm, po = self._opt(dDirModel, torch.float64, (B, _capi.MODEL_DOUBLES), "dDirModel"), out.data_ptr()
        if dDirRot0 is None:
            self._launch(dX.device, lambda st: self._lib.cmpc_plant_step_jvp_device(self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step),
                                                                                    int(substeps), ps, px, pp, pm, po, st))
        else:
            pr = self._opt(dDirRot0, torch.float64, (B, 2, 3), "dDirRot0")
            self._launch(dX.device, lambda st: self._lib.cmpc_plant_step_jvp_rot_device(self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step),
                                                                                        int(substeps), ps, px, pp, pm, pr, po, st))
        return out

    def plant_step_vjp_device(self, dX, dP, dState, dGradStateOut, step=0.01, substeps=6, grad_p=True, grad_model=True, grad_rot=False):
        """(d plant step)^T g: dGradStateOut[B, 9] float64 -> (dGradState[B, 9] float64, dGradX[B, n_x] float32, dGradP[B, n_p] float32 or None,
        dGradModel[B, 34] float64 or None); dGradX is zero but for the knot-0 positions and forces, dGradP but for fExt_0 / tauExt_0.
        grad_rot=True (cmpc_plant_step_vjp_rot_device): a fifth result, dGradRot0[B, 2, 3] float64 = dl / d omega of the knot-0 rotations."""
        import torch
        L, B, dev = self.layout, self.batch, dX.device
        pg = self._opt(dGradStateOut, torch.float64, (B, 9), "dGradStateOut")
        gS = torch.empty((B, 9), dtype=torch.float64, device=dev)
        gX = torch.empty((B, L.nx), dtype=torch.float32, device=dev)
        gP = torch.empty((B, L.np), dtype=torch.float32, device=dev) if grad_p else None
        gM = torch.empty((B, _capi.MODEL_DOUBLES), dtype=torch.float64, device=dev) if grad_model else None
        args = (self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step), int(substeps), pg, gS.data_ptr(), gX.data_ptr(),
                gP.data_ptr() if grad_p else None, gM.data_ptr() if grad_model else None)
        if not grad_rot:
            self._launch(dev, lambda st: self._lib.cmpc_plant_step_vjp_device(*args, st))
            return gS, gX, gP, gM
        gR = torch.empty((B, 2, 3), dtype=torch.float64, device=dev)
        self._launch(dev, lambda st: self._lib.cmpc_plant_step_vjp_rot_device(*args, gR.data_ptr(), st))
        return gS, gX, gP, gM, gR

    def _list_tape(self, M, list_t, list_n, land, plan, prev, ok):
        """the tape arguments the list-path derivatives share, as checked pointers in the C ABI's order: plan / prev = (t, n) or None, then this
        tick's list_t[B,2,M,2] float64 / list_n[B,2] int32, land[B,2] and ok[B] int32"""
        import torch
        B, f64, i32 = self.batch, torch.float64, torch.int32
        tn = lambda pair: (None, None) if pair is None else (self._opt(pair[0], f64, (B, 2, M, 2), "times"), self._opt(pair[1], i32, (B, 2), "counts"))
        return (*tn(plan), *tn(prev), ptr(list_t, f64, (B, 2, M, 2), "list_t", True), self._opt(list_n, i32, (B, 2), "list_n"),
                self._opt(land, i32, (B, 2), "land"), self._opt(ok, i32, (B,), "ok"))

    def contacts_orientation_vjp_device(self, now, list_t, list_n, land=None, plan=None, prev=None, ok=None, dGradListRotOut=None, dGradRot=None,
                                        dGradPlanRot=None, force_sample_time=False, out=None):
        """Adjoint of the list path of one tick in the contacts' orientations (cmpc_contacts_orientation_vjp_device), the counterpart of phase 2 of
        contacts_position_vjp_device with the same tape arguments.  dGradListRotOut[B,2,M,3] / dGradRot[B,2,N,3] float64 (None: zero), dGradPlanRot
        [B,2,M,3] float64 (+=, in place), all in the body-frame tangent of the quaternions.  Returns (dGradPrevListRot[B,2,M,3] float64, status[B] int32)."""
        import torch
        L, B, M, dev = self.layout, self.batch, list_t.shape[2], list_t.device
        g3 = (B, 2, M, 3)
        tape = self._list_tape(M, list_t, list_n, land, plan, prev, ok)
        gprev = _args.out(out, torch.float64, g3, "out", dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        args = (self._opt(dGradListRotOut, torch.float64, g3, "dGradListRotOut"), self._opt(dGradRot, torch.float64, (B, 2, L.N, 3), "dGradRot"),
                gprev.data_ptr(), self._opt(dGradPlanRot, torch.float64, g3, "dGradPlanRot"), status.data_ptr())
        self._launch(dev, lambda st: self._lib.cmpc_contacts_orientation_vjp_device(self._h, M, float(now), 1 if force_sample_time else 0, *tape, *args, st))
        return gprev, status

    def contacts_position_vjp_device(self, now, list_t, list_n, land, plan=None, prev=None, ok=None, dGradListOut=None, dGradP=None, dGradX=None,
                                     dGradPlan=None, phase=3, force_sample_time=False, out=None):
        """Adjoint of the list path of one tick in the contacts' positions (cmpc_contacts_position_vjp_device): list_t[B,2,M,2] float64 / list_n[B,2]
        int32 = this tick's (merged) list, plan / prev = (t, n) of the planner's and the previous tick's lists (prev None: first tick), land[B,2],
        ok[B] or None.  phase 1: the adjust part (adds to dGradX in place); 2: sample + merge; 3: both.  dGradListOut[B,2,M,3] float64, dGradP[B,n_p]
        float32, dGradPlan[B,2,M,3] float64 (+=, in place).  Returns (dGradPrevList[B,2,M,3] float64 or None for phase 1, status[B] int32 or None)."""
        import torch
        L, B, M, dev = self.layout, self.batch, list_t.shape[2], list_t.device
        g3 = (B, 2, M, 3)
        tape = self._list_tape(M, list_t, list_n, land, plan, prev, ok)
        gprev = status = None
        if phase & 2:
            gprev = _args.out(out, torch.float64, g3, "out", dev)
            status = torch.empty((B,), dtype=torch.int32, device=dev)
        args = (self._opt(dGradListOut, torch.float64, g3, "dGradListOut"), self._opt(dGradP, torch.float32, (B, L.np), "dGradP"),
                self._opt(dGradX, torch.float32, (B, L.nx), "dGradX"), opt_ptr(gprev), self._opt(dGradPlan, torch.float64, g3, "dGradPlan"), opt_ptr(status))
        self._launch(dev, lambda st: self._lib.cmpc_contacts_position_vjp_device(
            self._h, M, float(now), int(phase), 1 if force_sample_time else 0, *tape, *args, st))
        return gprev, status

    def closed_loop_transition_device(self, dX, dP, dLamG, dState, step=0.01, substeps=6):
        """A_cl[B, 9, 9] = d state' / d state of one tick (solve + plant, float64; row i = component i of state'): the nine-column JVP of
        feedback_gain_device (dx* / d(com0, dcom0, h0)) pushed column by column through the plant JVP together with the plant's own d state' / d state.
        The forward-mode cousin of rollout_tick_vjp_device.  Returns (A_cl, sens[B, CMPC_SENS]); a flagged problem's JVP columns are zero, so its A_cl is the
        plant's own."""
        import torch
        L, B = self.layout, self.batch
        dirs = torch.zeros((B, 9, L.np), dtype=torch.float32, device=dX.device)
        for i in range(9):
            dirs[:, i, L.p_com0 + i] = 1.0
        dDX, sens = self.solution_jvp_device(dX, dP, dLamG, dirs)
        A = torch.empty((B, 9, 9), dtype=torch.float64, device=dX.device)
        for i in range(9):
            e = torch.zeros((B, 9), dtype=torch.float64, device=dX.device)
            e[:, i] = 1.0
            A[:, :, i] = self.plant_step_jvp_device(dX, dP, dState, e, dDirX=dDX[:, i].contiguous(), step=step, substeps=substeps)
        return A, sens

    # ---- SURVEY 8f-1 / 8f-2 on the device (torch CUDA tensors; everything stays in HBM) ----
    def contacts_merge_device(self, now, plan, mpc, out=None):
        """updateContactPhaseList (CentroidalMPCBlock.cpp:32-110) for the batch: plan / mpc / out = (t[B,2,M,2] float64,
        pose[B,2,M,7] float32, n[B,2] int32) CUDA tensors.  Returns (out, ok[B] int32)."""
        import torch
        pt, pp, pn = plan
        mt, mp, mn = mpc
        M = pt.shape[2]
        if out is None:
            out = (torch.zeros_like(pt), torch.zeros_like(pp), torch.zeros_like(pn))
        ok = torch.empty((self.batch,), dtype=torch.int32, device=pt.device)
        self._launch(pt.device, lambda st: self._lib.cmpc_contacts_merge_device(
            self._h, M, float(now), pt.data_ptr(), pp.data_ptr(), pn.data_ptr(), mt.data_ptr(), mp.data_ptr(), mn.data_ptr(),
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ok.data_ptr(), st))
        return out, ok

    def contacts_force_sample_time_device(self, t, n, out=None, ok=None, dt=None):
        """forceSampleTime (CentroidalMPCBlock.cpp:586-592) for the batch: t[B,2,M,2] float64 / n[B,2] int32 CUDA tensors snapped to the grid of dt
        (default: the sampling time) into out (None: a new tensor; may be t itself).  Returns (out, ok[B] int32)."""
        import torch
        B = self.batch
        pt, pn = ptr(t, torch.float64, (B, 2, None, 2), "t", True), ptr(n, torch.int32, (B, 2), "n", True)
        out = _args.out(out, torch.float64, tuple(t.shape), "out", t.device)
        if ok is None:
            ok = torch.empty((B,), dtype=torch.int32, device=t.device)
        self._launch(t.device, lambda st: self._lib.cmpc_contacts_force_sample_time_device(
            self._h, t.shape[2], float(self.cfg.sampling_time if dt is None else dt), pt, pn, out.data_ptr(), ok.data_ptr(), st))
        return out, ok

    def contacts_sample_device(self, now, lists, dP, land=None):
        """setContactPhaseList for the batch: samples `lists` at now + k dt into the contact blocks of dP[B,np]; returns
        land[B,2] (landing knots)."""
        import torch
        t, pose, n = lists
        if land is None:
            land = torch.empty((self.batch, 2), dtype=torch.int32, device=dP.device)
        up, lo = self._box_arrays()
        self._launch(dP.device, lambda st: self._lib.cmpc_contacts_sample_device(
            self._h, t.shape[2], float(now), t.data_ptr(), pose.data_ptr(), n.data_ptr(), up.ctypes.data, lo.ctypes.data, dP.data_ptr(),
            land.data_ptr(), st))
        return land

    def contacts_adjust_device(self, now, dX, land, lists):
        """getOutput().contactPhaseList: the next contact of every foot landing inside the horizon takes x.pos[land] (in place)."""
        t, pose, n = lists
        self._launch(dX.device, lambda st: self._lib.cmpc_contacts_adjust_device(
            self._h, t.shape[2], float(now), dX.data_ptr(), land.data_ptr(), t.data_ptr(), pose.data_ptr(), n.data_ptr(), st))

    def write_state_device(self, dState, dP, dWrench=None):
        """setState for the batch: dState[B,9] (+ dWrench[B,N,6]) into the rows of dP."""
        self._launch(dP.device, lambda st: self._lib.cmpc_write_state_device(
            self._h, dState.data_ptr(), opt_ptr(dWrench), dP.data_ptr(), st))

    def write_reference_from_planner_device(self, dComIn, dHIn, in_dt, t_offset, robot_mass, com_height, dP):
        """setReferenceTrajectory from the planner's trajectories (8f-3) on the device: dComIn / dHIn [B, n_in, 3] float32 CUDA tensors -> comRef / hRef rows of dP."""
        import torch
        pc = ptr(dComIn, torch.float32, (self.batch, None, 3), "dComIn", True)
        ph = ptr(dHIn, torch.float32, tuple(dComIn.shape), "dHIn", True)
        self._launch(dP.device, lambda st: self._lib.cmpc_write_reference_from_planner_device(
            self._h, pc, ph, int(dComIn.shape[1]), float(in_dt), float(t_offset), float(robot_mass),
            float("nan") if com_height is None else float(com_height), dP.data_ptr(), st))

    @staticmethod
    def planner_refs(knots, dt, t_first=0.0, robot_mass=1.0, com_height=0.7):
        """a _capi.CmpcPlannerRefs (cmpc_planner_refs, include/cmpc.h); com_height None: NaN, the trajectory's own z row"""
        return _capi.CmpcPlannerRefs(int(knots), float(dt), float(t_first), float(robot_mass), float("nan") if com_height is None else float(com_height))

    def reference_from_planner_vjp_device(self, tick0, rows, refs, end_tick, grad_p, grad_com=None, grad_h=None):
        """cmpc_reference_from_planner_vjp_device: the reference rows of grad_p[rows, B, n_p] float32 (row r = tick tick0 + r; the reverse walk's grad_p)
        carried to the planner's trajectories in ONE launch: grad_com / grad_h[B, knots, 3] float64 are ADDED TO (either may be None, not both).
        refs: planner_refs(...) or a dict of its arguments; end_tick: int32 [B] (a walk record's) or None -- rows at or past a problem's end are not read."""
        import torch
        if isinstance(refs, dict):
            refs = self.planner_refs(**refs)
        B, L, n = self.batch, self.layout, int(refs.knots)
        gp = self._opt(grad_p, torch.float32, (int(rows), B, L.np), "grad_p")
        gc, gh = self._opt(grad_com, torch.float64, (B, n, 3), "grad_com"), self._opt(grad_h, torch.float64, (B, n, 3), "grad_h")
        e = self._opt(end_tick, torch.int32, (B,), "end_tick")
        self._launch(grad_p.device, lambda st: self._lib.cmpc_reference_from_planner_vjp_device(self._h, int(tick0), int(rows), C.byref(refs), e, gp, gc, gh, st))

    def reference_from_planner_jvp_device(self, tick0, rows, k, refs, dir_p, dir_com=None, dir_h=None):
        """cmpc_reference_from_planner_jvp_device: dir_com / dir_h[B, k, knots, 3] float64 (either may be None: zero, not both) -> the comRef / hRef entries of
        dir_p[rows, B, k, n_p] float32 (row r = tick tick0 + r; rollout_walk_jvp_device's dir_p), written; every other entry of dir_p is left alone."""
        import torch
        if isinstance(refs, dict):
            refs = self.planner_refs(**refs)
        B, L, n, k = self.batch, self.layout, int(refs.knots), int(k)
        dp = self._opt(dir_p, torch.float32, (int(rows), B, k, L.np), "dir_p")
        dc, dh = self._opt(dir_com, torch.float64, (B, k, n, 3), "dir_com"), self._opt(dir_h, torch.float64, (B, k, n, 3), "dir_h")
        self._launch(dir_p.device, lambda st: self._lib.cmpc_reference_from_planner_jvp_device(self._h, int(tick0), int(rows), k, C.byref(refs), dc, dh, dp, st))

    def shift_solution_device(self, dXprev, dX0):
        """is_warm_start_enabled: dX0 = dXprev shifted by one knot; solve from it with solve_device(..., warm=True)."""
        self._launch(dX0.device, lambda st: self._lib.cmpc_shift_solution_device(self._h, dXprev.data_ptr(), dX0.data_ptr(), st))


def rotate_parameters(P, rot, N):
    """P[B, n_p] float32 with every R_{c,k} replaced by float32(R_{c,k} exp([rot_{c,k}]x)) (Rodrigues, float64, on P's device); rot[B, 2, N, 3]
    float64.  A stage whose rot is zero keeps its bits."""
    import torch
    from .layout import Layout
    L = Layout(N)
    B = P.shape[0]
    w = rot.detach().to(torch.float64)
    th2 = (w * w).sum(-1, keepdim=True)
    th = th2.sqrt()
    small = th < 1e-4
    ths = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, 1.0 - th2 / 6.0, torch.sin(ths) / ths)[..., None]
    b = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(ths)) / (ths * ths))[..., None]
    K = torch.zeros((B, 2, N, 3, 3), dtype=torch.float64, device=P.device)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    E = torch.eye(3, dtype=torch.float64, device=P.device) + a * K + b * (K @ K)
    out = P.clone()
    moved = (w != 0).any(-1)                                                      # [B, 2, N]
    for c in range(2):
        blk = P[:, L.p_R[c]:L.p_R[c] + 9 * N].reshape(B, N, 3, 3)                  # column-major: [.., col, row]
        Rn = (blk.to(torch.float64).transpose(-1, -2) @ E[:, c]).transpose(-1, -2).to(torch.float32)
        out[:, L.p_R[c]:L.p_R[c] + 9 * N] = torch.where(moved[:, c, :, None, None], Rn, blk).reshape(B, 9 * N)
    return out


def solve_differentiable(solver: BatchSolver, P, X0, warm: bool = False, models=None, rot=None):
    """x*(P) as a torch.autograd.Function: forward solves (solve_device) and keeps (X, P, lam_g); backward returns P.grad by the VJP of
    include/cmpc.h (cmpc_solution_vjp_device) and None for X0.  The multiplier output of `solver` is turned on if it is off (it stays on).
    Problems whose sensitivity status is not 0 get zero rows of P.grad; solver.last_sensitivity_info holds the [B, CMPC_SENS] words of the
    last backward, and solver.last_info the [B, CMPC_INFO] words of the last forward.
    models: None, or a [B, 34] float64 CUDA tensor of per-problem models (cmpc_model's order): forward installs it with set_models_device and
    leaves it installed on `solver` (solver.last_models_ok holds the [B] ok words), and backward returns models.grad from the same adjoint solve
    (cmpc_solution_vjp_model_device: P.grad is bit for bit that of the models=None path at the same models).
    rot: None, or a [B, 2, N, 3] float64 CUDA tensor of stage rotations: forward solves with R_{c,k} <- float32(R_{c,k} exp([rot_{c,k}]x))
    (rotate_parameters; rot = 0 leaves P's bits unchanged), and backward fills rot.grad with the rotation VJP (cmpc_solution_vjp_rot_device) at the
    rotated R.  That is the gradient in the local body-frame tangent at the rotated R -- the usual retraction convention -- and the plain gradient
    at rot = 0; P.grad (and models.grad) are taken at the rotated P, bit for bit those of the rot=None path there."""
    import torch

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, P, X0, models, rot):
            solver.set_multiplier_output(True)
            if models is not None:
                solver.last_models_ok = solver.set_models_device(models.detach().contiguous())
            Pc, X0c = P.detach().contiguous(), X0.detach().contiguous()
            if rot is not None:
                Pc = rotate_parameters(Pc, rot, solver.layout.N)
            X, info = solver.solve_device(Pc, X0c, warm=warm)
            lam = solver.multipliers_device(X, Pc)
            solver.last_info = info
            ctx.with_models, ctx.with_rot = models is not None, rot is not None
            ctx.save_for_backward(X, Pc, lam)
            return X

        @staticmethod
        def backward(ctx, gX):
            X, Pc, lam = ctx.saved_tensors
            gX = gX.contiguous().to(torch.float32)
            if ctx.with_rot:
                gR, gM, gP, sens = solver.solution_vjp_rot_device(X, Pc, lam, gX, grad_model=ctx.with_models)
                solver.last_sensitivity_info = sens
                return gP, None, gM, gR
            if not ctx.with_models:
                gP, sens = solver.solution_vjp_device(X, Pc, lam, gX)
                solver.last_sensitivity_info = sens
                return gP, None, None, None
            gM, gP, sens = solver.solution_vjp_model_device(X, Pc, lam, gX)
            solver.last_sensitivity_info = sens
            return gP, None, gM, None

    return _Fn.apply(P, X0, models, rot)
