"""Host-side mirror of the reference's CentroidalMPC surface for a batch of problems.

Reference interface (BipedalLocomotion::ReducedModelControllers::CentroidalMPC, used at
src/centroidal-mpc-walking/src/CentroidalMPCBlock.cpp:144,407,579,609,615,622):
    initialize / setState / setReferenceTrajectory / setContactPhaseList / advance / getOutput
Every mutator returns bool like the reference's (False => the caller logs and aborts the tick,
CentroidalMPCBlock.cpp:609-619); `last_error` holds the text.  All compute happens in
libcmpc_hip.so (hand-written gfx950 kernels) through the C ABI of include/cmpc.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi
from .config import GRAVITY, CentroidalMPCConfig, from_ini, model_array
from .contacts import PlannedContact, pack_lists, sample_schedule, sample_schedule_batch
from .layout import Layout


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


def _upload(a, dev, dtype, hold):
    """`a` on the device in `dtype` for launches that are queued and not waited for: a torch tensor is cast as it is; anything else goes through a host
    tensor appended to `hold` and a copy the host does not wait for, so `hold` has to outlive that copy (WalkingRollout._walk_inputs, a builder
    dict's "_host")"""
    import torch
    if isinstance(a, torch.Tensor):
        return a.detach().to(dev, dtype)
    hold.append(torch.from_numpy(np.ascontiguousarray(a, str(dtype).split(".")[1])))
    return hold[-1].to(dev, non_blocking=True)


class BatchSolver:
    """Thin RAII wrapper of a cmpc_handle: device-resident batched solve."""

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
        assert dP.is_cuda and dP.dtype == torch.float32 and dP.is_contiguous() and tuple(dP.shape) == (self.batch, L.np)
        assert dX0.is_cuda and dX0.dtype == torch.float32 and dX0.is_contiguous() and tuple(dX0.shape) == (self.batch, L.nx)
        if dX is None:
            dX = torch.empty_like(dX0)
        if dInfo is None:
            dInfo = torch.empty((self.batch, _capi.INFO), dtype=torch.float32, device=dP.device)
        cur = None
        if stream is None:
            stream, cur = self._stream_pair(dP.device)
        fn = self._lib.cmpc_solve_device_warm if warm else self._lib.cmpc_solve_device
        rc = fn(self._h, dP.data_ptr(), dX0.data_ptr(), dX.data_ptr(), dInfo.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"cmpc_solve_device failed ({rc}): {self.last_error}")
        if cur is not None:
            cur.wait_stream(self._stream)
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

    @property
    def launch_stream(self):
        """torch.cuda.Stream the solve kernel runs on (record timing events here)."""
        import torch
        if self._stream is None:
            self._stream = torch.cuda.Stream(torch.device("cuda", self._device_index))
        return self._stream

    def solve_host(self, P: np.ndarray, X0: np.ndarray):
        """numpy float32 in/out through the PCIe-inclusive entry point.  Returns (X, info, rc)."""
        L = self.layout
        P = np.ascontiguousarray(P, np.float32)
        X0 = np.ascontiguousarray(X0, np.float32)
        assert P.shape == (self.batch, L.np) and X0.shape == (self.batch, L.nx)
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
        assert models.is_cuda and models.dtype == torch.float64 and models.is_contiguous() and tuple(models.shape) == (self.batch, _capi.MODEL_DOUBLES)
        if ok is None:
            ok = torch.empty((self.batch,), dtype=torch.int32, device=models.device)
        assert ok.dtype == torch.int32 and ok.is_contiguous() and ok.numel() == self.batch
        self._launch(models.device, lambda st: self._lib.cmpc_set_models_device(self._h, models.data_ptr(), ok.data_ptr(), st))
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
        if end_tick is not None:
            import torch
            assert end_tick.is_cuda and end_tick.dtype == torch.int32 and end_tick.is_contiguous() and tuple(end_tick.shape) == (self.batch,)
        rc = self._lib.cmpc_set_ended_device(self._h, end_tick.data_ptr() if end_tick is not None else None)
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
            rows = 0
            if measures is not None:
                assert measures.is_cuda and measures.dtype == torch.float32 and measures.is_contiguous() and measures.dim() == 3 and \
                    tuple(measures.shape[1:]) == (self.batch, _capi.WALK_MEASURES)
                rows = int(measures.shape[0])
            if extremes is not None:
                assert extremes.is_cuda and extremes.dtype == torch.float32 and extremes.is_contiguous() and \
                    tuple(extremes.shape) == (self.batch, _capi.WALK_EXTREMES)
            lim = _capi.CmpcWalkLimits(nan(height[0]), nan(height[1]), nan(reach_max), nan(margin_min), nan(track_max),
                                       measures.data_ptr() if measures is not None else None, rows, extremes.data_ptr() if extremes is not None else None)
            rc = self._lib.cmpc_set_walk_limits(self._h, C.byref(lim))
            if rc == 0:
                self._walk_limits = (measures, extremes)
        if rc != 0:
            raise RuntimeError(f"cmpc_set_walk_limits failed ({rc}): {self.last_error}")

    def walk_extremes_init_device(self, extremes=None, device=None):
        """cmpc_walk_extremes_init_device: extremes [B, 5] float32 (made when None) at its start -- +inf in the minima (height min, margin min), -inf in
        the maxima (height max, reach max, track max)."""
        import torch
        if extremes is None:
            dev = torch.device("cuda", self._device_index) if device is None else device
            extremes = torch.empty((self.batch, _capi.WALK_EXTREMES), dtype=torch.float32, device=dev)
        assert extremes.is_cuda and extremes.dtype == torch.float32 and extremes.is_contiguous() and tuple(extremes.shape) == (self.batch, _capi.WALK_EXTREMES)
        self._launch(extremes.device, lambda st: self._lib.cmpc_walk_extremes_init_device(self._h, extremes.data_ptr(), st))
        return extremes

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
        if out is None:
            out = torch.empty((self.batch, W), dtype=torch.float32, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, W)
        st, cur = self._stream_pair(dX.device)
        rc = self._lib.cmpc_compact_output_device(self._h, dX.data_ptr(), dInfo.data_ptr(), out.data_ptr(), st)
        if rc != 0:
            raise RuntimeError(f"cmpc_compact_output_device failed ({rc}): {self.last_error}")
        if cur is not None:
            cur.wait_stream(self._stream)
        return out

    # ---- multipliers of the reference NLP, KKT certificate, gradient of the optimal cost (include/cmpc.h) ----
    def set_multiplier_output(self, enabled: bool = True):
        """cmpc_set_multiplier_output: every later solve on this handle also keeps its dual record (what multipliers_device maps)."""
        rc = self._lib.cmpc_set_multiplier_output(self._h, 1 if enabled else 0)
        if rc != 0:
            raise RuntimeError(f"cmpc_set_multiplier_output failed ({rc}): {self.last_error}")

    def _nlp_out(self, dX, dP, dLamG, out, width, fn, name):
        import torch
        L = self.layout
        assert tuple(dX.shape) == (self.batch, L.nx) and tuple(dP.shape) == (self.batch, L.np)
        for t in (dX, dP) + ((dLamG,) if dLamG is not None else ()):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        if dLamG is not None:
            assert tuple(dLamG.shape) == (self.batch, L.ng)
        if out is None:
            out = torch.empty((self.batch, width), dtype=torch.float32, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, width) and out.dtype == torch.float32
        st, cur = self._stream_pair(dX.device)
        rc = fn(st)(out)
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc}): {self.last_error}")
        if cur is not None:
            cur.wait_stream(self._stream)
        return out

    def multipliers_device(self, dX, dP, out=None):
        """lam_g[B, n_g] of the last solve (dX, dP: its solution and parameters) in the reference's row order and IPOPT's sign convention."""
        return self._nlp_out(dX, dP, None, out, self.layout.ng,
                             lambda st: lambda o: self._lib.cmpc_get_multipliers_device(self._h, dX.data_ptr(), dP.data_ptr(), o.data_ptr(), st),
                             "cmpc_get_multipliers_device")

    def kkt_certificate_device(self, dX, dP, dLamG, out=None):
        """[B, CMPC_CERT] KKT certificate of the reference NLP at (x, lam_g): stationarity, primal infeasibility, complementarity, sign violation,
        f, status, scale, unscaled stationarity (include/cmpc.h)."""
        return self._nlp_out(dX, dP, dLamG, out, _capi.CERT,
                             lambda st: lambda o: self._lib.cmpc_kkt_certificate_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                        o.data_ptr(), st),
                             "cmpc_kkt_certificate_device")

    def value_gradient_device(self, dX, dP, dLamG, out=None):
        """dV*/dp [B, n_p] at a KKT point (x*, lam*): grad_p L plus the terms of the parameters that only enter the bounds."""
        return self._nlp_out(dX, dP, dLamG, out, self.layout.np,
                             lambda st: lambda o: self._lib.cmpc_value_gradient_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                       o.data_ptr(), st),
                             "cmpc_value_gradient_device")

    # ---- solution sensitivities dx*/dp (include/cmpc.h) ----
    def solution_jvp_device(self, dX, dP, dLamG, dDirP, out=None, sens=None):
        """dx*/dp applied to k directions: dDirP[B, k, n_p] -> (dDX[B, k, n_x], sens[B, CMPC_SENS]) at the returned point (x, p, lam_g) of a solve.
        sens = (status 0 ok / 1 non-positive pivot / 2 not finite / 3 outside the subset, relative residual, weakly active rows, largest Sigma, ...);
        a flagged problem's outputs are zero."""
        import torch
        L = self.layout
        assert dDirP.is_cuda and dDirP.dtype == torch.float32 and dDirP.is_contiguous() and dDirP.dim() == 3
        assert tuple(dDirP.shape[::2]) == (self.batch, L.np) and dDirP.shape[1] >= 1
        k = int(dDirP.shape[1])
        if out is None:
            out = torch.empty((self.batch, k, L.nx), dtype=torch.float32, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, k, L.nx) and out.dtype == torch.float32
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda st: lambda o: self._lib.cmpc_solution_jvp_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                     dDirP.data_ptr(), k, out.data_ptr(), o.data_ptr(), st),
                             "cmpc_solution_jvp_device")
        return out, sens

    def solution_vjp_device(self, dX, dP, dLamG, dGradX, out=None, sens=None):
        """(dx*/dp)^T v: dGradX[B, n_x] = dl/dx -> (dl/dp [B, n_p], sens[B, CMPC_SENS])."""
        import torch
        L = self.layout
        assert dGradX.is_cuda and dGradX.dtype == torch.float32 and dGradX.is_contiguous() and tuple(dGradX.shape) == (self.batch, L.nx)
        if out is None:
            out = torch.empty((self.batch, L.np), dtype=torch.float32, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, L.np) and out.dtype == torch.float32
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda st: lambda o: self._lib.cmpc_solution_vjp_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                     dGradX.data_ptr(), out.data_ptr(), o.data_ptr(), st),
                             "cmpc_solution_vjp_device")
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
        assert dDirP is not None or dDirModel is not None, "solution_jvp_model_device: no direction"
        if dDirP is not None:
            assert dDirP.is_cuda and dDirP.dtype == torch.float32 and dDirP.is_contiguous() and dDirP.dim() == 3
            assert tuple(dDirP.shape[::2]) == (self.batch, L.np) and dDirP.shape[1] >= 1
        if dDirModel is not None:
            assert dDirModel.is_cuda and dDirModel.dtype == torch.float64 and dDirModel.is_contiguous() and dDirModel.dim() == 3
            assert tuple(dDirModel.shape[::2]) == (self.batch, _capi.MODEL_DOUBLES) and dDirModel.shape[1] >= 1
            assert dDirP is None or dDirP.shape[1] == dDirModel.shape[1]
        k = int((dDirP if dDirP is not None else dDirModel).shape[1])
        if out is None:
            out = torch.empty((self.batch, k, L.nx), dtype=torch.float32, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, k, L.nx) and out.dtype == torch.float32
        pp = dDirP.data_ptr() if dDirP is not None else None
        pm = dDirModel.data_ptr() if dDirModel is not None else None
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda st: lambda o: self._lib.cmpc_solution_jvp_model_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                           pp, pm, k, out.data_ptr(), o.data_ptr(), st),
                             "cmpc_solution_jvp_model_device")
        return out, sens

    def solution_vjp_model_device(self, dX, dP, dLamG, dGradX, out_model=None, out_p=None, sens=None, grad_p=True):
        """(dx*/d(p, theta))^T v from one adjoint solve: dGradX[B, n_x] = dl/dx -> (dl/dtheta [B, 34] float64, dl/dp [B, n_p] float32 or None
        when grad_p is False, sens[B, CMPC_SENS]).  dl/dp equals solution_vjp_device's bit for bit; sens[:, 6]: the largest relative component
        along the internal-force direction over the 34 fields."""
        import torch
        L = self.layout
        assert dGradX.is_cuda and dGradX.dtype == torch.float32 and dGradX.is_contiguous() and tuple(dGradX.shape) == (self.batch, L.nx)
        if out_model is None:
            out_model = torch.empty((self.batch, _capi.MODEL_DOUBLES), dtype=torch.float64, device=dX.device)
        assert out_model.is_contiguous() and tuple(out_model.shape) == (self.batch, _capi.MODEL_DOUBLES) and out_model.dtype == torch.float64
        if grad_p and out_p is None:
            out_p = torch.empty((self.batch, L.np), dtype=torch.float32, device=dX.device)
        if out_p is not None:
            assert out_p.is_contiguous() and tuple(out_p.shape) == (self.batch, L.np) and out_p.dtype == torch.float32
        pp = out_p.data_ptr() if out_p is not None else None
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda st: lambda o: self._lib.cmpc_solution_vjp_model_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                           dGradX.data_ptr(), pp, out_model.data_ptr(), o.data_ptr(), st),
                             "cmpc_solution_vjp_model_device")
        return out_model, out_p, sens

    def model_value_gradient_device(self, dX, dP, dLamG, out=None):
        """dV*/dtheta [B, 34] float64 at a KKT point (x*, lam*): d_theta f + lam^T d_theta g, at each problem's own model (zeros for a row whose model
        broke the model rule).  At a double-support point the corner entries depend on the internal force the solve returned (include/cmpc.h)."""
        import torch
        L = self.layout
        assert tuple(dX.shape) == (self.batch, L.nx) and tuple(dP.shape) == (self.batch, L.np) and tuple(dLamG.shape) == (self.batch, L.ng)
        for t in (dX, dP, dLamG):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        if out is None:
            out = torch.empty((self.batch, _capi.MODEL_DOUBLES), dtype=torch.float64, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, _capi.MODEL_DOUBLES) and out.dtype == torch.float64
        self._launch(dX.device, lambda st: self._lib.cmpc_model_value_gradient_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                      out.data_ptr(), st))
        return out

    # ---- derivatives with respect to the stage rotations (include/cmpc.h, "rotation directions") ----
    def solution_jvp_rot_device(self, dX, dP, dLamG, dDirP=None, dDirModel=None, dDirRot=None, out=None, sens=None):
        """dx*/d(p, theta, omega) applied to k directions: dDirP[B, k, n_p] float32, dDirModel[B, k, 34] float64 and dDirRot[B, k, 2, N, 3] float64
        (omega moves R_{c,k} along R [omega]x; any may be None: zero) -> (dDX[B, k, n_x], sens[B, CMPC_SENS]).  sens[:, 6]: the largest relative
        component of the model and rotation right-hand sides along the internal-force direction that was removed.  dDirRot None gives
        solution_jvp_model_device's result bit for bit."""
        import torch
        L = self.layout
        shapes = ((dDirP, torch.float32, (L.np,)), (dDirModel, torch.float64, (_capi.MODEL_DOUBLES,)), (dDirRot, torch.float64, (2, L.N, 3)))
        ks = set()
        for t, dt, tail in shapes:
            if t is not None:
                assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.dim() == 2 + len(tail)
                assert t.shape[0] == self.batch and tuple(t.shape[2:]) == tail and t.shape[1] >= 1
                ks.add(int(t.shape[1]))
        assert len(ks) == 1, "solution_jvp_rot_device: no direction, or directions of different k"
        k = ks.pop()
        if out is None:
            out = torch.empty((self.batch, k, L.nx), dtype=torch.float32, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, k, L.nx) and out.dtype == torch.float32
        pp, pm, pr = (t.data_ptr() if t is not None else None for t in (dDirP, dDirModel, dDirRot))
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda st: lambda o: self._lib.cmpc_solution_jvp_rot_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                         pp, pm, pr, k, out.data_ptr(), o.data_ptr(), st),
                             "cmpc_solution_jvp_rot_device")
        return out, sens

    def solution_vjp_rot_device(self, dX, dP, dLamG, dGradX, out_rot=None, out_model=None, out_p=None, sens=None, grad_p=True, grad_model=True):
        """(dx*/d(p, theta, omega))^T v from one adjoint solve: dGradX[B, n_x] = dl/dx -> (dl/domega [B, 2, N, 3] float64, dl/dtheta [B, 34]
        float64 or None, dl/dp [B, n_p] float32 or None, sens[B, CMPC_SENS]).  dl/dp and dl/dtheta equal solution_vjp_model_device's bit for bit."""
        import torch
        L = self.layout
        assert dGradX.is_cuda and dGradX.dtype == torch.float32 and dGradX.is_contiguous() and tuple(dGradX.shape) == (self.batch, L.nx)
        if out_rot is None:
            out_rot = torch.empty((self.batch, 2, L.N, 3), dtype=torch.float64, device=dX.device)
        assert out_rot.is_contiguous() and tuple(out_rot.shape) == (self.batch, 2, L.N, 3) and out_rot.dtype == torch.float64
        if grad_model and out_model is None:
            out_model = torch.empty((self.batch, _capi.MODEL_DOUBLES), dtype=torch.float64, device=dX.device)
        if out_model is not None:
            assert out_model.is_contiguous() and tuple(out_model.shape) == (self.batch, _capi.MODEL_DOUBLES) and out_model.dtype == torch.float64
        if grad_p and out_p is None:
            out_p = torch.empty((self.batch, L.np), dtype=torch.float32, device=dX.device)
        if out_p is not None:
            assert out_p.is_contiguous() and tuple(out_p.shape) == (self.batch, L.np) and out_p.dtype == torch.float32
        pp = out_p.data_ptr() if out_p is not None else None
        pm = out_model.data_ptr() if out_model is not None else None
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda st: lambda o: self._lib.cmpc_solution_vjp_rot_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                         dGradX.data_ptr(), pp, pm, out_rot.data_ptr(), o.data_ptr(), st),
                             "cmpc_solution_vjp_rot_device")
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
        assert grad_p or grad_model or grad_rot, "solution_vjp_cols_device: no output requested"
        assert dGradX.dim() == 3, "solution_vjp_cols_device: dGradX is [B, k, n_x]"
        assert dGradX.dtype == torch.float32, "solution_vjp_cols_device: dGradX is float32"
        assert dGradX.is_cuda and dGradX.is_contiguous() and tuple(dGradX.shape[::2]) == (self.batch, L.nx) and dGradX.shape[1] >= 1
        k = int(dGradX.shape[1])
        outs = []
        for want, out, dt, tail in ((grad_p, out_p, torch.float32, (L.np,)), (grad_model, out_model, torch.float64, (_capi.MODEL_DOUBLES,)),
                                    (grad_rot, out_rot, torch.float64, (2, L.N, 3))):
            if want and out is None:
                out = torch.empty((self.batch, k) + tail, dtype=dt, device=dX.device)
            if not want:
                out = None
            if out is not None:
                assert out.is_contiguous() and tuple(out.shape) == (self.batch, k) + tail and out.dtype == dt
            outs.append(out)
        pp, pm, pr = (t.data_ptr() if t is not None else None for t in outs)
        sens = self._nlp_out(dX, dP, dLamG, sens, _capi.SENS,
                             lambda st: lambda o: self._lib.cmpc_solution_vjp_cols_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                          dGradX.data_ptr(), k, pp, pm, pr, o.data_ptr(), st),
                             "cmpc_solution_vjp_cols_device")
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
        assert rows.size >= 1 and rows.min() >= 0 and rows.max() < L.nx, "policy_jacobian_device: rows index x"
        V = torch.zeros((self.batch, rows.size, L.nx), dtype=torch.float32, device=dX.device)
        V[:, torch.arange(rows.size, device=dX.device), torch.as_tensor(rows, device=dX.device)] = 1.0
        return self.solution_vjp_cols_device(dX, dP, dLamG, V, grad_p=True, grad_model=model, grad_rot=rot)

    def rotation_value_gradient_device(self, dX, dP, dLamG, out=None):
        """dV*/domega [B, 2, N, 3] float64 at a KKT point (x*, lam*): lam^T d_omega g (the cost does not depend on R).  At a double-support point
        the entries depend on the internal force the solve returned (include/cmpc.h)."""
        import torch
        L = self.layout
        assert tuple(dX.shape) == (self.batch, L.nx) and tuple(dP.shape) == (self.batch, L.np) and tuple(dLamG.shape) == (self.batch, L.ng)
        for t in (dX, dP, dLamG):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        if out is None:
            out = torch.empty((self.batch, 2, L.N, 3), dtype=torch.float64, device=dX.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.batch, 2, L.N, 3) and out.dtype == torch.float64
        self._launch(dX.device, lambda st: self._lib.cmpc_rotation_value_gradient_device(self._h, dX.data_ptr(), dP.data_ptr(), dLamG.data_ptr(),
                                                                                         out.data_ptr(), st))
        return out

    def contacts_rotation_vjp_device(self, now, list_t, list_n, dGradRot, out=None):
        """Per-stage -> per-list-entry (cmpc_contacts_rotation_vjp_device): list_t[B,2,M,2] float64 / list_n[B,2] int32 = the sampled lists,
        dGradRot[B,2,N,3] float64 -> dGradListRot[B,2,M,3] float64: entry m receives the sum of dGradRot over the stages it owns, in the body-frame
        tangent of its quaternion (q <- q (x) exp(omega / 2))."""
        import torch
        L, B, M, dev = self.layout, self.batch, list_t.shape[2], list_t.device
        assert list_t.is_cuda and list_t.dtype == torch.float64 and list_t.is_contiguous() and tuple(list_t.shape) == (B, 2, M, 2)
        if out is None:
            out = torch.empty((B, 2, M, 3), dtype=torch.float64, device=dev)
        args = (self._opt(list_n, torch.int32, (B, 2), "list_n"), self._opt(dGradRot, torch.float64, (B, 2, L.N, 3), "dGradRot"),
                self._opt(out, torch.float64, (B, 2, M, 3), "out"))
        self._launch(dev, lambda st: self._lib.cmpc_contacts_rotation_vjp_device(self._h, M, float(now), list_t.data_ptr(), *args, st))
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
        st, cur = self._stream_pair(dState.device)
        rc = self._lib.cmpc_plant_step_device(self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), dStateOut.data_ptr(),
                                              dZmp.data_ptr(), float(step), int(substeps), float(zmp_half_x), float(zmp_half_y), st)
        if rc != 0:
            raise RuntimeError(f"cmpc_plant_step_device failed ({rc}): {self.last_error}")
        if cur is not None:
            cur.wait_stream(self._stream)
        return dStateOut, dZmp


    # ---- plant-model mismatch (include/cmpc.h, "plant-model mismatch on the device walk"; DESIGN.md 7f, "Mismatch") ----
    def plant_mismatch(self, hidden_wrench=None, state_noise=None, force_gain=None, tick_first=0, device=None):
        """A cmpc_plant_mismatch as a dict: hidden_wrench[Th, B, 6], state_noise[Tn, B, 9], force_gain[B] float32 (numpy or CUDA tensors, any subset; a
        schedule of zero rows counts as absent), tick_first the tick number of row 0 of the two schedules.  The dict keeps the device tensors alive and holds
        "_c", the C struct that points at them."""
        import torch
        B = self.batch
        dev = torch.device("cuda", self._device_index) if device is None else device
        hold = []

        def up(a, tail, name):
            if a is None:
                return None
            if not isinstance(a, torch.Tensor):    # (uploaded without the host waiting for the copy; the host array is kept with the dict)
                hold.append(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
                a = hold[-1].to(dev, non_blocking=True)
            t = a
            t = t.detach().to(dev, torch.float32).contiguous()
            assert tuple(t.shape[-len(tail):]) == tuple(tail) and t.dim() == len(tail) + (0 if name == "force_gain" else 1), f"{name}: expected [.., {tail}]"
            return t if t.numel() > 0 else None
        m = dict(hidden_wrench=up(hidden_wrench, (B, 6), "hidden_wrench"), state_noise=up(state_noise, (B, 9), "state_noise"),
                 force_gain=up(force_gain, (B,), "force_gain"), tick_first=int(tick_first))
        ptr = lambda t: None if t is None else t.data_ptr()
        rows = lambda t: 0 if t is None else int(t.shape[0])
        m["_host"] = hold
        m["_c"] = _capi.CmpcPlantMismatch(int(tick_first), ptr(m["hidden_wrench"]), rows(m["hidden_wrench"]), ptr(m["state_noise"]), rows(m["state_noise"]),
                                          ptr(m["force_gain"]))
        return m

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

    # ---- the roll-out tick in reverse (include/cmpc.h, "plant-step derivatives" and "the roll-out tick in reverse") ----
    def _opt(self, t, dtype, shape, name):
        """data_ptr of an optional CUDA tensor (None -> NULL), checked"""
        if t is None:
            return None
        assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape), f"{name}: expected {dtype} {tuple(shape)}"
        return t.data_ptr()

    def plant_step_jvp_device(self, dX, dP, dState, dDirState, dDirX=None, dDirP=None, dDirModel=None, step=0.01, substeps=6, out=None, dDirRot0=None):
        """d(plant step) applied to one direction per problem: dDirState[B, 9] float64, dDirX[B, n_x] / dDirP[B, n_p] float32, dDirModel[B, 34]
        float64 and dDirRot0[B, 2, 3] float64 (the knot-0 rotations, dR = R [omega]x; cmpc_plant_step_jvp_rot_device) (None: zero) -> d state'[B, 9]
        float64.  What is and is not differentiated: include/cmpc.h."""
        import torch
        L, B = self.layout, self.batch
        if out is None:
            out = torch.empty((B, 9), dtype=torch.float64, device=dX.device)
        ps = self._opt(dDirState, torch.float64, (B, 9), "dDirState")
        px, pp = self._opt(dDirX, torch.float32, (B, L.nx), "dDirX"), self._opt(dDirP, torch.float32, (B, L.np), "dDirP")
        pm, po = self._opt(dDirModel, torch.float64, (B, _capi.MODEL_DOUBLES), "dDirModel"), self._opt(out, torch.float64, (B, 9), "out")
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

    def contacts_orientation_vjp_device(self, now, list_t, list_n, land=None, plan=None, prev=None, ok=None, dGradListRotOut=None, dGradRot=None,
                                        dGradPlanRot=None, force_sample_time=False, out=None):
        """Adjoint of the list path of one tick in the contacts' orientations (cmpc_contacts_orientation_vjp_device), the counterpart of phase 2 of
        contacts_position_vjp_device with the same tape arguments.  dGradListRotOut[B,2,M,3] / dGradRot[B,2,N,3] float64 (None: zero), dGradPlanRot
        [B,2,M,3] float64 (+=, in place), all in the body-frame tangent of the quaternions.  Returns (dGradPrevListRot[B,2,M,3] float64, status[B] int32)."""
        import torch
        L, B, M, dev = self.layout, self.batch, list_t.shape[2], list_t.device
        g3 = (B, 2, M, 3)
        assert list_t.is_cuda and list_t.dtype == torch.float64 and list_t.is_contiguous() and tuple(list_t.shape) == (B, 2, M, 2)
        gprev = out if out is not None else torch.empty(g3, dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        tn = lambda pair: (None, None) if pair is None else (self._opt(pair[0], torch.float64, (B, 2, M, 2), "times"), self._opt(pair[1], torch.int32, (B, 2), "counts"))
        (plt, pln), (pvt, pvn) = tn(plan), tn(prev)
        args = (self._opt(list_n, torch.int32, (B, 2), "list_n"), self._opt(land, torch.int32, (B, 2), "land"), self._opt(ok, torch.int32, (B,), "ok"),
                self._opt(dGradListRotOut, torch.float64, g3, "dGradListRotOut"), self._opt(dGradRot, torch.float64, (B, 2, L.N, 3), "dGradRot"),
                self._opt(gprev, torch.float64, g3, "out"), self._opt(dGradPlanRot, torch.float64, g3, "dGradPlanRot"), status.data_ptr())
        self._launch(dev, lambda st: self._lib.cmpc_contacts_orientation_vjp_device(
            self._h, M, float(now), 1 if force_sample_time else 0, plt, pln, pvt, pvn, list_t.data_ptr(), *args, st))
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
        assert list_t.is_cuda and list_t.dtype == torch.float64 and list_t.is_contiguous() and tuple(list_t.shape) == (B, 2, M, 2)
        gprev = status = None
        if phase & 2:
            gprev = out if out is not None else torch.empty(g3, dtype=torch.float64, device=dev)
            status = torch.empty((B,), dtype=torch.int32, device=dev)
        tn = lambda pair: (None, None) if pair is None else (self._opt(pair[0], torch.float64, (B, 2, M, 2), "times"), self._opt(pair[1], torch.int32, (B, 2), "counts"))
        (plt, pln), (pvt, pvn) = tn(plan), tn(prev)
        args = (self._opt(list_n, torch.int32, (B, 2), "list_n"), self._opt(land, torch.int32, (B, 2), "land"), self._opt(ok, torch.int32, (B,), "ok"),
                self._opt(dGradListOut, torch.float64, g3, "dGradListOut"), self._opt(dGradP, torch.float32, (B, L.np), "dGradP"),
                self._opt(dGradX, torch.float32, (B, L.nx), "dGradX"), self._opt(gprev, torch.float64, g3, "out"),
                self._opt(dGradPlan, torch.float64, g3, "dGradPlan"), status.data_ptr() if status is not None else None)
        self._launch(dev, lambda st: self._lib.cmpc_contacts_position_vjp_device(
            self._h, M, float(now), int(phase), 1 if force_sample_time else 0, plt, pln, pvt, pvn, list_t.data_ptr(), *args, st))
        return gprev, status

    def rollout_tick_vjp_device(self, now, tape, dGradStateOut, dGradListOut=None, dGradX=None, dGradPlan=None, dGradModel=None, wrench=True, grad_p=False,
                                dGradListRotOut=None, rot=False, dGradPlanRot=None, mismatch=False, hidden_wrench=None, force_gain=None, dGradGain=None):
        """cmpc_rollout_tick_vjp_device: one tick in reverse.  tape: dict(X, P, lam_g, state, info, ok (or None), land, plan_t, plan_n, prev_t, prev_n
        (both None on the first tick), list_t, list_n, step, substeps, force_sample_time) of CUDA tensors as the forward tick left them.
        dGradStateOut[B,9] float64, dGradListOut[B,2,M,3] float64 or None, dGradX[B,n_x] float32 or None; dGradPlan / dGradModel: float64 tensors added to
        in place, or None.  Returns dict(state[B,9], prev_list[B,2,M,3] float64, wrench[B,N,6] float32 or None, p[B,n_p] float32 or None,
        sens[B,CMPC_SENS] float32 with the tick's status in word 0).
        rot=True (cmpc_rollout_tick_vjp_rot_device): the contacts' orientations are carried along, in the body-frame tangent of their quaternions --
        dGradListRotOut[B,2,M,3] float64 or None, dGradPlanRot[B,2,M,3] float64 added to in place or None; the dict also holds prev_list_rot[B,2,M,3] and
        rot[B,2,N,3] float64 (the tick's per-stage dl/domega: the solve's, plus the plant's on stage 0), every other entry bit-equal to rot=False but
        sens, which is the rotation VJP's.
        mismatch=True (cmpc_rollout_tick_vjp_mismatch_device; with or without rot): the tick ran under hidden_wrench[B,6] / force_gain[B] float32 (its own
        rows; None: not applied) and tape["state"] is the TRUE state; the dict also holds hidden[B,6] float64 and noise[B,9] float32, and dGradGain[B]
        float64 (or None) is added to in place."""
        import torch
        from ._capi import CmpcTickTape
        L, B, N = self.layout, self.batch, self.cfg.N
        lt = tape["list_t"]
        M, dev = lt.shape[2], lt.device
        g3 = (B, 2, M, 3)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        tt, tn = (B, 2, M, 2), (B, 2)
        ct = CmpcTickTape(self._opt(tape["X"], f32, (B, L.nx), "X"), self._opt(tape["P"], f32, (B, L.np), "P"), self._opt(tape["lam_g"], f32, (B, L.ng), "lam_g"),
                          self._opt(tape["state"], f32, (B, 9), "state"), self._opt(tape["info"], f32, (B, _capi.INFO), "info"),
                          self._opt(tape.get("ok"), i32, (B,), "ok"), self._opt(tape["land"], i32, tn, "land"),
                          self._opt(tape.get("plan_t"), f64, tt, "plan_t"), self._opt(tape.get("plan_n"), i32, tn, "plan_n"),
                          self._opt(tape.get("prev_t"), f64, tt, "prev_t"), self._opt(tape.get("prev_n"), i32, tn, "prev_n"),
                          self._opt(lt, f64, tt, "list_t"), self._opt(tape["list_n"], i32, tn, "list_n"),
                          float(tape["step"]), int(tape["substeps"]), 1 if tape.get("force_sample_time") else 0)
        out = dict(state=torch.empty((B, 9), dtype=f64, device=dev), prev_list=torch.empty(g3, dtype=f64, device=dev),
                   wrench=torch.empty((B, N, 6), dtype=f32, device=dev) if wrench else None,
                   p=torch.empty((B, L.np), dtype=f32, device=dev) if grad_p else None, sens=torch.empty((B, _capi.SENS), dtype=f32, device=dev))
        args = (self._opt(dGradStateOut, f64, (B, 9), "dGradStateOut"), self._opt(dGradListOut, f64, g3, "dGradListOut"),
                self._opt(dGradX, f32, (B, L.nx), "dGradX"), out["state"].data_ptr(), out["prev_list"].data_ptr(),
                out["wrench"].data_ptr() if wrench else None, self._opt(dGradPlan, f64, g3, "dGradPlan"),
                self._opt(dGradModel, f64, (B, _capi.MODEL_DOUBLES), "dGradModel"), out["p"].data_ptr() if grad_p else None, out["sens"].data_ptr())
        margs = None
        if mismatch:
            out["hidden"] = torch.empty((B, 6), dtype=f64, device=dev)
            out["noise"] = torch.empty((B, 9), dtype=f32, device=dev)
            margs = (self._opt(hidden_wrench, f32, (B, 6), "hidden_wrench"), self._opt(force_gain, f32, (B,), "force_gain"), out["hidden"].data_ptr(),
                     out["noise"].data_ptr(), self._opt(dGradGain, f64, (B,), "dGradGain"))
        else:
            assert hidden_wrench is None and force_gain is None and dGradGain is None, "mismatch arguments need mismatch=True"
        if not rot:
            assert dGradListRotOut is None and dGradPlanRot is None, "orientation gradients need rot=True"
            if mismatch:
                self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_mismatch_device(self._h, M, float(now), ct, *args, None, None, None, None, *margs, st))
            else:
                self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_device(self._h, M, float(now), ct, *args, st))
            return out
        out["prev_list_rot"] = torch.empty(g3, dtype=f64, device=dev)
        out["rot"] = torch.empty((B, 2, N, 3), dtype=f64, device=dev)
        rargs = (self._opt(dGradListRotOut, f64, g3, "dGradListRotOut"), out["prev_list_rot"].data_ptr(), self._opt(dGradPlanRot, f64, g3, "dGradPlanRot"),
                 out["rot"].data_ptr())
        if mismatch:
            self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_mismatch_device(self._h, M, float(now), ct, *args, *rargs, *margs, st))
        else:
            self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_vjp_rot_device(self._h, M, float(now), ct, *args, *rargs, st))
        return out

    # ---- the roll-out tick forwards, in k directions (include/cmpc.h, "the roll-out tick FORWARDS") ----
    def plant_step_jvp_cols_device(self, dX, dP, dState, dDirState, dDirX=None, dDirP=None, dDirModel=None, dDirRot0=None, step=0.01, substeps=6, out=None):
        """cmpc_plant_step_jvp_cols_device: plant_step_jvp_device with k columns per problem -- dDirState[B, k, 9] float64, dDirX[B, k, n_x] /
        dDirP[B, k, n_p] float32, dDirModel[B, k, 34] and dDirRot0[B, k, 2, 3] float64 (None: zero) -> d state'[B, k, 9] float64; column j is bit-equal to
        plant_step_jvp_device on column j."""
        import torch
        L, B = self.layout, self.batch
        assert dDirState.dim() == 3
        k = int(dDirState.shape[1])
        if out is None:
            out = torch.empty((B, k, 9), dtype=torch.float64, device=dX.device)
        args = (self._opt(dDirState, torch.float64, (B, k, 9), "dDirState"), self._opt(dDirX, torch.float32, (B, k, L.nx), "dDirX"),
                self._opt(dDirP, torch.float32, (B, k, L.np), "dDirP"), self._opt(dDirModel, torch.float64, (B, k, _capi.MODEL_DOUBLES), "dDirModel"),
                self._opt(dDirRot0, torch.float64, (B, k, 2, 3), "dDirRot0"), self._opt(out, torch.float64, (B, k, 9), "out"))
        self._launch(dX.device, lambda st: self._lib.cmpc_plant_step_jvp_cols_device(self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step),
                                                                                     int(substeps), k, *args, st))
        return out

    def plant_step_jvp_mismatch_cols_device(self, dX, dP, dState, dDirState, dDirX=None, dDirP=None, dDirModel=None, dDirRot0=None, hidden_wrench=None,
                                            force_gain=None, dDirHidden=None, dDirGain=None, step=0.01, substeps=6, out=None):
        """cmpc_plant_step_jvp_mismatch_cols_device: plant_step_jvp_cols_device at the mismatched plant (hidden_wrench[B, 6], force_gain[B] float32 or
        None) with the directions dDirHidden[B, k, 6] and dDirGain[B, k] float64 (None: zero) -> d state'[B, k, 9] float64.  All four None: the call
        above, bit for bit; column j is bit-equal to a k = 1 call on column j."""
        import torch
        L, B = self.layout, self.batch
        assert dDirState.dim() == 3
        k = int(dDirState.shape[1])
        f32, f64 = torch.float32, torch.float64
        if out is None:
            out = torch.empty((B, k, 9), dtype=f64, device=dX.device)
        args = (self._opt(dDirState, f64, (B, k, 9), "dDirState"), self._opt(dDirX, f32, (B, k, L.nx), "dDirX"), self._opt(dDirP, f32, (B, k, L.np), "dDirP"),
                self._opt(dDirModel, f64, (B, k, _capi.MODEL_DOUBLES), "dDirModel"), self._opt(dDirRot0, f64, (B, k, 2, 3), "dDirRot0"),
                self._opt(hidden_wrench, f32, (B, 6), "hidden_wrench"), self._opt(force_gain, f32, (B,), "force_gain"),
                self._opt(dDirHidden, f64, (B, k, 6), "dDirHidden"), self._opt(dDirGain, f64, (B, k), "dDirGain"), self._opt(out, f64, (B, k, 9), "out"))
        self._launch(dX.device, lambda st: self._lib.cmpc_plant_step_jvp_mismatch_cols_device(
            self._h, dX.data_ptr(), dP.data_ptr(), dState.data_ptr(), float(step), int(substeps), k, *args, st))
        return out

    def contacts_jvp_device(self, now, list_t, list_n, land, k, plan=None, prev=None, ok=None, dDirPrevList=None, dDirPrevListRot=None, dDirPlan=None,
                            dDirPlanRot=None, dDirX=None, phase=3, force_sample_time=False, out=None, out_rot=None, dDirP=None, rot=True):
        """The list path of one tick forwards (cmpc_contacts_jvp_device), the transpose of contacts_position_vjp_device + contacts_orientation_vjp_device
        with their tape arguments: directions [B, k, 2, M, 3] float64 of the previous list's and the planner's positions and orientations (None: zero),
        dDirX[B, k, n_x] float32 (phase bit 2: the landing entry takes the solution's direction).  phase 1: merge + sample; 2: adjust (out / out_rot
        are then the phase-1 results, updated in place); 3: both.  -> dict(list, list_rot [B, k, 2, M, 3] float64, p[B, k, n_p] float32 (dDirP or a
        zero tensor: only the nominalPos / currentPos rows are written), rot[B, k, 2, N, 3] float64 (rot=False: None), status[B] int32)."""
        import torch
        L, B, M, dev = self.layout, self.batch, list_t.shape[2], list_t.device
        g3 = (B, k, 2, M, 3)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        assert list_t.is_cuda and list_t.dtype == f64 and list_t.is_contiguous() and tuple(list_t.shape) == (B, 2, M, 2)
        res = dict(list=out if out is not None else torch.zeros(g3, dtype=f64, device=dev),
                   list_rot=out_rot if out_rot is not None else torch.zeros(g3, dtype=f64, device=dev), p=None, rot=None,
                   status=torch.empty((B,), dtype=i32, device=dev))
        if phase & 1:
            res["p"] = dDirP if dDirP is not None else torch.zeros((B, k, L.np), dtype=f32, device=dev)
            res["rot"] = torch.empty((B, k, 2, L.N, 3), dtype=f64, device=dev) if rot else None
        tn = lambda pair: (None, None) if pair is None else (self._opt(pair[0], f64, (B, 2, M, 2), "times"), self._opt(pair[1], i32, (B, 2), "counts"))
        (plt, pln), (pvt, pvn) = tn(plan), tn(prev)
        args = (self._opt(list_n, i32, (B, 2), "list_n"), self._opt(land, i32, (B, 2), "land"), self._opt(ok, i32, (B,), "ok"),
                self._opt(dDirPrevList, f64, g3, "dDirPrevList"), self._opt(dDirPrevListRot, f64, g3, "dDirPrevListRot"),
                self._opt(dDirPlan, f64, g3, "dDirPlan"), self._opt(dDirPlanRot, f64, g3, "dDirPlanRot"), self._opt(dDirX, f32, (B, k, L.nx), "dDirX"),
                self._opt(res["list"], f64, g3, "out"), self._opt(res["list_rot"], f64, g3, "out_rot"), self._opt(res["p"], f32, (B, k, L.np), "dDirP"),
                self._opt(res["rot"], f64, (B, k, 2, L.N, 3), "rot"), res["status"].data_ptr())
        self._launch(dev, lambda st: self._lib.cmpc_contacts_jvp_device(
            self._h, M, float(now), int(phase), 1 if force_sample_time else 0, int(k), plt, pln, pvt, pvn, list_t.data_ptr(), *args, st))
        return res

    def rollout_tick_jvp_device(self, now, tape, k, dDirState=None, dDirPrevList=None, dDirPrevListRot=None, dDirPlan=None, dDirPlanRot=None, dDirWrench=None,
                                dDirModel=None, dDirP=None, x=False, rot=False, p_full=False, out_state=None):
        """cmpc_rollout_tick_jvp_device: one tick forwards in k directions (arguments and the returned dict: _rollout_tick_jvp)."""
        return self._rollout_tick_jvp(now, tape, k, dDirState, dDirPrevList, dDirPrevListRot, dDirPlan, dDirPlanRot, dDirWrench, dDirModel, dDirP, x, rot,
                                      p_full, out_state, None)

    def rollout_tick_jvp_mismatch_device(self, now, tape, k, hidden_wrench=None, force_gain=None, dDirHidden=None, dDirNoise=None, dDirGain=None,
                                         dDirState=None, dDirPrevList=None, dDirPrevListRot=None, dDirPlan=None, dDirPlanRot=None, dDirWrench=None,
                                         dDirModel=None, dDirP=None, x=False, rot=False, p_full=False, out_state=None):
        """cmpc_rollout_tick_jvp_mismatch_device: rollout_tick_jvp_device on a tick that ran under a mismatch -- hidden_wrench[B, 6] / force_gain[B]
        float32 are the tick's own rows (None: not applied), dDirHidden[B, k, 6] / dDirGain[B, k] float64 and dDirNoise[B, k, 9] float32 the mismatch
        directions (None: zero).  The noise direction enters the solve only.  All five None: rollout_tick_jvp_device, bit for bit."""
        return self._rollout_tick_jvp(now, tape, k, dDirState, dDirPrevList, dDirPrevListRot, dDirPlan, dDirPlanRot, dDirWrench, dDirModel, dDirP, x, rot,
                                      p_full, out_state, (hidden_wrench, force_gain, dDirHidden, dDirNoise, dDirGain))

    def _rollout_tick_jvp(self, now, tape, k, dDirState, dDirPrevList, dDirPrevListRot, dDirPlan, dDirPlanRot, dDirWrench, dDirModel, dDirP, x, rot, p_full,
                          out_state, mm):
        """cmpc_rollout_tick_jvp_device: one tick forwards in k directions, on the tape of rollout_tick_vjp_device.  Directions (each None: zero), with the
        column axis behind the batch axis: dDirState[B,k,9], dDirPrevList / dDirPrevListRot / dDirPlan / dDirPlanRot[B,k,2,M,3], dDirModel[B,k,34] float64;
        dDirWrench[B,k,N,6], dDirP[B,k,n_p] float32.  Returns dict(state[B,k,9], list[B,k,2,M,3], list_rot[B,k,2,M,3] float64, x[B,k,n_x] float32 (x=True),
        rot[B,k,2,N,3] float64 (rot=True), p[B,k,n_p] float32 (p_full=True: the assembled p direction), sens[B,CMPC_SENS] float32 with the tick's status
        in word 0) -- the keys of rollout_tick_vjp_device's dict, each holding the direction of what that one holds the gradient of."""
        import torch
        from ._capi import CmpcTickDirs, CmpcTickDirsOut, CmpcTickTape
        L, B, N = self.layout, self.batch, self.cfg.N
        lt = tape["list_t"]
        M, dev = lt.shape[2], lt.device
        k = int(k)
        g3 = (B, k, 2, M, 3)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        tt, tn = (B, 2, M, 2), (B, 2)
        ct = CmpcTickTape(self._opt(tape["X"], f32, (B, L.nx), "X"), self._opt(tape["P"], f32, (B, L.np), "P"), self._opt(tape["lam_g"], f32, (B, L.ng), "lam_g"),
                          self._opt(tape["state"], f32, (B, 9), "state"), self._opt(tape["info"], f32, (B, _capi.INFO), "info"),
                          self._opt(tape.get("ok"), i32, (B,), "ok"), self._opt(tape["land"], i32, tn, "land"),
                          self._opt(tape.get("plan_t"), f64, tt, "plan_t"), self._opt(tape.get("plan_n"), i32, tn, "plan_n"),
                          self._opt(tape.get("prev_t"), f64, tt, "prev_t"), self._opt(tape.get("prev_n"), i32, tn, "prev_n"),
                          self._opt(lt, f64, tt, "list_t"), self._opt(tape["list_n"], i32, tn, "list_n"),
                          float(tape["step"]), int(tape["substeps"]), 1 if tape.get("force_sample_time") else 0)
        din = CmpcTickDirs(self._opt(dDirState, f64, (B, k, 9), "dDirState"), self._opt(dDirPrevList, f64, g3, "dDirPrevList"),
                           self._opt(dDirPrevListRot, f64, g3, "dDirPrevListRot"), self._opt(dDirPlan, f64, g3, "dDirPlan"),
                           self._opt(dDirPlanRot, f64, g3, "dDirPlanRot"), self._opt(dDirWrench, f32, (B, k, N, 6), "dDirWrench"),
                           self._opt(dDirModel, f64, (B, k, _capi.MODEL_DOUBLES), "dDirModel"), self._opt(dDirP, f32, (B, k, L.np), "dDirP"))
        out = dict(state=out_state if out_state is not None else torch.empty((B, k, 9), dtype=f64, device=dev), list=torch.empty(g3, dtype=f64, device=dev),
                   list_rot=torch.empty(g3, dtype=f64, device=dev), x=torch.empty((B, k, L.nx), dtype=f32, device=dev) if x else None,
                   rot=torch.empty((B, k, 2, N, 3), dtype=f64, device=dev) if rot else None,
                   p=torch.empty((B, k, L.np), dtype=f32, device=dev) if p_full else None, sens=torch.empty((B, _capi.SENS), dtype=f32, device=dev))
        dout = CmpcTickDirsOut(self._opt(out["state"], f64, (B, k, 9), "out_state"), out["list"].data_ptr(), out["list_rot"].data_ptr(),
                               out["x"].data_ptr() if x else None, out["rot"].data_ptr() if rot else None, out["p"].data_ptr() if p_full else None)
        if mm is not None:   # (the mismatch entry; all of it None: the library makes the plain call)
            hw, fg, dh, dn, dg = mm
            md = None
            if dh is not None or dn is not None or dg is not None:
                md = C.byref(_capi.CmpcTickDirsMismatch(self._opt(dh, f64, (B, k, 6), "dDirHidden"), self._opt(dn, f32, (B, k, 9), "dDirNoise"),
                                                        self._opt(dg, f64, (B, k), "dDirGain")))
            ph, pg = self._opt(hw, f32, (B, 6), "hidden_wrench"), self._opt(fg, f32, (B,), "force_gain")
            self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_jvp_mismatch_device(self._h, M, float(now), ct, k, din, dout, out["sens"].data_ptr(),
                                                                                         ph, pg, md, st))
            return out
        self._launch(dev, lambda st: self._lib.cmpc_rollout_tick_jvp_device(self._h, M, float(now), ct, k, din, dout, out["sens"].data_ptr(), st))
        return out

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
    def _launch(self, dev, fn):
        """runs fn(raw_stream) on torch's current stream (the default stream: on the solver's side stream, ordered after it and joined back; _stream_pair)"""
        st, cur = self._stream_pair(dev)
        rc = fn(st)
        if rc != 0:
            raise RuntimeError(f"libcmpc_hip call failed ({rc}): {self.last_error}")
        if cur is not None:
            cur.wait_stream(self._stream)

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
        if out is None:
            out = torch.empty_like(t)
        if ok is None:
            ok = torch.empty((self.batch,), dtype=torch.int32, device=t.device)
        assert t.is_contiguous() and out.is_contiguous() and t.dtype == torch.float64 and n.dtype == torch.int32 and t.shape[0] == self.batch
        self._launch(t.device, lambda st: self._lib.cmpc_contacts_force_sample_time_device(
            self._h, t.shape[2], float(self.cfg.sampling_time if dt is None else dt), t.data_ptr(), n.data_ptr(), out.data_ptr(), ok.data_ptr(), st))
        return out, ok

    def contacts_sample_device(self, now, lists, dP, land=None):
        """setContactPhaseList for the batch: samples `lists` at now + k dt into the contact blocks of dP[B,np]; returns
        land[B,2] (landing knots)."""
        import torch
        t, pose, n = lists
        if land is None:
            land = torch.empty((self.batch, 2), dtype=torch.int32, device=dP.device)
        up = np.ascontiguousarray([c.bounding_box_upper_limit for c in self.cfg.contacts], np.float32)
        lo = np.ascontiguousarray([c.bounding_box_lower_limit for c in self.cfg.contacts], np.float32)
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
            self._h, dState.data_ptr(), dWrench.data_ptr() if dWrench is not None else None, dP.data_ptr(), st))

    def write_reference_from_planner_device(self, dComIn, dHIn, in_dt, t_offset, robot_mass, com_height, dP):
        """setReferenceTrajectory from the planner's trajectories (8f-3) on the device: dComIn / dHIn [B, n_in, 3] float32 CUDA tensors -> comRef / hRef rows of dP."""
        assert dComIn.is_contiguous() and dHIn.is_contiguous() and dComIn.shape == dHIn.shape and dComIn.shape[0] == self.batch
        self._launch(dP.device, lambda st: self._lib.cmpc_write_reference_from_planner_device(
            self._h, dComIn.data_ptr(), dHIn.data_ptr(), int(dComIn.shape[1]), float(in_dt), float(t_offset), float(robot_mass),
            float("nan") if com_height is None else float(com_height), dP.data_ptr(), st))

    def _tick_io(self, plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                 force_sample_time):
        """the cmpc_tick_io of one tick (include/cmpc.h) from torch CUDA tensors; the box limits are the configuration's"""
        from ._capi import CmpcTickIO
        if getattr(self, "_box", None) is None:
            self._box = (np.ascontiguousarray([c.bounding_box_upper_limit for c in self.cfg.contacts], np.float32),
                         np.ascontiguousarray([c.bounding_box_lower_limit for c in self.cfg.contacts], np.float32))
        ptr = lambda a: a.data_ptr() if a is not None else None
        io = CmpcTickIO(ptr(plan[0]), ptr(plan[1]), ptr(plan[2]),
                        *(tuple(ptr(a) for a in prev) if prev is not None else (None, None, None)),
                        ptr(lists[0]), ptr(lists[1]), ptr(lists[2]), ptr(ok), ptr(land), self._box[0].ctypes.data, self._box[1].ctypes.data,
                        ptr(dState), ptr(dWrench), ptr(dP), ptr(dX0), ptr(dX), ptr(dInfo), ptr(dStateOut), ptr(dZmp),
                        float(step), int(substeps), float(zmp_half_x), float(zmp_half_y))
        if planner is not None:   # (dComIn, dHIn, in_dt, t_offset, robot_mass, com_height): the tick writes the reference rows itself
            pc, ph, pdt, poff, mass, height = planner
            io.dPlanCom, io.dPlanH, io.plan_knots, io.plan_dt, io.plan_t_offset = pc.data_ptr(), ph.data_ptr(), int(pc.shape[1]), float(pdt), float(poff)
            io.robot_mass, io.com_height = float(mass), float("nan") if height is None else float(height)
        io.force_sample_time = 1 if force_sample_time else 0
        return io

    def rollout_tick_device(self, now, plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, warm,
                            step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False):
        """cmpc_rollout_tick_device: merge -> sample -> setState -> shift -> solve -> step adjustment -> plant as ONE call (include/cmpc.h); plan / prev /
        lists = (t, pose, n) CUDA tensors, prev None on the first tick (lists is then taken as filled by the caller); dWrench may be None.
        force_sample_time: the planner's lists (the caller's lists on the first tick, in place) are snapped to the MPC grid first (forceSampleTime,
        CentroidalMPCBlock.cpp:586-592); ok is then written on the first tick too."""
        io = self._tick_io(plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                           force_sample_time)
        self._launch(dP.device, lambda st: self._lib.cmpc_rollout_tick_device(self._h, lists[0].shape[2], float(now), 1 if warm else 0, io, st))

    def rollout_tick_mismatch_device(self, tick, mismatch, now, plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, warm,
                                     step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False):
        """cmpc_rollout_tick_mismatch_device: rollout_tick_device with the tick number `tick` selecting the rows of mismatch (plant_mismatch(...), or None:
        rollout_tick_device bit for bit).  dState / dStateOut hold the TRUE state; the measured one goes into dP."""
        io = self._tick_io(plan, prev, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dStateOut, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                           force_sample_time)
        mc = C.byref(mismatch["_c"]) if mismatch is not None else None
        self._launch(dP.device, lambda st: self._lib.cmpc_rollout_tick_mismatch_device(self._h, lists[0].shape[2], float(now), 1 if warm else 0, io, int(tick),
                                                                                       mc, st))

    # ---- the walk on the device (include/cmpc.h, "a walk of the whole batch on the device") ----
    def walk_record(self, rows, stop=("merge", "solver", "nonfinite"), trace=True, device=None):
        """The arrays of a cmpc_walk_record as a dict of CUDA tensors (trace arrays only with trace=True) plus "_c", the C struct that points at them.
        stop: which tick codes end a problem, names of _capi.STOP_BITS ("merge" is always honoured).  The outcome is NOT set up: outcome_init_device."""
        import torch
        B = self.batch
        dev = torch.device("cuda", self._device_index) if device is None else device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        r = dict(end_tick=z((B,), torch.int32), end_code=z((B,), torch.int32), iterations_sum=z((B,), torch.int32), iterations_max=z((B,), torch.int32),
                 final_state=z((B, 9), torch.float32), box_slack_min=z((B,), torch.float32), stats=z((rows, 6), torch.int32))
        if trace:
            r.update(com=z((rows, B, 3), torch.float32), zmp=z((rows, B, 2), torch.float32), land=z((rows, B, 2), torch.int32),
                     landing_offset=z((rows, B, 2, 3), torch.float64), iterations=z((rows, B), torch.int32), code=z((rows, B), torch.int32))
        ptr = lambda k: r[k].data_ptr() if k in r else None
        mask = 0
        for name in stop:
            mask |= _capi.STOP_BITS[name]
        r["_c"] = _capi.CmpcWalkRecord(int(rows), mask, ptr("com"), ptr("zmp"), ptr("land"), ptr("landing_offset"), ptr("iterations"), ptr("code"),
                                       ptr("end_tick"), ptr("end_code"), ptr("iterations_sum"), ptr("iterations_max"), ptr("final_state"),
                                       ptr("box_slack_min"), ptr("stats"))
        return r

    def outcome_init_device(self, dState0, rec):
        """cmpc_rollout_outcome_init_device: the outcome arrays of rec (walk_record) at their start, final_state = dState0[B, 9]."""
        assert dState0.is_contiguous() and tuple(dState0.shape) == (self.batch, 9)
        self._launch(dState0.device, lambda st: self._lib.cmpc_rollout_outcome_init_device(self._h, dState0.data_ptr(), rec["_c"], st))

    def rollout_record_device(self, tick, row, dX, dP, dInfo, ok, land, dStateOut, dZmp, rec):
        """cmpc_rollout_record_device: the record of one tick into row `row` of rec (walk_record) from what the tick left; ok / dZmp may be None."""
        ptr = lambda a: a.data_ptr() if a is not None else None
        self._launch(dX.device, lambda st: self._lib.cmpc_rollout_record_device(
            self._h, int(tick), int(row), dX.data_ptr(), dP.data_ptr(), dInfo.data_ptr(), ptr(ok), land.data_ptr(), dStateOut.data_ptr(), ptr(dZmp),
            rec["_c"], st))

    def cold_start_device(self, dP, dX0=None):
        """cmpc_cold_start_device: the cold start (CoM at com0, feet at nominal, f_z = g / 8 per corner) of dP[B, np] into dX0[B, nx]."""
        import torch
        L = self.layout
        assert dP.is_contiguous() and dP.dtype == torch.float32 and tuple(dP.shape) == (self.batch, L.np)
        if dX0 is None:
            dX0 = torch.empty((self.batch, L.nx), dtype=torch.float32, device=dP.device)
        assert dX0.is_contiguous() and dX0.dtype == torch.float32 and tuple(dX0.shape) == (self.batch, L.nx)
        self._launch(dP.device, lambda st: self._lib.cmpc_cold_start_device(self._h, dP.data_ptr(), dX0.data_ptr(), st))
        return dX0

    def walk_tape(self, rows, max_contacts, step=0.01, substeps=6, force_sample_time=False, first_row_is_first_tick=True, device=None):
        """The arrays of a cmpc_walk_tape (include/cmpc.h) as a dict of CUDA tensors stacked over `rows` ticks -- X, P, lam_g, info, states[rows + 1], ok,
        land, plan_t, list_t, plan_n, list_n -- plus the host scalars (step, substeps, force_sample_time) and "_c", the C struct that points at them."""
        import torch
        B, L, M = self.batch, self.layout, int(max_contacts)
        dev = torch.device("cuda", self._device_index) if device is None else device
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        t = dict(X=z((rows, B, L.nx), f32), P=z((rows, B, L.np), f32), lam_g=z((rows, B, L.ng), f32), info=z((rows, B, _capi.INFO), f32),
                 states=z((rows + 1, B, 9), f32), ok=z((rows, B), i32), land=z((rows, B, 2), i32), plan_t=z((rows, B, 2, M, 2), f64),
                 list_t=z((rows, B, 2, M, 2), f64), plan_n=z((rows, B, 2), i32), list_n=z((rows, B, 2), i32))
        t["_c"] = _capi.CmpcWalkTape(int(rows), *(t[k].data_ptr() for k in ("X", "P", "lam_g", "info", "states", "ok", "land", "plan_t", "list_t", "plan_n",
                                                                            "list_n")), float(step), int(substeps), 1 if force_sample_time else 0,
                                     1 if first_row_is_first_tick else 0)
        t.update(rows=int(rows), max_contacts=M, step=float(step), substeps=int(substeps), force_sample_time=bool(force_sample_time))
        return t

    def rollout_tape_device(self, row, tape, dX, dP, dInfo, ok, land, dStateIn, dStateOut, plan, lists, parts=3):
        """cmpc_rollout_tape_device: row `row` of tape (walk_tape) from what a tick left.  parts 1: dStateIn -> states[row], BEFORE a tick that runs in place;
        2: everything else behind the tick (the multiplier output must be on); 3: both, behind a tick that did not run in place.  ok may be None (a first
        tick without force_sample_time), plan = (t, pose, n) or None on a first tick; lists = (t, pose, n) of the tick."""
        ptr = lambda a: a.data_ptr() if a is not None else None
        dev = (dStateIn if dStateIn is not None else dX).device
        self._launch(dev, lambda st: self._lib.cmpc_rollout_tape_device(
            self._h, int(tape["max_contacts"]), int(row), int(parts), ptr(dX), ptr(dP), ptr(dInfo), ptr(ok), ptr(land), ptr(dStateIn), ptr(dStateOut),
            ptr(plan[0]) if plan is not None else None, ptr(plan[2]) if plan is not None else None, ptr(lists[0]) if lists is not None else None,
            ptr(lists[2]) if lists is not None else None, tape["_c"], st))

    def rollout_walk_vjp_device(self, tick0, ticks, tape, row0, end_tick, grad_states, carry_state, carry_list, status, grad_X=None, wrench=None, grad_p=None,
                                dGradPlan=None, dGradModel=None, carry_list_rot=None, dGradPlanRot=None, grad_rot=None, removed=None, mismatch=None,
                                grad_hidden=None, grad_noise=None, grad_gain=None):
        """cmpc_rollout_walk_vjp_device: rows row0 .. row0 + ticks - 1 of tape (walk_tape) in reverse in ONE call.  grad_states[rows + 1, B, 9] float64 and
        grad_X[rows, B, n_x] float32 (or None) are the seeds; carry_state[B, 9] / carry_list[B, 2, M, 3] float64 go in as the carry entering the last row
        and come back as the carry leaving the first; wrench[rows, B, N, 6] / grad_p[rows, B, n_p] float32 (or None) and status[rows, B] int32 are written
        row by row; dGradPlan[B, 2, M, 3] / dGradModel[B, 34] float64 are added to in place.  end_tick: int32 [B] (a walk record's) or None.
        carry_list_rot[B, 2, M, 3] float64 given: cmpc_rollout_walk_vjp_rot_device, the contacts' orientations carried along -- it is the third carry;
        dGradPlanRot[B, 2, M, 3] float64 (or None) is added to in place, grad_rot[rows, B, 2, N, 3] float64 and removed[rows, B] float32 (or None) are
        written row by row.  Without it the three other arguments must be None and the call is the one it always was.
        mismatch (plant_mismatch(...)) given: cmpc_rollout_walk_vjp_mismatch_device, with or without carry_list_rot -- the walk ran under it; grad_hidden
        [rows, B, 6] float64 and grad_noise[rows, B, 9] float32 are written row by row, grad_gain[B] float64 is added to in place (each may be None)."""
        import torch
        L, B, N, M, R = self.layout, self.batch, self.cfg.N, int(tape["max_contacts"]), int(tape["rows"])
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        g = _capi.CmpcWalkGrads(self._opt(grad_states, f64, (R + 1, B, 9), "grad_states"), self._opt(grad_X, f32, (R, B, L.nx), "grad_X"),
                                self._opt(carry_state, f64, (B, 9), "carry_state"), self._opt(carry_list, f64, (B, 2, M, 3), "carry_list"),
                                self._opt(wrench, f32, (R, B, N, 6), "wrench"), self._opt(grad_p, f32, (R, B, L.np), "grad_p"),
                                self._opt(dGradPlan, f64, (B, 2, M, 3), "dGradPlan"), self._opt(dGradModel, f64, (B, _capi.MODEL_DOUBLES), "dGradModel"),
                                self._opt(status, i32, (R, B), "status"))
        e = self._opt(end_tick, i32, (B,), "end_tick")
        if mismatch is None:
            assert grad_hidden is None and grad_noise is None and grad_gain is None, "mismatch gradients need mismatch"
        if carry_list_rot is None:
            assert dGradPlanRot is None and grad_rot is None and removed is None, "orientation gradients need carry_list_rot"
            if mismatch is None:
                self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_device(self._h, M, int(tick0), int(ticks), tape["_c"], int(row0), e, g, st))
                return
        r = None
        if carry_list_rot is not None:
            r = _capi.CmpcWalkGradsRot(self._opt(carry_list_rot, f64, (B, 2, M, 3), "carry_list_rot"), self._opt(dGradPlanRot, f64, (B, 2, M, 3), "dGradPlanRot"),
                                       self._opt(grad_rot, f64, (R, B, 2, N, 3), "grad_rot"), self._opt(removed, f32, (R, B), "removed"))
        if mismatch is not None:
            mg = _capi.CmpcWalkGradsMismatch(self._opt(grad_hidden, f64, (R, B, 6), "grad_hidden"), self._opt(grad_noise, f32, (R, B, 9), "grad_noise"),
                                             self._opt(grad_gain, f64, (B,), "grad_gain"))
            self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_mismatch_device(
                self._h, M, int(tick0), int(ticks), tape["_c"], int(row0), e, g, C.byref(r) if r is not None else None, C.byref(mismatch["_c"]), C.byref(mg), st))
            return
        self._launch(carry_state.device,
                     lambda st: self._lib.cmpc_rollout_walk_vjp_rot_device(self._h, M, int(tick0), int(ticks), tape["_c"], int(row0), e, g, r, st))

    def rollout_walk_vjp_rows_device(self, tick0, ticks, tape, row0, end_tick, grad_states, carry_state, carry_list, status, grad_X=None, wrench=None,
                                     dGradPlan=None, dGradModel=None, carry_list_rot=None, dGradPlanRot=None, grad_rot=None, removed=None, grad_X_rows=None,
                                     mismatch=None, grad_hidden=None, grad_noise=None, grad_gain=None):
        """rollout_walk_vjp_device on a SEGMENT tape (a few rows, re-used) with WHOLE-WALK arrays: grad_states[T + 1, B, 9], grad_X / wrench / grad_rot
        [T, B, ..] and status / removed [T, B] are indexed by the tick number, the tape by row0 + i for tick tick0 + i.  Each array goes to the library
        as the leading-axis view that starts tick0 - row0 rows in, so that tape row and array row coincide; the call reads and writes rows tick0 ..
        tick0 + ticks - 1 of them (and no other), exactly as rollout_walk_vjp_device does on a whole-walk tape.  The carries and the += outputs as
        there.  grad_X_rows[rows, B, n_x] float32 (instead of grad_X): the solutions' seeds of this segment alone, indexed like the tape.
        mismatch (plant_mismatch(...)) given: cmpc_rollout_walk_vjp_mismatch_device -- the segment ran under it; grad_hidden[T, B, 6] float64 and
        grad_noise[T, B, 9] float32 are whole-walk arrays written at the segment's rows, grad_gain[B] float64 is added to in place (each may be None)."""
        import torch
        L, B, N, M = self.layout, self.batch, self.cfg.N, int(tape["max_contacts"])
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        tick0, ticks, row0 = int(tick0), int(ticks), int(row0)
        shift = tick0 - row0
        assert shift >= 0 and ticks >= 1 and 0 <= row0 and row0 + ticks <= int(tape["rows"]), "the segment must lie inside its tape"

        def view(t, dtype, tail, name, extra=0):
            if t is None:
                return None
            assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape[1:]) == tuple(tail) and t.shape[0] >= tick0 + ticks + extra, \
                f"{name}: expected {dtype} [>= {tick0 + ticks + extra}, {tuple(tail)}]"
            return t.data_ptr() + shift * t.stride(0) * t.element_size()
        assert grad_X is None or grad_X_rows is None, "grad_X or grad_X_rows, not both"
        gx = view(grad_X, f32, (B, L.nx), "grad_X") if grad_X_rows is None else self._opt(grad_X_rows, f32, (int(tape["rows"]), B, L.nx), "grad_X_rows")
        g = _capi.CmpcWalkGrads(view(grad_states, f64, (B, 9), "grad_states", 1), gx,
                                self._opt(carry_state, f64, (B, 9), "carry_state"), self._opt(carry_list, f64, (B, 2, M, 3), "carry_list"),
                                view(wrench, f32, (B, N, 6), "wrench"), None,
                                self._opt(dGradPlan, f64, (B, 2, M, 3), "dGradPlan"), self._opt(dGradModel, f64, (B, _capi.MODEL_DOUBLES), "dGradModel"),
                                view(status, i32, (B,), "status"))
        e = self._opt(end_tick, i32, (B,), "end_tick")
        if mismatch is None:
            assert grad_hidden is None and grad_noise is None and grad_gain is None, "mismatch gradients need mismatch"
        if carry_list_rot is None:
            assert dGradPlanRot is None and grad_rot is None and removed is None, "orientation gradients need carry_list_rot"
            if mismatch is None:
                self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_device(self._h, M, tick0, ticks, tape["_c"], row0, e, g, st))
                return
        r = None
        if carry_list_rot is not None:
            r = _capi.CmpcWalkGradsRot(self._opt(carry_list_rot, f64, (B, 2, M, 3), "carry_list_rot"), self._opt(dGradPlanRot, f64, (B, 2, M, 3), "dGradPlanRot"),
                                       view(grad_rot, f64, (B, 2, N, 3), "grad_rot"), view(removed, f32, (B,), "removed"))
        if mismatch is not None:
            mg = _capi.CmpcWalkGradsMismatch(view(grad_hidden, f64, (B, 6), "grad_hidden"), view(grad_noise, f32, (B, 9), "grad_noise"),
                                             self._opt(grad_gain, f64, (B,), "grad_gain"))
            self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_mismatch_device(
                self._h, M, tick0, ticks, tape["_c"], row0, e, g, C.byref(r) if r is not None else None, C.byref(mismatch["_c"]), C.byref(mg), st))
            return
        self._launch(carry_state.device, lambda st: self._lib.cmpc_rollout_walk_vjp_rot_device(self._h, M, tick0, ticks, tape["_c"], row0, e, g, r, st))

    # ---- the state of a walk between two ticks (include/cmpc.h, cmpc_walk_snapshot) ----
    def walk_snapshot(self, tick, lists_in, max_contacts, batch=None, device=None, tensors=None):
        """The arrays of a cmpc_walk_snapshot (include/cmpc.h) as a dict of CUDA tensors -- state[B, 9], P, X, X0, info, zmp, ok[B], land[B, 2], lists = the
        two list sets [(t, pose, n), (t, pose, n)], and the outcome end_tick, end_code, iterations_sum, iterations_max, final_state, box_slack_min --
        plus tick, lists_in, max_contacts, batch and "_c", the C struct that points at them.  Zero-filled; batch: the snapshot's own (default: the
        handle's).  tensors: a dict with some of these keys -- those tensors are taken as they are and not allocated (a walk's live buffers described as
        a snapshot); X0, info or zmp given as None there are left out of the struct (NULL: skipped by the copy)."""
        import torch
        B, L, M = int(self.batch if batch is None else batch), self.layout, int(max_contacts)
        dev = torch.device("cuda", self._device_index) if device is None else device
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        shapes = dict(state=((B, 9), f32), P=((B, L.np), f32), X=((B, L.nx), f32), X0=((B, L.nx), f32), info=((B, _capi.INFO), f32), zmp=((B, 2), f32),
                      ok=((B,), i32), land=((B, 2), i32), end_tick=((B,), i32), end_code=((B,), i32), iterations_sum=((B,), i32),
                      iterations_max=((B,), i32), final_state=((B, 9), f32), box_slack_min=((B,), f32))
        lshapes = (((B, 2, M, 2), f64), ((B, 2, M, 7), f32), ((B, 2), i32))
        given = dict(tensors or {})

        def chk(t, shape, dt, name):
            assert t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == tuple(shape), f"walk_snapshot: {name}: expected {dt} {tuple(shape)}"
            return t
        s = {}
        for k, (shape, dt) in shapes.items():
            if k in given:
                s[k] = None if given[k] is None else chk(given[k], shape, dt, k)
                assert s[k] is not None or k in ("X0", "info", "zmp"), f"walk_snapshot: {k} is required"
            else:
                s[k] = torch.zeros(shape, dtype=dt, device=dev)
        if "lists" in given:
            s["lists"] = [tuple(chk(a, sh, dt, "lists") for a, (sh, dt) in zip(st, lshapes)) for st in given["lists"]]
            assert len(s["lists"]) == 2
        else:
            s["lists"] = [tuple(torch.zeros(sh, dtype=dt, device=dev) for sh, dt in lshapes) for _ in range(2)]
        ptr = lambda t: None if t is None else t.data_ptr()
        s["_c"] = _capi.CmpcWalkSnapshot(int(tick), int(lists_in), *(ptr(s[k]) for k in ("state", "P", "X", "X0", "info", "zmp", "ok", "land")),
                                         *(ptr(a) for st in s["lists"] for a in st),
                                         *(ptr(s[k]) for k in ("end_tick", "end_code", "iterations_sum", "iterations_max", "final_state", "box_slack_min")))
        s.update(tick=int(tick), lists_in=int(lists_in), max_contacts=M, batch=B)
        return s

    def walk_snapshot_mark(self, snap, tick, lists_in):
        """the host words of a snapshot dict (walk_snapshot) and of its C struct"""
        snap["tick"] = snap["_c"].tick = int(tick)
        snap["lists_in"] = snap["_c"].lists_in = int(lists_in)

    def rollout_snapshot_device(self, src, dst, index=None, ok=None, src_batch=None):
        """cmpc_rollout_snapshot_device: ONE launch on torch's current stream, no host read: problem b of dst (walk_snapshot; the handle's batch) receives
        the bit copy of problem index[b] of src (index: int32 [B] CUDA tensor; None: problem b, and src must then hold the handle's batch).  An index
        outside [0, src_batch) leaves that problem of dst unwritten and gives ok[b] = 0 (ok: int32 [B], written when given).  src_batch: default
        src["batch"].  dst's host words tick and lists_in become src's.  Save and restore are the same call with the arguments swapped; repeated
        indices branch one problem into many."""
        import torch
        B = self.batch
        sb = int(src["batch"] if src_batch is None else src_batch)
        assert src["max_contacts"] == dst["max_contacts"] and dst["batch"] == B and sb <= src["batch"], "rollout_snapshot_device: snapshots of other sizes"
        i = self._opt(index, torch.int32, (B,), "index")
        o = self._opt(ok, torch.int32, (B,), "ok")
        self._launch(dst["state"].device, lambda st: self._lib.cmpc_rollout_snapshot_device(
            self._h, int(src["max_contacts"]), sb, C.byref(src["_c"]), C.byref(dst["_c"]), i, o, st))
        self.walk_snapshot_mark(dst, src["tick"], src["lists_in"])
        return dst

    def rollout_walk_vjp_gate_device(self, gate, device=None):
        """cmpc_rollout_walk_vjp_gate_device: one gate step of the reverse walk as one launch; gate: a _capi.CmpcWalkGate of device pointers."""
        import torch
        dev = torch.device("cuda", self._device_index) if device is None else device
        self._launch(dev, lambda st: self._lib.cmpc_rollout_walk_vjp_gate_device(self._h, C.byref(gate), st))

    def rollout_walk_vjp_rot_gate_device(self, gate, device=None):
        """cmpc_rollout_walk_vjp_rot_gate_device: one gate step of the reverse walk with the orientation arrays as one launch; gate: a
        _capi.CmpcWalkGateRot of device pointers."""
        import torch
        dev = torch.device("cuda", self._device_index) if device is None else device
        self._launch(dev, lambda st: self._lib.cmpc_rollout_walk_vjp_rot_gate_device(self._h, C.byref(gate), st))

    def rollout_walk_jvp_device(self, tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot=None, dir_plan=None,
                                dir_plan_rot=None, dir_wrench=None, dir_model=None, dir_p=None, dir_x=None, removed=None):
        """cmpc_rollout_walk_jvp_device: rows row0 .. row0 + ticks - 1 of tape (walk_tape) forwards in k directions in ONE call.  dir_states
        [rows + 1, B, k, 9] float64: row row0 is read, rows row0 + 1 .. row0 + ticks are written; carry_list / carry_list_rot[B, k, 2, M, 3] float64 go in as
        the list directions entering the first row and come back as those leaving the last (carry_list_rot and dir_plan_rot both None: no rotation chain);
        dir_plan / dir_plan_rot[B, k, 2, M, 3], dir_model[B, k, 34] float64, dir_wrench[rows, B, k, N, 6], dir_p[rows, B, k, n_p] float32 (None: zero);
        dir_x[rows, B, k, n_x] float32 (or None), status[rows, B] int32 and removed[rows, B] float32 (or None) are written row by row.  end_tick: int32
        [B] (a walk record's) or None."""
        self._rollout_walk_jvp(tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot, dir_plan, dir_plan_rot, dir_wrench,
                               dir_model, dir_p, dir_x, removed, None)

    def rollout_walk_jvp_mismatch_device(self, tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, mismatch=None, dir_hidden=None,
                                         dir_noise=None, dir_gain=None, carry_list_rot=None, dir_plan=None, dir_plan_rot=None, dir_wrench=None, dir_model=None,
                                         dir_p=None, dir_x=None, removed=None):
        """cmpc_rollout_walk_jvp_mismatch_device: rollout_walk_jvp_device on a walk that ran under `mismatch` (plant_mismatch(...); None: none was applied and
        only the directions are), with the directions of its three parts, rows as the tape's: dir_hidden[rows, B, k, 6] float64, dir_noise[rows, B, k, 9]
        float32, dir_gain[B, k] float64 (each may be None: zero).  All four None: the call above, bit for bit."""
        self._rollout_walk_jvp(tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot, dir_plan, dir_plan_rot, dir_wrench,
                               dir_model, dir_p, dir_x, removed, (mismatch, dir_hidden, dir_noise, dir_gain))

    def _rollout_walk_jvp(self, tick0, ticks, tape, row0, end_tick, k, dir_states, carry_list, status, carry_list_rot, dir_plan, dir_plan_rot, dir_wrench,
                          dir_model, dir_p, dir_x, removed, mm):
        import torch
        L, B, N, M, R, k = self.layout, self.batch, self.cfg.N, int(tape["max_contacts"]), int(tape["rows"]), int(k)
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        g3 = (B, k, 2, M, 3)
        d = _capi.CmpcWalkDirs(self._opt(dir_states, f64, (R + 1, B, k, 9), "dir_states"), self._opt(carry_list, f64, g3, "carry_list"),
                               self._opt(carry_list_rot, f64, g3, "carry_list_rot"), self._opt(dir_plan, f64, g3, "dir_plan"),
                               self._opt(dir_plan_rot, f64, g3, "dir_plan_rot"), self._opt(dir_wrench, f32, (R, B, k, N, 6), "dir_wrench"),
                               self._opt(dir_model, f64, (B, k, _capi.MODEL_DOUBLES), "dir_model"), self._opt(dir_p, f32, (R, B, k, L.np), "dir_p"),
                               self._opt(dir_x, f32, (R, B, k, L.nx), "dir_x"), self._opt(status, i32, (R, B), "status"),
                               self._opt(removed, f32, (R, B), "removed"))
        e = self._opt(end_tick, i32, (B,), "end_tick")
        if mm is None:
            self._launch(dir_states.device, lambda st: self._lib.cmpc_rollout_walk_jvp_device(self._h, M, int(tick0), int(ticks), tape["_c"], int(row0), e, k, d, st))
            return
        mismatch, dir_hidden, dir_noise, dir_gain = mm
        md = _capi.CmpcWalkDirsMismatch(self._opt(dir_hidden, f64, (R, B, k, 6), "dir_hidden"), self._opt(dir_noise, f32, (R, B, k, 9), "dir_noise"),
                                        self._opt(dir_gain, f64, (B, k), "dir_gain"))
        self._launch(dir_states.device, lambda st: self._lib.cmpc_rollout_walk_jvp_mismatch_device(
            self._h, M, int(tick0), int(ticks), tape["_c"], int(row0), e, k, d, C.byref(mismatch["_c"]) if mismatch is not None else None, C.byref(md), st))

    def rollout_walk_jvp_gate_device(self, gate, device=None):
        """cmpc_rollout_walk_jvp_gate_device: one gate step of the forward walk as one launch; gate: a _capi.CmpcWalkJvpGate of device pointers."""
        import torch
        dev = torch.device("cuda", self._device_index) if device is None else device
        self._launch(dev, lambda st: self._lib.cmpc_rollout_walk_jvp_gate_device(self._h, C.byref(gate), st))

    def walk_measures_vjp_device(self, tick0, ticks, tape, row0, end_tick, grad_measures, grad_states, grad_X, direct):
        """cmpc_walk_measures_vjp_device: the cotangents grad_measures[rows, B, 4] float64 of the stability measures of rows row0 .. row0 + ticks - 1 of
        tape (walk_tape) in ONE launch -> grad_states[rows + 1, B, 9] float64 and grad_X[rows, B, n_x] float32 ADDED TO (the reverse walk's seeds), and
        direct[rows, B, 32] float64 written (comRef_xy 2, omega [2][3], corner [2][4][3]).  The corners are the handle's or the installed models'.
        end_tick: int32 [B] (a walk record's) or None -- rows at or past a problem's end select zero and are not read."""
        import torch
        L, B, R = self.layout, self.batch, int(tape["rows"])
        f32, f64 = torch.float32, torch.float64
        g = _capi.CmpcWalkMeasureGrads(self._opt(grad_measures, f64, (R, B, _capi.WALK_MEASURES), "grad_measures"),
                                       self._opt(grad_states, f64, (R + 1, B, 9), "grad_states"), self._opt(grad_X, f32, (R, B, L.nx), "grad_X"),
                                       self._opt(direct, f64, (R, B, _capi.WALK_MEASURE_DIRECT), "direct"))
        e = self._opt(end_tick, torch.int32, (B,), "end_tick")
        self._launch(grad_measures.device,
                     lambda st: self._lib.cmpc_walk_measures_vjp_device(self._h, int(tick0), int(ticks), tape["_c"], int(row0), e, C.byref(g), st))

    def walk_measures_vjp_fold_device(self, direct, grad_p=None, grad_model=None):
        """cmpc_walk_measures_vjp_fold_device: behind the reverse walk, direct[rows, B, 32]'s comRef pair ADDED TO grad_p[rows, B, n_p] float32 (the
        reverse walk's grad_p) and its corner words summed over the rows into grad_model[B, 34] float64 (entries 10..33); either may be None."""
        import torch
        L, B, R = self.layout, self.batch, int(direct.shape[0])
        d = self._opt(direct, torch.float64, (R, B, _capi.WALK_MEASURE_DIRECT), "direct")
        gp = self._opt(grad_p, torch.float32, (R, B, L.np), "grad_p")
        gm = self._opt(grad_model, torch.float64, (B, _capi.MODEL_DOUBLES), "grad_model")
        self._launch(direct.device, lambda st: self._lib.cmpc_walk_measures_vjp_fold_device(self._h, R, d, gp, gm, st))

    def walk_measures_jvp_device(self, tick0, ticks, tape, row0, end_tick, k, dir_states, dir_x, dir_measures, dir_p=None, dir_model=None):
        """cmpc_walk_measures_jvp_device: the transpose of walk_measures_vjp_device in k columns, in rollout_walk_jvp_device's layouts: dir_states
        [rows + 1, B, k, 9] float64, dir_x[rows, B, k, n_x] float32, dir_p[rows, B, k, n_p] float32 or None (its knot-1 comRef xy only), dir_model
        [B, k, 34] float64 or None (its corners only) -> dir_measures[rows, B, k, 4] float64, written; rows at or past a problem's end are zero."""
        import torch
        L, B, R, k = self.layout, self.batch, int(tape["rows"]), int(k)
        f32, f64 = torch.float32, torch.float64
        d = _capi.CmpcWalkMeasureDirs(self._opt(dir_states, f64, (R + 1, B, k, 9), "dir_states"), self._opt(dir_x, f32, (R, B, k, L.nx), "dir_x"),
                                      self._opt(dir_p, f32, (R, B, k, L.np), "dir_p"), self._opt(dir_model, f64, (B, k, _capi.MODEL_DOUBLES), "dir_model"),
                                      self._opt(dir_measures, f64, (R, B, k, _capi.WALK_MEASURES), "dir_measures"))
        e = self._opt(end_tick, torch.int32, (B,), "end_tick")
        self._launch(dir_states.device,
                     lambda st: self._lib.cmpc_walk_measures_jvp_device(self._h, int(tick0), int(ticks), tape["_c"], int(row0), e, k, C.byref(d), st))

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

    def _walk_io(self, plan, lists, lists_b, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                 force_sample_time):
        """the cmpc_walk_io of a walk that runs in place on dState (include/cmpc.h): _tick_io's tick without previous lists, the second list set and the
        time of the planner trajectories' first knot"""
        io = _capi.CmpcWalkIO()
        io.tick = self._tick_io(plan, None, lists, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dState, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                                force_sample_time)
        io.dListTB, io.dListPoseB, io.dListNB = (a.data_ptr() for a in lists_b)
        io.plan_t_first = float(planner[3]) if planner is not None else 0.0
        return io

    def rollout_walk_device(self, tick0, ticks, cold_first, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, row0=0,
                            wrench_ticks=None, dWrench=None, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False,
                            tape=None, tape_row0=None, mismatch=None):
        """cmpc_rollout_walk_device: `ticks` ticks from tick number tick0 queued in one call, each followed by its record (rec: walk_record, or None), in
        place on dState.  lists / lists_b: the two sets of list buffers (t, pose, n), lists_in the one that holds the previous tick's lists (the first
        tick's own with cold_first); returns the set that holds the last tick's.  wrench_ticks[T, B, N, 6]: tick i < T of the call writes row i.
        planner = (dComIn, dHIn, in_dt, t_first, robot_mass, com_height), t_first the time of the trajectories' first knot.
        tape (walk_tape): cmpc_rollout_walk_taped_device -- tick i of the call also writes row tape_row0 + i (default: row0 + i) of the tape; the
        multiplier output must be on.
        mismatch (plant_mismatch(...)): cmpc_rollout_walk_mismatch_device, taped or not -- tick tick0 + i runs under row tick0 + i - tick_first of its schedules."""
        io = self._walk_io(plan, lists, lists_b, ok, land, dState, dWrench, dP, dX0, dX, dInfo, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner,
                           force_sample_time)
        if wrench_ticks is not None:
            assert wrench_ticks.is_contiguous() and tuple(wrench_ticks.shape[1:]) == (self.batch, self.cfg.N, 6)
            io.dWrenchTicks, io.wrench_ticks = wrench_ticks.data_ptr(), int(wrench_ticks.shape[0])
        out = C.c_int(-1)
        if mismatch is not None:
            self._launch(dP.device, lambda st: self._lib.cmpc_rollout_walk_mismatch_device(
                self._h, lists[0].shape[2], int(tick0), int(ticks), 1 if cold_first else 0, C.byref(io), rec["_c"] if rec is not None else None, int(row0),
                int(lists_in), C.byref(out), tape["_c"] if tape is not None else None, int(row0 if tape_row0 is None else tape_row0) if tape is not None else 0,
                C.byref(mismatch["_c"]), st))
            return out.value
        if tape is not None:
            self._launch(dP.device, lambda st: self._lib.cmpc_rollout_walk_taped_device(
                self._h, lists[0].shape[2], int(tick0), int(ticks), 1 if cold_first else 0, C.byref(io), rec["_c"] if rec is not None else None, int(row0),
                int(lists_in), C.byref(out), tape["_c"], int(row0 if tape_row0 is None else tape_row0), st))
            return out.value
        self._launch(dP.device, lambda st: self._lib.cmpc_rollout_walk_device(
            self._h, lists[0].shape[2], int(tick0), int(ticks), 1 if cold_first else 0, C.byref(io), rec["_c"] if rec is not None else None, int(row0),
            int(lists_in), C.byref(out), st))
        return out.value

    # ---- refill: a queue of trials behind the slots of a walk (include/cmpc.h, cmpc_walk_refill) ----
    def _need_refill(self):
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_device")

    def walk_refill(self, state0, trial_ticks, wrench_trials=None, trace_rows=0, trace_tick_first=0, device=None, init=True):
        """The arrays of a cmpc_walk_refill as a dict of CUDA tensors plus "_c", the C struct that points at them: state0 [Q, 9] float32 (the queue, kept),
        wrench_trials [R, Q, N, 6] float32 or None, the slots' start_tick / trial [B], next [1], the per-trial outcome end_tick, end_code, iterations_sum,
        iterations_max, final_state, box_slack_min, ticks, slot, start [Q, ..], and trial_of [trace_rows, B] (trace_rows > 0; row r is tick trace_tick_first
        + r).  init: cmpc_rollout_refill_init_device is queued (every slot empty, no trial started)."""
        import torch
        self._need_refill()
        B = self.batch
        dev = torch.device("cuda", self._device_index) if device is None else device
        assert state0.is_cuda and state0.dtype == torch.float32 and state0.is_contiguous() and state0.dim() == 2 and state0.shape[1] == 9, "state0 [Q, 9] float32"
        Q = int(state0.shape[0])
        z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)
        r = dict(state0=state0, wrench_trials=wrench_trials, start_tick=z((B,)), trial=z((B,)), next=z((1,)), end_tick=z((Q,)), end_code=z((Q,)),
                 iterations_sum=z((Q,)), iterations_max=z((Q,)), final_state=z((Q, 9), torch.float32), box_slack_min=z((Q,), torch.float32), ticks=z((Q,)),
                 slot=z((Q,)), start=z((Q,)), trials=Q, trial_ticks=int(trial_ticks))
        if trace_rows > 0:
            r["trial_of"] = z((int(trace_rows), B))
        c = _capi.CmpcWalkRefill()
        c.trials, c.trial_ticks = Q, int(trial_ticks)
        c.dStartTick, c.dTrial, c.dNext, c.dState0 = r["start_tick"].data_ptr(), r["trial"].data_ptr(), r["next"].data_ptr(), state0.data_ptr()
        if wrench_trials is not None:
            assert wrench_trials.is_cuda and wrench_trials.dtype == torch.float32 and wrench_trials.is_contiguous() and \
                tuple(wrench_trials.shape[1:]) == (Q, self.cfg.N, 6), "wrench_trials [R, Q, N, 6] float32"
            c.dWrenchTrials, c.wrench_ticks = wrench_trials.data_ptr(), int(wrench_trials.shape[0])
        for field, key in (("dTrialEndTick", "end_tick"), ("dTrialEndCode", "end_code"), ("dTrialIterationsSum", "iterations_sum"),
                           ("dTrialIterationsMax", "iterations_max"), ("dTrialFinalState", "final_state"), ("dTrialBoxSlackMin", "box_slack_min"),
                           ("dTrialTicks", "ticks"), ("dTrialSlot", "slot"), ("dTrialStart", "start")):
            setattr(c, field, r[key].data_ptr())
        if trace_rows > 0:
            c.trace = _capi.CmpcWalkRefillTrace(int(trace_rows), int(trace_tick_first), r["trial_of"].data_ptr())
        r["_c"] = c
        if init:
            self._launch(dev, lambda st: self._lib.cmpc_rollout_refill_init_device(self._h, C.byref(c), st))
        return r

    def rollout_refill_device(self, tick_next, rec, refill, dStateLive):
        """cmpc_rollout_refill_device: the refill in front of tick tick_next as ONE launch -- archive the occupied slots' outcome (rec: walk_record) into
        their trials' rows, then free slots take the queue's next trials in ascending slot order (refill: walk_refill).  dStateLive [B, 9] float32, the walk's
        state buffer; None: the archive pass only."""
        self._need_refill()
        if dStateLive is not None:
            assert dStateLive.is_contiguous() and tuple(dStateLive.shape) == (self.batch, 9)
        dev = refill["start_tick"].device
        self._launch(dev, lambda st: self._lib.cmpc_rollout_refill_device(self._h, int(tick_next), C.byref(rec["_c"]), C.byref(refill["_c"]),
                                                                          dStateLive.data_ptr() if dStateLive is not None else None, st))

    def walk_refill_trials(self, models=None, hidden_wrench=None, state_noise=None, force_gain=None, device=None):
        """A cmpc_walk_refill_trials as a dict: the per-TRIAL data of a refill walk over a queue of Q trials -- models [Q, 34] float64 (cmpc_model's order,
        config.model_array's rows), hidden_wrench [Th, Q, 6], state_noise [Tn, Q, 9], force_gain [Q] float32 (numpy or CUDA tensors, any subset; a schedule
        of zero rows counts as absent; the schedules' rows are the trial's LOCAL ticks).  With models the dict holds model_ok [Q] int32, -1 until the trial's
        first tick writes 1 or 0.  The dict keeps the device tensors alive and holds "_c", the C struct that points at them."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_trials_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_trials_device")
        dev = torch.device("cuda", self._device_index) if device is None else device
        hold = []

        def up(a, dtype, tail, name):
            if a is None:
                return None
            t = _upload(a, dev, dtype, hold).contiguous()    # (the host array is kept with the dict)
            assert t.dim() == len(tail) and all(w is None or int(t.shape[i]) == w for i, w in enumerate(tail)), f"{name}: expected {list(tail)}"
            return t if t.numel() > 0 else None
        r = dict(models=up(models, torch.float64, (None, _capi.MODEL_DOUBLES), "models"), hidden_wrench=up(hidden_wrench, torch.float32, (None, None, 6), "hidden_wrench"),
                 state_noise=up(state_noise, torch.float32, (None, None, 9), "state_noise"), force_gain=up(force_gain, torch.float32, (None,), "force_gain"))
        counts = {int(t.shape[0 if k in ("models", "force_gain") else 1]) for k, t in r.items() if t is not None}
        assert len(counts) <= 1, f"walk_refill_trials: the arrays disagree on the number of trials {sorted(counts)}"
        r["trials"] = counts.pop() if counts else None
        r["model_ok"] = torch.full((r["trials"],), -1, dtype=torch.int32, device=dev) if r["models"] is not None else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rows = lambda t: 0 if t is None else int(t.shape[0])
        r["_host"] = hold
        r["_c"] = _capi.CmpcWalkRefillTrials(ptr(r["models"]), ptr(r["model_ok"]), ptr(r["hidden_wrench"]), rows(r["hidden_wrench"]), ptr(r["state_noise"]),
                                             rows(r["state_noise"]), ptr(r["force_gain"]))
        return r

    def rollout_walk_refill_device(self, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0=0,
                                   step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False, tape=None, tape_row0=0,
                                   trials=None):
        """cmpc_rollout_walk_refill_device: `ticks` ticks of a refill walk from tick number tick0 in one call -- per tick the refill launch, the tick's three
        launches and the record -- in place on dState; the other arguments as rollout_walk_device's (no cold_first, wrench_ticks or mismatch: a slot's
        first tick runs inside the merge launches, and the wrench schedule is refill's per-trial one).  Returns the set that holds the last tick's lists.
        trials (walk_refill_trials(...)): cmpc_rollout_walk_refill_trials_device -- per-trial models and a per-trial plant mismatch; with models the handle
        is left on its per-problem table, which then holds each slot's last trial's model (set_models[_device] afterwards to go on with one's own).
        tape (walk_tape(...)): cmpc_rollout_walk_refill_taped_device -- tick i of the call also writes row tape_row0 + i of the tape, SLOT-major (seven
        launches a tick; the multiplier output must be on); tape_regroup_device gathers a trial's rows out of it.  (tape and tape_row0 stand in front of
        trials: that the parameter list ends with trials is pinned.)"""
        return self._rollout_walk_refill("taped" if tape is not None else "trials" if trials is not None else "", tick0, ticks, plan, lists, lists_b, lists_in, ok,
                                         land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0, step, substeps, zmp_half_x, zmp_half_y, planner,
                                         force_sample_time, tape=tape, tape_row0=tape_row0, trials=trials)

    def _rollout_walk_refill(self, entry, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0=0,
                             step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False, tape=None, tape_row0=0,
                             trials=None, snapshot=None, plans=None):
        """The one call behind rollout_walk_refill_device, _snapshot_device and _plans_device: the cmpc_walk_io, the queue-length checks, and the C entry
        point cmpc_rollout_walk_refill_<entry>_device -- entry "plans", "snapshot", "taped", "trials" or "" (the plain one).  Each takes, of the
        optional structs trials, snapshot, plans and tape, the ones its argument list has (include/cmpc.h), NULL where None."""
        name = f"cmpc_rollout_walk_refill_{entry}{'_' if entry else ''}device"
        if not hasattr(self._lib, name):
            raise RuntimeError(f"this build of libcmpc_hip has no {name}")
        io = self._walk_io(plan, lists, lists_b, ok, land, dState, None, dP, dX0, dX, dInfo, dZmp, step, substeps, zmp_half_x, zmp_half_y, planner, force_sample_time)
        for given, what in ((trials, "trials: the per-trial arrays"), (snapshot, "snapshot_of"), (plans, "plan_of")):
            assert given is None or given["trials"] in (None, refill["trials"]), f"{what} must have the queue's length"    # (None: trials without an array)
        if snapshot is not None:
            assert snapshot["pool"]["max_contacts"] == lists[0].shape[2], "the pool's lists must have the walk's length"
            assert snapshot["pool"]["_c"].tick == snapshot["tick"], "the pool was marked with another tick since walk_refill_snapshot"
        ref = lambda d: C.byref(d["_c"]) if d is not None else None
        out = C.c_int(-1)
        structs = {"": (), "trials": (ref(trials),), "taped": (ref(trials),), "snapshot": (ref(trials), ref(snapshot)), "plans": (ref(trials), ref(plans))}[entry]
        taped = (ref(tape), int(tape_row0)) if entry in ("taped", "plans") else ()
        self._launch(dP.device, lambda st: getattr(self._lib, name)(
            self._h, lists[0].shape[2], int(tick0), int(ticks), C.byref(io), ref(rec), ref(refill), *structs, int(row0), int(lists_in), C.byref(out), *taped, st))
        return out.value

    def walk_refill_snapshot(self, snapshot, snapshot_of, device=None):
        """A cmpc_walk_refill_snapshot as a dict: the pool -- snapshot, a walk_snapshot dict filled by rollout_snapshot_device (its tick >= 1 and lists_in
        as marked; any batch size) -- and snapshot_of [Q] int32 (numpy or CUDA), the pool row each trial of the queue starts from.  The dict holds
        snapshot_of on the device, snapshot_ok [Q] int32 (-1 until the trial's spawn writes 1 or 0), trials = Q, tick = the pool's, the pool itself (kept
        alive) and "_c", the C struct that points at them."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_snapshot_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_snapshot_device")
        dev = torch.device("cuda", self._device_index) if device is None else device
        hold = []
        idx = _upload(snapshot_of, dev, torch.int32, hold).contiguous()    # (the host array is kept with the dict)
        assert idx.dim() == 1, "snapshot_of: expected [Q]"
        Q = int(idx.shape[0])
        ok = torch.full((Q,), -1, dtype=torch.int32, device=dev)
        c = _capi.CmpcWalkRefillSnapshot(C.addressof(snapshot["_c"]), int(snapshot["batch"]), idx.data_ptr() if Q else None, ok.data_ptr() if Q else None)
        return dict(pool=snapshot, snapshot_of=idx, snapshot_ok=ok, trials=Q, tick=int(snapshot["tick"]), _host=hold, _c=c)

    def rollout_walk_refill_snapshot_device(self, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, snapshot,
                                            row0=0, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False,
                                            trials=None):
        """cmpc_rollout_walk_refill_snapshot_device: rollout_walk_refill_device with trials that start from a pool of saved problems (snapshot:
        walk_refill_snapshot(...); None: cmpc_rollout_walk_refill_trials_device through the new entry point).  Six launches per tick: the restore goes
        between the refill and the front kernel, and a slot spawned at tick s runs tick t at the pool's tick + (t - s).  (A method of its own: the parameter
        list of rollout_walk_refill_device is pinned.)"""
        return self._rollout_walk_refill("snapshot", tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0,
                                         step, substeps, zmp_half_x, zmp_half_y, planner, force_sample_time, trials=trials, snapshot=snapshot)

    def walk_refill_plans(self, pool, plan_of, plan, pool_refs=None, planner=None, device=None):
        """A cmpc_walk_refill_plans as a dict: pool = (t [Pn, 2, M, 2] float64, pose [Pn, 2, M, 7] float32, n [Pn, 2] int32), the pool of footstep plans
        in the layout of the planner's lists; plan_of [Q] int32 (numpy or CUDA), the pool row of each trial of the queue; plan = (t, pose, n) [B, ..], the
        slots' planner rows the walk is given -- WRITTEN by the walk: pass clones; pool_refs = (com, h) [Pn, n, 3] float32 or None, the planner
        trajectories of each plan, with planner = the (com, h, ...) tuple the walk is given (com / h [B, n, 3], written too).  The dict holds plan_of on the
        device, plan_ok [Q] int32 (-1 until the trial's spawn writes 1 or 0), trials = Q, pool_plans = Pn, the tensors (kept alive) and "_c"."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_walk_refill_plans_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_walk_refill_plans_device")
        dev = torch.device("cuda", self._device_index) if device is None else device
        hold = []
        up = lambda a, dtype: _upload(a, dev, dtype, hold).contiguous()    # (the host arrays are kept with the dict)
        pt, pp, pn = up(pool[0], torch.float64), up(pool[1], torch.float32), up(pool[2], torch.int32)
        Pn, M = int(pt.shape[0]), int(plan[0].shape[2])
        assert Pn >= 1 and tuple(pt.shape) == (Pn, 2, M, 2) and tuple(pp.shape) == (Pn, 2, M, 7) and tuple(pn.shape) == (Pn, 2), \
            f"pool: (t [Pn, 2, {M}, 2], pose [Pn, 2, {M}, 7], n [Pn, 2])"
        for a, dt, shape in zip(plan, (torch.float64, torch.float32, torch.int32), ((2, M, 2), (2, M, 7), (2,))):
            assert a.is_cuda and a.dtype == dt and a.is_contiguous() and tuple(a.shape) == (self.batch,) + shape, "plan: the slots' (t, pose, n) on the device"
        idx = up(plan_of, torch.int32)
        assert idx.dim() == 1, "plan_of: expected [Q]"
        Q = int(idx.shape[0])
        ok = torch.full((Q,), -1, dtype=torch.int32, device=dev)
        c = _capi.CmpcWalkRefillPlans()
        c.pool_plans = Pn
        c.dPoolT, c.dPoolPose, c.dPoolN = pt.data_ptr(), pp.data_ptr(), pn.data_ptr()
        c.dTrialPlan, c.dTrialPlanOk = (idx.data_ptr(), ok.data_ptr()) if Q else (None, None)
        c.dPlanT, c.dPlanPose, c.dPlanN = (a.data_ptr() for a in plan)
        refs = None
        if pool_refs is not None:
            assert planner is not None, "pool_refs need the walk's planner tuple (the slots' trajectories)"
            n = int(planner[0].shape[1])
            refs = (up(pool_refs[0], torch.float32), up(pool_refs[1], torch.float32))
            assert all(tuple(a.shape) == (Pn, n, 3) for a in refs), f"pool_refs: com and h [Pn, {n}, 3] (the knots of the slots' trajectories)"
            assert all(a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and tuple(a.shape) == (self.batch, n, 3) for a in planner[:2])
            c.dPoolCom, c.dPoolH = refs[0].data_ptr(), refs[1].data_ptr()
            c.dPlanCom, c.dPlanH = planner[0].data_ptr(), planner[1].data_ptr()
        return dict(pool=(pt, pp, pn), pool_refs=refs, plan_of=idx, plan_ok=ok, trials=Q, pool_plans=Pn, plan=plan, planner=planner, _host=hold, _c=c)

    def rollout_walk_refill_plans_device(self, tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, plans,
                                         row0=0, step=0.01, substeps=6, zmp_half_x=0.08, zmp_half_y=0.03, planner=None, force_sample_time=False,
                                         tape=None, tape_row0=0, trials=None):
        """cmpc_rollout_walk_refill_plans_device: rollout_walk_refill_device with a footstep plan (and planner trajectories) per TRIAL (plans:
        walk_refill_plans(...) over the same `plan` and `planner` tensors, which the walk WRITES; None: the taped / trials call through the new entry
        point).  One launch more per tick, the plan select, behind the refill: six, eight when taped.  (A method of its own: the parameter list of
        rollout_walk_refill_device is pinned.)"""
        return self._rollout_walk_refill("plans", tick0, ticks, plan, lists, lists_b, lists_in, ok, land, dState, dP, dX0, dX, dInfo, dZmp, rec, refill, row0,
                                         step, substeps, zmp_half_x, zmp_half_y, planner, force_sample_time, tape=tape, tape_row0=tape_row0, trials=trials,
                                         plans=plans)

    def plan_fold_device(self, index, per_trial, pool_rows, out=None):
        """cmpc_rollout_plan_fold_device: out[p] = the sum of per_trial[q] over the trials with index[q] == p, in ascending q, without atomics (the bits do
        not depend on scheduling).  index [Q] int32, per_trial [Q, ..] float64 CUDA tensors -> out [pool_rows, ..] float64, written whole (zero for a row
        no trial has); an index outside the pool contributes nowhere."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_plan_fold_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_plan_fold_device")
        Q = int(per_trial.shape[0])
        tail = tuple(per_trial.shape[1:])
        words = int(np.prod(tail)) if tail else 1
        assert per_trial.is_cuda and per_trial.dtype == torch.float64 and per_trial.is_contiguous(), "per_trial [Q, ..] float64"
        assert index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and tuple(index.shape) == (Q,), "index [Q] int32"
        if out is None:
            out = torch.empty((int(pool_rows),) + tail, dtype=torch.float64, device=per_trial.device)
        po = self._opt(out, torch.float64, (int(pool_rows),) + tail, "out")
        self._launch(per_trial.device, lambda st: self._lib.cmpc_rollout_plan_fold_device(
            self._h, Q, words, index.data_ptr() if Q else None, per_trial.data_ptr() if Q else None, int(pool_rows), po, st))
        return out

    def tape_regroup_device(self, src_tape, refill, trial_index, dst_tape=None, tick_first=0):
        """cmpc_rollout_tape_regroup_device: ONE launch on torch's current stream, no host read -- column j of dst_tape (walk_tape of refill["trial_ticks"]
        rows with first_row_is_first_tick; None: allocated here with src_tape's scalars) receives the rows of trial trial_index[j] out of the slot-major
        src_tape of a taped refill walk (rollout_walk_refill_device(tape=...), whose row 0 holds tick tick_first), by the rule at cmpc_walk_tape_regroup in
        include/cmpc.h.  trial_index: int32 [B] CUDA tensor; an entry outside the queue: no trial.  refill: the walk's walk_refill dict, its archive pass
        (rollout_refill_device(ticks, rec, refill, None)) queued behind the last tick.
        -> (dst_tape, end_tick [B] int32 -- what the reverse and the forward walks take as end_tick -- and ok [B] int32, 0 where the column has no trial)."""
        import torch
        if not hasattr(self._lib, "cmpc_rollout_tape_regroup_device"):
            raise RuntimeError("this build of libcmpc_hip has no cmpc_rollout_tape_regroup_device")
        B, M = self.batch, int(src_tape["max_contacts"])
        dev = src_tape["X"].device
        assert trial_index.is_cuda and trial_index.dtype == torch.int32 and trial_index.is_contiguous() and tuple(trial_index.shape) == (B,), \
            "trial_index [B] int32"
        if dst_tape is None:
            dst_tape = self.walk_tape(int(refill["trial_ticks"]), M, step=src_tape["step"], substeps=src_tape["substeps"],
                                      force_sample_time=src_tape["force_sample_time"], first_row_is_first_tick=True, device=dev)
        assert dst_tape["max_contacts"] == M and dst_tape["rows"] == int(refill["trial_ticks"]), "dst_tape: trial_ticks rows of the same list length"
        end = torch.zeros((B,), dtype=torch.int32, device=dev)
        ok = torch.zeros((B,), dtype=torch.int32, device=dev)
        g = _capi.CmpcWalkTapeRegroup(int(tick_first), trial_index.data_ptr(), end.data_ptr(), ok.data_ptr())
        self._launch(dev, lambda st: self._lib.cmpc_rollout_tape_regroup_device(self._h, M, C.byref(src_tape["_c"]), C.byref(refill["_c"]), C.byref(g),
                                                                                C.byref(dst_tape["_c"]), st))
        return dst_tape, end, ok

    def shift_solution_device(self, dXprev, dX0):
        """is_warm_start_enabled: dX0 = dXprev shifted by one knot; solve from it with solve_device(..., warm=True)."""
        self._launch(dX0.device, lambda st: self._lib.cmpc_shift_solution_device(self._h, dXprev.data_ptr(), dX0.data_ptr(), st))


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
