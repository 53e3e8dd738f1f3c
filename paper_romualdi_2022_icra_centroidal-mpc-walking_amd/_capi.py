"""ctypes binding of libcmpc_hip.so (include/cmpc.h).  There is no CPU path: if the HIP library is
missing or fails to load, every entry point raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("CMPC_LIB", "libcmpc_hip.so"))   # (CMPC_LIB: developer knob, another build of the same library in the package directory)

INFO = 8
CERT = 8   # CMPC_CERT: fields of the KKT certificate (include/cmpc.h)
SENS = 8   # CMPC_SENS: per-problem info words of the solution sensitivities (include/cmpc.h)


class CmpcConfig(C.Structure):
    _fields_ = [
        ("horizon", C.c_int),
        ("sampling_time", C.c_double),
        ("friction_coefficient", C.c_double),
        ("gravity", C.c_double),
        ("com_weight", C.c_double * 3),
        ("angular_momentum_weight", C.c_double),
        ("contact_position_weight", C.c_double),
        ("force_rate_of_change_weight", C.c_double * 3),
        ("contact_force_symmetry_weight", C.c_double),
        ("corners", C.c_double * 24),
        ("max_iterations", C.c_int),
        ("tolerance", C.c_double),
        ("step_tolerance", C.c_double),
        ("mu_init", C.c_double),
        ("mu_min", C.c_double),
        ("exact_hessian", C.c_int),
        ("final_extrapolation", C.c_int),
        ("tail_stages", C.c_int),
        ("tail_iterations", C.c_int),
        ("tail_trigger", C.c_double),
        ("factor_storage", C.c_int),
    ]


class CmpcTickIO(C.Structure):
    """mirror of cmpc_tick_io (include/cmpc.h): the buffers of one receding-horizon tick, cmpc_rollout_tick_device"""
    _fields_ = [(k, C.c_void_p) for k in (
        "dPlanT", "dPlanPose", "dPlanN", "dPrevT", "dPrevPose", "dPrevN", "dListT", "dListPose", "dListN", "dOk", "dLand",
        "box_upper", "box_lower", "dState", "dWrench", "dP", "dX0", "dX", "dInfo", "dStateOut", "dZmp")] + [
        ("plant_step", C.c_double), ("plant_substeps", C.c_int), ("zmp_half_x", C.c_double), ("zmp_half_y", C.c_double),
        ("dPlanCom", C.c_void_p), ("dPlanH", C.c_void_p), ("plan_knots", C.c_int), ("plan_dt", C.c_double), ("plan_t_offset", C.c_double),
        ("robot_mass", C.c_double), ("com_height", C.c_double), ("force_sample_time", C.c_int)]


class CmpcWalkRecord(C.Structure):
    """mirror of cmpc_walk_record (include/cmpc.h): the trace, outcome and statistics arrays of cmpc_rollout_record[_device] / cmpc_rollout_walk_device"""
    _fields_ = [("rows", C.c_int), ("stop_mask", C.c_int)] + [(k, C.c_void_p) for k in (
        "dCom", "dZmp", "dLand", "dLandingOffset", "dIterations", "dCode", "dEndTick", "dEndCode", "dIterationsSum", "dIterationsMax", "dFinalState",
        "dBoxSlackMin", "dStats")]


class CmpcWalkIO(C.Structure):
    """mirror of cmpc_walk_io (include/cmpc.h): the buffers of cmpc_rollout_walk_device"""
    _fields_ = [("tick", CmpcTickIO), ("dListTB", C.c_void_p), ("dListPoseB", C.c_void_p), ("dListNB", C.c_void_p), ("plan_t_first", C.c_double),
                ("dWrenchTicks", C.c_void_p), ("wrench_ticks", C.c_int)]


class CmpcWalkRefillTrace(C.Structure):
    """mirror of cmpc_walk_refill_trace (include/cmpc.h): which trial occupied each slot, tick by tick"""
    _fields_ = [("rows", C.c_int), ("tick_first", C.c_int), ("dTrialOf", C.c_void_p)]


class CmpcWalkRefill(C.Structure):
    """mirror of cmpc_walk_refill (include/cmpc.h): the queue of trials behind a walk's slots, cmpc_rollout_refill[_device] / cmpc_rollout_walk_refill_device"""
    _fields_ = [("trials", C.c_int), ("trial_ticks", C.c_int), ("dStartTick", C.c_void_p), ("dTrial", C.c_void_p), ("dNext", C.c_void_p),
                ("dState0", C.c_void_p), ("dWrenchTrials", C.c_void_p), ("wrench_ticks", C.c_int)] + [(k, C.c_void_p) for k in (
        "dTrialEndTick", "dTrialEndCode", "dTrialIterationsSum", "dTrialIterationsMax", "dTrialFinalState", "dTrialBoxSlackMin", "dTrialTicks",
        "dTrialSlot", "dTrialStart")] + [("trace", CmpcWalkRefillTrace)]


class CmpcWalkRefillTrials(C.Structure):
    """mirror of cmpc_walk_refill_trials (include/cmpc.h): the per-trial models and plant mismatch of cmpc_rollout_walk_refill_trials_device; 56 bytes"""
    _fields_ = [("dModels", C.c_void_p), ("dModelOk", C.c_void_p), ("dHiddenWrench", C.c_void_p), ("hidden_ticks", C.c_int), ("dStateNoise", C.c_void_p),
                ("noise_ticks", C.c_int), ("dForceGain", C.c_void_p)]


class CmpcWalkRefillSnapshot(C.Structure):
    """mirror of cmpc_walk_refill_snapshot (include/cmpc.h): the pool of saved problems the trials of cmpc_rollout_walk_refill_snapshot_device start from;
    32 bytes.  (CmpcWalkSnapshot is defined below: the pool is held as a plain address.)"""
    _fields_ = [("pool", C.c_void_p), ("pool_batch", C.c_int), ("dTrialSnapshot", C.c_void_p), ("dTrialSnapshotOk", C.c_void_p)]


class CmpcWalkRefillPlans(C.Structure):
    """mirror of cmpc_walk_refill_plans (include/cmpc.h): the pool of footstep plans (and planner trajectories) the trials of
    cmpc_rollout_walk_refill_plans_device name a row of, and the writable views of the slots' rows; 104 bytes"""
    _fields_ = [("pool_plans", C.c_int)] + [(k, C.c_void_p) for k in (
        "dPoolT", "dPoolPose", "dPoolN", "dPoolCom", "dPoolH", "dTrialPlan", "dTrialPlanOk", "dPlanT", "dPlanPose", "dPlanN", "dPlanCom", "dPlanH")]


class CmpcWalkTapeRegroup(C.Structure):
    """mirror of cmpc_walk_tape_regroup (include/cmpc.h): which trial each column of a regrouped tape takes, and the end ticks and flags that come back;
    32 bytes"""
    _fields_ = [("tick_first", C.c_int), ("dTrialIndex", C.c_void_p), ("dEndOut", C.c_void_p), ("dOkOut", C.c_void_p)]


STOP_BITS = {"merge": 1, "solver": 2, "nonfinite": 4, "limits": 8}   # cmpc_walk_record.stop_mask

WALK_MEASURES = 4   # CMPC_WALK_MEASURES: height, reach, margin, track
WALK_EXTREMES = 5   # CMPC_WALK_EXTREMES: height min, height max, reach max, margin min, track max


class CmpcWalkLimits(C.Structure):
    """mirror of cmpc_walk_limits (include/cmpc.h): the physical limits of a walk's record (NaN: off), its measures trace and its extremes; 64 bytes"""
    _fields_ = [("height_min", C.c_double), ("height_max", C.c_double), ("reach_max", C.c_double), ("margin_min", C.c_double), ("track_max", C.c_double),
                ("dMeasures", C.c_void_p), ("rows", C.c_int), ("dExtremes", C.c_void_p)]


WALK_MEASURE_INPUTS = 44   # CMPC_WALK_MEASURE_INPUTS: com 3, dcom 3, q [2][3], omega [2][3], corner [2][4][3], comRef_xy 2
WALK_MEASURE_DIRECT = 32   # CMPC_WALK_MEASURE_DIRECT: comRef_xy 2, omega [2][3], corner [2][4][3]


class CmpcWalkMeasureGrads(C.Structure):
    """mirror of cmpc_walk_measure_grads (include/cmpc.h): the cotangents and outputs of cmpc_walk_measures_vjp_device"""
    _fields_ = [(k, C.c_void_p) for k in ("dGradMeasures", "dGradStates", "dGradX", "dDirect")]


class CmpcWalkMeasureDirs(C.Structure):
    """mirror of cmpc_walk_measure_dirs (include/cmpc.h): the direction columns and the output of cmpc_walk_measures_jvp_device"""
    _fields_ = [(k, C.c_void_p) for k in ("dDirStates", "dDirX", "dDirP", "dDirModel", "dDirMeasures")]


class CmpcTickTape(C.Structure):
    """mirror of cmpc_tick_tape (include/cmpc.h): what a forward tick left behind, read by cmpc_rollout_tick_vjp_device"""
    _fields_ = [(k, C.c_void_p) for k in (
        "dX", "dP", "dLamG", "dState", "dInfo", "dOk", "dLand", "dPlanT", "dPlanN", "dPrevT", "dPrevN", "dListT", "dListN")] + [
        ("plant_step", C.c_double), ("plant_substeps", C.c_int), ("force_sample_time", C.c_int)]


class CmpcWalkTape(C.Structure):
    """mirror of cmpc_walk_tape (include/cmpc.h): the device tape of a walk, `rows` rows laid out like the fields of cmpc_tick_tape"""
    _fields_ = [("rows", C.c_int)] + [(k, C.c_void_p) for k in (
        "dX", "dP", "dLamG", "dInfo", "dStates", "dOk", "dLand", "dPlanT", "dListT", "dPlanN", "dListN")] + [
        ("plant_step", C.c_double), ("plant_substeps", C.c_int), ("force_sample_time", C.c_int), ("first_row_is_first_tick", C.c_int)]


class CmpcWalkSnapshot(C.Structure):
    """mirror of cmpc_walk_snapshot (include/cmpc.h): the state of a walk between two ticks -- also the description of a walk's live buffers"""
    _fields_ = [("tick", C.c_int), ("lists_in", C.c_int)] + [(k, C.c_void_p) for k in (
        "dState", "dP", "dX", "dX0", "dInfo", "dZmp", "dOk", "dLand", "dListT", "dListPose", "dListN", "dListTB", "dListPoseB", "dListNB",
        "dEndTick", "dEndCode", "dIterationsSum", "dIterationsMax", "dFinalState", "dBoxSlackMin")]


class CmpcWalkGrads(C.Structure):
    """mirror of cmpc_walk_grads (include/cmpc.h): the seeds, carries and outputs of cmpc_rollout_walk_vjp_device"""
    _fields_ = [(k, C.c_void_p) for k in (
        "dGradStates", "dGradX", "dCarryState", "dCarryList", "dGradWrench", "dGradP", "dGradPlan", "dGradModel", "dStatus")]


class CmpcWalkGate(C.Structure):
    """mirror of cmpc_walk_gate (include/cmpc.h): one gate step of the reverse walk on the host, cmpc_rollout_walk_vjp_gate"""
    _fields_ = [("batch", C.c_int), ("max_contacts", C.c_int), ("horizon", C.c_int), ("end_tick", C.c_void_p), ("do_post", C.c_int), ("tick_post", C.c_int)] + [
        (k, C.c_void_p) for k in ("seed_state", "tick_state", "tick_list", "tick_sens", "carry_state", "carry_list", "wrench_row", "grad_p_row", "status_row")] + [
        ("do_pre", C.c_int), ("tick_pre", C.c_int), ("first", C.c_int)] + [(k, C.c_void_p) for k in ("ok_row", "grad_x_row", "ok_out", "grad_x_out")]


class CmpcWalkGradsRot(C.Structure):
    """mirror of cmpc_walk_grads_rot (include/cmpc.h): the orientation carry and outputs of cmpc_rollout_walk_vjp_rot_device"""
    _fields_ = [(k, C.c_void_p) for k in ("dCarryListRot", "dGradPlanRot", "dGradRot", "dRemoved")]


class CmpcWalkGateRot(C.Structure):
    """mirror of cmpc_walk_gate_rot (include/cmpc.h): one gate step of the reverse walk with the orientation arrays, cmpc_rollout_walk_vjp_rot_gate[_device]"""
    _fields_ = [("base", CmpcWalkGate)] + [(k, C.c_void_p) for k in ("tick_list_rot", "carry_list_rot", "rot_row", "removed_row")]


class CmpcPlantMismatch(C.Structure):
    """mirror of cmpc_plant_mismatch (include/cmpc.h): the schedules of hidden wrenches and state noise and the force gain of a mismatched plant"""
    _fields_ = [("tick_first", C.c_int), ("dHiddenWrench", C.c_void_p), ("hidden_ticks", C.c_int), ("dStateNoise", C.c_void_p), ("noise_ticks", C.c_int),
                ("dForceGain", C.c_void_p)]


class CmpcWrenchSensor(C.Structure):
    """mirror of cmpc_wrench_sensor (include/cmpc.h): the sensor between the hidden-wrench schedule and the MPC of a sensed walk; 32 bytes"""
    _fields_ = [("delay_ticks", C.c_int), ("hold_knots", C.c_int), ("deadband", C.c_double), ("dSensorNoise", C.c_void_p), ("noise_ticks", C.c_int)]


class CmpcWalkGradsMismatch(C.Structure):
    """mirror of cmpc_walk_grads_mismatch (include/cmpc.h): the mismatch outputs of cmpc_rollout_walk_vjp_mismatch_device"""
    _fields_ = [(k, C.c_void_p) for k in ("dGradHidden", "dGradNoise", "dGradGain")]


class CmpcTickDirsMismatch(C.Structure):
    """mirror of cmpc_tick_dirs_mismatch (include/cmpc.h): the mismatch directions of cmpc_rollout_tick_jvp_mismatch_device, each pointer NULL = zero; 24 bytes"""
    _fields_ = [(k, C.c_void_p) for k in ("dDirHidden", "dDirNoise", "dDirGain")]


class CmpcWalkDirsMismatch(C.Structure):
    """mirror of cmpc_walk_dirs_mismatch (include/cmpc.h): the mismatch directions of cmpc_rollout_walk_jvp_mismatch_device, rows as the tape's; 24 bytes"""
    _fields_ = [(k, C.c_void_p) for k in ("dDirHidden", "dDirNoise", "dDirGain")]


class CmpcWalkDirs(C.Structure):
    """mirror of cmpc_walk_dirs (include/cmpc.h): the direction columns, carries and outputs of cmpc_rollout_walk_jvp_device"""
    _fields_ = [(k, C.c_void_p) for k in (
        "dDirStates", "dCarryList", "dCarryListRot", "dDirPlan", "dDirPlanRot", "dDirWrench", "dDirModel", "dDirP", "dDirX", "dStatus", "dRemoved")]


class CmpcWalkJvpGate(C.Structure):
    """mirror of cmpc_walk_jvp_gate (include/cmpc.h): one gate step of the forward walk, cmpc_rollout_walk_jvp_gate[_device]"""
    _fields_ = [("batch", C.c_int), ("max_contacts", C.c_int), ("horizon", C.c_int), ("k", C.c_int), ("end_tick", C.c_void_p), ("do_post", C.c_int),
                ("tick_post", C.c_int)] + [(k, C.c_void_p) for k in (
                    "tick_sens", "state_out", "list_out", "list_rot_out", "x_row", "status_row", "removed_row")] + [
        ("do_pre", C.c_int), ("tick_pre", C.c_int), ("first", C.c_int)] + [(k, C.c_void_p) for k in (
            "ok_row", "ok_out", "first_state", "first_list", "first_list_rot")]


class CmpcTickDirs(C.Structure):
    """mirror of cmpc_tick_dirs (include/cmpc.h): the k direction columns that go into cmpc_rollout_tick_jvp_device, each pointer NULL = zero"""
    _fields_ = [(k, C.c_void_p) for k in (
        "dDirState", "dDirPrevList", "dDirPrevListRot", "dDirPlan", "dDirPlanRot", "dDirWrench", "dDirModel", "dDirP")]


class CmpcTickDirsOut(C.Structure):
    """mirror of cmpc_tick_dirs_out (include/cmpc.h): what cmpc_rollout_tick_jvp_device writes (the first two required)"""
    _fields_ = [(k, C.c_void_p) for k in ("dDirStateOut", "dDirList", "dDirListRot", "dDirX", "dDirRot", "dDirPFull")]


class CmpcPlannerRefs(C.Structure):
    """mirror of cmpc_planner_refs (include/cmpc.h): the timing, mass and height of the planner's CoM / angular-momentum trajectories"""
    _fields_ = [("knots", C.c_int), ("dt", C.c_double), ("t_first", C.c_double), ("robot_mass", C.c_double), ("com_height", C.c_double)]


class CmpcModel(C.Structure):
    """mirror of cmpc_model (include/cmpc.h): the per-problem part of cmpc_config, 34 packed doubles"""
    _fields_ = [
        ("friction_coefficient", C.c_double),
        ("com_weight", C.c_double * 3),
        ("angular_momentum_weight", C.c_double),
        ("contact_position_weight", C.c_double),
        ("force_rate_of_change_weight", C.c_double * 3),
        ("contact_force_symmetry_weight", C.c_double),
        ("corners", C.c_double * 24),
    ]


MODEL_DOUBLES = 34   # CMPC_MODEL_DOUBLES


FACTORS = {None: 0, "auto": 0, "lds": 1, "hbm": 2}   # cmpc_config.factor_storage


EXPORTS = [
    "cmpc_default_config", "cmpc_dims", "cmpc_create", "cmpc_destroy", "cmpc_last_error",
    "cmpc_batch", "cmpc_stream", "cmpc_solve_device", "cmpc_solve", "cmpc_last_solve_ms", "cmpc_set_timing",
    "cmpc_eval_nlp_device", "cmpc_nlp_sparsity", "cmpc_set_state", "cmpc_set_reference",
    "cmpc_set_contacts", "cmpc_set_initial_guess", "cmpc_advance", "cmpc_get_solution",
    "cmpc_get_output", "cmpc_set_reference_from_planner", "cmpc_plant_step_device", "cmpc_test_poison_lds",
    "cmpc_compact_output_device", "cmpc_contacts_merge", "cmpc_contacts_merge_device", "cmpc_contacts_sample",
    "cmpc_contacts_sample_device", "cmpc_set_contact_lists", "cmpc_contacts_adjust", "cmpc_contacts_adjust_device",
    "cmpc_write_state_device", "cmpc_shift_solution_device", "cmpc_eval_nlp_grad_device", "cmpc_solve_device_warm", "cmpc_set_warm_policy",
    "cmpc_get_parameters", "cmpc_get_parameters_device", "cmpc_allgather_compact_device",
    "cmpc_rollout_tick_device", "cmpc_write_reference_from_planner_device", "cmpc_default_tolerance",
    "cmpc_contacts_force_sample_time", "cmpc_contacts_force_sample_time_device",
    "cmpc_model_from_config", "cmpc_check_models", "cmpc_set_models", "cmpc_set_models_device",
    "cmpc_set_multiplier_output", "cmpc_get_multipliers_device", "cmpc_get_multipliers", "cmpc_kkt_certificate_device",
    "cmpc_value_gradient_device", "cmpc_solution_jvp_device", "cmpc_solution_vjp_device",
    "cmpc_sensitivity_workspace_bytes", "cmpc_solution_jvp_model_device", "cmpc_solution_vjp_model_device", "cmpc_model_value_gradient_device",
    "cmpc_plant_step_jvp_device", "cmpc_plant_step_vjp_device", "cmpc_contacts_position_vjp_device", "cmpc_rollout_tick_vjp_device",
    "cmpc_solution_jvp_rot_device", "cmpc_solution_vjp_rot_device", "cmpc_rotation_value_gradient_device", "cmpc_contacts_rotation_vjp_device",
    "cmpc_plant_step_jvp_rot_device", "cmpc_plant_step_vjp_rot_device", "cmpc_contacts_orientation_vjp_device", "cmpc_rollout_tick_vjp_rot_device",
    "cmpc_plant_step_jvp_cols_device", "cmpc_contacts_jvp_device", "cmpc_rollout_tick_jvp_device",
    "cmpc_rollout_record", "cmpc_rollout_record_device", "cmpc_rollout_outcome_init_device", "cmpc_cold_start_device", "cmpc_rollout_walk_device",
    "cmpc_set_ended_device",
    "cmpc_rollout_tape_device", "cmpc_rollout_walk_taped_device", "cmpc_rollout_walk_vjp_device", "cmpc_rollout_walk_vjp_gate",
    "cmpc_rollout_walk_vjp_gate_device",
    "cmpc_rollout_walk_jvp_device", "cmpc_rollout_walk_jvp_gate", "cmpc_rollout_walk_jvp_gate_device",
    "cmpc_rollout_walk_vjp_rot_device", "cmpc_rollout_walk_vjp_rot_gate", "cmpc_rollout_walk_vjp_rot_gate_device",
    "cmpc_reference_from_planner_vjp", "cmpc_reference_from_planner_vjp_device", "cmpc_reference_from_planner_jvp", "cmpc_reference_from_planner_jvp_device",
    "cmpc_rollout_snapshot", "cmpc_rollout_snapshot_device", "cmpc_walk_snapshot_bytes",
    "cmpc_plant_step_mismatch_device", "cmpc_rollout_tick_mismatch_device", "cmpc_rollout_walk_mismatch_device",
    "cmpc_plant_step_vjp_mismatch_device", "cmpc_rollout_tick_vjp_mismatch_device", "cmpc_rollout_walk_vjp_mismatch_device",
    "cmpc_plant_step_jvp_mismatch_cols_device", "cmpc_rollout_tick_jvp_mismatch_device", "cmpc_rollout_walk_jvp_mismatch_device",
    "cmpc_rollout_refill_init", "cmpc_rollout_refill_init_device", "cmpc_rollout_refill", "cmpc_rollout_refill_device", "cmpc_rollout_walk_refill_device",
    "cmpc_rollout_walk_refill_trials_device", "cmpc_rollout_walk_refill_snapshot_device", "cmpc_rollout_refill_restore",
    "cmpc_rollout_walk_refill_taped_device", "cmpc_rollout_tape_regroup_device", "cmpc_rollout_tape_regroup",
    "cmpc_rollout_walk_refill_plans_device", "cmpc_rollout_refill_plans", "cmpc_rollout_plan_fold_device", "cmpc_rollout_plan_fold",
    "cmpc_factor_storage", "cmpc_solution_vjp_cols_device",
    "cmpc_set_walk_limits", "cmpc_walk_extremes_init_device", "cmpc_rollout_record_limits",
    "cmpc_walk_measures_vjp_device", "cmpc_walk_measures_vjp_fold_device", "cmpc_walk_measures_jvp_device",
    "cmpc_walk_measures_vjp", "cmpc_walk_measures_vjp_fold", "cmpc_walk_measures_jvp", "cmpc_walk_measures_jacobian",
    "cmpc_wrench_sense", "cmpc_wrench_sense_device", "cmpc_rollout_walk_sensed_device", "cmpc_wrench_sense_vjp", "cmpc_wrench_sense_vjp_device",
    "cmpc_wrench_sense_jvp", "cmpc_wrench_sense_jvp_device",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). This package has no CPU fallback.")
        try:
            # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; import it first so that this
            # library binds to the same HIP runtime (two runtimes in one process cannot share the GPU)
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.c_void_p
        L.cmpc_default_config.argtypes = [C.POINTER(CmpcConfig)]
        L.cmpc_default_config.restype = None
        L.cmpc_dims.argtypes = [C.c_int, ip, ip, ip, ip, ip]
        L.cmpc_default_tolerance.argtypes = [C.c_int]
        L.cmpc_default_tolerance.restype = C.c_double
        L.cmpc_create.argtypes = [C.POINTER(CmpcConfig), C.c_int, C.c_int, C.POINTER(vp)]
        L.cmpc_destroy.argtypes = [vp]
        L.cmpc_last_error.argtypes = [vp]
        L.cmpc_last_error.restype = C.c_char_p
        L.cmpc_batch.argtypes = [vp]
        if hasattr(L, "cmpc_factor_storage"):
            L.cmpc_factor_storage.argtypes = [vp]
        L.cmpc_stream.argtypes = [vp]
        L.cmpc_stream.restype = vp
        L.cmpc_solve_device.argtypes = [vp, fp, fp, fp, fp, vp]
        if hasattr(L, "cmpc_solve_device_warm"):   # (absent from round-2 builds of the library, which tools/ab_bench.sh may load as the baseline)
            L.cmpc_solve_device_warm.argtypes = [vp, fp, fp, fp, fp, vp]
        L.cmpc_solve.argtypes = [vp, fp, fp, fp, fp]
        L.cmpc_last_solve_ms.argtypes = [vp]
        if hasattr(L, "cmpc_set_timing"):
            L.cmpc_set_timing.argtypes = [vp, C.c_int]
        if hasattr(L, "cmpc_set_warm_policy"):
            L.cmpc_set_warm_policy.argtypes = [vp, C.c_int, C.c_int]
        L.cmpc_test_poison_lds.argtypes = [vp]
        L.cmpc_compact_output_device.argtypes = [vp, fp, fp, fp, vp]
        L.cmpc_last_solve_ms.restype = C.c_float
        L.cmpc_eval_nlp_device.argtypes = [vp, fp, fp, fp, C.c_float, fp, fp, fp, fp, fp, vp]
        L.cmpc_nlp_sparsity.argtypes = [C.c_int, vp, vp, vp, vp]
        L.cmpc_set_state.argtypes = [vp, fp, fp]
        L.cmpc_set_reference.argtypes = [vp, fp, fp]
        L.cmpc_set_contacts.argtypes = [vp, fp, fp, fp, fp, fp, fp]
        L.cmpc_set_initial_guess.argtypes = [vp, fp, C.c_int]
        L.cmpc_advance.argtypes = [vp]
        L.cmpc_get_solution.argtypes = [vp, fp, fp]
        L.cmpc_get_output.argtypes = [vp, fp, fp, fp, vp]
        L.cmpc_set_reference_from_planner.argtypes = [vp, fp, fp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
        L.cmpc_plant_step_device.argtypes = [vp, fp, fp, fp, fp, fp, C.c_double, C.c_int, C.c_double, C.c_double, vp]
        d, i = C.c_double, C.c_int
        L.cmpc_contacts_merge.argtypes = [i, i, d, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cmpc_contacts_merge_device.argtypes = [vp, i, d, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "cmpc_contacts_force_sample_time"):
            L.cmpc_contacts_force_sample_time.argtypes = [i, i, d, vp, vp, vp, vp]
            L.cmpc_contacts_force_sample_time_device.argtypes = [vp, i, d, vp, vp, vp, vp, vp]
        L.cmpc_contacts_sample.argtypes = [i, d, i, i, d, vp, vp, vp, vp, vp, vp, vp]
        L.cmpc_contacts_sample_device.argtypes = [vp, i, d, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cmpc_set_contact_lists.argtypes = [vp, i, d, vp, vp, vp, vp, vp, vp]
        L.cmpc_contacts_adjust.argtypes = [i, i, i, d, vp, vp, vp, vp, vp]
        L.cmpc_contacts_adjust_device.argtypes = [vp, i, d, vp, vp, vp, vp, vp, vp]
        L.cmpc_write_state_device.argtypes = [vp, fp, fp, fp, vp]
        L.cmpc_shift_solution_device.argtypes = [vp, fp, fp, vp]
        L.cmpc_eval_nlp_grad_device.argtypes = [vp, fp, fp, fp, C.c_float, fp, fp, vp]
        L.cmpc_set_multiplier_output.argtypes = [vp, C.c_int]
        L.cmpc_get_multipliers_device.argtypes = [vp, fp, fp, fp, vp]
        L.cmpc_get_multipliers.argtypes = [vp, fp]
        L.cmpc_kkt_certificate_device.argtypes = [vp, fp, fp, fp, fp, vp]
        L.cmpc_value_gradient_device.argtypes = [vp, fp, fp, fp, fp, vp]
        L.cmpc_solution_jvp_device.argtypes = [vp, fp, fp, fp, fp, C.c_int, fp, fp, vp]
        L.cmpc_solution_vjp_device.argtypes = [vp, fp, fp, fp, fp, fp, fp, vp]
        L.cmpc_sensitivity_workspace_bytes.argtypes = [C.c_int]
        L.cmpc_sensitivity_workspace_bytes.restype = C.c_size_t
        if hasattr(L, "cmpc_solution_jvp_model_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_solution_jvp_model_device.argtypes = [vp, fp, fp, fp, fp, vp, C.c_int, fp, fp, vp]
            L.cmpc_solution_vjp_model_device.argtypes = [vp, fp, fp, fp, fp, fp, vp, fp, vp]
            L.cmpc_model_value_gradient_device.argtypes = [vp, fp, fp, fp, vp, vp]
        if hasattr(L, "cmpc_solution_jvp_rot_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_solution_jvp_rot_device.argtypes = [vp, fp, fp, fp, fp, vp, vp, C.c_int, fp, fp, vp]
            L.cmpc_solution_vjp_rot_device.argtypes = [vp, fp, fp, fp, fp, fp, vp, vp, fp, vp]
            L.cmpc_rotation_value_gradient_device.argtypes = [vp, fp, fp, fp, vp, vp]
            L.cmpc_contacts_rotation_vjp_device.argtypes = [vp, i, d, vp, vp, vp, vp, vp]
        if hasattr(L, "cmpc_solution_vjp_cols_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_solution_vjp_cols_device.argtypes = [vp, fp, fp, fp, fp, C.c_int, fp, vp, vp, fp, vp]
        L.cmpc_plant_step_jvp_device.argtypes = [vp, fp, fp, fp, d, i, vp, fp, fp, vp, vp, vp]
        L.cmpc_plant_step_vjp_device.argtypes = [vp, fp, fp, fp, d, i, vp, vp, fp, fp, vp, vp]
        L.cmpc_contacts_position_vjp_device.argtypes = [vp, i, d, i, i] + [vp] * 15
        L.cmpc_rollout_tick_vjp_device.argtypes = [vp, i, d, C.POINTER(CmpcTickTape)] + [vp] * 11
        if hasattr(L, "cmpc_rollout_tick_vjp_rot_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_plant_step_jvp_rot_device.argtypes = [vp, fp, fp, fp, d, i, vp, fp, fp, vp, vp, vp, vp]
            L.cmpc_plant_step_vjp_rot_device.argtypes = [vp, fp, fp, fp, d, i, vp, vp, fp, fp, vp, vp, vp]
            L.cmpc_contacts_orientation_vjp_device.argtypes = [vp, i, d, i] + [vp] * 14
            L.cmpc_rollout_tick_vjp_rot_device.argtypes = [vp, i, d, C.POINTER(CmpcTickTape)] + [vp] * 15
        if hasattr(L, "cmpc_rollout_tick_jvp_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_plant_step_jvp_cols_device.argtypes = [vp, fp, fp, fp, d, i, i, vp, fp, fp, vp, vp, vp, vp]
            L.cmpc_contacts_jvp_device.argtypes = [vp, i, d, i, i, i] + [vp] * 19
            L.cmpc_rollout_tick_jvp_device.argtypes = [vp, i, d, C.POINTER(CmpcTickTape), i, C.POINTER(CmpcTickDirs), C.POINTER(CmpcTickDirsOut), vp, vp]
        if hasattr(L, "cmpc_get_parameters"):   # (absent from earlier rounds' builds of the library, which tools/ab_multi.sh may load as a baseline)
            L.cmpc_get_parameters.argtypes = [vp, fp]
            L.cmpc_get_parameters_device.argtypes = [vp, C.POINTER(vp)]
            L.cmpc_allgather_compact_device.argtypes = [vp, vp, C.c_int, fp, fp, vp]
        if hasattr(L, "cmpc_rollout_tick_device"):
            L.cmpc_rollout_tick_device.argtypes = [vp, i, d, i, C.POINTER(CmpcTickIO), vp]
        if hasattr(L, "cmpc_write_reference_from_planner_device"):
            L.cmpc_write_reference_from_planner_device.argtypes = [vp, fp, fp, i, d, d, d, d, fp, vp]
        if hasattr(L, "cmpc_rollout_walk_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            rp = C.POINTER(CmpcWalkRecord)
            L.cmpc_rollout_record.argtypes = [i, i, i, i] + [vp] * 9 + [rp]
            L.cmpc_rollout_record_device.argtypes = [vp, i, i] + [vp] * 7 + [rp, vp]
            L.cmpc_rollout_outcome_init_device.argtypes = [vp, vp, rp, vp]
            L.cmpc_cold_start_device.argtypes = [vp, fp, fp, vp]
            L.cmpc_rollout_walk_device.argtypes = [vp, i, i, i, i, C.POINTER(CmpcWalkIO), rp, i, i, ip, vp]
        if hasattr(L, "cmpc_set_ended_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_set_ended_device.argtypes = [vp, vp]
        if hasattr(L, "cmpc_set_walk_limits"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            lp = C.POINTER(CmpcWalkLimits)
            L.cmpc_set_walk_limits.argtypes = [vp, lp]
            L.cmpc_walk_extremes_init_device.argtypes = [vp, vp, vp]
            L.cmpc_rollout_record_limits.argtypes = [i, i, i, i] + [vp] * 9 + [C.POINTER(CmpcWalkRecord), lp, vp, i, d]
        if hasattr(L, "cmpc_rollout_walk_vjp_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            tp = C.POINTER(CmpcWalkTape)
            L.cmpc_rollout_tape_device.argtypes = [vp, i, i, i] + [vp] * 11 + [tp, vp]
            L.cmpc_rollout_walk_taped_device.argtypes = [vp, i, i, i, i, C.POINTER(CmpcWalkIO), C.POINTER(CmpcWalkRecord), i, i, ip, tp, i, vp]
            L.cmpc_rollout_walk_vjp_device.argtypes = [vp, i, i, i, tp, i, vp, C.POINTER(CmpcWalkGrads), vp]
            L.cmpc_rollout_walk_vjp_gate.argtypes = [C.POINTER(CmpcWalkGate)]
            L.cmpc_rollout_walk_vjp_gate_device.argtypes = [vp, C.POINTER(CmpcWalkGate), vp]
            if hasattr(L, "cmpc_rollout_walk_vjp_rot_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
                L.cmpc_rollout_walk_vjp_rot_device.argtypes = [vp, i, i, i, tp, i, vp, C.POINTER(CmpcWalkGrads), C.POINTER(CmpcWalkGradsRot), vp]
                L.cmpc_rollout_walk_vjp_rot_gate.argtypes = [C.POINTER(CmpcWalkGateRot)]
                L.cmpc_rollout_walk_vjp_rot_gate_device.argtypes = [vp, C.POINTER(CmpcWalkGateRot), vp]
        if hasattr(L, "cmpc_rollout_walk_jvp_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_rollout_walk_jvp_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkTape), i, vp, i, C.POINTER(CmpcWalkDirs), vp]
            L.cmpc_rollout_walk_jvp_gate.argtypes = [C.POINTER(CmpcWalkJvpGate)]
            L.cmpc_rollout_walk_jvp_gate_device.argtypes = [vp, C.POINTER(CmpcWalkJvpGate), vp]
        if hasattr(L, "cmpc_walk_measures_vjp_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_walk_measures_vjp_device.argtypes = [vp, i, i, C.POINTER(CmpcWalkTape), i, vp, C.POINTER(CmpcWalkMeasureGrads), vp]
            L.cmpc_walk_measures_vjp_fold_device.argtypes = [vp, i, vp, vp, vp, vp]
            L.cmpc_walk_measures_jvp_device.argtypes = [vp, i, i, C.POINTER(CmpcWalkTape), i, vp, i, C.POINTER(CmpcWalkMeasureDirs), vp]
            L.cmpc_walk_measures_vjp.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, i, d, vp, vp, vp, vp]
            L.cmpc_walk_measures_vjp_fold.argtypes = [i, i, i, vp, vp, vp]
            L.cmpc_walk_measures_jvp.argtypes = [i, i, i, i, i, vp, vp, vp, vp, vp, i, d, vp, vp, vp, vp, vp]
            L.cmpc_walk_measures_jacobian.argtypes = [i, i, i, vp, vp, vp, vp, i, d, vp]
        if hasattr(L, "cmpc_reference_from_planner_vjp"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            pr = C.POINTER(CmpcPlannerRefs)
            L.cmpc_reference_from_planner_vjp.argtypes = [i, d, i, i, i, pr, vp, vp, vp, vp]
            L.cmpc_reference_from_planner_vjp_device.argtypes = [vp, i, i, pr, vp, vp, vp, vp, vp]
            L.cmpc_reference_from_planner_jvp.argtypes = [i, d, i, i, i, i, pr, vp, vp, vp]
            L.cmpc_reference_from_planner_jvp_device.argtypes = [vp, i, i, i, pr, vp, vp, vp, vp]
        if hasattr(L, "cmpc_rollout_snapshot_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            sp = C.POINTER(CmpcWalkSnapshot)
            L.cmpc_rollout_snapshot_device.argtypes = [vp, i, i, sp, sp, vp, vp, vp]
            L.cmpc_rollout_snapshot.argtypes = [i, i, i, i, sp, sp, vp, vp]
            L.cmpc_walk_snapshot_bytes.argtypes = [i, i]
            L.cmpc_walk_snapshot_bytes.restype = C.c_size_t
        if hasattr(L, "cmpc_rollout_walk_mismatch_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            mp = C.POINTER(CmpcPlantMismatch)
            L.cmpc_plant_step_mismatch_device.argtypes = [vp, fp, fp, fp, fp, fp, d, i, d, d, vp, vp, vp]
            L.cmpc_rollout_tick_mismatch_device.argtypes = [vp, i, d, i, C.POINTER(CmpcTickIO), i, mp, vp]
            L.cmpc_rollout_walk_mismatch_device.argtypes = [vp, i, i, i, i, C.POINTER(CmpcWalkIO), C.POINTER(CmpcWalkRecord), i, i, ip,
                                                            C.POINTER(CmpcWalkTape), i, mp, vp]
            L.cmpc_plant_step_vjp_mismatch_device.argtypes = [vp, fp, fp, fp, d, i, vp, vp, fp, fp, vp, vp, vp, vp, vp, vp, vp]
            L.cmpc_rollout_tick_vjp_mismatch_device.argtypes = [vp, i, d, C.POINTER(CmpcTickTape)] + [vp] * 20
            L.cmpc_rollout_walk_vjp_mismatch_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkTape), i, vp, C.POINTER(CmpcWalkGrads),
                                                                C.POINTER(CmpcWalkGradsRot), mp, C.POINTER(CmpcWalkGradsMismatch), vp]
        if hasattr(L, "cmpc_rollout_walk_jvp_mismatch_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            L.cmpc_plant_step_jvp_mismatch_cols_device.argtypes = [vp, fp, fp, fp, d, i, i, vp, fp, fp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.cmpc_rollout_tick_jvp_mismatch_device.argtypes = [vp, i, d, C.POINTER(CmpcTickTape), i, C.POINTER(CmpcTickDirs), C.POINTER(CmpcTickDirsOut), vp,
                                                                vp, vp, C.POINTER(CmpcTickDirsMismatch), vp]
            L.cmpc_rollout_walk_jvp_mismatch_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkTape), i, vp, i, C.POINTER(CmpcWalkDirs),
                                                                C.POINTER(CmpcPlantMismatch), C.POINTER(CmpcWalkDirsMismatch), vp]
        if hasattr(L, "cmpc_rollout_walk_sensed_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            mp, sn = C.POINTER(CmpcPlantMismatch), C.POINTER(CmpcWrenchSensor)
            L.cmpc_wrench_sense.argtypes = [i, i, i, i, mp, sn, vp, vp, vp]
            L.cmpc_wrench_sense_device.argtypes = [vp, i, i, mp, sn, vp, vp, vp, vp]
            L.cmpc_rollout_walk_sensed_device.argtypes = [vp, i, i, i, i, C.POINTER(CmpcWalkIO), C.POINTER(CmpcWalkRecord), i, i, ip,
                                                          C.POINTER(CmpcWalkTape), i, mp, sn, vp, vp]
            L.cmpc_wrench_sense_vjp.argtypes = [i, i, i, i, mp, sn, vp, vp, vp, vp]
            L.cmpc_wrench_sense_vjp_device.argtypes = [vp, i, i, mp, sn, vp, vp, vp, vp, vp]
            L.cmpc_wrench_sense_jvp.argtypes = [i, i, i, i, i, mp, sn, vp, vp, vp, vp]
            L.cmpc_wrench_sense_jvp_device.argtypes = [vp, i, i, i, mp, sn, vp, vp, vp, vp, vp]
        if hasattr(L, "cmpc_rollout_walk_refill_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
            fl, wr = C.POINTER(CmpcWalkRefill), C.POINTER(CmpcWalkRecord)
            L.cmpc_rollout_refill_init.argtypes = [i, fl]
            L.cmpc_rollout_refill_init_device.argtypes = [vp, fl, vp]
            L.cmpc_rollout_refill.argtypes = [i, i, wr, fl, vp]
            L.cmpc_rollout_refill_device.argtypes = [vp, i, wr, fl, vp, vp]
            L.cmpc_rollout_walk_refill_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkIO), wr, fl, i, i, ip, vp]
            if hasattr(L, "cmpc_rollout_walk_refill_trials_device"):
                L.cmpc_rollout_walk_refill_trials_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkIO), wr, fl, C.POINTER(CmpcWalkRefillTrials), i, i, ip, vp]
            if hasattr(L, "cmpc_rollout_walk_refill_snapshot_device"):
                fs = C.POINTER(CmpcWalkRefillSnapshot)
                L.cmpc_rollout_walk_refill_snapshot_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkIO), wr, fl, C.POINTER(CmpcWalkRefillTrials), fs, i, i, ip, vp]
                L.cmpc_rollout_refill_restore.argtypes = [i, i, i, i, C.POINTER(CmpcWalkSnapshot), fl, fs]
            if hasattr(L, "cmpc_rollout_walk_refill_taped_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
                tp, rg = C.POINTER(CmpcWalkTape), C.POINTER(CmpcWalkTapeRegroup)
                L.cmpc_rollout_walk_refill_taped_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkIO), wr, fl, C.POINTER(CmpcWalkRefillTrials), i, i, ip,
                                                                    tp, i, vp]
                L.cmpc_rollout_tape_regroup_device.argtypes = [vp, i, tp, fl, rg, tp, vp]
                L.cmpc_rollout_tape_regroup.argtypes = [i, i, i, tp, fl, rg, tp]
            if hasattr(L, "cmpc_rollout_walk_refill_plans_device"):   # (absent from earlier builds, which tools/ab_*.sh may load as a baseline)
                pl = C.POINTER(CmpcWalkRefillPlans)
                L.cmpc_rollout_walk_refill_plans_device.argtypes = [vp, i, i, i, C.POINTER(CmpcWalkIO), wr, fl, C.POINTER(CmpcWalkRefillTrials), pl, i, i, ip,
                                                                    C.POINTER(CmpcWalkTape), i, vp]
                L.cmpc_rollout_refill_plans.argtypes = [i, i, i, fl, pl, wr, i]
                L.cmpc_rollout_plan_fold_device.argtypes = [vp, i, i, vp, vp, i, vp, vp]
                L.cmpc_rollout_plan_fold.argtypes = [i, i, vp, vp, i, vp]
        if hasattr(L, "cmpc_set_models"):
            L.cmpc_model_from_config.argtypes = [C.POINTER(CmpcConfig), C.POINTER(CmpcModel)]
            L.cmpc_model_from_config.restype = None
            L.cmpc_check_models.argtypes = [vp, i]
            L.cmpc_set_models.argtypes = [vp, vp]
            L.cmpc_set_models_device.argtypes = [vp, vp, vp, vp]
        _lib = L
    return _lib
