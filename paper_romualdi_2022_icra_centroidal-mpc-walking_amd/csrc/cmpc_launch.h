// The launchers and size queries that cross a translation unit: declared once, here.  The three files of the C ABI call them (cmpc_api.hip,
// cmpc_api_rollout.hip and cmpc_api_walk_grad.hip, through cmpc_handle.h), and no launcher reads a handle; every file that defines one includes
// this header too, so that a definition that drifts from its declaration is a compile error (extern "C" functions cannot be overloaded) and not
// a wrong address in a kernel argument.
#pragma once
#include "cmpc_contacts.h"
#include "cmpc_device.h"

extern "C" {

// ---- cmpc_solver.hip ----
size_t cmpc_solver_lds_bytes(int N, int factors_global);
int cmpc_launch_solver(const CmpcParams* prm, size_t lds_bytes, hipStream_t stream);
int cmpc_prepare_solver(int N, int factors_global, size_t lds_bytes);

// ---- cmpc_nlp_eval.hip ----
int cmpc_launch_nlp_eval(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG,
                         float lam_f, float* dF, float* dG, float* dGradF, float* dJac, float* dHess,
                         hipStream_t stream);
int cmpc_launch_nlp_grad(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, float lam_f, float* dGradX,
                         float* dGradP, hipStream_t stream);
int cmpc_launch_multipliers(const CmpcParams* prm, const float* dX, const float* dP, float* dLamG, hipStream_t stream);
int cmpc_launch_kkt_certificate(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, float* dCert, hipStream_t stream);
int cmpc_launch_value_gradient(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, float* dGradP, hipStream_t stream);
int cmpc_launch_model_value_gradient(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, double* dGradModel,
                                     hipStream_t stream);
int cmpc_launch_rotation_value_gradient(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, double* dGradRot,
                                        hipStream_t stream);

// ---- cmpc_rollout.hip ----
int cmpc_launch_warm_shift(const CmpcParams* prm, const float* dXprev, float* dX0, hipStream_t stream);
int cmpc_launch_compact(int N, int B, const float* dX, const float* dInfo, float* dOut, hipStream_t stream);
int cmpc_launch_tick_pre(int B, int N, int M, double dt, double now, int merge, const double* plan_t, const float* plan_pose, const int* plan_n,
                         const double* prev_t, const float* prev_pose, const int* prev_n, double* list_t, float* list_pose, int* list_n, int* ok,
                         int* land, const float* box, const float* state, const float* wrench, float* P, const float* Xprev, float* X0,
                         const float* plan_com, const float* plan_h, int plan_knots, double plan_dt, double plan_t_offset, double robot_mass,
                         double com_height, long long snap_dt_ns, const int* snap_ok, const int* ended, const float* noise, hipStream_t stream);
int cmpc_launch_tick_post(int B, int N, int M, double now, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                          const float* dStateIn, float* dStateOut, float* dZmp, float h, int nsub, float zx, float zy, const int* land,
                          const double* t, float* pose, const int* n, const int* ended, const float* hidden, const float* gain, hipStream_t stream);
int cmpc_launch_rollout_record(const CmpcRecordArgs* a, int* stats, hipStream_t stream);
int cmpc_launch_rollout_record_limits(const CmpcRecordArgs* a, const CmpcLimitArgs* lm, int* stats, hipStream_t stream);
int cmpc_launch_extremes_init(int B, float* ext, hipStream_t stream);
int cmpc_launch_walk_measures_vjp(const CmpcMeasureVjpArgs* v, hipStream_t stream);
int cmpc_launch_walk_measures_fold(int N, int B, int rows, const double* direct, float* grad_p, double* grad_model, hipStream_t stream);
int cmpc_launch_walk_measures_jvp(const CmpcMeasureJvpArgs* v, hipStream_t stream);
int cmpc_launch_wrench_sense(const CmpcSenseArgs* a, float* wrench_rows, float* plant_rows, int* pass_rows, hipStream_t stream);
int cmpc_launch_wrench_sense_vjp(const CmpcSenseVjpArgs* v, hipStream_t stream);
int cmpc_launch_wrench_sense_jvp(const CmpcSenseJvpArgs* v, hipStream_t stream);
int cmpc_launch_outcome_init(int B, const float* state0, int* end_tick, int* end_code, int* it_sum, int* it_max, float* final_state,
                             float* slack_min, hipStream_t stream);
int cmpc_launch_cold_start(int N, int B, float g8, const float* dP, float* dX0, const int* ended, hipStream_t stream);
int cmpc_launch_refill(const CmpcRefillArgs* a, int* next, hipStream_t stream);
int cmpc_launch_refill_init(const CmpcRefillArgs* a, int* next, hipStream_t stream);
int cmpc_launch_tick_pre_refill(int B, int N, int M, double dt, const double* plan_t, const float* plan_pose, const int* plan_n,
                                const double* prev_t, const float* prev_pose, const int* prev_n, double* list_t, float* list_pose, int* list_n,
                                int* ok, int* land, const float* box, const float* state, float* P, const float* Xprev, float* X0,
                                const float* plan_com, const float* plan_h, int plan_knots, double plan_dt, double robot_mass, double com_height,
                                long long snap_dt_ns, const int* ended, const int* start, const int* trial, int tick, const float* wrench_trials,
                                int wrench_ticks, int trials, double plan_t_first, float g8, const CmpcRefillTrialArgs* tr,
                                int offset, hipStream_t stream);
int cmpc_launch_tick_post_refill(int B, int N, int M, double dt, float grav, const float* dCorners, int corners_stride, const float* dX,
                                 const float* dP, const float* dStateIn, float* dStateOut, float* dZmp, float h, int nsub, float zx, float zy,
                                 const int* land, const double* t, float* pose, const int* n, const int* ended, const int* start, int tick,
                                 const int* trial, const CmpcRefillTrialArgs* tr, int offset, hipStream_t stream);
int cmpc_launch_refill_restore(const CmpcRefillRestoreArgs* a, hipStream_t stream);
int cmpc_launch_refill_plans(const CmpcRefillPlansArgs* a, hipStream_t stream);
int cmpc_launch_plan_fold(int Q, int words, const int* index, const double* per, int pool_rows, double* out, hipStream_t stream);
int cmpc_launch_rollout_tape(const CmpcTapeArgs* a, hipStream_t stream);
int cmpc_launch_rollout_snapshot(const CmpcSnapshotArgs* a, hipStream_t stream);
int cmpc_launch_rollout_tape_regroup(const CmpcRegroupArgs* a, hipStream_t stream);
int cmpc_launch_walk_vjp_gate(const CmpcGateArgs* a, hipStream_t stream);
size_t cmpc_walk_gate_wide_entries(const CmpcGateArgs* a);
int cmpc_launch_walk_jvp_gate(const CmpcJvpGateArgs* a, hipStream_t stream);
size_t cmpc_walk_jvp_gate_wide_entries(const CmpcJvpGateArgs* a);
int cmpc_launch_plant_step(int N, int B, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                           const float* dStateIn, float* dStateOut, float* dZmp, float h, int nsub, float zx, float zy,
                           const float* dHidden, const float* dGain, hipStream_t stream);
int cmpc_launch_plant_jvp(int N, int B, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                          const float* dStateIn, float h, int nsub, const double* dDirState, const float* dDirX, const float* dDirP,
                          const double* dDirModel, const double* dDirRot0, double* dOut, hipStream_t stream);
int cmpc_launch_plant_vjp(int N, int B, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                          const float* dStateIn, float h, int nsub, const double* dGradOut, double* dGradState, float* dGradX, float* dGradP,
                          double* dGradModel, double* dGradRot0, int mismatch, const float* dHidden, const float* dGain, double* dGradHidden,
                          double* dGradGain, hipStream_t stream);
int cmpc_launch_axpy_float(size_t n, const float* x, float* y, hipStream_t stream);
int cmpc_launch_tick_vjp_combine(int B, int N, const float* info, const int* ok, const float* gp_sol, const float* gp_plant, const double* gm_sol,
                                 const double* gm_plant, double* g_state, float* g_wrench, double* g_model, float* g_p, float* sens, int* ok_out,
                                 const double* g_rot0, double* g_rot, const double* gh_plant, const double* gg_plant, double* g_hidden, float* g_noise,
                                 double* g_gain, hipStream_t stream);
int cmpc_launch_tick_jvp_assemble(size_t cols, int N, const double* d_state, const float* d_wrench, const float* d_extra, float* d_p, const float* d_noise,
                                  hipStream_t stream);
int cmpc_launch_tick_jvp_flag(int B, int N, int K, const float* info, const int* ok, const float* state_in, float* sens, float* d_x, float* d_p, double* d_rot,
                              double* d_rot0, int* ok_out, hipStream_t stream);
int cmpc_launch_plant_jvp_cols(int N, int B, int K, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                               const float* dStateIn, float h, int nsub, const double* dDirState, const float* dDirX, const float* dDirP,
                               const double* dDirModel, const double* dDirRot0, const int* dOk, double* dOut, hipStream_t stream);
int cmpc_launch_plant_jvp_cols_mismatch(int N, int B, int K, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                                        const float* dStateIn, float h, int nsub, const double* dDirState, const float* dDirX, const float* dDirP,
                                        const double* dDirModel, const double* dDirRot0, const int* dOk, double* dOut, int mismatch, const float* dHidden,
                                        const float* dGain, const double* dDirHidden, const double* dDirGain, hipStream_t stream);

// ---- cmpc_contacts.hip ----
int cmpc_launch_contacts_rotation_vjp(int B, int N, int M, double dt, double now, const double* list_t, const int* list_n, const double* g_rot,
                                      double* g_list, hipStream_t stream);
int cmpc_launch_contacts_merge(int B, int M, double now, const double* plan_t, const float* plan_pose, const int* plan_n,
                               const double* mpc_t, const float* mpc_pose, const int* mpc_n, double* out_t, float* out_pose,
                               int* out_n, int* ok, hipStream_t stream);
int cmpc_launch_contacts_sample(int B, int N, int M, double dt, double now, const double* t, const float* pose, const int* n,
                                const float* box, float* P, int* land, hipStream_t stream);
int cmpc_launch_contacts_adjust(int B, int N, int M, double now, const float* X, const int* land, const double* t, float* pose,
                                const int* n, hipStream_t stream);
int cmpc_launch_write_state(int B, int N, const float* state, const float* wrench, float* P, hipStream_t stream);
int cmpc_launch_reference_from_planner(int B, int N, int n_in, double dt, double in_dt, double t_offset, double robot_mass, double com_height,
                                       const float* com_in, const float* h_in, float* P, hipStream_t stream);
int cmpc_launch_reference_vjp(const CmpcRefArgs* a, const int* end_tick, const float* grad_p, double* grad_com, double* grad_h, hipStream_t stream);
int cmpc_launch_reference_jvp(const CmpcRefArgs* a, const double* dir_com, const double* dir_h, float* dir_p, hipStream_t stream);
int cmpc_launch_force_sample_time(int B, int M, long long dt_ns, const double* t, const int* n, double* out_t, int* ok, int ok_per_foot,
                                  const int* ended, hipStream_t stream);
int cmpc_launch_contacts_orientation_vjp(int B, int N, int M, double dt, double now, long long snap_dt_ns, const double* plan_t, const int* plan_n,
                                         const double* prev_t, const int* prev_n, const double* list_t, const int* list_n, const int* land,
                                         const int* ok, const double* g_out, const double* g_rot, double* g_prev, double* g_plan, int* status,
                                         hipStream_t stream);
int cmpc_launch_contacts_position_vjp(int B, int N, int M, double dt, double now, int phase, long long snap_dt_ns, const double* plan_t,
                                      const int* plan_n, const double* prev_t, const int* prev_n, const double* list_t, const int* list_n,
                                      const int* land, const int* ok, const double* g_out, const float* g_p, float* g_x, double* g_prev,
                                      double* g_plan, int* status, hipStream_t stream);
int cmpc_launch_contacts_jvp(int B, int N, int M, int K, double dt, double now, int phase, long long snap_dt_ns, const double* plan_t,
                             const int* plan_n, const double* prev_t, const int* prev_n, const double* list_t, const int* list_n, const int* land,
                             const int* ok, const double* d_prev, const double* d_prev_rot, const double* d_plan, const double* d_plan_rot,
                             const float* d_x, double* d_list, double* d_list_rot, float* d_p, double* d_rot, int* status, hipStream_t stream);

// ---- cmpc_sensitivity.hip ----
int cmpc_launch_sensitivity(const CmpcConsts* kc, int kc_per_problem, int N, int b0, int nb, const float* dX, const float* dP, const float* dLamG,
                            const float* dDir, const float* dGradX, int kdir, float* dOut, float* dSens, double* dWs, const double* dDirModel,
                            double* dGradModel, const double* dDirRot, double* dGradRot, hipStream_t stream);

}  // extern "C"
