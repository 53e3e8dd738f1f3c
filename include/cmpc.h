/* cmpc.h -- C ABI of the MI355X batched centroidal-MPC solver (libcmpc_hip.so).
 *
 * Drop-in boundary for ONE path of GiulioRomualdi/paper_romualdi_2022_icra_centroidal-mpc-walking:
 * the solve inside BipedalLocomotion::ReducedModelControllers::CentroidalMPC, as the reference
 * drives it from src/centroidal-mpc-walking/src/CentroidalMPCBlock.cpp:
 *     initialize              :144   -> cmpc_create            (keys of config/robots/<robot>/centroidal_mpc.ini)
 *     setState                :407   -> cmpc_set_state
 *     setReferenceTrajectory  :579   -> cmpc_set_reference
 *     setContactPhaseList     :609   -> cmpc_set_contacts
 *     advance                 :615   -> cmpc_solve / cmpc_solve_device   (replaces CasADi Opti -> IPOPT)
 *     getOutput               :622   -> cmpc_get_solution / cmpc_get_output
 * and the NLP callbacks IPOPT would call (generated code config/robots/ergoCubGazeboV1/tmp.c:
 * nlp_fg :12430, nlp_jac_fg :71962, nlp_hess_l :58926) -> cmpc_eval_nlp_device; nlp_grad :24791 -> cmpc_eval_nlp_grad_device.
 *
 * Conventions: plain C, no exceptions; every function returns 0 on success or a negative
 * cmpc_status; cmpc_last_error() gives the text.  The caller owns every buffer it passes; the
 * handle owns its device buffers; one handle = one device + one HIP stream, single caller
 * (the reference calls the class from one thread, Main.cpp:98-110).
 *
 * Data layout: decision vector x[n_x] and parameter vector p[n_p] of every problem are laid out
 * exactly as in the reference's generated NLP (tmp.c:62-67): n_x = 45N+15, n_p = 50N+27,
 *   x = com[3(N+1)] dcom[3(N+1)] h[3(N+1)] then per contact (left_foot, right_foot):
 *       pos[3(N+1)] vel[3N] f_corner0..3[3N each]           (3 x knots, column-major)
 *   p = per contact: R[9N] (vec of 3x3 col-major per knot) upper[3N] lower[3N] enabled[N]
 *       nominalPos[3(N+1)] currentPos[3]; then com0 dcom0 h0 comRef[3(N+1)] hRef[3(N+1)]
 *       fExt[3N] tauExt[3N]
 * Batches are row-major: P[B][n_p], X[B][n_x], float32.
 */
#ifndef CMPC_H
#define CMPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cmpc_handle_s* cmpc_handle;

typedef enum {
    CMPC_OK = 0,
    CMPC_ERR_ARG = -1,       /* bad argument / unsupported configuration */
    CMPC_ERR_HIP = -2,       /* HIP runtime error (no device, allocation, launch) */
    CMPC_ERR_NOT_CONVERGED = -3 /* at least one problem of the batch did not converge (see info) */
} cmpc_status;

/* keys of centroidal_mpc.ini (ergoCubGazeboV1/centroidal_mpc.ini:3-42) + solver options */
typedef struct {
    int horizon;              /* N = time_horizon / sampling_time (or controller_horizon)        */
    double sampling_time;     /* dt                                                               */
    double friction_coefficient; /* static_friction_coefficient (number_of_slices must be 1)      */
    double gravity;           /* 9.80665                                                          */
    double com_weight[3];
    double angular_momentum_weight;
    double contact_position_weight;
    double force_rate_of_change_weight[3];
    double contact_force_symmetry_weight;
    double corners[2][4][3];  /* [CONTACT_i] corner_j, contacts in alphabetical name order        */
    /* solver options (ipopt_tolerance / ipopt_max_iteration take the place of IPOPT's) */
    int max_iterations;       /* Newton iteration budget per solve (default 40)                   */
    double tolerance;         /* on the primal residuals and on max t*z (<= 0: default 1e-6 for N = 4 .. 20, 3e-7 beyond and for N <= 3) */
    double step_tolerance;    /* on the last Newton step, max-norm over states and forces (default 1e-4) */
    double mu_init;           /* initial barrier parameter; <= 0 (default): per problem, from its
                               * initial infeasibility ep0: clamp(3.5 ep0^2, 0.03, 0.5)           */
    double mu_min;            /* final barrier parameter (<= 0: default max(0.05 x tolerance, 5e-8): the float32 factorisations start to fail below) */
    int exact_hessian;        /* 1 (default): Lagrangian Hessian; 0: Gauss-Newton                 */
    int final_extrapolation;  /* 1 (default): a converged solve finishes with one affine-scaling Newton step towards
                               * mu = 0 (one more factorisation): removes the O(mu) bias of the barrier floor and
                               * the remaining termination error -- worst parity error of 1024 problems 8.7e-5 ->
                               * 1.7e-5 (config 2) for +0.8 iteration; 0: stop at the barrier floor */
    /* tail polish (needs final_extrapolation): when the extrapolation step of the forces of the last tail_stages stages
     * exceeds tail_trigger x the largest force component -- the symptom of nearly degenerate friction rows there, e.g. an
     * unloaded corner at the apex of its pyramid, which the barrier keeps sqrt(mu / curvature) away from the optimum --
     * those stages are re-solved on their own (state entering them held): tail_iterations Newton steps with per-row
     * barrier targets, then their own extrapolation step.  Defaults 3 / 2 / 2e-5; tail_stages 0 switches it off. */
    int tail_stages;
    int tail_iterations;
    double tail_trigger;
    /* where the per-stage factor records of the Riccati recursion live: CMPC_FACTORS_AUTO (default) = in LDS, one problem per compute unit, eight waves
     * (the latency variant) when the batch does not exceed the number of compute units and the horizon's image fits 160 KiB, else in HBM scratch with three
     * problems per compute unit (the throughput variant); CMPC_FACTORS_LDS / _HBM force one (LDS only where it fits).  Both give the same solutions to
     * the tolerance; tests use the switch to hold them together. */
    int factor_storage;
} cmpc_config;
#define CMPC_FACTORS_AUTO 0
#define CMPC_FACTORS_LDS 1
#define CMPC_FACTORS_HBM 2

/* number of floats per solve in the info array */
#define CMPC_INFO 8
/* info[b] = { iterations, kkt_error = max(primal_inf, max t*z), mu, safeguards, primal_inf,
 * status (0 ok, 1 iteration budget exhausted, 2 factorisation failed or a residual that is not finite -- NaN/inf in P or
 * X0: IPOPT's "invalid number", 3 outside the supported NLP subset, see below), solve_cycles (shader clock),
 * last_step (max-norm of the last Newton step taken inside the loop, forces relative to the largest force) }.
 * kkt_error, mu and primal_inf are those of the last iterate whose residuals were evaluated: the iterate the
 * termination test accepted.  With final_extrapolation the returned x is one affine-scaling step beyond it.
 * safeguards = Gauss-Newton fallbacks + 100 x emergency re-centrings (warm starts) + 10000 x (1 if the warm-started pass
 * was abandoned and the problem solved again from the cold start) + 100000 x (1 if the tail was polished)
 * + 1000000 x (times a wave of the streaming backward stage gave up waiting at a hand-off word: never observed; a protocol bug would show HERE and not
 * as a failed factorisation -- the pass is repeated once unchanged.  Tests, the soak tool and bench.py assert / report that this digit is zero).
 * iterations counts both passes of a restarted warm start: it can reach 2 x max_iterations. */

/* The supported NLP subset.  The solver keeps a foot's bounding-box row only in swing stages (there it bounds the landing offset); the
 * row of a stance stage is dropped as a constant or a duplicate.  That is exact when, for each foot c and stage k:
 *   1. Gamma_c,k is exactly 0 or 1;
 *   2. if foot c is in stance at every stage 0..k: R_k^T (current_c - nominal_c,k+1) lies in [lower_k - 1e-6, upper_k + 1e-6]
 *      (otherwise the reference NLP is infeasible);
 *   3. if stage k is in stance after a swing, k' being the last swing stage before it: R_k, nominal_c,k+1, lower_k and upper_k are
 *      bit-equal to R_k', nominal_c,k'+1, lower_k' and upper_k' (the row is then a duplicate of the landing row).
 * A problem that breaks the rule is not iterated: it comes back at once with status 3 and its initial iterate as x; the other problems
 * of the batch are untouched.  cmpc_set_contacts / cmpc_set_contact_lists write schedules inside the subset.  So does a problem whose row of a
 * per-problem model table set on the device breaks the model rule (cmpc_set_models_device, below: dOk[b] = 0). */
void cmpc_default_config(cmpc_config* cfg);                      /* ergoCubGazeboV1 values, N=20 */
/* sizes of the NLP at a horizon cmpc_create accepts (2 .. 40); CMPC_ERR_ARG, with the range in cmpc_last_error(NULL), outside it */
int cmpc_dims(int horizon, int* n_x, int* n_p, int* n_g, int* nnz_jac, int* nnz_hess);

/* the tolerance cmpc_create uses when cmpc_config.tolerance <= 0: 1e-6 for N = 4 .. 20, 3e-7 beyond and for N <= 3 (parity with the float64 solve
 * needs it).  A caller mapping the reference's ipopt_tolerance passes it only when it is tighter than this, and 0 otherwise. */
double cmpc_default_tolerance(int horizon);
/* Short horizons ("Both ends of the horizon range"; profiles/horizon_ends.txt).  Walking problems with pushes are inside the 1e-4 target
 * at every horizon 2 .. 40; the 3e-7 at N <= 3 is what that takes (at 1e-6: CoM velocity up to 1.9e-4 with status 0).  Standing problems with a
 * perturbed CoM are not, below N = 15: a weakly active friction row of the first stages stays at its barrier-floor bias, and a tighter tolerance
 * does not remove it.  Measured on MI355X, of 256 problems outside 1e-4 against the float64 optimum: N = 2: 57 (31 of them status 1, iteration
 * budget), N = 3: 60 (30 status 1), N = 4: 99 (CoM velocity 9.5e-3), N = 7: 21 (1.7e-3), N = 10: 4 (2.7e-4), N = 12: 0, N = 13: 1 (3.3e-4),
 * N = 20: 0.  The CPU model of the algorithm (oracle/ipm_ref.c) shows the same family: 37, 16, 24, 5, 1, 1, 1, 0. */
int cmpc_create(const cmpc_config* cfg, int batch, int device, cmpc_handle* out);
int cmpc_destroy(cmpc_handle h);
const char* cmpc_last_error(cmpc_handle h);                       /* h may be NULL */
int cmpc_batch(cmpc_handle h);
/* the storage the handle's kernel variant really uses: CMPC_FACTORS_LDS or CMPC_FACTORS_HBM.  A CMPC_FACTORS_LDS request at a horizon whose resident
 * image exceeds 160 KiB (N >= 23) is served by the HBM-factor variant: this is how a caller sees it. */
int cmpc_factor_storage(cmpc_handle h);
void* cmpc_stream(cmpc_handle h);                                 /* hipStream_t of the handle */

/* ---- the hot path: solve a batch, operands resident in device memory ----
 * dP[B][n_p], dX0[B][n_x] (initial guess), dX[B][n_x] (solution), dInfo[B][CMPC_INFO] or NULL.
 * Asynchronous on the handle's stream (or on `stream` if non-NULL); nothing is copied. */
int cmpc_solve_device(cmpc_handle h, const float* dP, const float* dX0, float* dX, float* dInfo,
                      void* stream);
/* the same when dX0 is the previous solution shifted by one knot (cmpc_shift_solution_device; is_warm_start_enabled,
 * ergoCubGazeboV1/centroidal_mpc.ini:9): the barrier starts near the central path (mu = 1e-2) and a problem whose warm
 * start does not converge is solved again inside the kernel from the cold start.  The warm property is this argument
 * list's, not the handle's: any buffer, any stream. */
int cmpc_solve_device_warm(cmpc_handle h, const float* dP, const float* dX0, float* dX, float* dInfo,
                           void* stream);
/* What a warm-started problem that does not converge costs (both cmpc_solve_device_warm and the class path): warm_budget =
 * iterations the warm-started pass may take (0: max_iterations; default 14: healthy warm ticks of the walking roll-out need at
 * most 13, and a tick is as slow as its slowest problem); restart_in_kernel != 0 (default): such a problem is then
 * started again from the cold start inside the same launch (info: safeguards += 10000); 0: it comes back with status 1 and
 * the caller re-solves it -- in a batch, the few stragglers of a tick in a small launch of their own (one CU each) instead of
 * one workgroup holding its CU for two budgets.  The reference can only abort the tick (CentroidalMPCBlock.cpp:615-619). */
int cmpc_set_warm_policy(cmpc_handle h, int warm_budget, int restart_in_kernel);
/* host buffers (includes the PCIe copies; synchronous). info may be NULL. Returns
 * CMPC_ERR_NOT_CONVERGED if any problem's status != 0 (the solutions are still written). */
int cmpc_solve(cmpc_handle h, const float* P, const float* X0, float* X, float* info);
/* duration of the last solve kernel in ms (HIP events on the launch stream); < 0 if none, or if timing is off */
float cmpc_last_solve_ms(cmpc_handle h);
/* The event pair every solve launch is bracketed with (what cmpc_last_solve_ms reads) costs the stream two barrier packets per solve: measured ~9 us each
 * between back-to-back launches on MI355X.  enabled = 0 stops recording them (a caller that queues solves back to back and times them itself);
 * default: enabled.  No reference counterpart (the reference times its tick on the host, CentroidalMPCBlock.cpp:615-634). */
int cmpc_set_timing(cmpc_handle h, int enabled);
/* test hook: fills the LDS of every compute unit with NaN bit patterns (a kernel on the handle's stream), so that a
 * test can show that a solve does not depend on what an earlier workgroup or kernel left there.  No reference
 * counterpart. */
int cmpc_test_poison_lds(cmpc_handle h);

/* ---- per-problem models ----
 * A problem's model is the part of cmpc_config a Monte-Carlo study randomises: friction, cost weights and foot corners.  Fields are named and
 * ordered as in cmpc_config: 34 packed doubles.  Everything else stays per handle: horizon, sampling_time, gravity, every solver option
 * (tolerances, budgets, mu_*, tail polish, factor_storage) and the warm policy (cmpc_set_warm_policy).
 * The model rule: friction_coefficient > 0 and finite; every weight finite and >= 0; each force_rate_of_change_weight > 0 (the Levenberg shift and
 * the float32 factorisations depend on it); corners finite. */
typedef struct {
    double friction_coefficient;
    double com_weight[3];
    double angular_momentum_weight;
    double contact_position_weight;
    double force_rate_of_change_weight[3];
    double contact_force_symmetry_weight;
    double corners[2][4][3];
} cmpc_model;
#define CMPC_MODEL_DOUBLES 34
void cmpc_model_from_config(const cmpc_config* cfg, cmpc_model* model);
/* checks models[0..batch) against the model rule on the host: CMPC_OK, or CMPC_ERR_ARG for the first failing problem, and cmpc_last_error(NULL) names
 * its index and field ("model 7: friction_coefficient = 0 must be > 0 and finite").  No handle, no GPU. */
int cmpc_check_models(const cmpc_model* models, int batch);
/* models[B] (host): problem b of every later launch of the handle -- cmpc_solve_device[_warm], cmpc_solve, cmpc_advance, the NLP evaluations,
 * cmpc_plant_step_device and cmpc_rollout_tick_device -- uses models[b] in place of the config's model.  The derived constants are bit-equal to those
 * of a handle created with that model in its config.  models is checked first (cmpc_check_models); on failure the handle keeps its previous table.
 * NULL returns the handle to its config's model for every problem.  Synchronous: waits for the device before the table is replaced. */
int cmpc_set_models(cmpc_handle h, const cmpc_model* models);
/* the same from a device table dModels[B] (e.g. randomised in a torch tensor), derived by a kernel on `stream` (NULL: the handle's); later launches
 * must be ordered after it.  Records are bit-equal to those of cmpc_set_models.  A row that breaks the model rule is not an error: dOk[b] = 0 (dOk[B] or
 * NULL; 1 otherwise), that problem's solves return status 3 and their initial iterate, and its NLP evaluations and plant steps use the config's model;
 * every other problem is untouched. */
int cmpc_set_models_device(cmpc_handle h, const cmpc_model* dModels, int* dOk, void* stream);

/* ---- NLP callbacks (what IPOPT evaluated through the generated code), batched on the device ----
 * any output pointer may be NULL.  dLamG[B][n_g], lam_f scalar (hess of lam_f f + lam_g^T g).
 * dJac[B][nnz_jac] / dHess[B][nnz_hess] are in the reference's CCS nonzero order
 * (cmpc_nlp_sparsity gives row/col per nonzero; tmp.c:66-67 for N=12). */
int cmpc_eval_nlp_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG,
                         float lam_f, float* dF, float* dG, float* dGradF, float* dJac,
                         float* dHess, void* stream);
int cmpc_nlp_sparsity(int horizon, int* jac_row, int* jac_col, int* hess_row, int* hess_col);
/* nlp_grad (tmp.c:24791): gradient of gamma = lam_f f + lam_g^T g with respect to x (dGradX[B][n_x]) and to the
 * parameters (dGradP[B][n_p]; zero for limA/limB, currentPos, com0/dcom0/h0, which only enter the bounds).  Either
 * output may be NULL. */
int cmpc_eval_nlp_grad_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, float lam_f,
                              float* dGradX, float* dGradP, void* stream);

/* ---- multipliers of the reference NLP (what CasADi's Opti -> IPOPT hands back as lam_g), its KKT certificate and the gradient of the optimal cost ----
 * cmpc_set_multiplier_output(h, 1): every later solve on the handle -- cmpc_solve, cmpc_solve_device[_warm], cmpc_advance, the solve inside
 * cmpc_rollout_tick_device -- also writes the handle's dual record of each problem (costates, slacks and multipliers of the solver's stage form,
 * [B][15 (N+1) + 88 N] floats, allocated on first use; ~8 KB per problem at N = 20), taken at the x the solve returns.  0 frees it.  Off (the default),
 * no record exists and x / info are those of a handle that never turned it on.  The record is read only by the calls below, never by a solve.
 *
 * cmpc_get_multipliers_device: dLamG[B][n_g] of the LAST solve on the handle, whose dX / dP the caller passes again (the initial-condition rows are
 * recovered from x and p).  n_g = 53N + 15, rows in the order of the reference's g (cmpc_nlp_sparsity): init[15] com[3N] dcom[3N] h[3N] pos_c[3N]
 * (c = 0, 1) then per contact bbox_c[3N] fric_c[16N].  Sign convention of IPOPT and of the goldens: L = f + lam_g^T g, lam >= 0 at an active upper
 * bound, <= 0 at an active lower bound.  Row by row (derivation: DESIGN.md, "Multipliers"):
 *   com / dcom / h rows of stage k (x_{k+1} - phi_k(x_k, u_k)): minus the solver's costate of stage k+1, formed at the returned x;
 *   pos_c rows of stage k: minus the foot's costate of stage k+1 in stance; exactly 0 in swing (vel is free and costs nothing: dL/dvel = 0);
 *   bbox_c rows of stage k: in swing, zU - zL of the offset's upper and lower rows; a component with lower == upper (the solver eliminates it)
 *     -(R_k^T lam_pos)_i from stationarity in the landing position; in stance exactly 0 -- the row duplicates the landing row (subset rule 3) and the
 *     multiplier, not unique there, is put entirely on the landing row;
 *   fric_c rows (upper bound 0): the solver's friction multipliers z;
 *   init rows (Jacobian = identity on com_0 dcom_0 h_0 pos_0): lam_init = -grad_x (f + lam'^T g) on those columns, lam' = lam_g without them (nlp_grad).
 * A problem with status 3 gets zeros; status 1 or 2 the values of the last iterate.  CMPC_ERR_ARG when the output is off.
 * cmpc_get_multipliers: the same for the handle's own problem set after cmpc_advance, into host memory (synchronous). */
int cmpc_set_multiplier_output(cmpc_handle h, int enabled);
int cmpc_get_multipliers_device(cmpc_handle h, const float* dX, const float* dP, float* dLamG, void* stream);
int cmpc_get_multipliers(cmpc_handle h, float* LamG);
/* KKT certificate of the reference NLP at (x, lam_g), per problem, in double on the device (f, g and grad_x L from the restatement of the generated
 * code above; bounds built from p: init rows = com0 dcom0 h0 currentPos, dynamics rows 0, box rows [lower, upper], friction rows (-inf, 0]).
 * dCert[B][CMPC_CERT] = { stationarity  max|grad f + J^T lam| / scale,  scale = max(1, max|lam|),
 *                         primal infeasibility  max(lbg - g, g - ubg, 0),
 *                         complementarity  max |lam_i dist(g_i, nearer bound)| / scale over inequality rows (ubg - lbg > 1e-12),
 *                         sign violation  max wrong-sign |lam_i| / scale (lam >= 0 on rows bounded above only, <= 0 below only, the sign of the nearer
 *                           bound on two-sided rows),
 *                         f,  status of the handle's last solve (-1 when the multiplier output is off),  scale,  max|grad f + J^T lam| }.
 * Per-problem models (cmpc_set_models*) apply. */
#define CMPC_CERT 8
int cmpc_kkt_certificate_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, float* dCert, void* stream);
/* Gradient of the optimal cost with respect to every parameter (envelope theorem) at a KKT point (x*, lam*): dGradP[B][n_p] = grad_p L(x, lam)
 * (nlp_grad, lam_f = 1) plus the parameters that only enter the bounds: -lam_init on com0, dcom0, h0 and currentPos; -max(lam, 0) on upper and
 * -min(lam, 0) on lower of each box row.  The entries of enabled (Gamma, binary) and R (constrained to rotations) are formal derivatives of the
 * generated code, not derivatives along feasible perturbations; the derivative along rotations is cmpc_rotation_value_gradient_device (below,
 * "rotation directions").  The derivatives with respect to the per-problem model fields are cmpc_model_value_gradient_device (below, "model
 * directions"). */
int cmpc_value_gradient_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, float* dGradP, void* stream);

/* ---- solution sensitivities: dx* / dp as JVP and VJP (derivation: DESIGN.md 7c) ----
 * The derivative of the library's own solution map p -> x*(p) at a returned point, in the barrier form (as sIPOPT): inputs per problem are x, p and
 * lam_g exactly as exported (cmpc_get_multipliers_device: layout, sign convention, duplicate rows credited to the landing row).
 *   Equality rows E: the 15 initial rows, the com / dcom / h dynamics, the foot-position dynamics, swing-stage box components with lower == upper.
 *   Inequality rows I: friction rows (z = max(lam, 0)); swing-stage box components with lower < upper, both sides (zU = max(lam, 0), zL = max(-lam, 0)).
 *     Each side enters with Sigma_i = z_i / s_i, s_i = the distance of g_i(x) to that bound floored at CMPC_SENS_SMIN (at the returned x an active
 *     row's slack is rounding noise and can be <= 0).
 *   Not in the map: stance-stage box rows and stance vel columns (the stage form): their entries of dx are 0.
 * With L = f + lam_g^T g and W = grad_xx L + sum_{i in I} J_i^T Sigma_i J_i (exact Hessian, with the bilinear momentum term):
 *     [ W    J_E^T ] [ dx    ]      [ d_p(grad_x L) dp + sum_{i in I} J_i^T Sigma_i (d_p g_i dp - db_i) ]
 *     [ J_E  0     ] [ dlam_E] = -  [ d_p g_E dp - db_E                                                ]
 * b are the bounds as functions of p: com0, dcom0, h0, currentPos (initial rows), box lower / upper; an equality box component's bound is
 * (lower + upper) / 2 (a perturbation that stays in the subset moves both).  JVP: dx.  VJP: the same symmetric system with right-hand side [v; 0],
 * v = dl/dx, and dl/dp = -w^T r_p.
 * Parameters covered: com0, dcom0, h0, currentPos, comRef, hRef, nominalPos, box upper / lower, fExt, tauExt.  Not covered: Gamma (enabled, discrete):
 * the JVP reads those entries of dp, and the entries of R, as zero, the VJP writes zeros there.  R is covered in its tangent space by the *_rot_device
 * entry points below ("rotation directions"), the fields of the per-problem model by the *_model_device entry points ("model directions").
 * Tied entries (subset rule 3): a stance stage after a landing repeats the last swing stage's R, nominal, lower and upper.  Under this map a stance
 * stage's lower / upper have zero derivative and a stance knot's nominalPos acts through the cost only; a perturbation that stays in the subset moves
 * the whole group, and its derivative is the sum over the group.
 * Internal-force direction: when both feet are in stance over the whole horizon, a constant internal force along currentPos_0 - currentPos_1 (left
 * corners +e, right corners -e, every knot) is not determined by the NLP.  The JVP's dx has no component along it; the VJP
 * treats v's component along it as zero.
 * Weakly active rows (slack and multiplier both below CMPC_SENS_WEAK: an unloaded corner at the apex of its pyramid): the true
 * map has a kink there and the barrier derivative is one value between its one-sided slopes.  They are counted, not hidden (dSens[2]).
 * Linear algebra: the stage Riccati recursion of the solver's form in float64, one factorisation per problem shared by every right-hand side, the
 * control Hessian shifted by CMPC_SENS_SHIFT on the force diagonal, two steps of float64 iterative refinement against the unshifted operator.
 * dSens[B][CMPC_SENS] = { status: 0 ok, 1 a non-positive pivot of the reduced Hessian (no Gauss-Newton fallback: it would change the derivative),
 *                           2 non-finite input or result, 3 outside the supported subset (the rule of solver status 3, or a model that broke the
 *                           model rule);
 *                         relative residual max|K s - rhs| / max|rhs| of the returned solution against the unshifted system (largest over the k columns);
 *                         number of weakly active rows of loaded feet (friction rows of stance stages) and of box sides;  largest Sigma;
 *                         1 if the internal-force direction exists (and was projected out);
 *                         number of weakly active friction rows of swing stages (counted apart: a swing foot's forces enter no dynamics, and they
 *                           sit near the apex because the costs pull them towards zero from inside the pyramid, not because a face binds);
 *                         the removed relative component of model and rotation directions along the internal-force direction (0 here; "model
 *                           directions", "rotation directions");  0 }.
 * A flagged problem gets zero outputs; its neighbours are unaffected.  Per-problem models (cmpc_set_models*) apply; every horizon the handle supports.
 * Workspace: per-handle HBM, allocated on first use and freed by cmpc_destroy, for min(B, CMPC_SENS_SUB_BATCH) problems (larger batches run in
 * sub-batches): cmpc_sensitivity_workspace_bytes(N) per problem -- 8 (39^2 (N+1) + 2070 N + 8 (216 N + 117)) bytes, 0.85 MB at N = 20.
 * Results depend on nothing but the problem's own inputs: not on its batch position, the batch size, the sub-batching or k (columns are processed
 * in chunks of 8, bit for bit the same as one at a time).  The workspace is the handle's: a call on another stream than the previous call's waits
 * for it (an event), so calls on one handle run one after the other whatever their streams.
 * Slack floor: an active row's Sigma is capped at z / CMPC_SENS_SMIN, which biases the derivative along that row by about curvature x s_min / z
 * relative (1e-4 for a landing-offset row with z ~ 0.1; 1e-6 for a loaded friction row). */
#define CMPC_SENS 8
#define CMPC_SENS_SMIN 5e-8
#define CMPC_SENS_WEAK 1e-3
#define CMPC_SENS_SHIFT 1e-7
#define CMPC_SENS_SUB_BATCH 1024
/* JVP: dDirP[B][k][n_p] directions (k >= 1) -> dDX[B][k][n_x]; dSens[B][CMPC_SENS] or NULL */
int cmpc_solution_jvp_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dDirP, int k, float* dDX, float* dSens,
                             void* stream);
/* VJP: dGradX[B][n_x] = dl/dx -> dGradP[B][n_p] = dl/dp */
int cmpc_solution_vjp_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, float* dGradP, float* dSens,
                             void* stream);
size_t cmpc_sensitivity_workspace_bytes(int horizon);

/* ---- model directions: derivatives with respect to the per-problem model (derivation: DESIGN.md 7c) ----
 * theta = the 34 doubles of cmpc_model in its field order (0 friction, 1..3 com_weight, 4 angular_momentum_weight, 5 contact_position_weight,
 * 6..8 force_rate_of_change_weight, 9 contact_force_symmetry_weight, 10 + 12 c + 3 j + b corner j of contact c, axis b).  No bound depends on theta.
 * At fixed (x, lam) theta enters L = f + lam_g^T g as follows:
 *   weights: linearly through f, except com_weight[2], which enters quadratically: the term is (w_z(k) (com_z - ref_z))^2 with
 *     w_z(k) = (w_cz / 2)(1 + e^-k) (the solver's record wz2 = 2 w_z^2);  the symmetry and force-rate weights act on the corner forces, the rate
 *     cost couples knots k and k+1 only;
 *   friction: linearly through the friction rows, as -mu (R^T f)_z;
 *   corners: linearly through the angular-momentum dynamics, (R cn + pos - com) x f, and so also through grad_x(lam^T g) on the force columns.
 * In the barrier system of the solution sensitivities above, a model direction dtheta has the right-hand side
 *     r_x = d_theta(grad_x L) dtheta + sum_{i in I} J_i^T Sigma_i d_theta g_i dtheta,     r_E = d_theta g_E dtheta
 * (Sigma, the rows E / I, the slack floor, the shift, the refinement and dSens exactly as there).  JVP: dx = the first block of K^-1 (-r(dp, dtheta)),
 * so p and theta directions combine in one column.  VJP: dl/dtheta = -w^T r_theta with the same w as cmpc_solution_vjp_device.  Value gradient:
 * dV* / dtheta = d_theta f + lam^T d_theta g at (x, lam) (envelope theorem).
 * The derivative is taken at the model the solve used: the float32 record that cmpc_create or cmpc_set_models* derived (d wz2 / d w_cz =
 * sqrt(2 wz2(k)) (1 + e^-k)).  Without a model table theta is the config's model for every problem.  A row whose model broke the model rule gets
 * status 3 and zero outputs.
 * Internal force (both feet in stance over the whole horizon): K has a null vector whose primal part is n (left corners +e, right corners -e) and
 * whose dual part sits on the foot-position rows, which no model field enters; a model right-hand side is consistent only if n^T r_x = 0.  The weights
 * satisfy it up to rounding (the symmetry cost is blind to a force constant over a foot's corners, the rate terms telescope); friction leaves a
 * component through Sigma (small, up to order one where the friction rows carry the load); a corner direction that moves the two feet's rotated
 * corner sums differently gives the internal force a moment arm, and its component is sum_k lam_h,k . (R e_b x e): zero up to the solve's tolerance
 * while the couples about x and z are free (no loaded friction row), large otherwise.  Along a direction with a component the true map has no
 * derivative.  Rule: the JVP removes r_x's component along n before the solve; the VJP removes the same component from every r_t (it contracts with
 * -w^T r_t + (n^T w)(n^T r_t): w can carry a component along n, since v is projected in float32 and the shifted system amplifies what is left), so the
 * two stay adjoint.  The removed relative size |n^T r_x| / |r_x| (r_x in the NLP's x layout, of the model part of the column) is reported in dSens[6]:
 * the largest over the k columns (JVP) or over the 34 fields (VJP); 0 without model directions or without n.  For the same reason the friction and
 * corner entries of dV* / dtheta at such a point depend on the internal force the solve happened to return: not exact derivatives where that
 * direction's dSens[6] is not small.
 * No workspace beyond cmpc_sensitivity_workspace_bytes; sub-batches, the event ordering and the bit-for-bit independence of batch position, batch
 * size, k and sub-batching as for the solution sensitivities.
 * JVP: dDirP[B][k][n_p] float (NULL: zero), dDirModel[B][k][34] double (NULL: zero) -> dDX[B][k][n_x].  With dDirModel == NULL the result is
 * cmpc_solution_jvp_device's, bit for bit. */
int cmpc_solution_jvp_model_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dDirP, const double* dDirModel, int k,
                                   float* dDX, float* dSens, void* stream);
/* VJP: dGradX[B][n_x] -> dGradP[B][n_p] (NULL: not written; otherwise cmpc_solution_vjp_device's output bit for bit) and dGradModel[B][34] double,
 * from one adjoint solve */
int cmpc_solution_vjp_model_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, float* dGradP,
                                   double* dGradModel, float* dSens, void* stream);
/* dV* / dtheta [B][34] double at (x, lam_g); zeros for a row whose model broke the model rule */
int cmpc_model_value_gradient_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, double* dGradModel, void* stream);

/* ---- rotation directions: derivatives with respect to the stage rotations R (derivation: DESIGN.md 7c) ----
 * omega[c][k] in R^3, one per contact c in {0, 1} and stage k = 0..N-1, moves that stage's rotation along dR_{c,k} = R_{c,k} [omega_{c,k}]x: the right
 * (body-frame) tangent, manif's rplus, which the reference's poses use; for a flat foot, yaw is omega = e_z in either frame.  R_{c,k} is the float32
 * matrix as stored in p (column-major 3x3 at p_R(c) + 9 k), not re-orthonormalised.  Every term of the NLP is linear in the entries of R --
 * (R corner + pos - com) x f, R^T (pos - nominalPos), A R^T f -- so the formal derivative of the NLP along dR is exact, and no bound depends on R.
 * In the barrier system of the solution sensitivities a rotation direction has the right-hand side
 *     r_x = d_omega(grad_x L) omega + sum_{i in I} J_i^T Sigma_i d_omega g_i omega,     r_E = d_omega g_E omega
 * (Sigma, the rows E / I, the slack floor, the shift, the refinement and dSens exactly as there).  JVP: dx = the first block of
 * K^-1 (-r(dp, dtheta, omega)), so p, model and rotation directions combine in one column.  VJP: dl/domega_{c,k} = -w^T r_{omega_{c,k}} with the same w
 * as cmpc_solution_vjp_device.  Value gradient: dV* / domega = lam^T d_omega g at (x, lam_g) (envelope theorem; f does not depend on R).
 * Where R enters: the angular-momentum rows of stage k through the lever arms (R [omega]x corner in place of the corner fields' R e_b); the friction
 * rows of stage k, a_i^T R^T f, with d_omega g_i = a_i^T ([R^T f]x omega), through lam and through Sigma -- swing feet's rows too; the box rows of
 * swing stages, R_k^T (pos_{k+1} - nominalPos_{k+1}) (index k of R pairs with knot k+1).  The stage form lands a swing foot at nominalPos + R^-T q, so
 * its change of variables moves with R, d(R^-T) = R^-T [omega]x: the position dynamics get R^-T (omega x q) at the returned q = R^T (pos - nominalPos),
 * free and fixed components alike, and the free offsets get omega x lam_box; dx comes out in the NLP's x layout as before.
 * Tied entries (subset rule 3): a stance stage after a landing repeats the last swing stage's R.  The entries here are per stage; a perturbation that
 * stays in the subset moves the whole group, and its derivative is the sum over the group (cmpc_contacts_rotation_vjp_device does that sum per list
 * entry).
 * Internal force (both feet in stance over the whole horizon): the rule of the model directions, unchanged -- rotating one foot gives the internal
 * force a moment arm.  The JVP removes n (n^T r_x) from the rotation part of the column before the solve, the VJP removes the same component from
 * every r_omega, and the removed relative size joins dSens[6] (the largest over the columns or the 6 N entries, combined with the model part's by
 * max).  Without loaded friction rows it is at the solve's tolerance (<= 3e-7 on the config 2 goldens; up to 0.2 on synthetic config 2 problems whose friction rows carry load) and the derivative exists; with them (a push in
 * double support: 0.11 .. 0.16 for a whole foot, 0.19 for the worst single entry) there is none, as for friction there.
 * Swing feet: a rotation acts directly on the friction rows of swing feet, which sit at the apex of their pyramids (weakly active, counted in
 * dSens[5]); for a group of stages that contains swing stages the barrier derivative and the true one differ by a small absolute amount (4e-6 ..
 * 1.6e-5 in dx per radian on the goldens, 5e-4 of the effect where the effect is not itself that small) -- the effect the model directions state for
 * the symmetry and force-rate weights.
 * No workspace beyond cmpc_sensitivity_workspace_bytes; argument checks, sub-batches, the event ordering, per-problem models and the bit-for-bit
 * independence of batch position, batch size, k and sub-batching as for the model directions.  A flagged problem (a non-finite omega: status 2) gets
 * zeros, its neighbours keep their bits.
 * JVP: dDirP[B][k][n_p] float, dDirModel[B][k][34] double, dDirRot[B][k][2][N][3] double (each NULL: zero) -> dDX[B][k][n_x].  With dDirRot == NULL the
 * result is cmpc_solution_jvp_model_device's, bit for bit. */
int cmpc_solution_jvp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dDirP, const double* dDirModel,
                                 const double* dDirRot, int k, float* dDX, float* dSens, void* stream);
/* VJP: dGradX[B][n_x] -> dGradRot[B][2][N][3] double, dGradP[B][n_p] float and dGradModel[B][34] double from ONE adjoint solve (each may be NULL, not
 * all three); dGradP and dGradModel are cmpc_solution_vjp_model_device's, bit for bit */
int cmpc_solution_vjp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, float* dGradP,
                                 double* dGradModel, double* dGradRot, float* dSens, void* stream);
/* Cotangent columns: the VJP of k cotangents from ONE factorisation per problem.  dGradX[B][k][n_x] (k >= 1) -> dGradP[B][k][n_p] float,
 * dGradModel[B][k][34] double, dGradRot[B][k][2][N][3] double (each may be NULL, not all three).  The adjoint solves run in chunks of 8 columns behind
 * the one Riccati factorisation, as the JVP's columns do.  Column j is cmpc_solution_vjp_rot_device on cotangent j bit for bit -- and therefore
 * cmpc_solution_vjp_device and cmpc_solution_vjp_model_device on their outputs -- whatever k and the column's place in it: every cotangent loses its own
 * component along the internal-force direction with the single call's float32 rounding, and every reduction keeps the single call's order.
 * dSens[B][CMPC_SENS] stays one row per problem: the status, the weak-row counts, the largest Sigma and the internal-force word are the problem's;
 * word 1 is the largest relative residual over the k columns, each measured as its single call measures it; word 6 is the largest removed component
 * over columns and fields.  A non-finite entry in any cotangent column flags the whole problem (status 2); a flagged problem gets zeros in every column
 * of every output, its neighbours keep their bits.  Derivatives are those of the barrier form above, weakly active rows included.
 * CMPC_ERR_ARG, before anything is queued: a NULL handle or input, k < 1, all three outputs NULL.  No workspace beyond
 * cmpc_sensitivity_workspace_bytes (its eight column slots); sub-batches, the event ordering, per-problem models and the bit-for-bit independence of batch
 * position, batch size, k and sub-batching as for the entries above. */
int cmpc_solution_vjp_cols_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, int k, float* dGradP,
                                  double* dGradModel, double* dGradRot, float* dSens, void* stream);
/* dV* / domega [B][2][N][3] double at (x, lam_g); zeros for a row whose model broke the model rule.  At a double-support point the entries depend
 * on the internal force the solve returned, as the corner entries of dV* / dtheta do. */
int cmpc_rotation_value_gradient_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, double* dGradRot, void* stream);
/* Per stage -> per list entry: dGradListRot[B][2][max_contacts][3] double = for each entry m of the sampled lists (dT[B][2][max_contacts][2],
 * dN[B][2], sampled at `now`), the sum over the stages k it owns of dGradRot[c][k] (cmpc_contacts_sample's owner rule: the active contact, else the
 * next, else the last), in the body-frame tangent of the entry's quaternion, q <- q (x) exp(omega / 2): a sampled stage copies its owner's rotation, so
 * omega_stage = omega_owner.  float64 sums in stage order, one thread per (problem, foot), no atomics.  Entries at or beyond n carry none; a foot
 * that the sampling would not sample (an empty list, or n > max_contacts) gets zeros. */
int cmpc_contacts_rotation_vjp_device(cmpc_handle h, int max_contacts, double now, const double* dT, const int* dN, const double* dGradRot,
                                      double* dGradListRot, void* stream);

/* ---- class-shaped setters (host buffers -> the handle's own device P, X0) ----
 * batch-major float32; NULL keeps the previous value (zeros initially).
 *   state    [B][9]            com0, dcom0, h0 (h and wrench already mass-normalised,
 *                              CentroidalMPCBlock.cpp:403-410)
 *   wrench   [B][N][6]         external force (3) and torque (3) per knot, or NULL = 0
 *   com_ref, h_ref [B][N+1][3]
 *   R [B][2][N][9] row-major 3x3, upper/lower [B][2][N][3], enabled [B][2][N],
 *   nominal [B][2][N+1][3], current [B][2][3] */
int cmpc_set_state(cmpc_handle h, const float* state, const float* wrench);
int cmpc_set_reference(cmpc_handle h, const float* com_ref, const float* h_ref);
int cmpc_set_contacts(cmpc_handle h, const float* R, const float* upper, const float* lower,
                      const float* enabled, const float* nominal, const float* current);
/* x0: [B][n_x] or NULL = cold start (CoM at com0, feet at nominal, f_z = g/8 per corner);
 * shift_previous != 0: warm start from the previous solution shifted by one knot
 * (is_warm_start_enabled, ergoCubGazeboV1/centroidal_mpc.ini:9) */
int cmpc_set_initial_guess(cmpc_handle h, const float* x0, int shift_previous);
/* solve the handle's own problem set (set_* above); synchronous */
int cmpc_advance(cmpc_handle h);
int cmpc_get_solution(cmpc_handle h, float* X, float* info);
/* read-back of what the setters above have written: the handle's parameter set P[B][n_p] exactly as the next cmpc_advance will solve it
 * (the reference's setState / setReferenceTrajectory / setContactPhaseList fill CasADi's parameter vector p the same way, CentroidalMPCBlock.cpp:407, :579,
 * :609) -- host copy, or the handle's device buffer after uploading the staged values (valid until the next setter call / cmpc_advance). */
int cmpc_get_parameters(cmpc_handle h, float* P);
int cmpc_get_parameters_device(cmpc_handle h, const float** dP);
/* compact output of getOutput(): per problem first-knot corner forces [2][4][3], contact
 * positions at knot 0 [2][3], next (adjusted) landing position per contact [2][3] and its knot
 * index [2] (-1 if the contact does not land inside the horizon) */
int cmpc_get_output(cmpc_handle h, float* forces0, float* pos0, float* next_pos, int* next_knot);

/* ---- rows next to the solve ----
 * 8f-3, CentroidalMPCBlock.cpp:525-577: planner trajectories (n_in knots every in_dt seconds, the first one t_offset
 * seconds before "now"; com_in/h_in [B][n_in][3], h_in NOT yet divided by the mass) -> comRef/hRef at the N+1 MPC knots
 * by linear interpolation; the CoM height is replaced by com_height unless it is NaN (the reference forces 0.7, :534). */
int cmpc_set_reference_from_planner(cmpc_handle h, const float* com_in, const float* h_in, int n_in, double in_dt,
                                    double t_offset, double robot_mass, double com_height);
/* the same on the device (one thread per problem and knot), into the reference rows of the caller's dP[B][n_p]; dComIn / dHIn [B][n_in][3] device pointers;
 * asynchronous on `stream` (NULL: the handle's) */
int cmpc_write_reference_from_planner_device(cmpc_handle h, const float* dComIn, const float* dHIn, int n_in, double in_dt, double t_offset,
                                             double robot_mass, double com_height, float* dP, void* stream);
/* 8f-3 differentiated in the planner's trajectories, over the rows of a walk ("References").  The map: the handle's sampling time is dt; tick
 * number i runs at now = i * dt and reads the trajectories c, h [knots][3] (float32, a knot every pl->dt seconds, knot 0 at time pl->t_first) at
 * t_off = now - t_first, as cmpc_rollout_walk_device does (plan_t_first).  For MPC knot k = 0 .. N
 *     s = clamp((t_off + k dt) / pl->dt, 0, knots - 1),  i0 = min((int)s, knots - 2),  w = s - i0
 *     comRef_k[a] = (float)((1 - w) c[i0][a] + w c[i0+1][a])                  a = 0, 1; a = 2 only if com_height is NaN
 *     hRef_k[a]   = (float)(((1 - w) h[i0][a] + w h[i0+1][a]) / robot_mass)
 * Times, robot_mass and com_height are not differentiated.  The weights are those of the clamped forward: a knot beyond an end puts its whole weight on the
 * end knot.  With com_height a number the z row of comRef is a constant: its entries of the gradient are not read, its direction is 0.0f.  (i0, w) come
 * from ONE __host__ __device__ function (cmpc_reference_weight, csrc/cmpc_contacts.h) that repeats cmpc_resample_reference_knot's arithmetic with
 * contraction into fma off; that function itself is untouched.  All four entry points compile with contraction off; the host forms need no handle and no
 * GPU and are bit-equal to the kernels.  A single tick at an arbitrary offset is rows = 1, tick0 = 0, t_first = -t_offset.  The array pointers point at
 * the first row used. */
typedef struct cmpc_planner_refs {
    int knots;             /* knots of each trajectory, >= 2 */
    double dt;             /* seconds between two knots (cmpc_write_reference_from_planner_device's in_dt) */
    double t_first;        /* time of knot 0 */
    double robot_mass;
    double com_height;     /* NaN: the trajectory's own z row is used, and differentiated */
} cmpc_planner_refs;
/* Reverse: grad_p[rows][B][n_p] float, row r the dl/dp of tick tick0 + r (cmpc_walk_grads.dGradP) -> grad_com / grad_h [B][knots][3] double, ADDED TO
 * (either may be NULL when only the other is wanted, not both).  Problem b with e = end_tick[b] (NULL or -1: never ended) contributes the rows with
 * tick0 + r < e -- its solutions 0 .. e - 1, the rule of cmpc_rollout_walk_vjp_device.  Rows at or past e are NOT READ: a select, so NaN there cannot leak.
 * Each output entry is owned by one thread (no atomics): it loads the entry's current value, then adds its terms in ascending (row, knot) order,
 * (1 - w) * (double)g for i0 == j, w * (double)g for i0 + 1 == j, for h the same divided by robot_mass.  Because of that order ascending segments compose
 * to the bit with one call over all rows.  The device form is ONE launch whatever the number of rows (one workgroup per problem and 128 planner knots,
 * the rows' terms staged through LDS eight rows at a time; every barrier is uniform over the workgroup, an ended problem only shortens the loop), asynchronous on
 * `stream` (NULL: the handle's), no workspace, no host wait; lanes past `knots` touch no memory.
 * CMPC_ERR_ARG: a NULL handle, pl or grad_p, both outputs NULL, knots < 2, dt or robot_mass not > 0 or not finite, t_first not finite, rows < 1,
 * tick0 < 0; the host form also for a horizon outside 1 .. 40, a sampling time not > 0 or a batch < 1. */
int cmpc_reference_from_planner_vjp(int horizon, double sampling_time, int batch, int tick0, int rows, const cmpc_planner_refs* pl, const int* end_tick,
                                    const float* grad_p, double* grad_com, double* grad_h);
int cmpc_reference_from_planner_vjp_device(cmpc_handle h, int tick0, int rows, const cmpc_planner_refs* pl, const int* dEndTick, const float* dGradP,
                                           double* dGradCom, double* dGradH, void* stream);
/* Forwards: dir_com / dir_h [B][k][knots][3] double (either may be NULL: zero, not both) -> the 6 (N + 1) reference entries (comRef, hRef) of every column
 * of dir_p[rows][B][k][n_p] float, the layout of cmpc_walk_dirs.dDirP.  Entry = the forward's expression applied to the direction in double, then cast to
 * float; z of comRef is 0.0f when com_height is a number.  It WRITES those entries and leaves every other entry of dir_p alone.  No ending logic: the
 * forward walk's gate discards what an ended problem is given.  One thread per written entry; asynchronous on `stream` (NULL: the handle's), no workspace.
 * CMPC_ERR_ARG as above, and k < 1. */
int cmpc_reference_from_planner_jvp(int horizon, double sampling_time, int batch, int tick0, int rows, int k, const cmpc_planner_refs* pl,
                                    const double* dir_com, const double* dir_h, float* dir_p);
int cmpc_reference_from_planner_jvp_device(cmpc_handle h, int tick0, int rows, int k, const cmpc_planner_refs* pl, const double* dDirCom, const double* dDirH,
                                           float* dDirP, void* stream);
/* 8f-4, WholeBodyQPBlock.cpp:805-873, 1083-1084, 1150, 1259-1262: between two MPC ticks the plant integrates the
 * centroidal dynamics under the first-knot corner forces of the active contacts + the external wrench of knot 0 (RK4,
 * `substeps` steps of `step` seconds, forces held) and reports the desired ZMP (local ZMP clamped to +-zmp_half_x/y:
 * 0.08 / 0.03 in the reference).  dStateIn/dStateOut [B][9] (com, dcom, h; may alias), dZmp [B][2] or NULL. Device
 * pointers; asynchronous on `stream` (NULL: the handle's). */
int cmpc_plant_step_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, float* dStateOut,
                           float* dZmp, double step, int substeps, double zmp_half_x, double zmp_half_y, void* stream);

/* ---- plant-step derivatives (derivation: DESIGN.md 7d) ----
 * The map of cmpc_plant_step_device, (state, x, p, theta) -> state', differentiated at the float32 inputs in float64.  With the forces held the dynamics are
 * affine and nilpotent, so the RK4 sweep equals the closed form over T = substeps * step (step rounded to float32, as the forward does):
 *     com' = com + T dcom + T^2/2 a,  dcom' = dcom + T a,  h' = h + T tau0 - I x F,   I = T com + T^2/2 dcom + T^3/6 a,
 *     a = F + fExt_0 - g e_z,  F = sum_q f_q,  tau0 = tauExt_0 + sum_q (pos_c,0 + R_c,0 corner_q) x f_q.
 * Differentiated inputs: state [9]; from x the knot-0 foot positions pos_c,0 (6) and the knot-0 corner forces f_c,j,0 (24), gated by Gamma_c,0 exactly as
 * the forward gates them (a foot with Gamma_c,0 <= 0.5 has zero force derivatives; its position derivative is then zero too, since no force acts there);
 * from p the wrench of knot 0, fExt_0 and tauExt_0; from the model the 24 corner entries (theta indices 10..33), through R_c,0 corner.
 * NOT differentiated by the first pair: R and Gamma (as for the solution sensitivities), step, substeps, gravity, and the ZMP output (clipped; an output
 * only).  The *_rot_* pair below adds R_c,0.
 * JVP and VJP apply one set of partials (T, F, I, the contact points and the gated forces), forwards and transposed term by term: adjoint by construction.
 * One thread per problem; per-problem models (cmpc_set_models*) apply (a row that broke the model rule uses the config's corners, as the forward does);
 * results depend on nothing but the problem's own inputs.  No status word: non-finite inputs give non-finite outputs.  Device pointers; asynchronous on
 * `stream` (NULL: the handle's).
 * JVP: dDirState[B][9] double, dDirX[B][n_x] float or NULL (zero; only the 30 entries above are read), dDirP[B][n_p] float or NULL (only fExt_0, tauExt_0),
 * dDirModel[B][34] double or NULL (only the corners) -> dDirStateOut[B][9] double (may alias dDirState). */
int cmpc_plant_step_jvp_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, const double* dDirState,
                               const float* dDirX, const float* dDirP, const double* dDirModel, double* dDirStateOut, void* stream);
/* VJP: dGradStateOut[B][9] double -> dGradState[B][9] double (may alias dGradStateOut), dGradX[B][n_x] float (written whole: zero but for the 30 entries),
 * dGradP[B][n_p] float or NULL (written whole: zero but for fExt_0, tauExt_0), dGradModel[B][34] double or NULL (written whole: entries 0..9 zero). */
int cmpc_plant_step_vjp_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, const double* dGradStateOut,
                               double* dGradState, float* dGradX, float* dGradP, double* dGradModel, void* stream);
/* The same pair with the knot-0 rotations R_c,0 differentiated, in the tangent of the rotation directions above: omega_c in R^3 per foot moves
 * dR_c,0 = R_c,0 [omega_c]x, R_c,0 the float32 matrix stored in p, not re-orthonormalised.  Only h' depends on R, through the lever arms
 * pos_c,0 + R_c,0 corner_q:  d h' = T sum_q (R_c,0 (omega_c x corner_q)) x f_q,  so  d h' / d omega_c = T sum_q [f_q]x R_c,0 [corner_q]x  with the forces gated
 * by Gamma_c,0 as everywhere above (a gated-off foot has zero dGradRot0) and the float32 corners of the problem's model.  The term joins the one set of
 * partials; JVP and VJP apply it forwards and transposed like the others.  dDirRot0[B][2][3] double (NULL: zero), dGradRot0[B][2][3] double (may be NULL);
 * with the pointer NULL the results are the first pair's bit for bit (the first pair calls these with NULL). */
int cmpc_plant_step_jvp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, const double* dDirState,
                                   const float* dDirX, const float* dDirP, const double* dDirModel, const double* dDirRot0, double* dDirStateOut, void* stream);
int cmpc_plant_step_vjp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps,
                                   const double* dGradStateOut, double* dGradState, float* dGradX, float* dGradP, double* dGradModel, double* dGradRot0,
                                   void* stream);

/* 8e, the record a Monte-Carlo driver gathers across GPUs (no reference counterpart: the reference runs one problem):
 * dOut[B][3(N+1) + 38] = CoM trajectory 3(N+1) | first-knot corner forces 24 | knot-0 and knot-1 foot positions 12 |
 * iterations | status, from dX[B][n_x] and dInfo[B][8].  Device pointers; asynchronous on `stream` (NULL: the handle's). */
int cmpc_compact_output_device(cmpc_handle h, const float* dX, const float* dInfo, float* dOut, void* stream);
/* ... and the gather itself: ncclAllGather (RCCL, over xGMI) of every rank's B compact records, dLocal[B][3(N+1) + 38] -> dAll[world_size][B][...], on
 * `stream` (NULL: the handle's).  nccl_comm is the caller's ncclComm_t (one rank per GPU and process, ncclCommInitRank; every rank's handle must have the
 * same batch -- pad ragged shards).  librccl.so is opened on first use.  The Python harness does the same with torch.distributed (distributed.py); this entry
 * point is what a C++ Monte-Carlo driver shaped after the reference's Main.cpp:98-134 calls (examples/montecarlo_allgather.cpp). */
int cmpc_allgather_compact_device(cmpc_handle h, void* nccl_comm, int world_size, const float* dLocal, float* dAll, void* stream);

/* ---- 8f-1: contact schedules, batched ----
 * What the reference does with BipedalLocomotion::Contacts::ContactPhaseList objects around the solve, for a batch.
 * One foot of one problem = a list of at most M = max_contacts contacts sorted by activation time (contacts in
 * alphabetical name order: left_foot, right_foot):
 *     t[B][2][M][2]     activation, deactivation time [s] (double)
 *     pose[B][2][M][7]  position x y z, orientation quaternion w x y z (float)
 *     n[B][2]           contacts in use
 * ContactList::getActiveContact(t) = the contact with activation <= t < deactivation; getNextContact(t) = the first
 * one that activates after t (the two queries the reference makes, CentroidalMPCBlock.cpp:44, :61, :69). */

/* ContactPhaseList::forceSampleTime(m_dT), CentroidalMPCBlock.cpp:586-592: the reference snaps the planner's lists to the MPC grid on every
 * tick before the merge; the merge and the sampling below assume times on the grid.  The rule is BipedalLocomotionFramework's, whose source is not
 * in the reference tree: PARITY UNPINNED.  Ours, on integer nanoseconds as the reference's clock (std::chrono::nanoseconds):
 *   t_ns = llround(t 1e9), dt_ns = llround(dt 1e9);
 *   every activation and deactivation time goes to the nearest multiple of dt_ns counted from time 0, ties to the later one:
 *     q = floor((2 t_ns + dt_ns) / (2 dt_ns)) (floor division: right for negative times too), snapped time (q dt_ns) 1e-9 s;
 *   a time on the grid (t_ns % dt_ns == 0) keeps its bits: snapping an on-grid list changes nothing;
 *   |t| >= 1e9 s (the "never" of an open-ended contact) is kept;
 *   poses are not touched; the rounding is monotone, so the order of a foot's contacts and their non-overlap are kept.
 * Failure (the reference's `return false`, :588-592): a contact of positive duration whose snapped duration is zero, or a time that is not finite:
 * ok[b] = 0 for that problem (its times are still written: the finite ones snapped, the others unchanged), the rest of the batch is processed; the
 * function then returns CMPC_ERR_ARG.  Entries m >= n[b][c] are copied unchanged.  out_t may be t (in place).  dt <= 0 (or below 1 ns, or >= 1e9 s)
 * and a list length outside 0..max_contacts are argument errors.  Host buffers; no handle, no GPU. */
int cmpc_contacts_force_sample_time(int batch, int max_contacts, double dt, const double* t, const int* n, double* out_t, int* ok /* [B] or NULL */);
/* same on the device (one thread per problem, foot and contact; bit-equal to the host); dOk[B] or NULL; dOutT may be dT; asynchronous on `stream`
 * (NULL: the handle's).  A list length outside 0..max_contacts gives dOk = 0 and that foot's entries are neither read nor written. */
int cmpc_contacts_force_sample_time_device(cmpc_handle h, int max_contacts, double dt, const double* dT, const int* dN, double* dOutT, int* dOk,
                                           void* stream);

/* updateContactPhaseList, CentroidalMPCBlock.cpp:32-110 (call site :594-607): out = the planner's future contacts
 * (activation > now), preceded -- when the MPC's previous list has an active contact -- by that contact with the pose
 * the MPC gave it and the timing of the planner's active contact (:79-82).  Where the planner has no active contact
 * for such a foot the reference returns false (:69-77): ok[b] = 0 and the function returns CMPC_ERR_ARG after
 * processing the whole batch.  Host buffers; no handle, no GPU. */
int cmpc_contacts_merge(int batch, int max_contacts, double now, const double* plan_t, const float* plan_pose, const int* plan_n,
                        const double* mpc_t, const float* mpc_pose, const int* mpc_n, double* out_t, float* out_pose, int* out_n,
                        int* ok /* [B] or NULL */);
/* same on the device (one thread per problem and foot); dOk[B] or NULL; asynchronous on `stream` (NULL: the handle's).
 * A list length outside 0..max_contacts gives an empty merged list and dOk = 0 (nothing is read through it). */
int cmpc_contacts_merge_device(cmpc_handle h, int max_contacts, double now, const double* dPlanT, const float* dPlanPose,
                               const int* dPlanN, const double* dMpcT, const float* dMpcPose, const int* dMpcN, double* dOutT,
                               float* dOutPose, int* dOutN, int* dOk, void* stream);

/* setContactPhaseList, CentroidalMPCBlock.cpp:609: samples the lists at the knots now + k dt into the contact blocks of
 * P[B][n_p] (R, upper, lower, enabled, nominalPos, currentPos; the other entries of P are left alone).  Rule: stage k
 * is in contact iff a contact is active at its start; its orientation, box limits and the nominal position of knot
 * k+1 come from the stage's owner = the active contact, else the next one to activate, else the last.  box_upper /
 * box_lower [2][3]: bounding_box_{upper,lower}_limit of [CONTACT_i].  land[B][2] (or NULL) receives the landing knot of
 * each foot: first knot in contact after a swing stage, N if still in the air at the end, -1 if it never lifts.
 * A foot whose list is empty or longer than max_contacts: the host entry points return CMPC_ERR_ARG; the device kernel
 * leaves that foot's blocks of dP untouched and writes land = -2 (the caller must not solve that problem: the reference
 * aborts the tick when its merge fails, CentroidalMPCBlock.cpp:603-607). */
int cmpc_contacts_sample(int horizon, double dt, int batch, int max_contacts, double now, const double* t, const float* pose,
                         const int* n, const float* box_upper, const float* box_lower, float* P, int* land);
int cmpc_contacts_sample_device(cmpc_handle h, int max_contacts, double now, const double* dT, const float* dPose, const int* dN,
                                const float* box_upper /* host */, const float* box_lower /* host */, float* dP, int* dLand,
                                void* stream);
/* the same into the handle's own parameter set (what the class facade's setContactPhaseList calls) */
int cmpc_set_contact_lists(cmpc_handle h, int max_contacts, double now, const double* t, const float* pose, const int* n,
                           const float* box_upper, const float* box_lower, int* land);

/* getOutput().contactPhaseList, CentroidalMPCBlock.cpp:598, :626: the next contact (getNextContact(now)) of every foot
 * that lands inside the horizon takes the optimised landing position x.pos[land]. */
int cmpc_contacts_adjust(int horizon, int batch, int max_contacts, double now, const float* X, const int* land, const double* t,
                         float* pose, const int* n);
int cmpc_contacts_adjust_device(cmpc_handle h, int max_contacts, double now, const float* dX, const int* dLand, const double* dT,
                                float* dPose, const int* dN, void* stream);

/* setState on the device: dState[B][9] (com, dcom, h) and dWrench[B][N][6] (or NULL: left alone) into the rows of dP */
int cmpc_write_state_device(cmpc_handle h, const float* dState, const float* dWrench, float* dP, void* stream);

/* ONE receding-horizon tick of the whole batch as ONE call: what CentroidalMPCBlock::advance does between two solves
 * (CentroidalMPCBlock.cpp:586-626) and WholeBodyQPBlock::advance after it (WholeBodyQPBlock.cpp:1083-1150), chained on
 * `stream` (NULL: the handle's) without returning to the host in between:
 *   [io->force_sample_time: cmpc_contacts_force_sample_time_device (forceSampleTime :586-592) on the planner's lists, or on dList* on the first tick]
 *   -> cmpc_contacts_merge_device (updateContactPhaseList :594-607) -> cmpc_contacts_sample_device (setContactPhaseList :609)
 *   -> cmpc_write_state_device (setState :407) -> cmpc_shift_solution_device (is_warm_start_enabled; warm != 0)
 *   -> cmpc_solve_device[_warm] (advance :615) -> cmpc_contacts_adjust_device (getOutput :626) -> cmpc_plant_step_device.
 * Every step is what the entry point of that name computes, with the same argument checks; the steps in front of the solve are ONE launch and so are the
 * two behind it (they touch disjoint entries; same per-problem device functions: results identical to the last bit), so that a tick is three dispatches instead of ten.  It saves the
 * caller six trips through its FFI and the idle GPU time between them (a seventh of a tick at B <= 256,
 * tools/gpu_rollout_tick_overhead.py).  The reference rows of dP (comRef, hRef) are the caller's -- write them before the call -- unless dPlanCom / dPlanH are given.
 * All pointers are device pointers except box_upper / box_lower (host, [2][3]). */
typedef struct cmpc_tick_io {
    const double* dPlanT; const float* dPlanPose; const int* dPlanN; /* the planner's lists (layout above) */
    const double* dPrevT; const float* dPrevPose; const int* dPrevN; /* the MPC's lists of the previous tick.  All NULL (first tick):
                                                                        no merge, dList* is taken as the caller filled it, dOk is left alone */
    double* dListT; float* dListPose; int* dListN;                   /* this tick's lists: merged here, sampled, and step-adjusted after
                                                                        the solve (the next tick's dPrev*); must not alias dPrev* */
    int* dOk;               /* [B] merge status (0: the tick of that problem must be discarded, :603-607), or NULL */
    int* dLand;             /* [B][2] landing knots */
    const float* box_upper; const float* box_lower;
    const float* dState;    /* [B][9] measured com, dcom, h */
    const float* dWrench;   /* [B][N][6] or NULL (rows of dP left alone) */
    float* dP;              /* [B][n_p] */
    float* dX0;             /* [B][n_x] starting point: written (dX shifted by one knot) when warm != 0, read when warm == 0 */
    float* dX;              /* [B][n_x] previous solution in (warm != 0), this tick's solution out */
    float* dInfo;           /* [B][CMPC_INFO] */
    float* dStateOut;       /* [B][9] state at the next tick (may alias dState) */
    float* dZmp;            /* [B][2] or NULL */
    double plant_step; int plant_substeps; double zmp_half_x, zmp_half_y; /* as cmpc_plant_step_device */
    /* optional: the planner's CoM / angular-momentum trajectories (cmpc_write_reference_from_planner_device: [B][plan_knots][3] each, a knot every plan_dt seconds,
     * the first one plan_t_offset seconds before `now`) -- the tick then writes comRef / hRef of dP itself (setReferenceTrajectory, CentroidalMPCBlock.cpp:525-579).
     * Both NULL: the reference rows of dP are the caller's. */
    const float* dPlanCom; const float* dPlanH; int plan_knots; double plan_dt, plan_t_offset, robot_mass, com_height;
    /* 0 (a zero-initialised struct): the planner's times are used as given.  != 0: forceSampleTime (the rule at cmpc_contacts_force_sample_time, grid
     * = the handle's sampling_time) first.  Merge ticks: the planner's lists are snapped (the caller's dPlanT is not written) before the merge; a foot whose
     * snap fails is treated as an empty planner list: dOk = 0, its merged list is empty, dLand = -2, as a failed merge.  First tick: dListT is snapped in
     * place (the reference passes the snapped list on) and dOk IS written; a failed foot's dListN becomes 0 and dLand = -2.  Up to max_contacts = 16
     * the snap runs inside the front kernel (three launches per tick); beyond, one launch of the standalone kernel comes first (four launches; merge
     * ticks snap into a buffer the handle allocates on first use). */
    int force_sample_time;
} cmpc_tick_io;
int cmpc_rollout_tick_device(cmpc_handle h, int max_contacts, double now, int warm, const cmpc_tick_io* io, void* stream);

/* ---- a walk of the whole batch on the device: per-problem outcomes, the trace and the batch statistics written by a kernel ----
 * The reference runs one robot and ends its tick when updateContactPhaseList or advance fail (CentroidalMPCBlock.cpp:603-607, :615-619).  In a batch
 * every problem ends on its own terms: the record kernel runs behind a tick (one thread per problem), reads what the tick left and keeps, per problem,
 * whether and why it has ended.  Nothing is read back between the ticks.
 * Tick code, one int per problem and tick, first match wins:
 *     -1  the problem had ended before this tick
 *      1  the merge (or the snap of force_sample_time) failed: dOk[b] == 0
 *  1 + s  the solve's status s != 0 (dInfo word 5): 2 budget exhausted, 3 factorisation failed / not finite, 4 outside the supported subset
 *      5  an entry of dStateOut[b] is not finite
 *   6..9  with physical limits set (cmpc_set_walk_limits, below), behind all of the above: 6 height, 7 reach, 8 margin, 9 track out of its limit
 *      0  none of the above
 * stop_mask says which codes END a problem: bit 0 code 1 (always honoured, set or not: such a tick solved a stale problem), bit 1 codes 2..4, bit 2
 * code 5, bit 3 (value 8) codes 6..9.  A code whose bit is off is recorded and the problem walks on; that tick is a good tick like one with code 0.
 * Trace, row `row` of arrays with `rows` rows; every pointer may be NULL:
 *     dCom[rows][B][3], dZmp[rows][B][2]   float: bit copies of dStateOut[b][0..2] and dZmp[b]
 *     dLand[rows][B][2]                    int: dLand of the tick
 *     dLandingOffset[rows][B][2][3]        double: R^T (pos_k - nominalPos_k) of a foot whose landing knot k = dLand[b][c] has 0 < k <= N, zero otherwise;
 *                                          R = the column-major block of stage k - 1 in dP; the differences, products and three-term sums (left to
 *                                          right, not contracted) in double from the float values: the offset the NLP's box rows bound
 *     dIterations[rows][B], dCode[rows][B] int: dInfo word 0; the tick code
 * Rows of a problem that has ended, the ending tick included: NaN in the float and double arrays, -2 in dLand, 0 in dIterations; dCode holds the ending
 * code on the ending tick and -1 on later ticks.
 * Outcome, per problem, carried from call to call (all required; set up by cmpc_rollout_outcome_init_device):
 *     dEndTick[B]        int: -1 while walking, else `tick` of the call that ended it;  dEndCode[B] int: 0 while walking, else that tick's code
 *     dIterationsSum[B], dIterationsMax[B]  int: over its good ticks
 *     dFinalState[B][9]  float: dStateOut of its last good tick, or the initial state if it had none (kept here because a tick may run in place)
 *     dBoxSlackMin[B]    float, from +inf: the least of upper - off and off - lower over its good ticks, landing feet (0 < k <= N) and axes, off as in
 *                        dLandingOffset, the limits the handle's box (the last one a sampling or a tick uploaded), each slack formed in double and
 *                        rounded to float
 * Batch statistics, dStats[rows][6] int or NULL, row `row`: { problems not ended before the tick, problems ended by it, sum and max of dIterations over
 * the tick's good problems, problems not ended before the tick whose code is 2..4, the same for codes 6..9 (0 without limits) }: what a reduction of
 * the trace row gives.  Integer atomics, so
 * the result does not depend on the order: each wave reduces first, then adds once per word; lanes past B and lanes of ended problems contribute the
 * identity.  The call clears the row first.
 * Isolation: the record writes nothing a tick reads, so a recorded walk is bit-identical to an unrecorded one.  By default an ended problem stays in
 * every launch: it keeps running unobserved, holds its CU in every solve, a failed merge keeps failing, and its buffers go on being overwritten (only
 * dFinalState keeps a state of it worth reading).  cmpc_set_ended_device (below) takes it out:
 *   - with the mask set, everything a tick writes for an ended problem -- its rows of dP, dX0, dX, dInfo, dOk, dLand, dStateOut, dZmp, of both list
 *     sets and of the multiplier record -- holds, after any number of further ticks, exactly what it held after the problem's ending tick (the ending
 *     tick itself ran in full: the record that ends a problem runs behind it.  dStateOut of a problem ended at tick i is therefore what tick i left,
 *     one plant step past dFinalState, the state after its last GOOD tick);
 *   - every walking problem is bit-identical to the same walk without the mask;
 *   - with the mask NULL every entry point behaves as it does without this setting. */
typedef struct cmpc_walk_record {
    int rows;                /* rows of the trace arrays and of dStats */
    int stop_mask;
    float* dCom; float* dZmp; int* dLand; double* dLandingOffset; int* dIterations; int* dCode;                            /* trace */
    int* dEndTick; int* dEndCode; int* dIterationsSum; int* dIterationsMax; float* dFinalState; float* dBoxSlackMin;    /* outcome */
    int* dStats;
} cmpc_walk_record;
/* the outcome arrays at their start: dEndTick -1, dEndCode 0, the iteration words 0, dFinalState = dState0[B][9], dBoxSlackMin +inf (the trace and
 * dStats are not touched).  Asynchronous on `stream` (NULL: the handle's). */
int cmpc_rollout_outcome_init_device(cmpc_handle h, const float* dState0, const cmpc_walk_record* rec, void* stream);
/* the record of one tick (`tick`: the number dEndTick takes; 0 <= row < rec->rows) from what that tick left: dX, dP, dInfo, dOk (NULL: every merge
 * good -- a first tick without force_sample_time leaves dOk alone), dLand, dStateOut, dZmp (NULL only with rec->dZmp NULL).  Device pointers;
 * asynchronous on `stream` (NULL: the handle's); CMPC_ERR_ARG before any sampling or tick has given the handle its box. */
int cmpc_rollout_record_device(cmpc_handle h, int tick, int row, const float* dX, const float* dP, const float* dInfo, const int* dOk, const int* dLand,
                               const float* dStateOut, const float* dZmp, const cmpc_walk_record* rec, void* stream);
/* the same on the host: host buffers throughout (rec's pointers too), box_upper / box_lower [2][3]; no handle, no GPU.  Bit-equal to the kernel. */
int cmpc_rollout_record(int horizon, int batch, int tick, int row, const float* X, const float* P, const float* info, const int* ok, const int* land,
                        const float* state_out, const float* zmp, const float* box_upper, const float* box_lower, const cmpc_walk_record* rec);

/* ---- physical limits: a walk that can say its robot fell ----
 * The centroidal plant has no kinematics, so codes 1..5 end a problem for numerical reasons only.  With limits set, the record launch behind a tick also
 * forms four stability measures per problem and holds them against five limits: tick codes 6..9, behind the chain above (first match still wins, so a
 * tick whose code is 1..5 never takes one).  The measures refer to the time of dStateOut, t + dt, which is stage 1 of the tick's problem (N >= 2):
 * the support set S = { c : Gamma_c,1 > 0.5 }, foot c at q_c = pos_c[knot 1] of dX with the rotation R_c of stage 1 in dP and the corners the plant
 * kernel reads (the handle's, or the problem's own model's), com = dStateOut[0..2], dcom = dStateOut[3..5]:
 *     0 height  com_z - mean over c in S of q_c,z
 *     1 reach   max over c in S of |com - q_c|, in 3-D
 *     2 margin  the signed Euclidean distance of the capture point xi = com_xy + dcom_xy sqrt(max(height, 0) / gravity) to the support region, positive
 *               inside; the region is the convex hull of the xy of q_c + R_c corner_j over c in S, j = 0..3 (a rectangle, a point foot, a segment, a
 *               single point alike).  No hull is built: the margin is the least of max_k n.v_k - n.xi over the unit normals of every pair of the
 *               points and the unit directions from every point to xi (lengths under 1e-12 left out; 0 if none is left)
 *     3 track   |com_xy - comRef_xy[knot 1]|, the reference row of dP
 * in double from the float inputs, not contracted, sums left to right, each rounded to float ONCE; the limits are compared against that float, so every
 * ending can be recomputed from the trace exactly.  S empty: measures 0..2 are NaN.  A dStateOut that is not finite: all four are NaN.
 *     6  height < height_min or height > height_max      7  reach > reach_max      8  margin < margin_min      9  track > track_max
 * A NaN measure or a NaN limit never fires: NaN switches a limit off.  stop_mask bit 3 makes codes 6..9 END a problem; with the bit off they are
 * recorded and the problem walks on as a good tick.  dStats word 5 counts the problems not ended before the tick whose code is 6..9.
 *     dMeasures[rows][B][4] float or NULL: row `row` of every record launch.  A row is written on every tick of a problem that had not ended before it --
 *                           the tick a code 6..9 ends included, so the value that fired can be read; later ticks, and ticks ended by codes 1..5, hold NaN
 *     dExtremes[B][5] float or NULL: height min, height max, reach max, margin min, track max over the problem's GOOD ticks (a NaN measure is passed
 *                           over), carried from call to call; set up by cmpc_walk_extremes_init_device (+inf in the minima, -inf in the maxima)
 * cmpc_set_walk_limits is sticky on the handle, like cmpc_set_ended_device; lim == NULL: off (the default, and then every record launch is the one it
 * was without this setting).  The struct is copied, and captured when a launch is queued; the arrays must stay allocated until the queued launches have
 * run.  Every record launch of the handle then evaluates the limits: cmpc_rollout_record_device and every cmpc_rollout_walk_* call, the mismatch, taped,
 * refill and snapshot forms included -- the gates of the reverse and forward walks, the ended mask and the refill queue read dEndTick and so inherit the
 * physical endings.  On a refill walk dExtremes must be NULL (CMPC_ERR_ARG otherwise): a slot's extremes would span several trials, so per-trial
 * extremes come from the measures trace and dTrialOf; snapshots do not carry extremes.  CMPC_ERR_ARG for height_min > height_max, for dMeasures with
 * rows < 1, and, from the record calls, for a row >= rows.  Out of scope: per-trial limits, limits that must hold for n consecutive ticks.  (The
 * derivatives of the measures: "the measures, differentiated", behind the forward walk.) */
#define CMPC_WALK_MEASURES 4
#define CMPC_WALK_EXTREMES 5   /* height min, height max, reach max, margin min, track max */
typedef struct cmpc_walk_limits {
    double height_min, height_max, reach_max, margin_min, track_max;   /* NaN: off */
    float* dMeasures; int rows;     /* [rows][B][4] or NULL */
    float* dExtremes;               /* [B][5] or NULL, over the problem's good ticks */
} cmpc_walk_limits;
int cmpc_set_walk_limits(cmpc_handle h, const cmpc_walk_limits* lim);
int cmpc_walk_extremes_init_device(cmpc_handle h, float* dExtremes, void* stream);
/* cmpc_rollout_record with the limits, on the host: host buffers throughout (lim's arrays too), corners [2][4][3] float of problem 0 with problem b's
 * corners_stride floats further on (0: one set for the batch), gravity > 0, horizon >= 2; no handle, no GPU.  Bit-equal to the kernel.  lim == NULL:
 * cmpc_rollout_record, to the bit (corners and gravity are not read). */
int cmpc_rollout_record_limits(int horizon, int batch, int tick, int row, const float* X, const float* P, const float* info, const int* ok, const int* land,
                               const float* state_out, const float* zmp, const float* box_upper, const float* box_lower, const cmpc_walk_record* rec,
                               const cmpc_walk_limits* lim, const float* corners, int corners_stride, double gravity);

/* The cold start of cmpc_set_initial_guess with x0 == NULL as a kernel, from the caller's dP[B][n_p] into dX0[B][n_x]: CoM at com0 on every knot, feet at
 * nominalPos, f_z = (float)(gravity / 8) per corner and stage, every other entry zero; bit-equal to the host form.  Asynchronous on `stream` (NULL:
 * the handle's). */
int cmpc_cold_start_device(cmpc_handle h, const float* dP, float* dX0, void* stream);

/* `ticks` ticks, numbers tick0 .. tick0 + ticks - 1, queued on `stream` (NULL: the handle's) with no host wait: tick i runs at
 * now = (double)(tick0 + i) * sampling_time as the three launches of cmpc_rollout_tick_device plus the record launch, row row0 + i, tick number tick0 + i.
 * Every tick is bit-identical to the same calls made one by one.
 * io->tick: the buffers of cmpc_tick_io, with these differences.  dPrev* are not read: the lists alternate between two sets, set 0 = tick.dList*, set 1 =
 * dListTB / dListPoseB / dListNB.  `lists_in` (0 or 1) names the set that holds the lists of the tick before tick0; a tick merges into the other set,
 * and *lists_out (may be NULL) receives the set of the last tick's lists.  dState is read by the first tick only; later ticks run in place on dStateOut.
 * plan_t_offset is not read: tick i passes now - plan_t_first.  dWrenchTicks[wrench_ticks][B][N][6] (or NULL): tick i < wrench_ticks writes row i
 * into dP, later ticks leave the wrench rows alone, and tick.dWrench is not read; with dWrenchTicks NULL every tick writes tick.dWrench (NULL: none).
 * cold_first != 0: tick 0 of the call is a first tick -- no merge, set `lists_in` taken as the caller filled it (and kept: the next tick merges into the
 * other set), started from cmpc_cold_start_device launched between the front kernel and the solve (five launches), its record reads dOk only with
 * force_sample_time.  Every other tick is a warm merge tick.  The box is uploaded once; the event pair of cmpc_set_timing is left off for the call and
 * the setting restored.  rec may be NULL (no record launches).  On an error the ticks queued so far stay queued. */
typedef struct cmpc_walk_io {
    cmpc_tick_io tick;
    double* dListTB; float* dListPoseB; int* dListNB;   /* the second set of list buffers */
    double plan_t_first;                                /* time of the planner trajectories' first knot (with tick.dPlanCom / dPlanH) */
    const float* dWrenchTicks; int wrench_ticks;
} cmpc_walk_io;
int cmpc_rollout_walk_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                             int row0, int lists_in, int* lists_out, void* stream);
/* Ended problems out of the launches.  dEndTick: [B] device ints in the convention of cmpc_walk_record.dEndTick -- -1 a walking problem, >= 0 an ended
 * one -- or NULL: off (the default).  Sticky on the handle, like cmpc_set_warm_policy and cmpc_set_multiplier_output.  Only the pointer is kept: the words
 * are read on the device by each launch when that launch runs, so what the record kernel of tick i wrote is what tick i + 1 on the same stream sees, and a
 * walk passes rec->dEndTick itself:
 *     cmpc_set_ended_device(h, rec->dEndTick);  cmpc_rollout_walk_device(h, ...);  cmpc_set_ended_device(h, NULL);
 * (or the same around cmpc_rollout_tick_device + cmpc_rollout_record_device called tick by tick).  The pointer is captured when a launch is queued:
 * clearing the setting behind a queued walk does not affect the queued ticks, and the array must stay allocated until they have run.
 * While it is set, a problem whose word is >= 0 is left out of -- none of its data is written by --
 *   - the solve, whichever call launches it through the handle (cmpc_solve_device[_warm], cmpc_solve, cmpc_advance, the tick, the walk; both factor
 *     storages): no dX, no dInfo, no multiplier record, no factor scratch; its workgroup returns before it touches LDS and frees its CU at once
 *     (cmpc_solve / cmpc_advance still copy such a problem's rows back and judge its status words as they find them);
 *   - the front kernel of a tick (no merge, snap, sample, state, wrench or reference rows, no warm shift into dX0, no dOk, no dLand), the standalone
 *     snap launch a tick issues for max_contacts > 16, the cold start (of a walk's first tick and of cmpc_cold_start_device);
 *   - the back kernel of a tick (no dStateOut, no dZmp, no step adjustment of the list).
 * The record kernel needs nothing: it treats an ended problem from dEndTick alone.  No kernel gains a barrier and no tick gains a launch.  Every other
 * entry point (the single-step kernels, the NLP evaluations, the sensitivities) does not read the mask.  CMPC_ERR_ARG for a NULL handle. */
int cmpc_set_ended_device(cmpc_handle h, const int* dEndTick);
/* ---- refill: a queue of Q trials walked through the B slots of one walk (derivation and measurements: DESIGN.md 7f) ----
 * A Monte-Carlo study has Q >> B trials, and a slot whose robot has fallen is dead for the rest of a walk.  Here a slot takes the next trial of a queue the
 * tick after its robot ended or finished: one call walks Q trials through B slots, with no host read.  Three things become per problem for that: time -- a
 * trial spawned at tick s runs tick t at its LOCAL time (double)(t - s) * sampling_time, the very double a walk of its own would use, not a shifted plan; the
 * first tick -- a slot whose dStartTick equals the tick runs that tick as a first tick inside the merge launch (below); the wrench schedule -- per trial.
 * All arrays are device arrays (host arrays for cmpc_rollout_refill[_init]).
 *   per slot:   dStartTick[B] int, the tick number at which the slot's trial had local tick 0;  dTrial[B] int, the trial in the slot, -1: none
 *   queue:      trials = Q >= 0, trial_ticks >= 1 (the length of a trial);  dNext[1] int, the next trial to hand out;  dState0[Q][9] float;
 *               dWrenchTrials[wrench_ticks][Q][N][6] float or NULL: local tick r < wrench_ticks of trial q writes row [r][q] into dP, later ticks leave
 *               the wrench rows alone
 *   per trial:  dTrialEndTick (-1 while walking or walked through), dTrialEndCode, dTrialIterationsSum, dTrialIterationsMax [Q] int, dTrialFinalState
 *               [Q][9] float, dTrialBoxSlackMin [Q] float: the words of cmpc_walk_record's outcome arrays, tick numbers LOCAL;  dTrialTicks[Q] int: local
 *               ticks recorded so far;  dTrialSlot[Q], dTrialStart[Q] int: the slot and the start tick, -1 for a trial never started
 *   trace:      dTrialOf[trace_rows][B] int or NULL: row tick - trace_tick_first holds the trial that occupies each slot during that tick (-1: none);
 *               with it a caller reassembles per-trial traces from the slot-major trace of cmpc_walk_record
 * With trials == 0 the per-trial arrays and dState0 are not read. */
typedef struct cmpc_walk_refill_trace {
    int rows, tick_first;
    int* dTrialOf;
} cmpc_walk_refill_trace;
typedef struct cmpc_walk_refill {
    int trials, trial_ticks;
    int* dStartTick; int* dTrial; int* dNext;
    const float* dState0;
    const float* dWrenchTrials; int wrench_ticks;
    int* dTrialEndTick; int* dTrialEndCode; int* dTrialIterationsSum; int* dTrialIterationsMax; float* dTrialFinalState; float* dTrialBoxSlackMin;
    int* dTrialTicks; int* dTrialSlot; int* dTrialStart;
    cmpc_walk_refill_trace trace;
} cmpc_walk_refill;
/* Every slot empty (dTrial -1, dStartTick 0), *dNext = 0, every trial not started: its outcome as cmpc_rollout_outcome_init_device sets a problem's (final
 * state = dState0[q]), dTrialTicks 0, dTrialSlot and dTrialStart -1.  ONE launch / a host loop.  The refill in front of tick 0 then fills the B slots with
 * trials 0 .. B - 1.  (rec needs no set-up of its own for slots that get a trial; set it up with cmpc_rollout_outcome_init_device all the same when Q < B.) */
int cmpc_rollout_refill_init_device(cmpc_handle h, const cmpc_walk_refill* refill, void* stream);
int cmpc_rollout_refill_init(int batch, const cmpc_walk_refill* refill);
/* The refill in front of tick `tick_next`, ONE launch: two passes over the slots in ascending order.
 *   archive:  every occupied slot copies its outcome words from rec into its trial's row and sets dTrialTicks = tick_next - dStartTick.
 *   retire and spawn:  a slot is free if it is empty, if rec->dEndTick[b] >= 0, or if tick_next - dStartTick[b] >= trial_ticks.  Free slots, in ascending
 *     slot order, take trials *dNext, *dNext + 1, ...  A slot that receives trial q gets dTrial = q, dStartTick = tick_next, dStateLive[b] = dState0[q], its
 *     outcome in rec as cmpc_rollout_outcome_init_device sets it (end tick -1, code 0, iteration words 0, final state dState0[q], slack +inf), and
 *     dTrialSlot[q] = b, dTrialStart[q] = tick_next.  A free slot with no trial left gets dTrial = -1 and -- unless it was empty already and holds one --
 *     dEndTick = tick_next: it is out of every later launch through the ended mask.
 * The trace row tick_next - trace.tick_first (inside [0, trace.rows), else none) then receives dTrial of every slot.
 * dStateLive == NULL: the archive pass only -- nothing else is read or written.  A walk ends with one such call (tick_next = the tick after the last), since
 * the record of its last tick runs behind that tick's refill.
 * The assignment does not depend on scheduling: one workgroup walks the slots in chunks, a wave64 ballot ranks the free slots of a wave, the wave totals go
 * through LDS and a running base is carried from chunk to chunk; no atomics, and only that workgroup reads and writes *dNext.  The host form is bit-equal,
 * needs no handle and no GPU.  CMPC_ERR_ARG: a NULL argument or array (per-trial arrays excepted when trials == 0), trials < 0, trial_ticks < 1,
 * tick_next < 0, dWrenchTrials with wrench_ticks < 1. */
int cmpc_rollout_refill_device(cmpc_handle h, int tick_next, const cmpc_walk_record* rec, const cmpc_walk_refill* refill, float* dStateLive, void* stream);
int cmpc_rollout_refill(int batch, int tick_next, const cmpc_walk_record* rec, const cmpc_walk_refill* refill, float* state_live);
/* `ticks` ticks of a refill walk, numbers tick0 .. tick0 + ticks - 1, queued with no host read; each tick is FIVE launches: the refill with tick_next = tick
 * (dStateLive = io->tick.dStateOut, the buffer the walk runs in place on -- io->tick.dState must be that buffer), the tick's three, the record (row
 * row0 + i; the tick number dEndTick takes is the local one).  There is no cold_first: every tick is queued as a merge tick (lists as
 * cmpc_rollout_walk_device, `lists_in` / *lists_out), and a slot whose dStartTick equals the tick runs it as its first tick inside those launches:
 *   front kernel: no merge; its lists are the PLANNER's lists of its slot, snapped with force_sample_time, written to the set the tick writes (entries in use
 *     and the count; a foot whose snap fails gets the count 0 and no entry -- the entries of an empty list are not read); dOk = 1, or the snap's status; dX0 = the cold start of its dP (cmpc_cold_start_device's entries), in the same kernel;
 *   solve: inside the warm launch that problem takes the cold policy for its whole solve (not warm, the cold launch's barrier scalars).
 * Every other slot runs the merge tick it would run in a walk of its own, at its own local time, with plan_t_offset = local time - plan_t_first and the wrench
 * row of its trial.  A trial's outcome, trace rows, dX, dP, dInfo, state and the entries in use of its lists are those of cmpc_rollout_walk_device(cold_first = 1) on a batch
 * that holds it in the same slot; list entries past a foot's count are whatever the set held before.
 * While the call queues, the ended mask is rec->dEndTick itself; the handle's own setting is saved and restored.  io->tick.dWrench is not read.
 * CMPC_ERR_ARG before anything is queued: max_contacts > 16 (the first tick uses the front kernel's LDS stage), io->dWrenchTicks set (the schedule is the
 * per-trial one), rec NULL or with too few rows, io->tick.dState != io->tick.dStateOut, no dOk, and what cmpc_rollout_walk_device and
 * cmpc_rollout_refill_device refuse.  Tapes, gradients and forward mode are out of scope: no entry point takes a refill together with them.  (What is
 * now in: cmpc_rollout_walk_refill_taped_device tapes a refill walk slot-major and cmpc_rollout_tape_regroup_device gathers every trial's rows into a tape
 * of its own, on which the reverse and the forward walks run as they are -- behind the snapshot section; orientation and reference gradients, checkpoints
 * and trials from a snapshot stay out.)  Per-trial models and a per-trial plant mismatch are cmpc_rollout_walk_refill_trials_device's (below), of which this is the call with trials == NULL; trials that
 * start from a snapshot of a walk in progress instead of standing are cmpc_rollout_walk_refill_snapshot_device's (behind the snapshot section); a
 * footstep plan and reference trajectories per TRIAL instead of the slot's are cmpc_rollout_walk_refill_plans_device's (behind the regroup). */
int cmpc_rollout_walk_refill_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                    const cmpc_walk_refill* refill, int row0, int lists_in, int* lists_out, void* stream);
/* Per-trial data of a refill walk; every array is a device array indexed by TRIAL q (0 <= q < refill->trials), schedules by the trial's LOCAL tick r.
 * Each pointer may be NULL: that part is then what cmpc_rollout_walk_refill_device does today.  sizeof == 56 (LP64; the ctypes mirror is held to it). */
typedef struct cmpc_walk_refill_trials {
    const cmpc_model* dModels;  int* dModelOk;      /* [Q]; dModelOk [Q] or NULL: 1 / 0 written at the trial's first tick, untouched for a trial never started */
    const float* dHiddenWrench; int hidden_ticks;   /* [hidden_ticks][Q][6] */
    const float* dStateNoise;   int noise_ticks;    /* [noise_ticks][Q][9]  */
    const float* dForceGain;                        /* [Q] */
} cmpc_walk_refill_trials;
/* cmpc_rollout_walk_refill_device with what a Monte-Carlo study randomises per TRIAL: the robot (dModels, the rows of cmpc_set_models_device) and the
 * disturbance (the three parts of cmpc_plant_mismatch, row = the trial's local tick, column = the trial).  Still FIVE launches per tick; the solver kernel
 * is the one of every other entry point.  trials == NULL, or every pointer in it NULL: cmpc_rollout_walk_refill_device, bit for bit.
 *   dModels: on a slot's first tick the front kernel's workgroup writes the slot's record of the handle's per-problem table -- the handle's own record with
 *     dModels[q] applied, bit-equal to what cmpc_set_models_device would have put there; a row that breaks the model rule keeps the handle's model, is
 *     flagged (dModelOk[q] = 0) and ends the trial at its first tick through the solver's status 3.  The solve and the back kernel of that tick and of
 *     every later tick of the trial read the record in stream order.  The call allocates the table if needed and switches the handle to it before it queues
 *     anything, and leaves it switched on: AFTER THE CALL THE TABLE HOLDS EACH SLOT'S LAST TRIAL'S MODEL (a slot that never received a trial holds whatever
 *     it held before, behind the ended mask) -- follow the call with cmpc_set_models[_device] to go on with models of one's own.
 *   dStateNoise: the front kernel adds row [r][q] to the state the MPC measures, one float32 add, when 0 <= r < noise_ticks; else the plain copy.
 *   dHiddenWrench, dForceGain: the back kernel's plant step uses row [r][q] when 0 <= r < hidden_ticks -- outside the range the hidden term is not
 *     added (a select, never an add of zero) -- and dForceGain[q]; nothing of them is written to dP.
 * A trial's outcome, trace rows, dX, dP, dInfo, state and the entries in use of its lists are those of cmpc_rollout_walk_mismatch_device(cold_first = 1,
 * tick_first = 0) on a handle of the same batch size, factor storage and options that holds it in the same slot, with cmpc_set_models_device's row `slot`
 * the trial's model and the schedules' column `slot` the trial's rows.
 * CMPC_ERR_ARG before anything is queued: everything cmpc_rollout_walk_refill_device refuses, in its order; a negative count; a schedule with a zero
 * count; dModelOk without dModels. */
int cmpc_rollout_walk_refill_trials_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                           const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, int row0, int lists_in, int* lists_out,
                                           void* stream);
/* ---- the roll-out tick in reverse (derivation: DESIGN.md 7d) ----
 * Adjoint of the list path of one tick in the contacts' POSITIONS; times are not differentiated; the orientations have their own entry point below
 * (cmpc_contacts_orientation_vjp_device).  The forward maps move positions
 * through index maps that depend on the contact times only, so the adjoint needs the lists' times and counts, not their poses: the planner's lists, the
 * previous tick's and this tick's merged list as cmpc_rollout_tick_device (or the seven calls) left them, and dLand / dOk of that tick.  The maps are
 * re-derived with the forward's own functions (getActiveContact, getNextContact, the stage owner).  Gradients of list positions are double
 * [B][2][max_contacts][3], laid out like the position part of pose.
 *   adjust (phase bit 1; runs BEFORE the solution VJP, it adds to dGradX): where 0 <= land <= N and there is a next contact nx = getNextContact(now),
 *     dGradX[pos_c + 3 land] += dGradListOut[c][nx], and nothing of dGradListOut[c][nx] flows on to the merged list (the pose was overwritten after the
 *     sampling had read it; the sampling's own contribution to [c][nx] still does).  Every other entry passes through.
 *   sample (phase bit 2; runs AFTER the solution VJP, it reads dGradP): list entry m receives the sum over the stages k it owns of dGradP[nominalPos_c,k+1],
 *     and the owner of stage 0 also dGradP[nominalPos_c,0] + dGradP[currentPos_c] -- the "tied entries" sum of the solution sensitivities (subset rule 3).
 *   merge (phase bit 2): merged entry 0, when the previous list has an active contact ma, sends its gradient to dGradPrevList[c][ma]; the entries copied from
 *     the planner send theirs to dGradPlan[c][m] (optional, +=).  Entries at or beyond the list's length are not part of it and carry none.  First tick (dPrevT ==
 *     dPrevN == NULL: no merge): dGradPrevList is the list's gradient itself.
 * dGradPrevList is written whole.  Order of the float64 sums (one thread per problem and foot owns its entries, no atomics): the entry's own dGradListOut
 * first, then the sampling's terms stage by stage, k = 0 .. N-1, within stage 0 nominalPos_0, currentPos, nominalPos_1.
 * force_sample_time != 0: the planner's times are snapped first (the rule at cmpc_contacts_force_sample_time, grid = the handle's sampling_time), exactly
 * as the forward tick does, so that the index maps are those the forward saw (the first tick's list was snapped in place by the forward).
 * dOk[b] == 0 (a failed merge or snap; NULL: every problem is good): zero dGradPrevList, nothing added to dGradX or dGradPlan, dStatus[b] = 5; else
 * dStatus[b] = 0 (dStatus [B] or NULL; written by the phase-2 part).  A foot that was not sampled (dLand = -2) passes nothing on.
 * phase = 1, 2, or 3 (both parts in one launch: right when dGradP does not depend on dGradX).  dGradListOut NULL = zero; dGradP NULL = zero. */
int cmpc_contacts_position_vjp_device(cmpc_handle h, int max_contacts, double now, int phase, int force_sample_time, const double* dPlanT, const int* dPlanN,
                                      const double* dPrevT, const int* dPrevN, const double* dListT, const int* dListN, const int* dLand, const int* dOk,
                                      const double* dGradListOut, const float* dGradP, float* dGradX, double* dGradPrevList, double* dGradPlan, int* dStatus,
                                      void* stream);

/* The orientation counterpart of the sample + merge part, with the same tape arguments.  Gradients are double [B][2][max_contacts][3] in the body-frame
 * tangent of each entry's quaternion, q <- q (x) exp(omega / 2) (the convention of cmpc_contacts_rotation_vjp_device).  The forward maps copy quaternions,
 * and in this tangent every copy is the identity: no pose is needed, the index maps come from the times.
 *   entry gradient: every entry m < n of this tick's list carries dGradListRotOut[c][m] -- NO entry is cut: the step adjustment overwrites positions only, so
 *     the landing entry's orientation passes through to the next tick.
 *   sample: entry o receives the sum over the stages k it owns (cmpc_stage_owner) of dGradRot[c][k], in stage order k = 0 .. N-1 -- what
 *     cmpc_contacts_rotation_vjp_device computes.
 *   merge: merged entry 0, when the previous list has an active contact ma, sends its gradient to dGradPrevListRot[c][ma]; the entries copied from the planner
 *     send theirs to dGradPlanRot[c][first + m - n0] (optional, +=).  First tick (dPrevT == dPrevN == NULL): dGradPrevListRot is the list's gradient itself, and
 *     with dGradListRotOut == NULL it equals cmpc_contacts_rotation_vjp_device's result bit for bit.
 * dGradPrevListRot is written whole; entries at or beyond n carry nothing; a foot that was not sampled (dLand = -2, an empty list, n > max_contacts) passes
 * nothing on; dOk[b] == 0 gives zeros, adds nothing to dGradPlanRot and sets dStatus[b] = 5 (else 0; dStatus [B] or NULL); force_sample_time as above.  One
 * thread per (problem, foot) owns its outputs; float64 sums in the order stated (the entry's own gradient, then the stages); no atomics.  dGradRot
 * [B][2][N][3] NULL = zero, dGradListRotOut NULL = zero, dLand may be NULL. */
int cmpc_contacts_orientation_vjp_device(cmpc_handle h, int max_contacts, double now, int force_sample_time, const double* dPlanT, const int* dPlanN,
                                         const double* dPrevT, const int* dPrevN, const double* dListT, const int* dListN, const int* dLand, const int* dOk,
                                         const double* dGradListRotOut, const double* dGradRot, double* dGradPrevListRot, double* dGradPlanRot, int* dStatus,
                                         void* stream);

/* One tick in reverse.  What a forward tick left behind is a tape of read-only device pointers: the tick's solution, parameters and multipliers
 * (cmpc_get_multipliers_device right after that tick's solve, with the multiplier output on -- x and info are bit-identical with it on, so a taped roll-out
 * is bit-identical to an untaped one), the state that went IN (copy it before the tick: a roll-out may alias dState / dStateOut), dInfo, dOk, dLand, the
 * times and counts of the planner's, the previous tick's (both NULL on the first tick) and the merged lists (copy the previous tick's before the tick if the
 * roll-out alternates two list buffers), and the plant's step.  No new forward entry point is needed.
 * Chain, on one stream: cmpc_plant_step_vjp_device -> the adjust part of cmpc_contacts_position_vjp_device -> cmpc_solution_vjp_model_device (called, not
 * copied: its definition, its workspace and its dSens hold) -> gState += gP[com0, dcom0, h0] (cmpc_write_state_device in reverse) -> the sample + merge part.
 * The solution map is taken as independent of x0: warm start, shift and cold restart carry no derivative.  The planner's reference rows are inputs of the
 * tick, not functions of the state: their gradient arrives in dGradP, which cmpc_reference_from_planner_vjp_device carries to the planner's trajectories.
 * Inputs: dGradStateOut[B][9] double, dGradListOut[B][2][max_contacts][3] double or NULL (zero), dGradX[B][n_x] float or NULL (a loss on this tick's solution).
 * Outputs: dGradState[B][9] double (may alias dGradStateOut), dGradPrevList[B][2][max_contacts][3] double (must not alias dGradListOut), dGradWrench[B][N][6]
 * float or NULL (the fExt / tauExt rows of gP, laid out as cmpc_write_state_device's dWrench), dGradPlan or NULL (+=), dGradModel[B][34] double or NULL (+=),
 * dGradP[B][n_p] float or NULL (the tick's full dl/dp: the solve's, plus the plant's on fExt_0 / tauExt_0), dTickSens[B][CMPC_SENS] float: dSens of the
 * solution VJP with word 0 replaced by the tick's status: 0 ok; 1..3 as the solution sensitivities; 4 the solve's status is not 0 (not converged, or flagged);
 * 5 the merge failed (dOk == 0).  Precedence: 5, then 2 and 3 (they speak of the inputs), then 4, then 1.  A flagged problem gets zeros in every array (nothing is added to the += outputs); its
 * neighbours are bit for bit what they are without it.  Workspace: per-handle HBM allocated on first use by whichever of the two tick entry points runs
 * first, 4 (n_x + 2 n_p) + 48 N + 652 bytes per problem (the rotation entry's arrays, 48 N + 48, and the mismatch entry's, 56, included); calls on one handle run one after the other
 * whatever their streams (an event, as for the solution sensitivities). */
typedef struct cmpc_tick_tape {
    const float* dX; const float* dP; const float* dLamG;   /* [B][n_x], [B][n_p], [B][n_g] of the tick's solve */
    const float* dState;                                     /* [B][9] the state the tick started from */
    const float* dInfo;                                      /* [B][CMPC_INFO] */
    const int* dOk;                                          /* [B] merge status, or NULL (every problem good) */
    const int* dLand;                                        /* [B][2] */
    const double* dPlanT; const int* dPlanN;                 /* the planner's lists: times [B][2][M][2] and counts [B][2] (merge ticks) */
    const double* dPrevT; const int* dPrevN;                 /* the previous tick's; both NULL on the first tick */
    const double* dListT; const int* dListN;                 /* this tick's (merged) list */
    double plant_step; int plant_substeps;                   /* as the forward tick's */
    int force_sample_time;                                   /* as the forward tick's */
} cmpc_tick_tape;
int cmpc_rollout_tick_vjp_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, const double* dGradStateOut,
                                 const double* dGradListOut, const float* dGradX, double* dGradState, double* dGradPrevList, float* dGradWrench,
                                 double* dGradPlan, double* dGradModel, float* dGradP, float* dTickSens, void* stream);
/* The same tick with the contacts' ORIENTATIONS carried along (the tangents above).  Further arguments: dGradListRotOut[B][2][max_contacts][3] double or NULL
 * (zero): dl / d(orientations of this tick's outgoing list); dGradPrevListRot[B][2][max_contacts][3] double (written whole; must not alias dGradListRotOut);
 * dGradPlanRot or NULL (+=); dGradRot[B][2][N][3] double or NULL: the tick's full per-stage dl/domega -- the solve's, plus the plant's dGradRot0 on stage 0.
 * Chain, on one stream: cmpc_plant_step_vjp_rot_device -> the adjust part -> cmpc_solution_vjp_rot_device (called, not copied: ONE adjoint solve for p, model
 * and rotations; its dGradP and dGradModel are cmpc_solution_vjp_model_device's bit for bit) -> the combine kernel (also stage 0 += dGradRot0, and zeros in the
 * rotation arrays of a flagged problem) -> the position sample + merge part -> cmpc_contacts_orientation_vjp_device: one launch more than the entry above.
 * Every output the entry above also has is bit-identical to it on the same tape.  dTickSens is the rotation VJP's dSens (word 0 replaced as above): words 5
 * and 6 and the internal-force removal are those of "rotation directions" -- a double-support tick under load has no orientation derivative and says so in
 * word 6.  Status codes and precedence as above; a flagged problem gets zeros in the rotation outputs and adds nothing to dGradPlanRot. */
int cmpc_rollout_tick_vjp_rot_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, const double* dGradStateOut,
                                     const double* dGradListOut, const float* dGradX, double* dGradState, double* dGradPrevList, float* dGradWrench,
                                     double* dGradPlan, double* dGradModel, float* dGradP, float* dTickSens, const double* dGradListRotOut,
                                     double* dGradPrevListRot, double* dGradPlanRot, double* dGradRot, void* stream);

/* ---- the roll-out tick FORWARDS, in k directions (derivation: DESIGN.md 7d, "Forwards") ----
 * The transposes of the entry points above: the same linear maps at the same tape, applied to k direction columns per problem instead of one cotangent.
 * Every direction array carries a column axis right behind the batch axis, [B][k][...].
 *
 * The plant JVP with k columns: one thread per (problem, column) runs the partials and the JVP of cmpc_plant_step_jvp_rot_device.  dDirState[B][k][9]
 * double, dDirX[B][k][n_x] float, dDirP[B][k][n_p] float, dDirModel[B][k][34] double, dDirRot0[B][k][2][3] double -> dDirStateOut[B][k][9] double (may
 * alias dDirState).  NULL rules as cmpc_plant_step_jvp_rot_device (dDirState is required; dDirRot0 NULL is the kernel without the rotation term).  Column j
 * is bit-equal to that entry point on column j alone. */
int cmpc_plant_step_jvp_cols_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, int k,
                                    const double* dDirState, const float* dDirX, const float* dDirP, const double* dDirModel, const double* dDirRot0,
                                    double* dDirStateOut, void* stream);
/* The list path of one tick forwards, positions and orientations together, with the tape arguments of cmpc_contacts_position_vjp_device /
 * cmpc_contacts_orientation_vjp_device; the index maps are re-derived from the times with the forward's own functions.  One thread per (problem, foot,
 * column) owns its outputs: copies only, no atomics.  List directions are double [B][k][2][max_contacts][3], orientations in the body-frame tangent.
 *   merge + sample (phase bit 1; runs BEFORE the solution JVP): merged entry 0 takes the direction of the previous list's active contact,
 *     dDirPrevList[c][ma]; the entries copied from the planner take dDirPlan[c][first + m - n0] (zero when that lies beyond the array); first tick (dPrevT ==
 *     dPrevN == NULL): the list's direction is dDirPrevList itself and the planner's directions are not read.  The owner of stage k writes its position
 *     direction to nominalPos_{c,k+1} of column j of dDirP[B][k][n_p] float (stage 0 also to nominalPos_{c,0} and currentPos_c: 6 (N + 2) rows per column
 *     are written, the others are left alone) and its orientation direction to omega_{c,k} of dDirRot[B][k][2][N][3] double.  The list's orientation
 *     direction goes out unchanged: no entry is cut.  dDirList, dDirListRot, the rows of dDirP and dDirRot are written whole; entries at or beyond n are 0.
 *   adjust (phase bit 2; runs AFTER the solution JVP, it reads dDirX[B][k][n_x] float): where 0 <= land <= N and there is a next contact nx,
 *     dDirList[c][nx] is OVERWRITTEN with dDirX[pos_c + 3 land] -- the transpose of "nothing of dGradListOut[c][nx] flows on".
 * A foot that was not sampled (dLand = -2, an empty list, n > max_contacts) passes nothing on.  dOk[b] == 0 gives zeros (phase 2 alone zeroes the list
 * directions) and dStatus[b] = 5, else 0 (dStatus[B] or NULL).  force_sample_time as above.  phase = 1, 2 or 3.  dDirList is required and must not alias
 * dDirPrevList; every other direction pointer may be NULL (inputs: zero; outputs: not written). */
int cmpc_contacts_jvp_device(cmpc_handle h, int max_contacts, double now, int phase, int force_sample_time, int k, const double* dPlanT, const int* dPlanN,
                             const double* dPrevT, const int* dPrevN, const double* dListT, const int* dListN, const int* dLand, const int* dOk,
                             const double* dDirPrevList, const double* dDirPrevListRot, const double* dDirPlan, const double* dDirPlanRot, const float* dDirX,
                             double* dDirList, double* dDirListRot, float* dDirP, double* dDirRot, int* dStatus, void* stream);
/* One tick forwards in k directions, on the tape of cmpc_rollout_tick_vjp_device: no new forward entry point, no change to the tape.
 * Chain, on one stream: the merge + sample part of cmpc_contacts_jvp_device -> the p direction of every column assembled in float32 (the list's rows; the
 * state direction on com0 / dcom0 / h0, cmpc_write_state_device's rows; the wrench direction on the fExt / tauExt rows; plus the caller's dDirP) ->
 * cmpc_solution_jvp_rot_device (called, not copied: its definition, its chunks of eight columns, its workspace, its internal-force rule and its dSens hold) ->
 * the tick's flags -> the adjust part -> cmpc_plant_step_jvp_cols_device, which reads dDirX, the knot-0 wrench rows of the assembled p direction, dDirModel
 * and stage 0 of the rotation direction.  The state direction reaches the plant in double and the solve rounded to float32.  As in reverse, the solution map
 * is taken as independent of x0, and the planner's reference rows are inputs (their direction enters through dDirP).
 * cmpc_tick_dirs: every pointer may be NULL (zero; `in` itself may be NULL).  With dDirPrevListRot == dDirPlanRot == NULL no rotation direction exists: the
 * solve and the plant run without one, bit for bit cmpc_solution_jvp_model_device / cmpc_plant_step_jvp_device.
 * cmpc_tick_dirs_out: dDirStateOut and dDirList are required; dDirList is the next tick's dDirPrevList and must not alias it (nor dDirListRot
 * dDirPrevListRot).
 * dTickSens[B][CMPC_SENS] float: dSens of the solution JVP with word 0 replaced by the tick's status, codes and precedence as cmpc_rollout_tick_vjp_device
 * (5, then 2 and 3, then 4, then 1; a non-finite tape state gives 2, as it does in reverse through the plant VJP).  A flagged problem gets zeros in every output of every column (the transpose of the VJP's zero map); its neighbours
 * are bit for bit what they are without it.  Results depend on nothing but the problem's own inputs and the column: not on k, the batch position or the
 * batch size.  Workspace: per-handle HBM allocated on first use and grown when a larger k arrives (that call waits for the device),
 * 4 (n_x + n_p) + 48 N + 120 bytes per problem and column, plus 4 bytes per problem; calls on one handle run one after the other whatever their streams
 * (the event of the tick VJP). */
typedef struct cmpc_tick_dirs {
    const double* dDirState;                                  /* [B][k][9] */
    const double* dDirPrevList; const double* dDirPrevListRot; /* [B][k][2][max_contacts][3]: the previous tick's list (first tick: the list itself) */
    const double* dDirPlan; const double* dDirPlanRot;         /* [B][k][2][max_contacts][3]: the planner's contacts (not read on a first tick) */
    const float* dDirWrench;                                  /* [B][k][N][6], laid out as cmpc_write_state_device's dWrench */
    const double* dDirModel;                                  /* [B][k][34] */
    const float* dDirP;                                       /* [B][k][n_p], added to the assembled p direction: reference rows, boxes.  Entries of R and
                                                                 Gamma are read as zero, as the solution JVP reads them */
} cmpc_tick_dirs;
typedef struct cmpc_tick_dirs_out {
    double* dDirStateOut;                                     /* [B][k][9], required; may alias dDirState */
    double* dDirList;                                         /* [B][k][2][max_contacts][3], required */
    double* dDirListRot;                                      /* [B][k][2][max_contacts][3] or NULL */
    float* dDirX;                                             /* [B][k][n_x] or NULL: the solution's direction */
    double* dDirRot;                                          /* [B][k][2][N][3] or NULL: the per-stage rotation direction the solve was given */
    float* dDirPFull;                                         /* [B][k][n_p] or NULL: the assembled p direction the solve was given */
} cmpc_tick_dirs_out;
int cmpc_rollout_tick_jvp_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, int k, const cmpc_tick_dirs* in,
                                 const cmpc_tick_dirs_out* out, float* dTickSens, void* stream);

/* ---- the device walk taped and run in reverse, per-problem endings kept (derivation and the rule: DESIGN.md 7f) ----
 * cmpc_walk_tape: what cmpc_rollout_tick_vjp_device needs of `rows` ticks, in device arrays the caller owns (BatchSolver.walk_tape allocates them), row
 * after row laid out like the fields of cmpc_tick_tape; M = max_contacts:
 *     dX[rows][B][n_x], dP[rows][B][n_p], dLamG[rows][B][n_g], dInfo[rows][B][CMPC_INFO]   float
 *     dStates[rows + 1][B][9]                                                              float: row r the state tick r started from, row r + 1 what it left
 *     dOk[rows][B], dLand[rows][B][2]                                                      int
 *     dPlanT, dListT[rows][B][2][M][2]                                                     double: the planner's and the merged lists' times
 *     dPlanN, dListN[rows][B][2]                                                           int
 * The previous tick's list of row r is row r - 1's dListT / dListN: no second copy is kept.  The planner's times are copied per row, so that a replanned
 * walk tapes correctly and the tape does not depend on the caller's buffers staying alive.  Host scalars: plant_step, plant_substeps, force_sample_time as
 * the forward ticks'; first_row_is_first_tick != 0: row 0 is a first tick (no merge, no previous list) -- otherwise row 0 cannot be reversed.
 * Size: 4 (n_x + n_p + n_g) + 64 M + 96 bytes per problem and tick (the three wide rows, then 2 x 32 M of times, info 32, state 36, ok 4, land and the two
 * counts 8 each), about 12 KB at N = 20 (x, p and lam_g are a thousand floats each).
 * Both walks below carry the contacts' orientations on this layout too: nothing more is taped for them.  Contact times and Gamma stay undifferentiated,
 * as everywhere. */
typedef struct cmpc_walk_tape {
    int rows;
    float* dX; float* dP; float* dLamG; float* dInfo; float* dStates;
    int* dOk; int* dLand;
    double* dPlanT; double* dListT; int* dPlanN; int* dListN;
    double plant_step; int plant_substeps; int force_sample_time; int first_row_is_first_tick;
} cmpc_walk_tape;
/* One row of the tape from what a tick left, in two parts (`parts`: 1, 2 or 3 = both):
 *   part 1, BEFORE the tick: dStateIn[B][9] -> dStates[row].  Needed for the first taped tick only (every later row was written by part 2 of the row before);
 *     it exists because a roll-out runs in place (dState == dStateOut): the state a tick started from is gone once it has run.
 *   part 2, BEHIND the tick: one launch of cmpc_rollout_tape_kernel makes bit copies of dX, dP, dInfo, dOk (NULL -- a first tick without force_sample_time
 *     leaves dOk alone -- gives dOk = 1 for every problem, as the record treats it), dLand, dPlanT / dPlanN (NULL on a first tick: the row is left alone),
 *     dListT / dListN, and dStateOut -> dStates[row + 1]; then cmpc_get_multipliers_device (called, not copied) writes the row's dLamG.
 * parts = 3 does both behind a tick that did NOT run in place.  cmpc_rollout_walk_taped_device uses part 1 in front of its first tick and part 2 behind every tick.
 * The multiplier output must be on already (cmpc_set_multiplier_output: turning it on synchronises, so it is not done here): else CMPC_ERR_ARG.  x and info
 * are bit-identical with it on.  Device pointers; asynchronous on `stream` (NULL: the handle's).  With cmpc_set_ended_device set nothing changes here: an ended
 * problem's buffers are frozen, so its later rows hold its ending tick's data. */
int cmpc_rollout_tape_device(cmpc_handle h, int max_contacts, int row, int parts, const float* dX, const float* dP, const float* dInfo, const int* dOk,
                             const int* dLand, const float* dStateIn, const float* dStateOut, const double* dPlanT, const int* dPlanN, const double* dListT,
                             const int* dListN, const cmpc_walk_tape* tape, void* stream);
/* cmpc_rollout_walk_device with the tape part behind every tick: tick i of the call writes row tape_row0 + i (part 1 in front of tick 0 of the call, part 2
 * and the multipliers behind each tick: two launches more per tick).  Every tick is bit-identical to the untaped walk's and the record is unchanged.  tape's
 * scalars must agree with io (plant_step, plant_substeps, force_sample_time; first_row_is_first_tick with cold_first when tape_row0 == 0) and the multiplier
 * output must be on: else CMPC_ERR_ARG. */
int cmpc_rollout_walk_taped_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                   int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream);
/* ---- the state of a walk between two ticks: save, restore, branch ("Snapshots") ----
 * cmpc_walk_snapshot: everything tick `tick` of a walk reads that an earlier tick wrote, in device arrays the caller owns (BatchSolver.walk_snapshot
 * allocates them), M = max_contacts:
 *     dState[B][9], dP[B][n_p] (its wrench rows survive the ticks past wrench_ticks, so it belongs), dX[B][n_x], dX0[B][n_x], dInfo[B][CMPC_INFO], dZmp[B][2]   float
 *     dOk[B], dLand[B][2]                                                                    int
 *     both list sets, set 0 = dListT / dListPose / dListN, set 1 = dListTB / dListPoseB / dListNB (the sets of cmpc_walk_io):
 *     t[B][2][M][2] double, pose[B][2][M][7] float, n[B][2] int, twice
 *     the six outcome arrays of cmpc_walk_record: dEndTick, dEndCode, dIterationsSum, dIterationsMax [B] int, dFinalState[B][9], dBoxSlackMin[B] float
 * and two host words: `tick`, the number of the next tick, and `lists_in`, the set that holds the lists of the tick before it (cmpc_rollout_walk_device's
 * argument of that name).  dX0, dInfo and dZmp may be NULL, in the source or in the destination, and are then skipped: a walking problem's next tick
 * overwrites all three before it reads them; they are in the struct so that an ENDED problem's rows of a resumed walk equal the unbroken walk's.  The
 * trace and the statistics of a record are not part of it (a resumed walk writes its own rows), nor is anything in the handle: a tick reads nothing of an
 * earlier tick through the handle (the box, the models and the warm policy are settings, the same in every tick).
 * The live buffers of a walk are described by the same struct, so ONE copy serves as save (live -> snapshot) and as restore (snapshot -> live).
 * Size: 4 (2 n_x + n_p) + 176 M + 160 bytes per problem (the three wide rows; 2 x (32 M + 56 M + 8) of lists; state 36, info 32, zmp 8, ok 4, land 8; the
 * outcome 4 x 4 + 36 + 4), about 13 KB at N = 20 -- one row of the tape above: cmpc_walk_snapshot_bytes.
 * cmpc_rollout_snapshot_device: ONE launch, asynchronous on `stream` (NULL: the handle's), no host read.  Destination problem b (b < the handle's batch)
 * receives the bit copy of source problem dIndex[b] (dIndex: [B] device ints; NULL: source problem b, and src_batch must then equal the batch); the source
 * arrays hold src_batch problems.  An index outside [0, src_batch) leaves that destination problem entirely unwritten and sets dOk[b] = 0 when dOk ([B]
 * device ints, or NULL) is given, otherwise dOk[b] = 1: the idiom of cmpc_set_models_device.  Repeated indices are the normal case of branching.  The
 * host words of dst are the caller's to set.  One workgroup per destination problem; the index is read once per row; the rows of 64 words and more go as
 * 16-byte pieces aligned on the destination, with a head and a tail of single words (n_x and n_p are not multiples of four floats at every N); no LDS,
 * no barrier, no atomics.
 * CMPC_ERR_ARG: a NULL handle, src or dst; a NULL required pointer (every array but dX0, dInfo, dZmp) in either; max_contacts < 1; src_batch < 1;
 * dIndex == NULL with src_batch != batch; any destination array that is also a source array. */
typedef struct cmpc_walk_snapshot {
    int tick; int lists_in;
    float* dState; float* dP; float* dX; float* dX0; float* dInfo; float* dZmp;
    int* dOk; int* dLand;
    double* dListT; float* dListPose; int* dListN;
    double* dListTB; float* dListPoseB; int* dListNB;
    int* dEndTick; int* dEndCode; int* dIterationsSum; int* dIterationsMax; float* dFinalState; float* dBoxSlackMin;
} cmpc_walk_snapshot;
int cmpc_rollout_snapshot_device(cmpc_handle h, int max_contacts, int src_batch, const cmpc_walk_snapshot* src, const cmpc_walk_snapshot* dst,
                                 const int* dIndex, int* dOk, void* stream);
/* the same on the host: host buffers throughout; no handle, no GPU.  Bit-equal to the kernel. */
int cmpc_rollout_snapshot(int horizon, int batch, int src_batch, int max_contacts, const cmpc_walk_snapshot* src, const cmpc_walk_snapshot* dst,
                          const int* index, int* ok);
/* bytes per problem of a snapshot with all its arrays (the formula above); 0 for horizon < 1 or max_contacts < 1 */
size_t cmpc_walk_snapshot_bytes(int horizon, int max_contacts);
/* Trials that start from a snapshot of a walk in progress (DESIGN.md 7f "Refill", "Trials from a snapshot"): every trial of the queue is a fork of one row
 * of a POOL of saved problems (cmpc_walk_snapshot arrays of pool_batch problems, filled by cmpc_rollout_snapshot_device) and walks trial_ticks RESUMED
 * ticks from the pool's tick t_s = pool->tick.  sizeof == 32 (LP64; the ctypes mirror is held to it). */
typedef struct cmpc_walk_refill_snapshot {
    const cmpc_walk_snapshot* pool;   /* device arrays of pool_batch problems; pool->tick = t_s >= 1, pool->lists_in as saved */
    int pool_batch;
    const int* dTrialSnapshot;        /* [Q] device: the pool row trial q starts from; repeats are the normal case */
    int* dTrialSnapshotOk;            /* [Q] device or NULL: 1 / 0 written when the trial is spawned, untouched for a trial never started */
} cmpc_walk_refill_snapshot;
/* cmpc_rollout_walk_refill_trials_device with trials that start mid-walk.  from == NULL: that call, bit for bit.  Otherwise, with t_s = from->pool->tick:
 *   - Who gets which slot does not change: the refill launch, its free rule, dStartTick (the spawn tick s), dTrialTicks, dTrialSlot, dTrialStart and
 *     trial_ticks (now the RESUMED ticks of a trial) keep their meaning.
 *   - A tick is SIX launches: the restore launch goes between the refill launch and the front kernel, one workgroup per slot.  A workgroup whose slot
 *     was not spawned this tick returns after one scalar load (dStartTick[b] != tick; an empty slot whose word happens to match, after a second: no
 *     trial in it).  The gate is workgroup-uniform and comes ahead of everything.  A spawned slot with trial q receives the bit
 *     copy of pool row dTrialSnapshot[q] into the live buffers, through cmpc_rollout_snapshot_device's row copy: state (into io->tick.dStateOut), dP, dX,
 *     dOk, dLand; dX0, dInfo and dZmp where both sides have them; the six outcome arrays into rec, over the refill launch's fresh outcome; and both list
 *     sets -- the pool's set pool->lists_in goes to the set THIS tick reads as "previous", the pool's other set to the other live set (the live parity
 *     alternates with the walk tick, the pool's is fixed).  dTrialSnapshotOk[q] = 1.
 *   - An index outside [0, pool_batch): nothing is copied, dTrialSnapshotOk[q] = 0, the slot's dEndTick = t_s and dEndCode = 0: the slot is behind the
 *     ended mask for this tick's other launches and is archived and freed by the next refill.
 *   - A pool row that had already ended: its outcome is restored with it, so the trial is ended at spawn the same way, with that row's outcome.
 *   - Time: a slot spawned at s runs tick t at local tick t_s + (t - s); the integer sum is converted once, now = (double)(t_s + t - s) * sampling_time
 *     -- the double cmpc_rollout_walk_device uses for that tick -- in the front kernel, the back kernel and the planner offset.  The outcome's tick
 *     numbers are whole-walk numbers, t_s + (t - s).
 *   - No cold first tick: the spawn tick is an ordinary warm merge tick on the restored lists and the restored dX (no planner lists as the slot's own, no
 *     cold dX0, no cold policy in the solve: every problem of every solve is warm).
 *   - Everything the trial owns is indexed by r = t - s, the ticks since spawn: dWrenchTrials, the three schedules of cmpc_walk_refill_trials, and the
 *     per-trial model write at r == 0 -- cmpc_rollout_walk_mismatch_device's rows with tick_first = t_s.
 *   - refill->dState0 does not reach a spawned trial (the refill launch, unchanged, still copies it into the state and the final state, and the restore
 *     overwrites both; a trial whose index lies outside the pool keeps it as its final state).  The pool's own wrench schedule is not continued: the
 *     restored wrench rows of dP stay until a dWrenchTrials row overwrites them.
 * A trial's outcome, its trace rows, and the dX, dP, state and in-use list entries of each slot's last trial are those of
 * cmpc_rollout_walk_mismatch_device(cold_first = 0, tick0 = t_s) run after a cmpc_rollout_snapshot_device restore of the same pool row, on a handle of the
 * same batch size, factor storage and options that holds the trial in the same slot, with cmpc_set_models_device's row `slot` the trial's model and the
 * schedules' column `slot` the trial's rows.
 * CMPC_ERR_ARG before anything is queued: everything cmpc_rollout_walk_refill_trials_device refuses, in its order (max_contacts > 16 stays refused); and
 * with from != NULL: pool NULL, pool->tick < 1, pool_batch < 1, a required pool array NULL (every array but dX0, dInfo, dZmp), pool->lists_in not 0 or 1,
 * dTrialSnapshot NULL with refill->trials > 0, a pool array that is also a live array.  The refusals that need no handle come ahead of the handle check. */
int cmpc_rollout_walk_refill_snapshot_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                             const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, const cmpc_walk_refill_snapshot* from,
                                             int row0, int lists_in, int* lists_out, void* stream);
/* The restore launch of tick `tick` on the host: host buffers throughout; no handle, no GPU.  Bit-equal to the kernel.  live: the walk's live buffers
 * described as a snapshot -- dState the state buffer the walk runs in place on, the outcome arrays the record's, live->lists_in the set this tick reads as
 * "previous"; live->tick is not read.  Of refill only trials, dStartTick and dTrial are read.  CMPC_ERR_ARG: the new refusals above, a NULL live or refill
 * or a NULL required array in them, horizon, batch or max_contacts < 1, tick < 0, trials < 0, live->lists_in not 0 or 1. */
int cmpc_rollout_refill_restore(int horizon, int batch, int max_contacts, int tick, const cmpc_walk_snapshot* live, const cmpc_walk_refill* refill,
                                const cmpc_walk_refill_snapshot* from);
/* ---- the refill walk taped, and its tape regrouped by trial (DESIGN.md 7f "Refill, taped") ----
 * cmpc_rollout_walk_refill_trials_device with a row of a device tape behind every tick: behind each tick's record launch come part 2 of
 * cmpc_rollout_tape_device -- the copy kernel -- and the multiplier call, SEVEN launches a tick.  Tick tick0 + i writes tape row tape_row0 + i, SLOT-major:
 * column b of a row holds whatever trial sat in slot b at that tick.  Part 1 is never queued: the state a spawned trial starts from is refill->dState0[q],
 * and the regroup below supplies it (dStates[0] of a tape that starts at tape_row0 == 0 is left as allocated).  io->tick.dOk and the planner's times are
 * taped on every tick: every tick is queued as a merge tick.  Every output of the trials call is bit-identical; tape == NULL: the trials call itself.
 * No existing kernel changes, and there is no snapshot variant: trials that start from a pool stay untaped.
 * CMPC_ERR_ARG before anything is queued: what the trials call refuses without a handle, in its order; then an incomplete tape, a tape with too few rows
 * (tape_row0 < 0 or tape_row0 + ticks > tape->rows), tape scalars that disagree with io (plant_step, plant_substeps, force_sample_time); then a NULL
 * handle; the multiplier output off (cmpc_set_multiplier_output before the walk); and the rest of what the trials call refuses. */
int cmpc_rollout_walk_refill_taped_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                          const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, int row0, int lists_in, int* lists_out,
                                          const cmpc_walk_tape* tape, int tape_row0, void* stream);
/* Regroup by trial: a tape row does not need to know its trial -- the refill launch records, per trial, the slot, the start tick, the ticks recorded and
 * the local end tick, and that is enough to gather a trial's rows out of the slot-major tape.  ONE launch copies up to B trials into a tape `dst` of
 * refill->trial_ticks rows of B columns whose row r is the trial's LOCAL tick r and whose row 0 is a cold first tick (dst->first_row_is_first_tick = 1, the
 * caller's to set, like its other scalars): a taped walk of its own, on which cmpc_rollout_walk_vjp[_mismatch]_device and cmpc_rollout_walk_jvp[_mismatch]_device
 * run unchanged with tick0 = 0 and dEndTick = dEndOut.  The refill's archive pass (cmpc_rollout_refill_device with dStateLive == NULL) must have run behind
 * the walk's last tick.  sizeof(cmpc_walk_tape_regroup) == 32 (LP64; the ctypes mirror is held to it).
 * The rule for destination column j with trial q = dTrialIndex[j], s = dTrialSlot[q], t0 = dTrialStart[q] - tick_first, n = dTrialTicks[q],
 * e = dTrialEndTick[q]; every choice is a select, and repeated indices are allowed:
 *   - a started trial (n >= 1): destination row r (0 <= r < trial_ticks) takes the bit copy of source row t0 + min(r, n - 1), column s, of dX, dP, dLamG,
 *     dInfo, dOk, dLand, dListT, dListN, dPlanT and dPlanN; the rows past the trial's last recorded one repeat that row (what a walk of its own that
 *     takes ended problems out of its launches holds there).  Row 0's dPlanT and dPlanN are written zero: a first tick of a walk of its own leaves them as
 *     allocated, and the reverse never reads them.  States: dst.dStates[0][j] = dState0[q], dst.dStates[r + 1][j] = src.dStates[t0 + min(r, n - 1) + 1][s].
 *     dEndOut[j] = e if e >= 0; else n if n < trial_ticks -- the walk's end cut the trial off: its good ticks are i < n and its states 0 .. n exist, the
 *     convention of cmpc_rollout_walk_vjp_device; else -1.  dOkOut[j] = 1.
 *   - a trial never started (n == 0, slot -1): dStates[0][j] = dState0[q], dEndOut[j] = 0, dOkOut[j] = 1; nothing else is written.
 *   - no trial for the column -- an index outside [0, refill->trials), a slot outside the batch, or a needed source row outside [0, src->rows):
 *     dEndOut[j] = 0, dOkOut[j] = 0; nothing else is written.  The walks' gates select and never multiply, so the unwritten rows of a column whose end
 *     tick is 0 cannot reach a result.
 * The rule is one function shared by the kernel and the host form.  The kernel: one workgroup per (destination row, destination column); the four trial
 * words are read once per workgroup; rows of 64 words and more go as 16-byte pieces aligned on the destination with single-word heads and tails (n_x, n_p
 * and n_g are not multiples of four at every N), the scheme of cmpc_rollout_snapshot_device; no LDS, no barrier, no atomics.  Pure bandwidth: about 12 KB
 * in and out per trial-tick at N = 20.
 * CMPC_ERR_ARG before anything is queued, the checks that need no handle first (they are the host form's too): a NULL argument or required array
 * (dTrialIndex, dEndOut; with trials > 0 dState0, dTrialSlot, dTrialStart, dTrialTicks, dTrialEndTick); incomplete tapes; dst->rows != refill->trial_ticks;
 * refill->trials < 0; a destination array that is also a source array; max_contacts < 1.  Then a NULL handle, and more than 65535 rows. */
typedef struct cmpc_walk_tape_regroup {
    int tick_first;                 /* the tick number source row 0 holds */
    const int* dTrialIndex;         /* [B] the trial of destination column j; outside [0, trials): none */
    int* dEndOut;                   /* [B] the end tick the reverse / forward walk is to be given */
    int* dOkOut;                    /* [B] or NULL: 1 / 0 */
} cmpc_walk_tape_regroup;
int cmpc_rollout_tape_regroup_device(cmpc_handle h, int max_contacts, const cmpc_walk_tape* src, const cmpc_walk_refill* refill,
                                     const cmpc_walk_tape_regroup* g, const cmpc_walk_tape* dst, void* stream);
/* the same on the host: host buffers throughout (refill's and g's arrays too); no handle, no GPU.  Bit-equal to the kernel. */
int cmpc_rollout_tape_regroup(int horizon, int batch, int max_contacts, const cmpc_walk_tape* src, const cmpc_walk_refill* refill,
                              const cmpc_walk_tape_regroup* g, const cmpc_walk_tape* dst);
/* ---- the refill walk with a footstep plan and reference trajectories per TRIAL (DESIGN.md 7f "Refill, plans per trial") ----
 * Which slot a trial lands in depends on who ended before it, so the planner's lists of a SLOT are nothing a study can choose.  Here every trial names a
 * row of a POOL of plans, and the row is copied into the slot's rows when the trial is spawned.  Device arrays all.  sizeof == 104 (LP64; the ctypes
 * mirror is held to it).
 *   pool:  dPoolT[Pn][2][M][2] double, dPoolPose[Pn][2][M][7] float, dPoolN[Pn][2] int in the layout of the planner's lists (M = max_contacts), Pn =
 *     pool_plans >= 1; optional dPoolCom / dPoolH[Pn][plan_knots][3] float, both or neither: the planner's trajectories of each plan, with io->tick's
 *     plan_knots, plan_dt, robot_mass, com_height and io->plan_t_first (they need io->tick.dPlanCom / dPlanH).
 *   index: dTrialPlan[Q] the pool row of each trial (repeats are the normal case); dTrialPlanOk[Q] or NULL: 1 / 0 written when the trial is spawned,
 *     untouched for a trial never started.
 *   views: dPlanT, dPlanPose, dPlanN (and dPlanCom, dPlanH with pool trajectories; not read without) are the slots' rows the walk reads through
 *     io->tick's const pointers -- the SAME addresses: the struct only lifts the const. */
typedef struct cmpc_walk_refill_plans {
    int pool_plans;
    const double* dPoolT; const float* dPoolPose; const int* dPoolN;
    const float* dPoolCom; const float* dPoolH;
    const int* dTrialPlan; int* dTrialPlanOk;
    double* dPlanT; float* dPlanPose; int* dPlanN; float* dPlanCom; float* dPlanH;
} cmpc_walk_refill_plans;
/* cmpc_rollout_walk_refill_taped_device with `plans`.  plans == NULL: that call, bit for bit; with tape == NULL as well,
 * cmpc_rollout_walk_refill_trials_device.  Otherwise a tick gains ONE launch, the plan select (cmpc_refill_plans_kernel), directly behind the refill
 * launch: six launches a tick, eight when taped.  One workgroup per slot; the gate is workgroup-uniform and comes ahead of everything: a slot that was not
 * spawned this tick (dStartTick[b] != tick, or no trial in it) costs its workgroup that load.  A spawned slot with trial q receives the bit copy of pool row
 * dTrialPlan[q]: its rows of the three list arrays (8 M, 14 M and 2 words) and, with pool trajectories, its 3 plan_knots words of each, through
 * cmpc_rollout_snapshot_device's row copy (rows of 64 words and more in 16-byte pieces aligned on the destination); dTrialPlanOk[q] = 1.  No LDS, no
 * barrier, no atomics.  The front kernel of the same tick then reads the slot's rows as it always has, and so does every later tick of the trial and the
 * tape's copy kernel: no existing kernel changes.
 *   - An index outside [0, pool_plans): nothing is copied, dTrialPlanOk[q] = 0, rec->dEndTick[b] = 0 and dEndCode[b] = 0 -- the slot is behind the ended
 *     mask for this tick's other launches, is archived and freed by the next refill, and takes the next trial at the next tick (the rule of a snapshot
 *     index outside its pool).
 *   - A pool row is copied as it is: what the front kernel makes of a count outside 0 .. M, or of a snap that fails, is what it makes of it in a walk of
 *     its own.
 *   - AFTER THE CALL THE SLOTS' ROWS HOLD EACH SLOT'S LAST TRIAL'S PLAN.
 * A trial's outcome, trace rows, dX, dP, dInfo, state and the entries in use of its lists are those of cmpc_rollout_walk_mismatch_device(cold_first = 1,
 * tick_first = 0) on a handle of the same batch size, factor storage and options that holds it in the same slot, when that slot's planner lists (and
 * trajectory rows) are the trial's pool row, cmpc_set_models_device's row `slot` the trial's model and the schedules' column `slot` the trial's rows.
 * On the tape every tick's planner times and counts are the trial's own, so the regroup and the reverse / forward walks run unchanged, and a trial's
 * dGradPlan is the gradient with respect to ITS plan row (not to "the slot's lists"); cmpc_rollout_plan_fold_device sums it over the trials of a row.
 * CMPC_ERR_ARG before anything is queued: everything cmpc_rollout_walk_refill_taped_device refuses, in its order; and with plans != NULL, ahead of the
 * handle check: pool_plans < 1; a NULL pool list array; dTrialPlan NULL with refill->trials > 0; one of dPoolCom / dPoolH without the other, or pool
 * trajectories without io->tick.dPlanCom / dPlanH; a writable view that is not io's pointer; a pool array that is also a live array (a view, or a list
 * buffer of either set).  Plans together with a snapshot pool are refused: no entry point takes both.
 * Out of scope: per-trial plans for trials from a snapshot (a replan of a walk in progress); a replan inside a refill walk; orientation and
 * reference-trajectory gradients of a refill walk; per-trial extremes and per-trial limits; an autograd wrapper; lists longer than 16 contacts. */
int cmpc_rollout_walk_refill_plans_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                          const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, const cmpc_walk_refill_plans* plans,
                                          int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream);
/* The plan select launch of tick `tick` on the host: host buffers throughout; no handle, no GPU.  Bit-equal to the kernel.  Of refill only trials,
 * dStartTick and dTrial are read, of rec only dEndTick and dEndCode; there is no io, so the views are taken as given (non-NULL) and plan_knots -- read
 * with pool trajectories only -- is an argument.  CMPC_ERR_ARG: the refusals above that need no io, a NULL argument or required array, batch or
 * max_contacts < 1, tick < 0, trials < 0, pool trajectories with plan_knots < 1. */
int cmpc_rollout_refill_plans(int batch, int max_contacts, int tick, const cmpc_walk_refill* refill, const cmpc_walk_refill_plans* plans,
                              const cmpc_walk_record* rec, int plan_knots);
/* The pool's gradient: dOut[p][w] = the sum of dPerTrial[q][w] over the trials with dIndex[q] == p, from +0.0 and in ASCENDING q; dOut[pool_rows][words]
 * double is written whole, zero where no trial has the row.  A member is selected, never multiplied in: NaN in a trial that is not a member cannot reach
 * the row, and an index outside [0, pool_rows) contributes nowhere.  One thread per entry of dOut walks the queue; no atomics -- the order is fixed, so the
 * bits do not depend on scheduling (an index_add_ on the device is an atomic sum).  For a plan pool: words = 6 M, dPerTrial = a trial's dGradPlan + its
 * first-tick list gradient, dIndex = dTrialPlan.
 * CMPC_ERR_ARG: trials < 0, words < 1, pool_rows < 1, more than 2^31 - 1 entries, a NULL dOut, a NULL dIndex or dPerTrial with trials > 0, dOut ==
 * dPerTrial; then a NULL handle. */
int cmpc_rollout_plan_fold_device(cmpc_handle h, int trials, int words, const int* dIndex, const double* dPerTrial, int pool_rows, double* dOut, void* stream);
/* the same on the host: host buffers; no handle, no GPU.  Bit-equal to the kernel (one function forms an entry in both). */
int cmpc_rollout_plan_fold(int trials, int words, const int* index, const double* per_trial, int pool_rows, double* out);
/* The reverse walk: `ticks` calls of cmpc_rollout_tick_vjp_device (called, not copied: its workspace, statuses and zero rule for flagged problems hold),
 * last row first, on one stream, with one gate launch between the ticks (ticks + 1 launches of cmpc_walk_vjp_gate_kernel).  Tick number tick0 + i is row
 * row0 + i of the tape and of every [rows] array below, now = (tick0 + i) * sampling_time.
 * The fields of cmpc_walk_grads, device pointers all:
 *     dGradStates[rows + 1][B][9] double   in: the seeds G on the states (row r: the state tick r started from)
 *     dGradX[rows][B][n_x] float or NULL   in: the seeds GX on the solutions
 *     dCarryState[B][9] double             in: the carry entering the last row of the call; out: the carry leaving its first row
 *     dCarryList[B][2][M][3] double        the same for the lists' positions
 *     dGradWrench[rows][B][N][6] float or NULL, dGradP[rows][B][n_p] float or NULL   out, per row
 *     dGradPlan[B][2][M][3] double or NULL, dGradModel[B][34] double or NULL        out, +=
 *     dStatus[rows][B] int                 out: word 0 of the tick's dTickSens, or 6: the problem had ended
 * A walk is reversed in segments through the two carry buffers (a replanned walk may pass a different dGradPlan per segment).  A call over the whole walk
 * with dCarryState = dGradStates[rows] and dCarryList = 0 leaves dl/dstate_0 and dl/dlist_0 in them.
 * Ended problems (dEndTick[B] in the convention of cmpc_walk_record, tick numbers; NULL: none).  Let e = dEndTick[b], -1 read as never.  The good ticks are
 * i < e; the states s_0 .. s_e exist (s_e = dFinalState); the loss is sum_{i <= e} <G_i, s_i> + sum_{i < e} <GX_i, x_i>, and seeds of rows past e are not read
 * for that problem.  Carry: c_i = [i < e] J_i^T c_{i+1} + [i <= e] G_i.  For a tick i >= e the gate feeds the tick VJP a zero state carry, a zero list carry,
 * a zero dGradX row and dOk = 0 (gated copies in handle workspace; the tick then flags the problem -- its status 5 -- and adds nothing to the += outputs), and
 * behind the tick it SELECTS zero for the carries, the wrench row and the dGradP row and writes dStatus = 6: it selects and does not multiply, so stale or
 * non-finite data of an ended problem cannot leak.  For i < e the gate's add is carry = the tick's dGradState + G_i in double.  The rule is one
 * __host__ __device__ function (cmpc_walk_gate_problem / cmpc_walk_gate_wide); the gate has no barrier and no atomics; lanes past B do nothing.
 * No host wait beyond the first call's workspace allocation (4 n_x + 96 M + 108 bytes per problem: the tick's dGradState, dGradPrevList and -- for the
 * orientation entry below, sized for it whichever entry runs first -- dGradPrevListRot, the gated dGradX row and dOk, the tick's dTickSens; grown when a larger
 * max_contacts arrives, and that call waits for the device); calls on one handle run one after the other whatever their streams (the tick VJP's event). */
typedef struct cmpc_walk_grads {
    const double* dGradStates; const float* dGradX;
    double* dCarryState; double* dCarryList;
    float* dGradWrench; float* dGradP; double* dGradPlan; double* dGradModel;
    int* dStatus;
} cmpc_walk_grads;
int cmpc_rollout_walk_vjp_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                 const cmpc_walk_grads* g, void* stream);
/* One gate step on the host (host buffers; no handle, no GPU; bit-equal to the kernel): the POST part finishes tick `tick_post` from what the tick VJP left
 * (tick_state[B][9], tick_list[B][2][M][3], tick_sens[B][CMPC_SENS]) and the seed row seed_state[B][9] into carry_state / carry_list, and selects zero in
 * wrench_row[B][N][6] / grad_p_row[B][n_p] (either may be NULL) and writes status_row[B]; the PRE part prepares tick `tick_pre`: ok_out[B] from ok_row (NULL:
 * ones), grad_x_out[B][n_x] from grad_x_row (both NULL: none), and with first != 0 (the first step of a call) zero is selected in the caller's carries too.
 * A step between two reverse ticks has both parts (tick_pre = tick_post - 1); the first step of a call has PRE only, the last POST only. */
typedef struct cmpc_walk_gate {
    int batch, max_contacts, horizon;
    const int* end_tick;
    int do_post, tick_post;
    const double* seed_state; const double* tick_state; const double* tick_list; const float* tick_sens;
    double* carry_state; double* carry_list; float* wrench_row; float* grad_p_row; int* status_row;
    int do_pre, tick_pre, first;
    const int* ok_row; const float* grad_x_row; int* ok_out; float* grad_x_out;
} cmpc_walk_gate;
int cmpc_rollout_walk_vjp_gate(const cmpc_walk_gate* g);
/* the same step as ONE launch of the gate kernel, device pointers throughout (batch and horizon the handle's): what cmpc_rollout_walk_vjp_device queues
 * between its ticks, for a caller who reverses a walk tick by tick.  Asynchronous on `stream` (NULL: the handle's); it takes no part in the tick VJP's event. */
int cmpc_rollout_walk_vjp_gate_device(cmpc_handle h, const cmpc_walk_gate* g, void* stream);
/* The reverse walk with the contacts' ORIENTATIONS carried along (body-frame tangents, as cmpc_rollout_tick_vjp_rot_device): the same loop -- one function
 * behind both entries -- with cmpc_rollout_tick_vjp_rot_device per row, so one launch more per tick, and still ticks + 1 gate launches.  Tape rows, the
 * `now` of a row and the first-tick rule of row 0 are the walk's above; nothing more is taped.  g as above; the fields of cmpc_walk_grads_rot, device
 * pointers all:
 *     dCarryListRot[B][2][M][3] double             in: the orientation carry entering the last row of the call; out: the one leaving its first row.  It is
 *                                                  the tick's dGradListRotOut; the tick's dGradPrevListRot is a second buffer of the walk's workspace
 *     dGradPlanRot[B][2][M][3] double or NULL      out, +=
 *     dGradRot[rows][B][2][N][3] double or NULL    out, per row: each tick's full per-stage dl/domega (NULL: the tick's own workspace)
 *     dRemoved[rows][B] float or NULL              out, per row: word 6 of the tick's dTickSens
 * Segments compose through three carries; a call over the whole walk with dCarryListRot = 0 leaves dl/d(orientations of the first tick's lists) in it.
 * Every output the entry above also has is bit-identical to it on the same tape and seeds (the tick's own guarantee).
 * Ended problems: the rule above, extended.  l_rot_i = [i < e] (the tick's dGradPrevListRot); row i of dGradRot is the tick's when i < e and zero
 * otherwise; dRemoved[i] is word 6 when i < e and 0 otherwise; nothing is added to dGradPlanRot for i >= e (the gated dOk = 0 makes the tick flag the
 * problem); the first gate step of a call also selects zero in the caller's dCarryListRot of an ended problem.  Each of these is a select, never a
 * multiply.  A problem that has not ended but whose tick is flagged passes zeros on, as the rotation tick VJP does.  The gate writes dGradRot only where
 * the problem has ended: the tick's bits of a walking problem are never touched.
 * CMPC_ERR_ARG: r == NULL, r->dCarryListRot == NULL, and everything cmpc_rollout_walk_vjp_device rejects. */
typedef struct cmpc_walk_grads_rot {
    double* dCarryListRot;
    double* dGradPlanRot;
    double* dGradRot;
    float* dRemoved;
} cmpc_walk_grads_rot;
int cmpc_rollout_walk_vjp_rot_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                     const cmpc_walk_grads* g, const cmpc_walk_grads_rot* r, void* stream);
/* One gate step with the orientation arrays, host form and one-launch device form as above.  base: the step above, unchanged -- its outputs are bit for bit
 * what cmpc_rollout_walk_vjp_gate writes for the same base.  POST: carry_list_rot[B][2][M][3] from tick_list_rot (the tick's dGradPrevListRot), zero
 * selected in rot_row[B][2][N][3] of an ended problem (may be NULL; a walking problem's row is not written), removed_row[B] (may be NULL) from tick_sens.
 * PRE with first != 0: zero selected in carry_list_rot of an ended problem.  The base's argument check, plus: carry_list_rot is required, and tick_list_rot
 * with do_post. */
typedef struct cmpc_walk_gate_rot {
    cmpc_walk_gate base;
    const double* tick_list_rot; double* carry_list_rot; double* rot_row; float* removed_row;
} cmpc_walk_gate_rot;
int cmpc_rollout_walk_vjp_rot_gate(const cmpc_walk_gate_rot* g);
int cmpc_rollout_walk_vjp_rot_gate_device(cmpc_handle h, const cmpc_walk_gate_rot* g, void* stream);

/* ---- the device walk FORWARDS on the same tape, k direction columns, per-problem endings kept (derivation and the rule: DESIGN.md 7f, "Forwards") ----
 * The forward walk: `ticks` calls of cmpc_rollout_tick_jvp_device (called, not copied: its chunks of eight columns, its workspace, its internal-force rule,
 * its statuses and its zero rule for flagged problems hold), first row first, on one stream, with one gate launch between the ticks (ticks + 1 launches of
 * cmpc_walk_jvp_gate_kernel).  Tick number tick0 + i is row row0 + i of the tape and of every [rows] array below, now = (tick0 + i) * sampling_time; each
 * row's cmpc_tick_tape is built as the reverse walk builds it (the previous lists are row - 1's, NULL on row 0 of a tape whose first row is a first tick).
 * The fields of cmpc_walk_dirs, device pointers all, the column axis right behind the batch axis:
 *     dDirStates[rows + 1][B][k][9] double    row row0 is read (t of the first tick of the call), rows row0 + 1 .. row0 + ticks are written
 *     dCarryList, dCarryListRot[B][k][2][M][3] double   in: the list directions entering the first row of the call; out: those leaving its last row,
 *                                             whatever the parity of `ticks` (the tick needs in != out: the walk alternates with a workspace buffer).
 *                                             dCarryListRot and dDirPlanRot both NULL: no rotation chain (the tick's NULL rule; results are then bit for
 *                                             bit those without it); dDirPlanRot without dCarryListRot is CMPC_ERR_ARG
 *     dDirPlan, dDirPlanRot[B][k][2][M][3] double or NULL   read by every merge tick of the call (a replanned walk passes other ones per segment)
 *     dDirWrench[rows][B][k][N][6] float or NULL, dDirModel[B][k][34] double or NULL, dDirP[rows][B][k][n_p] float or NULL (the tick's extra p direction)
 *     dDirX[rows][B][k][n_x] float or NULL    out: the solutions' directions
 *     dStatus[rows][B] int                    out: word 0 of the tick's dTickSens, or 6: the problem had ended
 *     dRemoved[rows][B] float or NULL         out: word 6 of the tick's dTickSens, 0 for an ended problem
 * Segments compose through dDirStates and the two carries: rows 8 .. 15 behind rows 0 .. 7 equal one call over 0 .. 15 to the bit.
 * Ended problems (dEndTick[B] as in the reverse walk; NULL: none).  Let e = dEndTick[b], -1 read as never; t_i is the direction of the state tick i starts
 * from, l_i that of the lists (positions and orientations).  The rule, the exact transpose of c_i = [i < e] J_i^T c_{i+1} + [i <= e] G_i:
 *     t_{i+1} = [i < e] (the tick's dDirStateOut), l_{i+1} = [i < e] (the tick's dDirList / dDirListRot);
 *     row i of dDirX is the tick's when i < e, zero otherwise; dStatus[i] is word 0 of dTickSens when i < e and 6 when i >= e; dRemoved[i] is word 6
 *     when i < e and 0 when i >= e.
 * The directions t_0 .. t_e exist; everything behind the end is zero.  For a tick i >= e the gate feeds the tick dOk = 0 (a gated copy in handle
 * workspace); the tick then flags the problem -- its status 5 -- and writes zeros, and behind the tick the gate still SELECTS zero for that problem in
 * every array the tick wrote for the row: it never multiplies, so stale or non-finite data of an ended problem -- in its tape rows, in its rows of the
 * caller's direction arrays, in what the tick left -- cannot leak.  The first gate step of a call also selects zero in dDirStates[row0] and in the
 * carries of a problem with e < tick0.  A problem that has not ended but whose tick is flagged (status 1 .. 5) passes zeros on, as the tick JVP does:
 * the transpose of the reverse walk there.  The rule is one __host__ __device__ function pair (cmpc_walk_jvp_gate_column / cmpc_walk_jvp_gate_wide); the
 * gate has no LDS, no barrier and no atomics; lanes past B k do nothing.
 * No host wait beyond the workspace allocation: per-handle HBM, 96 M bytes per problem and column (the second buffers of the two list directions) plus
 * 36 bytes per problem (dTickSens and the gated dOk), allocated on first use, grown when a larger k or max_contacts arrives (that call waits for the
 * device), freed with the handle; calls on one handle run one after the other whatever their streams (the tick VJP's event).
 * CMPC_ERR_ARG: a NULL handle, tape or d, k < 1, rows outside the tape, row 0 of a tape whose first row is not a first tick, dDirStates, dCarryList or
 * dStatus missing. */
typedef struct cmpc_walk_dirs {
    double* dDirStates;
    double* dCarryList; double* dCarryListRot;
    const double* dDirPlan; const double* dDirPlanRot;
    const float* dDirWrench; const double* dDirModel; const float* dDirP;
    float* dDirX; int* dStatus; float* dRemoved;
} cmpc_walk_dirs;
int cmpc_rollout_walk_jvp_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick, int k,
                                 const cmpc_walk_dirs* d, void* stream);
/* One gate step of the forward walk on the host (host buffers; no handle, no GPU; bit-equal to the kernel).  The POST part finishes tick `tick_post` IN
 * PLACE on what the tick JVP wrote -- state_out[B][k][9] (its dDirStateOut), list_out / list_rot_out[B][k][2][M][3] (list_rot_out may be NULL),
 * x_row[B][k][n_x] (may be NULL): zero is selected where the problem has ended -- and writes status_row[B] and removed_row[B] (may be NULL) from
 * tick_sens[B][CMPC_SENS].  The PRE part prepares tick `tick_pre`: ok_out[B] from ok_row (NULL: ones); with first != 0 (the first step of a call) zero is
 * selected in first_state[B][k][9], first_list and first_list_rot[B][k][2][M][3] (each may be NULL) of a problem that ended before tick_pre.  A step
 * between two forward ticks has both parts (tick_pre = tick_post + 1); the first step of a call has PRE only, the last POST only.  The two parts touch
 * disjoint arrays. */
typedef struct cmpc_walk_jvp_gate {
    int batch, max_contacts, horizon, k;
    const int* end_tick;
    int do_post, tick_post;
    const float* tick_sens;
    double* state_out; double* list_out; double* list_rot_out; float* x_row; int* status_row; float* removed_row;
    int do_pre, tick_pre, first;
    const int* ok_row; int* ok_out;
    double* first_state; double* first_list; double* first_list_rot;
} cmpc_walk_jvp_gate;
int cmpc_rollout_walk_jvp_gate(const cmpc_walk_jvp_gate* g);
/* the same step as ONE launch of the gate kernel, device pointers throughout (batch and horizon the handle's): what the forward walk queues between its
 * ticks.  Asynchronous on `stream` (NULL: the handle's); it takes no part in the tick VJP's event. */
int cmpc_rollout_walk_jvp_gate_device(cmpc_handle h, const cmpc_walk_jvp_gate* g, void* stream);

/* ---- the measures, differentiated: a loss on the stability measures of a taped walk, reverse and forward (derivation: DESIGN.md 7f, "Measures,
 * differentiated") ----
 * The four measures of "physical limits" above are a function of what a tick left: dStates[row + 1] (com, dcom), the knot-1 foot positions of dX, the
 * stage-1 rotations and the knot-1 comRef row of dP, and the model's corners.  Its derivative ignores the final rounding to float.  The independent
 * inputs per (row, problem) are CMPC_WALK_MEASURE_INPUTS = 44 numbers, in this order:
 *     com[3], dcom[3] (dcom_z has zero derivative), q_c[2][3], omega_c[2][3], corner[2][4][3], comRef_xy[2]
 * omega_c is the body-frame tangent of the stage-1 rotation, R <- R Exp(omega), the convention of every rotation gradient here; the margin reads rows 0
 * and 1 of R only.  Branches -- each a SELECT, never a multiply by zero, so that NaN in what a branch does not take cannot leak:
 *     height  d/dcom_z = 1, d/dq_c,z = -1/n for c in S
 *     reach   (com - q_c) / r of the foot the forward's `r > reach` chain keeps (the first foot wins a tie); zero when r == 0
 *     track   (com_xy - ref_xy) / track; zero when track == 0
 *     margin  the derivative of a smooth branch of the forward's own comparison chain: the same candidate order, the same strict <, the same
 *             length >= 1e-12 exclusions, the same arg-max or arg-min vertex (the first in index order), with the dependence of the unit normal on its
 *             two defining points, or on xi, included.  The branch is the chain's winner among the FACES of the region -- a pair whose extremal
 *             vertex lies on the pair's own line, a direction whose extremal vertex is its own point, both within 1e-9 m -- and not simply the
 *             chain's winner: the parallel sides of a rectangular sole alias each other (one normal, one value to rounding, the last bit decides
 *             which the forward keeps), and an alias equals the margin only while the sole stays a rectangle, so in the corners and in omega its
 *             gradient is no element of the generalised gradient.  The least over all directions is attained at a face, so that winner has the
 *             forward's value to rounding; with no face admitted the chain's own winner is taken.  No candidate left: 0.  A vertex the forward
 *             filled from the other foot (single support) sends
 *             its derivative to the foot and corner it was copied from: a foot outside S receives exactly zero.  xi = com_xy + dcom_xy tau, tau =
 *             sqrt(max(height, 0) / g): through tau the margin also depends on com_z and q_z, dtau/dheight = 1 / (2 g tau) when height > 0 and tau > 0,
 *             and 0 otherwise
 *     a measure the forward reports as NaN (S empty, a state that is not finite) has a zero row, and its cotangent is not read
 * The measures are piecewise smooth: at a tie between branches this is ONE element of the generalised gradient, the branch the forward's comparisons
 * pick.  Nothing is smoothed.
 *
 * cmpc_walk_measures_vjp_device: ONE launch over rows row0 .. row0 + ticks - 1 of the tape (tick numbers tick0 ..), one thread per (row, problem); no LDS,
 * no barrier, no atomics; lanes past ticks * B touch no memory.  It reads the tape's dX[r], dP[r], dStates[r + 1] and the corners the record launch reads
 * (the handle's, or the installed models').  The arrays of cmpc_walk_measure_grads are indexed by tape row, as those of cmpc_walk_grads:
 *     dGradMeasures[rows][B][4] double        in: the cotangents of height, reach, margin, track
 *     dGradStates[rows + 1][B][9] double      +=, row r + 1, entries 0..4 (com, dcom_xy); entries 5..8 are not touched: the seeds of the reverse walk
 *     dGradX[rows][B][n_x] float              +=, the six knot-1 foot positions only; each term formed in double, rounded once, then one float add
 *     dDirect[rows][B][CMPC_WALK_MEASURE_DIRECT = 32] double   written whole: comRef_xy (2), omega [2][3], corner [2][4][3] -- what no seed of the
 *                                             reverse walk carries
 * A term that is exactly zero is not added to a += entry (the entry keeps its bits), so a zero cotangent leaves the seeds as they were to the bit.
 * Endings, the reverse walk's convention: with e = dEndTick[b] (NULL or -1: never), the rows with tick0 + r < e count.  Row e itself -- the measure that
 * fired -- and every later row select zero in dDirect and leave the += entries unwritten; nothing of such a row is read, so NaN there cannot leak.
 * cmpc_walk_measures_vjp_fold_device: one small launch for behind the reverse walk, over `rows` rows from the pointers given.  It adds dDirect's comRef
 * pair to the knot-1 comRef xy of dGradP[rows][B][n_p] float (rounded once; a zero term is not added), so that
 * cmpc_reference_from_planner_vjp_device carries it to the planner's trajectories, and it sums dDirect's corner words over the rows, in ascending row
 * order, into dGradModel[B][10..33] (one thread per problem and word, no atomics).  Either output may be NULL.
 * cmpc_walk_measures_jvp_device: the transpose, k columns, in cmpc_walk_dirs' layouts, indexed by tape row, so the forward walk's outputs feed it:
 *     dDirStates[rows + 1][B][k][9] double, dDirX[rows][B][k][n_x] float, dDirP[rows][B][k][n_p] float or NULL (its knot-1 comRef xy only),
 *     dDirModel[B][k][34] double or NULL (its corners only)  ->  dDirMeasures[rows][B][k][4] double; rows at or past e select zero
 * One thread per (row, problem) forms the partials once and contracts the k columns.
 * Host forms, no handle and no GPU, bit-equal to the kernels: the arrays start at the first row of the call (X[rows][B][n_x], P[rows][B][n_p],
 * states[rows + 1][B][9], and the gradient / direction arrays likewise); corners [2][4][3] float of problem 0 with problem b's corners_stride floats
 * further on (0: one set for the batch), gravity > 0, as cmpc_rollout_record_limits.  cmpc_walk_measures_jacobian: the dense [rows][B][4][44], every
 * row counted, host only (for tests; the kernels never form it).
 * CMPC_ERR_ARG: a NULL required pointer, rows outside the tape (rows < 1 on the host), k < 1, horizon < 2.
 * Out of scope: chaining the omega term of dDirect into the lists' or the planner's orientations (the tick VJP has no per-stage rotation seed: the term
 * is returned and not carried); checkpointed reverse walks; per-trial corners of a regrouped refill tape (the corners are the handle's or the installed
 * models'); derivatives of dExtremes; any smoothing of the min / max. */
#define CMPC_WALK_MEASURE_INPUTS 44
#define CMPC_WALK_MEASURE_DIRECT 32
typedef struct cmpc_walk_measure_grads {
    const double* dGradMeasures;
    double* dGradStates; float* dGradX;
    double* dDirect;
} cmpc_walk_measure_grads;
typedef struct cmpc_walk_measure_dirs {
    const double* dDirStates; const float* dDirX; const float* dDirP; const double* dDirModel;
    double* dDirMeasures;
} cmpc_walk_measure_dirs;
int cmpc_walk_measures_vjp_device(cmpc_handle h, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                  const cmpc_walk_measure_grads* g, void* stream);
int cmpc_walk_measures_vjp_fold_device(cmpc_handle h, int rows, const double* dDirect, float* dGradP, double* dGradModel, void* stream);
int cmpc_walk_measures_jvp_device(cmpc_handle h, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick, int k,
                                  const cmpc_walk_measure_dirs* d, void* stream);
int cmpc_walk_measures_vjp(int horizon, int batch, int tick0, int rows, const float* X, const float* P, const float* states, const int* end_tick,
                           const float* corners, int corners_stride, double gravity, const double* grad_measures, double* grad_states, float* grad_X,
                           double* direct);
int cmpc_walk_measures_vjp_fold(int horizon, int batch, int rows, const double* direct, float* grad_P, double* grad_model);
int cmpc_walk_measures_jvp(int horizon, int batch, int tick0, int rows, int k, const float* X, const float* P, const float* states, const int* end_tick,
                           const float* corners, int corners_stride, double gravity, const double* dir_states, const float* dir_X, const float* dir_P,
                           const double* dir_model, double* dir_measures);
int cmpc_walk_measures_jacobian(int horizon, int batch, int rows, const float* X, const float* P, const float* states, const float* corners,
                                int corners_stride, double gravity, double* jacobian);

/* ---- plant-model mismatch on the device walk: hidden pushes, sensor noise, force gain (derivation: DESIGN.md 7f, "Mismatch") ----
 * In every entry point above the plant IS the model: the wrench the plant integrates is the knot-0 wrench rows of dP, which setState handed to the MPC; the
 * MPC measures the plant's exact state; the plant applies exactly the forces the MPC asked for.  The reference has the split this section adds:
 * CentroidalMPCBlock receives input.totalExternalWrench, an ESTIMATE, while the simulator applies the true one.  Nothing in the solver kernel changes.
 * Per problem, at tick number t, row r = t - tick_first of the two schedules (device pointers; a problem's results depend on its own rows only):
 *   hidden wrench (0 <= r < hidden_ticks): the plant uses a = (F + fExt_0) + fHidden - g e_z and tau0 = (tauExt_0 + tauHidden) + sum_q cp_q x f_q, in double
 *     from the float values, in that order (the mismatch-free expression keeps its bits).  Nothing of it is written to dP: the MPC never sees it.  Outside
 *     the range the term is NOT ADDED -- a select, not an add of zero.
 *   state noise (0 <= r < noise_ticks): the front kernel writes com0 / dcom0 / h0 = state[e] + noise[r][b][e], ONE float32 add; the plant integrates from the
 *     true state (dState / dStateOut, unchanged).  Outside the range it is a plain copy.
 *   force gain: cf = on ? (double)gain * (double)f : 0 for every corner force -- fsum, tau0 and the ZMP's F, T all use the applied force, so the 0.001
 *     thresholds see it.  A mass error is gain = m_nominal / m_true.  No device-side validation: a NaN or non-positive gain gives what the arithmetic gives, and
 *     the record ends the problem by code 5 if the state goes non-finite.
 * sizeof(cmpc_plant_mismatch) == 48 (LP64; the ctypes mirror is held to this number). */
typedef struct cmpc_plant_mismatch {
    int tick_first;                                /* tick number of row 0 of the two schedules */
    const float* dHiddenWrench; int hidden_ticks;  /* [hidden_ticks][B][6] mass-normalised force | torque about the CoM, or NULL */
    const float* dStateNoise;   int noise_ticks;   /* [noise_ticks][B][9] added to the MEASURED com, dcom, h, or NULL */
    const float* dForceGain;                       /* [B] or NULL (1): the plant applies gain * f to every corner force */
} cmpc_plant_mismatch;
/* cmpc_plant_step_device with one tick's hidden-wrench row dHiddenWrench[B][6] (or NULL) and dForceGain[B] (or NULL).  Both NULL: cmpc_plant_step_device bit
 * for bit (it calls this with NULL, and the kernel then is the instantiation without the mismatch); gain = 1 and a zero wrench give the same bits too, on
 * inputs without negative zeros in the wrench sums. */
int cmpc_plant_step_mismatch_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, float* dStateOut, float* dZmp, double step,
                                    int substeps, double zmp_half_x, double zmp_half_y, const float* dHiddenWrench, const float* dForceGain, void* stream);
/* cmpc_rollout_tick_device with the explicit tick number that selects the rows of m.  Still three launches: the noise add lives in the front kernel's setState
 * loop, the hidden wrench and the gain in the back kernel's plant step.  m == NULL: cmpc_rollout_tick_device, bit for bit (`tick` is then not looked at).
 * CMPC_ERR_ARG, besides cmpc_rollout_tick_device's: a negative count, a non-NULL schedule with a zero count, tick < 0. */
int cmpc_rollout_tick_mismatch_device(cmpc_handle h, int max_contacts, double now, int warm, const cmpc_tick_io* io, int tick, const cmpc_plant_mismatch* m,
                                      void* stream);
/* The recorded walk (tape == NULL: cmpc_rollout_walk_device) or the taped walk (cmpc_rollout_walk_taped_device) with each tick passing its own number
 * tick0 + i to the tick above.  No launch is added per tick and nothing more is taped: dStates already holds the true state and dP the measured one.
 * cmpc_set_ended_device, stop_mask, dWrenchTicks and the planner references compose with it unchanged.  m == NULL: the existing entry point, bit for bit.
 * CMPC_ERR_ARG as the two walks', and the mismatch's above. */
int cmpc_rollout_walk_mismatch_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                      int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, const cmpc_plant_mismatch* m,
                                      void* stream);
/* Reverse.  The plant's closed form holds with f_q -> gain f_q and fExt_0 -> fExt_0 + fHidden (the same for the torque), so the partials are those of
 * "plant-step derivatives" taken at the gained forces and the summed wrench; the VJPs above on a mismatch tape would be silently wrong.
 * cmpc_plant_step_vjp_rot_device's arguments (dGradRot0 may be NULL) plus the inputs dHiddenWrench[B][6] / dForceGain[B] (either NULL as in the forward) and
 * the outputs dGradHidden[B][6] double = the plant's own gradient on fExt_0 / tauExt_0 (unrounded) and dGradGain[B] double = sum_q <dl/d(gain f_q), f_q> over
 * the gated-on corners in corner order, both WRITTEN, either may be NULL; dGradX on the 24 forces is gain * dl/d(gain f).  With both inputs NULL the outputs
 * shared with cmpc_plant_step_vjp_rot_device are bit-equal to it. */
int cmpc_plant_step_vjp_mismatch_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps,
                                        const double* dGradStateOut, double* dGradState, float* dGradX, float* dGradP, double* dGradModel, double* dGradRot0,
                                        const float* dHiddenWrench, const float* dForceGain, double* dGradHidden, double* dGradGain, void* stream);
/* One tick in reverse under a mismatch: cmpc_rollout_tick_vjp_rot_device's arguments (dGradPrevListRot == NULL: the chain without orientations, as
 * cmpc_rollout_tick_vjp_device), the tick's own rows dHiddenWrench[B][6] / dForceGain[B] (either NULL: not applied in the forward), and three outputs, each
 * may be NULL: dGradHidden[B][6] double, written; dGradNoise[B][9] float, written: the solve VJP's dGradP on com0 / dcom0 / h0, the part of dGradState that
 * arrived through setState; dGradGain[B] double, += (one thread per problem, no atomics).  tape->dState is the TRUE state the tick started from, tape->dP the
 * parameters the solve saw (the measured state in them).  A flagged problem (status != 0) gets explicit zeros in the first two and adds nothing to the third,
 * written by the branch of the combine kernel that zeroes everything else.  With both inputs NULL every output the existing entries have is bit-identical to
 * theirs.  Workspace: the tick VJP's, which holds 56 bytes per problem for this entry. */
int cmpc_rollout_tick_vjp_mismatch_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, const double* dGradStateOut,
                                          const double* dGradListOut, const float* dGradX, double* dGradState, double* dGradPrevList, float* dGradWrench,
                                          double* dGradPlan, double* dGradModel, float* dGradP, float* dTickSens, const double* dGradListRotOut,
                                          double* dGradPrevListRot, double* dGradPlanRot, double* dGradRot, const float* dHiddenWrench, const float* dForceGain,
                                          double* dGradHidden, float* dGradNoise, double* dGradGain, void* stream);
/* The reverse walk under a mismatch: the same loop as cmpc_rollout_walk_vjp[_rot]_device -- ONE function behind all three entries -- with the tick above per
 * row; r may be NULL (no orientation chain), m is the walk's mismatch (NULL: none was applied; the gradient rows are still written), mg may be NULL.  Each
 * pointer of mg may be NULL; rows are the tape's rows, as dGradWrench's.
 * Ended problems: the gate structs and the gate kernel are NOT changed.  For ticks i >= e of an ended problem the gate already feeds the tick dOk = 0; the
 * tick then flags the problem and writes zeros in its dGradHidden / dGradNoise rows and adds nothing to dGradGain -- the endings are kept by selection, with no
 * new gate work, and stale or non-finite data behind an end cannot leak.
 * Rows whose tick lies outside a schedule's range still get their gradient row: dGradHidden there is the gradient with respect to a wrench that was zero (not
 * added), dGradNoise with respect to a noise that was zero.  Forward mode under a mismatch is the section below; the checkpointed reverse is this entry
 * run segment by segment (segments compose to the bit: dGradGain accumulates in the full walk's order when they are reversed last first). */
typedef struct cmpc_walk_grads_mismatch {
    double* dGradHidden;   /* [rows][B][6], written per row */
    float* dGradNoise;     /* [rows][B][9], written per row */
    double* dGradGain;     /* [B], += */
} cmpc_walk_grads_mismatch;
int cmpc_rollout_walk_vjp_mismatch_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                          const cmpc_walk_grads* g, const cmpc_walk_grads_rot* r, const cmpc_plant_mismatch* m,
                                          const cmpc_walk_grads_mismatch* mg, void* stream);

/* ---- the mismatch FORWARDS, in k directions (derivation: DESIGN.md 7f, "Mismatch, forwards") ----
 * The transposes of the three reverse entries above, column for column.  On a mismatch tape the entries of "the roll-out tick FORWARDS" take the plant's
 * partials at the MPC's forces and the MPC's wrench and would be silently wrong; these take them at the gained forces and the summed wrench.
 *
 * The plant: cmpc_plant_step_jvp_cols_device's arguments plus the inputs dHiddenWrench[B][6] / dForceGain[B] float (either NULL as in the forward) and the
 * directions dDirHidden[B][k][6] / dDirGain[B][k] double (either NULL: zero).  With cf_q = gain f_q on gated-on corners:
 *     d cf_q = dgain f_q + gain df_q,   dF = sum_q d cf_q,   da = dF + dfExt_0 + dfHidden,   dtau = dtauExt_0 + dtauHidden + sum_q (dcp_q x cf_q + cp_q x d cf_q)
 * and the three output rows of the plant JVP unchanged -- cmpc_plant_step_vjp_mismatch_device transposed term by term.  With the four new pointers NULL it is
 * cmpc_plant_step_jvp_cols_device bit for bit (the same kernel instantiation); column j is bit-equal to a k = 1 call on column j alone. */
int cmpc_plant_step_jvp_mismatch_cols_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, int k,
                                             const double* dDirState, const float* dDirX, const float* dDirP, const double* dDirModel, const double* dDirRot0,
                                             const float* dHiddenWrench, const float* dForceGain, const double* dDirHidden, const double* dDirGain,
                                             double* dDirStateOut, void* stream);
/* One tick forwards under a mismatch: cmpc_rollout_tick_jvp_device's arguments, the tick's own rows dHiddenWrench[B][6] / dForceGain[B] (either NULL: not
 * applied in the forward) and the mismatch directions, each may be NULL (zero; md itself may be NULL).  Two differences from that entry:
 *   the noise direction enters the SOLVE only: the assembled p direction holds (float)dDirState[e] + dDirNoise[e] on com0 / dcom0 / h0, ONE float32 add as in
 *     the forward's setState (the transpose of "dGradNoise = the solve VJP's dGradP on those rows").  The plant still receives dDirState alone, in double: it
 *     integrates from the true state.
 *   the plant launch is the mismatched instantiation, at the tick's hidden row and gain, with dDirHidden / dDirGain.
 * A flagged problem gets zeros in every output, by the flags and the plant kernel's ok branch of the entry above.  With dHiddenWrench, dForceGain and md all
 * NULL (or md without a pointer set) it is cmpc_rollout_tick_jvp_device bit for bit (which calls the same function that way).  No workspace beyond that entry's.
 * sizeof(cmpc_tick_dirs_mismatch) == 24 (LP64; the ctypes mirror is held to this number). */
typedef struct cmpc_tick_dirs_mismatch {
    const double* dDirHidden;   /* [B][k][6] */
    const float* dDirNoise;     /* [B][k][9] */
    const double* dDirGain;     /* [B][k] */
} cmpc_tick_dirs_mismatch;
int cmpc_rollout_tick_jvp_mismatch_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, int k, const cmpc_tick_dirs* in,
                                          const cmpc_tick_dirs_out* out, float* dTickSens, const float* dHiddenWrench, const float* dForceGain,
                                          const cmpc_tick_dirs_mismatch* md, void* stream);
/* The forward walk under a mismatch: the same loop as cmpc_rollout_walk_jvp_device -- ONE function behind both entries -- with the tick above per row.  m is
 * the walk's mismatch (NULL: none was applied; the directions still are), md may be NULL and so may each of its pointers.  Tick tick0 + i takes its hidden row
 * by TICK NUMBER (m->tick_first) and its direction rows by TAPE ROW, the two indices of the reverse walk.  A tick outside the hidden schedule runs the
 * partials without the hidden term (a select, as in the forward) and still applies dDirHidden: the map is linear in a wrench that was zero.  A tick with
 * no hidden row, no gain and no direction pointer is the plain tick, by the rule of the entry above.
 * The gate structs, the gate kernel and the host gate are NOT changed: the mismatch directions are inputs only, and for a tick at or behind a problem's end
 * the gate already feeds the tick dOk = 0, which then writes zeros whatever the direction rows hold.  Segments compose to the bit through dDirStates and the
 * carries.  No workspace beyond pointers.  CMPC_ERR_ARG as cmpc_rollout_walk_jvp_device's and the mismatch's own (a negative count, a non-NULL schedule with
 * a zero count, tick0 < 0), each refused before anything is queued.
 * sizeof(cmpc_walk_dirs_mismatch) == 24 (LP64; the ctypes mirror is held to this number). */
typedef struct cmpc_walk_dirs_mismatch {
    const double* dDirHidden;   /* [rows][B][k][6], rows = the tape's rows, as dGradHidden's */
    const float* dDirNoise;     /* [rows][B][k][9] */
    const double* dDirGain;     /* [B][k] */
} cmpc_walk_dirs_mismatch;
int cmpc_rollout_walk_jvp_mismatch_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                          int k, const cmpc_walk_dirs* d, const cmpc_plant_mismatch* m, const cmpc_walk_dirs_mismatch* md, void* stream);

/* ---- sensed pushes: a wrench sensor between the hidden schedule and the MPC (derivation: DESIGN.md 7f, "Sensed pushes") ----
 * The two ends of the split above exist: cmpc_walk_io.dWrenchTicks tells the MPC the exact wrench and how many knots it lasts (foresight), and
 * cmpc_plant_mismatch.dHiddenWrench is never told.  The reference does neither: WholeBodyQPBlock reads the F/T sensors each tick, mass-normalises the sum,
 * zeroes it when the force's norm is below 0.7, and hands that reading to setState; the MPC re-plans under a wrench it measured NOW and ASSUMES into the
 * horizon.  This section is that sensor, per problem and tick, as one small launch in front of each tick and no host read.
 * At tick number t, problem b, with m the walk's cmpc_plant_mismatch -- every step a select, never a product with zero:
 *   true_t    = hidden row t - m->tick_first when it is in range, else six zeros
 *   src_t     = hidden row t - delay_ticks - m->tick_first when it is in range, else six zeros
 *   reading_t = src_t + noise row t - m->tick_first when that is in range (ONE float32 add per component), else src_t
 *   pass_t    = !(n2 < deadband * deadband): n2 the sum of squares of the three FORCE components, in double from the floats, left to right, not contracted;
 *               the square of deadband formed once in double.  A force exactly on the threshold passes; a NaN reading passes, and the solve then reports
 *               it as it does a NaN state
 *   est_t     = pass_t ? reading_t : 0, all six components (the reference zeroes the whole wrench)
 *   wrench rows of dP: knot k < hold_knots gets est_t (force | torque), the knots beyond get zero; all N knots are written every tick
 *   plant_t   = pass_t ? true_t - est_t : true_t (ONE float32 subtract per component): the part of the disturbance the MPC was not told
 * The plant integrates (F + fExt_0) + fHidden, so with plant_t as the tick's hidden row it feels est_t + (true_t - est_t): the true wrench up to the rounding
 * of that one subtraction -- exact when the sensor is perfect, when the dead-band zeroed the reading, and whenever Sterbenz's lemma applies (est within a
 * factor two of true).  That is why no plant kernel changes.  How the reference spreads the wrench over the horizon is inside BLF ("parity
 * unpinned"); hold_knots is this library's documented rule, like the sampling rule for contacts.
 * sizeof(cmpc_wrench_sensor) == 32 (LP64; the ctypes mirror is held to this number). */
typedef struct cmpc_wrench_sensor {
    int delay_ticks;            /* >= 0: the reading of tick t is the hidden wrench of tick t - delay_ticks */
    int hold_knots;             /* 1 .. N: knots 0 .. hold_knots-1 of fExt / tauExt get the estimate, the rest zero */
    double deadband;            /* the reference's 0.7 (WholeBodyQPBlock.cpp:1018); 0: off */
    const float* dSensorNoise; int noise_ticks;   /* [noise_ticks][B][6] added to the reading, row t - m->tick_first; or NULL */
} cmpc_wrench_sensor;
/* Rows tick0 .. tick0 + rows - 1 of the rule.  Outputs dWrenchRows[rows][B][N][6] float (may be NULL), dPlantWrench[rows][B][6] float, dPass[rows][B] int
 * (may be NULL).  The host form needs no handle and no GPU (its pointers, m's and s's included, are host pointers); the device form is ONE launch, one thread
 * per (row, problem, knot), no LDS, no atomics; the two are bit-equal (one __host__ __device__ function).  Of m only tick_first, dHiddenWrench and
 * hidden_ticks are read.  CMPC_ERR_ARG: hold_knots outside 1..N, delay_ticks < 0, a negative or NaN deadband, a noise pointer with a count < 1, a negative
 * count, m without dHiddenWrench (or with hidden_ticks < 1), tick0 < 0, rows < 1, no dPlantWrench. */
int cmpc_wrench_sense(int horizon, int batch, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, float* wrench_rows,
                      float* plant_wrench, int* pass);
int cmpc_wrench_sense_device(cmpc_handle h, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, float* dWrenchRows,
                             float* dPlantWrench, int* dPass, void* stream);
/* cmpc_rollout_walk_mismatch_device with one sense launch (rows = 1, tick tick0 + i) in front of each tick.  The launch writes the tick's wrench rows into a
 * [B][N][6] buffer of the handle's workspace (allocated on first use, freed with the handle; the [ticks][B][N][6] array is never materialised) and row i of
 * the caller's dPlantWrench[ticks][B][6]; the tick then runs with that buffer as tick.dWrench and that row as its hidden row.  State noise and force gain of
 * m apply as before.  Tick numbers are explicit, so segments, resumed walks and cmpc_set_ended_device compose with it.  s == NULL:
 * cmpc_rollout_walk_mismatch_device bit for bit, and dPlantWrench is not written.  CMPC_ERR_ARG before anything is queued, besides that entry's and the sense
 * entry's: io->dWrenchTicks or io->tick.dWrench set (a known push and a sensed one are not summed); s without m->dHiddenWrench or without dPlantWrench.
 * The reverse and forward walks of a sensed tape are cmpc_rollout_walk_vjp_mismatch_device / cmpc_rollout_walk_jvp_mismatch_device with a cmpc_plant_mismatch
 * whose hidden schedule is dPlantWrench (tick_first = tick0, hidden_ticks = ticks) and whose gain is the walk's (neither walk reads the state-noise values:
 * the tape's dP holds the measured state); the tape already holds the wrench rows the solve saw. */
int cmpc_rollout_walk_sensed_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                    int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, const cmpc_plant_mismatch* m,
                                    const cmpc_wrench_sensor* s, float* dPlantWrench, void* stream);
/* The transpose.  Inputs: the reverse walk's dGradWrench[rows][B][N][6] (float) and its dGradHidden[rows][B][6] (double) taken on the plant rows.  Outputs,
 * both double, of the shape of the schedules themselves, written whole: dGradHiddenTrue[hidden_ticks][B][6], dGradSensorNoise[noise_ticks][B][6] (may be
 * NULL).  With g_j = pass_j ? (sum over k < hold_knots of dGradWrench[j][k], ascending, in double) - dGradHidden[j] : 0, hidden row r receives dGradHidden of
 * tick r + tick_first plus g of tick r + tick_first + delay_ticks, each only where that tick lies inside the call's rows; noise row r receives g of tick
 * r + tick_first.  A gather: one thread per output element, no atomics; the branch is recomputed by the shared function, not stored.  Ended problems need no
 * gate: the reverse walk has selected zero in both inputs from the ending tick on, and g selects. */
int cmpc_wrench_sense_vjp(int horizon, int batch, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, const float* grad_wrench,
                          const double* grad_hidden, double* grad_hidden_true, double* grad_sensor_noise);
int cmpc_wrench_sense_vjp_device(cmpc_handle h, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, const float* dGradWrench,
                                 const double* dGradHidden, double* dGradHiddenTrue, double* dGradSensorNoise, void* stream);
/* The tangent, in k columns.  Inputs dDirHidden[hidden_ticks][B][k][6] and dDirSensorNoise[noise_ticks][B][k][6] (or NULL), double; outputs
 * dDirWrench[rows][B][k][N][6] (float: the estimate's direction rounded once) and dDirPlantWrench[rows][B][k][6] (double) -- exactly the arrays
 * cmpc_walk_dirs.dDirWrench and cmpc_walk_dirs_mismatch.dDirHidden take.  Column j is bit-equal to a k = 1 call on column j.
 * NOT here ("next"): per-trial sensors on refill walks; the checkpointed reverse (the delay couples rows across segments, so the fold must run
 * once over the whole arrays); an autograd wrapper; a low-pass filter; a state-residual disturbance observer (state-dependent: a new carry in the gates);
 * derivatives in deadband, delay_ticks and hold_knots (discrete). */
int cmpc_wrench_sense_jvp(int horizon, int batch, int tick0, int rows, int k, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s,
                          const double* dir_hidden, const double* dir_sensor_noise, float* dir_wrench, double* dir_plant_wrench);
int cmpc_wrench_sense_jvp_device(cmpc_handle h, int tick0, int rows, int k, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s,
                                 const double* dDirHidden, const double* dDirSensorNoise, float* dDirWrench, double* dDirPlantWrench, void* stream);

/* is_warm_start_enabled on the device: dX0 = dXprev shifted by one knot; solve from it with cmpc_solve_device_warm
 * (cmpc_set_initial_guess(NULL, 1) + cmpc_advance do the same for the handle's own buffers) */
int cmpc_shift_solution_device(cmpc_handle h, const float* dXprev, float* dX0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMPC_H */
