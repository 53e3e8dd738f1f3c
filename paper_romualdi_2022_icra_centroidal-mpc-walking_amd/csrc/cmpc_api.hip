// C ABI of libcmpc_hip.so (include/cmpc.h): handle management, host<->device plumbing, launches.
#include "../../include/cmpc.h"
#include "cmpc_contacts.h"
#include "cmpc_device.h"
#include "cmpc_launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

struct cmpc_handle_s {
    cmpc_config cfg;
    CmpcLayout L;
    int B = 0, device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool timing = true;          // record the event pair around every solve launch (cmpc_set_timing)
    float* dP = nullptr;
    float* dX0 = nullptr;
    float* dX = nullptr;
    float* dInfo = nullptr;
    CmpcConsts* dConsts = nullptr;
    double hExpK[CMPC_NMAX + 1];  // exp(-k), k = 0..N: the one transcendental of a model's record, computed once here (cmpc_consts_apply_model)
    double* dExpK = nullptr;      // ... and its device copy (cmpc_set_models_device)
    CmpcConsts* dModels = nullptr;  // [B] per-problem records (cmpc_set_models*), allocated on first use
    bool models_set = false;      // launches read dModels[b] instead of dConsts
    float* dScratch = nullptr;   // factor storage when the horizon's LDS image exceeds 160 KiB
    float* dBox = nullptr;       // bounding-box limits upper[2][3] | lower[2][3] of the schedule sampler
    float* dDuals = nullptr;     // the dual record of the last solve [B][NS (N+1) + 2 NI N] (cmpc_set_multiplier_output, or the diagnostic knob below)
    bool mult_out = false;       // cmpc_set_multiplier_output: every solve writes dDuals
    const int* dEnded = nullptr; // cmpc_set_ended_device: the caller's [B] words, read by the launches on the device (>= 0: the problem is left out); null: off
    bool limits_set = false;     // cmpc_set_walk_limits: every record launch evaluates `limits` (the caller's struct, copied)
    cmpc_walk_limits limits{};
    float* dLamG = nullptr;      // [B][n_g] staging of cmpc_get_multipliers (allocated on first use)
    double* dSensWs = nullptr;   // workspace of the solution sensitivities, min(B, CMPC_SENS_SUB_BATCH) problems (allocated on first use)
    hipEvent_t sens_ev = nullptr; // recorded after the last sensitivity launch: the next one, on any stream, waits for it (one workspace)
    double* dSnapT = nullptr;    // the planner's lists snapped to the grid (cmpc_rollout_tick_device with force_sample_time, lists beyond the LDS stage)
    int* dSnapOk = nullptr;      // ... and the per-foot status words [B][2]
    char* dTickWs = nullptr;     // workspace of cmpc_rollout_tick_vjp[_rot]_device (allocated on first use, sized for both): model gradients of the solve and of
                                 // the plant [B][34] each | rotation gradients of the solve [B][2][N][3] and of the plant [B][2][3] | the plant's gradient on the
                                 // hidden wrench [B][6] and on the force gain [B] (the mismatch entry) (double) | gX[B][n_x] | gP of
                                 // the solve [B][n_p] | gP of the plant [B][n_p] (float) | the tick's ok words [B] (int)
    hipEvent_t tick_ev = nullptr; // recorded after the last kernel of a tick VJP or JVP: the next one, on any stream, waits for it (one workspace each)
    char* dTickJvpWs = nullptr;  // workspace of cmpc_rollout_tick_jvp_device for tick_jvp_cols columns per problem (allocated on first use, grown when a larger k
    int tick_jvp_cols = 0;       // arrives): rotation direction [B][k][2][N][3] | its stage 0 [B][k][2][3] | a zero state direction [B][k][9] (double) |
                                 // dx [B][k][n_x] | the assembled p direction [B][k][n_p] (float) | the tick's ok words [B] (int)
    char* dWalkWs = nullptr;     // workspace of cmpc_rollout_walk_vjp[_rot]_device for lists of walk_ws_M contacts (allocated on first use, grown when a larger
    int walk_ws_M = 0;           // max_contacts arrives): the tick's dGradState [B][9] | its dGradPrevList | its dGradPrevListRot [B][2][M][3] each (double) |
                                 // the gated dGradX row [B][n_x] | the tick's dTickSens [B][CMPC_SENS] (float) | the gated dOk [B] (int)
    char* dWalkJvpWs = nullptr;  // workspace of cmpc_rollout_walk_jvp_device for walk_jvp_cols columns and lists of walk_jvp_M contacts (allocated on first use,
    int walk_jvp_cols = 0;       // grown when a larger k or max_contacts arrives): the second buffers of the list directions, positions and orientations
    int walk_jvp_M = 0;          // [B][k][2][M][3] each (double) | the tick's dTickSens [B][CMPC_SENS] (float) | the gated dOk [B] (int)
    size_t snap_cap = 0;         // doubles allocated at dSnapT     // costates, slacks, multipliers of the last solve (warm start with duals: allocated by cmpc_create when the developer knob CMPC_WARM_DUALS is set)
    int warm_duals = 0;          // 0: primal shift only (default); 1: + costates; 2: + multipliers
    float hBox[12] = {0};
    bool box_set = false;
    long long scratch_stride = 0;
    std::vector<float> hP, hX0;  // host staging for the class-shaped setters
    bool have_solution = false, x0_set = false;
    // pinned host mirror of the handle's solution and status words, filled by cmpc_advance in the same synchronisation as the solve (the class surface's
    // getOutput / cmpc_get_solution then cost no GPU call: a pageable device-to-host copy of their own was 25 us of a 0.83 ms tick at B = 1)
    float* hXpin = nullptr;
    float* hInfoPin = nullptr;
    bool hX_valid = false;
    bool warm = false;           // class path only (cmpc_set_initial_guess(.., 1) -> cmpc_advance): the handle's own dX0 is a shifted previous solution
    double mu_warm = 1e-2, floor_warm = 1e-2;  // measured: 1e-2 saves 35 % (standing) / 15 % (walking) of the iterations; 1e-4 can stall
    int warm_budget = 14, warm_no_restart = 0;  // cmpc_set_warm_policy (CmpcParams); 14: measured on the walking roll-out (profiles/r03_walking_rollout.txt)
    bool force_warm = false;     // developer knob CMPC_FORCE_WARM (read once, at cmpc_create)
    float mu_adapt = 3.5f;       // cold starts: mu0 = clamp(mu_adapt ep0^2, 0.03, 0.5) (developer knob CMPC_MU_ADAPT, read once)
    size_t lds = 0;
    std::string err;
};

static thread_local std::string g_err;

static int fail(cmpc_handle h, int code, const std::string& msg)
{
    if (h) h->err = msg;
    g_err = msg;
    return code;
}
#define HIPCHK(h, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(h, CMPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));  \
    } while (0)

// the stream of a call: the caller's, or the handle's
static hipStream_t stream_of(cmpc_handle h, void* stream) { return stream ? (hipStream_t)stream : h->stream; }

// a launcher's return code as the entry point's: CMPC_OK, or CMPC_ERR_HIP with "<what> launch: <the HIP error string>"
static int launch_status(cmpc_handle h, const char* what, int rc)
{
    return rc == 0 ? CMPC_OK : fail(h, CMPC_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString((hipError_t)rc));
}

static void fill_consts(cmpc_handle h, CmpcConsts& q);

extern "C" {

void cmpc_default_config(cmpc_config* c)
{
    // config/robots/ergoCubGazeboV1/centroidal_mpc.ini:3-42
    std::memset(c, 0, sizeof(*c));
    c->horizon = 20;
    c->sampling_time = 0.06;
    c->friction_coefficient = 0.33;
    c->gravity = 9.80665;
    c->com_weight[0] = 10; c->com_weight[1] = 10; c->com_weight[2] = 200;
    c->angular_momentum_weight = 1e2;
    c->contact_position_weight = 2e3;
    c->force_rate_of_change_weight[0] = c->force_rate_of_change_weight[1] = c->force_rate_of_change_weight[2] = 10;
    c->contact_force_symmetry_weight = 100;
    const double cr[4][3] = {{0.08, 0.01, 0}, {0.08, -0.01, 0}, {-0.08, -0.01, 0}, {-0.08, 0.01, 0}};
    for (int ct = 0; ct < 2; ++ct)
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 3; ++i) c->corners[ct][j][i] = cr[j][i];
    c->max_iterations = 40;
    c->tolerance = 1e-6;
    c->step_tolerance = 1e-4;
    c->mu_init = 0.0;  // <= 0: chosen per problem from its initial infeasibility
    c->mu_min = 5e-8;
    c->exact_hessian = 1;
    c->final_extrapolation = 1;
    c->tail_stages = 3;
    c->tail_iterations = 2;
    c->tail_trigger = 2e-5;
}

int cmpc_dims(int N, int* nx, int* np, int* ng, int* nnzj, int* nnzh)
{
    // (the range of cmpc_create: sizes of a horizon no handle can have would only size buffers nothing can fill)
    if (N < 2 || N > CMPC_NMAX) return fail(nullptr, CMPC_ERR_ARG, "cmpc_dims: horizon must be in [2, " + std::to_string(CMPC_NMAX) + "]");
    if (nx) *nx = 45 * N + 15;
    if (np) *np = 50 * N + 27;
    if (ng) *ng = 53 * N + 15;
    if (nnzj) *nnzj = 243 * N + 15;
    if (nnzh) *nnzh = 348 * N - 36;
    return CMPC_OK;
}

const char* cmpc_last_error(cmpc_handle h) { return h ? h->err.c_str() : g_err.c_str(); }
int cmpc_batch(cmpc_handle h) { return h ? h->B : 0; }
int cmpc_factor_storage(cmpc_handle h) { return !h ? CMPC_ERR_ARG : h->scratch_stride ? CMPC_FACTORS_HBM : CMPC_FACTORS_LDS; }
void* cmpc_stream(cmpc_handle h) { return h ? (void*)h->stream : nullptr; }

// The one statement of the default tolerance rule (include/cmpc.h); the reasons are at its use in cmpc_create.
double cmpc_default_tolerance(int horizon) { return (horizon > 20 || horizon <= 3) ? 3e-7 : 1e-6; }

int cmpc_create(const cmpc_config* cfg, int batch, int device, cmpc_handle* out)
{
    if (!cfg || !out || batch < 1) return fail(nullptr, CMPC_ERR_ARG, "cmpc_create: null argument or batch < 1");
    if (cfg->horizon < 2 || cfg->horizon > CMPC_NMAX)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_create: horizon must be in [2, " + std::to_string(CMPC_NMAX) + "]");
    if (!(cfg->sampling_time > 0) || !(cfg->friction_coefficient > 0))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_create: sampling_time and friction_coefficient must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, CMPC_ERR_HIP, "cmpc_create: no HIP device (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(nullptr, CMPC_ERR_ARG, "cmpc_create: bad device index");
    cmpc_handle h = new cmpc_handle_s();
    h->cfg = *cfg;
    if (h->cfg.max_iterations <= 0) h->cfg.max_iterations = 40;
    // Default tolerance by horizon: 1e-6 up to N = 20; 3e-7 beyond (the step tolerance follows it).  The error of the far-horizon CoM velocity is fed by the
    // complementarity products that still lag above the barrier floor at termination (max t z <= tolerance), and it grows with the number of stages behind the
    // first knots.  Config 5 (N = 30), worst of 5 unseen seeds x 512 problems against the float64 oracle (profiles/r04_accuracy_sweep.txt), barrier floor 5e-8:
    // tolerance 1e-6 -> 1.05e-4 (round 3), 5e-7 -> 9.3e-5, 4e-7 -> 9.3e-5, 3e-7 -> 6.8e-5 at 8.57 / 8.95 / 9.08 / 9.24 iterations on the mean.
    // N <= 3 (no tail polish exists there: tail_stages >= horizon): 3e-7 as well.  With two or three stages the lagging products of stage 0 feed the first CoM
    // velocities directly.  Walking problems with pushes at N = 2, 3, 256 problems each, worst CoM velocity against the float64 oracle (profiles/horizon_ends.txt):
    // device 1.9e-4 / 1.3e-4 / 1.2e-4 at 1e-6 (status 0), 4.9e-5 / 3.3e-5 / 1.9e-5 at 3e-7 for +0.4 .. 0.9 iterations; the CPU model over four seeds: up to 3.4e-4 at 1e-6,
    // 1.0e-4 at 3e-7.  N = 4 and 7 are inside at 1e-6 (2.3e-5, 8.5e-6: the polish covers their stages).
    if (!(h->cfg.tolerance > 0)) h->cfg.tolerance = cmpc_default_tolerance(h->cfg.horizon);
    if (!(h->cfg.step_tolerance > 0)) h->cfg.step_tolerance = 100.0 * h->cfg.tolerance;
    // 0.05 x tolerance: the same iteration counts as tolerance / 10 (the barrier decreases superlinearly at the end)
    // at 0.7 x the sqrt(mu) bias of the nearly degenerate rows; float32 factorisations start to fail at 2e-8 (8 of 512
    // problems of config 5), 1e-8 loses most of config 3
    // ... so the default floor never goes below 5e-8, whatever the tolerance (N > 20: tolerance 3e-7, floor 5e-8)
    if (!(h->cfg.mu_min > 0)) h->cfg.mu_min = std::max(0.05 * h->cfg.tolerance, 5e-8);
    if (!(h->cfg.gravity > 0)) h->cfg.gravity = 9.80665;
    h->B = batch;
    h->device = device;
#ifdef CMPC_PROFILE
    // developer knobs exist in the diagnostic build only (-DCMPC_PROFILE), read once, here: the shipped library reads no environment variable
    if (const char* e = std::getenv("CMPC_WARM_DUALS")) h->warm_duals = std::atoi(e);
    if (const char* e = std::getenv("CMPC_MU_WARM")) { h->mu_warm = std::atof(e); h->floor_warm = std::min(1e-2, h->mu_warm); }
    h->force_warm = std::getenv("CMPC_FORCE_WARM") != nullptr;
    if (const char* e = std::getenv("CMPC_MU_ADAPT")) h->mu_adapt = (float)std::atof(e);
#endif
    if (h->cfg.tail_stages < 0 || h->cfg.tail_stages >= h->cfg.horizon) h->cfg.tail_stages = 0;
    if (h->cfg.tail_iterations < 0) h->cfg.tail_iterations = 0;
    if (!(h->cfg.tail_trigger > 0)) h->cfg.tail_trigger = 2e-5;
    if (!h->cfg.final_extrapolation) h->cfg.tail_stages = 0;   // (the polish hangs off the extrapolation step)
    cmpc_layout_init(h->L, cfg->horizon);
    h->lds = cmpc_solver_lds_bytes(cfg->horizon, 0);
    // factors in HBM scratch when the LDS image would not fit -- or, by choice, to halve the image so that
    // two workgroups share a CU (CMPC_FACTORS=hbm|lds overrides; default: LDS whenever it fits)
    bool fg = h->lds > 160 * 1024;
    {
        // more problems than CUs: the batch is throughput-bound, and two 67 KB workgroups per CU overlap
        // each other's single-wave phases (measured 1.42x at B = 4096); at B <= #CU latency rules: LDS
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && batch > prop.multiProcessorCount) fg = true;
    }
    if (h->cfg.factor_storage == CMPC_FACTORS_HBM) fg = true;
    if (h->cfg.factor_storage == CMPC_FACTORS_LDS && h->lds <= 160 * 1024) fg = false;
    if (fg) {
        h->lds = cmpc_solver_lds_bytes(cfg->horizon, 1);
        h->scratch_stride = ((long long)CMPC_REC_N + 2 * CMPC_NI) * cfg->horizon;   // factor records | slacks | multipliers
    }
    if (h->lds > 160 * 1024) {
        const int n = cfg->horizon;
        delete h;
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_create: horizon " + std::to_string(n) + " needs more than 160 KiB of LDS per problem");
    }
    // a failure below releases whatever the handle already owns (cmpc_destroy copes with a partly built handle)
#define HIPCHK_CREATE(call)                                                                                   \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            const std::string m_ = std::string("cmpc_create: " #call ": ") + hipGetErrorString(e_);           \
            (void)hipGetLastError(); /* the runtime keeps the error until it is read: a later launch must not see it */ \
            cmpc_destroy(h);                                                                                  \
            return fail(nullptr, CMPC_ERR_HIP, m_);                                                           \
        }                                                                                                     \
    } while (0)
    HIPCHK_CREATE(hipSetDevice(device));
    HIPCHK_CREATE((hipError_t)cmpc_prepare_solver(cfg->horizon, fg ? 1 : 0, h->lds));   // (the kernel variant's dynamic-LDS limit: once per handle, not per launch)
    if (fg) {
        // the factor records rely on never-written zero blocks (layout: cmpc_solver.hip): zero once
        HIPCHK_CREATE(hipMalloc(&h->dScratch, sizeof(float) * (size_t)h->scratch_stride * (size_t)batch));
        HIPCHK_CREATE(hipMemset(h->dScratch, 0, sizeof(float) * (size_t)h->scratch_stride * (size_t)batch));
    }
    HIPCHK_CREATE(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK_CREATE(hipEventCreate(&h->ev0));
    HIPCHK_CREATE(hipEventCreate(&h->ev1));
    HIPCHK_CREATE(hipMalloc(&h->dInfo, sizeof(float) * CMPC_INFO_N * (size_t)batch));
    HIPCHK_CREATE(hipMalloc(&h->dConsts, sizeof(CmpcConsts)));
    for (int k = 0; k <= cfg->horizon; ++k) h->hExpK[k] = std::exp(-(double)k);
    HIPCHK_CREATE(hipMalloc(&h->dExpK, sizeof(double) * (cfg->horizon + 1)));
    HIPCHK_CREATE(hipMemcpy(h->dExpK, h->hExpK, sizeof(double) * (cfg->horizon + 1), hipMemcpyHostToDevice));
    HIPCHK_CREATE(hipMalloc(&h->dBox, sizeof(float) * 12));
    if (h->warm_duals) {
        const size_t nd = (size_t)batch * (CMPC_NS * (cfg->horizon + 1) + 2 * CMPC_NI * cfg->horizon);
        HIPCHK_CREATE(hipMalloc(&h->dDuals, sizeof(float) * nd));
        HIPCHK_CREATE(hipMemset(h->dDuals, 0, sizeof(float) * nd));
    }
    {
        CmpcConsts q;
        fill_consts(h, q);
        HIPCHK_CREATE(hipMemcpy(h->dConsts, &q, sizeof(q), hipMemcpyHostToDevice));
    }
    // the memset and the copy above ran on the null stream; solves run on a non-blocking stream that does not
    // wait for it (a first solve racing the tail of a 350 MB memset was observed to fail): drain the device once
    HIPCHK_CREATE(hipDeviceSynchronize());
#undef HIPCHK_CREATE
    *out = h;
    return CMPC_OK;
}

int cmpc_destroy(cmpc_handle h)
{
    if (!h) return CMPC_OK;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->hXpin) hipHostFree(h->hXpin);
    if (h->hInfoPin) hipHostFree(h->hInfoPin);
    hipFree(h->dP); hipFree(h->dX0); hipFree(h->dX); hipFree(h->dInfo); hipFree(h->dConsts); hipFree(h->dScratch); hipFree(h->dBox); hipFree(h->dDuals); hipFree(h->dLamG); hipFree(h->dSensWs);
    if (h->sens_ev) hipEventDestroy(h->sens_ev);
    hipFree(h->dSnapT); hipFree(h->dSnapOk); hipFree(h->dTickWs); hipFree(h->dTickJvpWs); hipFree(h->dWalkWs); hipFree(h->dWalkJvpWs); if (h->tick_ev) hipEventDestroy(h->tick_ev); hipFree(h->dExpK); hipFree(h->dModels);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return CMPC_OK;
}

static void fill_consts(cmpc_handle h, CmpcConsts& q)
{
    const cmpc_config& c = h->cfg;
    std::memset(&q, 0, sizeof(q));
    q.N = c.horizon; q.max_iter = c.max_iterations;
    q.exact_hessian = c.exact_hessian; q.final_extrap = c.final_extrapolation;
    q.tail_stages = c.tail_stages; q.tail_iters = c.tail_iterations; q.tail_trigger = (float)c.tail_trigger;
    q.dt = (float)c.sampling_time; q.grav = (float)c.gravity;
    q.tol = (float)c.tolerance; q.step_tol = (float)c.step_tolerance; q.mu_init = (float)c.mu_init; q.mu_min = (float)c.mu_min;
    // the model: friction, weights (wz2: w_z(k) = (w_cz/2)(1+exp(-k))), corners, and the Levenberg shift reg: 5e-5 of the smallest cost curvature
    // (2 w_rate).  The shift does not move the fixed point (the right-hand side is exact); it keeps the stage Hessians factorisable in float32 along
    // directions the cost does not see (measured on MI355X: 1e-5..1e-2 all converge in the same number of iterations, 1e-1 doubles it)
    {
        cmpc_model m;
        cmpc_model_from_config(&c, &m);
        cmpc_consts_apply_model(q, m, h->hExpK);
#ifdef CMPC_PROFILE
        if (const char* e = std::getenv("CMPC_REG")) q.reg = (float)std::atof(e);
#endif
    }
    // Mehrotra's sigma = (mu_aff/mu)^3 can ask for a 1000-fold barrier decrease in one step; the linearisation
    // does not hold that far and the blocked step costs the problem 3-6 extra iterations.  A floor of 0.03
    // costs +0.3 iterations on the mean of config 2 and removes the tail (max 11 -> 8 of 4096 problems; config 3:
    // mean 8.60 -> 8.49, max 14 -> 12), and a batch is as slow as its slowest problem.
    q.sigma_min = 0.03f;
#ifdef CMPC_PROFILE
    if (const char* e = std::getenv("CMPC_SIGMA_MIN")) q.sigma_min = (float)std::atof(e);
    if (const char* e = std::getenv("CMPC_HWID_PROBE")) q.hwid_probe = std::atoi(e);
#endif
}

// the corners the plant step reads: problem 0's, and the distance in floats to the next problem's (0: one set for the batch).  Device pointer arithmetic only.
static const float* model_corners(cmpc_handle h) { return h->models_set ? h->dModels->corners : h->dConsts->corners; }
static int corners_stride(cmpc_handle h) { return h->models_set ? (int)(sizeof(CmpcConsts) / sizeof(float)) : 0; }

static void fill_params(cmpc_handle h, CmpcParams& p)
{
    std::memset(&p, 0, sizeof(p));
    p.kc = h->models_set ? h->dModels : h->dConsts; p.N = h->cfg.horizon; p.B = h->B;
    p.kc_per_problem = h->models_set ? 1 : 0;
    p.scratch = h->dScratch; p.scratch_stride = h->scratch_stride;
    // cold start: a fixed initial barrier parameter if the configuration names one, else per problem
    // mu0 = clamp(3.5 ep0^2, 0.03, 0.5) from the initial primal infeasibility ep0 (measured on 4096-problem batches:
    // config 2 wants ~0.03, config 3 ~0.3; the rule cuts the slowest problem of a 256-batch by ~0.7 iterations)
    p.mu_init = h->cfg.mu_init > 0 ? (float)h->cfg.mu_init : 0.1f;
    p.mu_adapt = h->cfg.mu_init > 0 ? 0.f : h->mu_adapt;
    p.t_floor = 1e-2f;
    p.warm_budget = h->warm_budget; p.warm_no_restart = h->warm_no_restart;
    p.duals = (h->mult_out || h->warm_duals) ? h->dDuals : nullptr; p.warm_duals = h->warm_duals;
    p.ended = h->dEnded;
    p.cold_mu_init = p.mu_init; p.cold_t_floor = p.t_floor; p.cold_mu_adapt = p.mu_adapt;   // (what a warm launch overwrites below; read only with p.start set)
}

// start / tick: the refill walk's per-problem first tick inside a warm launch (CmpcParams.start), or null
static int solve_device_impl(cmpc_handle h, const float* dP, const float* dX0, float* dX, float* dInfo, void* stream, bool warm, const int* start = nullptr,
                             int tick = 0)
{
    if (!h || !dP || !dX0 || !dX) return fail(h, CMPC_ERR_ARG, "cmpc_solve_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    CmpcParams p;
    fill_params(h, p);
    p.P = dP; p.X0 = dX0; p.X = dX; p.info = dInfo ? dInfo : h->dInfo;
    p.start = start; p.tick = tick;
    if (warm || h->force_warm) {  // dX0 is a previous solution shifted by one knot: start near the central path
        p.mu_init = (float)h->mu_warm; p.mu_adapt = 0.f; p.t_floor = (float)h->floor_warm; p.warm = 1;
    }
    if (h->timing) HIPCHK(h, hipEventRecord(h->ev0, st));
    int rc = cmpc_launch_solver(&p, h->lds, st);
    if (const int err = launch_status(h, "solver", rc)) return err;
    if (h->timing) HIPCHK(h, hipEventRecord(h->ev1, st));
    h->timed = h->timing;
    return CMPC_OK;
}

int cmpc_solve_device(cmpc_handle h, const float* dP, const float* dX0, float* dX, float* dInfo, void* stream)
{
    return solve_device_impl(h, dP, dX0, dX, dInfo, stream, false);
}

int cmpc_set_warm_policy(cmpc_handle h, int warm_budget, int restart_in_kernel)
{
    if (!h || warm_budget < 0) return fail(h, CMPC_ERR_ARG, "cmpc_set_warm_policy: bad argument");
    h->warm_budget = warm_budget;
    h->warm_no_restart = restart_in_kernel ? 0 : 1;
    return CMPC_OK;
}

int cmpc_solve_device_warm(cmpc_handle h, const float* dP, const float* dX0, float* dX, float* dInfo, void* stream)
{
    return solve_device_impl(h, dP, dX0, dX, dInfo, stream, true);
}

int cmpc_set_ended_device(cmpc_handle h, const int* dEndTick)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_set_ended_device: null handle");
    h->dEnded = dEndTick;   // (only the pointer is kept: the words are read on the device, by each launch when it runs)
    return CMPC_OK;
}

// what both forms of the record refuse in a cmpc_walk_limits; null: nothing.  (height_min > height_max is false when either is NaN: a limit that is off)
static const char* limits_refusal(const cmpc_walk_limits* lim)
{
    if (lim->height_min > lim->height_max) return "height_min above height_max";
    if (lim->dMeasures && lim->rows < 1) return "dMeasures with rows < 1";
    return nullptr;
}

int cmpc_set_walk_limits(cmpc_handle h, const cmpc_walk_limits* lim)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_set_walk_limits: null handle");
    if (!lim) { h->limits_set = false; h->limits = cmpc_walk_limits{}; return CMPC_OK; }
    if (const char* why = limits_refusal(lim)) return fail(h, CMPC_ERR_ARG, std::string("cmpc_set_walk_limits: ") + why);
    h->limits = *lim;
    h->limits_set = true;
    return CMPC_OK;
}

namespace {
__global__ __launch_bounds__(256) void poison_lds_kernel(int words, unsigned* sink)
{
    extern __shared__ unsigned pl[];
    for (int e = threadIdx.x; e < words; e += 256) pl[e] = 0x7fc00000u | (unsigned)(e & 0xffff);
    __syncthreads();
    if (sink && threadIdx.x == 0 && pl[(blockIdx.x * 97) % words] == 1u) *sink = 1u;  // keep the stores alive
}
}  // namespace

int cmpc_test_poison_lds(cmpc_handle h)
{
    if (!h) return CMPC_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const int bytes = 160 * 1024;
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(poison_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    // one workgroup per CU at a time (160 KiB each); several waves of them so that every CU is visited
    hipLaunchKernelGGL(poison_lds_kernel, dim3(2048), dim3(256), bytes, h->stream, bytes / 4, reinterpret_cast<unsigned*>(h->dInfo));
    HIPCHK(h, hipGetLastError());
    return CMPC_OK;
}

int cmpc_set_timing(cmpc_handle h, int enabled)
{
    if (!h) return CMPC_ERR_ARG;
    h->timing = enabled != 0;
    if (!h->timing) h->timed = false;
    return CMPC_OK;
}

float cmpc_last_solve_ms(cmpc_handle h)
{
    if (!h || !h->timed) return -1.f;
    float ms = -1.f;
    if (hipEventSynchronize(h->ev1) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) return -1.f;
    return ms;
}

static int ensure_buffers(cmpc_handle h)
{
    const size_t nP = (size_t)h->B * h->L.np, nX = (size_t)h->B * h->L.nx;
    if (!h->dP) HIPCHK(h, hipMalloc(&h->dP, sizeof(float) * nP));
    if (!h->dX0) HIPCHK(h, hipMalloc(&h->dX0, sizeof(float) * nX));
    if (!h->dX) HIPCHK(h, hipMalloc(&h->dX, sizeof(float) * nX));
    if (h->hP.empty()) h->hP.assign(nP, 0.f);
    return CMPC_OK;
}

static int check_status(cmpc_handle h, const std::vector<float>& info)
{
    int bad = 0, first = -1, outside = 0, first_out = -1;
    for (int b = 0; b < h->B; ++b) {
        const float st = info[(size_t)b * CMPC_INFO_N + 5];
        if (st != 0.f) { if (first < 0) first = b; ++bad; }
        if (st == 3.f) { if (first_out < 0) first_out = b; ++outside; }
    }
    if (bad) {
        char buf[240];
        int n = std::snprintf(buf, sizeof(buf), "%d of %d problems did not converge (first: %d, status %d, kkt %.3g)", bad, h->B, first,
                              (int)info[(size_t)first * CMPC_INFO_N + 5], info[(size_t)first * CMPC_INFO_N + 1]);
        if (outside && n > 0 && n < (int)sizeof(buf))
            std::snprintf(buf + n, sizeof(buf) - n, "; %d with status 3, outside the supported NLP subset (first: %d)", outside, first_out);
        return fail(h, CMPC_ERR_NOT_CONVERGED, buf);
    }
    return CMPC_OK;
}

int cmpc_solve(cmpc_handle h, const float* P, const float* X0, float* X, float* info)
{
    if (!h || !P || !X0 || !X) return fail(h, CMPC_ERR_ARG, "cmpc_solve: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure_buffers(h);
    if (rc) return rc;
    const size_t nP = (size_t)h->B * h->L.np, nX = (size_t)h->B * h->L.nx;
    HIPCHK(h, hipMemcpyAsync(h->dP, P, sizeof(float) * nP, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->dX0, X0, sizeof(float) * nX, hipMemcpyHostToDevice, h->stream));
    h->hX_valid = false;   // (dX is about to change behind the pinned mirror of cmpc_advance)
    rc = cmpc_solve_device(h, h->dP, h->dX0, h->dX, h->dInfo, nullptr);
    if (rc) return rc;
    std::vector<float> hinfo((size_t)h->B * CMPC_INFO_N);
    HIPCHK(h, hipMemcpyAsync(X, h->dX, sizeof(float) * nX, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hinfo.data(), h->dInfo, sizeof(float) * hinfo.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (info) std::memcpy(info, hinfo.data(), sizeof(float) * hinfo.size());
    h->have_solution = true;
    return check_status(h, hinfo);
}

// ---------------- class-shaped setters ----------------
int cmpc_set_state(cmpc_handle h, const float* state, const float* wrench)
{
    if (!h || !state) return fail(h, CMPC_ERR_ARG, "cmpc_set_state: null argument");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    const int N = h->cfg.horizon;
    for (int b = 0; b < h->B; ++b) {
        float* p = h->hP.data() + (size_t)b * h->L.np;
        std::memcpy(p + h->L.p_com0, state + 9 * (size_t)b, sizeof(float) * 9);
        for (int k = 0; k < N; ++k)
            for (int i = 0; i < 3; ++i) {
                p[h->L.p_fext + 3 * k + i] = wrench ? wrench[((size_t)b * N + k) * 6 + i] : 0.f;
                p[h->L.p_text + 3 * k + i] = wrench ? wrench[((size_t)b * N + k) * 6 + 3 + i] : 0.f;
            }
    }
    return CMPC_OK;
}

int cmpc_set_reference(cmpc_handle h, const float* com_ref, const float* h_ref)
{
    if (!h || !com_ref || !h_ref) return fail(h, CMPC_ERR_ARG, "cmpc_set_reference: null argument");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    const size_t n = 3 * (size_t)(h->cfg.horizon + 1);
    for (int b = 0; b < h->B; ++b) {
        float* p = h->hP.data() + (size_t)b * h->L.np;
        std::memcpy(p + h->L.p_comref, com_ref + n * b, sizeof(float) * n);
        std::memcpy(p + h->L.p_href, h_ref + n * b, sizeof(float) * n);
    }
    return CMPC_OK;
}

int cmpc_set_contacts(cmpc_handle h, const float* R, const float* upper, const float* lower, const float* enabled,
                      const float* nominal, const float* current)
{
    if (!h || !R || !upper || !lower || !enabled || !nominal || !current)
        return fail(h, CMPC_ERR_ARG, "cmpc_set_contacts: null argument");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    const int N = h->cfg.horizon;
    for (int b = 0; b < h->B; ++b) {
        float* p = h->hP.data() + (size_t)b * h->L.np;
        for (int ct = 0; ct < 2; ++ct) {
            const size_t bc = (size_t)b * 2 + ct;
            for (int k = 0; k < N; ++k) {
                const float* Rk = R + (bc * N + k) * 9;  // row-major
                for (int r = 0; r < 3; ++r)
                    for (int cc = 0; cc < 3; ++cc) p[h->L.p_R[ct] + 9 * k + 3 * cc + r] = Rk[3 * r + cc];
                const float e = enabled[bc * N + k];
                if (e != 0.f && e != 1.f) return fail(h, CMPC_ERR_ARG, "cmpc_set_contacts: enabled must be 0 or 1");
                p[h->L.p_gam[ct] + k] = e;
                for (int i = 0; i < 3; ++i) {
                    p[h->L.p_up[ct] + 3 * k + i] = upper[(bc * N + k) * 3 + i];
                    p[h->L.p_lo[ct] + 3 * k + i] = lower[(bc * N + k) * 3 + i];
                    if (p[h->L.p_up[ct] + 3 * k + i] < p[h->L.p_lo[ct] + 3 * k + i])
                        return fail(h, CMPC_ERR_ARG, "cmpc_set_contacts: bounding box upper < lower");
                }
            }
            std::memcpy(p + h->L.p_nom[ct], nominal + bc * 3 * (N + 1), sizeof(float) * 3 * (N + 1));
            std::memcpy(p + h->L.p_cur[ct], current + bc * 3, sizeof(float) * 3);
        }
    }
    return CMPC_OK;
}

static void cold_start(cmpc_handle h)
{
    const int N = h->cfg.horizon;
    h->hX0.assign((size_t)h->B * h->L.nx, 0.f);
    for (int b = 0; b < h->B; ++b) {
        const float* p = h->hP.data() + (size_t)b * h->L.np;
        float* x = h->hX0.data() + (size_t)b * h->L.nx;
        for (int k = 0; k <= N; ++k)
            for (int i = 0; i < 3; ++i) x[h->L.o_com + 3 * k + i] = p[h->L.p_com0 + i];
        for (int ct = 0; ct < 2; ++ct) {
            std::memcpy(x + h->L.o_pos[ct], p + h->L.p_nom[ct], sizeof(float) * 3 * (N + 1));
            for (int j = 0; j < 4; ++j)
                for (int k = 0; k < N; ++k) x[h->L.o_f[ct][j] + 3 * k + 2] = (float)(h->cfg.gravity / 8.0);
        }
    }
}

int cmpc_set_initial_guess(cmpc_handle h, const float* x0, int shift_previous)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_set_initial_guess: null handle");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nX = (size_t)h->B * h->L.nx;
    h->warm = false;   // only a shifted previous solution starts the barrier at mu_warm
    if (x0) {
        HIPCHK(h, hipMemcpyAsync(h->dX0, x0, sizeof(float) * nX, hipMemcpyHostToDevice, h->stream));
    } else if (shift_previous && h->have_solution) {
        CmpcParams p;
        fill_params(h, p);
        int r = cmpc_launch_warm_shift(&p, h->dX, h->dX0, h->stream);
        if (r != 0) return fail(h, CMPC_ERR_HIP, "warm-start shift launch failed");
        h->warm = true;
    } else {
        cold_start(h);
        HIPCHK(h, hipMemcpyAsync(h->dX0, h->hX0.data(), sizeof(float) * nX, hipMemcpyHostToDevice, h->stream));
    }
    h->x0_set = true;
    return CMPC_OK;
}

int cmpc_advance(cmpc_handle h)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_advance: null handle");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->x0_set) { rc = cmpc_set_initial_guess(h, nullptr, 0); if (rc) return rc; }
    HIPCHK(h, hipMemcpyAsync(h->dP, h->hP.data(), sizeof(float) * h->hP.size(), hipMemcpyHostToDevice, h->stream));
    {
        // a shifted previous solution starts close to the optimum: start the barrier at mu_warm (not 0.1) with a
        // smaller slack floor, i.e. near the central path where the previous solve passed through
        CmpcParams p;
        fill_params(h, p);
        p.P = h->dP; p.X0 = h->dX0; p.X = h->dX; p.info = h->dInfo;
        if (h->warm) { p.mu_init = (float)h->mu_warm; p.mu_adapt = 0.f; p.t_floor = (float)h->floor_warm; p.warm = 1; }
        if (h->timing) HIPCHK(h, hipEventRecord(h->ev0, h->stream));
        int lrc = cmpc_launch_solver(&p, h->lds, h->stream);
        if (const int err = launch_status(h, "solver", lrc)) return err;
        if (h->timing) HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        h->timed = h->timing;
        h->warm = false;
    }
    const size_t nXo = (size_t)h->B * h->L.nx, nIo = (size_t)h->B * CMPC_INFO_N;
    h->hX_valid = false;
    if (!h->hXpin) HIPCHK(h, hipHostMalloc((void**)&h->hXpin, sizeof(float) * nXo, hipHostMallocDefault));
    if (!h->hInfoPin) HIPCHK(h, hipHostMalloc((void**)&h->hInfoPin, sizeof(float) * nIo, hipHostMallocDefault));
    HIPCHK(h, hipMemcpyAsync(h->hXpin, h->dX, sizeof(float) * nXo, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->hInfoPin, h->dInfo, sizeof(float) * nIo, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_solution = true;
    h->hX_valid = true;
    h->x0_set = false;  // the next tick picks its own start unless told otherwise
    const std::vector<float> hinfo(h->hInfoPin, h->hInfoPin + nIo);
    return check_status(h, hinfo);
}

int cmpc_get_parameters(cmpc_handle h, float* P)
{
    if (!h || !P) return fail(h, CMPC_ERR_ARG, "cmpc_get_parameters: null argument");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    std::memcpy(P, h->hP.data(), sizeof(float) * h->hP.size());
    return CMPC_OK;
}

int cmpc_get_parameters_device(cmpc_handle h, const float** dP)
{
    if (!h || !dP) return fail(h, CMPC_ERR_ARG, "cmpc_get_parameters_device: null argument");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->dP, h->hP.data(), sizeof(float) * h->hP.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *dP = h->dP;
    return CMPC_OK;
}

int cmpc_get_solution(cmpc_handle h, float* X, float* info)
{
    if (!h || !h->have_solution) return fail(h, CMPC_ERR_ARG, "cmpc_get_solution: no solution yet");
    if (h->hX_valid) {   // (the last writer of dX was cmpc_advance: its pinned mirror is the solution)
        if (X) std::memcpy(X, h->hXpin, sizeof(float) * (size_t)h->B * h->L.nx);
        if (info) std::memcpy(info, h->hInfoPin, sizeof(float) * (size_t)h->B * CMPC_INFO_N);
        return CMPC_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (X) HIPCHK(h, hipMemcpyAsync(X, h->dX, sizeof(float) * (size_t)h->B * h->L.nx, hipMemcpyDeviceToHost, h->stream));
    if (info) HIPCHK(h, hipMemcpyAsync(info, h->dInfo, sizeof(float) * (size_t)h->B * CMPC_INFO_N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CMPC_OK;
}

int cmpc_get_output(cmpc_handle h, float* forces0, float* pos0, float* next_pos, int* next_knot)
{
    if (!h || !h->have_solution) return fail(h, CMPC_ERR_ARG, "cmpc_get_output: no solution yet");
    std::vector<float> Xcopy;
    const float* Xh = h->hXpin;
    if (!h->hX_valid) {
        Xcopy.resize((size_t)h->B * h->L.nx);
        int rc = cmpc_get_solution(h, Xcopy.data(), nullptr);
        if (rc) return rc;
        Xh = Xcopy.data();
    }
    const int N = h->cfg.horizon;
    for (int b = 0; b < h->B; ++b) {
        const float* x = Xh + (size_t)b * h->L.nx;
        const float* p = h->hP.data() + (size_t)b * h->L.np;
        for (int ct = 0; ct < 2; ++ct) {
            for (int j = 0; j < 4; ++j)
                for (int i = 0; i < 3; ++i)
                    if (forces0) forces0[(((size_t)b * 2 + ct) * 4 + j) * 3 + i] = x[h->L.o_f[ct][j] + i];
            int land = -1;  // first knot after a swing stage whose successor is in contact (or the horizon end)
            for (int k = 0; k < N; ++k)
                if (p[h->L.p_gam[ct] + k] < 0.5f && (k + 1 == N || p[h->L.p_gam[ct] + k + 1] > 0.5f)) { land = k + 1; break; }
            for (int i = 0; i < 3; ++i) {
                if (pos0) pos0[((size_t)b * 2 + ct) * 3 + i] = x[h->L.o_pos[ct] + i];
                if (next_pos) next_pos[((size_t)b * 2 + ct) * 3 + i] = land >= 0 ? x[h->L.o_pos[ct] + 3 * land + i] : x[h->L.o_pos[ct] + i];
            }
            if (next_knot) next_knot[(size_t)b * 2 + ct] = land;
        }
    }
    return CMPC_OK;
}

int cmpc_eval_nlp_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, float lam_f, float* dF,
                         float* dG, float* dGradF, float* dJac, float* dHess, void* stream)
{
    if (!h || !dX || !dP) return fail(h, CMPC_ERR_ARG, "cmpc_eval_nlp_device: null argument");
    if (dHess && !dLamG) return fail(h, CMPC_ERR_ARG, "cmpc_eval_nlp_device: the Hessian needs lam_g");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_nlp_eval(&p, dX, dP, dLamG, lam_f, dF, dG, dGradF, dJac, dHess, stream_of(h, stream));
    return launch_status(h, "nlp eval", rc);
}

int cmpc_eval_nlp_grad_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, float lam_f, float* dGradX, float* dGradP,
                              void* stream)
{
    if (!h || !dX || !dP || !dLamG) return fail(h, CMPC_ERR_ARG, "cmpc_eval_nlp_grad_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_nlp_grad(&p, dX, dP, dLamG, lam_f, dGradX, dGradP, stream_of(h, stream));
    return launch_status(h, "nlp grad", rc);
}

// ---- multipliers of the reference NLP (include/cmpc.h) ----
int cmpc_set_multiplier_output(cmpc_handle h, int enabled)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_set_multiplier_output: null handle");
    HIPCHK(h, hipSetDevice(h->device));
    if (enabled && !h->dDuals) {
        const size_t nd = (size_t)h->B * (CMPC_NS * (h->cfg.horizon + 1) + 2 * CMPC_NI * h->cfg.horizon);
        HIPCHK(h, hipMalloc(&h->dDuals, sizeof(float) * nd));
        HIPCHK(h, hipMemsetAsync(h->dDuals, 0, sizeof(float) * nd, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    } else if (!enabled && h->dDuals && !h->warm_duals) {   // (the diagnostic warm start with duals keeps its record)
        HIPCHK(h, hipDeviceSynchronize());   // (a launch on any stream may still write the record)
        HIPCHK(h, hipFree(h->dDuals));
        h->dDuals = nullptr;
    }
    h->mult_out = enabled != 0;
    return CMPC_OK;
}

int cmpc_get_multipliers_device(cmpc_handle h, const float* dX, const float* dP, float* dLamG, void* stream)
{
    if (!h || !dX || !dP || !dLamG) return fail(h, CMPC_ERR_ARG, "cmpc_get_multipliers_device: null argument");
    if (!h->mult_out || !h->dDuals) return fail(h, CMPC_ERR_ARG, "cmpc_get_multipliers_device: the multiplier output is off (cmpc_set_multiplier_output)");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_multipliers(&p, dX, dP, dLamG, stream_of(h, stream));
    return launch_status(h, "multipliers", rc);
}

int cmpc_get_multipliers(cmpc_handle h, float* LamG)
{
    if (!h || !LamG) return fail(h, CMPC_ERR_ARG, "cmpc_get_multipliers: null argument");
    if (!h->have_solution) return fail(h, CMPC_ERR_ARG, "cmpc_get_multipliers: no solution yet (cmpc_advance)");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->B * h->L.ng;
    if (!h->dLamG) HIPCHK(h, hipMalloc(&h->dLamG, sizeof(float) * n));
    int rc = cmpc_get_multipliers_device(h, h->dX, h->dP, h->dLamG, nullptr);
    if (rc != CMPC_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(LamG, h->dLamG, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CMPC_OK;
}

int cmpc_kkt_certificate_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, float* dCert, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dCert) return fail(h, CMPC_ERR_ARG, "cmpc_kkt_certificate_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_kkt_certificate(&p, dX, dP, dLamG, dCert, stream_of(h, stream));
    return launch_status(h, "kkt certificate", rc);
}

int cmpc_value_gradient_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, float* dGradP, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dGradP) return fail(h, CMPC_ERR_ARG, "cmpc_value_gradient_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_value_gradient(&p, dX, dP, dLamG, dGradP, stream_of(h, stream));
    return launch_status(h, "value gradient", rc);
}

// ---- solution sensitivities (include/cmpc.h; cmpc_sensitivity.hip) ----
static int sensitivity(cmpc_handle h, const char* name, const float* dX, const float* dP, const float* dLamG, const float* dDirP, const float* dGradX,
                       int k, float* dOut, float* dSens, void* stream, const double* dDirModel = nullptr, double* dGradModel = nullptr,
                       const double* dDirRot = nullptr, double* dGradRot = nullptr)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int N = h->cfg.horizon, sb = h->B < CMPC_SENS_SUB_BATCH ? h->B : CMPC_SENS_SUB_BATCH;
    if (!h->dSensWs) HIPCHK(h, hipMalloc(&h->dSensWs, cmpc_sensitivity_workspace_bytes(N) * (size_t)sb));
    const hipStream_t st = stream_of(h, stream);
    const CmpcConsts* kc = h->models_set ? h->dModels : h->dConsts;
    // the workspace is the handle's: a call on another stream than the previous one is ordered after it
    if (!h->sens_ev) HIPCHK(h, hipEventCreateWithFlags(&h->sens_ev, hipEventDisableTiming));
    else HIPCHK(h, hipStreamWaitEvent(st, h->sens_ev, 0));
    for (int b0 = 0; b0 < h->B; b0 += sb) {
        const int nb = h->B - b0 < sb ? h->B - b0 : sb;
        int rc = cmpc_launch_sensitivity(kc, h->models_set ? 1 : 0, N, b0, nb, dX, dP, dLamG, dDirP, dGradX, k, dOut, dSens, h->dSensWs, dDirModel,
                                         dGradModel, dDirRot, dGradRot, st);
        if (const int err = launch_status(h, name, rc)) return err;
    }
    HIPCHK(h, hipEventRecord(h->sens_ev, st));
    return CMPC_OK;
}

int cmpc_solution_jvp_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dDirP, int k, float* dDX, float* dSens,
                             void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dDirP || !dDX) return fail(h, CMPC_ERR_ARG, "cmpc_solution_jvp_device: null argument");
    if (k < 1) return fail(h, CMPC_ERR_ARG, "cmpc_solution_jvp_device: k must be >= 1");
    return sensitivity(h, "cmpc_solution_jvp_device", dX, dP, dLamG, dDirP, nullptr, k, dDX, dSens, stream);
}

int cmpc_solution_vjp_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, float* dGradP, float* dSens,
                             void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dGradX || !dGradP) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_device: null argument");
    return sensitivity(h, "cmpc_solution_vjp_device", dX, dP, dLamG, nullptr, dGradX, 1, dGradP, dSens, stream);
}

// ---- derivatives with respect to the per-problem model (include/cmpc.h, "model directions") ----
int cmpc_solution_jvp_model_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dDirP, const double* dDirModel, int k,
                                   float* dDX, float* dSens, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dDX) return fail(h, CMPC_ERR_ARG, "cmpc_solution_jvp_model_device: null argument");
    if (k < 1) return fail(h, CMPC_ERR_ARG, "cmpc_solution_jvp_model_device: k must be >= 1");
    return sensitivity(h, "cmpc_solution_jvp_model_device", dX, dP, dLamG, dDirP, nullptr, k, dDX, dSens, stream, dDirModel, nullptr);
}

int cmpc_solution_vjp_model_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, float* dGradP,
                                   double* dGradModel, float* dSens, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dGradX || !dGradModel) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_model_device: null argument");
    return sensitivity(h, "cmpc_solution_vjp_model_device", dX, dP, dLamG, nullptr, dGradX, 1, dGradP, dSens, stream, nullptr, dGradModel);
}

int cmpc_model_value_gradient_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, double* dGradModel, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dGradModel) return fail(h, CMPC_ERR_ARG, "cmpc_model_value_gradient_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_model_value_gradient(&p, dX, dP, dLamG, dGradModel, stream_of(h, stream));
    return launch_status(h, "model value gradient", rc);
}

// ---- derivatives with respect to the stage rotations (include/cmpc.h, "rotation directions") ----
int cmpc_solution_jvp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dDirP, const double* dDirModel,
                                 const double* dDirRot, int k, float* dDX, float* dSens, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dDX) return fail(h, CMPC_ERR_ARG, "cmpc_solution_jvp_rot_device: null argument");
    if (k < 1) return fail(h, CMPC_ERR_ARG, "cmpc_solution_jvp_rot_device: k must be >= 1");
    return sensitivity(h, "cmpc_solution_jvp_rot_device", dX, dP, dLamG, dDirP, nullptr, k, dDX, dSens, stream, dDirModel, nullptr, dDirRot, nullptr);
}

int cmpc_solution_vjp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, float* dGradP,
                                 double* dGradModel, double* dGradRot, float* dSens, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dGradX) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_rot_device: null argument");
    if (!dGradP && !dGradModel && !dGradRot) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_rot_device: no output requested");
    return sensitivity(h, "cmpc_solution_vjp_rot_device", dX, dP, dLamG, nullptr, dGradX, 1, dGradP, dSens, stream, nullptr, dGradModel, nullptr, dGradRot);
}

// ---- cotangent columns (include/cmpc.h): k VJPs behind one factorisation per problem ----
int cmpc_solution_vjp_cols_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, const float* dGradX, int k, float* dGradP,
                                  double* dGradModel, double* dGradRot, float* dSens, void* stream)
{
    // (what needs no handle is refused ahead of the handle check, so the message says which refusal it was)
    if (!dX || !dP || !dLamG || !dGradX) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_cols_device: null input (dX, dP, dLamG and dGradX are required)");
    if (k < 1) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_cols_device: k must be >= 1");
    if (!dGradP && !dGradModel && !dGradRot) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_cols_device: no output requested");
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_solution_vjp_cols_device: null handle");
    return sensitivity(h, "cmpc_solution_vjp_cols_device", dX, dP, dLamG, nullptr, dGradX, k, dGradP, dSens, stream, nullptr, dGradModel, nullptr, dGradRot);
}

int cmpc_rotation_value_gradient_device(cmpc_handle h, const float* dX, const float* dP, const float* dLamG, double* dGradRot, void* stream)
{
    if (!h || !dX || !dP || !dLamG || !dGradRot) return fail(h, CMPC_ERR_ARG, "cmpc_rotation_value_gradient_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_rotation_value_gradient(&p, dX, dP, dLamG, dGradRot, stream_of(h, stream));
    return launch_status(h, "rotation value gradient", rc);
}

int cmpc_contacts_rotation_vjp_device(cmpc_handle h, int max_contacts, double now, const double* dT, const int* dN, const double* dGradRot,
                                      double* dGradListRot, void* stream)
{
    if (!h || max_contacts < 1 || !dT || !dN || !dGradRot || !dGradListRot) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_rotation_vjp_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_contacts_rotation_vjp(h->B, h->cfg.horizon, max_contacts, h->cfg.sampling_time, now, dT, dN, dGradRot, dGradListRot,
                                               stream_of(h, stream));
    return launch_status(h, "contact rotation adjoint", rc);
}

// ---- 8f-3: planner references -> MPC knots (CentroidalMPCBlock.cpp:525-577): angular momentum / mass, CoM height
// override, linear spline from the planner's knots (period in_dt, first knot t_offset in the past) to the N+1 MPC
// knots; clamped at both ends.  Host-side like the reference's LinearSpline; fills the handle's parameter staging. ----
int cmpc_set_reference_from_planner(cmpc_handle h, const float* com_in, const float* h_in, int n_in, double in_dt, double t_offset,
                                    double robot_mass, double com_height)
{
    if (!h || !com_in || !h_in || n_in < 2 || !(in_dt > 0) || !(robot_mass > 0))
        return fail(h, CMPC_ERR_ARG, "cmpc_set_reference_from_planner: bad argument");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    const int N = h->cfg.horizon;
    for (int b = 0; b < h->B; ++b) {
        float* p = h->hP.data() + (size_t)b * h->L.np;
        const float* ci = com_in + (size_t)b * n_in * 3;
        const float* hi = h_in + (size_t)b * n_in * 3;
        for (int k = 0; k <= N; ++k)
            cmpc_resample_reference_knot(ci, hi, n_in, in_dt, t_offset, h->cfg.sampling_time, k, robot_mass, com_height, p + h->L.p_comref + 3 * k,
                                         p + h->L.p_href + 3 * k);
    }
    return CMPC_OK;
}

// the same on the device, into the caller's dP (one thread per problem and knot)
int cmpc_write_reference_from_planner_device(cmpc_handle h, const float* dComIn, const float* dHIn, int n_in, double in_dt, double t_offset, double robot_mass,
                                             double com_height, float* dP, void* stream)
{
    if (!h || !dComIn || !dHIn || !dP || n_in < 2 || !(in_dt > 0) || !(robot_mass > 0))
        return fail(h, CMPC_ERR_ARG, "cmpc_write_reference_from_planner_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_reference_from_planner(h->B, h->cfg.horizon, n_in, h->cfg.sampling_time, in_dt, t_offset, robot_mass, com_height, dComIn, dHIn, dP,
                                                stream_of(h, stream));
    return launch_status(h, "reference resampling", rc);
}

// ---- 8f-3 differentiated in the planner's trajectories (include/cmpc.h): the transpose of the resampling summed over the rows of a walk, and its image of
// k directions.  The rule is cmpc_contacts.h's (cmpc_reference_weight, cmpc_reference_vjp_terms, cmpc_reference_jvp_entry), shared with the kernels. ----
static bool ref_args(const char* name, cmpc_handle h, int horizon, double sampling_time, int batch, int tick0, int rows, int k, const cmpc_planner_refs* pl,
                     CmpcRefArgs* a, int* rc)
{
    const bool good = pl && horizon >= 1 && horizon <= CMPC_NMAX && sampling_time > 0 && std::isfinite(sampling_time) && batch >= 1 && tick0 >= 0 && rows >= 1 &&
                      (long long)tick0 + rows <= 2147483647LL && k >= 1 && pl->knots >= 2 && pl->dt > 0 && std::isfinite(pl->dt) && pl->robot_mass > 0 &&
                      std::isfinite(pl->robot_mass) && std::isfinite(pl->t_first);
    if (!good) {
        *rc = fail(h, CMPC_ERR_ARG, std::string(name) + ": bad argument (rows >= 1, tick0 >= 0, k >= 1, knots >= 2, dt and robot_mass positive and finite)");
        return false;
    }
    *a = CmpcRefArgs{horizon, batch, pl->knots, tick0, rows, k, sampling_time, pl->dt, pl->t_first, pl->robot_mass, pl->com_height};
    return true;
}

int cmpc_reference_from_planner_vjp(int horizon, double sampling_time, int batch, int tick0, int rows, const cmpc_planner_refs* pl, const int* end_tick,
                                    const float* grad_p, double* grad_com, double* grad_h)
{
    CmpcRefArgs a;
    int rc = CMPC_OK;
    if (!ref_args("cmpc_reference_from_planner_vjp", nullptr, horizon, sampling_time, batch, tick0, rows, 1, pl, &a, &rc)) return rc;
    if (!grad_p || (!grad_com && !grad_h)) return fail(nullptr, CMPC_ERR_ARG, "cmpc_reference_from_planner_vjp: grad_p and one of grad_com / grad_h are needed");
    const CmpcIdx L{horizon};
    const int K1 = horizon + 1, np = L.np(), base = L.pComref();
    const bool z_fixed = a.com_height == a.com_height;
    std::vector<int> i0((size_t)rows * K1);
    std::vector<double> w((size_t)rows * K1);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < K1; ++k) cmpc_reference_weight(a.knots, a.in_dt, a.t_first, a.dt, tick0 + r, k, &i0[(size_t)r * K1 + k], &w[(size_t)r * K1 + k]);
    // (in place: an entry's terms arrive in ascending (row, knot) order, which is the order its owner adds them in on the device)
    for (int b = 0; b < batch; ++b) {
        const int nr = cmpc_reference_rows_of(end_tick, b, tick0, rows);
        double* gc = grad_com ? grad_com + (size_t)b * a.knots * 3 : nullptr;
        double* gh = grad_h ? grad_h + (size_t)b * a.knots * 3 : nullptr;
        for (int r = 0; r < nr; ++r) {
            const float* g = grad_p + ((size_t)r * batch + b) * np + base;
            for (int k = 0; k < K1; ++k) {
                const int j = i0[(size_t)r * K1 + k];
                for (int c = 0; c < 3; ++c) {
                    const bool with_com = !(z_fixed && c == 2);
                    double tc[2] = {0.0, 0.0}, th[2];
                    cmpc_reference_vjp_terms(w[(size_t)r * K1 + k], with_com, with_com ? g[3 * k + c] : 0.f, g[3 * K1 + 3 * k + c], a.robot_mass, tc, th);
                    for (int t = 0; t < 2; ++t) {
                        if (gc && with_com) gc[3 * (j + t) + c] += tc[t];
                        if (gh) gh[3 * (j + t) + c] += th[t];
                    }
                }
            }
        }
    }
    return CMPC_OK;
}

int cmpc_reference_from_planner_vjp_device(cmpc_handle h, int tick0, int rows, const cmpc_planner_refs* pl, const int* dEndTick, const float* dGradP,
                                           double* dGradCom, double* dGradH, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_reference_from_planner_vjp_device: null handle");
    CmpcRefArgs a;
    int rc = CMPC_OK;
    if (!ref_args("cmpc_reference_from_planner_vjp_device", h, h->cfg.horizon, h->cfg.sampling_time, h->B, tick0, rows, 1, pl, &a, &rc)) return rc;
    if (!dGradP || (!dGradCom && !dGradH))
        return fail(h, CMPC_ERR_ARG, "cmpc_reference_from_planner_vjp_device: dGradP and one of dGradCom / dGradH are needed");
    if ((a.knots + 127) / 128 > 65535) return fail(h, CMPC_ERR_ARG, "cmpc_reference_from_planner_vjp_device: too many knots for one launch");
    HIPCHK(h, hipSetDevice(h->device));
    rc = cmpc_launch_reference_vjp(&a, dEndTick, dGradP, dGradCom, dGradH, stream_of(h, stream));
    return launch_status(h, "reference VJP", rc);
}

int cmpc_reference_from_planner_jvp(int horizon, double sampling_time, int batch, int tick0, int rows, int k, const cmpc_planner_refs* pl,
                                    const double* dir_com, const double* dir_h, float* dir_p)
{
    CmpcRefArgs a;
    int rc = CMPC_OK;
    if (!ref_args("cmpc_reference_from_planner_jvp", nullptr, horizon, sampling_time, batch, tick0, rows, k, pl, &a, &rc)) return rc;
    if (!dir_p || (!dir_com && !dir_h)) return fail(nullptr, CMPC_ERR_ARG, "cmpc_reference_from_planner_jvp: dir_p and one of dir_com / dir_h are needed");
    const CmpcIdx L{horizon};
    const int per = 6 * (horizon + 1), np = L.np(), base = L.pComref();
    const size_t cols = (size_t)batch * k;
    for (int r = 0; r < rows; ++r)
        for (size_t bk = 0; bk < cols; ++bk) {
            const size_t in = bk * a.knots * 3;
            float* out = dir_p + ((size_t)r * cols + bk) * np + base;
            for (int e6 = 0; e6 < per; ++e6)
                out[e6] = cmpc_reference_jvp_entry(a, tick0 + r, e6, dir_com ? dir_com + in : nullptr, dir_h ? dir_h + in : nullptr);
        }
    return CMPC_OK;
}

int cmpc_reference_from_planner_jvp_device(cmpc_handle h, int tick0, int rows, int k, const cmpc_planner_refs* pl, const double* dDirCom, const double* dDirH,
                                           float* dDirP, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_reference_from_planner_jvp_device: null handle");
    CmpcRefArgs a;
    int rc = CMPC_OK;
    if (!ref_args("cmpc_reference_from_planner_jvp_device", h, h->cfg.horizon, h->cfg.sampling_time, h->B, tick0, rows, k, pl, &a, &rc)) return rc;
    if (!dDirP || (!dDirCom && !dDirH)) return fail(h, CMPC_ERR_ARG, "cmpc_reference_from_planner_jvp_device: dDirP and one of dDirCom / dDirH are needed");
    const double total = (double)rows * h->B * k * 6.0 * (h->cfg.horizon + 1);
    if (total / 256.0 > 2147483000.0) return fail(h, CMPC_ERR_ARG, "cmpc_reference_from_planner_jvp_device: too many entries for one launch");
    HIPCHK(h, hipSetDevice(h->device));
    rc = cmpc_launch_reference_jvp(&a, dDirCom, dDirH, dDirP, stream_of(h, stream));
    return launch_status(h, "reference JVP", rc);
}

// ---- 8f-4: plant step on the device (see cmpc_plant_step_kernel) ----
int cmpc_plant_step_mismatch_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, float* dStateOut, float* dZmp,
                                    double step, int substeps, double zmp_half_x, double zmp_half_y, const float* dHiddenWrench, const float* dForceGain,
                                    void* stream)
{
    if (!h || !dX || !dP || !dStateIn || !dStateOut || !(step > 0) || substeps < 1)
        return fail(h, CMPC_ERR_ARG, "cmpc_plant_step_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_plant_step(h->cfg.horizon, h->B, (float)h->cfg.gravity, model_corners(h), corners_stride(h), dX, dP, dStateIn, dStateOut, dZmp, (float)step,
                                    substeps, (float)zmp_half_x, (float)zmp_half_y, dHiddenWrench, dForceGain, stream_of(h, stream));
    return launch_status(h, "plant step", rc);
}

int cmpc_plant_step_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, float* dStateOut, float* dZmp,
                           double step, int substeps, double zmp_half_x, double zmp_half_y, void* stream)
{
    return cmpc_plant_step_mismatch_device(h, dX, dP, dStateIn, dStateOut, dZmp, step, substeps, zmp_half_x, zmp_half_y, nullptr, nullptr, stream);
}

// ---- plant-step derivatives (include/cmpc.h; cmpc_plant_jvp_kernel / cmpc_plant_vjp_kernel, next to the plant kernel) ----
int cmpc_plant_step_jvp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, const double* dDirState,
                                   const float* dDirX, const float* dDirP, const double* dDirModel, const double* dDirRot0, double* dDirStateOut, void* stream)
{
    if (!h || !dX || !dP || !dStateIn || !dDirState || !dDirStateOut || !(step > 0) || substeps < 1)
        return fail(h, CMPC_ERR_ARG, "cmpc_plant_step_jvp_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_plant_jvp(h->cfg.horizon, h->B, (float)h->cfg.gravity, model_corners(h), corners_stride(h), dX, dP, dStateIn, (float)step, substeps,
                                   dDirState, dDirX, dDirP, dDirModel, dDirRot0, dDirStateOut, stream_of(h, stream));
    return launch_status(h, "plant JVP", rc);
}

int cmpc_plant_step_jvp_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, const double* dDirState,
                               const float* dDirX, const float* dDirP, const double* dDirModel, double* dDirStateOut, void* stream)
{
    return cmpc_plant_step_jvp_rot_device(h, dX, dP, dStateIn, step, substeps, dDirState, dDirX, dDirP, dDirModel, nullptr, dDirStateOut, stream);
}

static int plant_vjp(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, const double* dGradStateOut,
                     double* dGradState, float* dGradX, float* dGradP, double* dGradModel, double* dGradRot0, bool mismatch, const float* dHiddenWrench,
                     const float* dForceGain, double* dGradHidden, double* dGradGain, void* stream)
{
    if (!h || !dX || !dP || !dStateIn || !dGradStateOut || !dGradState || !dGradX || !(step > 0) || substeps < 1)
        return fail(h, CMPC_ERR_ARG, "cmpc_plant_step_vjp_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_plant_vjp(h->cfg.horizon, h->B, (float)h->cfg.gravity, model_corners(h), corners_stride(h), dX, dP, dStateIn, (float)step, substeps,
                                   dGradStateOut, dGradState, dGradX, dGradP, dGradModel, dGradRot0, mismatch ? 1 : 0, dHiddenWrench, dForceGain, dGradHidden,
                                   dGradGain, stream_of(h, stream));
    return launch_status(h, "plant VJP", rc);
}

int cmpc_plant_step_vjp_rot_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps,
                                   const double* dGradStateOut, double* dGradState, float* dGradX, float* dGradP, double* dGradModel, double* dGradRot0,
                                   void* stream)
{
    return plant_vjp(h, dX, dP, dStateIn, step, substeps, dGradStateOut, dGradState, dGradX, dGradP, dGradModel, dGradRot0, false, nullptr, nullptr, nullptr,
                     nullptr, stream);
}

int cmpc_plant_step_vjp_mismatch_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps,
                                        const double* dGradStateOut, double* dGradState, float* dGradX, float* dGradP, double* dGradModel, double* dGradRot0,
                                        const float* dHiddenWrench, const float* dForceGain, double* dGradHidden, double* dGradGain, void* stream)
{
    return plant_vjp(h, dX, dP, dStateIn, step, substeps, dGradStateOut, dGradState, dGradX, dGradP, dGradModel, dGradRot0, true, dHiddenWrench, dForceGain,
                     dGradHidden, dGradGain, stream);
}

int cmpc_plant_step_vjp_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, const double* dGradStateOut,
                               double* dGradState, float* dGradX, float* dGradP, double* dGradModel, void* stream)
{
    return cmpc_plant_step_vjp_rot_device(h, dX, dP, dStateIn, step, substeps, dGradStateOut, dGradState, dGradX, dGradP, dGradModel, nullptr, stream);
}

// ---- 8e: compact per-problem output for the all-gather (see cmpc_compact_kernel) ----
int cmpc_compact_output_device(cmpc_handle h, const float* dX, const float* dInfo, float* dOut, void* stream)
{
    if (!h || !dX || !dInfo || !dOut) return fail(h, CMPC_ERR_ARG, "cmpc_compact_output_device: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_compact(h->cfg.horizon, h->B, dX, dInfo, dOut, stream_of(h, stream));
    return launch_status(h, "compact output", rc);
}

// ---- 8f-1: contact schedules, batched (logic: cmpc_contacts.h) ----
// ---- 8e: the gather of compact solutions across the GPUs of a node, through RCCL (ncclAllGather over xGMI).  librccl is opened on first use, so that the
// library itself carries no link-time dependency on it: a single-GPU caller never loads it. ----
namespace {
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int /*ncclDataType_t*/, void* /*ncclComm_t*/, hipStream_t);
nccl_allgather_fn load_allgather(std::string& why)
{
    static nccl_allgather_fn fn = nullptr;
    static bool tried = false;
    if (tried) { if (!fn) why = "librccl.so: ncclAllGather not available"; return fn; }
    tried = true;
    void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) { why = std::string("dlopen(librccl.so): ") + dlerror(); return nullptr; }
    fn = reinterpret_cast<nccl_allgather_fn>(dlsym(lib, "ncclAllGather"));
    if (!fn) why = "librccl.so has no ncclAllGather";
    return fn;
}
}  // namespace

int cmpc_allgather_compact_device(cmpc_handle h, void* nccl_comm, int world_size, const float* dLocal, float* dAll, void* stream)
{
    if (!h || !nccl_comm || world_size < 1 || !dLocal || !dAll) return fail(h, CMPC_ERR_ARG, "cmpc_allgather_compact_device: bad argument");
    std::string why;
    nccl_allgather_fn ag = load_allgather(why);
    if (!ag) return fail(h, CMPC_ERR_HIP, "cmpc_allgather_compact_device: " + why);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    const size_t count = (size_t)h->B * (size_t)(3 * (h->cfg.horizon + 1) + 38);   // floats of this rank's compact records (cmpc_compact_output_device)
    const int rc = ag(dLocal, dAll, count, 7 /* ncclFloat32 */, nccl_comm, st);
    if (rc != 0) return fail(h, CMPC_ERR_HIP, "ncclAllGather failed with code " + std::to_string(rc));
    return CMPC_OK;
}

int cmpc_contacts_merge(int batch, int max_contacts, double now, const double* plan_t, const float* plan_pose, const int* plan_n,
                        const double* mpc_t, const float* mpc_pose, const int* mpc_n, double* out_t, float* out_pose, int* out_n, int* ok)
{
    if (batch < 1 || max_contacts < 1 || !plan_t || !plan_pose || !plan_n || !mpc_t || !mpc_pose || !mpc_n || !out_t || !out_pose || !out_n)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_merge: bad argument");
    const int M = max_contacts;
    int all = CMPC_OK;
    for (int b = 0; b < batch; ++b) {
        bool good = true;
        for (int c = 0; c < 2; ++c) {
            const size_t e = (size_t)b * 2 + c, o = e * M;
            if (plan_n[e] < 0 || plan_n[e] > M || mpc_n[e] < 0 || mpc_n[e] > M) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_merge: list length out of range");
            good = cmpc_merge_foot(now, plan_t + 2 * o, plan_pose + 7 * o, plan_n[e], mpc_t + 2 * o, mpc_pose + 7 * o, mpc_n[e], M,
                                   out_t + 2 * o, out_pose + 7 * o, out_n + e) && good;
        }
        if (ok) ok[b] = good ? 1 : 0;
        if (!good) all = CMPC_ERR_ARG;
    }
    if (all != CMPC_OK) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_merge: the planner has no active contact where the MPC list has one");
    return CMPC_OK;
}

int cmpc_contacts_sample(int horizon, double dt, int batch, int max_contacts, double now, const double* t, const float* pose, const int* n,
                         const float* box_upper, const float* box_lower, float* P, int* land)
{
    if (horizon < 1 || !(dt > 0) || batch < 1 || max_contacts < 1 || !t || !pose || !n || !box_upper || !box_lower || !P)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_sample: bad argument");
    const CmpcIdx L{horizon};
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < 2; ++c) {
            const size_t e = (size_t)b * 2 + c, o = e * max_contacts;
            if (n[e] < 1 || n[e] > max_contacts) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_sample: every foot needs 1..max_contacts contacts");
            const int lk = cmpc_sample_foot(horizon, dt, now, c, t + 2 * o, pose + 7 * o, n[e], box_upper, box_lower, P + (size_t)b * L.np());
            if (land) land[e] = lk;
        }
    return CMPC_OK;
}

int cmpc_contacts_adjust(int horizon, int batch, int max_contacts, double now, const float* X, const int* land, const double* t, float* pose, const int* n)
{
    if (horizon < 1 || batch < 1 || max_contacts < 1 || !X || !land || !t || !pose || !n) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_adjust: bad argument");
    const CmpcIdx L{horizon};
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < 2; ++c) {
            const size_t e = (size_t)b * 2 + c, o = e * max_contacts;
            if (land[e] < 0 || land[e] > horizon) continue;
            if (n[e] < 1 || n[e] > max_contacts) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_adjust: every foot needs 1..max_contacts contacts");
            const int nx = cmpc_next_contact(t + 2 * o, n[e], now);
            if (nx < 0) continue;
            for (int i = 0; i < 3; ++i) pose[7 * (o + nx) + i] = X[(size_t)b * L.nx() + L.oPos(c) + 3 * land[e] + i];
        }
    return CMPC_OK;
}

int cmpc_contacts_merge_device(cmpc_handle h, int max_contacts, double now, const double* dPlanT, const float* dPlanPose, const int* dPlanN,
                               const double* dMpcT, const float* dMpcPose, const int* dMpcN, double* dOutT, float* dOutPose, int* dOutN,
                               int* dOk, void* stream)
{
    if (!h || max_contacts < 1 || !dPlanT || !dPlanPose || !dPlanN || !dMpcT || !dMpcPose || !dMpcN || !dOutT || !dOutPose || !dOutN)
        return fail(h, CMPC_ERR_ARG, "cmpc_contacts_merge_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_contacts_merge(h->B, max_contacts, now, dPlanT, dPlanPose, dPlanN, dMpcT, dMpcPose, dMpcN, dOutT, dOutPose, dOutN, dOk,
                                        stream_of(h, stream));
    return launch_status(h, "contact merge", rc);
}

// forceSampleTime (CentroidalMPCBlock.cpp:586-592): dt in integer nanoseconds, or 0 if it is not a usable grid
static long long snap_dt_ns(double dt)
{
    if (!(dt > 0) || !(dt < CMPC_TIME_NEVER)) return 0;
    const long long dt_ns = llround(dt * 1e9);
    return dt_ns >= 1 ? dt_ns : 0;
}

int cmpc_contacts_force_sample_time(int batch, int max_contacts, double dt, const double* t, const int* n, double* out_t, int* ok)
{
    const long long dt_ns = snap_dt_ns(dt);
    if (batch < 1 || max_contacts < 1 || dt_ns < 1 || !t || !n || !out_t) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_force_sample_time: bad argument");
    const int M = max_contacts;
    for (int e = 0; e < 2 * batch; ++e)
        if (n[e] < 0 || n[e] > M) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_force_sample_time: list length out of range");
    int all = CMPC_OK;
    for (int b = 0; b < batch; ++b) {
        bool good = true;
        for (int c = 0; c < 2; ++c) {
            const size_t o = ((size_t)b * 2 + c) * M;
            good = cmpc_force_sample_time_foot(t + 2 * o, n[2 * b + c], dt_ns, out_t + 2 * o) && good;
            if (out_t != t) std::memcpy(out_t + 2 * (o + n[2 * b + c]), t + 2 * (o + n[2 * b + c]), sizeof(double) * 2 * (M - n[2 * b + c]));
        }
        if (ok) ok[b] = good ? 1 : 0;
        if (!good) all = CMPC_ERR_ARG;
    }
    if (all != CMPC_OK) return fail(nullptr, CMPC_ERR_ARG, "cmpc_contacts_force_sample_time: a time is not finite or a contact collapses on the grid");
    return CMPC_OK;
}

int cmpc_contacts_force_sample_time_device(cmpc_handle h, int max_contacts, double dt, const double* dT, const int* dN, double* dOutT, int* dOk, void* stream)
{
    const long long dt_ns = snap_dt_ns(dt);
    if (!h || max_contacts < 1 || dt_ns < 1 || !dT || !dN || !dOutT) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_force_sample_time_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_force_sample_time(h->B, max_contacts, dt_ns, dT, dN, dOutT, dOk, 0, nullptr, stream_of(h, stream));
    return launch_status(h, "forceSampleTime", rc);
}

// ---- adjoint of the list path in the contacts' positions (include/cmpc.h; cmpc_contacts_position_vjp_kernel) ----
int cmpc_contacts_position_vjp_device(cmpc_handle h, int max_contacts, double now, int phase, int force_sample_time, const double* dPlanT, const int* dPlanN,
                                      const double* dPrevT, const int* dPrevN, const double* dListT, const int* dListN, const int* dLand, const int* dOk,
                                      const double* dGradListOut, const float* dGradP, float* dGradX, double* dGradPrevList, double* dGradPlan, int* dStatus,
                                      void* stream)
{
    if (!h || max_contacts < 1 || phase < 1 || phase > 3 || !dListT || !dListN) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_position_vjp_device: bad argument");
    const bool merge = dPrevT || dPrevN;
    if (merge && (!dPrevT || !dPrevN || !dPlanT || !dPlanN))
        return fail(h, CMPC_ERR_ARG, "cmpc_contacts_position_vjp_device: a merge tick needs the planner's and the previous tick's times and counts");
    if ((phase & 1) && (!dGradX || !dLand)) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_position_vjp_device: the adjust part needs dGradX and dLand");
    if ((phase & 2) && !dGradPrevList) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_position_vjp_device: the sample + merge part needs dGradPrevList");
    long long dt_ns = 0;
    if (force_sample_time) {
        dt_ns = snap_dt_ns(h->cfg.sampling_time);
        if (dt_ns < 1) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_position_vjp_device: force_sample_time needs a sampling time of at least 1 ns");
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_contacts_position_vjp(h->B, h->cfg.horizon, max_contacts, h->cfg.sampling_time, now, phase, dt_ns, dPlanT, dPlanN, dPrevT, dPrevN, dListT,
                                               dListN, dLand, dOk, dGradListOut, dGradP, dGradX, dGradPrevList, dGradPlan, dStatus,
                                               stream_of(h, stream));
    return launch_status(h, "contact position VJP", rc);
}

// ---- ... and in their orientations (include/cmpc.h; cmpc_contacts_orientation_vjp_kernel) ----
int cmpc_contacts_orientation_vjp_device(cmpc_handle h, int max_contacts, double now, int force_sample_time, const double* dPlanT, const int* dPlanN,
                                         const double* dPrevT, const int* dPrevN, const double* dListT, const int* dListN, const int* dLand, const int* dOk,
                                         const double* dGradListRotOut, const double* dGradRot, double* dGradPrevListRot, double* dGradPlanRot, int* dStatus,
                                         void* stream)
{
    if (!h || max_contacts < 1 || !dListT || !dListN || !dGradPrevListRot) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_orientation_vjp_device: bad argument");
    const bool merge = dPrevT || dPrevN;
    if (merge && (!dPrevT || !dPrevN || !dPlanT || !dPlanN))
        return fail(h, CMPC_ERR_ARG, "cmpc_contacts_orientation_vjp_device: a merge tick needs the planner's and the previous tick's times and counts");
    long long dt_ns = 0;
    if (force_sample_time) {
        dt_ns = snap_dt_ns(h->cfg.sampling_time);
        if (dt_ns < 1) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_orientation_vjp_device: force_sample_time needs a sampling time of at least 1 ns");
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_contacts_orientation_vjp(h->B, h->cfg.horizon, max_contacts, h->cfg.sampling_time, now, dt_ns, dPlanT, dPlanN, dPrevT, dPrevN, dListT,
                                                  dListN, dLand, dOk, dGradListRotOut, dGradRot, dGradPrevListRot, dGradPlanRot, dStatus,
                                                  stream_of(h, stream));
    return launch_status(h, "contact orientation VJP", rc);
}

// the bounding boxes of the two contacts on the device (uploaded when they change)
static int upload_box(cmpc_handle h, const float* box_upper, const float* box_lower, hipStream_t st)
{
    float box[12];
    std::memcpy(box, box_upper, sizeof(float) * 6);
    std::memcpy(box + 6, box_lower, sizeof(float) * 6);
    if (!h->box_set || std::memcmp(box, h->hBox, sizeof(box)) != 0) {
        std::memcpy(h->hBox, box, sizeof(box));
        HIPCHK(h, hipMemcpyAsync(h->dBox, h->hBox, sizeof(box), hipMemcpyHostToDevice, st));
        h->box_set = true;
    }
    return CMPC_OK;
}

int cmpc_contacts_sample_device(cmpc_handle h, int max_contacts, double now, const double* dT, const float* dPose, const int* dN,
                                const float* box_upper, const float* box_lower, float* dP, int* dLand, void* stream)
{
    if (!h || max_contacts < 1 || !dT || !dPose || !dN || !box_upper || !box_lower || !dP) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_sample_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    int rc = upload_box(h, box_upper, box_lower, st);
    if (rc != CMPC_OK) return rc;
    rc = cmpc_launch_contacts_sample(h->B, h->cfg.horizon, max_contacts, h->cfg.sampling_time, now, dT, dPose, dN, h->dBox, dP, dLand, st);
    return launch_status(h, "contact sampling", rc);
}

int cmpc_contacts_adjust_device(cmpc_handle h, int max_contacts, double now, const float* dX, const int* dLand, const double* dT, float* dPose,
                                const int* dN, void* stream)
{
    if (!h || max_contacts < 1 || !dX || !dLand || !dT || !dPose || !dN) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_adjust_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_contacts_adjust(h->B, h->cfg.horizon, max_contacts, now, dX, dLand, dT, dPose, dN, stream_of(h, stream));
    return launch_status(h, "contact adjustment", rc);
}

int cmpc_write_state_device(cmpc_handle h, const float* dState, const float* dWrench, float* dP, void* stream)
{
    if (!h || !dState || !dP) return fail(h, CMPC_ERR_ARG, "cmpc_write_state_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_write_state(h->B, h->cfg.horizon, dState, dWrench, dP, stream_of(h, stream));
    return launch_status(h, "state write", rc);
}

int cmpc_shift_solution_device(cmpc_handle h, const float* dXprev, float* dX0, void* stream)
{
    if (!h || !dXprev || !dX0) return fail(h, CMPC_ERR_ARG, "cmpc_shift_solution_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    CmpcParams p;
    fill_params(h, p);
    int rc = cmpc_launch_warm_shift(&p, dXprev, dX0, stream_of(h, stream));
    if (rc != 0) return fail(h, CMPC_ERR_HIP, "warm-start shift launch failed");
    return CMPC_OK;   // (no state on the handle: the caller solves from dX0 with cmpc_solve_device_warm)
}

// ---- 8f-1 .. 8f-4 chained: one tick of the receding-horizon loop in one call (include/cmpc.h): the steps of the entry points above in the reference's order, with the
// same argument checks, as THREE launches -- everything in front of the solve, the solve, everything behind it (cmpc_tick_pre_kernel / cmpc_tick_post_kernel call the same
// per-problem functions as the single kernels; results identical to the last bit). ----
// cold: the solve starts from cmpc_cold_start_kernel, launched between the front kernel and the solve (the first tick of cmpc_rollout_walk_device; needs
// warm == 0).  box_done: the caller has uploaded the box already.
// m: the plant mismatch (include/cmpc.h, cmpc_plant_mismatch) with `tick` selecting its rows, or null -- then every launch is the one this function always queued
static int mismatch_check(cmpc_handle h, const char* who, const cmpc_plant_mismatch* m)
{
    if (m && (m->hidden_ticks < 0 || m->noise_ticks < 0 || (m->dHiddenWrench && m->hidden_ticks == 0) || (m->dStateNoise && m->noise_ticks == 0)))
        return fail(h, CMPC_ERR_ARG, std::string(who) + ": bad mismatch (a negative count, or a schedule with no rows)");
    return CMPC_OK;
}

// the rows of tick number `tick`: a schedule's row inside its range, else null (the term is then not applied: a select on the host, no add of zero)
static void mismatch_rows(const cmpc_plant_mismatch* m, int B, int tick, const float** hidden, const float** noise, const float** gain)
{
    *hidden = nullptr; *noise = nullptr; *gain = nullptr;
    if (!m) return;
    const long long r = (long long)tick - m->tick_first;
    if (m->dHiddenWrench && r >= 0 && r < m->hidden_ticks) *hidden = m->dHiddenWrench + (size_t)r * B * 6;
    if (m->dStateNoise && r >= 0 && r < m->noise_ticks) *noise = m->dStateNoise + (size_t)r * B * 9;
    *gain = m->dForceGain;
}

static int rollout_tick_impl(cmpc_handle h, int max_contacts, double now, int warm, const cmpc_tick_io* io, void* stream, bool cold, bool box_done,
                             int tick = 0, const cmpc_plant_mismatch* m = nullptr)
{
    if (!h || !io) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_device: null argument");
    if (m && tick < 0) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_mismatch_device: negative tick number");
    {
        const int mrc = mismatch_check(h, "cmpc_rollout_tick_mismatch_device", m);
        if (mrc != CMPC_OK) return mrc;
    }
    const float *mm_hidden, *mm_noise, *mm_gain;
    mismatch_rows(m, h->B, tick, &mm_hidden, &mm_noise, &mm_gain);
    if (!io->dLand || !io->dInfo) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_device: dLand and dInfo are needed");
    const bool merge = io->dPrevT || io->dPrevPose || io->dPrevN;
    if (merge && (io->dPrevT == io->dListT || io->dPrevPose == io->dListPose || io->dPrevN == io->dListN))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_device: the merged lists must not alias the previous tick's");
    if (merge && (!io->dPlanT || !io->dPlanPose || !io->dPlanN || !io->dPrevT || !io->dPrevPose || !io->dPrevN))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_device: the merge needs the planner's and the previous tick's lists");
    if (max_contacts < 1 || !io->dListT || !io->dListPose || !io->dListN || !io->box_upper || !io->box_lower || !io->dState || !io->dP || !io->dX0 || !io->dX ||
        !io->dStateOut || !(io->plant_step > 0) || io->plant_substeps < 1)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_device: bad argument");
    if ((io->dPlanCom || io->dPlanH) && (!io->dPlanCom || !io->dPlanH || io->plan_knots < 2 || !(io->plan_dt > 0) || !(io->robot_mass > 0)))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_device: bad planner trajectory");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    const int* const ended = h->dEnded;   // cmpc_set_ended_device: every launch of the tick leaves out the problems it names (the solve reads it through fill_params)
    long long dt_ns = 0;
    if (io->force_sample_time) {
        dt_ns = snap_dt_ns(h->cfg.sampling_time);
        if (dt_ns < 1) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_device: force_sample_time needs a sampling time of at least 1 ns");
    }
    int rc = box_done ? CMPC_OK : upload_box(h, io->box_upper, io->box_lower, st);
    if (rc != CMPC_OK) return rc;
    // forceSampleTime: inside the front kernel when the lists fit its LDS stage (cmpc_tick_pre_kernel, M <= 16); else one launch of the standalone kernel
    // in front of it -- the planner's lists into the handle's dSnapT (merge ticks) or the caller's lists in place (first tick), per-foot status into dSnapOk
    const double* plan_t = io->dPlanT;
    const int* snap_ok = nullptr;
    if (dt_ns > 0 && max_contacts > 16) {
        const size_t need = (size_t)h->B * 2 * max_contacts * 2;
        if (merge && need > h->snap_cap) {
            HIPCHK(h, hipStreamSynchronize(st));
            hipFree(h->dSnapT);
            h->dSnapT = nullptr; h->snap_cap = 0;
            HIPCHK(h, hipMalloc(&h->dSnapT, sizeof(double) * need));
            h->snap_cap = need;
        }
        if (!h->dSnapOk) HIPCHK(h, hipMalloc(&h->dSnapOk, sizeof(int) * 2 * (size_t)h->B));
        const int lrc = merge ? cmpc_launch_force_sample_time(h->B, max_contacts, dt_ns, io->dPlanT, io->dPlanN, h->dSnapT, h->dSnapOk, 1, ended, st)
                              : cmpc_launch_force_sample_time(h->B, max_contacts, dt_ns, io->dListT, io->dListN, io->dListT, h->dSnapOk, 1, ended, st);
        if (const int err = launch_status(h, "tick (forceSampleTime)", lrc)) return err;
        if (merge) plan_t = h->dSnapT;
        snap_ok = h->dSnapOk;
    }
    int lrc = cmpc_launch_tick_pre(h->B, h->cfg.horizon, max_contacts, h->cfg.sampling_time, now, merge ? 1 : 0, plan_t, io->dPlanPose, io->dPlanN, io->dPrevT,
                                   io->dPrevPose, io->dPrevN, io->dListT, io->dListPose, io->dListN, io->dOk, io->dLand, h->dBox, io->dState, io->dWrench, io->dP,
                                   warm ? io->dX : nullptr, io->dX0, io->dPlanCom, io->dPlanH, io->plan_knots, io->plan_dt, io->plan_t_offset, io->robot_mass,
                                   io->com_height, dt_ns, snap_ok, ended, mm_noise, st);
    if (const int err = launch_status(h, "tick (front)", lrc)) return err;
    if (cold) {
        lrc = cmpc_launch_cold_start(h->cfg.horizon, h->B, (float)(h->cfg.gravity / 8.0), io->dP, io->dX0, ended, st);
        if (const int err = launch_status(h, "tick (cold start)", lrc)) return err;
    }
    rc = solve_device_impl(h, io->dP, io->dX0, io->dX, io->dInfo, stream, warm != 0);
    if (rc != CMPC_OK) return rc;
    lrc = cmpc_launch_tick_post(h->B, h->cfg.horizon, max_contacts, now, (float)h->cfg.gravity, model_corners(h), corners_stride(h), io->dX, io->dP, io->dState, io->dStateOut, io->dZmp,
                                (float)io->plant_step, io->plant_substeps, (float)io->zmp_half_x, (float)io->zmp_half_y, io->dLand, io->dListT, io->dListPose,
                                io->dListN, ended, mm_hidden, mm_gain, st);
    return launch_status(h, "tick (back)", lrc);
}

int cmpc_rollout_tick_device(cmpc_handle h, int max_contacts, double now, int warm, const cmpc_tick_io* io, void* stream)
{
    return rollout_tick_impl(h, max_contacts, now, warm, io, stream, false, false);
}

int cmpc_rollout_tick_mismatch_device(cmpc_handle h, int max_contacts, double now, int warm, const cmpc_tick_io* io, int tick, const cmpc_plant_mismatch* m,
                                      void* stream)
{
    return rollout_tick_impl(h, max_contacts, now, warm, io, stream, false, false, tick, m);
}

// ---- the walk (include/cmpc.h): the record behind a tick, the cold start as a kernel, and `ticks` ticks queued in one call ----
static bool record_args(int N, int B, int tick, int row, const float* X, const float* P, const float* info, const int* ok, const int* land,
                        const float* state_out, const float* zmp, const float* box, const cmpc_walk_record* rec, CmpcRecordArgs& a)
{
    if (N < 1 || B < 1 || !X || !P || !info || !land || !state_out || !box || !rec || row < 0 || row >= rec->rows || (rec->dZmp && !zmp)) return false;
    if (!rec->dEndTick || !rec->dEndCode || !rec->dIterationsSum || !rec->dIterationsMax || !rec->dFinalState || !rec->dBoxSlackMin) return false;
    a = CmpcRecordArgs{N, B, tick, row, rec->stop_mask, X, P, info, ok, land, state_out, zmp, box, rec->dCom, rec->dZmp, rec->dLand, rec->dLandingOffset,
                       rec->dIterations, rec->dCode, rec->dEndTick, rec->dEndCode, rec->dIterationsSum, rec->dIterationsMax, rec->dFinalState,
                       rec->dBoxSlackMin};
    return true;
}

int cmpc_rollout_record(int horizon, int batch, int tick, int row, const float* X, const float* P, const float* info, const int* ok, const int* land,
                        const float* state_out, const float* zmp, const float* box_upper, const float* box_lower, const cmpc_walk_record* rec)
{
    float box[12];
    CmpcRecordArgs a;
    if (!box_upper || !box_lower || !record_args(horizon, batch, tick, row, X, P, info, ok, land, state_out, zmp, box, rec, a))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_record: bad argument");
    std::memcpy(box, box_upper, sizeof(float) * 6);
    std::memcpy(box + 6, box_lower, sizeof(float) * 6);
    int st[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < batch; ++b) {
        int t[5];
        cmpc_record_problem<false>(a, CmpcLimitArgs{}, b, t);
        st[0] += t[0]; st[1] += t[1]; st[2] += t[2]; st[3] = std::max(st[3], t[3]); st[4] += t[4];
    }
    if (rec->dStats) std::memcpy(rec->dStats + 6 * (size_t)row, st, sizeof(st));
    return CMPC_OK;
}

// the limits as the record takes them, row `row` of the measures trace
static CmpcLimitArgs limit_args(const cmpc_walk_limits& lim, int B, int row, const float* corners, int stride, double gravity)
{
    return CmpcLimitArgs{lim.height_min, lim.height_max, lim.reach_max, lim.margin_min, lim.track_max, gravity, corners, stride,
                         lim.dMeasures ? lim.dMeasures + (size_t)row * B * CMPC_WALK_MEASURES : nullptr, lim.dExtremes};
}

int cmpc_rollout_record_limits(int horizon, int batch, int tick, int row, const float* X, const float* P, const float* info, const int* ok, const int* land,
                               const float* state_out, const float* zmp, const float* box_upper, const float* box_lower, const cmpc_walk_record* rec,
                               const cmpc_walk_limits* lim, const float* corners, int corners_stride, double gravity)
{
    if (!lim) return cmpc_rollout_record(horizon, batch, tick, row, X, P, info, ok, land, state_out, zmp, box_upper, box_lower, rec);
    float box[12];
    CmpcRecordArgs a;
    if (!box_upper || !box_lower || !record_args(horizon, batch, tick, row, X, P, info, ok, land, state_out, zmp, box, rec, a))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_record_limits: bad argument");
    if (horizon < 2 || !corners || corners_stride < 0 || !(gravity > 0)) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_record_limits: bad argument");
    if (const char* why = limits_refusal(lim)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_rollout_record_limits: ") + why);
    if (lim->dMeasures && row >= lim->rows) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_record_limits: the measures trace has too few rows");
    std::memcpy(box, box_upper, sizeof(float) * 6);
    std::memcpy(box + 6, box_lower, sizeof(float) * 6);
    const CmpcLimitArgs lm = limit_args(*lim, batch, row, corners, corners_stride, gravity);
    int st[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < batch; ++b) {
        int t[6];
        cmpc_record_problem<true>(a, lm, b, t);
        st[0] += t[0]; st[1] += t[1]; st[2] += t[2]; st[3] = std::max(st[3], t[3]); st[4] += t[4]; st[5] += t[5];
    }
    if (rec->dStats) std::memcpy(rec->dStats + 6 * (size_t)row, st, sizeof(st));
    return CMPC_OK;
}

// the record launch behind a tick: without limits the launch it has always been, with them (cmpc_set_walk_limits) the kernel that also evaluates them,
// on the corners the plant kernel reads
static int record_launch(cmpc_handle h, const char* who, const CmpcRecordArgs& a, int* stats, hipStream_t st)
{
    if (!h->limits_set) return launch_status(h, who, cmpc_launch_rollout_record(&a, stats, st));
    if (h->limits.dMeasures && a.row >= h->limits.rows)
        return fail(h, CMPC_ERR_ARG, std::string(who) + ": the measures trace of cmpc_set_walk_limits has too few rows");
    const CmpcLimitArgs lm = limit_args(h->limits, a.B, a.row, model_corners(h), corners_stride(h), h->cfg.gravity);
    return launch_status(h, who, cmpc_launch_rollout_record_limits(&a, &lm, stats, st));
}

// the record launch of one tick; clear_row: the statistics row is cleared here (the walk clears all its rows at once)
static int rollout_record_impl(cmpc_handle h, int tick, int row, const float* dX, const float* dP, const float* dInfo, const int* dOk, const int* dLand,
                               const float* dStateOut, const float* dZmp, const cmpc_walk_record* rec, hipStream_t st, bool clear_row)
{
    CmpcRecordArgs a;
    if (!h || !h->box_set || !record_args(h->cfg.horizon, h->B, tick, row, dX, dP, dInfo, dOk, dLand, dStateOut, dZmp, h->dBox, rec, a))
        return fail(h, CMPC_ERR_ARG, h && !h->box_set ? "cmpc_rollout_record_device: the handle has no box yet (a sampling or a tick uploads it)"
                                                      : "cmpc_rollout_record_device: bad argument");
    int* stats = rec->dStats ? rec->dStats + 6 * (size_t)row : nullptr;
    if (stats && clear_row) HIPCHK(h, hipMemsetAsync(stats, 0, sizeof(int) * 6, st));
    return record_launch(h, "roll-out record", a, stats, st);
}

int cmpc_walk_extremes_init_device(cmpc_handle h, float* dExtremes, void* stream)
{
    if (!h || !dExtremes) return fail(h, CMPC_ERR_ARG, "cmpc_walk_extremes_init_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_extremes_init(h->B, dExtremes, stream_of(h, stream));
    return launch_status(h, "extremes init", lrc);
}

// ---- the measures differentiated (include/cmpc.h): the host forms run the kernels' own per-entry functions ----
static bool measures_rows_ok(int horizon, int batch, int tick0, int rows, const float* X, const float* P, const float* states, const float* corners,
                             int corners_stride, double gravity)
{
    return horizon >= 2 && batch >= 1 && tick0 >= 0 && rows >= 1 && X && P && states && corners && corners_stride >= 0 && gravity > 0;
}

int cmpc_walk_measures_vjp(int horizon, int batch, int tick0, int rows, const float* X, const float* P, const float* states, const int* end_tick,
                           const float* corners, int corners_stride, double gravity, const double* grad_measures, double* grad_states, float* grad_X,
                           double* direct)
{
    if (!measures_rows_ok(horizon, batch, tick0, rows, X, P, states, corners, corners_stride, gravity) || !grad_measures || !grad_states || !grad_X || !direct)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_walk_measures_vjp: bad argument");
    const CmpcMeasureVjpArgs v{horizon, batch, tick0, rows, X, P, states, end_tick, corners, corners_stride, gravity, grad_measures, grad_states, grad_X, direct};
    for (int r = 0; r < rows; ++r)
        for (int b = 0; b < batch; ++b) cmpc_walk_measures_vjp_entry(v, r, b);
    return CMPC_OK;
}

int cmpc_walk_measures_vjp_fold(int horizon, int batch, int rows, const double* direct, float* grad_P, double* grad_model)
{
    if (horizon < 2 || batch < 1 || rows < 1 || !direct) return fail(nullptr, CMPC_ERR_ARG, "cmpc_walk_measures_vjp_fold: bad argument");
    const size_t np = (size_t)rows * batch, nm = (size_t)24 * batch;
    for (size_t e = 0; e < (np > nm ? np : nm); ++e) cmpc_walk_measures_fold_entry(horizon, batch, rows, direct, grad_P, grad_model, e);
    return CMPC_OK;
}

int cmpc_walk_measures_jvp(int horizon, int batch, int tick0, int rows, int k, const float* X, const float* P, const float* states, const int* end_tick,
                           const float* corners, int corners_stride, double gravity, const double* dir_states, const float* dir_X, const float* dir_P,
                           const double* dir_model, double* dir_measures)
{
    if (!measures_rows_ok(horizon, batch, tick0, rows, X, P, states, corners, corners_stride, gravity) || k < 1 || !dir_states || !dir_X || !dir_measures)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_walk_measures_jvp: bad argument");
    const CmpcMeasureJvpArgs v{horizon, batch, tick0, rows, k, X, P, states, end_tick, corners, corners_stride, gravity, dir_states, dir_X, dir_P, dir_model,
                               dir_measures};
    for (int r = 0; r < rows; ++r)
        for (int b = 0; b < batch; ++b) cmpc_walk_measures_jvp_entry(v, r, b);
    return CMPC_OK;
}

int cmpc_walk_measures_jacobian(int horizon, int batch, int rows, const float* X, const float* P, const float* states, const float* corners,
                                int corners_stride, double gravity, double* jacobian)
{
    if (!measures_rows_ok(horizon, batch, 0, rows, X, P, states, corners, corners_stride, gravity) || !jacobian)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_walk_measures_jacobian: bad argument");
    const int nx = 45 * horizon + 15, np = CmpcIdx{horizon}.np();
    for (int r = 0; r < rows; ++r) {
        const CmpcMeasureArgs a{horizon, batch, X + (size_t)r * batch * nx, P + (size_t)r * batch * np, states + (size_t)(r + 1) * batch * 9, corners,
                                corners_stride, gravity};
        for (int b = 0; b < batch; ++b)
            for (int m = 0; m < 4; ++m) {   // row m: the VJP of the unit cotangent e_m (products with 1.0 and sums with 0.0 are exact)
                double w[4] = {0.0, 0.0, 0.0, 0.0}, gs[5], gq[6], d[32];
                w[m] = 1.0;
                cmpc_walk_measures_vjp_problem(a, b, w, gs, gq, d);
                double* J = jacobian + (((size_t)r * batch + b) * 4 + m) * CMPC_WALK_MEASURE_INPUTS;
                for (int i = 0; i < 3; ++i) J[i] = gs[i];
                J[3] = gs[3]; J[4] = gs[4]; J[5] = 0.0;
                for (int i = 0; i < 6; ++i) J[6 + i] = gq[i];
                for (int i = 0; i < 6; ++i) J[12 + i] = d[2 + i];
                for (int i = 0; i < 24; ++i) J[18 + i] = d[8 + i];
                J[42] = d[0]; J[43] = d[1];
            }
    }
    return CMPC_OK;
}

// the rows of a call inside the tape, and the tape arrays the measures read
static const char* measures_tape_refusal(cmpc_handle h, int tick0, int ticks, const cmpc_walk_tape* tape, int row0)
{
    if (!h || !tape || !tape->dX || !tape->dP || !tape->dStates) return "null argument or incomplete tape";
    if (h->cfg.horizon < 2) return "the measures refer to stage 1: the horizon must be at least 2";
    if (tick0 < 0 || ticks < 1 || row0 < 0 || (long long)row0 + ticks > tape->rows) return "bad argument (the rows must lie inside the tape)";
    return nullptr;
}

int cmpc_walk_measures_vjp_device(cmpc_handle h, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                  const cmpc_walk_measure_grads* g, void* stream)
{
    if (const char* why = measures_tape_refusal(h, tick0, ticks, tape, row0)) return fail(h, CMPC_ERR_ARG, std::string("cmpc_walk_measures_vjp_device: ") + why);
    if (!g || !g->dGradMeasures || !g->dGradStates || !g->dGradX || !g->dDirect)
        return fail(h, CMPC_ERR_ARG, "cmpc_walk_measures_vjp_device: dGradMeasures, dGradStates, dGradX and dDirect are needed");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t B = (size_t)h->B, r0 = (size_t)row0;
    const CmpcMeasureVjpArgs v{h->cfg.horizon, h->B, tick0, ticks, tape->dX + r0 * B * h->L.nx, tape->dP + r0 * B * h->L.np, tape->dStates + r0 * B * 9,
                               dEndTick, model_corners(h), corners_stride(h), h->cfg.gravity, g->dGradMeasures + r0 * B * CMPC_WALK_MEASURES,
                               g->dGradStates + r0 * B * 9, g->dGradX + r0 * B * h->L.nx, g->dDirect + r0 * B * CMPC_WALK_MEASURE_DIRECT};
    return launch_status(h, "measures VJP", cmpc_launch_walk_measures_vjp(&v, stream_of(h, stream)));
}

int cmpc_walk_measures_vjp_fold_device(cmpc_handle h, int rows, const double* dDirect, float* dGradP, double* dGradModel, void* stream)
{
    if (!h || !dDirect || rows < 1 || h->cfg.horizon < 2) return fail(h, CMPC_ERR_ARG, "cmpc_walk_measures_vjp_fold_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    return launch_status(h, "measures fold", cmpc_launch_walk_measures_fold(h->cfg.horizon, h->B, rows, dDirect, dGradP, dGradModel, stream_of(h, stream)));
}

int cmpc_walk_measures_jvp_device(cmpc_handle h, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick, int k,
                                  const cmpc_walk_measure_dirs* d, void* stream)
{
    if (const char* why = measures_tape_refusal(h, tick0, ticks, tape, row0)) return fail(h, CMPC_ERR_ARG, std::string("cmpc_walk_measures_jvp_device: ") + why);
    if (k < 1 || !d || !d->dDirStates || !d->dDirX || !d->dDirMeasures)
        return fail(h, CMPC_ERR_ARG, "cmpc_walk_measures_jvp_device: k >= 1, dDirStates, dDirX and dDirMeasures are needed");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t B = (size_t)h->B, r0 = (size_t)row0, K = (size_t)k;
    const CmpcMeasureJvpArgs v{h->cfg.horizon, h->B, tick0, ticks, k, tape->dX + r0 * B * h->L.nx, tape->dP + r0 * B * h->L.np, tape->dStates + r0 * B * 9,
                               dEndTick, model_corners(h), corners_stride(h), h->cfg.gravity, d->dDirStates + r0 * B * K * 9, d->dDirX + r0 * B * K * h->L.nx,
                               d->dDirP ? d->dDirP + r0 * B * K * h->L.np : nullptr, d->dDirModel, d->dDirMeasures + r0 * B * K * CMPC_WALK_MEASURES};
    return launch_status(h, "measures JVP", cmpc_launch_walk_measures_jvp(&v, stream_of(h, stream)));
}

int cmpc_rollout_record_device(cmpc_handle h, int tick, int row, const float* dX, const float* dP, const float* dInfo, const int* dOk, const int* dLand,
                               const float* dStateOut, const float* dZmp, const cmpc_walk_record* rec, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_record_device: null handle");
    HIPCHK(h, hipSetDevice(h->device));
    return rollout_record_impl(h, tick, row, dX, dP, dInfo, dOk, dLand, dStateOut, dZmp, rec, stream_of(h, stream), true);
}

int cmpc_rollout_outcome_init_device(cmpc_handle h, const float* dState0, const cmpc_walk_record* rec, void* stream)
{
    if (!h || !dState0 || !rec || !rec->dEndTick || !rec->dEndCode || !rec->dIterationsSum || !rec->dIterationsMax || !rec->dFinalState || !rec->dBoxSlackMin)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_outcome_init_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_outcome_init(h->B, dState0, rec->dEndTick, rec->dEndCode, rec->dIterationsSum, rec->dIterationsMax, rec->dFinalState,
                                             rec->dBoxSlackMin, stream_of(h, stream));
    return launch_status(h, "outcome init", lrc);
}

int cmpc_cold_start_device(cmpc_handle h, const float* dP, float* dX0, void* stream)
{
    if (!h || !dP || !dX0) return fail(h, CMPC_ERR_ARG, "cmpc_cold_start_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_cold_start(h->cfg.horizon, h->B, (float)(h->cfg.gravity / 8.0), dP, dX0, h->dEnded, stream_of(h, stream));
    return launch_status(h, "cold start", lrc);
}

// ---- the device tape (include/cmpc.h, cmpc_walk_tape): one row from what a tick left ----
static bool tape_complete(const cmpc_walk_tape* t)
{
    return t && t->rows >= 1 && t->dX && t->dP && t->dLamG && t->dInfo && t->dStates && t->dOk && t->dLand && t->dPlanT && t->dListT && t->dPlanN && t->dListN &&
           t->plant_step > 0 && t->plant_substeps >= 1;
}

static int rollout_tape_impl(cmpc_handle h, int max_contacts, int row, int parts, const float* dX, const float* dP, const float* dInfo, const int* dOk,
                             const int* dLand, const float* dStateIn, const float* dStateOut, const double* dPlanT, const int* dPlanN, const double* dListT,
                             const int* dListN, const cmpc_walk_tape* tape, void* stream)
{
    if (!h || !tape_complete(tape) || max_contacts < 1 || row < 0 || row >= tape->rows || parts < 1 || parts > 3)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tape_device: bad argument");
    if (((parts & 1) && !dStateIn) || ((parts & 2) && (!dX || !dP || !dInfo || !dLand || !dStateOut || !dListT || !dListN || (!dPlanT != !dPlanN))))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tape_device: null argument");
    if (parts == 3 && dStateIn == dStateOut)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tape_device: a tick that ran in place needs part 1 in front of it");
    if ((parts & 2) && (!h->mult_out || !h->dDuals))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tape_device: the multiplier output is off (cmpc_set_multiplier_output before the ticks)");
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, stream);
    const CmpcTapeArgs a{h->B, max_contacts, h->L.nx, h->L.np, row, parts, dX, dP, dInfo, dOk, dLand, dStateIn, dStateOut, dPlanT, dPlanN, dListT, dListN,
                         tape->dX, tape->dP, tape->dInfo, tape->dStates, tape->dOk, tape->dLand, tape->dPlanT, tape->dListT, tape->dPlanN, tape->dListN};
    const int lrc = cmpc_launch_rollout_tape(&a, st);
    if (const int err = launch_status(h, "roll-out tape", lrc)) return err;
    if (parts & 2) return cmpc_get_multipliers_device(h, dX, dP, tape->dLamG + (size_t)row * h->B * h->L.ng, stream);
    return CMPC_OK;
}

int cmpc_rollout_tape_device(cmpc_handle h, int max_contacts, int row, int parts, const float* dX, const float* dP, const float* dInfo, const int* dOk,
                             const int* dLand, const float* dStateIn, const float* dStateOut, const double* dPlanT, const int* dPlanN, const double* dListT,
                             const int* dListN, const cmpc_walk_tape* tape, void* stream)
{
    return rollout_tape_impl(h, max_contacts, row, parts, dX, dP, dInfo, dOk, dLand, dStateIn, dStateOut, dPlanT, dPlanN, dListT, dListN, tape, stream);
}

static int rollout_walk_impl(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                             int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream,
                             const cmpc_plant_mismatch* m = nullptr);

int cmpc_rollout_walk_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                             int row0, int lists_in, int* lists_out, void* stream)
{
    return rollout_walk_impl(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, nullptr, 0, stream);
}

static int walk_taped(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                      int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream, const cmpc_plant_mismatch* m)
{
    if (!h || !io || !tape_complete(tape)) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_taped_device: null argument or incomplete tape");
    if (ticks < 1 || tape_row0 < 0 || (long long)tape_row0 + ticks > tape->rows)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_taped_device: the tape has too few rows");
    if (tape->plant_step != io->tick.plant_step || tape->plant_substeps != io->tick.plant_substeps ||
        (tape->force_sample_time != 0) != (io->tick.force_sample_time != 0) ||
        (tape_row0 == 0 ? (tape->first_row_is_first_tick != 0) != (cold_first != 0) : cold_first != 0))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_taped_device: the tape's scalars do not agree with the walk (or a first tick beyond row 0)");
    if (!h->mult_out || !h->dDuals)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_taped_device: the multiplier output is off (cmpc_set_multiplier_output before the walk)");
    return rollout_walk_impl(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, tape, tape_row0, stream, m);
}

int cmpc_rollout_walk_taped_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                   int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream)
{
    return walk_taped(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, tape, tape_row0, stream, nullptr);
}

int cmpc_rollout_walk_mismatch_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                      int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, const cmpc_plant_mismatch* m,
                                      void* stream)
{
    if (tape) return walk_taped(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, tape, tape_row0, stream, m);
    return rollout_walk_impl(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, nullptr, 0, stream, m);
}

// tape != null: the tape part around the ticks (cmpc_rollout_walk_taped_device, which has checked it); null: the launches of cmpc_rollout_walk_device
// m: the plant mismatch, every tick passing its own number tick0 + i (no launch more per tick, nothing more on the tape: dStates holds the true state, dP the measured one)
static int rollout_walk_impl(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                             int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream, const cmpc_plant_mismatch* m)
{
    if (!h || !io) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_device: null argument");
    {
        const int mrc = mismatch_check(h, "cmpc_rollout_walk_mismatch_device", m);
        if (mrc != CMPC_OK) return mrc;
    }
    if (ticks < 1 || tick0 < 0 || lists_in < 0 || lists_in > 1 || !io->dListTB || !io->dListPoseB || !io->dListNB || !io->tick.dListT || !io->tick.dListPose ||
        !io->tick.dListN || !io->tick.box_upper || !io->tick.box_lower || !io->tick.dState || !io->tick.dStateOut || (io->dWrenchTicks && io->wrench_ticks < 1))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_device: bad argument");
    if (io->dListTB == io->tick.dListT || io->dListPoseB == io->tick.dListPose || io->dListNB == io->tick.dListN)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_device: the two sets of list buffers must not alias");
    if (rec && (row0 < 0 || (long long)row0 + ticks > rec->rows)) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_device: the record has too few rows");
    if (rec && h->limits_set && h->limits.dMeasures && (long long)row0 + ticks > h->limits.rows)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_device: the measures trace of cmpc_set_walk_limits has too few rows");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    int rc = upload_box(h, io->tick.box_upper, io->tick.box_lower, st);
    if (rc != CMPC_OK) return rc;
    if (rec && rec->dStats) HIPCHK(h, hipMemsetAsync(rec->dStats + 6 * (size_t)row0, 0, sizeof(int) * 6 * (size_t)ticks, st));
    const bool timing = h->timing;   // (an event record is a barrier packet on the stream: cmpc_set_timing)
    h->timing = false; h->timed = false;
    double* const set_t[2] = {io->tick.dListT, io->dListTB};
    float* const set_p[2] = {io->tick.dListPose, io->dListPoseB};
    int* const set_n[2] = {io->tick.dListN, io->dListNB};
    const size_t wrench_row = (size_t)h->B * h->cfg.horizon * 6;
    int cur = lists_in;
    rc = CMPC_OK;
    for (int i = 0; i < ticks && rc == CMPC_OK; ++i) {
        const bool cold = cold_first && i == 0;
        const double now = (double)(tick0 + i) * h->cfg.sampling_time;
        cmpc_tick_io t = io->tick;
        if (cold) {
            t.dPrevT = nullptr; t.dPrevPose = nullptr; t.dPrevN = nullptr;
        } else {
            t.dPrevT = set_t[cur]; t.dPrevPose = set_p[cur]; t.dPrevN = set_n[cur];
            cur = 1 - cur;
        }
        t.dListT = set_t[cur]; t.dListPose = set_p[cur]; t.dListN = set_n[cur];
        if (i > 0) t.dState = io->tick.dStateOut;
        if (io->dWrenchTicks) t.dWrench = i < io->wrench_ticks ? io->dWrenchTicks + wrench_row * i : nullptr;
        t.plan_t_offset = now - io->plan_t_first;
        const int* const ok_read = (cold && !t.force_sample_time) ? nullptr : t.dOk;
        if (tape && i == 0)   // (the ticks run in place: the state the first one starts from is copied in front of it)
            rc = rollout_tape_impl(h, max_contacts, tape_row0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, t.dState, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   tape, stream);
        if (rc == CMPC_OK) rc = rollout_tick_impl(h, max_contacts, now, cold ? 0 : 1, &t, stream, cold, true, tick0 + i, m);
        if (rc == CMPC_OK && rec)
            rc = rollout_record_impl(h, tick0 + i, row0 + i, t.dX, t.dP, t.dInfo, ok_read, t.dLand, t.dStateOut, t.dZmp, rec, st, false);
        if (rc == CMPC_OK && tape)
            rc = rollout_tape_impl(h, max_contacts, tape_row0 + i, 2, t.dX, t.dP, t.dInfo, ok_read, t.dLand, nullptr, t.dStateOut, cold ? nullptr : t.dPlanT,
                                   cold ? nullptr : t.dPlanN, t.dListT, t.dListN, tape, stream);
    }
    h->timing = timing;
    if (rc == CMPC_OK && lists_out) *lists_out = cur;
    return rc;
}

// ---- refill (include/cmpc.h, cmpc_walk_refill): the queue of trials behind a walk's slots ----
// the argument block of the per-slot functions; false: a required pointer is NULL or a count is out of range.  rec may be NULL for the init (no slot outcome).
static bool refill_args(int B, int tick_next, const cmpc_walk_record* rec, const cmpc_walk_refill* r, float* state_live, CmpcRefillArgs& a)
{
    if (B < 1 || tick_next < 0 || !r || r->trials < 0 || r->trial_ticks < 1 || !r->dStartTick || !r->dTrial || !r->dNext) return false;
    if (r->dWrenchTrials && r->wrench_ticks < 1) return false;
    if (r->trials > 0 && (!r->dState0 || !r->dTrialEndTick || !r->dTrialEndCode || !r->dTrialIterationsSum || !r->dTrialIterationsMax || !r->dTrialFinalState ||
                          !r->dTrialBoxSlackMin || !r->dTrialTicks || !r->dTrialSlot || !r->dTrialStart))
        return false;
    if (rec && (!rec->dEndTick || !rec->dEndCode || !rec->dIterationsSum || !rec->dIterationsMax || !rec->dFinalState || !rec->dBoxSlackMin)) return false;
    if (r->trace.dTrialOf && r->trace.rows < 1) return false;
    const long long row = (long long)tick_next - r->trace.tick_first;
    int* const trial_of = (r->trace.dTrialOf && row >= 0 && row < r->trace.rows) ? r->trace.dTrialOf + (size_t)row * B : nullptr;
    a = CmpcRefillArgs{B, r->trials, r->trial_ticks, tick_next, r->dStartTick, r->dTrial, r->dState0, r->dTrialEndTick, r->dTrialEndCode, r->dTrialIterationsSum,
                       r->dTrialIterationsMax, r->dTrialFinalState, r->dTrialBoxSlackMin, r->dTrialTicks, r->dTrialSlot, r->dTrialStart,
                       rec ? rec->dEndTick : nullptr, rec ? rec->dEndCode : nullptr, rec ? rec->dIterationsSum : nullptr, rec ? rec->dIterationsMax : nullptr,
                       rec ? rec->dFinalState : nullptr, rec ? rec->dBoxSlackMin : nullptr, state_live, trial_of};
    return true;
}

int cmpc_rollout_refill_init(int batch, const cmpc_walk_refill* refill)
{
    CmpcRefillArgs a;
    if (!refill_args(batch, 0, nullptr, refill, nullptr, a)) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill_init: bad argument");
    cmpc_refill_init_host(a, refill->dNext);
    return CMPC_OK;
}

int cmpc_rollout_refill_init_device(cmpc_handle h, const cmpc_walk_refill* refill, void* stream)
{
    CmpcRefillArgs a;
    if (!h || !refill_args(h->B, 0, nullptr, refill, nullptr, a)) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_refill_init_device: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_refill_init(&a, refill->dNext, stream_of(h, stream));
    return launch_status(h, "refill init", lrc);
}

int cmpc_rollout_refill(int batch, int tick_next, const cmpc_walk_record* rec, const cmpc_walk_refill* refill, float* state_live)
{
    CmpcRefillArgs a;
    if (!rec || !refill_args(batch, tick_next, rec, refill, state_live, a)) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill: bad argument");
    cmpc_refill_host(a, refill->dNext);
    return CMPC_OK;
}

static int rollout_refill_impl(cmpc_handle h, int tick_next, const cmpc_walk_record* rec, const cmpc_walk_refill* refill, float* dStateLive, hipStream_t st)
{
    CmpcRefillArgs a;
    if (!h || !rec || !refill_args(h->B, tick_next, rec, refill, dStateLive, a)) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_refill_device: bad argument");
    const int lrc = cmpc_launch_refill(&a, refill->dNext, st);
    return launch_status(h, "refill", lrc);
}

int cmpc_rollout_refill_device(cmpc_handle h, int tick_next, const cmpc_walk_record* rec, const cmpc_walk_refill* refill, float* dStateLive, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_refill_device: null handle");
    HIPCHK(h, hipSetDevice(h->device));
    return rollout_refill_impl(h, tick_next, rec, refill, dStateLive, stream_of(h, stream));
}

static int ensure_models(cmpc_handle h);
static_assert(sizeof(cmpc_walk_refill_plans) == 104, "cmpc_walk_refill_plans: the size include/cmpc.h states");
static_assert(sizeof(cmpc_walk_refill_trials) == 56, "cmpc_walk_refill_trials: the size include/cmpc.h states");
static_assert(sizeof(cmpc_walk_refill_snapshot) == 32, "cmpc_walk_refill_snapshot: the size include/cmpc.h states");

// ---- trials from a snapshot (include/cmpc.h, cmpc_walk_refill_snapshot): the restore step between the refill launch and the front kernel ----
static bool snapshot_args(int N, int B, int src_B, int M, const cmpc_walk_snapshot* s, const cmpc_walk_snapshot* d, const int* index, int* ok, CmpcSnapshotArgs& a);
// the 20 arrays of a cmpc_walk_snapshot in the struct's order
static void snapshot_pointers(const cmpc_walk_snapshot& s, const void* out[CMPC_SNAP_ARRAYS])
{
    const void* const p[CMPC_SNAP_ARRAYS] = {s.dState, s.dP, s.dX, s.dX0, s.dInfo, s.dZmp, s.dOk, s.dLand, s.dListT, s.dListPose, s.dListN, s.dListTB, s.dListPoseB,
                                             s.dListNB, s.dEndTick, s.dEndCode, s.dIterationsSum, s.dIterationsMax, s.dFinalState, s.dBoxSlackMin};
    for (int i = 0; i < CMPC_SNAP_ARRAYS; ++i) out[i] = p[i];
}
// the live buffers of a walk described as a snapshot: the state buffer the walk runs in place on, the record's outcome; prev: the set this tick reads
static cmpc_walk_snapshot walk_live_view(const cmpc_walk_io* io, const cmpc_walk_record* rec, int prev)
{
    const cmpc_tick_io& k = io->tick;
    return cmpc_walk_snapshot{0, prev, k.dStateOut, k.dP, k.dX, k.dX0, k.dInfo, k.dZmp, k.dOk, k.dLand, k.dListT, k.dListPose, k.dListN, io->dListTB,
                              io->dListPoseB, io->dListNB, rec->dEndTick, rec->dEndCode, rec->dIterationsSum, rec->dIterationsMax, rec->dFinalState,
                              rec->dBoxSlackMin};
}
// what is refused of `from` without a handle, in the header's order; null: nothing.  live (or null: not compared): the arrays a pool array must not be
static const char* restore_refusal(const cmpc_walk_refill_snapshot* from, int trials, const cmpc_walk_snapshot* live)
{
    const cmpc_walk_snapshot* pool = from->pool;
    if (!pool) return "pool is NULL";
    if (pool->tick < 1) return "pool->tick must be at least 1 (trials from tick 0 are cmpc_rollout_walk_refill_trials_device's)";
    if (from->pool_batch < 1) return "pool_batch must be at least 1";
    const void* sp[CMPC_SNAP_ARRAYS];
    snapshot_pointers(*pool, sp);
    for (int i = 0; i < CMPC_SNAP_ARRAYS; ++i)
        if (!sp[i] && i != 3 && i != 4 && i != 5) return "a required pool array is NULL (every array but dX0, dInfo, dZmp)";
    if (pool->lists_in < 0 || pool->lists_in > 1) return "pool->lists_in must be 0 or 1";
    if (trials > 0 && !from->dTrialSnapshot) return "dTrialSnapshot is NULL";
    if (live) {
        const void* lp[CMPC_SNAP_ARRAYS];
        snapshot_pointers(*live, lp);
        for (int i = 0; i < CMPC_SNAP_ARRAYS; ++i)
            for (int j = 0; j < CMPC_SNAP_ARRAYS; ++j)
                if (sp[i] && sp[i] == lp[j]) return "a pool array is also a live array";
    }
    return nullptr;
}
// the argument block of the restore step of tick `tick`: the snapshot's table, the pool's set pool->lists_in paired with the live set live->lists_in (the
// one this tick reads as "previous") and the pool's other set with the other live set
static bool restore_args(int N, int B, int M, int tick, const cmpc_walk_snapshot* live, const cmpc_walk_refill* r, const cmpc_walk_refill_snapshot* from,
                         CmpcRefillRestoreArgs& a)
{
    if (tick < 0 || !live || !r || r->trials < 1 || !r->dStartTick || !r->dTrial || live->lists_in < 0 || live->lists_in > 1) return false;
    cmpc_walk_snapshot pool = *from->pool;
    if (pool.lists_in != live->lists_in) {
        std::swap(pool.dListT, pool.dListTB);
        std::swap(pool.dListPose, pool.dListPoseB);
        std::swap(pool.dListN, pool.dListNB);
    }
    if (!snapshot_args(N, B, from->pool_batch, M, &pool, live, from->dTrialSnapshot, nullptr, a.copy)) return false;
    a.start = r->dStartTick; a.trial = r->dTrial;
    a.tick = tick; a.Q = r->trials; a.pool_tick = pool.tick;
    a.ok = from->dTrialSnapshotOk;
    a.end_tick = live->dEndTick; a.end_code = live->dEndCode;
    return true;
}

int cmpc_rollout_refill_restore(int horizon, int batch, int max_contacts, int tick, const cmpc_walk_snapshot* live, const cmpc_walk_refill* refill,
                                const cmpc_walk_refill_snapshot* from)
{
    if (!from || !live || !refill || refill->trials < 0) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill_restore: null argument or a negative count");
    if (const char* why = restore_refusal(from, refill->trials, live)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_rollout_refill_restore: ") + why);
    if (horizon < 1 || batch < 1 || max_contacts < 1 || tick < 0 || !refill->dStartTick || !refill->dTrial || live->lists_in < 0 || live->lists_in > 1)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill_restore: bad argument");
    if (refill->trials == 0) return CMPC_OK;   // (no slot ever holds a trial)
    CmpcRefillRestoreArgs a;
    if (!restore_args(horizon, batch, max_contacts, tick, live, refill, from, a))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill_restore: bad argument (a NULL live array)");
    cmpc_refill_restore_host(a);
    return CMPC_OK;
}

static int walk_refill_impl(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                            const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, const cmpc_walk_refill_snapshot* from, int row0,
                            int lists_in, int* lists_out, void* stream, const cmpc_walk_tape* tape = nullptr, int tape_row0 = 0,
                            const cmpc_walk_refill_plans* plans = nullptr);

int cmpc_rollout_walk_refill_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                    const cmpc_walk_refill* refill, int row0, int lists_in, int* lists_out, void* stream)
{
    return cmpc_rollout_walk_refill_trials_device(h, max_contacts, tick0, ticks, io, rec, refill, nullptr, row0, lists_in, lists_out, stream);
}

// the refill walk: per tick the refill launch, the tick's three launches (front and back kernels in refill mode, the warm solve with the per-problem cold
// policy) and the record with local tick numbers.  trials (cmpc_walk_refill_trials) null, or with nothing set: the launches this function always queued;
// else the front and back kernels' per-trial instantiations, each only when it has something to do, and the handle's per-problem table as the solve's and
// the back kernel's records when there are per-trial models
int cmpc_rollout_walk_refill_trials_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                           const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, int row0, int lists_in, int* lists_out,
                                           void* stream)
{
    return walk_refill_impl(h, max_contacts, tick0, ticks, io, rec, refill, trials, nullptr, row0, lists_in, lists_out, stream);
}

int cmpc_rollout_walk_refill_snapshot_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                             const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, const cmpc_walk_refill_snapshot* from,
                                             int row0, int lists_in, int* lists_out, void* stream)
{
    return walk_refill_impl(h, max_contacts, tick0, ticks, io, rec, refill, trials, from, row0, lists_in, lists_out, stream);
}

// the trials call with a tape row behind every tick (include/cmpc.h); tape null: the trials call itself
int cmpc_rollout_walk_refill_taped_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                          const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, int row0, int lists_in, int* lists_out,
                                          const cmpc_walk_tape* tape, int tape_row0, void* stream)
{
    return walk_refill_impl(h, max_contacts, tick0, ticks, io, rec, refill, trials, nullptr, row0, lists_in, lists_out, stream, tape, tape_row0);
}

// ---- plans per trial (include/cmpc.h, cmpc_walk_refill_plans): the plan select step between the refill launch and the front kernel ----
// what is refused of `plans` without a handle, in the header's order; null: nothing.  io (or null: the host form, which has the views only): the walk's
// buffers the views must be and a pool array must not be
static const char* plans_refusal(const cmpc_walk_refill_plans* p, int trials, const cmpc_walk_io* io, const cmpc_walk_refill_snapshot* from)
{
    if (from) return "plans together with a snapshot pool (per-trial plans for trials from a snapshot would be a replan of a walk in progress)";
    if (p->pool_plans < 1) return "pool_plans must be at least 1";
    if (!p->dPoolT || !p->dPoolPose || !p->dPoolN) return "a pool list array is NULL (dPoolT, dPoolPose, dPoolN)";
    if (trials > 0 && !p->dTrialPlan) return "dTrialPlan is NULL";
    if (!p->dPoolCom != !p->dPoolH) return "dPoolCom and dPoolH go together: both or neither";
    const bool traj = p->dPoolCom != nullptr;
    if (io && traj && (!io->tick.dPlanCom || !io->tick.dPlanH)) return "pool trajectories need io->tick.dPlanCom and dPlanH";
    if (io) {
        const cmpc_tick_io& k = io->tick;
        if (p->dPlanT != k.dPlanT || p->dPlanPose != k.dPlanPose || p->dPlanN != k.dPlanN || (traj && (p->dPlanCom != k.dPlanCom || p->dPlanH != k.dPlanH)))
            return "a writable view is not io's pointer (dPlanT, dPlanPose, dPlanN, and dPlanCom / dPlanH with pool trajectories)";
    } else if (!p->dPlanT || !p->dPlanPose || !p->dPlanN || (traj && (!p->dPlanCom || !p->dPlanH))) {
        return "a writable view is NULL";
    }
    const void* const pool[5] = {p->dPoolT, p->dPoolPose, p->dPoolN, p->dPoolCom, p->dPoolH};
    const void* live[11] = {p->dPlanT, p->dPlanPose, p->dPlanN, traj ? p->dPlanCom : nullptr, traj ? p->dPlanH : nullptr,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (io) {
        const void* const lists[6] = {io->tick.dListT, io->tick.dListPose, io->tick.dListN, io->dListTB, io->dListPoseB, io->dListNB};
        for (int i = 0; i < 6; ++i) live[5 + i] = lists[i];
    }
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 11; ++j)
            if (pool[i] && pool[i] == live[j]) return "a pool array is also a live array";
    return nullptr;
}
// the argument block of the select step of tick `tick`; knots: the planner trajectories' (read with pool trajectories only)
static bool plans_args(int B, int M, int tick, int knots, const cmpc_walk_refill* r, const cmpc_walk_refill_plans* p, const cmpc_walk_record* rec,
                       CmpcRefillPlansArgs& a)
{
    if (B < 1 || M < 1 || tick < 0 || !r || r->trials < 1 || !r->dStartTick || !r->dTrial || !rec || !rec->dEndTick || !rec->dEndCode) return false;
    if (p->dPoolCom && knots < 1) return false;
    a = CmpcRefillPlansArgs{};
    a.B = B; a.Q = r->trials; a.tick = tick; a.pool_plans = p->pool_plans;
    a.start = r->dStartTick; a.trial = r->dTrial; a.index = p->dTrialPlan; a.ok = p->dTrialPlanOk;
    a.end_tick = rec->dEndTick; a.end_code = rec->dEndCode;
    int n = 0;
    auto add = [&](const void* sp, void* dp, int words) {
        a.src[n] = static_cast<const unsigned*>(sp); a.dst[n] = static_cast<unsigned*>(dp); a.words[n] = words;
        ++n;
    };
    add(p->dPoolT, p->dPlanT, 8 * M); add(p->dPoolPose, p->dPlanPose, 14 * M); add(p->dPoolN, p->dPlanN, 2);
    if (p->dPoolCom) { add(p->dPoolCom, p->dPlanCom, 3 * knots); add(p->dPoolH, p->dPlanH, 3 * knots); }
    a.count = n;
    return true;
}

int cmpc_rollout_refill_plans(int batch, int max_contacts, int tick, const cmpc_walk_refill* refill, const cmpc_walk_refill_plans* plans,
                              const cmpc_walk_record* rec, int plan_knots)
{
    if (!plans || !refill || !rec || refill->trials < 0) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill_plans: null argument or a negative count");
    if (const char* why = plans_refusal(plans, refill->trials, nullptr, nullptr)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_rollout_refill_plans: ") + why);
    if (batch < 1 || max_contacts < 1 || tick < 0 || !refill->dStartTick || !refill->dTrial || !rec->dEndTick || !rec->dEndCode ||
        (plans->dPoolCom && plan_knots < 1))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill_plans: bad argument");
    if (refill->trials == 0) return CMPC_OK;   // (no slot ever holds a trial)
    CmpcRefillPlansArgs a;
    if (!plans_args(batch, max_contacts, tick, plan_knots, refill, plans, rec, a)) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_refill_plans: bad argument");
    cmpc_refill_plans_host(a);
    return CMPC_OK;
}

// the taped call with a plan pool (include/cmpc.h); plans null: the taped call itself, and with tape null as well the trials call
int cmpc_rollout_walk_refill_plans_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                          const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, const cmpc_walk_refill_plans* plans,
                                          int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream)
{
    return walk_refill_impl(h, max_contacts, tick0, ticks, io, rec, refill, trials, nullptr, row0, lists_in, lists_out, stream, tape, tape_row0, plans);
}

// ---- the fold of per-trial gradients onto the pool's rows (include/cmpc.h) ----
static const char* fold_refusal(int trials, int words, const int* index, const double* per, int pool_rows, const double* out)
{
    if (trials < 0 || words < 1 || pool_rows < 1) return "trials < 0, words < 1 or pool_rows < 1";
    if (!out || (trials > 0 && (!index || !per))) return "a NULL array";
    if (out == per) return "dOut is also dPerTrial";
    if ((long long)pool_rows * words > 0x7fffffffLL) return "more than 2^31 - 1 entries in dOut";
    return nullptr;
}

int cmpc_rollout_plan_fold(int trials, int words, const int* index, const double* per_trial, int pool_rows, double* out)
{
    if (const char* why = fold_refusal(trials, words, index, per_trial, pool_rows, out)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_rollout_plan_fold: ") + why);
    for (int p = 0; p < pool_rows; ++p)
        for (int w = 0; w < words; ++w) out[(size_t)p * words + w] = cmpc_plan_fold_entry(trials, words, index, per_trial, p, w);
    return CMPC_OK;
}

int cmpc_rollout_plan_fold_device(cmpc_handle h, int trials, int words, const int* dIndex, const double* dPerTrial, int pool_rows, double* dOut, void* stream)
{
    if (const char* why = fold_refusal(trials, words, dIndex, dPerTrial, pool_rows, dOut))
        return fail(h, CMPC_ERR_ARG, std::string("cmpc_rollout_plan_fold_device: ") + why);
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_plan_fold_device: null handle");
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_plan_fold(trials, words, dIndex, dPerTrial, pool_rows, dOut, stream_of(h, stream));
    return launch_status(h, "plan fold", lrc);
}

// from (cmpc_walk_refill_snapshot) null: the walk above.  Else the trials start from pool rows: a sixth launch per tick, the restore, behind the refill; the
// front and back kernels and the record take the pool's tick as the offset of every slot's local tick, and no problem of any solve is on a first tick (the
// solve is launched without the slots' start ticks: warm for all)
// tape (cmpc_rollout_walk_refill_taped_device; never together with from) non-null: part 2 of the tape behind every tick's record -- the copy kernel and the
// multiplier call, seven launches a tick -- tick tick0 + i into row tape_row0 + i, slot-major.  Part 1 is never queued: the state a spawned trial starts
// from is dState0[q], which the regroup supplies.  dOk and the planner's times go on every tick: every tick is queued as a merge tick
// plans (cmpc_rollout_walk_refill_plans_device; never together with from) non-null: one launch more per tick, the plan select, behind the refill -- a
// spawned slot's rows of the planner's lists and trajectories become its trial's pool row before the front kernel reads them
static int walk_refill_impl(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                            const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, const cmpc_walk_refill_snapshot* from, int row0,
                            int lists_in, int* lists_out, void* stream, const cmpc_walk_tape* tape, int tape_row0, const cmpc_walk_refill_plans* plans)
{
    // (the refusals that need no handle come first: they are the same with and without one)
    if (!io || !rec || !refill) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: null argument");
    const cmpc_tick_io& k = io->tick;
    if (max_contacts < 1 || max_contacts > 16)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: max_contacts must be 1 .. 16 (a slot's first tick uses the front kernel's LDS stage)");
    if (io->dWrenchTicks) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: dWrenchTicks is not taken (the schedule is the per-trial dWrenchTrials)");
    if (trials && (trials->hidden_ticks < 0 || trials->noise_ticks < 0))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_trials_device: a negative count of schedule rows");
    if (trials && ((trials->dHiddenWrench && trials->hidden_ticks == 0) || (trials->dStateNoise && trials->noise_ticks == 0)))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_trials_device: a schedule with no rows");
    if (trials && trials->dModelOk && !trials->dModels) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_trials_device: dModelOk without dModels");
    if (from) {
        const cmpc_walk_snapshot live = walk_live_view(io, rec, 0);
        if (const char* why = restore_refusal(from, refill->trials, &live))
            return fail(h, CMPC_ERR_ARG, std::string("cmpc_rollout_walk_refill_snapshot_device: ") + why);
    }
    if (tape) {
        if (!tape_complete(tape)) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_taped_device: incomplete tape");
        if (tape_row0 < 0 || (long long)tape_row0 + ticks > tape->rows)
            return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_taped_device: the tape has too few rows");
        if (tape->plant_step != k.plant_step || tape->plant_substeps != k.plant_substeps || (tape->force_sample_time != 0) != (k.force_sample_time != 0))
            return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_taped_device: the tape's scalars do not agree with the walk");
    }
    if (plans)
        if (const char* why = plans_refusal(plans, refill->trials, io, from))
            return fail(h, CMPC_ERR_ARG, std::string("cmpc_rollout_walk_refill_plans_device: ") + why);
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: null handle");
    if (h->limits_set && h->limits.dExtremes)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: dExtremes of cmpc_set_walk_limits must be NULL on a refill walk (a slot's extremes "
                                     "would span several trials: take them from the measures trace and dTrialOf)");
    if (tape && (!h->mult_out || !h->dDuals))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_taped_device: the multiplier output is off (cmpc_set_multiplier_output before the walk)");
    if (ticks < 1 || tick0 < 0 || lists_in < 0 || lists_in > 1 || !io->dListTB || !io->dListPoseB || !io->dListNB || !k.dListT || !k.dListPose || !k.dListN ||
        !k.box_upper || !k.box_lower || !k.dState || !k.dStateOut || k.dState != k.dStateOut || !k.dPlanT || !k.dPlanPose || !k.dPlanN || !k.dOk || !k.dLand ||
        !k.dInfo || !k.dP || !k.dX0 || !k.dX || !(k.plant_step > 0) || k.plant_substeps < 1)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: bad argument");
    if (io->dListTB == k.dListT || io->dListPoseB == k.dListPose || io->dListNB == k.dListN)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: the two sets of list buffers must not alias");
    if ((k.dPlanCom || k.dPlanH) && (!k.dPlanCom || !k.dPlanH || k.plan_knots < 2 || !(k.plan_dt > 0) || !(k.robot_mass > 0)))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: bad planner trajectory");
    if (row0 < 0 || (long long)row0 + ticks > rec->rows) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: the record has too few rows");
    if (h->limits_set && h->limits.dMeasures && (long long)row0 + ticks > h->limits.rows)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: the measures trace of cmpc_set_walk_limits has too few rows");
    CmpcRefillArgs probe;
    if (!refill_args(h->B, tick0, rec, refill, k.dStateOut, probe)) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: bad refill or record");
    long long dt_ns = 0;
    if (k.force_sample_time) {
        dt_ns = snap_dt_ns(h->cfg.sampling_time);
        if (dt_ns < 1) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: force_sample_time needs a sampling time of at least 1 ns");
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    int rc = upload_box(h, k.box_upper, k.box_lower, st);
    if (rc != CMPC_OK) return rc;
    if (rec->dStats) HIPCHK(h, hipMemsetAsync(rec->dStats + 6 * (size_t)row0, 0, sizeof(int) * 6 * (size_t)ticks, st));
    // the per-trial data as the kernels take it, or null.  With models the handle reads its per-problem table from here on (the launches below capture the
    // table's address and the corner stride when they are queued); a slot's record is written by the front kernel of the slot's first tick, ahead of every
    // launch that reads it, and a slot that never gets a trial stays behind the ended mask
    CmpcRefillTrialArgs tr_args{};
    const CmpcRefillTrialArgs* tr = nullptr;
    if (trials && (trials->dModels || trials->dHiddenWrench || trials->dStateNoise || trials->dForceGain)) {
        if (trials->dModels) {
            rc = ensure_models(h);
            if (rc != CMPC_OK) return rc;
            h->models_set = true;
        }
        tr_args = CmpcRefillTrialArgs{trials->dModels, trials->dModelOk, h->dConsts, h->dExpK, h->dModels, trials->dHiddenWrench, trials->hidden_ticks,
                                      trials->dStateNoise, trials->noise_ticks, trials->dForceGain, refill->trials};
        tr = &tr_args;
    }
    const bool timing = h->timing;   // (as cmpc_rollout_walk_device)
    const int* const ended_saved = h->dEnded;
    h->timing = false; h->timed = false;
    h->dEnded = rec->dEndTick;
    double* const set_t[2] = {k.dListT, io->dListTB};
    float* const set_p[2] = {k.dListPose, io->dListPoseB};
    int* const set_n[2] = {k.dListN, io->dListNB};
    const int N = h->cfg.horizon, B = h->B;
    const int offset = from ? from->pool->tick : 0;
    int cur = lists_in;
    for (int i = 0; i < ticks && rc == CMPC_OK; ++i) {
        const int tick = tick0 + i;
        const int prev = cur;
        cur = 1 - cur;
        rc = rollout_refill_impl(h, tick, rec, refill, k.dStateOut, st);
        if (rc != CMPC_OK) break;
        if (from && refill->trials > 0) {
            const cmpc_walk_snapshot live = walk_live_view(io, rec, prev);
            CmpcRefillRestoreArgs ra;
            if (!restore_args(N, B, max_contacts, tick, &live, refill, from, ra)) {
                rc = fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_snapshot_device: bad restore");
                break;
            }
            const int rrc = cmpc_launch_refill_restore(&ra, st);
            if ((rc = launch_status(h, "refill restore", rrc)) != CMPC_OK) break;
        }
        if (plans && refill->trials > 0) {
            CmpcRefillPlansArgs pa;
            if (!plans_args(B, max_contacts, tick, k.plan_knots, refill, plans, rec, pa)) {
                rc = fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_plans_device: bad plan select");
                break;
            }
            const int prc = cmpc_launch_refill_plans(&pa, st);
            if ((rc = launch_status(h, "refill plan select", prc)) != CMPC_OK) break;
        }
        int lrc = cmpc_launch_tick_pre_refill(B, N, max_contacts, h->cfg.sampling_time, k.dPlanT, k.dPlanPose, k.dPlanN, set_t[prev], set_p[prev], set_n[prev],
                                              set_t[cur], set_p[cur], set_n[cur], k.dOk, k.dLand, h->dBox, k.dStateOut, k.dP, k.dX, k.dX0, k.dPlanCom, k.dPlanH,
                                              k.plan_knots, k.plan_dt, k.robot_mass, k.com_height, dt_ns, h->dEnded, refill->dStartTick, refill->dTrial, tick,
                                              refill->dWrenchTrials, refill->wrench_ticks, refill->trials, io->plan_t_first, (float)(h->cfg.gravity / 8.0), tr,
                                              offset, st);
        if ((rc = launch_status(h, "refill tick (front)", lrc)) != CMPC_OK) break;
        rc = solve_device_impl(h, k.dP, k.dX0, k.dX, k.dInfo, (void*)st, true, from ? nullptr : refill->dStartTick, tick);
        if (rc != CMPC_OK) break;
        lrc = cmpc_launch_tick_post_refill(B, N, max_contacts, h->cfg.sampling_time, (float)h->cfg.gravity, model_corners(h), corners_stride(h), k.dX, k.dP,
                                           k.dStateOut, k.dStateOut, k.dZmp, (float)k.plant_step, k.plant_substeps, (float)k.zmp_half_x, (float)k.zmp_half_y,
                                           k.dLand, set_t[cur], set_p[cur], set_n[cur], h->dEnded, refill->dStartTick, tick, refill->dTrial, tr, offset, st);
        if ((rc = launch_status(h, "refill tick (back)", lrc)) != CMPC_OK) break;
        CmpcRecordArgs a;
        // (the tick number an ending takes is tick - start[b]; with trials from a snapshot the whole-walk number offset + tick - start[b]: the offset goes in here)
        if (!h->box_set || !record_args(N, B, offset + tick, row0 + i, k.dX, k.dP, k.dInfo, k.dOk, k.dLand, k.dStateOut, k.dZmp, h->dBox, rec, a)) {
            rc = fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_refill_device: bad record");
            break;
        }
        a.start = refill->dStartTick;
        rc = record_launch(h, "refill walk record", a, rec->dStats ? rec->dStats + 6 * (size_t)(row0 + i) : nullptr, st);
        if (rc == CMPC_OK && tape)
            rc = rollout_tape_impl(h, max_contacts, tape_row0 + i, 2, k.dX, k.dP, k.dInfo, k.dOk, k.dLand, nullptr, k.dStateOut, k.dPlanT, k.dPlanN, set_t[cur],
                                   set_n[cur], tape, stream);
    }
    h->timing = timing;
    h->dEnded = ended_saved;
    if (rc == CMPC_OK && lists_out) *lists_out = cur;
    return rc;
}

// ---- the snapshot of a walk (include/cmpc.h, cmpc_walk_snapshot): one copy kernel, destination problem b <- source problem index[b] ----
size_t cmpc_walk_snapshot_bytes(int horizon, int max_contacts)
{
    if (horizon < 1 || max_contacts < 1) return 0;
    CmpcLayout L;
    cmpc_layout_init(L, horizon);
    return sizeof(float) * (2 * (size_t)L.nx + L.np) + 176 * (size_t)max_contacts + 160;
}

// the table of arrays both sides have, as rows of 32-bit words; false: a required pointer is NULL, or a destination array is also a source array
static bool snapshot_args(int N, int B, int src_B, int M, const cmpc_walk_snapshot* s, const cmpc_walk_snapshot* d, const int* index, int* ok, CmpcSnapshotArgs& a)
{
    if (N < 1 || B < 1 || src_B < 1 || M < 1 || !s || !d || (!index && src_B != B)) return false;
    CmpcLayout L;
    cmpc_layout_init(L, N);
    a.B = B; a.src_B = src_B; a.count = 0; a.index = index; a.ok = ok;
    bool complete = true;
    auto add = [&](const void* sp, void* dp, int words, bool optional) {
        if (!sp || !dp) { complete = complete && optional; return; }
        a.src[a.count] = static_cast<const unsigned*>(sp); a.dst[a.count] = static_cast<unsigned*>(dp); a.words[a.count] = words;
        ++a.count;
    };
    add(s->dState, d->dState, 9, false); add(s->dP, d->dP, L.np, false); add(s->dX, d->dX, L.nx, false); add(s->dX0, d->dX0, L.nx, true);
    add(s->dInfo, d->dInfo, CMPC_INFO, true); add(s->dZmp, d->dZmp, 2, true); add(s->dOk, d->dOk, 1, false); add(s->dLand, d->dLand, 2, false);
    add(s->dListT, d->dListT, 8 * M, false); add(s->dListPose, d->dListPose, 14 * M, false); add(s->dListN, d->dListN, 2, false);
    add(s->dListTB, d->dListTB, 8 * M, false); add(s->dListPoseB, d->dListPoseB, 14 * M, false); add(s->dListNB, d->dListNB, 2, false);
    add(s->dEndTick, d->dEndTick, 1, false); add(s->dEndCode, d->dEndCode, 1, false); add(s->dIterationsSum, d->dIterationsSum, 1, false);
    add(s->dIterationsMax, d->dIterationsMax, 1, false); add(s->dFinalState, d->dFinalState, 9, false); add(s->dBoxSlackMin, d->dBoxSlackMin, 1, false);
    if (!complete) return false;
    for (int i = 0; i < a.count; ++i)
        for (int j = 0; j < a.count; ++j)
            if (a.dst[i] == a.src[j]) return false;
    return true;
}

int cmpc_rollout_snapshot(int horizon, int batch, int src_batch, int max_contacts, const cmpc_walk_snapshot* src, const cmpc_walk_snapshot* dst,
                          const int* index, int* ok)
{
    CmpcSnapshotArgs a;
    if (!snapshot_args(horizon, batch, src_batch, max_contacts, src, dst, index, ok, a))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_snapshot: bad argument (a NULL array, sizes, or a destination array that is also a source array)");
    for (int b = 0; b < batch; ++b) {
        const int s = cmpc_snapshot_source(a, b);
        if (ok) ok[b] = s >= 0 ? 1 : 0;
        if (s < 0) continue;
        for (int i = 0; i < a.count; ++i) {
            const size_t w = (size_t)a.words[i];
            std::memcpy(a.dst[i] + w * b, a.src[i] + w * s, sizeof(unsigned) * w);
        }
    }
    return CMPC_OK;
}

int cmpc_rollout_snapshot_device(cmpc_handle h, int max_contacts, int src_batch, const cmpc_walk_snapshot* src, const cmpc_walk_snapshot* dst,
                                 const int* dIndex, int* dOk, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_snapshot_device: null handle");
    CmpcSnapshotArgs a;
    if (!snapshot_args(h->cfg.horizon, h->B, src_batch, max_contacts, src, dst, dIndex, dOk, a))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_snapshot_device: bad argument (a NULL array, sizes, or a destination array that is also a source array)");
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_rollout_snapshot(&a, stream_of(h, stream));
    return launch_status(h, "walk snapshot", lrc);
}

// ---- the tape of a refill walk regrouped by trial (include/cmpc.h, cmpc_walk_tape_regroup): one copy kernel ----
static_assert(sizeof(cmpc_walk_tape_regroup) == 32, "cmpc_walk_tape_regroup: the size include/cmpc.h states");
// the 11 arrays of a cmpc_walk_tape in the struct's order
static void tape_pointers(const cmpc_walk_tape& t, const void* out[11])
{
    const void* const p[11] = {t.dX, t.dP, t.dLamG, t.dInfo, t.dStates, t.dOk, t.dLand, t.dPlanT, t.dListT, t.dPlanN, t.dListN};
    for (int i = 0; i < 11; ++i) out[i] = p[i];
}
// what is refused without a handle, in the header's order; null: nothing
static const char* regroup_refusal(int max_contacts, const cmpc_walk_tape* src, const cmpc_walk_refill* r, const cmpc_walk_tape_regroup* g,
                                   const cmpc_walk_tape* dst)
{
    if (!src || !r || !g || !dst) return "null argument";
    if (!g->dTrialIndex || !g->dEndOut) return "dTrialIndex or dEndOut is NULL";
    if (r->trials > 0 && (!r->dState0 || !r->dTrialSlot || !r->dTrialStart || !r->dTrialTicks || !r->dTrialEndTick))
        return "a required array of the refill is NULL (dState0, dTrialSlot, dTrialStart, dTrialTicks, dTrialEndTick)";
    if (!tape_complete(src) || !tape_complete(dst)) return "incomplete tape";
    if (dst->rows != r->trial_ticks) return "the destination tape must have refill->trial_ticks rows";
    if (r->trials < 0) return "a negative count of trials";
    const void* sp[11];
    const void* dp[11];
    tape_pointers(*src, sp);
    tape_pointers(*dst, dp);
    for (int i = 0; i < 11; ++i)
        for (int j = 0; j < 11; ++j)
            if (dp[i] == sp[j]) return "a destination array is also a source array";
    if (max_contacts < 1) return "max_contacts must be at least 1";
    return nullptr;
}
static void regroup_args(int N, int B, int M, const cmpc_walk_tape* s, const cmpc_walk_refill* r, const cmpc_walk_tape_regroup* g, const cmpc_walk_tape* d,
                         CmpcRegroupArgs& a)
{
    CmpcLayout L;
    cmpc_layout_init(L, N);
    a.B = B; a.rows = d->rows; a.src_rows = s->rows; a.Q = r->trials; a.tick_first = g->tick_first;
    a.index = g->dTrialIndex;
    a.slot = r->dTrialSlot; a.start = r->dTrialStart; a.ticks = r->dTrialTicks; a.end = r->dTrialEndTick;
    a.state0 = reinterpret_cast<const unsigned*>(r->dState0);
    a.end_out = g->dEndOut; a.ok_out = g->dOkOut;
    int n = 0;
    auto add = [&](const void* sp, void* dp, int words) {
        a.src[n] = static_cast<const unsigned*>(sp); a.dst[n] = static_cast<unsigned*>(dp); a.words[n] = words;
        ++n;
    };
    add(s->dX, d->dX, L.nx); add(s->dP, d->dP, L.np); add(s->dLamG, d->dLamG, L.ng); add(s->dInfo, d->dInfo, CMPC_INFO);
    add(s->dOk, d->dOk, 1); add(s->dLand, d->dLand, 2); add(s->dListT, d->dListT, 8 * M); add(s->dListN, d->dListN, 2);
    add(s->dPlanT, d->dPlanT, 8 * M); add(s->dPlanN, d->dPlanN, 2);   // (CMPC_REGROUP_PLAN: the planner's rows come last)
    a.src_states = reinterpret_cast<const unsigned*>(s->dStates); a.dst_states = reinterpret_cast<unsigned*>(d->dStates);
}

int cmpc_rollout_tape_regroup(int horizon, int batch, int max_contacts, const cmpc_walk_tape* src, const cmpc_walk_refill* refill,
                              const cmpc_walk_tape_regroup* g, const cmpc_walk_tape* dst)
{
    if (const char* why = regroup_refusal(max_contacts, src, refill, g, dst)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_rollout_tape_regroup: ") + why);
    if (horizon < 1 || batch < 1) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_tape_regroup: bad horizon or batch");
    CmpcRegroupArgs a;
    regroup_args(horizon, batch, max_contacts, src, refill, g, dst, a);
    cmpc_regroup_host(a);
    return CMPC_OK;
}

int cmpc_rollout_tape_regroup_device(cmpc_handle h, int max_contacts, const cmpc_walk_tape* src, const cmpc_walk_refill* refill,
                                     const cmpc_walk_tape_regroup* g, const cmpc_walk_tape* dst, void* stream)
{
    if (const char* why = regroup_refusal(max_contacts, src, refill, g, dst))
        return fail(h, CMPC_ERR_ARG, std::string("cmpc_rollout_tape_regroup_device: ") + why);
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tape_regroup_device: null handle");
    if (dst->rows > 65535) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tape_regroup_device: more than 65535 rows (one workgroup per row and column)");
    CmpcRegroupArgs a;
    regroup_args(h->cfg.horizon, h->B, max_contacts, src, refill, g, dst, a);
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_rollout_tape_regroup(&a, stream_of(h, stream));
    return launch_status(h, "tape regroup", lrc);
}

// ---- one tick in reverse (include/cmpc.h): plant VJP -> adjust part of the list VJP -> cmpc_solution_vjp_model_device -> the state rows of gP and the flags
// (cmpc_tick_vjp_combine_kernel) -> sample + merge part of the list VJP [-> the orientation list VJP], on one stream ----
namespace {
// one workgroup per problem.  Flags first: 5 merge failed, else the sensitivity's 2 / 3 (about the inputs), else 4 when the solve's status is not 0, else the
// sensitivity's 1; a flagged problem gets zeros
// in every array written here and ok = 0 (the list kernel behind this one then writes zeros too and adds nothing to g_plan).  Otherwise
// gP = gP(solve) + gP(plant: fExt_0, tauExt_0), gState += gP[com0, dcom0, h0], gWrench = the fExt / tauExt rows of gP, gModel += solve's + plant's.
// g_rot (the rotation entry; null otherwise) holds the solve's dl/domega [B][2][N][3] and receives the plant's g_rot0[B][2][3] on stage 0.
__global__ __launch_bounds__(128) void cmpc_tick_vjp_combine_kernel(int B, int N, const float* __restrict__ info, const int* __restrict__ ok,
                                                                    const float* __restrict__ gp_sol, const float* __restrict__ gp_plant,
                                                                    const double* __restrict__ gm_sol, const double* __restrict__ gm_plant,
                                                                    double* __restrict__ g_state, float* __restrict__ g_wrench, double* __restrict__ g_model,
                                                                    float* __restrict__ g_p, float* __restrict__ sens, int* __restrict__ ok_out,
                                                                    const double* __restrict__ g_rot0, double* __restrict__ g_rot,
                                                                    const double* __restrict__ gh_plant, const double* __restrict__ gg_plant,
                                                                    double* __restrict__ g_hidden, float* __restrict__ g_noise, double* __restrict__ g_gain)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const CmpcIdx L{N};
    const int np = L.np();
    const float s0 = sens[(size_t)b * CMPC_SENS];
    int status = s0 == s0 ? (int)s0 : 2;
    if (status < 2 && info[(size_t)b * CMPC_INFO_N + 5] != 0.f) status = 4;
    if (ok && ok[b] == 0) status = 5;
    __syncthreads();   // (every thread has read the status word before thread 0 rewrites it)
    const float* gs = gp_sol + (size_t)b * np;
    const float* gq = gp_plant + (size_t)b * np;
    if (status != 0) {
        for (int e = tid; e < 9; e += 128) g_state[(size_t)b * 9 + e] = 0.0;
        if (g_wrench) for (int e = tid; e < 6 * N; e += 128) g_wrench[(size_t)b * 6 * N + e] = 0.f;
        if (g_p) for (int e = tid; e < np; e += 128) g_p[(size_t)b * np + e] = 0.f;
        if (g_rot) for (int e = tid; e < 6 * N; e += 128) g_rot[(size_t)b * 6 * N + e] = 0.0;
        if (g_hidden) for (int e = tid; e < 6; e += 128) g_hidden[(size_t)b * 6 + e] = 0.0;   // (the mismatch entry: zeros, and nothing added to g_gain)
        if (g_noise) for (int e = tid; e < 9; e += 128) g_noise[(size_t)b * 9 + e] = 0.f;
    } else {
        for (int e = tid; e < 9; e += 128) g_state[(size_t)b * 9 + e] += (double)gs[L.pCom0() + e];
        if (g_wrench)
            for (int e = tid; e < 6 * N; e += 128) {
                const int k = e / 6, i = e % 6;
                const int src = (i < 3 ? L.pFext() : L.pText() - 3) + 3 * k + i;
                g_wrench[(size_t)b * 6 * N + e] = gs[src] + gq[src];
            }
        if (g_p) for (int e = tid; e < np; e += 128) g_p[(size_t)b * np + e] = gs[e] + gq[e];
        if (g_model) for (int e = tid; e < CMPC_MODEL_DOUBLES; e += 128)
            g_model[(size_t)b * CMPC_MODEL_DOUBLES + e] += gm_sol[(size_t)b * CMPC_MODEL_DOUBLES + e] + gm_plant[(size_t)b * CMPC_MODEL_DOUBLES + e];
        if (g_rot) for (int e = tid; e < 6; e += 128) g_rot[((size_t)b * 2 + e / 3) * 3 * N + e % 3] += g_rot0[(size_t)b * 6 + e];
        // the mismatch entry: the hidden wrench and the gain are the plant's alone; the noise entered through setState, so its gradient is the solve's gP there
        if (g_hidden) for (int e = tid; e < 6; e += 128) g_hidden[(size_t)b * 6 + e] = gh_plant[(size_t)b * 6 + e];
        if (g_noise) for (int e = tid; e < 9; e += 128) g_noise[(size_t)b * 9 + e] = gs[L.pCom0() + e];
        if (g_gain && tid == 0) g_gain[b] += gg_plant[b];
    }
    if (tid == 0) { sens[(size_t)b * CMPC_SENS] = (float)status; ok_out[b] = status == 0 ? 1 : 0; }
}

__global__ __launch_bounds__(256) void cmpc_axpy_float_kernel(size_t n, const float* __restrict__ x, float* __restrict__ y)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) y[e] += x[e];
}
}  // namespace

// the mismatch entry's further arguments (cmpc_rollout_tick_vjp_mismatch_device); null in tick_vjp: the launches and bits of the two entries before it
struct TickMismatch {
    const float* hidden; const float* gain;              // this tick's hidden-wrench row [B][6] and the gain [B], either may be null
    double* g_hidden; float* g_noise; double* g_gain;    // outputs, each may be null
};

// rot: the rotation entry -- the plant VJP also gives dGradRot0, the solve's VJP is cmpc_solution_vjp_rot_device (its dGradP and dGradModel are
// cmpc_solution_vjp_model_device's bit for bit), the combine kernel adds the plant's part to stage 0, and the orientation list VJP runs last
static int tick_vjp(cmpc_handle h, bool rot, int max_contacts, double now, const cmpc_tick_tape* tape, const double* dGradStateOut, const double* dGradListOut,
                    const float* dGradX, double* dGradState, double* dGradPrevList, float* dGradWrench, double* dGradPlan, double* dGradModel, float* dGradP,
                    float* dTickSens, const double* dGradListRotOut, double* dGradPrevListRot, double* dGradPlanRot, double* dGradRot, void* stream,
                    const TickMismatch* mm = nullptr)
{
    if (!h || !tape || max_contacts < 1 || !dGradStateOut || !dGradState || !dGradPrevList || !dTickSens || (rot && !dGradPrevListRot))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_vjp_device: null argument");
    if (!tape->dX || !tape->dP || !tape->dLamG || !tape->dState || !tape->dInfo || !tape->dLand || !tape->dListT || !tape->dListN ||
        !(tape->plant_step > 0) || tape->plant_substeps < 1)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_vjp_device: incomplete tape");
    const bool merge = tape->dPrevT || tape->dPrevN;
    if (merge && (!tape->dPrevT || !tape->dPrevN || !tape->dPlanT || !tape->dPlanN))
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_vjp_device: a merge tick's tape needs the planner's and the previous tick's times and counts");
    long long dt_ns = 0;
    if (tape->force_sample_time) {
        dt_ns = snap_dt_ns(h->cfg.sampling_time);
        if (dt_ns < 1) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_tick_vjp_device: force_sample_time needs a sampling time of at least 1 ns");
    }
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, stream);
    const int B = h->B, N = h->cfg.horizon;
    const size_t nx = (size_t)B * h->L.nx, np = (size_t)B * h->L.np, nm = (size_t)B * CMPC_MODEL_DOUBLES;
    const size_t nr = (size_t)B * 6 * N, nr0 = (size_t)B * 6;
    if (!h->dTickWs)     // (sized for the rotation entry whichever entry runs first)
        HIPCHK(h, hipMalloc(&h->dTickWs, sizeof(double) * (2 * nm + nr + nr0 + 7 * (size_t)B) + sizeof(float) * (nx + 2 * np) + sizeof(int) * (size_t)B));
    double* gmSol = reinterpret_cast<double*>(h->dTickWs);
    double* gmPlant = gmSol + nm;
    double* grSol = gmPlant + nm;
    double* grPlant = grSol + nr;
    double* ghPlant = grPlant + nr0;            // (the mismatch entry: the plant's gradient on the hidden wrench [B][6] and on the gain [B])
    double* ggPlant = ghPlant + 6 * (size_t)B;
    float* gX = reinterpret_cast<float*>(ggPlant + (size_t)B);
    if (rot && dGradRot) grSol = dGradRot;     // (the solve's VJP writes the caller's array; the combine kernel finishes it in place)
    float* gpSol = gX + nx;
    float* gpPlant = gpSol + np;
    int* okTick = reinterpret_cast<int*>(gpPlant + np);
    if (!h->tick_ev) HIPCHK(h, hipEventCreateWithFlags(&h->tick_ev, hipEventDisableTiming));
    else HIPCHK(h, hipStreamWaitEvent(st, h->tick_ev, 0));
    int rc = cmpc_launch_plant_vjp(N, B, (float)h->cfg.gravity, model_corners(h), corners_stride(h), tape->dX, tape->dP, tape->dState, (float)tape->plant_step,
                                   tape->plant_substeps, dGradStateOut, dGradState, gX, gpPlant, gmPlant, rot ? grPlant : nullptr, mm ? 1 : 0,
                                   mm ? mm->hidden : nullptr, mm ? mm->gain : nullptr, mm && mm->g_hidden ? ghPlant : nullptr,
                                   mm && mm->g_gain ? ggPlant : nullptr, st);
    if (const int err = launch_status(h, "tick VJP (plant)", rc)) return err;
    if (dGradX) {
        hipLaunchKernelGGL(cmpc_axpy_float_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, nx, dGradX, gX);
        HIPCHK(h, hipGetLastError());
    }
    if (dGradListOut) {
        rc = cmpc_launch_contacts_position_vjp(B, N, max_contacts, h->cfg.sampling_time, now, 1, dt_ns, tape->dPlanT, tape->dPlanN, tape->dPrevT, tape->dPrevN,
                                               tape->dListT, tape->dListN, tape->dLand, tape->dOk, dGradListOut, nullptr, gX, nullptr, nullptr, nullptr, st);
        if (const int err = launch_status(h, "tick VJP (adjust)", rc)) return err;
    }
    rc = rot ? cmpc_solution_vjp_rot_device(h, tape->dX, tape->dP, tape->dLamG, gX, gpSol, gmSol, grSol, dTickSens, stream)
             : cmpc_solution_vjp_model_device(h, tape->dX, tape->dP, tape->dLamG, gX, gpSol, gmSol, dTickSens, stream);
    if (rc != CMPC_OK) return rc;
    hipLaunchKernelGGL(cmpc_tick_vjp_combine_kernel, dim3(B), dim3(128), 0, st, B, N, tape->dInfo, tape->dOk, gpSol, gpPlant, gmSol, gmPlant, dGradState,
                       dGradWrench, dGradModel, dGradP, dTickSens, okTick, rot ? grPlant : nullptr, rot ? grSol : nullptr, ghPlant, ggPlant,
                       mm ? mm->g_hidden : nullptr, mm ? mm->g_noise : nullptr, mm ? mm->g_gain : nullptr);
    HIPCHK(h, hipGetLastError());
    rc = cmpc_launch_contacts_position_vjp(B, N, max_contacts, h->cfg.sampling_time, now, 2, dt_ns, tape->dPlanT, tape->dPlanN, tape->dPrevT, tape->dPrevN,
                                           tape->dListT, tape->dListN, tape->dLand, okTick, dGradListOut, gpSol, nullptr, dGradPrevList, dGradPlan, nullptr, st);
    if (const int err = launch_status(h, "tick VJP (sample + merge)", rc)) return err;
    if (rot) {
        rc = cmpc_launch_contacts_orientation_vjp(B, N, max_contacts, h->cfg.sampling_time, now, dt_ns, tape->dPlanT, tape->dPlanN, tape->dPrevT, tape->dPrevN,
                                                  tape->dListT, tape->dListN, tape->dLand, okTick, dGradListRotOut, grSol, dGradPrevListRot, dGradPlanRot,
                                                  nullptr, st);
        if (const int err = launch_status(h, "tick VJP (orientations)", rc)) return err;
    }
    HIPCHK(h, hipEventRecord(h->tick_ev, st));
    return CMPC_OK;
}

int cmpc_rollout_tick_vjp_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, const double* dGradStateOut,
                                 const double* dGradListOut, const float* dGradX, double* dGradState, double* dGradPrevList, float* dGradWrench,
                                 double* dGradPlan, double* dGradModel, float* dGradP, float* dTickSens, void* stream)
{
    return tick_vjp(h, false, max_contacts, now, tape, dGradStateOut, dGradListOut, dGradX, dGradState, dGradPrevList, dGradWrench, dGradPlan, dGradModel,
                    dGradP, dTickSens, nullptr, nullptr, nullptr, nullptr, stream);
}

int cmpc_rollout_tick_vjp_rot_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, const double* dGradStateOut,
                                     const double* dGradListOut, const float* dGradX, double* dGradState, double* dGradPrevList, float* dGradWrench,
                                     double* dGradPlan, double* dGradModel, float* dGradP, float* dTickSens, const double* dGradListRotOut,
                                     double* dGradPrevListRot, double* dGradPlanRot, double* dGradRot, void* stream)
{
    return tick_vjp(h, true, max_contacts, now, tape, dGradStateOut, dGradListOut, dGradX, dGradState, dGradPrevList, dGradWrench, dGradPlan, dGradModel,
                    dGradP, dTickSens, dGradListRotOut, dGradPrevListRot, dGradPlanRot, dGradRot, stream);
}

int cmpc_rollout_tick_vjp_mismatch_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, const double* dGradStateOut,
                                          const double* dGradListOut, const float* dGradX, double* dGradState, double* dGradPrevList, float* dGradWrench,
                                          double* dGradPlan, double* dGradModel, float* dGradP, float* dTickSens, const double* dGradListRotOut,
                                          double* dGradPrevListRot, double* dGradPlanRot, double* dGradRot, const float* dHiddenWrench, const float* dForceGain,
                                          double* dGradHidden, float* dGradNoise, double* dGradGain, void* stream)
{
    const TickMismatch mm{dHiddenWrench, dForceGain, dGradHidden, dGradNoise, dGradGain};
    return tick_vjp(h, dGradPrevListRot != nullptr, max_contacts, now, tape, dGradStateOut, dGradListOut, dGradX, dGradState, dGradPrevList, dGradWrench, dGradPlan,
                    dGradModel, dGradP, dTickSens, dGradListRotOut, dGradPrevListRot, dGradPlanRot, dGradRot, stream, &mm);
}

// ---- the reverse walk on the device tape (include/cmpc.h, cmpc_rollout_walk_vjp_device): gate, tick VJP, gate, ..., gate ----
static CmpcGateArgs gate_args_of(const cmpc_walk_gate* g, int nx, int np)
{
    return CmpcGateArgs{g->batch, g->max_contacts, g->horizon, nx, np, g->end_tick, g->do_post, g->tick_post, g->seed_state, g->tick_state, g->tick_list,
                        g->tick_sens, g->carry_state, g->carry_list, g->wrench_row, g->grad_p_row, g->status_row, g->do_pre, g->tick_pre, g->first, g->ok_row,
                        g->grad_x_row, g->ok_out, g->grad_x_out};
}

static int gate_check(const cmpc_walk_gate* g);

// the gate with the orientation arrays: the base check, plus carry_list_rot, and tick_list_rot with the POST part
static int gate_rot_check(const cmpc_walk_gate_rot* g)
{
    if (!g) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_rot_gate: bad argument");
    const int rc = gate_check(&g->base);
    if (rc != CMPC_OK) return rc;
    if (!g->carry_list_rot || (g->base.do_post && !g->tick_list_rot))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_rot_gate: carry_list_rot is needed, and tick_list_rot with the POST part");
    return CMPC_OK;
}

static CmpcGateArgs gate_rot_args_of(const cmpc_walk_gate_rot* g, int nx, int np)
{
    CmpcGateArgs a = gate_args_of(&g->base, nx, np);
    a.t_list_rot = g->tick_list_rot; a.carry_list_rot = g->carry_list_rot; a.rot_row = g->rot_row; a.removed_row = g->removed_row;
    return a;
}

static int gate_launch(cmpc_handle h, const CmpcGateArgs& a, void* stream)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int lrc = cmpc_launch_walk_vjp_gate(&a, stream_of(h, stream));
    return launch_status(h, "reverse walk (gate)", lrc);
}

static void gate_on_host(const CmpcGateArgs& a)
{
    for (int b = 0; b < a.B; ++b) cmpc_walk_gate_problem(a, b);
    const size_t wide = cmpc_walk_gate_wide_entries(&a);
    for (size_t e = 0; e < wide; ++e) cmpc_walk_gate_wide(a, e);
}

int cmpc_rollout_walk_vjp_gate_device(cmpc_handle h, const cmpc_walk_gate* g, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_gate_device: null handle");
    const int rc = gate_check(g);
    if (rc != CMPC_OK) return rc;
    if (g->batch != h->B || g->horizon != h->cfg.horizon) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_gate_device: batch and horizon must be the handle's");
    return gate_launch(h, gate_args_of(g, h->L.nx, h->L.np), stream);
}

int cmpc_rollout_walk_vjp_rot_gate_device(cmpc_handle h, const cmpc_walk_gate_rot* g, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_rot_gate_device: null handle");
    const int rc = gate_rot_check(g);
    if (rc != CMPC_OK) return rc;
    if (g->base.batch != h->B || g->base.horizon != h->cfg.horizon)
        return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_rot_gate_device: batch and horizon must be the handle's");
    return gate_launch(h, gate_rot_args_of(g, h->L.nx, h->L.np), stream);
}

int cmpc_rollout_walk_vjp_rot_gate(const cmpc_walk_gate_rot* g)
{
    const int rc = gate_rot_check(g);
    if (rc != CMPC_OK) return rc;
    CmpcLayout L;
    cmpc_layout_init(L, g->base.horizon);
    gate_on_host(gate_rot_args_of(g, L.nx, L.np));
    return CMPC_OK;
}

static int gate_check(const cmpc_walk_gate* g)
{
    if (!g || g->batch < 1 || g->max_contacts < 1 || g->horizon < 1 || g->horizon > CMPC_NMAX || (!g->do_post && !g->do_pre) || !g->carry_state || !g->carry_list)
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_gate: bad argument");
    if (g->do_post && (!g->seed_state || !g->tick_state || !g->tick_list || !g->tick_sens || !g->status_row))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_gate: the POST part needs the seed row, the tick's outputs and the status row");
    if (g->do_pre && (!g->ok_out || (!g->grad_x_row != !g->grad_x_out)))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_gate: the PRE part needs ok_out, and grad_x_row and grad_x_out together");
    return CMPC_OK;
}

int cmpc_rollout_walk_vjp_gate(const cmpc_walk_gate* g)
{
    const int rc = gate_check(g);
    if (rc != CMPC_OK) return rc;
    CmpcLayout L;
    cmpc_layout_init(L, g->horizon);
    gate_on_host(gate_args_of(g, L.nx, L.np));
    return CMPC_OK;
}

// the loop of both reverse walks; r: the orientation chain of cmpc_rollout_walk_vjp_rot_device (checked by the caller), or null -- then every launch and
// every bit is what the walk without orientations always queued and gave
static int walk_vjp(cmpc_handle h, const char* who, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                    const cmpc_walk_grads* g, const cmpc_walk_grads_rot* r, void* stream, bool mismatch = false, const cmpc_plant_mismatch* m = nullptr,
                    const cmpc_walk_grads_mismatch* mg = nullptr)
{
    const std::string name(who);
    {
        const int mrc = mismatch_check(h, who, m);
        if (mrc != CMPC_OK) return mrc;
    }
    if (!h || !g || !tape_complete(tape)) return fail(h, CMPC_ERR_ARG, name + ": null argument or incomplete tape");
    if (max_contacts < 1 || tick0 < 0 || ticks < 1 || row0 < 0 || (long long)row0 + ticks > tape->rows)
        return fail(h, CMPC_ERR_ARG, name + ": bad argument (the rows must lie inside the tape)");
    if (!g->dGradStates || !g->dCarryState || !g->dCarryList || !g->dStatus)
        return fail(h, CMPC_ERR_ARG, name + ": dGradStates, the two carries and dStatus are needed");
    if (row0 == 0 && !tape->first_row_is_first_tick)
        return fail(h, CMPC_ERR_ARG, name + ": row 0 is not a first tick and has no row before it to take the previous lists from");
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, stream);
    const int B = h->B, N = h->cfg.horizon, M = max_contacts;
    const size_t nx = (size_t)B * h->L.nx, np = (size_t)B * h->L.np, ng = (size_t)B * h->L.ng, nl = (size_t)B * 6 * M, nt = (size_t)B * 4 * M;
    if (!h->dWalkWs || h->walk_ws_M < M) {
        if (h->dWalkWs) {   // (a larger max_contacts: launches that read the old workspace may still be queued)
            HIPCHK(h, hipDeviceSynchronize());
            hipFree(h->dWalkWs);
            h->dWalkWs = nullptr; h->walk_ws_M = 0;
        }
        // (sized for the rotation entry whichever entry runs first: the second list buffer is the tick's dGradPrevListRot)
        HIPCHK(h, hipMalloc(&h->dWalkWs, sizeof(double) * ((size_t)B * 9 + 2 * nl) + sizeof(float) * (nx + (size_t)B * CMPC_SENS) + sizeof(int) * (size_t)B));
        h->walk_ws_M = M;
    }
    double* wsState = reinterpret_cast<double*>(h->dWalkWs);
    double* wsList = wsState + (size_t)B * 9;
    double* wsListRot = wsList + (size_t)B * 6 * h->walk_ws_M;
    float* wsGx = reinterpret_cast<float*>(wsListRot + (size_t)B * 6 * h->walk_ws_M);
    float* wsSens = wsGx + nx;
    int* wsOk = reinterpret_cast<int*>(wsSens + (size_t)B * CMPC_SENS);
    if (h->tick_ev) HIPCHK(h, hipStreamWaitEvent(st, h->tick_ev, 0));   // (the gate writes workspace an earlier call on another stream may still read)
    CmpcGateArgs a{};
    a.B = B; a.M = M; a.N = N; a.nx = h->L.nx; a.np = h->L.np;
    a.end_tick = dEndTick;
    a.t_state = wsState; a.t_list = wsList; a.t_sens = wsSens;
    a.carry_state = g->dCarryState; a.carry_list = g->dCarryList;
    a.ok_out = wsOk; a.gx_out = g->dGradX ? wsGx : nullptr;
    if (r) { a.t_list_rot = wsListRot; a.carry_list_rot = r->dCarryListRot; }
    int rc = CMPC_OK;
    for (int i = ticks; i >= 0 && rc == CMPC_OK; --i) {
        // the gate step between tick i (POST: i < ticks) and tick i - 1 (PRE: i > 0), fused into one launch
        const size_t rq = (size_t)(row0 + i), rp = (size_t)(row0 + i - 1);
        a.do_post = i < ticks; a.tick_post = tick0 + i;
        if (a.do_post) {
            a.seed_state = g->dGradStates + rq * B * 9;
            a.wrench_row = g->dGradWrench ? g->dGradWrench + rq * B * 6 * N : nullptr;
            a.gp_row = g->dGradP ? g->dGradP + rq * np : nullptr;
            a.status_row = g->dStatus + rq * B;
            if (r) {
                a.rot_row = r->dGradRot ? r->dGradRot + rq * B * 6 * N : nullptr;
                a.removed_row = r->dRemoved ? r->dRemoved + rq * B : nullptr;
            }
        }
        a.do_pre = i > 0; a.tick_pre = tick0 + i - 1; a.first = i == ticks;
        if (a.do_pre) {
            a.ok_row = tape->dOk + rp * B;
            a.gx_row = g->dGradX ? g->dGradX + rp * nx : nullptr;
        }
        const int lrc = cmpc_launch_walk_vjp_gate(&a, st);
        if (const int err = launch_status(h, "reverse walk (gate)", lrc)) return err;
        if (i == 0) break;
        const bool first_tick = rp == 0;   // (row 0 of a tape whose first row is a first tick: checked above)
        cmpc_tick_tape tt{};
        tt.dX = tape->dX + rp * nx; tt.dP = tape->dP + rp * np; tt.dLamG = tape->dLamG + rp * ng;
        tt.dState = tape->dStates + rp * B * 9; tt.dInfo = tape->dInfo + rp * B * CMPC_INFO;
        tt.dOk = wsOk; tt.dLand = tape->dLand + rp * B * 2;
        tt.dPlanT = tape->dPlanT + rp * nt; tt.dPlanN = tape->dPlanN + rp * B * 2;
        tt.dPrevT = first_tick ? nullptr : tape->dListT + (rp - 1) * nt; tt.dPrevN = first_tick ? nullptr : tape->dListN + (rp - 1) * B * 2;
        tt.dListT = tape->dListT + rp * nt; tt.dListN = tape->dListN + rp * B * 2;
        tt.plant_step = tape->plant_step; tt.plant_substeps = tape->plant_substeps; tt.force_sample_time = tape->force_sample_time;
        // the mismatch entry: tick rp ran under its own schedule rows; its gradient rows are written whether or not the tick lay inside a schedule's range
        TickMismatch mm{};
        if (mismatch) {
            const float* unused;
            mismatch_rows(m, B, tick0 + i - 1, &mm.hidden, &unused, &mm.gain);
            if (mg) {
                mm.g_hidden = mg->dGradHidden ? mg->dGradHidden + rp * B * 6 : nullptr;
                mm.g_noise = mg->dGradNoise ? mg->dGradNoise + rp * B * 9 : nullptr;
                mm.g_gain = mg->dGradGain;
            }
        }
        rc = tick_vjp(h, r != nullptr, M, (double)(tick0 + i - 1) * h->cfg.sampling_time, &tt, g->dCarryState, g->dCarryList, a.gx_out, wsState, wsList,
                      g->dGradWrench ? g->dGradWrench + rp * B * 6 * N : nullptr, g->dGradPlan, g->dGradModel, g->dGradP ? g->dGradP + rp * np : nullptr, wsSens,
                      r ? r->dCarryListRot : nullptr, r ? wsListRot : nullptr, r ? r->dGradPlanRot : nullptr,
                      r && r->dGradRot ? r->dGradRot + rp * B * 6 * N : nullptr, stream, mismatch ? &mm : nullptr);
    }
    if (rc == CMPC_OK && h->tick_ev) HIPCHK(h, hipEventRecord(h->tick_ev, st));
    return rc;
}

int cmpc_rollout_walk_vjp_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                 const cmpc_walk_grads* g, void* stream)
{
    return walk_vjp(h, "cmpc_rollout_walk_vjp_device", max_contacts, tick0, ticks, tape, row0, dEndTick, g, nullptr, stream);
}

int cmpc_rollout_walk_vjp_rot_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                     const cmpc_walk_grads* g, const cmpc_walk_grads_rot* r, void* stream)
{
    if (!r || !r->dCarryListRot) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_rot_device: r and its dCarryListRot are needed");
    return walk_vjp(h, "cmpc_rollout_walk_vjp_rot_device", max_contacts, tick0, ticks, tape, row0, dEndTick, g, r, stream);
}

int cmpc_rollout_walk_vjp_mismatch_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                          const cmpc_walk_grads* g, const cmpc_walk_grads_rot* r, const cmpc_plant_mismatch* m,
                                          const cmpc_walk_grads_mismatch* mg, void* stream)
{
    if (r && !r->dCarryListRot) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_vjp_mismatch_device: r needs its dCarryListRot");
    return walk_vjp(h, "cmpc_rollout_walk_vjp_mismatch_device", max_contacts, tick0, ticks, tape, row0, dEndTick, g, r, stream, true, m, mg);
}

// ---- one tick FORWARDS in k directions (include/cmpc.h): list JVP (merge + sample) -> the p direction assembled (cmpc_tick_jvp_assemble_kernel) ->
// cmpc_solution_jvp_rot_device -> the flags (cmpc_tick_jvp_flag_kernel) -> list JVP (adjust) -> the k-column plant JVP, on one stream ----
namespace {
// one workgroup per (problem, column): the column's p direction, float32.  The list kernel has written the nominalPos / currentPos rows; here the state
// direction goes to com0 / dcom0 / h0 (cmpc_write_state_device's rows, rounded to float32), the wrench direction to the fExt / tauExt rows, every other row
// is zero, and the caller's extra p direction is added to all of them.  d_noise[B][k][9] (the mismatch entry; null otherwise): the direction of the sensor
// noise, added to the rounded state direction in ONE float32 add as the forward's setState adds the noise -- it reaches the solve and nothing else.
__global__ __launch_bounds__(128) void cmpc_tick_jvp_assemble_kernel(int N, const double* __restrict__ d_state, const float* __restrict__ d_wrench,
                                                                     const float* __restrict__ d_extra, float* __restrict__ d_p,
                                                                     const float* __restrict__ d_noise)
{
    const size_t col = blockIdx.x;
    const CmpcIdx L{N};
    const int np = L.np();
    float* dp = d_p + col * np;
    for (int e = threadIdx.x; e < np; e += 128) {
        float v = 0.f;
        const bool listed = (e >= L.pNom(0) && e < L.pNom(0) + 3 * N + 6) || (e >= L.pNom(1) && e < L.pNom(1) + 3 * N + 6);
        if (listed) v = dp[e];
        else if (e >= L.pCom0() && e < L.pCom0() + 9) {
            v = d_state ? (float)d_state[col * 9 + (e - L.pCom0())] : 0.f;
            if (d_noise) v = v + d_noise[col * 9 + (e - L.pCom0())];
        }
        else if (d_wrench && e >= L.pFext() && e < L.pText()) { const int q = e - L.pFext(); v = d_wrench[(col * N + q / 3) * 6 + q % 3]; }
        else if (d_wrench && e >= L.pText()) { const int q = e - L.pText(); v = d_wrench[(col * N + q / 3) * 6 + 3 + q % 3]; }
        dp[e] = d_extra ? v + d_extra[col * np + e] : v;
    }
}

// one workgroup per problem, after the solve: the tick's status with the VJP's codes and precedence (cmpc_tick_vjp_combine_kernel; 2 also for a non-finite
// tape state).  A flagged problem gets
// zeros in every column of dx, of the p direction and of the rotation direction, and ok = 0 (the adjust part of the list kernel and the plant kernel behind
// this one then write zeros too); otherwise stage 0 of the rotation direction is gathered for the plant.
__global__ __launch_bounds__(128) void cmpc_tick_jvp_flag_kernel(int N, int K, const float* __restrict__ info, const int* __restrict__ ok,
                                                                 const float* __restrict__ state_in, float* __restrict__ sens, float* __restrict__ d_x,
                                                                 float* __restrict__ d_p, double* __restrict__ d_rot, double* __restrict__ d_rot0,
                                                                 int* __restrict__ ok_out)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const CmpcIdx L{N};
    const float s0 = sens[(size_t)b * CMPC_SENS];
    int status = s0 == s0 ? (int)s0 : 2;
    // (the state the tick started from is an input of the plant alone here: in reverse a non-finite one reaches the solve through the plant VJP and comes
    //  back as status 2; forwards it is looked at directly, for the same word)
    bool finite = true;
    for (int e = 0; e < 9; ++e) finite = finite && __builtin_isfinite(state_in[(size_t)b * 9 + e]);
    if (status < 2 && !finite) status = 2;
    if (status < 2 && info[(size_t)b * CMPC_INFO_N + 5] != 0.f) status = 4;
    if (ok && ok[b] == 0) status = 5;
    __syncthreads();   // (every thread has read the status word before thread 0 rewrites it)
    if (status != 0) {
        for (size_t e = tid; e < (size_t)K * L.nx(); e += 128) d_x[(size_t)b * K * L.nx() + e] = 0.f;
        for (size_t e = tid; e < (size_t)K * L.np(); e += 128) d_p[(size_t)b * K * L.np() + e] = 0.f;
        if (d_rot) for (size_t e = tid; e < (size_t)K * 6 * N; e += 128) d_rot[(size_t)b * K * 6 * N + e] = 0.0;
        if (d_rot) for (int e = tid; e < K * 6; e += 128) d_rot0[(size_t)b * K * 6 + e] = 0.0;
    } else if (d_rot) {
        for (int e = tid; e < K * 6; e += 128)     // e = (column * 2 + foot) * 3 + axis
            d_rot0[(size_t)b * K * 6 + e] = d_rot[((size_t)b * K * 2 + e / 3) * 3 * N + e % 3];
    }
    if (tid == 0) { sens[(size_t)b * CMPC_SENS] = (float)status; ok_out[b] = status == 0 ? 1 : 0; }
}
}  // namespace

// (all four mismatch pointers null: the instantiation without the mismatch, which is the kernel as it was before the mismatch existed)
static int plant_jvp_cols(cmpc_handle h, const char* who, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, int k,
                          const double* dDirState, const float* dDirX, const float* dDirP, const double* dDirModel, const double* dDirRot0,
                          const float* dHiddenWrench, const float* dForceGain, const double* dDirHidden, const double* dDirGain, double* dDirStateOut,
                          void* stream)
{
    if (!h || !dX || !dP || !dStateIn || !dDirState || !dDirStateOut || !(step > 0) || substeps < 1 || k < 1)
        return fail(h, CMPC_ERR_ARG, std::string(who) + ": bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    const bool mm = dHiddenWrench || dForceGain || dDirHidden || dDirGain;
    int rc = cmpc_launch_plant_jvp_cols_mismatch(h->cfg.horizon, h->B, k, (float)h->cfg.gravity, model_corners(h), corners_stride(h), dX, dP, dStateIn, (float)step,
                                                 substeps, dDirState, dDirX, dDirP, dDirModel, dDirRot0, nullptr, dDirStateOut, mm ? 1 : 0, dHiddenWrench,
                                                 dForceGain, dDirHidden, dDirGain, stream_of(h, stream));
    return launch_status(h, "plant JVP (columns)", rc);
}

int cmpc_plant_step_jvp_cols_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, int k,
                                    const double* dDirState, const float* dDirX, const float* dDirP, const double* dDirModel, const double* dDirRot0,
                                    double* dDirStateOut, void* stream)
{
    return plant_jvp_cols(h, "cmpc_plant_step_jvp_cols_device", dX, dP, dStateIn, step, substeps, k, dDirState, dDirX, dDirP, dDirModel, dDirRot0, nullptr,
                          nullptr, nullptr, nullptr, dDirStateOut, stream);
}

int cmpc_plant_step_jvp_mismatch_cols_device(cmpc_handle h, const float* dX, const float* dP, const float* dStateIn, double step, int substeps, int k,
                                             const double* dDirState, const float* dDirX, const float* dDirP, const double* dDirModel, const double* dDirRot0,
                                             const float* dHiddenWrench, const float* dForceGain, const double* dDirHidden, const double* dDirGain,
                                             double* dDirStateOut, void* stream)
{
    return plant_jvp_cols(h, "cmpc_plant_step_jvp_mismatch_cols_device", dX, dP, dStateIn, step, substeps, k, dDirState, dDirX, dDirP, dDirModel, dDirRot0,
                          dHiddenWrench, dForceGain, dDirHidden, dDirGain, dDirStateOut, stream);
}

int cmpc_contacts_jvp_device(cmpc_handle h, int max_contacts, double now, int phase, int force_sample_time, int k, const double* dPlanT, const int* dPlanN,
                             const double* dPrevT, const int* dPrevN, const double* dListT, const int* dListN, const int* dLand, const int* dOk,
                             const double* dDirPrevList, const double* dDirPrevListRot, const double* dDirPlan, const double* dDirPlanRot, const float* dDirX,
                             double* dDirList, double* dDirListRot, float* dDirP, double* dDirRot, int* dStatus, void* stream)
{
    if (!h || max_contacts < 1 || phase < 1 || phase > 3 || k < 1 || !dListT || !dListN || !dDirList)
        return fail(h, CMPC_ERR_ARG, "cmpc_contacts_jvp_device: bad argument");
    const bool merge = dPrevT || dPrevN;
    if ((phase & 1) && merge && (!dPrevT || !dPrevN || !dPlanT || !dPlanN))
        return fail(h, CMPC_ERR_ARG, "cmpc_contacts_jvp_device: a merge tick needs the planner's and the previous tick's times and counts");
    if (dDirList == dDirPrevList || (dDirListRot && dDirListRot == dDirPrevListRot))
        return fail(h, CMPC_ERR_ARG, "cmpc_contacts_jvp_device: the outgoing list's directions must not alias the previous list's");
    long long dt_ns = 0;
    if (force_sample_time) {
        dt_ns = snap_dt_ns(h->cfg.sampling_time);
        if (dt_ns < 1) return fail(h, CMPC_ERR_ARG, "cmpc_contacts_jvp_device: force_sample_time needs a sampling time of at least 1 ns");
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = cmpc_launch_contacts_jvp(h->B, h->cfg.horizon, max_contacts, k, h->cfg.sampling_time, now, phase, dt_ns, dPlanT, dPlanN, dPrevT, dPrevN, dListT,
                                      dListN, dLand, dOk, dDirPrevList, dDirPrevListRot, dDirPlan, dDirPlanRot, dDirX, dDirList, dDirListRot, dDirP, dDirRot,
                                      dStatus, stream_of(h, stream));
    return launch_status(h, "list JVP", rc);
}

// the mismatch entry's further arguments (cmpc_rollout_tick_jvp_mismatch_device); null in tick_jvp: the launches and bits of the entry before it
struct TickMismatchDirs {
    const float* hidden; const float* gain;                               // this tick's hidden-wrench row [B][6] and the gain [B], either may be null
    const double* d_hidden; const float* d_noise; const double* d_gain;   // directions [B][k][6], [B][k][9], [B][k], each may be null
};

// (shared by the public entry points and the forward walk, as tick_vjp is)
static int tick_jvp(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, int k, const cmpc_tick_dirs* in, const cmpc_tick_dirs_out* out,
                    float* dTickSens, void* stream, const TickMismatchDirs* mm = nullptr, const char* who = "cmpc_rollout_tick_jvp_device")
{
    const std::string name(who);
    if (!h || !tape || max_contacts < 1 || k < 1 || !out || !out->dDirStateOut || !out->dDirList || !dTickSens)
        return fail(h, CMPC_ERR_ARG, name + ": null argument");
    if (!tape->dX || !tape->dP || !tape->dLamG || !tape->dState || !tape->dInfo || !tape->dLand || !tape->dListT || !tape->dListN ||
        !(tape->plant_step > 0) || tape->plant_substeps < 1)
        return fail(h, CMPC_ERR_ARG, name + ": incomplete tape");
    const bool merge = tape->dPrevT || tape->dPrevN;
    if (merge && (!tape->dPrevT || !tape->dPrevN || !tape->dPlanT || !tape->dPlanN))
        return fail(h, CMPC_ERR_ARG, name + ": a merge tick's tape needs the planner's and the previous tick's times and counts");
    const cmpc_tick_dirs none = {};
    if (!in) in = &none;
    if (out->dDirList == in->dDirPrevList || (out->dDirListRot && out->dDirListRot == in->dDirPrevListRot))
        return fail(h, CMPC_ERR_ARG, name + ": the outgoing list's directions must not alias the previous list's");
    long long dt_ns = 0;
    if (tape->force_sample_time) {
        dt_ns = snap_dt_ns(h->cfg.sampling_time);
        if (dt_ns < 1) return fail(h, CMPC_ERR_ARG, name + ": force_sample_time needs a sampling time of at least 1 ns");
    }
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, stream);
    const int B = h->B, N = h->cfg.horizon;
    const size_t cols = (size_t)B * k, nx = h->L.nx, np = h->L.np;
    if (k > h->tick_jvp_cols) {     // (hipFree waits for the device: no earlier call still reads the smaller workspace)
        if (h->dTickJvpWs) HIPCHK(h, hipFree(h->dTickJvpWs));
        h->dTickJvpWs = nullptr; h->tick_jvp_cols = 0;
        HIPCHK(h, hipMalloc(&h->dTickJvpWs, cols * (sizeof(double) * (6 * (size_t)N + 15) + sizeof(float) * (nx + np)) + sizeof(int) * (size_t)B));
        h->tick_jvp_cols = k;
    }
    // (carved for this call's k: the arrays are [B][k][...] without gaps)
    double* wsRot = reinterpret_cast<double*>(h->dTickJvpWs);
    double* wsRot0 = wsRot + cols * 6 * N;
    double* wsState = wsRot0 + cols * 6;
    float* wsX = reinterpret_cast<float*>(wsState + cols * 9);
    float* wsP = wsX + cols * nx;
    int* okTick = reinterpret_cast<int*>(wsP + cols * np);
    const bool rot = in->dDirPrevListRot || in->dDirPlanRot;
    double* dRot = !rot ? nullptr : out->dDirRot ? out->dDirRot : wsRot;
    float* dDX = out->dDirX ? out->dDirX : wsX;
    float* dPF = out->dDirPFull ? out->dDirPFull : wsP;
    if (!h->tick_ev) HIPCHK(h, hipEventCreateWithFlags(&h->tick_ev, hipEventDisableTiming));
    else HIPCHK(h, hipStreamWaitEvent(st, h->tick_ev, 0));
    const double* dState = in->dDirState;
    if (!dState) {
        HIPCHK(h, hipMemsetAsync(wsState, 0, sizeof(double) * cols * 9, st));
        dState = wsState;
    }
    if (!rot && out->dDirRot) HIPCHK(h, hipMemsetAsync(out->dDirRot, 0, sizeof(double) * cols * 6 * N, st));
    int rc = cmpc_launch_contacts_jvp(B, N, max_contacts, k, h->cfg.sampling_time, now, 1, dt_ns, tape->dPlanT, tape->dPlanN, tape->dPrevT, tape->dPrevN,
                                      tape->dListT, tape->dListN, tape->dLand, tape->dOk, in->dDirPrevList, in->dDirPrevListRot, in->dDirPlan, in->dDirPlanRot,
                                      nullptr, out->dDirList, out->dDirListRot, dPF, dRot, nullptr, st);
    if (const int err = launch_status(h, "tick JVP (merge + sample)", rc)) return err;
    hipLaunchKernelGGL(cmpc_tick_jvp_assemble_kernel, dim3((unsigned)cols), dim3(128), 0, st, N, in->dDirState, in->dDirWrench, in->dDirP, dPF,
                       mm ? mm->d_noise : (const float*)nullptr);
    HIPCHK(h, hipGetLastError());
    rc = cmpc_solution_jvp_rot_device(h, tape->dX, tape->dP, tape->dLamG, dPF, in->dDirModel, dRot, k, dDX, dTickSens, stream);
    if (rc != CMPC_OK) return rc;
    hipLaunchKernelGGL(cmpc_tick_jvp_flag_kernel, dim3(B), dim3(128), 0, st, N, k, tape->dInfo, tape->dOk, tape->dState, dTickSens, dDX, dPF, dRot, wsRot0, okTick);
    HIPCHK(h, hipGetLastError());
    rc = cmpc_launch_contacts_jvp(B, N, max_contacts, k, h->cfg.sampling_time, now, 2, dt_ns, nullptr, nullptr, nullptr, nullptr, tape->dListT, tape->dListN,
                                  tape->dLand, okTick, nullptr, nullptr, nullptr, nullptr, dDX, out->dDirList, out->dDirListRot, nullptr, nullptr, nullptr, st);
    if (const int err = launch_status(h, "tick JVP (adjust)", rc)) return err;
    // (the mismatch entry: the plant's partials at the gained forces and the summed wrench, the tick's own rows; the noise direction does not come here)
    rc = cmpc_launch_plant_jvp_cols_mismatch(N, B, k, (float)h->cfg.gravity, model_corners(h), corners_stride(h), tape->dX, tape->dP, tape->dState,
                                             (float)tape->plant_step, tape->plant_substeps, dState, dDX, dPF, in->dDirModel, rot ? wsRot0 : nullptr, okTick,
                                             out->dDirStateOut, mm ? 1 : 0, mm ? mm->hidden : nullptr, mm ? mm->gain : nullptr, mm ? mm->d_hidden : nullptr,
                                             mm ? mm->d_gain : nullptr, st);
    if (const int err = launch_status(h, "tick JVP (plant)", rc)) return err;
    HIPCHK(h, hipEventRecord(h->tick_ev, st));
    return CMPC_OK;
}

int cmpc_rollout_tick_jvp_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, int k, const cmpc_tick_dirs* in,
                                 const cmpc_tick_dirs_out* out, float* dTickSens, void* stream)
{
    return tick_jvp(h, max_contacts, now, tape, k, in, out, dTickSens, stream);
}

int cmpc_rollout_tick_jvp_mismatch_device(cmpc_handle h, int max_contacts, double now, const cmpc_tick_tape* tape, int k, const cmpc_tick_dirs* in,
                                          const cmpc_tick_dirs_out* out, float* dTickSens, const float* dHiddenWrench, const float* dForceGain,
                                          const cmpc_tick_dirs_mismatch* md, void* stream)
{
    const TickMismatchDirs mm{dHiddenWrench, dForceGain, md ? md->dDirHidden : nullptr, md ? md->dDirNoise : nullptr, md ? md->dDirGain : nullptr};
    if (!mm.hidden && !mm.gain && !mm.d_hidden && !mm.d_noise && !mm.d_gain)   // (nothing of a mismatch: the plain tick, bit for bit)
        return tick_jvp(h, max_contacts, now, tape, k, in, out, dTickSens, stream, nullptr, "cmpc_rollout_tick_jvp_mismatch_device");
    return tick_jvp(h, max_contacts, now, tape, k, in, out, dTickSens, stream, &mm, "cmpc_rollout_tick_jvp_mismatch_device");
}

// ---- the forward walk on the device tape (include/cmpc.h, cmpc_rollout_walk_jvp_device): gate, tick JVP, gate, ..., gate ----
static CmpcJvpGateArgs jvp_gate_args_of(const cmpc_walk_jvp_gate* g, int nx)
{
    return CmpcJvpGateArgs{g->batch, g->max_contacts, g->k, nx, g->end_tick, g->do_post, g->tick_post, g->tick_sens, g->state_out, g->list_out,
                           g->list_rot_out, g->x_row, g->status_row, g->removed_row, g->do_pre, g->tick_pre, g->first, g->ok_row, g->ok_out, g->first_state,
                           g->first_list, g->first_list_rot};
}

static int jvp_gate_check(const cmpc_walk_jvp_gate* g)
{
    if (!g || g->batch < 1 || g->max_contacts < 1 || g->horizon < 1 || g->horizon > CMPC_NMAX || g->k < 1 || (!g->do_post && !g->do_pre))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_jvp_gate: bad argument");
    if (g->do_post && (!g->tick_sens || !g->state_out || !g->list_out || !g->status_row))
        return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_jvp_gate: the POST part needs the tick's dTickSens, state and list directions and the status row");
    if (g->do_pre && !g->ok_out) return fail(nullptr, CMPC_ERR_ARG, "cmpc_rollout_walk_jvp_gate: the PRE part needs ok_out");
    return CMPC_OK;
}

int cmpc_rollout_walk_jvp_gate(const cmpc_walk_jvp_gate* g)
{
    const int rc = jvp_gate_check(g);
    if (rc != CMPC_OK) return rc;
    CmpcLayout L;
    cmpc_layout_init(L, g->horizon);
    const CmpcJvpGateArgs a = jvp_gate_args_of(g, L.nx);
    for (size_t c = 0; c < (size_t)g->batch * g->k; ++c) cmpc_walk_jvp_gate_column(a, c);
    const size_t wide = cmpc_walk_jvp_gate_wide_entries(&a);
    for (size_t e = 0; e < wide; ++e) cmpc_walk_jvp_gate_wide(a, e);
    return CMPC_OK;
}

int cmpc_rollout_walk_jvp_gate_device(cmpc_handle h, const cmpc_walk_jvp_gate* g, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_jvp_gate_device: null handle");
    const int rc = jvp_gate_check(g);
    if (rc != CMPC_OK) return rc;
    if (g->batch != h->B || g->horizon != h->cfg.horizon) return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_jvp_gate_device: batch and horizon must be the handle's");
    HIPCHK(h, hipSetDevice(h->device));
    const CmpcJvpGateArgs a = jvp_gate_args_of(g, h->L.nx);
    const int lrc = cmpc_launch_walk_jvp_gate(&a, stream_of(h, stream));
    return launch_status(h, "forward walk (gate)", lrc);
}

// the loop of both forward walks; m / md: the mismatch and its directions of cmpc_rollout_walk_jvp_mismatch_device, tick_who that entry's tick -- both
// null: every launch and every bit is what the walk without a mismatch always queued and gave
static int walk_jvp(cmpc_handle h, const char* who, const char* tick_who, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0,
                    const int* dEndTick, int k, const cmpc_walk_dirs* d, void* stream, const cmpc_plant_mismatch* m = nullptr,
                    const cmpc_walk_dirs_mismatch* md = nullptr)
{
    const std::string name(who);
    {
        const int mrc = mismatch_check(h, who, m);
        if (mrc != CMPC_OK) return mrc;
    }
    if (!h || !d || !tape_complete(tape)) return fail(h, CMPC_ERR_ARG, name + ": null argument or incomplete tape");
    if (max_contacts < 1 || tick0 < 0 || ticks < 1 || row0 < 0 || (long long)row0 + ticks > tape->rows || k < 1)
        return fail(h, CMPC_ERR_ARG, name + ": bad argument (k >= 1, and the rows must lie inside the tape)");
    if (!d->dDirStates || !d->dCarryList || !d->dStatus)
        return fail(h, CMPC_ERR_ARG, name + ": dDirStates, dCarryList and dStatus are needed");
    if (d->dDirPlanRot && !d->dCarryListRot)
        return fail(h, CMPC_ERR_ARG, name + ": the planner's orientation directions need dCarryListRot to carry them");
    if (row0 == 0 && !tape->first_row_is_first_tick)
        return fail(h, CMPC_ERR_ARG, name + ": row 0 is not a first tick and has no row before it to take the previous lists from");
    HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, stream);
    const int B = h->B, N = h->cfg.horizon, M = max_contacts;
    const size_t nx = (size_t)B * h->L.nx, np = (size_t)B * h->L.np, ng = (size_t)B * h->L.ng, nt = (size_t)B * 4 * M;
    const size_t cols = (size_t)B * k, nl = cols * 6 * M;
    if (!h->dWalkJvpWs || h->walk_jvp_cols < k || h->walk_jvp_M < M) {
        const int kk = k > h->walk_jvp_cols ? k : h->walk_jvp_cols, mm = M > h->walk_jvp_M ? M : h->walk_jvp_M;
        if (h->dWalkJvpWs) {   // (a larger k or max_contacts: launches that read the old workspace may still be queued)
            HIPCHK(h, hipDeviceSynchronize());
            hipFree(h->dWalkJvpWs);
            h->dWalkJvpWs = nullptr; h->walk_jvp_cols = 0; h->walk_jvp_M = 0;
        }
        HIPCHK(h, hipMalloc(&h->dWalkJvpWs, sizeof(double) * 2 * (size_t)B * kk * 6 * mm + sizeof(float) * (size_t)B * CMPC_SENS + sizeof(int) * (size_t)B));
        h->walk_jvp_cols = kk; h->walk_jvp_M = mm;
    }
    // (the two list buffers carved for this call's k and M; the per-problem words sit behind the full allocation)
    double* wsList = reinterpret_cast<double*>(h->dWalkJvpWs);
    double* wsListRot = wsList + nl;
    float* wsSens = reinterpret_cast<float*>(wsList + 2 * (size_t)B * h->walk_jvp_cols * 6 * h->walk_jvp_M);
    int* wsOk = reinterpret_cast<int*>(wsSens + (size_t)B * CMPC_SENS);
    if (h->tick_ev) HIPCHK(h, hipStreamWaitEvent(st, h->tick_ev, 0));   // (the gate writes workspace an earlier call on another stream may still read)
    const bool rot = d->dCarryListRot || d->dDirPlanRot;
    double* cur = d->dCarryList;  double* other = wsList;               // cur: the list directions entering the next tick; the tick writes `other`
    double* curRot = rot ? d->dCarryListRot : nullptr;  double* otherRot = rot ? wsListRot : nullptr;
    CmpcJvpGateArgs a{};
    a.B = B; a.M = M; a.K = k; a.nx = h->L.nx;
    a.end_tick = dEndTick;
    a.t_sens = wsSens; a.ok_out = wsOk;
    int rc = CMPC_OK;
    for (int i = 0; i <= ticks && rc == CMPC_OK; ++i) {
        // the gate step between tick i - 1 (POST: i > 0) and tick i (PRE: i < ticks), fused into one launch
        const size_t rq = (size_t)(row0 + i - 1), rp = (size_t)(row0 + i);
        a.do_post = i > 0; a.tick_post = tick0 + i - 1;
        if (a.do_post) {
            a.state_out = d->dDirStates + (rq + 1) * cols * 9;
            a.list_out = cur; a.list_rot_out = curRot;     // (what tick i - 1 wrote: the buffers were swapped behind it)
            a.x_row = d->dDirX ? d->dDirX + rq * (size_t)k * nx : nullptr;
            a.status_row = d->dStatus + rq * B;
            a.removed_row = d->dRemoved ? d->dRemoved + rq * B : nullptr;
        }
        a.do_pre = i < ticks; a.tick_pre = tick0 + i; a.first = i == 0;
        a.ok_row = a.do_pre ? tape->dOk + rp * B : nullptr;
        a.first_state = a.first ? d->dDirStates + rp * cols * 9 : nullptr;
        a.first_list = a.first ? d->dCarryList : nullptr;
        a.first_list_rot = a.first ? curRot : nullptr;
        const int lrc = cmpc_launch_walk_jvp_gate(&a, st);
        if (const int err = launch_status(h, "forward walk (gate)", lrc)) return err;
        if (i == ticks) break;
        const bool first_tick = rp == 0;   // (row 0 of a tape whose first row is a first tick: checked above)
        cmpc_tick_tape tt{};
        tt.dX = tape->dX + rp * nx; tt.dP = tape->dP + rp * np; tt.dLamG = tape->dLamG + rp * ng;
        tt.dState = tape->dStates + rp * B * 9; tt.dInfo = tape->dInfo + rp * B * CMPC_INFO;
        tt.dOk = wsOk; tt.dLand = tape->dLand + rp * B * 2;
        tt.dPlanT = tape->dPlanT + rp * nt; tt.dPlanN = tape->dPlanN + rp * B * 2;
        tt.dPrevT = first_tick ? nullptr : tape->dListT + (rp - 1) * nt; tt.dPrevN = first_tick ? nullptr : tape->dListN + (rp - 1) * B * 2;
        tt.dListT = tape->dListT + rp * nt; tt.dListN = tape->dListN + rp * B * 2;
        tt.plant_step = tape->plant_step; tt.plant_substeps = tape->plant_substeps; tt.force_sample_time = tape->force_sample_time;
        cmpc_tick_dirs in{};
        in.dDirState = d->dDirStates + rp * cols * 9;
        in.dDirPrevList = cur; in.dDirPrevListRot = curRot;
        in.dDirPlan = d->dDirPlan; in.dDirPlanRot = d->dDirPlanRot;
        in.dDirWrench = d->dDirWrench ? d->dDirWrench + rp * cols * 6 * N : nullptr;
        in.dDirModel = d->dDirModel;
        in.dDirP = d->dDirP ? d->dDirP + rp * (size_t)k * np : nullptr;
        cmpc_tick_dirs_out out{};
        out.dDirStateOut = d->dDirStates + (rp + 1) * cols * 9;
        out.dDirList = other; out.dDirListRot = otherRot;
        out.dDirX = d->dDirX ? d->dDirX + rp * (size_t)k * nx : nullptr;
        // the mismatch entry: tick rp ran under its own schedule row (selected by tick number); its direction rows are the tape row's, applied whether or
        // not the tick lay inside the schedule's range
        TickMismatchDirs mm{};
        const float* unused;
        mismatch_rows(m, B, tick0 + i, &mm.hidden, &unused, &mm.gain);
        if (md) {
            mm.d_hidden = md->dDirHidden ? md->dDirHidden + rp * cols * 6 : nullptr;
            mm.d_noise = md->dDirNoise ? md->dDirNoise + rp * cols * 9 : nullptr;
            mm.d_gain = md->dDirGain;
        }
        // (a tick with no row, no gain and no direction is the plain tick: the rule of cmpc_rollout_tick_jvp_mismatch_device, so walk = ticks to the bit)
        const bool plain = !mm.hidden && !mm.gain && !mm.d_hidden && !mm.d_noise && !mm.d_gain;
        rc = tick_jvp(h, M, (double)(tick0 + i) * h->cfg.sampling_time, &tt, k, &in, &out, wsSens, stream, plain ? nullptr : &mm, tick_who);
        std::swap(cur, other); std::swap(curRot, otherRot);
    }
    if (rc == CMPC_OK && cur != d->dCarryList) {     // (an odd number of ticks: the lists leaving the last row sit in the workspace)
        HIPCHK(h, hipMemcpyAsync(d->dCarryList, cur, sizeof(double) * nl, hipMemcpyDeviceToDevice, st));
        if (rot) HIPCHK(h, hipMemcpyAsync(d->dCarryListRot, curRot, sizeof(double) * nl, hipMemcpyDeviceToDevice, st));
    }
    if (rc == CMPC_OK && h->tick_ev) HIPCHK(h, hipEventRecord(h->tick_ev, st));
    return rc;
}

int cmpc_rollout_walk_jvp_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick, int k,
                                 const cmpc_walk_dirs* d, void* stream)
{
    return walk_jvp(h, "cmpc_rollout_walk_jvp_device", "cmpc_rollout_tick_jvp_device", max_contacts, tick0, ticks, tape, row0, dEndTick, k, d, stream);
}

int cmpc_rollout_walk_jvp_mismatch_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_tape* tape, int row0, const int* dEndTick,
                                          int k, const cmpc_walk_dirs* d, const cmpc_plant_mismatch* m, const cmpc_walk_dirs_mismatch* md, void* stream)
{
    return walk_jvp(h, "cmpc_rollout_walk_jvp_mismatch_device", "cmpc_rollout_tick_jvp_mismatch_device", max_contacts, tick0, ticks, tape, row0, dEndTick, k,
                    d, stream, m, md);
}

// the handle's own contact blocks from contact lists (what the class facade's setContactPhaseList calls)
int cmpc_set_contact_lists(cmpc_handle h, int max_contacts, double now, const double* t, const float* pose, const int* n,
                           const float* box_upper, const float* box_lower, int* land)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_set_contact_lists: null handle");
    int rc = ensure_buffers(h);
    if (rc) return rc;
    for (int c = 0; box_upper && box_lower && c < 6; ++c)
        if (box_upper[c] < box_lower[c]) return fail(h, CMPC_ERR_ARG, "cmpc_set_contact_lists: bounding box upper < lower");
    rc = cmpc_contacts_sample(h->cfg.horizon, h->cfg.sampling_time, h->B, max_contacts, now, t, pose, n, box_upper, box_lower, h->hP.data(), land);
    if (rc) return fail(h, rc, g_err);
    return CMPC_OK;
}


// ---- per-problem models (include/cmpc.h) ----
void cmpc_model_from_config(const cmpc_config* cfg, cmpc_model* m)
{
    if (!cfg || !m) return;
    m->friction_coefficient = cfg->friction_coefficient;
    for (int i = 0; i < 3; ++i) m->com_weight[i] = cfg->com_weight[i];
    m->angular_momentum_weight = cfg->angular_momentum_weight;
    m->contact_position_weight = cfg->contact_position_weight;
    for (int i = 0; i < 3; ++i) m->force_rate_of_change_weight[i] = cfg->force_rate_of_change_weight[i];
    m->contact_force_symmetry_weight = cfg->contact_force_symmetry_weight;
    std::memcpy(m->corners, cfg->corners, sizeof(m->corners));
}

static std::string model_field_name(int i)
{
    static const char* const scalar[] = {"friction_coefficient", "com_weight[0]", "com_weight[1]", "com_weight[2]", "angular_momentum_weight",
                                         "contact_position_weight", "force_rate_of_change_weight[0]", "force_rate_of_change_weight[1]",
                                         "force_rate_of_change_weight[2]", "contact_force_symmetry_weight"};
    if (i < 10) return scalar[i];
    const int e = i - 10;
    return "corners[" + std::to_string(e / 12) + "][" + std::to_string(e / 3 % 4) + "][" + std::to_string(e % 3) + "]";
}

int cmpc_check_models(const cmpc_model* models, int batch)
{
    if (!models || batch < 1) return fail(nullptr, CMPC_ERR_ARG, "cmpc_check_models: null table or batch < 1");
    for (int b = 0; b < batch; ++b) {
        const int i = cmpc_model_first_bad(models[b]);
        if (i < 0) continue;
        const char* rule = i == 0 ? "must be > 0 and finite" : (i >= 6 && i <= 8) ? "must be > 0 and finite" : i < 10 ? "must be >= 0 and finite" : "must be finite";
        char val[40];
        std::snprintf(val, sizeof(val), "%.17g", (&models[b].friction_coefficient)[i]);
        return fail(nullptr, CMPC_ERR_ARG, "model " + std::to_string(b) + ": " + model_field_name(i) + " = " + val + " " + rule);
    }
    return CMPC_OK;
}

static int ensure_models(cmpc_handle h)
{
    if (!h->dModels) HIPCHK(h, hipMalloc(&h->dModels, sizeof(CmpcConsts) * (size_t)h->B));
    return CMPC_OK;
}

int cmpc_set_models(cmpc_handle h, const cmpc_model* models)
{
    if (!h) return fail(nullptr, CMPC_ERR_ARG, "cmpc_set_models: null handle");
    if (!models) {
        h->models_set = false;   // (the table stays allocated: launches already queued may still read it)
        return CMPC_OK;
    }
    if (cmpc_check_models(models, h->B) != CMPC_OK) return fail(h, CMPC_ERR_ARG, "cmpc_set_models: " + g_err);
    HIPCHK(h, hipSetDevice(h->device));
    CmpcConsts base;
    fill_consts(h, base);
    std::vector<CmpcConsts> rec((size_t)h->B, base);
    for (int b = 0; b < h->B; ++b) cmpc_consts_apply_model(rec[b], models[b], h->hExpK);
    int rc = ensure_models(h);
    if (rc) return rc;
    HIPCHK(h, hipDeviceSynchronize());   // (launches queued on any stream may still read the previous table)
    HIPCHK(h, hipMemcpy(h->dModels, rec.data(), sizeof(CmpcConsts) * rec.size(), hipMemcpyHostToDevice));
    h->models_set = true;
    return CMPC_OK;
}

namespace {
// one thread per problem: the handle's record, then problem b's model over it (cmpc_consts_apply_model: the host's statement, bit-equal records).
// A row that breaks the model rule keeps the handle's model and is flagged (the solve returns status 3).
__global__ __launch_bounds__(256) void cmpc_models_kernel(int B, const CmpcConsts* __restrict__ base, const double* __restrict__ expk,
                                                          const cmpc_model* __restrict__ models, CmpcConsts* __restrict__ out, int* __restrict__ ok)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int* src = reinterpret_cast<const int*>(base);
    int* dst = reinterpret_cast<int*>(out + b);
    for (int e = 0; e < (int)(sizeof(CmpcConsts) / 4); ++e) dst[e] = src[e];
    const cmpc_model m = models[b];
    const bool bad = cmpc_model_first_bad(m) >= 0;
    if (!bad) cmpc_consts_apply_model(out[b], m, expk);
    out[b].model_bad = bad ? 1 : 0;
    if (ok) ok[b] = bad ? 0 : 1;
}
}  // namespace

int cmpc_set_models_device(cmpc_handle h, const cmpc_model* dModels, int* dOk, void* stream)
{
    if (!h || !dModels) return fail(h, CMPC_ERR_ARG, "cmpc_set_models_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure_models(h);
    if (rc) return rc;
    hipLaunchKernelGGL(cmpc_models_kernel, dim3((h->B + 255) / 256), dim3(256), 0, stream_of(h, stream), h->B, h->dConsts, h->dExpK,
                       dModels, h->dModels, dOk);
    HIPCHK(h, hipGetLastError());
    h->models_set = true;
    return CMPC_OK;
}

}  // extern "C"
