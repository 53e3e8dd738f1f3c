// C ABI of libcmpc_hip.so (include/cmpc.h): handle management, host<->device plumbing, launches.  The roll-out layer's entry points are in
// cmpc_api_rollout.hip and cmpc_api_walk_grad.hip; the helpers the three files share are defined here and there and declared in cmpc_handle.h.
#include "cmpc_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

static thread_local std::string g_err;

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

namespace cmpc_host {

int fail(cmpc_handle h, int code, const std::string& msg)
{
    if (h) h->err = msg;
    g_err = msg;
    return code;
}

// the stream of a call: the caller's, or the handle's
hipStream_t stream_of(cmpc_handle h, void* stream) { return stream ? (hipStream_t)stream : h->stream; }

// a launcher's return code as the entry point's: CMPC_OK, or CMPC_ERR_HIP with "<what> launch: <the HIP error string>"
int launch_status(cmpc_handle h, const char* what, int rc)
{
    return rc == 0 ? CMPC_OK : fail(h, CMPC_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString((hipError_t)rc));
}

// the corners the plant step reads: problem 0's, and the distance in floats to the next problem's (0: one set for the batch).  Device pointer arithmetic only.
const float* model_corners(cmpc_handle h) { return h->models_set ? h->dModels->corners : h->dConsts->corners; }
int corners_stride(cmpc_handle h) { return h->models_set ? (int)(sizeof(CmpcConsts) / sizeof(float)) : 0; }

void fill_params(cmpc_handle h, CmpcParams& p)
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
int solve_device_impl(cmpc_handle h, const float* dP, const float* dX0, float* dX, float* dInfo, void* stream, bool warm, const int* start, int tick)
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

// what both forms of the record refuse in a cmpc_walk_limits; null: nothing.  (height_min > height_max is false when either is NaN: a limit that is off)
const char* limits_refusal(const cmpc_walk_limits* lim)
{
    if (lim->height_min > lim->height_max) return "height_min above height_max";
    if (lim->dMeasures && lim->rows < 1) return "dMeasures with rows < 1";
    return nullptr;
}

// forceSampleTime (CentroidalMPCBlock.cpp:586-592): dt in integer nanoseconds, or 0 if it is not a usable grid
long long snap_dt_ns(double dt)
{
    if (!(dt > 0) || !(dt < CMPC_TIME_NEVER)) return 0;
    const long long dt_ns = llround(dt * 1e9);
    return dt_ns >= 1 ? dt_ns : 0;
}

// the bounding boxes of the two contacts on the device (uploaded when they change)
int upload_box(cmpc_handle h, const float* box_upper, const float* box_lower, hipStream_t st)
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

int ensure_models(cmpc_handle h)
{
    if (!h->dModels) HIPCHK(h, hipMalloc(&h->dModels, sizeof(CmpcConsts) * (size_t)h->B));
    return CMPC_OK;
}

}  // namespace cmpc_host

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
    hipFree(h->dSnapT); hipFree(h->dSnapOk); hipFree(h->dSenseWrench); hipFree(h->dTickWs); hipFree(h->dTickJvpWs); hipFree(h->dWalkWs); hipFree(h->dWalkJvpWs); if (h->tick_ev) hipEventDestroy(h->tick_ev); hipFree(h->dExpK); hipFree(h->dModels);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
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
