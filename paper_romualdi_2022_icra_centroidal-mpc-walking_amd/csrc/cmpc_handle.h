// The handle of the C ABI and the host helpers that more than one of its files needs.  Internal: included by cmpc_api.hip, cmpc_api_rollout.hip and
// cmpc_api_walk_grad.hip only, never installed, never included by include/cmpc.h.
#pragma once
#include "../../include/cmpc.h"
#include "cmpc_contacts.h"
#include "cmpc_device.h"
#include "cmpc_launch.h"

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
    float* dSenseWrench = nullptr; // the wrench rows [B][N][6] a sensed walk's tick reads (cmpc_rollout_walk_sensed_device, allocated on first use)
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

#define HIPCHK(h, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(h, CMPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));  \
    } while (0)

// Each helper is defined once, in the file named; hidden, so that none of them is a symbol of the library.  The error text of a thread without a handle
// (g_err) is cmpc_api.hip's alone: reached through fail and cmpc_last_error.
#pragma GCC visibility push(hidden)
namespace cmpc_host {

// ---- cmpc_api.hip ----
int fail(cmpc_handle h, int code, const std::string& msg);
hipStream_t stream_of(cmpc_handle h, void* stream);
int launch_status(cmpc_handle h, const char* what, int rc);
const float* model_corners(cmpc_handle h);
int corners_stride(cmpc_handle h);
void fill_params(cmpc_handle h, CmpcParams& p);
int solve_device_impl(cmpc_handle h, const float* dP, const float* dX0, float* dX, float* dInfo, void* stream, bool warm, const int* start = nullptr,
                      int tick = 0);
const char* limits_refusal(const cmpc_walk_limits* lim);
long long snap_dt_ns(double dt);
int upload_box(cmpc_handle h, const float* box_upper, const float* box_lower, hipStream_t st);
int ensure_models(cmpc_handle h);

// ---- cmpc_api_rollout.hip ----
int mismatch_check(cmpc_handle h, const char* who, const cmpc_plant_mismatch* m);
void mismatch_rows(const cmpc_plant_mismatch* m, int B, int tick, const float** hidden, const float** noise, const float** gain);
bool tape_complete(const cmpc_walk_tape* t);
const char* sensor_refusal(int N, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s);
CmpcSenseArgs sense_args(int N, int B, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s);

}  // namespace cmpc_host
#pragma GCC visibility pop
using namespace cmpc_host;
