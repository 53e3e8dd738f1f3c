// C ABI of libcmpc_hip.so, the roll-out layer (include/cmpc.h): the tick, the record and the measures, the tape, the walks and the refill walks, snapshot and
// regroup.  Host code only: every kernel and its launcher is in cmpc_rollout.hip / cmpc_contacts.hip (cmpc_launch.h).
#include "cmpc_handle.h"

#include <algorithm>
#include <cstring>
#include <string>

static_assert(sizeof(cmpc_walk_refill_plans) == 104, "cmpc_walk_refill_plans: the size include/cmpc.h states");
static_assert(sizeof(cmpc_walk_refill_trials) == 56, "cmpc_walk_refill_trials: the size include/cmpc.h states");
static_assert(sizeof(cmpc_walk_refill_snapshot) == 32, "cmpc_walk_refill_snapshot: the size include/cmpc.h states");
static_assert(sizeof(cmpc_wrench_sensor) == 32, "cmpc_wrench_sensor: the size include/cmpc.h states");

namespace cmpc_host {

int mismatch_check(cmpc_handle h, const char* who, const cmpc_plant_mismatch* m)
{
    if (m && (m->hidden_ticks < 0 || m->noise_ticks < 0 || (m->dHiddenWrench && m->hidden_ticks == 0) || (m->dStateNoise && m->noise_ticks == 0)))
        return fail(h, CMPC_ERR_ARG, std::string(who) + ": bad mismatch (a negative count, or a schedule with no rows)");
    return CMPC_OK;
}

// the rows of tick number `tick`: a schedule's row inside its range, else null (the term is then not applied: a select on the host, no add of zero)
void mismatch_rows(const cmpc_plant_mismatch* m, int B, int tick, const float** hidden, const float** noise, const float** gain)
{
    *hidden = nullptr; *noise = nullptr; *gain = nullptr;
    if (!m) return;
    const long long r = (long long)tick - m->tick_first;
    if (m->dHiddenWrench && r >= 0 && r < m->hidden_ticks) *hidden = m->dHiddenWrench + (size_t)r * B * 6;
    if (m->dStateNoise && r >= 0 && r < m->noise_ticks) *noise = m->dStateNoise + (size_t)r * B * 9;
    *gain = m->dForceGain;
}

bool tape_complete(const cmpc_walk_tape* t)
{
    return t && t->rows >= 1 && t->dX && t->dP && t->dLamG && t->dInfo && t->dStates && t->dOk && t->dLand && t->dPlanT && t->dListT && t->dPlanN && t->dListN &&
           t->plant_step > 0 && t->plant_substeps >= 1;
}

// the wrench sensor (include/cmpc.h, cmpc_wrench_sensor): why a sensor and the schedule it reads are refused, or null.  N <= 0: the horizon is not known yet
// (the upper end of hold_knots is then the caller's to check again)
const char* sensor_refusal(int N, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s)
{
    if (!s || !m) return "null sensor or mismatch";
    if (!m->dHiddenWrench || m->hidden_ticks < 1) return "a sensor needs the hidden-wrench schedule it reads (dHiddenWrench, hidden_ticks >= 1)";
    if (s->delay_ticks < 0) return "delay_ticks is negative";
    if (s->hold_knots < 1 || (N > 0 && s->hold_knots > N)) return "hold_knots lies outside 1..N";
    if (!(s->deadband >= 0.0)) return "deadband is negative or NaN";
    if (s->noise_ticks < 0 || (s->dSensorNoise && s->noise_ticks < 1)) return "bad sensor noise (a negative count, or a schedule with no rows)";
    return nullptr;
}

CmpcSenseArgs sense_args(int N, int B, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s)
{
    return CmpcSenseArgs{N, B, tick0, rows, m->tick_first, m->dHiddenWrench, m->hidden_ticks, s->delay_ticks, s->hold_knots, s->deadband * s->deadband,
                         s->dSensorNoise, s->dSensorNoise ? s->noise_ticks : 0};
}

}  // namespace cmpc_host

extern "C" {

// ---- 8f-1 .. 8f-4 chained: one tick of the receding-horizon loop in one call (include/cmpc.h): the steps of cmpc_api.hip's entry points in the reference's order, with the
// same argument checks, as THREE launches -- everything in front of the solve, the solve, everything behind it (cmpc_tick_pre_kernel / cmpc_tick_post_kernel call the same
// per-problem functions as the single kernels; results identical to the last bit). ----
// cold: the solve starts from cmpc_cold_start_kernel, launched between the front kernel and the solve (the first tick of cmpc_rollout_walk_device; needs
// warm == 0).  box_done: the caller has uploaded the box already.
// m: the plant mismatch (include/cmpc.h, cmpc_plant_mismatch) with `tick` selecting its rows, or null -- then every launch is the one this function always queued
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

// tape != null: the tape part around the ticks (cmpc_rollout_walk_taped_device, which has checked it); null: the launches of cmpc_rollout_walk_device
// m: the plant mismatch, every tick passing its own number tick0 + i (no launch more per tick, nothing more on the tape: dStates holds the true state, dP the measured one)
static int rollout_walk_impl(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                             int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream,
                             const cmpc_plant_mismatch* m = nullptr, const cmpc_wrench_sensor* s = nullptr, float* dPlantWrench = nullptr)
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
    if (s && !h->dSenseWrench) HIPCHK(h, hipMalloc(&h->dSenseWrench, sizeof(float) * (size_t)h->B * h->cfg.horizon * 6));
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
        // s: the sense launch writes this tick's wrench rows and its plant row; the tick then takes its hidden row from there and its noise row and gain from m
        cmpc_plant_mismatch sensed{};
        if (s) {
            const float *m_hidden, *m_noise, *m_gain;
            mismatch_rows(m, h->B, tick0 + i, &m_hidden, &m_noise, &m_gain);
            float* const plant_row = dPlantWrench + (size_t)i * h->B * 6;
            const CmpcSenseArgs sa = sense_args(h->cfg.horizon, h->B, tick0 + i, 1, m, s);
            rc = launch_status(h, "walk (wrench sensor)", cmpc_launch_wrench_sense(&sa, h->dSenseWrench, plant_row, nullptr, st));
            if (rc != CMPC_OK) break;
            t.dWrench = h->dSenseWrench;
            sensed.tick_first = tick0 + i;
            sensed.dHiddenWrench = plant_row; sensed.hidden_ticks = 1;
            sensed.dStateNoise = m_noise; sensed.noise_ticks = m_noise ? 1 : 0;
            sensed.dForceGain = m_gain;
        }
        const cmpc_plant_mismatch* const mt = s ? &sensed : m;
        const int* const ok_read = (cold && !t.force_sample_time) ? nullptr : t.dOk;
        if (tape && i == 0)   // (the ticks run in place: the state the first one starts from is copied in front of it)
            rc = rollout_tape_impl(h, max_contacts, tape_row0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, t.dState, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   tape, stream);
        if (rc == CMPC_OK) rc = rollout_tick_impl(h, max_contacts, now, cold ? 0 : 1, &t, stream, cold, true, tick0 + i, mt);
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

int cmpc_rollout_walk_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                             int row0, int lists_in, int* lists_out, void* stream)
{
    return rollout_walk_impl(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, nullptr, 0, stream);
}

static int walk_taped(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                      int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream, const cmpc_plant_mismatch* m,
                      const cmpc_wrench_sensor* s = nullptr, float* dPlantWrench = nullptr)
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
    return rollout_walk_impl(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, tape, tape_row0, stream, m, s, dPlantWrench);
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

// ---- sensed pushes (include/cmpc.h, cmpc_wrench_sensor): the sensor's rows on the host and in one launch, and the walk with a sense launch per tick ----
static const char* sense_rows_refusal(int horizon, int batch, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s)
{
    if (horizon < 1 || batch < 1 || tick0 < 0 || rows < 1) return "bad argument";
    return sensor_refusal(horizon, m, s);
}

int cmpc_wrench_sense(int horizon, int batch, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, float* wrench_rows,
                      float* plant_wrench, int* pass)
{
    if (const char* why = sense_rows_refusal(horizon, batch, tick0, rows, m, s)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_wrench_sense: ") + why);
    if (!plant_wrench) return fail(nullptr, CMPC_ERR_ARG, "cmpc_wrench_sense: plant_wrench is needed");
    const CmpcSenseArgs a = sense_args(horizon, batch, tick0, rows, m, s);
    const int knots = wrench_rows ? horizon : 1;
    for (int r = 0; r < rows; ++r)
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < knots; ++k) cmpc_wrench_sense_entry(a, wrench_rows, plant_wrench, pass, r, b, k);
    return CMPC_OK;
}

int cmpc_wrench_sense_device(cmpc_handle h, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, float* dWrenchRows,
                             float* dPlantWrench, int* dPass, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_wrench_sense_device: null handle");
    if (const char* why = sense_rows_refusal(h->cfg.horizon, h->B, tick0, rows, m, s))
        return fail(h, CMPC_ERR_ARG, std::string("cmpc_wrench_sense_device: ") + why);
    if (!dPlantWrench) return fail(h, CMPC_ERR_ARG, "cmpc_wrench_sense_device: dPlantWrench is needed");
    HIPCHK(h, hipSetDevice(h->device));
    const CmpcSenseArgs a = sense_args(h->cfg.horizon, h->B, tick0, rows, m, s);
    return launch_status(h, "wrench sensor", cmpc_launch_wrench_sense(&a, dWrenchRows, dPlantWrench, dPass, stream_of(h, stream)));
}

// (the checks that need no handle come first, so that each is refused without a device too)
int cmpc_rollout_walk_sensed_device(cmpc_handle h, int max_contacts, int tick0, int ticks, int cold_first, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                    int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, const cmpc_plant_mismatch* m,
                                    const cmpc_wrench_sensor* s, float* dPlantWrench, void* stream)
{
    if (s) {
        if (io && (io->dWrenchTicks || io->tick.dWrench))
            return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_sensed_device: dWrenchTicks or tick.dWrench is set (a known push and a sensed one are not summed)");
        if (!m || !m->dHiddenWrench || !dPlantWrench)
            return fail(h, CMPC_ERR_ARG, "cmpc_rollout_walk_sensed_device: a sensor needs m->dHiddenWrench and dPlantWrench");
        if (const char* why = sensor_refusal(h ? h->cfg.horizon : 0, m, s)) return fail(h, CMPC_ERR_ARG, std::string("cmpc_rollout_walk_sensed_device: ") + why);
    }
    if (tape) return walk_taped(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, tape, tape_row0, stream, m, s, dPlantWrench);
    return rollout_walk_impl(h, max_contacts, tick0, ticks, cold_first, io, rec, row0, lists_in, lists_out, nullptr, 0, stream, m, s, dPlantWrench);
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

// ---- trials from a snapshot (include/cmpc.h, cmpc_walk_refill_snapshot): the restore step between the refill launch and the front kernel ----
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

// the refill walk: per tick the refill launch, the tick's three launches (front and back kernels in refill mode, the warm solve with the per-problem cold
// policy) and the record with local tick numbers.  trials (cmpc_walk_refill_trials) null, or with nothing set: the launches this function always queued;
// else the front and back kernels' per-trial instantiations, each only when it has something to do, and the handle's per-problem table as the solve's and
// the back kernel's records when there are per-trial models
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
                            int lists_in, int* lists_out, void* stream, const cmpc_walk_tape* tape = nullptr, int tape_row0 = 0,
                            const cmpc_walk_refill_plans* plans = nullptr)
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

int cmpc_rollout_walk_refill_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                    const cmpc_walk_refill* refill, int row0, int lists_in, int* lists_out, void* stream)
{
    return cmpc_rollout_walk_refill_trials_device(h, max_contacts, tick0, ticks, io, rec, refill, nullptr, row0, lists_in, lists_out, stream);
}

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

// the taped call with a plan pool (include/cmpc.h); plans null: the taped call itself, and with tape null as well the trials call
int cmpc_rollout_walk_refill_plans_device(cmpc_handle h, int max_contacts, int tick0, int ticks, const cmpc_walk_io* io, const cmpc_walk_record* rec,
                                          const cmpc_walk_refill* refill, const cmpc_walk_refill_trials* trials, const cmpc_walk_refill_plans* plans,
                                          int row0, int lists_in, int* lists_out, const cmpc_walk_tape* tape, int tape_row0, void* stream)
{
    return walk_refill_impl(h, max_contacts, tick0, ticks, io, rec, refill, trials, nullptr, row0, lists_in, lists_out, stream, tape, tape_row0, plans);
}

// ---- the snapshot of a walk (include/cmpc.h, cmpc_walk_snapshot): one copy kernel, destination problem b <- source problem index[b] ----
size_t cmpc_walk_snapshot_bytes(int horizon, int max_contacts)
{
    if (horizon < 1 || max_contacts < 1) return 0;
    CmpcLayout L;
    cmpc_layout_init(L, horizon);
    return sizeof(float) * (2 * (size_t)L.nx + L.np) + 176 * (size_t)max_contacts + 160;
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

}  // extern "C"
