// C ABI of libcmpc_hip.so, the derivatives of the roll-out layer (include/cmpc.h): the tick and the walk in reverse and forwards, and their gates.  Host
// code only: every kernel and its launcher is in cmpc_rollout.hip / cmpc_contacts.hip (cmpc_launch.h).
#include "cmpc_handle.h"

#include <algorithm>
#include <string>

extern "C" {

// ---- one tick in reverse (include/cmpc.h): plant VJP -> adjust part of the list VJP -> cmpc_solution_vjp_model_device -> the state rows of gP and the flags
// (cmpc_tick_vjp_combine_kernel) -> sample + merge part of the list VJP [-> the orientation list VJP], on one stream ----
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
        rc = cmpc_launch_axpy_float(nx, dGradX, gX, st);
        if (const int err = launch_status(h, "tick VJP (dGradX)", rc)) return err;
    }
    if (dGradListOut) {
        rc = cmpc_launch_contacts_position_vjp(B, N, max_contacts, h->cfg.sampling_time, now, 1, dt_ns, tape->dPlanT, tape->dPlanN, tape->dPrevT, tape->dPrevN,
                                               tape->dListT, tape->dListN, tape->dLand, tape->dOk, dGradListOut, nullptr, gX, nullptr, nullptr, nullptr, st);
        if (const int err = launch_status(h, "tick VJP (adjust)", rc)) return err;
    }
    rc = rot ? cmpc_solution_vjp_rot_device(h, tape->dX, tape->dP, tape->dLamG, gX, gpSol, gmSol, grSol, dTickSens, stream)
             : cmpc_solution_vjp_model_device(h, tape->dX, tape->dP, tape->dLamG, gX, gpSol, gmSol, dTickSens, stream);
    if (rc != CMPC_OK) return rc;
    rc = cmpc_launch_tick_vjp_combine(B, N, tape->dInfo, tape->dOk, gpSol, gpPlant, gmSol, gmPlant, dGradState, dGradWrench, dGradModel, dGradP, dTickSens,
                                      okTick, rot ? grPlant : nullptr, rot ? grSol : nullptr, ghPlant, ggPlant, mm ? mm->g_hidden : nullptr,
                                      mm ? mm->g_noise : nullptr, mm ? mm->g_gain : nullptr, st);
    if (const int err = launch_status(h, "tick VJP (combine)", rc)) return err;
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
    rc = cmpc_launch_tick_jvp_assemble(cols, N, in->dDirState, in->dDirWrench, in->dDirP, dPF, mm ? mm->d_noise : nullptr, st);
    if (const int err = launch_status(h, "tick JVP (assemble)", rc)) return err;
    rc = cmpc_solution_jvp_rot_device(h, tape->dX, tape->dP, tape->dLamG, dPF, in->dDirModel, dRot, k, dDX, dTickSens, stream);
    if (rc != CMPC_OK) return rc;
    rc = cmpc_launch_tick_jvp_flag(B, N, k, tape->dInfo, tape->dOk, tape->dState, dTickSens, dDX, dPF, dRot, wsRot0, okTick, st);
    if (const int err = launch_status(h, "tick JVP (flags)", rc)) return err;
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

// ---- sensed pushes (include/cmpc.h, cmpc_wrench_sensor): the sensor's transpose and its tangent; the host forms run the kernels' own per-entry functions ----
static const char* sense_grad_refusal(int horizon, int batch, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s)
{
    if (horizon < 1 || batch < 1 || tick0 < 0 || rows < 1) return "bad argument";
    return sensor_refusal(horizon, m, s);
}

static CmpcSenseVjpArgs sense_vjp_args(int N, int B, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, const float* gw,
                                       const double* gh, double* gt, double* gn)
{
    return CmpcSenseVjpArgs{sense_args(N, B, tick0, rows, m, s), gw, gh, gt, s->dSensorNoise ? gn : nullptr};
}

int cmpc_wrench_sense_vjp(int horizon, int batch, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, const float* grad_wrench,
                          const double* grad_hidden, double* grad_hidden_true, double* grad_sensor_noise)
{
    if (const char* why = sense_grad_refusal(horizon, batch, tick0, rows, m, s)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_wrench_sense_vjp: ") + why);
    if (!grad_wrench || !grad_hidden || !grad_hidden_true) return fail(nullptr, CMPC_ERR_ARG, "cmpc_wrench_sense_vjp: null argument");
    const CmpcSenseVjpArgs v = sense_vjp_args(horizon, batch, tick0, rows, m, s, grad_wrench, grad_hidden, grad_hidden_true, grad_sensor_noise);
    const int out_rows = std::max(v.s.hidden_ticks, v.grad_noise ? v.s.noise_ticks : 0);
    for (int r = 0; r < out_rows; ++r)
        for (int b = 0; b < batch; ++b)
            for (int c = 0; c < 6; ++c) cmpc_wrench_sense_vjp_entry(v, r, b, c);
    return CMPC_OK;
}

int cmpc_wrench_sense_vjp_device(cmpc_handle h, int tick0, int rows, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s, const float* dGradWrench,
                                 const double* dGradHidden, double* dGradHiddenTrue, double* dGradSensorNoise, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_wrench_sense_vjp_device: null handle");
    if (const char* why = sense_grad_refusal(h->cfg.horizon, h->B, tick0, rows, m, s))
        return fail(h, CMPC_ERR_ARG, std::string("cmpc_wrench_sense_vjp_device: ") + why);
    if (!dGradWrench || !dGradHidden || !dGradHiddenTrue) return fail(h, CMPC_ERR_ARG, "cmpc_wrench_sense_vjp_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    const CmpcSenseVjpArgs v = sense_vjp_args(h->cfg.horizon, h->B, tick0, rows, m, s, dGradWrench, dGradHidden, dGradHiddenTrue, dGradSensorNoise);
    return launch_status(h, "wrench sensor VJP", cmpc_launch_wrench_sense_vjp(&v, stream_of(h, stream)));
}

int cmpc_wrench_sense_jvp(int horizon, int batch, int tick0, int rows, int k, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s,
                          const double* dir_hidden, const double* dir_sensor_noise, float* dir_wrench, double* dir_plant_wrench)
{
    if (const char* why = sense_grad_refusal(horizon, batch, tick0, rows, m, s)) return fail(nullptr, CMPC_ERR_ARG, std::string("cmpc_wrench_sense_jvp: ") + why);
    if (k < 1 || !dir_hidden || !dir_wrench || !dir_plant_wrench) return fail(nullptr, CMPC_ERR_ARG, "cmpc_wrench_sense_jvp: k >= 1 and the arrays are needed");
    const CmpcSenseJvpArgs v{sense_args(horizon, batch, tick0, rows, m, s), k, dir_hidden, s->dSensorNoise ? dir_sensor_noise : nullptr, dir_wrench,
                             dir_plant_wrench};
    for (int r = 0; r < rows; ++r)
        for (int b = 0; b < batch; ++b)
            for (int j = 0; j < k; ++j)
                for (int q = 0; q < horizon; ++q) cmpc_wrench_sense_jvp_entry(v, r, b, j, q);
    return CMPC_OK;
}

int cmpc_wrench_sense_jvp_device(cmpc_handle h, int tick0, int rows, int k, const cmpc_plant_mismatch* m, const cmpc_wrench_sensor* s,
                                 const double* dDirHidden, const double* dDirSensorNoise, float* dDirWrench, double* dDirPlantWrench, void* stream)
{
    if (!h) return fail(h, CMPC_ERR_ARG, "cmpc_wrench_sense_jvp_device: null handle");
    if (const char* why = sense_grad_refusal(h->cfg.horizon, h->B, tick0, rows, m, s))
        return fail(h, CMPC_ERR_ARG, std::string("cmpc_wrench_sense_jvp_device: ") + why);
    if (k < 1 || !dDirHidden || !dDirWrench || !dDirPlantWrench)
        return fail(h, CMPC_ERR_ARG, "cmpc_wrench_sense_jvp_device: k >= 1 and the arrays are needed");
    HIPCHK(h, hipSetDevice(h->device));
    const CmpcSenseJvpArgs v{sense_args(h->cfg.horizon, h->B, tick0, rows, m, s), k, dDirHidden, s->dSensorNoise ? dDirSensorNoise : nullptr, dDirWrench,
                             dDirPlantWrench};
    return launch_status(h, "wrench sensor JVP", cmpc_launch_wrench_sense_jvp(&v, stream_of(h, stream)));
}

}  // extern "C"
