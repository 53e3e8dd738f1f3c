// Contact-schedule logic shared by the host entry points and the device kernels:
//   * the merge of the planner's footsteps with the MPC-adjusted current contact -- updateContactPhaseList,
//     src/centroidal-mpc-walking/src/CentroidalMPCBlock.cpp:32-110 (call site :594-607);
//   * the sampling of a contact list at the MPC knots into the parameter tensors -- the job of
//     CentroidalMPC::setContactPhaseList (call site :609; the rule itself lives in BipedalLocomotionFramework, whose
//     source is not in the reference tree: ours is stated in contacts.py and restated here);
//   * the step adjustment getOutput() reports (:598, :626): the next contact takes the optimised landing position.
// One foot of one problem = a list of at most M contacts sorted by activation time:
//   t[m][2]    activation, deactivation time in seconds (double)
//   pose[m][7] position x y z, orientation quaternion w x y z (float)
#pragma once
#include "cmpc_device.h"

#define CMPC_TIME_EPS 1e-9

// ContactPhaseList::forceSampleTime(dT) (CentroidalMPCBlock.cpp:586-592): the planner's times snapped to the MPC grid before the merge.  The rule
// (include/cmpc.h, cmpc_contacts_force_sample_time; BLF's own is not in the reference tree: parity unpinned) on integer nanoseconds:
// t_ns = llround(t 1e9); to the nearest multiple of dt_ns from time 0, ties to the later one; a time already on the grid keeps its bits; |t| >= 1e9 s
// (the "never" sentinel) is kept.  Returns false for a non-finite time (*out = t).  dt_ns >= 1.
#define CMPC_TIME_NEVER 1e9
__host__ __device__ inline bool cmpc_snap_time(double t, long long dt_ns, double* out)
{
    *out = t;
    if (!__builtin_isfinite(t)) return false;
    if (fabs(t) >= CMPC_TIME_NEVER) return true;
    const long long t_ns = llround(t * 1e9);   // |t_ns| < 1e18: 2 t_ns + dt_ns does not overflow for dt_ns < 1e18
    if (t_ns % dt_ns == 0) return true;
    const long long num = 2 * t_ns + dt_ns, den = 2 * dt_ns;
    long long q = num / den;                   // C++ truncates towards zero: floor for a negative quotient
    if (num % den != 0 && num < 0) --q;
    *out = (double)(q * dt_ns) * 1e-9;
    return true;
}
// one contact (activation, deactivation) of a list: in[] and out[] may alias.  False when a time is not finite or a contact of positive duration
// collapses to zero duration (the reference's forceSampleTime returns false, :588-592).
__host__ __device__ inline bool cmpc_snap_contact(const double* in, long long dt_ns, double* out)
{
    const double a = in[0], d = in[1];
    double sa, sd;
    const bool fa = cmpc_snap_time(a, dt_ns, &sa), fd = cmpc_snap_time(d, dt_ns, &sd);
    out[0] = sa; out[1] = sd;
    return fa && fd && !(d > a && sd == sa);
}
// one foot: the n contacts of t[n][2] into out[n][2] (may alias); false if any contact fails (all n are still written)
__host__ __device__ inline bool cmpc_force_sample_time_foot(const double* t, int n, long long dt_ns, double* out)
{
    bool good = true;
    for (int m = 0; m < n; ++m) good = cmpc_snap_contact(t + 2 * m, dt_ns, out + 2 * m) && good;
    return good;
}

// ContactList::getActiveContact(t): activation <= t < deactivation (CentroidalMPCBlock.cpp:61, :69), or -1
__host__ __device__ inline int cmpc_active_contact(const double* t, int n, double now)
{
    for (int m = 0; m < n; ++m)
        if (t[2 * m] <= now + CMPC_TIME_EPS && now + CMPC_TIME_EPS < t[2 * m + 1]) return m;
    return -1;
}
// ContactList::getNextContact(t): the contact with the lowest activation time after t (:44), or -1
__host__ __device__ inline int cmpc_next_contact(const double* t, int n, double now)
{
    for (int m = 0; m < n; ++m)
        if (t[2 * m] > now + CMPC_TIME_EPS) return m;
    return -1;
}

// updateContactPhaseList for one foot (CentroidalMPCBlock.cpp:41-103).  Returns false when the MPC list has an
// active contact but the planner's has none (:69-77).  out must hold M contacts.
__host__ __device__ inline bool cmpc_merge_foot(double now, const double* plan_t, const float* plan_pose, int plan_n,
                                                const double* mpc_t, const float* mpc_pose, int mpc_n, int M,
                                                double* out_t, float* out_pose, int* out_n)
{
    int n = 0;
    // the current contact keeps the pose the MPC gave it and takes the planner's timing (:79-82); it starts before
    // every future contact, so it goes first (ContactList orders by time)
    const int ma = cmpc_active_contact(mpc_t, mpc_n, now);          // :61
    if (ma >= 0) {
        const int pa = cmpc_active_contact(plan_t, plan_n, now);    // :69
        if (pa < 0) { *out_n = 0; return false; }                   // :70-77
        out_t[0] = plan_t[2 * pa]; out_t[1] = plan_t[2 * pa + 1];
        for (int i = 0; i < 7; ++i) out_pose[i] = mpc_pose[7 * ma + i];
        n = 1;
    }
    // every future contact of the planner (:44-58)
    const int first = cmpc_next_contact(plan_t, plan_n, now);
    if (first >= 0)
        for (int m = first; m < plan_n && n < M; ++m, ++n) {
            out_t[2 * n] = plan_t[2 * m]; out_t[2 * n + 1] = plan_t[2 * m + 1];
            for (int i = 0; i < 7; ++i) out_pose[7 * n + i] = plan_pose[7 * m + i];
        }
    *out_n = n;
    return true;
}

// owner of the stage that starts at time t: the active contact, else the next one to activate, else the last
__host__ __device__ inline int cmpc_stage_owner(const double* t, int n, double now, bool* active)
{
    int m = cmpc_active_contact(t, n, now);
    *active = m >= 0;
    if (m >= 0) return m;
    m = cmpc_next_contact(t, n, now);
    return m >= 0 ? m : n - 1;
}

__host__ __device__ inline void cmpc_quat_to_R(const float* q /* w x y z */, float* R /* row-major 3x3 */)
{
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - w * z);       R[2] = 2.f * (x * z + w * y);
    R[3] = 2.f * (x * y + w * z);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - w * x);
    R[6] = 2.f * (x * z - w * y);       R[7] = 2.f * (y * z + w * x);       R[8] = 1.f - 2.f * (x * x + y * y);
}

// setContactPhaseList for one foot `c` of one problem: fills the foot's blocks of the parameter vector p
// (reference layout) and returns the landing knot (first knot in contact after a swing stage, N if the foot is still
// in the air at the end of the horizon, -1 if it never leaves the ground).  Rule (contacts.py): stage k starts at
// now + k dt; Gamma_k = 1 iff a contact is active then; R_k, the limits of row k and nominal_{k+1} come from the
// stage's owner; nominal_0 and currentPos from the owner of stage 0.
// stage k of foot c (the body of cmpc_sample_foot's loop): writes the stage's entries of p, returns whether the foot is in contact at the stage's start
__host__ __device__ inline bool cmpc_sample_stage(int N, double dt, double now, int c, int k, const double* t, const float* pose, int n,
                                                  const float* box_upper, const float* box_lower, float* p)
{
    const CmpcIdx L{N};
    bool act;
    const int o = cmpc_stage_owner(t, n, now + k * dt, &act);
    float R[9];
    cmpc_quat_to_R(pose + 7 * o + 3, R);
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) p[L.pR(c) + 9 * k + 3 * cc + r] = R[3 * r + cc];   // vec(R) column-major
    p[L.pGam(c) + k] = act ? 1.f : 0.f;
    for (int i = 0; i < 3; ++i) {
        p[L.pUp(c) + 3 * k + i] = box_upper[3 * c + i];
        p[L.pLo(c) + 3 * k + i] = box_lower[3 * c + i];
        p[L.pNom(c) + 3 * (k + 1) + i] = pose[7 * o + i];
        if (k == 0) { p[L.pNom(c) + i] = pose[7 * o + i]; p[L.pCur(c) + i] = pose[7 * o + i]; }
    }
    return act;
}
// the landing knot from the stages' contact flags (first knot in contact after a swing stage, N if still in the air at the end, -1 if the foot never lifts);
// act(k) is called once per stage, in order
template <class ActOf>
__host__ __device__ inline int cmpc_landing_knot(int N, ActOf act)
{
    int land = -1;
    bool prev_act = true;
    for (int k = 0; k < N; ++k) {
        const bool a = act(k);
        if (a && !prev_act && land < 0) land = k;
        prev_act = a;
    }
    if (!prev_act && land < 0) land = N;
    return land;
}
__host__ __device__ inline int cmpc_sample_foot(int N, double dt, double now, int c, const double* t, const float* pose, int n,
                                                const float* box_upper, const float* box_lower, float* p)
{
    return cmpc_landing_knot(N, [&](int k) { return cmpc_sample_stage(N, dt, now, c, k, t, pose, n, box_upper, box_lower, p); });
}


// 8f-3, CentroidalMPCBlock.cpp:525-577: knot k of the references from the planner's trajectories (n_in knots every in_dt seconds, the first one t_offset seconds
// before "now"; h_in not yet divided by the mass) by linear interpolation, clamped to the trajectory's ends; the CoM height is replaced by com_height unless it is
// NaN (the reference forces 0.7, :534).  ci / hi: the problem's [n_in][3]; com_out / h_out: the knot's three entries of comRef / hRef.
__host__ __device__ inline void cmpc_resample_reference_knot(const float* ci, const float* hi, int n_in, double in_dt, double t_offset, double dt, int k,
                                                             double robot_mass, double com_height, float* com_out, float* h_out)
{
    double s = (t_offset + k * dt) / in_dt;
    if (s < 0) s = 0;
    if (s > n_in - 1) s = n_in - 1;
    int i0 = (int)s;
    if (i0 > n_in - 2) i0 = n_in - 2;
    const double w = s - i0;
    for (int a = 0; a < 3; ++a) {
        double cv = (1 - w) * ci[3 * i0 + a] + w * ci[3 * (i0 + 1) + a];
        if (a == 2 && com_height == com_height) cv = com_height;
        com_out[a] = (float)cv;
        h_out[a] = (float)(((1 - w) * hi[3 * i0 + a] + w * hi[3 * (i0 + 1) + a]) / robot_mass);
    }
}

// ---- the reference rows differentiated in the planner's trajectories (include/cmpc.h, cmpc_reference_from_planner_vjp / _jvp; DESIGN.md 7f, "References").
// The map above is linear in (ci, hi); what follows is its weights, its transpose and its image of a direction, one statement each for the host forms and
// the kernels (contraction into fma is off: the host forms are bit-equal to the kernels).  Tick number `tick` runs at now = tick * dt and reads the
// trajectories at t_offset = now - t_first, as cmpc_rollout_walk_device does.
struct CmpcRefArgs {
    int N, B, knots, tick0, rows, K;     // K: direction columns (the JVP)
    double dt, in_dt, t_first, robot_mass, com_height;
};
// (i0, w) of MPC knot k of tick `tick`: cmpc_resample_reference_knot's arithmetic, clamps included
__host__ __device__ inline void cmpc_reference_weight(int n_in, double in_dt, double t_first, double dt, int tick, int k, int* i0_out, double* w_out)
{
#pragma clang fp contract(off)
    const double now = (double)tick * dt;
    const double t_offset = now - t_first;
    double s = (t_offset + k * dt) / in_dt;
    if (s < 0) s = 0;
    if (s > n_in - 1) s = n_in - 1;
    int i0 = (int)s;
    if (i0 > n_in - 2) i0 = n_in - 2;
    *i0_out = i0;
    *w_out = s - i0;
}
// the transpose, one component: what MPC knot (i0, w) sends to planner knot i0 (index 0) and to i0 + 1 (index 1) from the gradients gc / gh of one
// component of its comRef / hRef entry -- (1 - w) g and w g, for h divided by the mass.  with_com false (the z row under a fixed height): gc is not used.
// The owner of a planner knot adds these in ascending (row, knot) order.
__host__ __device__ inline void cmpc_reference_vjp_terms(double w, bool with_com, float gc, float gh, double robot_mass, double* tc, double* th)
{
#pragma clang fp contract(off)
    const double c0 = 1 - w;
    if (with_com) { tc[0] = c0 * (double)gc; tc[1] = w * (double)gc; }
    th[0] = (c0 * (double)gh) / robot_mass;
    th[1] = (w * (double)gh) / robot_mass;
}
// the image of a direction: entry e6 of the 6 (N + 1) reference rows (comRef [N + 1][3] | hRef [N + 1][3]) of tick `tick` from one column's dc / dh
// [knots][3] (either may be null: zero)
__host__ __device__ inline float cmpc_reference_jvp_entry(const CmpcRefArgs& r, int tick, int e6, const double* dc, const double* dh)
{
#pragma clang fp contract(off)
    const int n3 = 3 * (r.N + 1);
    const bool is_h = e6 >= n3;
    const int q = is_h ? e6 - n3 : e6, k = q / 3, a = q - 3 * k;
    const double* src = is_h ? dh : dc;
    if (!src || (!is_h && a == 2 && r.com_height == r.com_height)) return 0.f;
    int i0; double w;
    cmpc_reference_weight(r.knots, r.in_dt, r.t_first, r.dt, tick, k, &i0, &w);
    double v = (1 - w) * src[3 * i0 + a] + w * src[3 * (i0 + 1) + a];
    if (is_h) v = v / r.robot_mass;
    return (float)v;
}
// rows of problem b that the ending rule admits: tick0 + r < e (e < 0: never ended)
__host__ __device__ inline int cmpc_reference_rows_of(const int* end_tick, int b, int tick0, int rows)
{
    const int e = end_tick ? end_tick[b] : -1;
    if (e < 0) return rows;
    const long long lim = (long long)e - tick0;
    return lim <= 0 ? 0 : lim < rows ? (int)lim : rows;
}

// ---- the walk's record (include/cmpc.h, cmpc_rollout_record): what one tick left of one problem -> its trace row, its outcome and its share of the batch
// statistics.  One statement for the host form and the kernel, so that the two are bit-equal (contraction into fma is off: the offsets are sums of
// double products).  Plain pointers, host or device alike.
struct CmpcRecordArgs {
    int N, B, tick, row, stop_mask;
    const float* X; const float* P; const float* info; const int* ok; const int* land; const float* state_out; const float* zmp;
    const float* box;                                                                   // upper[2][3] | lower[2][3]
    float* t_com; float* t_zmp; int* t_land; double* t_off; int* t_iters; int* t_code;  // trace (each may be null)
    int* end_tick; int* end_code; int* it_sum; int* it_max; float* final_state; float* slack_min;
    const int* start;   // [B] or null (the refill walk): the tick number end_tick takes is tick - start[b], the problem's local one
};
// the physical limits of a walk (include/cmpc.h, cmpc_walk_limits) as the record takes them: the five limits (NaN: off), the model corners the plant
// kernel reads ([2][4][3] of problem 0, problem b's corners_stride floats further on), the gravity, this tick's row [B][4] of the measures trace (or
// null) and the extremes [B][5] (or null)
struct CmpcLimitArgs {
    double height_min, height_max, reach_max, margin_min, track_max, gravity;
    const float* corners; int corners_stride;
    float* measures; float* extremes;
};
// the signed distance of xi to the convex hull of the 8 points (vx, vy), positive inside, with no hull built: the least of max_k n.v_k - n.xi over the unit
// normals of every pair of points, both orientations, and the unit directions from every point to xi; pairs and directions shorter than 1e-12 are left
// out, and with none left the margin is 0.  The two orientations of a pair share their cross products: (max_k d_k - d_xi) / |e| and (d_xi - min_k d_k) / |e|,
// d = e_y x - e_x y.  Repeated points change nothing (the caller fills the rows of a foot that is not in the support set with the other foot's).  Constant
// trip counts: the loops unroll, and the arrays stay in registers.
__host__ __device__ inline double cmpc_support_margin(const double (&vx)[8], const double (&vy)[8], double xi_x, double xi_y)
{
#pragma clang fp contract(off)
    double m = 0.0;
    bool any = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = i + 1; j < 8; ++j) {
            const double ex = vx[j] - vx[i], ey = vy[j] - vy[i];
            const double len = __builtin_sqrt(ex * ex + ey * ey);
            const double dxi = ey * xi_x - ex * xi_y;
            double hi = ey * vx[0] - ex * vy[0], lo = hi;
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                const double d = ey * vx[k] - ex * vy[k];
                hi = d > hi ? d : hi;
                lo = d < lo ? d : lo;
            }
            const double c0 = (hi - dxi) / len, c1 = (dxi - lo) / len;
            const double c = c1 < c0 ? c1 : c0;
            if (len >= 1e-12 && (!any || c < m)) { m = c; any = true; }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double ex = xi_x - vx[i], ey = xi_y - vy[i];
        const double len = __builtin_sqrt(ex * ex + ey * ey);
        double hi = ex * (vx[0] - xi_x) + ey * (vy[0] - xi_y);
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const double d = ex * (vx[k] - xi_x) + ey * (vy[k] - xi_y);
            hi = d > hi ? d : hi;
        }
        const double c = hi / len;
        if (len >= 1e-12 && (!any || c < m)) { m = c; any = true; }
    }
    return m;
}
// the four measures of problem b at the time of state_out, stage 1 of the tick's problem (include/cmpc.h, "physical limits"): height, reach, margin,
// track, each formed in double from the float inputs, sums left to right, and rounded to float once.  A state that is not finite: NaN in all four.
__host__ __device__ inline void cmpc_walk_measures(const CmpcRecordArgs& a, const CmpcLimitArgs& lm, int b, bool finite, float* out)
{
#pragma clang fp contract(off)
    const CmpcIdx L{a.N};
    const float qnan = __builtin_nanf("");
    out[0] = out[1] = out[2] = out[3] = qnan;
    if (!finite) return;
    const float* so = a.state_out + 9 * (size_t)b;
    const float* x = a.X + (size_t)b * L.nx();
    const float* p = a.P + (size_t)b * L.np();
    const double com[3] = {(double)so[0], (double)so[1], (double)so[2]};
    const double tx = com[0] - (double)p[L.pComref() + 3], ty = com[1] - (double)p[L.pComref() + 4];
    out[3] = (float)__builtin_sqrt(tx * tx + ty * ty);
    const bool on0 = p[L.pGam(0) + 1] > 0.5f, on1 = p[L.pGam(1) + 1] > 0.5f;
    if (!on0 && !on1) return;
    double q[2][3], vx[8], vy[8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c) + 9;   // column-major block of stage 1
        const float* cn = lm.corners + (size_t)b * lm.corners_stride + 12 * c;
        for (int i = 0; i < 3; ++i) q[c][i] = (double)x[L.oPos(c) + 3 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            vx[4 * c + j] = ((q[c][0] + (double)R[0] * (double)cn[3 * j]) + (double)R[3] * (double)cn[3 * j + 1]) + (double)R[6] * (double)cn[3 * j + 2];
            vy[4 * c + j] = ((q[c][1] + (double)R[1] * (double)cn[3 * j]) + (double)R[4] * (double)cn[3 * j + 1]) + (double)R[7] * (double)cn[3 * j + 2];
        }
    }
    double zsum = 0.0, reach = 0.0;
    int n = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const bool on = c == 0 ? on0 : on1;
        const double dx = com[0] - q[c][0], dy = com[1] - q[c][1], dz = com[2] - q[c][2];
        const double r = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
        if (on) {
            zsum = zsum + q[c][2];
            reach = (n == 0 || r > reach) ? r : reach;
            ++n;
        }
    }
    const double height = com[2] - zsum / (double)n;
    // (a foot outside the support set takes the other foot's points: the margin's candidates are then the supporting foot's alone)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!on0) { vx[j] = vx[4 + j]; vy[j] = vy[4 + j]; }
        if (!on1) { vx[4 + j] = vx[j]; vy[4 + j] = vy[j]; }
    }
    const double tau = __builtin_sqrt((height > 0.0 ? height : 0.0) / lm.gravity);
    const double xi_x = com[0] + (double)so[3] * tau, xi_y = com[1] + (double)so[4] * tau;
    out[0] = (float)height;
    out[1] = (float)reach;
    out[2] = (float)cmpc_support_margin(vx, vy, xi_x, xi_y);
}
// the limit code of a tick whose code is 0 so far: 6..9, first match, or 0.  Written so that a NaN measure or a NaN limit never fires.
__host__ __device__ inline int cmpc_limit_code(const CmpcLimitArgs& lm, const float* m)
{
    if ((double)m[0] < lm.height_min || (double)m[0] > lm.height_max) return 6;
    if ((double)m[1] > lm.reach_max) return 7;
    if ((double)m[2] < lm.margin_min) return 8;
    if ((double)m[3] > lm.track_max) return 9;
    return 0;
}

// tally[5] (LIM: [6]): this problem's terms of the statistics row -- not ended before the tick, ended by it, iterations (for the sum and for the max: 0
// unless the tick is a good one), code 2..4 (LIM: and code 6..9)
// LIM (cmpc_set_walk_limits): the four measures of the tick, the codes 6..9 behind the chain, the measures row and the extremes.  LIM = false is the
// function without any of it, and lm is not read.
template <bool LIM>
__host__ __device__ inline void cmpc_record_problem(const CmpcRecordArgs& a, const CmpcLimitArgs& lm, int b, int* tally)
{
#pragma clang fp contract(off)
    const CmpcIdx L{a.N};
    const int N = a.N;
    const float* so = a.state_out + 9 * (size_t)b;
    const float* inf = a.info + (size_t)b * CMPC_INFO_N;
    const bool before = a.end_tick[b] >= 0;
    int code = -1;
    bool ends = false;
    float ms[4];
    if (!before) {
        bool finite = true;
        for (int i = 0; i < 9; ++i) finite = finite && __builtin_isfinite(so[i]);
        code = (a.ok && !a.ok[b]) ? 1 : inf[5] != 0.f ? 1 + (int)inf[5] : !finite ? 5 : 0;
        if (LIM) {
            cmpc_walk_measures(a, lm, b, finite, ms);
            if (code == 0) code = cmpc_limit_code(lm, ms);
        }
        ends = code == 1 || (code >= 2 && code <= 4 && (a.stop_mask & 2)) || (code == 5 && (a.stop_mask & 4)) || (LIM && code >= 6 && (a.stop_mask & 8));
    }
    const bool good = !before && !ends;
    if (LIM) {
        // the measures row: every tick of a problem that had not ended before it, the tick a limit ends included; NaN behind an end and on a tick that
        // codes 1..5 end.  The extremes: good ticks only (a NaN measure leaves them alone)
        const bool shown = good || (ends && code >= 6);
        if (lm.measures)
            for (int i = 0; i < 4; ++i) lm.measures[4 * (size_t)b + i] = shown ? ms[i] : __builtin_nanf("");
        if (lm.extremes && good) {
            float* e = lm.extremes + 5 * (size_t)b;
            if (ms[0] < e[0]) e[0] = ms[0];
            if (ms[0] > e[1]) e[1] = ms[0];
            if (ms[1] > e[2]) e[2] = ms[1];
            if (ms[2] < e[3]) e[3] = ms[2];
            if (ms[3] > e[4]) e[4] = ms[3];
        }
        tally[5] = (!before && code >= 6) ? 1 : 0;
    }
    const int it = good ? (int)inf[0] : 0;
    const size_t r = (size_t)a.row * a.B + b;
    const float qnan = __builtin_nanf("");
    if (a.t_code) a.t_code[r] = code;
    if (a.t_iters) a.t_iters[r] = it;
    if (a.t_com)
        for (int i = 0; i < 3; ++i) a.t_com[3 * r + i] = good ? so[i] : qnan;
    if (a.t_zmp)
        for (int i = 0; i < 2; ++i) a.t_zmp[2 * r + i] = good ? a.zmp[2 * (size_t)b + i] : qnan;
    float slack = a.slack_min[b];
    for (int c = 0; c < 2; ++c) {
        const int k = good ? a.land[2 * b + c] : -2;
        if (a.t_land) a.t_land[2 * r + c] = k;
        double off[3] = {0.0, 0.0, 0.0};
        if (!good) off[0] = off[1] = off[2] = (double)qnan;
        else if (k > 0 && k <= N) {
            const float* x = a.X + (size_t)b * L.nx() + L.oPos(c) + 3 * k;
            const float* p = a.P + (size_t)b * L.np();
            const float* R = p + L.pR(c) + 9 * (k - 1);   // column-major: R^T's row i is R[3 i .. 3 i + 2]
            double d[3];
            for (int i = 0; i < 3; ++i) d[i] = (double)x[i] - (double)p[L.pNom(c) + 3 * k + i];
            for (int i = 0; i < 3; ++i) {
                off[i] = ((double)R[3 * i] * d[0] + (double)R[3 * i + 1] * d[1]) + (double)R[3 * i + 2] * d[2];
                const double up = (double)a.box[3 * c + i] - off[i], lo = off[i] - (double)a.box[6 + 3 * c + i];
                const float s = (float)(up < lo ? up : lo);
                if (s < slack) slack = s;
            }
        }
        if (a.t_off)
            for (int i = 0; i < 3; ++i) a.t_off[(2 * r + c) * 3 + i] = off[i];
    }
    if (ends) { a.end_tick[b] = a.start ? a.tick - a.start[b] : a.tick; a.end_code[b] = code; }
    if (good) {
        a.it_sum[b] += it;
        if (it > a.it_max[b]) a.it_max[b] = it;
        for (int i = 0; i < 9; ++i) a.final_state[9 * (size_t)b + i] = so[i];
        a.slack_min[b] = slack;
    }
    tally[0] = before ? 0 : 1;
    tally[1] = ends ? 1 : 0;
    tally[2] = it;
    tally[3] = it;
    tally[4] = (!before && code >= 2 && code <= 4) ? 1 : 0;
}

// ---- the measures differentiated (include/cmpc.h, "the measures, differentiated"; DESIGN.md 7f, "Measures, differentiated") ----
// The derivative of cmpc_walk_measures in its 44 inputs per (row, problem) -- com[3], dcom[3], q[2][3], omega[2][3] (the body-frame tangent of the stage-1
// rotation, R <- R Exp(omega)), corner[2][4][3], comRef_xy[2] -- ignoring the final rounding to float.  Stated once, as the partials of one problem
// (cmpc_walk_measures_partials); the VJP, the JVP and the host's dense Jacobian are contractions of them.  One statement for the host forms and the
// kernels: double from the float inputs, contraction off, so that the two are bit-equal.  Every branch is a SELECT, never a multiply by zero: what a
// branch does not take is not read into the result, so NaN there cannot leak.  At a tie between branches (two faces of the support region at one
// distance, two feet at one distance, two vertices at one projection) the first in the forward's order is taken: ONE element of the generalised gradient.
struct CmpcMeasureArgs {
    int N, B;
    const float* X; const float* P; const float* state_out;    // one tape row: [B][n_x], [B][n_p], and dStates[row + 1] [B][9]
    const float* corners; int corners_stride; double gravity;  // as CmpcLimitArgs
};
// the gradient of cmpc_support_margin in xi and in at most three of the 8 points (idx < 0: no term)
struct CmpcMarginGrad {
    double gxi[2];
    int idx[3]; double gx[3], gy[3];
};
// a candidate of the margin's chain as the gradient needs it: kind 1 a pair (i, j) with sign s and extremal vertex k, kind 2 the direction from point i
struct CmpcMarginPick {
    bool any; double m;
    int kind, i, j, k;
    double ex, ey, len, a, b, s;
};
// the chain's step: candidate c replaces the pick if it is admitted and the first, or strictly less
__host__ __device__ inline void cmpc_margin_offer(CmpcMarginPick& p, bool admitted, double c, int kind, int i, int j, int k, double ex, double ey, double len,
                                                  double a, double b, double s)
{
    if (admitted && (!p.any || c < p.m)) {
        p.any = true; p.m = c; p.kind = kind; p.i = i; p.j = j; p.k = k;
        p.ex = ex; p.ey = ey; p.len = len; p.a = a; p.b = b; p.s = s;
    }
}
// cmpc_support_margin's comparison chain, expression for expression -- the same candidate order, the same strict <, the same len >= 1e-12 exclusions, the
// arg-max / arg-min vertex the first in index order -- remembering a candidate, then the gradient of that smooth branch:
//   a pair (i, j), e = v_j - v_i, s = +1 with the arg-max vertex k (c0) or -1 with the arg-min (c1): c = (e_y a - e_x b) / |e|, (a, b) = s (v_k - xi);
//       dc/dv_k = s n, dc/dxi = -s n, n = (e_y, -e_x) / |e|;  dc/de = ((-b, a) - c e / |e|) / |e| goes to v_j and, negated, to v_i
//   a direction from point i, e = xi - v_i, k the arg-max: c = e.r / |e|, r = v_k - xi, u = e / |e|;
//       dc/dv_k = u, dc/de = w = (r - c u) / |e| goes to xi and, negated, to v_i, dc/dxi = w - u
//   no candidate: zero.
// WHICH candidate.  The chain's winner gives the VALUE, but need not be the branch that is active: the parallel sides of a rectangular sole alias each
// other -- the pair (0, 3) taken backwards has the normal and, to rounding, the value of the pair (1, 2), with its extremal vertex k on the far side --
// and which of the two the strict < keeps is decided by the last bit.  Such an alias equals the margin only while the sole stays a rectangle: in the
// corners and in omega its gradient is NOT an element of the generalised gradient (nearby generic points are all governed by the true side).  So the
// same chain is run over the FACES alone -- a pair whose extremal vertex lies on the pair's own line, a direction whose extremal vertex is its own point
// (both within 1e-9 m: a million times the rounding, a thousandth of what a sole's geometry resolves) -- and its winner is differentiated.  The least
// over all directions is always attained at a face (an edge's normal or a vertex's direction), so this winner has the chain's value to rounding; where
// no face is admitted the chain's own winner is used.  Between two faces at one distance (a true kink) the first in the chain's order wins.
__host__ __device__ inline void cmpc_support_margin_grad(const double (&vx)[8], const double (&vy)[8], double xi_x, double xi_y, CmpcMarginGrad& g)
{
#pragma clang fp contract(off)
    const double on_line = 1e-9;
    CmpcMarginPick win{false, 0.0, 0, -1, -1, -1, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0}, face = win;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = i + 1; j < 8; ++j) {
            const double ex = vx[j] - vx[i], ey = vy[j] - vy[i];
            const double len = __builtin_sqrt(ex * ex + ey * ey);
            const double dxi = ey * xi_x - ex * xi_y;
            double hi = ey * vx[0] - ex * vy[0], lo = hi;
            int khi = 0, klo = 0;
            double hx = vx[0], hy = vy[0], lx = vx[0], ly = vy[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                const double d = ey * vx[k] - ex * vy[k];
                const bool up = d > hi, dn = d < lo;
                hi = up ? d : hi; khi = up ? k : khi; hx = up ? vx[k] : hx; hy = up ? vy[k] : hy;
                lo = dn ? d : lo; klo = dn ? k : klo; lx = dn ? vx[k] : lx; ly = dn ? vy[k] : ly;
            }
            const double c0 = (hi - dxi) / len, c1 = (dxi - lo) / len;
            const bool second = c1 < c0, admitted = len >= 1e-12;
            const double a0 = hx - xi_x, b0 = hy - xi_y, a1 = -(lx - xi_x), b1 = -(ly - xi_y);
            cmpc_margin_offer(win, admitted, second ? c1 : c0, 1, i, j, second ? klo : khi, ex, ey, len, second ? a1 : a0, second ? b1 : b0,
                              second ? -1.0 : 1.0);
            // the pair's own line: d_i and d_j (one number but for rounding) against the extremes
            const double di = ey * vx[i] - ex * vy[i], dj = ey * vx[j] - ex * vy[j];
            const double top = di > dj ? di : dj, bot = di < dj ? di : dj;
            cmpc_margin_offer(face, admitted && hi - top <= on_line * len, c0, 1, i, j, khi, ex, ey, len, a0, b0, 1.0);
            cmpc_margin_offer(face, admitted && bot - lo <= on_line * len, c1, 1, i, j, klo, ex, ey, len, a1, b1, -1.0);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double ex = xi_x - vx[i], ey = xi_y - vy[i];
        const double len = __builtin_sqrt(ex * ex + ey * ey);
        double hi = ex * (vx[0] - xi_x) + ey * (vy[0] - xi_y);
        int khi = 0;
        double hx = vx[0], hy = vy[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const double d = ex * (vx[k] - xi_x) + ey * (vy[k] - xi_y);
            const bool up = d > hi;
            hi = up ? d : hi; khi = up ? k : khi; hx = up ? vx[k] : hx; hy = up ? vy[k] : hy;
        }
        const double c = hi / len;
        const bool admitted = len >= 1e-12;
        cmpc_margin_offer(win, admitted, c, 2, i, -1, khi, ex, ey, len, hx - xi_x, hy - xi_y, 1.0);
        // its own point: e.(v_i - xi) = -|e|^2 is the greatest projection
        cmpc_margin_offer(face, admitted && hi + len * len <= on_line * len, c, 2, i, -1, khi, ex, ey, len, hx - xi_x, hy - xi_y, 1.0);
    }
    const CmpcMarginPick p = face.any ? face : win;
    const int kind = p.kind, bi = p.i, bj = p.j, bk = p.k;
    const double bex = p.ex, bey = p.ey, blen = p.len, ba = p.a, bb = p.b, bc = p.m, bs = p.s;
    g.gxi[0] = g.gxi[1] = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) { g.idx[t] = -1; g.gx[t] = g.gy[t] = 0.0; }
    if (kind == 1) {
        const double nx = bey / blen, ny = -bex / blen;
        const double dex = (-bb - (bc * bex) / blen) / blen, dey = (ba - (bc * bey) / blen) / blen;
        g.idx[0] = bk; g.gx[0] = bs * nx; g.gy[0] = bs * ny;
        g.idx[1] = bj; g.gx[1] = dex; g.gy[1] = dey;
        g.idx[2] = bi; g.gx[2] = -dex; g.gy[2] = -dey;
        g.gxi[0] = -(bs * nx); g.gxi[1] = -(bs * ny);
    } else if (kind == 2) {
        const double ux = bex / blen, uy = bey / blen;
        const double wx = (ba - bc * ux) / blen, wy = (bb - bc * uy) / blen;
        g.idx[0] = bk; g.gx[0] = ux; g.gy[0] = uy;
        g.idx[1] = bi; g.gx[1] = -wx; g.gy[1] = -wy;
        g.gxi[0] = wx - ux; g.gxi[1] = wy - uy;
    }
}
// the partials of one problem's four measures, by what they act on:
//   height  d/dcom_z = 1, d/dq_c,z = -inv_n for c in S
//   reach   u = (com - q_f) / r of the foot f the forward's `r > reach` chain keeps (the first foot wins a tie), zero when r == 0: d/dcom = u, d/dq_f = -u
//   track   t = (com_xy - ref_xy) / track, zero when track == 0: d/dcom_xy = t, d/dref_xy = -t
//   margin  gxi = d/dxi and (gvx, gvy)[4 c + j] = d/d(xy of vertex j of foot c), hit[] where there is one.  A vertex the forward filled from the other
//           foot (single support) is entered at the foot and corner it was copied from, so a foot outside S has no hit.  xi = com_xy + dcom_xy tau,
//           tau = sqrt(max(height, 0) / g); tau_on (height > 0 and tau > 0): dtau = dtau/dheight = 1 / (2 g tau), else the margin does not see the height
// alive: the state is finite (measure 3 is a number); alive && support: measures 0..2 are.  A measure the forward reports as NaN has no partials.
struct CmpcMeasurePartials {
    bool alive, support, on[2], tau_on;
    double inv_n;
    int reach_foot; double u[3];
    double t[2];
    double gxi[2], tau, dtau, dcx, dcy;
    bool hit[8]; double gvx[8], gvy[8];
};
__host__ __device__ inline void cmpc_walk_measures_partials(const CmpcMeasureArgs& a, int b, CmpcMeasurePartials& pt)
{
#pragma clang fp contract(off)
    const CmpcIdx L{a.N};
    const float* so = a.state_out + 9 * (size_t)b;
    const float* x = a.X + (size_t)b * L.nx();
    const float* p = a.P + (size_t)b * L.np();
    bool finite = true;
    for (int i = 0; i < 9; ++i) finite = finite && __builtin_isfinite(so[i]);
    pt.alive = finite; pt.support = false; pt.on[0] = pt.on[1] = false; pt.tau_on = false;
    pt.inv_n = 0.0; pt.reach_foot = 0; pt.u[0] = pt.u[1] = pt.u[2] = 0.0; pt.t[0] = pt.t[1] = 0.0;
    pt.gxi[0] = pt.gxi[1] = 0.0; pt.tau = pt.dtau = pt.dcx = pt.dcy = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) { pt.hit[s] = false; pt.gvx[s] = pt.gvy[s] = 0.0; }
    if (!finite) return;
    const double com[3] = {(double)so[0], (double)so[1], (double)so[2]};
    const double tx = com[0] - (double)p[L.pComref() + 3], ty = com[1] - (double)p[L.pComref() + 4];
    const double track = __builtin_sqrt(tx * tx + ty * ty);
    const bool moved = track != 0.0;
    pt.t[0] = moved ? tx / track : 0.0;
    pt.t[1] = moved ? ty / track : 0.0;
    const bool on0 = p[L.pGam(0) + 1] > 0.5f, on1 = p[L.pGam(1) + 1] > 0.5f;
    if (!on0 && !on1) return;
    pt.support = true; pt.on[0] = on0; pt.on[1] = on1;
    double q[2][3], vx[8], vy[8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c) + 9;   // column-major block of stage 1
        const float* cn = a.corners + (size_t)b * a.corners_stride + 12 * c;
        for (int i = 0; i < 3; ++i) q[c][i] = (double)x[L.oPos(c) + 3 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            vx[4 * c + j] = ((q[c][0] + (double)R[0] * (double)cn[3 * j]) + (double)R[3] * (double)cn[3 * j + 1]) + (double)R[6] * (double)cn[3 * j + 2];
            vy[4 * c + j] = ((q[c][1] + (double)R[1] * (double)cn[3 * j]) + (double)R[4] * (double)cn[3 * j + 1]) + (double)R[7] * (double)cn[3 * j + 2];
        }
    }
    double zsum = 0.0, reach = 0.0;
    int n = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const bool on = c == 0 ? on0 : on1;
        const double dx = com[0] - q[c][0], dy = com[1] - q[c][1], dz = com[2] - q[c][2];
        const double r = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
        if (on) {
            zsum = zsum + q[c][2];
            if (n == 0 || r > reach) {
                reach = r;
                pt.reach_foot = c;
                const bool apart = r != 0.0;
                pt.u[0] = apart ? dx / r : 0.0; pt.u[1] = apart ? dy / r : 0.0; pt.u[2] = apart ? dz / r : 0.0;
            }
            ++n;
        }
    }
    pt.inv_n = 1.0 / (double)n;
    const double height = com[2] - zsum / (double)n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!on0) { vx[j] = vx[4 + j]; vy[j] = vy[4 + j]; }
        if (!on1) { vx[4 + j] = vx[j]; vy[4 + j] = vy[j]; }
    }
    const double tau = __builtin_sqrt((height > 0.0 ? height : 0.0) / a.gravity);
    const double xi_x = com[0] + (double)so[3] * tau, xi_y = com[1] + (double)so[4] * tau;
    pt.tau = tau; pt.dcx = (double)so[3]; pt.dcy = (double)so[4];
    pt.tau_on = height > 0.0 && tau > 0.0;
    pt.dtau = pt.tau_on ? 1.0 / ((2.0 * a.gravity) * tau) : 0.0;
    CmpcMarginGrad mg;
    cmpc_support_margin_grad(vx, vy, xi_x, xi_y, mg);
    pt.gxi[0] = mg.gxi[0]; pt.gxi[1] = mg.gxi[1];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int raw = mg.idx[t] >> 2;                                                  // (idx < 0: slot < 0, no hit)
        const int foot = mg.idx[t] < 0 ? -1 : ((raw == 0 ? on0 : on1) ? raw : 1 - raw);   // the vertex fill: the foot it was copied from
        const int slot = mg.idx[t] < 0 ? -1 : 4 * foot + (mg.idx[t] & 3);
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if (slot == s) { pt.gvx[s] = pt.gvx[s] + mg.gx[t]; pt.gvy[s] = pt.gvy[s] + mg.gy[t]; pt.hit[s] = true; }
    }
}
// what one vertex's xy sends on, (ax, ay) = its gradient: foot position xy, corner (rows 0 and 1 of R), omega (v = q + R Exp(omega) cn: dv_x / domega =
// cn x R_0, dv_y / domega = cn x R_1, R_0 / R_1 the first two ROWS of R)
__host__ __device__ inline void cmpc_measures_vertex_rows(const float* R, const float* cn, double* r0, double* r1, double* x0, double* x1)
{
#pragma clang fp contract(off)
    const double c0 = (double)cn[0], c1 = (double)cn[1], c2 = (double)cn[2];
    r0[0] = (double)R[0]; r0[1] = (double)R[3]; r0[2] = (double)R[6];
    r1[0] = (double)R[1]; r1[1] = (double)R[4]; r1[2] = (double)R[7];
    x0[0] = c1 * r0[2] - c2 * r0[1]; x0[1] = c2 * r0[0] - c0 * r0[2]; x0[2] = c0 * r0[1] - c1 * r0[0];
    x1[0] = c1 * r1[2] - c2 * r1[1]; x1[1] = c2 * r1[0] - c0 * r1[2]; x1[2] = c0 * r1[1] - c1 * r1[0];
}
// the VJP of one problem: w[4] the cotangent of (height, reach, margin, track) -> gs[5] (com xyz, dcom xy), gq[2][3] (the knot-1 foot positions),
// direct[32] (comRef_xy 2, omega [2][3], corner [2][4][3]), all written whole.  The cotangent of a NaN measure is not read.
__host__ __device__ inline void cmpc_walk_measures_vjp_problem(const CmpcMeasureArgs& a, int b, const double* w, double* gs, double* gq, double* direct)
{
#pragma clang fp contract(off)
    const CmpcIdx L{a.N};
    CmpcMeasurePartials pt;
    cmpc_walk_measures_partials(a, b, pt);
    for (int i = 0; i < 5; ++i) gs[i] = 0.0;
    for (int i = 0; i < 6; ++i) gq[i] = 0.0;
    for (int i = 0; i < 32; ++i) direct[i] = 0.0;
    if (!pt.alive) return;
    {
        const double w3 = w[3], g0 = w3 * pt.t[0], g1 = w3 * pt.t[1];
        gs[0] = gs[0] + g0; gs[1] = gs[1] + g1;
        direct[0] = -g0; direct[1] = -g1;
    }
    if (!pt.support) return;
    const double w0 = w[0], w1 = w[1], w2 = w[2];
    // height
    gs[2] = gs[2] + w0;
#pragma unroll
    for (int c = 0; c < 2; ++c)
        if (pt.on[c]) gq[3 * c + 2] = gq[3 * c + 2] - w0 * pt.inv_n;
    // reach
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double r = w1 * pt.u[i];
        gs[i] = gs[i] + r;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (pt.reach_foot == c) gq[3 * c + i] = gq[3 * c + i] - r;
    }
    // margin: xi, and through tau the height
    const double gxx = w2 * pt.gxi[0], gxy = w2 * pt.gxi[1];
    gs[0] = gs[0] + gxx; gs[1] = gs[1] + gxy;
    gs[3] = gs[3] + gxx * pt.tau; gs[4] = gs[4] + gxy * pt.tau;
    if (pt.tau_on) {
        const double gh = (gxx * pt.dcx + gxy * pt.dcy) * pt.dtau;
        gs[2] = gs[2] + gh;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (pt.on[c]) gq[3 * c + 2] = gq[3 * c + 2] - gh * pt.inv_n;
    }
    // margin: the vertices
    const float* p = a.P + (size_t)b * L.np();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c) + 9;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!pt.hit[4 * c + j]) continue;
            const float* cn = a.corners + (size_t)b * a.corners_stride + 12 * c + 3 * j;
            double r0[3], r1[3], x0[3], x1[3];
            cmpc_measures_vertex_rows(R, cn, r0, r1, x0, x1);
            const double ax = w2 * pt.gvx[4 * c + j], ay = w2 * pt.gvy[4 * c + j];
            gq[3 * c] = gq[3 * c] + ax; gq[3 * c + 1] = gq[3 * c + 1] + ay;
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                direct[2 + 3 * c + l] = direct[2 + 3 * c + l] + (ax * x0[l] + ay * x1[l]);
                direct[8 + 12 * c + 3 * j + l] = ax * r0[l] + ay * r1[l];
            }
        }
    }
}
// the JVP of one problem, the transpose: ds[5] (com xyz, dcom xy), dq[6], dref[2], dcn[24] (read with has_cn only), dom[6] (NULL: zero) -> dm[4], zero for a
// measure the forward reports as NaN
__host__ __device__ inline void cmpc_walk_measures_jvp_problem(const CmpcMeasureArgs& a, int b, const CmpcMeasurePartials& pt, const double* ds, const double* dq,
                                                               const double* dref, const double* dcn, bool has_cn, const double* dom, double* dm)
{
#pragma clang fp contract(off)
    const CmpcIdx L{a.N};
    dm[0] = dm[1] = dm[2] = dm[3] = 0.0;
    if (!pt.alive) return;
    dm[3] = pt.t[0] * (ds[0] - dref[0]) + pt.t[1] * (ds[1] - dref[1]);
    if (!pt.support) return;
    double dh = ds[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
        if (pt.on[c]) dh = dh - dq[3 * c + 2] * pt.inv_n;
    dm[0] = dh;
    double dr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double dqi = 0.0;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (pt.reach_foot == c) dqi = dq[3 * c + i];
        dr = dr + pt.u[i] * (ds[i] - dqi);
    }
    dm[1] = dr;
    double dxx = ds[0] + ds[3] * pt.tau, dxy = ds[1] + ds[4] * pt.tau;
    if (pt.tau_on) {
        const double dt = pt.dtau * dh;
        dxx = dxx + pt.dcx * dt; dxy = dxy + pt.dcy * dt;
    }
    double d2 = pt.gxi[0] * dxx + pt.gxi[1] * dxy;
    const float* p = a.P + (size_t)b * L.np();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c) + 9;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!pt.hit[4 * c + j]) continue;
            const float* cn = a.corners + (size_t)b * a.corners_stride + 12 * c + 3 * j;
            double r0[3], r1[3], x0[3], x1[3];
            cmpc_measures_vertex_rows(R, cn, r0, r1, x0, x1);
            double dvx = dq[3 * c], dvy = dq[3 * c + 1];
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                if (has_cn) { dvx = dvx + r0[l] * dcn[12 * c + 3 * j + l]; dvy = dvy + r1[l] * dcn[12 * c + 3 * j + l]; }
                if (dom) { dvx = dvx + x0[l] * dom[3 * c + l]; dvy = dvy + x1[l] * dom[3 * c + l]; }
            }
            d2 = d2 + (pt.gvx[4 * c + j] * dvx + pt.gvy[4 * c + j] * dvy);
        }
    }
    dm[2] = d2;
}
// one (row, problem) of the measures VJP (include/cmpc.h, cmpc_walk_measures_vjp): rows of the call start at the pointers; the row counts when
// tick0 + r < e (cmpc_reference_rows_of).  A row that does not count: zero in direct, nothing else read or written.  A term that is exactly zero is not
// added to a += entry (a select: the entry keeps its bits, a -0.0 included).
struct CmpcMeasureVjpArgs {
    int N, B, tick0, rows;
    const float* X; const float* P; const float* states;       // [rows][B][n_x], [rows][B][n_p], [rows + 1][B][9]
    const int* end_tick;
    const float* corners; int corners_stride; double gravity;
    const double* grad_measures;                                 // [rows][B][4]
    double* grad_states; float* grad_X; double* direct;         // [rows + 1][B][9] +=, [rows][B][n_x] +=, [rows][B][32]
};
__host__ __device__ inline void cmpc_walk_measures_vjp_entry(const CmpcMeasureVjpArgs& v, int r, int b)
{
#pragma clang fp contract(off)
    const CmpcIdx L{v.N};
    const size_t rb = (size_t)r * v.B + b;
    double* direct = v.direct + 32 * rb;
    if (r >= cmpc_reference_rows_of(v.end_tick, b, v.tick0, v.rows)) {
        for (int i = 0; i < 32; ++i) direct[i] = 0.0;
        return;
    }
    const CmpcMeasureArgs a{v.N, v.B, v.X + (size_t)r * v.B * L.nx(), v.P + (size_t)r * v.B * L.np(), v.states + (size_t)(r + 1) * v.B * 9, v.corners,
                            v.corners_stride, v.gravity};
    double gs[5], gq[6], d[32];
    cmpc_walk_measures_vjp_problem(a, b, v.grad_measures + 4 * rb, gs, gq, d);
    for (int i = 0; i < 32; ++i) direct[i] = d[i];
    double* s = v.grad_states + ((size_t)(r + 1) * v.B + b) * 9;
    for (int i = 0; i < 5; ++i)
        if (gs[i] != 0.0) s[i] = s[i] + gs[i];
    float* gx = v.grad_X + rb * L.nx();
#pragma unroll
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 3; ++i) {
            const float t = (float)gq[3 * c + i];
            if (t != 0.f) gx[L.oPos(c) + 3 + i] = gx[L.oPos(c) + 3 + i] + t;
        }
}
// the fold behind the reverse walk (cmpc_walk_measures_vjp_fold): entry e < rows B adds direct's comRef pair of its (row, problem) to the knot-1 comRef
// xy of grad_p (float, each term rounded once; a zero term is not added), entry e < 24 B sums its (problem, corner word) of direct over the rows in
// ascending order into grad_model[b][10 + word].  Either output may be null.
__host__ __device__ inline void cmpc_walk_measures_fold_entry(int N, int B, int rows, const double* direct, float* grad_p, double* grad_model, size_t e)
{
#pragma clang fp contract(off)
    const CmpcIdx L{N};
    if (grad_p && e < (size_t)rows * B) {
        float* g = grad_p + e * L.np() + L.pComref() + 3;
        for (int i = 0; i < 2; ++i) {
            const float t = (float)direct[32 * e + i];
            if (t != 0.f) g[i] = g[i] + t;
        }
    }
    if (grad_model && e < (size_t)24 * B) {
        const size_t b = e / 24, wd = e - 24 * b;
        double s = 0.0;
        for (int r = 0; r < rows; ++r) s = s + direct[32 * ((size_t)r * B + b) + 8 + wd];
        if (s != 0.0) grad_model[34 * b + 10 + wd] = grad_model[34 * b + 10 + wd] + s;
    }
}
// one (row, problem) of the measures JVP (cmpc_walk_measures_jvp): K columns, the layouts of cmpc_walk_dirs.  A row that does not count: zeros.
struct CmpcMeasureJvpArgs {
    int N, B, tick0, rows, K;
    const float* X; const float* P; const float* states;
    const int* end_tick;
    const float* corners; int corners_stride; double gravity;
    const double* dir_states; const float* dir_X; const float* dir_P; const double* dir_model;   // [rows + 1][B][K][9], [rows][B][K][n_x], [rows][B][K][n_p] or null, [B][K][34] or null
    double* dir_measures;                                                                      // [rows][B][K][4]
};
__host__ __device__ inline void cmpc_walk_measures_jvp_entry(const CmpcMeasureJvpArgs& v, int r, int b)
{
#pragma clang fp contract(off)
    const CmpcIdx L{v.N};
    const size_t rb = (size_t)r * v.B + b;
    double* out = v.dir_measures + 4 * rb * v.K;
    if (r >= cmpc_reference_rows_of(v.end_tick, b, v.tick0, v.rows)) {
        for (int i = 0; i < 4 * v.K; ++i) out[i] = 0.0;
        return;
    }
    const CmpcMeasureArgs a{v.N, v.B, v.X + (size_t)r * v.B * L.nx(), v.P + (size_t)r * v.B * L.np(), v.states + (size_t)(r + 1) * v.B * 9, v.corners,
                            v.corners_stride, v.gravity};
    CmpcMeasurePartials pt;
    cmpc_walk_measures_partials(a, b, pt);
    for (int k = 0; k < v.K; ++k) {
        const double* s = v.dir_states + (((size_t)(r + 1) * v.B + b) * v.K + k) * 9;
        const float* x = v.dir_X + (rb * v.K + k) * L.nx();
        double ds[5], dq[6], dref[2] = {0.0, 0.0}, dcn[24], dm[4];
        for (int i = 0; i < 5; ++i) ds[i] = s[i];
#pragma unroll
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < 3; ++i) dq[3 * c + i] = (double)x[L.oPos(c) + 3 + i];
        if (v.dir_P) {
            const float* p = v.dir_P + (rb * v.K + k) * L.np() + L.pComref() + 3;
            dref[0] = (double)p[0]; dref[1] = (double)p[1];
        }
#pragma unroll
        for (int i = 0; i < 24; ++i) dcn[i] = v.dir_model ? v.dir_model[((size_t)b * v.K + k) * 34 + 10 + i] : 0.0;
        cmpc_walk_measures_jvp_problem(a, b, pt, ds, dq, dref, dcn, v.dir_model != nullptr, nullptr, dm);
        for (int i = 0; i < 4; ++i) out[4 * k + i] = dm[i];
    }
}

// the cold start (cmpc_api.hip, cold_start): entry e of one problem's x from its p -- CoM at com0, feet at nominalPos, f_z = g8 per corner and
// stage, zero elsewhere
__host__ __device__ inline float cmpc_cold_start_entry(int N, int e, const float* p, float g8)
{
    const CmpcIdx L{N};
    if (e < 3 * (N + 1)) return p[L.pCom0() + e % 3];
    if (e < L.oPos(0)) return 0.f;
    const int c = e >= L.oPos(1) ? 1 : 0, q = e - L.oPos(c);
    if (q < 3 * (N + 1)) return p[L.pNom(c) + q];
    if (q < 3 * (N + 1) + 3 * N) return 0.f;          // the foot's velocity block
    return (q - 3 * (N + 1)) % 3 == 2 ? g8 : 0.f;     // corner forces [j][k][3]: 3 (N + 1) and 3 N are multiples of three
}

// ---- the refill of a walk's slots from a queue of trials (include/cmpc.h, cmpc_walk_refill): one slot's share of the two passes, one statement for the host
// form and the kernel.  Plain pointers, host or device alike; bit copies and integer words only.
struct CmpcRefillArgs {
    int B, Q, trial_ticks, tick_next;
    int* start; int* trial;                                                                   // per slot
    const float* state0;                                                                      // [Q][9]
    int* q_end_tick; int* q_end_code; int* q_it_sum; int* q_it_max; float* q_final_state; float* q_slack_min; int* q_ticks; int* q_slot; int* q_start;
    int* end_tick; int* end_code; int* it_sum; int* it_max; float* final_state; float* slack_min;   // the record's outcome, per slot
    float* state_live;                                                                        // [B][9], or null: archive only
    int* trial_of;                                                                            // this tick's row [B] of the trace, or null
};
// archive: an occupied slot's outcome words into its trial's row.  -> the slot is free (empty, its trial ended, or its trial walked trial_ticks ticks)
__host__ __device__ inline bool cmpc_refill_archive(const CmpcRefillArgs& a, int b)
{
    const int q = a.trial[b];
    if (q < 0 || q >= a.Q) return true;
    const int walked = a.tick_next - a.start[b];
    a.q_end_tick[q] = a.end_tick[b]; a.q_end_code[q] = a.end_code[b]; a.q_it_sum[q] = a.it_sum[b]; a.q_it_max[q] = a.it_max[b];
    for (int i = 0; i < 9; ++i) a.q_final_state[9 * (size_t)q + i] = a.final_state[9 * (size_t)b + i];
    a.q_slack_min[q] = a.slack_min[b];
    a.q_ticks[q] = walked;
    return a.end_tick[b] >= 0 || walked >= a.trial_ticks;
}
// retire and spawn: free slot b takes trial q -- its outcome as cmpc_outcome_init_kernel sets it -- or, with the queue empty (q >= Q), leaves every later
// launch through the ended mask (a slot that was empty already keeps the word it has)
__host__ __device__ inline void cmpc_refill_assign(const CmpcRefillArgs& a, int b, int q)
{
    if (q >= a.Q) {
        if (a.trial[b] >= 0 || a.end_tick[b] < 0) a.end_tick[b] = a.tick_next;
        a.trial[b] = -1;
        return;
    }
    a.trial[b] = q; a.start[b] = a.tick_next;
    a.end_tick[b] = -1; a.end_code[b] = 0; a.it_sum[b] = 0; a.it_max[b] = 0;
    for (int i = 0; i < 9; ++i) {
        const float v = a.state0[9 * (size_t)q + i];
        a.state_live[9 * (size_t)b + i] = v;
        a.final_state[9 * (size_t)b + i] = v;
    }
    a.slack_min[b] = __builtin_inff();
    a.q_slot[q] = b; a.q_start[q] = a.tick_next;
}

// the per-trial data of a refill walk (include/cmpc.h, cmpc_walk_refill_trials) as the front and back kernels of a tick take it: the caller's arrays, each
// null or indexed by trial (schedules [local tick][trial]), and for the models the handle's base record, its exp(-k) table and its per-problem table [B]
struct CmpcRefillTrialArgs {
    const cmpc_model* models; int* model_ok;                       // [Q]
    const CmpcConsts* base; const double* expk; CmpcConsts* table; // read / written only with models
    const float* hidden; int hidden_ticks;                         // [hidden_ticks][Q][6]
    const float* noise; int noise_ticks;                           // [noise_ticks][Q][9]
    const float* gain;                                             // [Q]
    int Q;
};
// the model of trial q into a slot's record, which holds a bit copy of the base record: cmpc_models_kernel's statement (cmpc_api.hip), so that the record is
// bit-equal to the one cmpc_set_models_device derives.  A row that breaks the model rule keeps the base model and is flagged.
__host__ __device__ inline void cmpc_refill_trial_model(const CmpcRefillTrialArgs& a, int q, CmpcConsts& rec)
{
    const cmpc_model m = a.models[q];
    const bool bad = cmpc_model_first_bad(m) >= 0;
    if (!bad) cmpc_consts_apply_model(rec, m, a.expk);
    rec.model_bad = bad ? 1 : 0;
    if (a.model_ok) a.model_ok[q] = bad ? 0 : 1;
}

// the host form's two loops (cmpc_rollout_refill_init, cmpc_rollout_refill): the slots in ascending order, the counter a plain int.  Here, and not in
// cmpc_api_rollout.hip, so that a stand-alone host program can run them under a sanitizer without the library.
inline void cmpc_refill_init_host(const CmpcRefillArgs& a, int* next)
{
    *next = 0;
    for (int b = 0; b < a.B; ++b) { a.start[b] = 0; a.trial[b] = -1; }
    for (int q = 0; q < a.Q; ++q) {
        a.q_end_tick[q] = -1; a.q_end_code[q] = 0; a.q_it_sum[q] = 0; a.q_it_max[q] = 0;
        for (int i = 0; i < 9; ++i) a.q_final_state[9 * (size_t)q + i] = a.state0[9 * (size_t)q + i];
        a.q_slack_min[q] = __builtin_inff();
        a.q_ticks[q] = 0; a.q_slot[q] = -1; a.q_start[q] = -1;
    }
}
inline void cmpc_refill_host(const CmpcRefillArgs& a, int* next)
{
    int base = 0;
    if (a.state_live) base = *next < 0 ? 0 : *next > a.Q ? a.Q : *next;
    for (int b = 0; b < a.B; ++b) {
        const bool is_free = cmpc_refill_archive(a, b);
        if (!a.state_live) continue;
        if (is_free) {
            cmpc_refill_assign(a, b, base);
            base = base + 1 > a.Q ? a.Q : base + 1;
        }
        if (a.trial_of) a.trial_of[b] = a.trial[b];
    }
    if (a.state_live) *next = base;
}

// ---- the device tape of a walk (include/cmpc.h, cmpc_walk_tape): one row from what a tick left.  Bit copies only; one argument block for the kernel.
// Part 1 (before a tick that runs in place): state_in -> states[row].  Part 2 (behind the tick): everything else, state_out -> states[row + 1].
struct CmpcTapeArgs {
    int B, M, nx, np, row, parts;
    const float* X; const float* P; const float* info; const int* ok; const int* land; const float* state_in; const float* state_out;
    const double* plan_t; const int* plan_n; const double* list_t; const int* list_n;
    float* t_X; float* t_P; float* t_info; float* t_states; int* t_ok; int* t_land; double* t_plan_t; double* t_list_t; int* t_plan_n; int* t_list_n;
};

// ---- the snapshot of a walk (include/cmpc.h, cmpc_walk_snapshot): destination problem b <- source problem index[b], bit copies.  Every array goes as
// rows of 32-bit words (a double is two); the table lists the arrays both sides have, at most CMPC_SNAP_ARRAYS = the 20 of the struct.
#define CMPC_SNAP_ARRAYS 20
struct CmpcSnapshotArgs {
    int B, src_B, count;
    const int* index; int* ok;                     // either may be null
    const unsigned* src[CMPC_SNAP_ARRAYS]; unsigned* dst[CMPC_SNAP_ARRAYS]; int words[CMPC_SNAP_ARRAYS];   // words: per problem
};
// the source problem of destination b, or -1: b itself without an index, else index[b] where it lies in [0, src_B)
__host__ __device__ inline int cmpc_snapshot_source(const CmpcSnapshotArgs& a, int b)
{
    const int s = a.index ? a.index[b] : b;
    return s >= 0 && s < a.src_B ? s : -1;
}

// ---- the restore launch of a refill walk whose trials start from a snapshot (include/cmpc.h, cmpc_walk_refill_snapshot): a slot spawned this tick receives
// the pool row of its trial.  copy: the snapshot's table with the pool as source (src_B = pool_batch) and the live buffers as destination, the pool's list
// sets already paired with the live sets of this tick's parity; copy.index is dTrialSnapshot, indexed by TRIAL, and copy.ok is not used.
struct CmpcRefillRestoreArgs {
    CmpcSnapshotArgs copy;
    const int* start; const int* trial;   // [B]: the slots' start ticks and trials
    int tick, Q, pool_tick;
    int* ok;                              // [Q] or null: dTrialSnapshotOk
    int* end_tick; int* end_code;         // [B]: the record's outcome words (a bad index ends its slot at spawn)
};
// the trial spawned in slot b this tick, or -1: none (one load for a slot that was not spawned)
__host__ __device__ inline int cmpc_refill_restore_trial(const CmpcRefillRestoreArgs& a, int b)
{
    if (a.start[b] != a.tick) return -1;
    const int q = a.trial[b];
    return q >= 0 && q < a.Q ? q : -1;
}
// the pool row of trial q, or -1 for an index outside the pool
__host__ __device__ inline int cmpc_refill_restore_source(const CmpcRefillRestoreArgs& a, int q)
{
    const int s = a.copy.index[q];
    return s >= 0 && s < a.copy.src_B ? s : -1;
}
// the host form's loop (cmpc_rollout_refill_restore); here for the reason cmpc_refill_host is
inline void cmpc_refill_restore_host(const CmpcRefillRestoreArgs& a)
{
    for (int b = 0; b < a.copy.B; ++b) {
        const int q = cmpc_refill_restore_trial(a, b);
        if (q < 0) continue;
        const int s = cmpc_refill_restore_source(a, q);
        if (a.ok) a.ok[q] = s >= 0 ? 1 : 0;
        if (s < 0) { a.end_tick[b] = a.pool_tick; a.end_code[b] = 0; continue; }
        for (int i = 0; i < a.copy.count; ++i) {
            const size_t w = (size_t)a.copy.words[i];
            __builtin_memcpy(a.copy.dst[i] + w * b, a.copy.src[i] + w * s, sizeof(unsigned) * w);
        }
    }
}

// ---- the plan select launch of a refill walk with plans per trial (include/cmpc.h, cmpc_walk_refill_plans): a slot spawned this tick receives the pool row
// of its trial into its rows of the planner's lists (and of the planner's trajectories).  Every array goes as rows of 32-bit words (a double is two); the
// table's order: the lists' times, poses and counts, then the CoM and the angular-momentum trajectory when the pool has them (count 3 or 5).
#define CMPC_PLAN_ARRAYS 5
struct CmpcRefillPlansArgs {
    int B, Q, tick, pool_plans, count;
    const int* start; const int* trial;   // [B]: the slots' start ticks and trials
    const int* index; int* ok;            // [Q] dTrialPlan; [Q] or null: dTrialPlanOk
    int* end_tick; int* end_code;         // [B]: the record's outcome words (a bad index ends its slot at spawn)
    const unsigned* src[CMPC_PLAN_ARRAYS]; unsigned* dst[CMPC_PLAN_ARRAYS]; int words[CMPC_PLAN_ARRAYS];   // words: per slot / per pool row
};
// the trial spawned in slot b this tick, or -1: none (one load for a slot that was not spawned)
__host__ __device__ inline int cmpc_refill_plans_trial(const CmpcRefillPlansArgs& a, int b)
{
    if (a.start[b] != a.tick) return -1;
    const int q = a.trial[b];
    return q >= 0 && q < a.Q ? q : -1;
}
// the pool row of trial q, or -1 for an index outside the pool
__host__ __device__ inline int cmpc_refill_plans_source(const CmpcRefillPlansArgs& a, int q)
{
    const int s = a.index[q];
    return s >= 0 && s < a.pool_plans ? s : -1;
}
// the host form's loop (cmpc_rollout_refill_plans); here for the reason cmpc_refill_host is
inline void cmpc_refill_plans_host(const CmpcRefillPlansArgs& a)
{
    for (int b = 0; b < a.B; ++b) {
        const int q = cmpc_refill_plans_trial(a, b);
        if (q < 0) continue;
        const int s = cmpc_refill_plans_source(a, q);
        if (a.ok) a.ok[q] = s >= 0 ? 1 : 0;
        if (s < 0) { a.end_tick[b] = 0; a.end_code[b] = 0; continue; }
        for (int i = 0; i < a.count; ++i) {
            const size_t w = (size_t)a.words[i];
            __builtin_memcpy(a.dst[i] + w * b, a.src[i] + w * s, sizeof(unsigned) * w);
        }
    }
}

// ---- the fold of per-trial gradients onto the rows of a pool (include/cmpc.h, cmpc_rollout_plan_fold_device): entry [p][w] is the sum, from +0.0 and in
// ascending q, of per[q][w] over the trials with index[q] == p.  A member is selected, never multiplied in; one function for the kernel and the host form.
__host__ __device__ inline double cmpc_plan_fold_entry(int Q, int words, const int* index, const double* per, int p, int w)
{
    double s = 0.0;
    for (int q = 0; q < Q; ++q)
        if (index[q] == p) s += per[(size_t)q * words + w];
    return s;
}

// ---- the tape of a refill walk regrouped by trial (include/cmpc.h, cmpc_walk_tape_regroup; DESIGN.md 7f "Refill, taped"): destination column j of a tape of
// trial_ticks rows receives the rows of trial index[j] out of the slot-major tape.  Bit copies; every array goes as rows of 32-bit words (a double is two).
// The table's order: X, P, lam_g, info, ok, land, list_t, list_n, then plan_t and plan_n (CMPC_REGROUP_PLAN .. : written zero on destination row 0).
#define CMPC_REGROUP_ARRAYS 10
#define CMPC_REGROUP_PLAN 8
struct CmpcRegroupArgs {
    int B, rows, src_rows, Q, tick_first;          // rows: the destination's = trial_ticks
    const int* index;                              // [B] dTrialIndex
    const int* slot; const int* start; const int* ticks; const int* end;   // [Q] dTrialSlot, dTrialStart, dTrialTicks, dTrialEndTick
    const unsigned* state0;                        // [Q][9]
    int* end_out; int* ok_out;                     // [B]; ok_out may be null
    const unsigned* src[CMPC_REGROUP_ARRAYS]; unsigned* dst[CMPC_REGROUP_ARRAYS]; int words[CMPC_REGROUP_ARRAYS];   // words: per problem and row
    const unsigned* src_states; unsigned* dst_states;   // [rows + 1][B][9]
};
// what column j is: kind 0 no trial (an index outside the queue, a slot outside the batch, or a needed source row outside the tape), 1 a trial never started,
// 2 a started trial of n recorded ticks whose local tick 0 is source row t0 of column s.  end: the end tick the reverse / forward walk is given -- the
// trial's own if it ended, n for a trial the walk's end cut off (good ticks i < n, states 0 .. n), else -1.  Every choice is a select.
struct CmpcRegroupColumn { int kind, q, s, t0, n, end; };
__host__ __device__ inline CmpcRegroupColumn cmpc_regroup_column(const CmpcRegroupArgs& a, int j)
{
    CmpcRegroupColumn c{0, a.index[j], -1, 0, 0, 0};
    if (c.q < 0 || c.q >= a.Q) return c;
    c.n = a.ticks[c.q];
    c.s = a.slot[c.q];
    if (c.n < 1) { c.kind = 1; return c; }
    const long long t0 = (long long)a.start[c.q] - a.tick_first;
    const int last = (c.n < a.rows ? c.n : a.rows) - 1;     // the last source row taken, local
    if (c.s < 0 || c.s >= a.B || t0 < 0 || t0 + last >= a.src_rows) return c;
    const int e = a.end[c.q];
    c.kind = 2; c.t0 = (int)t0;
    c.end = e >= 0 ? e : c.n < a.rows ? c.n : -1;
    return c;
}
// the source row of destination row r of a started column: rows past the trial's last recorded one repeat that row
__host__ __device__ inline int cmpc_regroup_source_row(const CmpcRegroupColumn& c, int r)
{
    return c.t0 + (r < c.n - 1 ? r : c.n - 1);
}
// the host form's loop (cmpc_rollout_tape_regroup); here for the reason cmpc_refill_host is
inline void cmpc_regroup_host(const CmpcRegroupArgs& a)
{
    const size_t B = (size_t)a.B;
    for (int j = 0; j < a.B; ++j) {
        const CmpcRegroupColumn c = cmpc_regroup_column(a, j);
        a.end_out[j] = c.kind == 2 ? c.end : 0;
        if (a.ok_out) a.ok_out[j] = c.kind == 0 ? 0 : 1;
        if (c.kind == 0) continue;
        __builtin_memcpy(a.dst_states + 9 * (size_t)j, a.state0 + 9 * (size_t)c.q, sizeof(unsigned) * 9);
        if (c.kind == 1) continue;
        for (int r = 0; r < a.rows; ++r) {
            const size_t sr = (size_t)cmpc_regroup_source_row(c, r);
            for (int i = 0; i < CMPC_REGROUP_ARRAYS; ++i) {
                const size_t w = (size_t)a.words[i];
                unsigned* const d = a.dst[i] + w * ((size_t)r * B + j);
                if (r == 0 && i >= CMPC_REGROUP_PLAN) __builtin_memset(d, 0, sizeof(unsigned) * w);
                else __builtin_memcpy(d, a.src[i] + w * (sr * B + c.s), sizeof(unsigned) * w);
            }
            __builtin_memcpy(a.dst_states + 9 * (((size_t)r + 1) * B + j), a.src_states + 9 * ((sr + 1) * B + c.s), sizeof(unsigned) * 9);
        }
    }
}

// ---- the reverse walk's rule for ended problems (include/cmpc.h, cmpc_rollout_walk_vjp_device).  One statement for the host form and the
// kernel (contraction off: the one sum is a plain double add).  A gate step sits between two reverse ticks: its POST part finishes tick `tick_post`
// (row_post) from what cmpc_rollout_tick_vjp_device left, its PRE part prepares tick `tick_pre` (row_pre).  Either part may be absent (do_post / do_pre).
// A problem b has ended at tick t when e = end_tick[b] >= 0 and t >= e (end_tick null: nobody has).  Ended: everything is SELECTED to zero -- never
// multiplied, so that stale or non-finite data of an ended problem cannot reach an output.
struct CmpcGateArgs {
    int B, M, N, nx, np;
    const int* end_tick;
    int do_post, tick_post;
    const double* seed_state;     // [B][9]: G of row_post
    const double* t_state;        // [B][9]: the tick's dGradState
    const double* t_list;         // [B][2][M][3]: the tick's dGradPrevList
    const float* t_sens;          // [B][CMPC_SENS]: the tick's dTickSens
    double* carry_state; double* carry_list;          // out (POST) / sanitised in place (PRE with `first`)
    float* wrench_row; float* gp_row; int* status_row; // rows of row_post; wrench_row / gp_row may be null
    int do_pre, tick_pre, first;  // first: the PRE part of the call's first gate step also selects zero in the caller's carries
    const int* ok_row;            // [B] tape row of row_pre
    const float* gx_row;          // [B][nx] seeds of row_pre, or null
    int* ok_out; float* gx_out;   // the gated copies the tick VJP reads (gx_out null with gx_row null)
    // the orientation chain (cmpc_rollout_walk_vjp_rot_device), every pointer null without it: l_rot_i = [i < e] (the tick's dGradPrevListRot), the row of
    // dGradRot and the removed word zero for i >= e
    const double* t_list_rot;     // [B][2][M][3]: the tick's dGradPrevListRot
    double* carry_list_rot;       // [B][2][M][3]: out (POST) / sanitised in place (PRE with `first`)
    double* rot_row;              // [B][2][N][3] of row_post: written only where the problem has ended
    float* removed_row;           // [B] of row_post: word 6 of the tick's dTickSens, 0 for an ended problem
};
__host__ __device__ inline bool cmpc_gate_ended(const int* end_tick, int b, int tick)
{
    const int e = end_tick ? end_tick[b] : -1;
    return e >= 0 && tick >= e;
}
// the small arrays of problem b
__host__ __device__ inline void cmpc_walk_gate_problem(const CmpcGateArgs& a, int b)
{
#pragma clang fp contract(off)
    const size_t nl = (size_t)6 * a.M;
    if (a.do_post) {
        const int e = a.end_tick ? a.end_tick[b] : -1;
        const bool ended = e >= 0 && a.tick_post >= e;
        for (int i = 0; i < 9; ++i) {
            const size_t o = 9 * (size_t)b + i;
            // c_i = [i < e] J_i^T c_{i+1} + [i <= e] G_i: the ending tick keeps its seed (s_e exists), later rows carry nothing
            a.carry_state[o] = !ended ? a.t_state[o] + a.seed_state[o] : a.tick_post == e ? a.seed_state[o] : 0.0;
        }
        for (size_t i = 0; i < nl; ++i) a.carry_list[nl * b + i] = ended ? 0.0 : a.t_list[nl * b + i];
        if (a.carry_list_rot) for (size_t i = 0; i < nl; ++i) a.carry_list_rot[nl * b + i] = ended ? 0.0 : a.t_list_rot[nl * b + i];
        a.status_row[b] = ended ? 6 : (int)a.t_sens[(size_t)b * CMPC_SENS];
        if (a.removed_row) a.removed_row[b] = ended ? 0.f : a.t_sens[(size_t)b * CMPC_SENS + 6];
    }
    if (a.do_pre) {
        const bool ended = cmpc_gate_ended(a.end_tick, b, a.tick_pre);
        a.ok_out[b] = ended ? 0 : (a.ok_row ? a.ok_row[b] : 1);
        if (a.first && ended) {
            for (int i = 0; i < 9; ++i) a.carry_state[9 * (size_t)b + i] = 0.0;
            for (size_t i = 0; i < nl; ++i) a.carry_list[nl * b + i] = 0.0;
            if (a.carry_list_rot) for (size_t i = 0; i < nl; ++i) a.carry_list_rot[nl * b + i] = 0.0;
        }
    }
}
// entry idx of the wide rows: [B][nx] (the gated dGradX copy), [B][N][6] (the wrench row), [B][np] (the dGradP row) and [B][2][N][3] (the dGradRot row);
// idx runs to B max(nx, np, 6 N)
__host__ __device__ inline void cmpc_walk_gate_wide(const CmpcGateArgs& a, size_t idx)
{
    if (a.do_pre && a.gx_out && idx < (size_t)a.B * a.nx)
        a.gx_out[idx] = cmpc_gate_ended(a.end_tick, (int)(idx / a.nx), a.tick_pre) ? 0.f : a.gx_row[idx];
    if (a.do_post) {
        const size_t nw = (size_t)6 * a.N;
        if (a.wrench_row && idx < (size_t)a.B * nw && cmpc_gate_ended(a.end_tick, (int)(idx / nw), a.tick_post)) a.wrench_row[idx] = 0.f;
        if (a.gp_row && idx < (size_t)a.B * a.np && cmpc_gate_ended(a.end_tick, (int)(idx / a.np), a.tick_post)) a.gp_row[idx] = 0.f;
        if (a.rot_row && idx < (size_t)a.B * nw && cmpc_gate_ended(a.end_tick, (int)(idx / nw), a.tick_post)) a.rot_row[idx] = 0.0;
    }
}

// ---- the forward walk's rule for ended problems (include/cmpc.h, cmpc_rollout_walk_jvp_device; DESIGN.md 7f, "Forwards"): the transpose of the rule
// above.  One statement for the host form and the kernel (contraction off, although nothing here is arithmetic: every line is a selection).  A gate step sits
// between two forward ticks: its POST part finishes tick `tick_post` in place on what cmpc_rollout_tick_jvp_device wrote, its PRE part prepares tick
// `tick_pre`.  t_{i+1} = [i < e] (the tick's state direction), the same for the lists and for the row of dx; status 6 and removed 0 for i >= e.  With
// `first` the PRE part also selects zero in the directions that enter the call for a problem with e < tick_pre (t_e and l_e exist, later ones are zero).
struct CmpcJvpGateArgs {
    int B, M, K, nx;
    const int* end_tick;
    int do_post, tick_post;
    const float* t_sens;                              // [B][CMPC_SENS]: the tick's dTickSens
    double* state_out; double* list_out; double* list_rot_out;   // [B][K][9], [B][K][2][M][3] (list_rot_out may be null): what the tick wrote
    float* x_row;                                     // [B][K][nx] or null
    int* status_row; float* removed_row;              // [B]; removed_row may be null
    int do_pre, tick_pre, first;
    const int* ok_row; int* ok_out;                   // [B] tape row of tick_pre (null: ones) and the gated copy the tick JVP reads
    double* first_state; double* first_list; double* first_list_rot;   // with `first`: what enters the call (each may be null)
};
// the small arrays of column col = b K + j; the per-problem words go with column 0
__host__ __device__ inline void cmpc_walk_jvp_gate_column(const CmpcJvpGateArgs& a, size_t col)
{
#pragma clang fp contract(off)
    const int b = (int)(col / (size_t)a.K);
    const bool col0 = col % (size_t)a.K == 0;
    const size_t nl = (size_t)6 * a.M;
    if (a.do_post) {
        const bool ended = cmpc_gate_ended(a.end_tick, b, a.tick_post);
        if (ended) {
            for (int i = 0; i < 9; ++i) a.state_out[9 * col + i] = 0.0;
            for (size_t i = 0; i < nl; ++i) a.list_out[nl * col + i] = 0.0;
            if (a.list_rot_out) for (size_t i = 0; i < nl; ++i) a.list_rot_out[nl * col + i] = 0.0;
        }
        if (col0) {
            a.status_row[b] = ended ? 6 : (int)a.t_sens[(size_t)b * CMPC_SENS];
            if (a.removed_row) a.removed_row[b] = ended ? 0.f : a.t_sens[(size_t)b * CMPC_SENS + 6];
        }
    }
    if (a.do_pre) {
        if (col0) a.ok_out[b] = cmpc_gate_ended(a.end_tick, b, a.tick_pre) ? 0 : (a.ok_row ? a.ok_row[b] : 1);
        if (a.first && cmpc_gate_ended(a.end_tick, b, a.tick_pre - 1)) {     // e < tick_pre: nothing enters
            if (a.first_state) for (int i = 0; i < 9; ++i) a.first_state[9 * col + i] = 0.0;
            if (a.first_list) for (size_t i = 0; i < nl; ++i) a.first_list[nl * col + i] = 0.0;
            if (a.first_list_rot) for (size_t i = 0; i < nl; ++i) a.first_list_rot[nl * col + i] = 0.0;
        }
    }
}
// entry idx of the wide row [B][K][nx]: the solutions' directions of tick_post
__host__ __device__ inline void cmpc_walk_jvp_gate_wide(const CmpcJvpGateArgs& a, size_t idx)
{
    if (a.do_post && a.x_row && idx < (size_t)a.B * a.K * a.nx && cmpc_gate_ended(a.end_tick, (int)(idx / ((size_t)a.K * a.nx)), a.tick_post)) a.x_row[idx] = 0.f;
}

// ---- the wrench sensor of a walk under hidden pushes (include/cmpc.h, cmpc_wrench_sensor; DESIGN.md 7f, "Sensed pushes"): what the MPC is told of the
// hidden-wrench schedule and what only the plant feels.  One statement of the rule for the host forms and the kernels (contraction off): every step is a
// select, so a value outside a schedule's range is never read and a zeroed reading is +0, not a product with zero.
struct CmpcSenseArgs {
    int N, B, tick0, rows;
    int tick_first; const float* hidden; int hidden_ticks;   // cmpc_plant_mismatch: the true schedule [hidden_ticks][B][6]
    int delay, hold; double band2;                            // cmpc_wrench_sensor; band2 = deadband * deadband, formed once in double
    const float* noise; int noise_ticks;                      // [noise_ticks][B][6] or null
};
// row `row` of schedule [ticks][B][6] (problem b) when it is inside the schedule, else null
__host__ __device__ inline const float* cmpc_sense_row(const float* sched, int ticks, long long row, int B, int b)
{
    return sched && row >= 0 && row < ticks ? sched + ((size_t)row * B + b) * 6 : nullptr;
}
// the reading of tick t and whether it passes the dead-band: !(n2 < band2), so a force on the threshold passes and so does a NaN
__host__ __device__ inline bool cmpc_wrench_reading(const CmpcSenseArgs& a, int t, int b, float* reading)
{
#pragma clang fp contract(off)
    const float* src = cmpc_sense_row(a.hidden, a.hidden_ticks, (long long)t - a.delay - a.tick_first, a.B, b);
    const float* nz = cmpc_sense_row(a.noise, a.noise_ticks, (long long)t - a.tick_first, a.B, b);
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const float s = src ? src[e] : 0.f;
        reading[e] = nz ? s + nz[e] : s;
    }
    const double x = (double)reading[0], y = (double)reading[1], z = (double)reading[2];
    const double n2 = (x * x + y * y) + z * z;
    return !(n2 < a.band2);
}
// tick tick0 + r, problem b: est[6] (the wrench every knot k < hold receives) and plant[6] (the tick's hidden row); returns pass
__host__ __device__ inline bool cmpc_wrench_sense_problem(const CmpcSenseArgs& a, int r, int b, float* est, float* plant)
{
#pragma clang fp contract(off)
    const int t = a.tick0 + r;
    float reading[6];
    const bool pass = cmpc_wrench_reading(a, t, b, reading);
    const float* tr = cmpc_sense_row(a.hidden, a.hidden_ticks, (long long)t - a.tick_first, a.B, b);
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const float tv = tr ? tr[e] : 0.f;
        est[e] = pass ? reading[e] : 0.f;
        plant[e] = pass ? tv - reading[e] : tv;
    }
    return pass;
}
// entry (r, b, k) of the forward: knot k of the wrench rows; the thread of knot 0 writes the plant row and the pass word too
__host__ __device__ inline void cmpc_wrench_sense_entry(const CmpcSenseArgs& a, float* wrench_rows, float* plant_rows, int* pass_rows, int r, int b, int k)
{
    float est[6], plant[6];
    const bool pass = cmpc_wrench_sense_problem(a, r, b, est, plant);
    const size_t rb = (size_t)r * a.B + b;
    if (wrench_rows) {
#pragma unroll
        for (int e = 0; e < 6; ++e) wrench_rows[(rb * a.N + k) * 6 + e] = k < a.hold ? est[e] : 0.f;
    }
    if (k == 0) {
#pragma unroll
        for (int e = 0; e < 6; ++e) plant_rows[rb * 6 + e] = plant[e];
        if (pass_rows) pass_rows[rb] = pass ? 1 : 0;
    }
}
// the transpose.  g of tick t, component c: pass ? (sum over k < hold of grad_wrench, ascending, in double) - grad_hidden : 0; the branch is recomputed
struct CmpcSenseVjpArgs {
    CmpcSenseArgs s;
    const float* grad_wrench;    // [rows][B][N][6]
    const double* grad_hidden;   // [rows][B][6], taken on the plant rows
    double* grad_true;           // [hidden_ticks][B][6]
    double* grad_noise;          // [noise_ticks][B][6] or null
};
__host__ __device__ inline bool cmpc_sense_in_rows(const CmpcSenseArgs& a, long long t) { return t >= a.tick0 && t < (long long)a.tick0 + a.rows; }
__host__ __device__ inline double cmpc_wrench_sense_g(const CmpcSenseVjpArgs& v, int t, int b, int c)
{
#pragma clang fp contract(off)
    float reading[6];
    if (!cmpc_wrench_reading(v.s, t, b, reading)) return 0.0;
    const size_t rb = (size_t)(t - v.s.tick0) * v.s.B + b;
    double sum = 0.0;
    for (int k = 0; k < v.s.hold; ++k) sum = sum + (double)v.grad_wrench[(rb * v.s.N + k) * 6 + c];
    return sum - v.grad_hidden[rb * 6 + c];
}
// output element (r, b, c) of both gradients: a gather, no atomics
__host__ __device__ inline void cmpc_wrench_sense_vjp_entry(const CmpcSenseVjpArgs& v, int r, int b, int c)
{
#pragma clang fp contract(off)
    const CmpcSenseArgs& a = v.s;
    const long long t = (long long)r + a.tick_first, td = t + a.delay;
    if (r < a.hidden_ticks) {
        const bool own = cmpc_sense_in_rows(a, t), read = cmpc_sense_in_rows(a, td);
        const double gh = own ? v.grad_hidden[((size_t)(t - a.tick0) * a.B + b) * 6 + c] : 0.0;
        const double g = read ? cmpc_wrench_sense_g(v, (int)td, b, c) : 0.0;
        v.grad_true[((size_t)r * a.B + b) * 6 + c] = own && read ? gh + g : own ? gh : g;
    }
    if (v.grad_noise && r < a.noise_ticks)
        v.grad_noise[((size_t)r * a.B + b) * 6 + c] = cmpc_sense_in_rows(a, t) ? cmpc_wrench_sense_g(v, (int)t, b, c) : 0.0;
}
// the tangent in K columns: column j depends on column j of the directions alone
struct CmpcSenseJvpArgs {
    CmpcSenseArgs s;
    int K;
    const double* dir_hidden;    // [hidden_ticks][B][K][6]
    const double* dir_noise;     // [noise_ticks][B][K][6] or null
    float* dir_wrench;           // [rows][B][K][N][6]
    double* dir_plant;           // [rows][B][K][6]
};
__host__ __device__ inline const double* cmpc_sense_dir_row(const double* sched, int ticks, long long row, int B, int K, int b, int j)
{
    return sched && row >= 0 && row < ticks ? sched + (((size_t)row * B + b) * K + j) * 6 : nullptr;
}
// entry (r, b, j, k): knot k of column j's wrench direction; the thread of knot 0 writes the plant direction too
__host__ __device__ inline void cmpc_wrench_sense_jvp_entry(const CmpcSenseJvpArgs& v, int r, int b, int j, int k)
{
#pragma clang fp contract(off)
    const CmpcSenseArgs& a = v.s;
    const int t = a.tick0 + r;
    float reading[6];
    const bool pass = cmpc_wrench_reading(a, t, b, reading);
    const double* dt = cmpc_sense_dir_row(v.dir_hidden, a.hidden_ticks, (long long)t - a.tick_first, a.B, v.K, b, j);
    const double* ds = cmpc_sense_dir_row(v.dir_hidden, a.hidden_ticks, (long long)t - a.delay - a.tick_first, a.B, v.K, b, j);
    const double* dn = cmpc_sense_dir_row(v.dir_noise, a.noise_ticks, (long long)t - a.tick_first, a.B, v.K, b, j);
    const size_t col = ((size_t)r * a.B + b) * v.K + j;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const double s = ds ? ds[e] : 0.0;
        const double rd = dn ? s + dn[e] : s;
        const double tv = dt ? dt[e] : 0.0;
        v.dir_wrench[(col * a.N + k) * 6 + e] = pass && k < a.hold ? (float)rd : 0.f;
        if (k == 0) v.dir_plant[col * 6 + e] = pass ? tv - rd : tv;
    }
}
