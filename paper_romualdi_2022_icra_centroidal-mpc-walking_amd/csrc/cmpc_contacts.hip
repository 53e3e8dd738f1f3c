// Batched contact-schedule kernels: one thread per (problem, foot).  The lists are a few dozen
// bytes per foot and the work is a handful of comparisons per knot: these kernels exist so that a Monte-Carlo
// roll-out (solve -> plant -> merge -> sample -> shift, every tick) never leaves HBM, not because they are hot.
// The logic itself is in cmpc_contacts.h, shared with the host entry points of the C ABI.
#include "cmpc_contacts.h"
#include "cmpc_launch.h"

namespace {

__global__ __launch_bounds__(128) void cmpc_contacts_merge_kernel(int B, int M, double now, const double* __restrict__ plan_t,
                                                                  const float* __restrict__ plan_pose, const int* __restrict__ plan_n,
                                                                  const double* __restrict__ mpc_t, const float* __restrict__ mpc_pose,
                                                                  const int* __restrict__ mpc_n, double* __restrict__ out_t,
                                                                  float* __restrict__ out_pose, int* __restrict__ out_n, int* __restrict__ ok)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // problem * 2 + foot
    if (e >= 2 * B) return;
    const size_t o = (size_t)e * M;
    // list lengths outside 0..M (the host entry point rejects them with CMPC_ERR_ARG): nothing is read, the merged list is empty, ok = 0
    const bool sane = plan_n[e] >= 0 && plan_n[e] <= M && mpc_n[e] >= 0 && mpc_n[e] <= M;
    if (!sane) out_n[e] = 0;
    const bool good = sane && cmpc_merge_foot(now, plan_t + 2 * o, plan_pose + 7 * o, plan_n[e], mpc_t + 2 * o, mpc_pose + 7 * o, mpc_n[e], M,
                                              out_t + 2 * o, out_pose + 7 * o, out_n + e);
    if (ok && !good) atomicAnd(ok + (e >> 1), 0);   // (ok[] starts at 1: cmpc_launch_contacts_merge fills it)
}

// forceSampleTime (CentroidalMPCBlock.cpp:586-592): one thread per (problem, foot, contact), cmpc_snap_contact.  Entries m >= n are copied unchanged
// (a no-op in place).  A list length outside 0..M or a failed contact clears the foot's status word: ok[problem] (ok_per_foot = 0, as the merge kernel)
// or ok[problem * 2 + foot] (ok_per_foot = 1: the roll-out tick, which empties only that foot); a foot whose length is out of range is not read or written.
// ended (the roll-out tick under cmpc_set_ended_device, else null): the entries of a problem whose word is >= 0 are neither read nor written.
__global__ __launch_bounds__(128) void cmpc_force_sample_time_kernel(int B, int M, long long dt_ns, const double* t, const int* __restrict__ n, double* out_t,
                                                                     int* __restrict__ ok, int ok_per_foot, const int* __restrict__ ended)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (problem * 2 + foot) * M + contact
    if (i >= 2LL * B * M) return;
    const int e = (int)(i / M), m = (int)(i - (long long)e * M);
    if (ended && ended[e >> 1] >= 0) return;
    const int ne = n[e];
    bool good = ne >= 0 && ne <= M;
    if (good) {
        if (m < ne) good = cmpc_snap_contact(t + 2 * i, dt_ns, out_t + 2 * i);
        else if (out_t != t) { out_t[2 * i] = t[2 * i]; out_t[2 * i + 1] = t[2 * i + 1]; }
    }
    if (ok && !good) atomicAnd(ok + (ok_per_foot ? e : e >> 1), 0);
}

__global__ __launch_bounds__(128) void cmpc_fill_int_kernel(int n, int v, int* __restrict__ dst)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) dst[e] = v;
}

// one workgroup (one wave) per problem, one thread per (foot, stage); the landing knots from the stages' contact flags in LDS.  (One thread per foot walking its N
// stages through global-memory latency took 33 us per launch whatever the batch: profiles/r04_rollout_tick_overhead.txt.)
__global__ __launch_bounds__(64) void cmpc_contacts_sample_kernel(int B, int N, int M, double dt, double now, const double* __restrict__ t,
                                                                  const float* __restrict__ pose, const int* __restrict__ n,
                                                                  const float* __restrict__ box /* upper[6] | lower[6] */,
                                                                  float* __restrict__ P, int* __restrict__ land)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const CmpcIdx L{N};
    __shared__ unsigned char acts[2][CMPC_NMAX];
    // An empty list (cmpc_merge_foot leaves one where the reference's updateContactPhaseList returns false, CentroidalMPCBlock.cpp:70-77,
    // and the reference then aborts the tick, :603-607) or a length beyond M has no owner to sample: the foot's blocks of P are left
    // as they are and the landing knot reads -2 (the host entry point returns CMPC_ERR_ARG for the same input).
    for (int e2 = tid; e2 < 2 * N; e2 += 64) {
        const int c = e2 / N, k = e2 - c * N, e = 2 * b + c;
        const size_t o = (size_t)e * M;
        if (n[e] >= 1 && n[e] <= M)
            acts[c][k] = cmpc_sample_stage(N, dt, now, c, k, t + 2 * o, pose + 7 * o, n[e], box, box + 6, P + (size_t)b * L.np()) ? 1 : 0;
    }
    __syncthreads();
    if (tid < 2 && land) {
        const int e = 2 * b + tid;
        land[e] = (n[e] < 1 || n[e] > M) ? -2 : cmpc_landing_knot(N, [&](int k) { return acts[tid][k] != 0; });
    }
}

// step adjustment: the next contact of every foot that lands inside the horizon takes the optimised landing position
__global__ __launch_bounds__(128) void cmpc_contacts_adjust_kernel(int B, int N, int M, double now, const float* __restrict__ X,
                                                                   const int* __restrict__ land, const double* __restrict__ t,
                                                                   float* __restrict__ pose, const int* __restrict__ n)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * B) return;
    const int b = e >> 1, c = e & 1;
    const int lk = land[e];
    if (lk < 0 || lk > N || n[e] < 1 || n[e] > M) return;   // (no landing inside the horizon, or a list that was not sampled)
    const CmpcIdx L{N};
    const size_t o = (size_t)e * M;
    const int nx = cmpc_next_contact(t + 2 * o, n[e], now);
    if (nx < 0) return;
    const float* x = X + (size_t)b * L.nx() + L.oPos(c) + 3 * lk;
    for (int i = 0; i < 3; ++i) pose[7 * (o + nx) + i] = x[i];
}

// Where the entries of a merged list came from (cmpc_merge_foot in reverse, from the times alone): ma = the previous list's active contact, which became merged
// entry 0, or -1; first = the planner's first future contact, which became merged entry n0 = (ma >= 0), or -1.  snap_dt_ns > 0: the planner's times pass
// through cmpc_snap_contact first, as in the forward tick.  Shared by the position and the orientation adjoint.
__device__ inline void cmpc_merge_sources(int M, double now, long long snap_dt_ns, const double* __restrict__ plan_t, int pn, const double* __restrict__ prev_t,
                                          int mn, int& ma, int& first)
{
    ma = -1; first = -1;
    if (mn >= 0 && mn <= M) ma = cmpc_active_contact(prev_t, mn, now);
    if (pn >= 0 && pn <= M) {
        if (snap_dt_ns > 0) {
            for (int m = 0; m < pn && first < 0; ++m) {
                double s[2];
                cmpc_snap_contact(plan_t + 2 * m, snap_dt_ns, s);
                if (cmpc_next_contact(s, 1, now) == 0) first = m;
            }
        } else first = cmpc_next_contact(plan_t, pn, now);
    }
}

// Adjoint of the list path of one tick in the contacts' POSITIONS (include/cmpc.h, cmpc_contacts_position_vjp_device): adjust (phase bit 1), sample + merge
// (phase bit 2).  One thread per (problem, foot); it owns that foot's entries of every output, so the sums need no atomics and their order is fixed:
// an entry of g_prev / g_plan receives first the list's own gradient g_out, then the sampling's terms stage by stage, k = 0 .. N-1 (stage 0: nominalPos_0,
// currentPos, nominalPos_1).  The index maps are re-derived from the TIMES with the forward's functions: cmpc_next_contact (adjust, merge),
// cmpc_stage_owner (sample), cmpc_active_contact (merge); snap_dt_ns > 0: the planner's times pass through cmpc_snap_contact first, as in the forward tick.
// Entries m >= list_n are not part of the list and carry no gradient.
__global__ __launch_bounds__(128) void cmpc_contacts_position_vjp_kernel(int B, int N, int M, double dt, double now, int phase, long long snap_dt_ns,
                                                                         const double* __restrict__ plan_t, const int* __restrict__ plan_n,
                                                                         const double* __restrict__ prev_t, const int* __restrict__ prev_n,
                                                                         const double* __restrict__ list_t, const int* __restrict__ list_n,
                                                                         const int* __restrict__ land, const int* __restrict__ ok,
                                                                         const double* __restrict__ g_out, const float* __restrict__ g_p, float* __restrict__ g_x,
                                                                         double* __restrict__ g_prev, double* __restrict__ g_plan, int* __restrict__ status)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // problem * 2 + foot
    if (e >= 2 * B) return;
    const int b = e >> 1, c = e & 1;
    const CmpcIdx L{N};
    const size_t o = (size_t)e * M;
    const bool merge = prev_t != nullptr;
    const bool good = !ok || ok[b] != 0;
    if ((phase & 2) && status && c == 0) status[b] = good ? 0 : 5;
    if (phase & 2)
        for (int m = 0; m < 3 * M; ++m) g_prev[3 * o + m] = 0.0;
    if (!good) return;                                     // (a failed merge: the tick was discarded -- zero outputs, g_x and g_plan untouched)
    const int n = list_n[e];
    const bool sampled = n >= 1 && n <= M;
    // adjust: the entry the step adjustment overwrote, or -1
    int nx = -1;
    const int lk = land ? land[e] : -1;
    if (sampled && lk >= 0 && lk <= N) nx = cmpc_next_contact(list_t + 2 * o, n, now);
    if ((phase & 1) && nx >= 0 && g_out)
        for (int i = 0; i < 3; ++i) {
            float* gx = g_x + (size_t)b * L.nx() + L.oPos(c) + 3 * lk + i;
            *gx = (float)((double)*gx + g_out[3 * (o + nx) + i]);
        }
    if (!(phase & 2)) return;
    // merge: where entry m of this tick's list came from
    int ma = -1, first = -1;
    if (merge) cmpc_merge_sources(M, now, snap_dt_ns, plan_t + 2 * o, plan_n[e], prev_t + 2 * o, prev_n[e], ma, first);
    const int n0 = ma >= 0 ? 1 : 0;
    auto dest = [&](int m) -> double* {                    // (null: the entry's gradient goes nowhere)
        if (!merge) return g_prev + 3 * (o + m);
        if (m < n0) return g_prev + 3 * (o + ma);
        if (first < 0 || !g_plan || first + m - n0 >= M) return nullptr;
        return g_plan + 3 * (o + first + m - n0);
    };
    const int nlist = n < 0 ? 0 : n > M ? M : n;
    if (g_out)
        for (int m = 0; m < nlist; ++m) {
            double* d = dest(m);
            if (!d || m == nx) continue;
            for (int i = 0; i < 3; ++i) d[i] += g_out[3 * (o + m) + i];
        }
    if (!sampled || !g_p) return;
    const float* gp = g_p + (size_t)b * L.np();
    for (int k = 0; k < N; ++k) {
        bool act;
        double* d = dest(cmpc_stage_owner(list_t + 2 * o, n, now + k * dt, &act));
        if (!d) continue;
        for (int i = 0; i < 3; ++i) {
            if (k == 0) d[i] += (double)gp[L.pNom(c) + i] + (double)gp[L.pCur(c) + i];
            d[i] += (double)gp[L.pNom(c) + 3 * (k + 1) + i];
        }
    }
}

// Adjoint of the sampling in the contacts' ORIENTATIONS (include/cmpc.h, cmpc_contacts_rotation_vjp_device): a sampled stage copies its owner's rotation, so
// in the body-frame tangent omega_stage = omega_owner and entry m receives the sum of g_rot over the stages it owns.  One thread per (problem, foot), the
// float64 sum in stage order k = 0 .. N-1 with the forward's own cmpc_stage_owner: no atomics, a fixed order.  Entries at or beyond n carry none; a foot
// that the sampling would not sample (empty list, or longer than M) gets zeros.
__global__ __launch_bounds__(128) void cmpc_contacts_rotation_vjp_kernel(int B, int N, int M, double dt, double now, const double* __restrict__ list_t,
                                                                         const int* __restrict__ list_n, const double* __restrict__ g_rot,
                                                                         double* __restrict__ g_list)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // problem * 2 + foot
    if (e >= 2 * B) return;
    const size_t o = (size_t)e * M;
    double* out = g_list + 3 * o;
    for (int m = 0; m < 3 * M; ++m) out[m] = 0.0;
    const int n = list_n[e];
    if (n < 1 || n > M) return;
    const double* g = g_rot + (size_t)e * 3 * N;
    for (int k = 0; k < N; ++k) {
        bool act;
        const int m = cmpc_stage_owner(list_t + 2 * o, n, now + k * dt, &act);
        for (int i = 0; i < 3; ++i) out[3 * m + i] += g[3 * k + i];
    }
}

// Adjoint of the list path of one tick in the contacts' ORIENTATIONS (include/cmpc.h, cmpc_contacts_orientation_vjp_device): the counterpart of the sample +
// merge part above, in the body-frame tangent of each entry's quaternion, where every copy the forward makes is the identity.  Entry m of this tick's list
// carries first its own g_out[m] -- ALL of them: the step adjustment overwrites positions only, so the landing entry's orientation passes through -- then
// the sampling's terms, g_rot of the stages it owns, stage by stage, k = 0 .. N-1 (cmpc_stage_owner); the merge transposed sends entry 0 to the previous
// list's active contact and the rest to the planner's entries (+=).  One thread per (problem, foot) owns its outputs: no atomics, a fixed order.  A foot
// that was not sampled (an empty list, one longer than M, land = -2) passes nothing on.
__global__ __launch_bounds__(128) void cmpc_contacts_orientation_vjp_kernel(int B, int N, int M, double dt, double now, long long snap_dt_ns,
                                                                            const double* __restrict__ plan_t, const int* __restrict__ plan_n,
                                                                            const double* __restrict__ prev_t, const int* __restrict__ prev_n,
                                                                            const double* __restrict__ list_t, const int* __restrict__ list_n,
                                                                            const int* __restrict__ land, const int* __restrict__ ok,
                                                                            const double* __restrict__ g_out, const double* __restrict__ g_rot,
                                                                            double* __restrict__ g_prev, double* __restrict__ g_plan, int* __restrict__ status)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // problem * 2 + foot
    if (e >= 2 * B) return;
    const int b = e >> 1, c = e & 1;
    const size_t o = (size_t)e * M;
    const bool merge = prev_t != nullptr;
    const bool good = !ok || ok[b] != 0;
    if (status && c == 0) status[b] = good ? 0 : 5;
    for (int m = 0; m < 3 * M; ++m) g_prev[3 * o + m] = 0.0;
    const int n = list_n[e];
    if (!good || n < 1 || n > M || (land && land[e] == -2)) return;
    int ma = -1, first = -1;
    if (merge) cmpc_merge_sources(M, now, snap_dt_ns, plan_t + 2 * o, plan_n[e], prev_t + 2 * o, prev_n[e], ma, first);
    const int n0 = ma >= 0 ? 1 : 0;
    auto dest = [&](int m) -> double* {                    // (null: the entry's gradient goes nowhere)
        if (!merge) return g_prev + 3 * (o + m);
        if (m < n0) return g_prev + 3 * (o + ma);
        if (first < 0 || !g_plan || first + m - n0 >= M) return nullptr;
        return g_plan + 3 * (o + first + m - n0);
    };
    if (g_out)
        for (int m = 0; m < n; ++m) {
            double* d = dest(m);
            if (!d) continue;
            for (int i = 0; i < 3; ++i) d[i] += g_out[3 * (o + m) + i];
        }
    if (!g_rot) return;
    const double* g = g_rot + (size_t)e * 3 * N;
    for (int k = 0; k < N; ++k) {
        bool act;
        double* d = dest(cmpc_stage_owner(list_t + 2 * o, n, now + k * dt, &act));
        if (!d) continue;
        for (int i = 0; i < 3; ++i) d[i] += g[3 * k + i];
    }
}

// The list path of one tick FORWARDS, positions and orientations together (include/cmpc.h, cmpc_contacts_jvp_device): the transpose of the position and the
// orientation VJP above, with their tape arguments and the same index maps (cmpc_merge_sources, cmpc_stage_owner, cmpc_next_contact).  One thread per
// (problem, foot, column) owns its outputs -- the foot's entries of the list directions, its nominalPos / currentPos rows of the column's p direction and
// its stages of the rotation direction: copies only, no sums, no atomics.  Phase bit 1 (before the solve): merge + sample, every output written whole;
// phase bit 2 (after it): the entry the step adjustment overwrote takes the solution's direction at the landing knot.  Directions are [B][K][...].
__global__ __launch_bounds__(128) void cmpc_contacts_jvp_kernel(int B, int N, int M, int K, double dt, double now, int phase, long long snap_dt_ns,
                                                                const double* __restrict__ plan_t, const int* __restrict__ plan_n,
                                                                const double* __restrict__ prev_t, const int* __restrict__ prev_n,
                                                                const double* __restrict__ list_t, const int* __restrict__ list_n,
                                                                const int* __restrict__ land, const int* __restrict__ ok,
                                                                const double* __restrict__ d_prev, const double* __restrict__ d_prev_rot,
                                                                const double* __restrict__ d_plan, const double* __restrict__ d_plan_rot,
                                                                const float* __restrict__ d_x, double* __restrict__ d_list, double* __restrict__ d_list_rot,
                                                                float* __restrict__ d_p, double* __restrict__ d_rot, int* __restrict__ status)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (problem * 2 + foot) * K + column
    if (i >= 2LL * B * K) return;
    const int e = (int)(i / K), j = (int)(i - (long long)e * K);
    const int b = e >> 1, c = e & 1;
    const CmpcIdx L{N};
    const size_t o = (size_t)e * M;                            // the foot's times
    const size_t od = (((size_t)b * K + j) * 2 + c) * M;       // the foot's entries of column j
    const bool merge = prev_t != nullptr;
    const bool good = !ok || ok[b] != 0;
    if (status && c == 0 && j == 0) status[b] = good ? 0 : 5;
    const int n = list_n[e];
    const bool sampled = good && n >= 1 && n <= M && !(land && land[e] == -2);
    if (phase & 1) {
        int ma = -1, first = -1;
        if (sampled && merge) cmpc_merge_sources(M, now, snap_dt_ns, plan_t + 2 * o, plan_n[e], prev_t + 2 * o, prev_n[e], ma, first);
        const int n0 = ma >= 0 ? 1 : 0;
        auto src = [&](const double* dv, const double* dl, int m) -> const double* {    // (null: the entry's direction is zero)
            if (!merge) return dv ? dv + 3 * (od + m) : nullptr;
            if (m < n0) return dv ? dv + 3 * (od + ma) : nullptr;
            if (first < 0 || !dl || first + m - n0 >= M) return nullptr;
            return dl + 3 * (od + first + m - n0);
        };
        for (int m = 0; m < M; ++m) {
            const bool in = sampled && m < n;
            const double* sp = in ? src(d_prev, d_plan, m) : nullptr;
            const double* sr = in ? src(d_prev_rot, d_plan_rot, m) : nullptr;
            for (int a = 0; a < 3; ++a) {
                if (d_list) d_list[3 * (od + m) + a] = sp ? sp[a] : 0.0;
                if (d_list_rot) d_list_rot[3 * (od + m) + a] = sr ? sr[a] : 0.0;
            }
        }
        if (d_p || d_rot) {
            float* dp = d_p ? d_p + ((size_t)b * K + j) * L.np() : nullptr;
            double* dr = d_rot ? d_rot + (((size_t)b * K + j) * 2 + c) * 3 * N : nullptr;
            for (int k = 0; k < N; ++k) {
                const double* sp = nullptr;
                const double* sr = nullptr;
                if (sampled) {
                    bool act;
                    const int w = cmpc_stage_owner(list_t + 2 * o, n, now + k * dt, &act);
                    sp = src(d_prev, d_plan, w);
                    sr = src(d_prev_rot, d_plan_rot, w);
                }
                for (int a = 0; a < 3; ++a) {
                    const float v = sp ? (float)sp[a] : 0.f;
                    if (dp) {
                        if (k == 0) { dp[L.pNom(c) + a] = v; dp[L.pCur(c) + a] = v; }
                        dp[L.pNom(c) + 3 * (k + 1) + a] = v;
                    }
                    if (dr) dr[3 * k + a] = sr ? sr[a] : 0.0;
                }
            }
        }
    }
    if (phase & 2) {
        if (!good) {                                           // (a flagged tick: nothing of it goes on)
            for (int m = 0; m < 3 * M; ++m) {
                if (d_list) d_list[3 * od + m] = 0.0;
                if (d_list_rot) d_list_rot[3 * od + m] = 0.0;
            }
            return;
        }
        const int lk = land ? land[e] : -1;
        if (!sampled || lk < 0 || lk > N || !d_list) return;
        const int nx = cmpc_next_contact(list_t + 2 * o, n, now);
        if (nx < 0) return;
        for (int a = 0; a < 3; ++a)
            d_list[3 * (od + nx) + a] = d_x ? (double)d_x[((size_t)b * K + j) * L.nx() + L.oPos(c) + 3 * lk + a] : 0.0;
    }
}

// measured state (and external wrench) into the parameter rows of every problem: setState on the device
__global__ __launch_bounds__(128) void cmpc_write_state_kernel(int B, int N, const float* __restrict__ state, const float* __restrict__ wrench,
                                                               float* __restrict__ P)
{
    const int b = blockIdx.x;
    const CmpcIdx L{N};
    float* p = P + (size_t)b * L.np();
    for (int e = threadIdx.x; e < 9; e += blockDim.x) p[L.pCom0() + e] = state[9 * (size_t)b + e];
    if (wrench)
        for (int e = threadIdx.x; e < 3 * N; e += blockDim.x) {
            const int k = e / 3, i = e % 3;
            p[L.pFext() + e] = wrench[((size_t)b * N + k) * 6 + i];
            p[L.pText() + e] = wrench[((size_t)b * N + k) * 6 + 3 + i];
        }
}

// 8f-3 on the device: comRef / hRef of every problem from the planner's trajectories, one thread per knot (cmpc_resample_reference_knot)
__global__ __launch_bounds__(64) void cmpc_reference_from_planner_kernel(int B, int N, int n_in, double dt, double in_dt, double t_offset, double robot_mass,
                                                                         double com_height, const float* __restrict__ com_in, const float* __restrict__ h_in,
                                                                         float* __restrict__ P)
{
    const int b = blockIdx.x;
    const CmpcIdx L{N};
    float* p = P + (size_t)b * L.np();
    for (int k = threadIdx.x; k <= N; k += 64)
        cmpc_resample_reference_knot(com_in + (size_t)b * n_in * 3, h_in + (size_t)b * n_in * 3, n_in, in_dt, t_offset, dt, k, robot_mass, com_height,
                                     p + L.pComref() + 3 * k, p + L.pHref() + 3 * k);
}

// The kernel above in reverse, summed over the rows of a walk (include/cmpc.h, cmpc_reference_from_planner_vjp_device): one workgroup per (problem, tile of
// 128 planner knots), one lane per planner knot, which owns that knot's six outputs -- no atomics, and the sum in ascending (row, knot) order.  The rows
// go through LDS in chunks of CMPC_REF_CHUNK.  Staging, one thread per (row, MPC knot, component): it loads the component's comRef / hRef gradient from
// dGradP (consecutive threads read consecutive floats; the rows are B n_p apart, the problems n_p), forms (i0, w) and leaves the four terms the knot sends
// to planner knots i0 and i0 + 1 (cmpc_reference_vjp_terms: the products and the divisions by the mass happen here, once, not in the divergent scan) and
// i0 itself in LDS.  Scan: every lane walks the chunk in (row, knot) order and adds the terms of the knots whose i0 or i0 + 1 it is (all lanes read one
// i0: a broadcast).  The loop bound is the problem's, so it is uniform over the workgroup, and both barriers sit in it unconditionally: an ended problem
// runs fewer chunks, nobody returns in front of a barrier.  Rows at or past the problem's end and, with a fixed height, the z entries of comRef are never
// loaded.  A lane past `knots` stages and waits with the others and touches no output.
#define CMPC_REF_CHUNK 8
__global__ __launch_bounds__(128) void cmpc_reference_vjp_kernel(CmpcRefArgs a, const int* __restrict__ end_tick, const float* __restrict__ grad_p,
                                                                 double* __restrict__ grad_com, double* __restrict__ grad_h)
{
    const int b = blockIdx.x, tid = threadIdx.x, j = blockIdx.y * 128 + tid;
    const CmpcIdx L{a.N};
    const int K1 = a.N + 1, n3 = 3 * K1, np = L.np(), base = L.pComref();
    const bool z_fixed = a.com_height == a.com_height;
    __shared__ double st[CMPC_REF_CHUNK][CMPC_NMAX + 1][2][6];    // [row][knot][to i0 | to i0 + 1][com x y z, h x y z]
    __shared__ int si[CMPC_REF_CHUNK][CMPC_NMAX + 1];
    const int rows = cmpc_reference_rows_of(end_tick, b, a.tick0, a.rows);      // (one problem per workgroup: uniform)
    const bool own = j < a.knots;
    const size_t o = ((size_t)b * a.knots + (own ? j : 0)) * 3;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (own)
        for (int i = 0; i < 3; ++i) {
            if (grad_com) acc[i] = grad_com[o + i];
            if (grad_h) acc[3 + i] = grad_h[o + i];
        }
    for (int r0 = 0; r0 < rows; r0 += CMPC_REF_CHUNK) {
        const int nr = rows - r0 < CMPC_REF_CHUNK ? rows - r0 : CMPC_REF_CHUNK;
        for (int q = tid; q < nr * n3; q += 128) {
            const int rr = q / n3, e3 = q - rr * n3, k = e3 / 3, c = e3 - 3 * k;
            const float* g = grad_p + ((size_t)(r0 + rr) * a.B + b) * np + base;
            const bool with_com = !(z_fixed && c == 2);
            int i0; double w, tc[2] = {0.0, 0.0}, th[2];
            cmpc_reference_weight(a.knots, a.in_dt, a.t_first, a.dt, a.tick0 + r0 + rr, k, &i0, &w);
            cmpc_reference_vjp_terms(w, with_com, with_com ? g[e3] : 0.f, g[n3 + e3], a.robot_mass, tc, th);
            if (c == 0) si[rr][k] = i0;
            for (int t = 0; t < 2; ++t) { st[rr][k][t][c] = tc[t]; st[rr][k][t][3 + c] = th[t]; }
        }
        __syncthreads();
        if (own)
            for (int rr = 0; rr < nr; ++rr)
                for (int k = 0; k < K1; ++k) {
                    const int i0 = si[rr][k];
                    if (j != i0 && j != i0 + 1) continue;
                    const double* t = st[rr][k][j == i0 ? 0 : 1];
                    for (int c = 0; c < 3; ++c) {
                        if (!(z_fixed && c == 2)) acc[c] += t[c];
                        acc[3 + c] += t[3 + c];
                    }
                }
        __syncthreads();
    }
    if (own && rows > 0)
        for (int i = 0; i < 3; ++i) {
            if (grad_com) grad_com[o + i] = acc[i];
            if (grad_h) grad_h[o + i] = acc[3 + i];
        }
}

// ... and forwards in K columns (cmpc_reference_from_planner_jvp_device): one thread per written entry, (row, problem, column, entry of the 6 (N + 1)
// reference rows) with the entry fastest, so a wave writes consecutive floats; nothing else of dir_p is touched.  No LDS, no barrier, no atomics.
__global__ __launch_bounds__(256) void cmpc_reference_jvp_kernel(CmpcRefArgs a, const double* __restrict__ dir_com, const double* __restrict__ dir_h,
                                                                 float* __restrict__ dir_p)
{
    const CmpcIdx L{a.N};
    const size_t per = 6 * (size_t)(a.N + 1), cols = (size_t)a.B * a.K;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)a.rows * cols * per) return;
    const size_t col = idx / per, r = col / cols, bk = col - r * cols;    // col = (row * B + problem) * K + column
    const int e6 = (int)(idx - col * per);
    const size_t in = bk * a.knots * 3;
    dir_p[col * L.np() + L.pComref() + e6] = cmpc_reference_jvp_entry(a, a.tick0 + (int)r, e6, dir_com ? dir_com + in : nullptr, dir_h ? dir_h + in : nullptr);
}

}  // namespace

extern "C" int cmpc_launch_reference_vjp(const CmpcRefArgs* a, const int* end_tick, const float* grad_p, double* grad_com, double* grad_h, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_reference_vjp_kernel, dim3(a->B, (a->knots + 127) / 128), dim3(128), 0, stream, *a, end_tick, grad_p, grad_com, grad_h);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_reference_jvp(const CmpcRefArgs* a, const double* dir_com, const double* dir_h, float* dir_p, hipStream_t stream)
{
    const size_t total = (size_t)a->rows * a->B * a->K * 6 * (a->N + 1);
    hipLaunchKernelGGL(cmpc_reference_jvp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *a, dir_com, dir_h, dir_p);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_reference_from_planner(int B, int N, int n_in, double dt, double in_dt, double t_offset, double robot_mass, double com_height,
                                                  const float* com_in, const float* h_in, float* P, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_reference_from_planner_kernel, dim3(B), dim3(64), 0, stream, B, N, n_in, dt, in_dt, t_offset, robot_mass, com_height, com_in, h_in, P);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_contacts_merge(int B, int M, double now, const double* plan_t, const float* plan_pose, const int* plan_n,
                                          const double* mpc_t, const float* mpc_pose, const int* mpc_n, double* out_t, float* out_pose,
                                          int* out_n, int* ok, hipStream_t stream)
{
    if (ok) hipLaunchKernelGGL(cmpc_fill_int_kernel, dim3((B + 127) / 128), dim3(128), 0, stream, B, 1, ok);
    hipLaunchKernelGGL(cmpc_contacts_merge_kernel, dim3((2 * B + 127) / 128), dim3(128), 0, stream, B, M, now, plan_t, plan_pose, plan_n,
                       mpc_t, mpc_pose, mpc_n, out_t, out_pose, out_n, ok);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_force_sample_time(int B, int M, long long dt_ns, const double* t, const int* n, double* out_t, int* ok, int ok_per_foot,
                                             const int* ended, hipStream_t stream)
{
    if (ok) hipLaunchKernelGGL(cmpc_fill_int_kernel, dim3((B * (ok_per_foot ? 2 : 1) + 127) / 128), dim3(128), 0, stream, B * (ok_per_foot ? 2 : 1), 1, ok);
    const long long threads = 2LL * B * M;
    hipLaunchKernelGGL(cmpc_force_sample_time_kernel, dim3((unsigned)((threads + 127) / 128)), dim3(128), 0, stream, B, M, dt_ns, t, n, out_t, ok, ok_per_foot, ended);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_contacts_sample(int B, int N, int M, double dt, double now, const double* t, const float* pose, const int* n,
                                           const float* box, float* P, int* land, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_contacts_sample_kernel, dim3(B), dim3(64), 0, stream, B, N, M, dt, now, t, pose, n, box, P, land);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_contacts_adjust(int B, int N, int M, double now, const float* X, const int* land, const double* t, float* pose,
                                           const int* n, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_contacts_adjust_kernel, dim3((2 * B + 127) / 128), dim3(128), 0, stream, B, N, M, now, X, land, t, pose, n);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_write_state(int B, int N, const float* state, const float* wrench, float* P, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_write_state_kernel, dim3(B), dim3(128), 0, stream, B, N, state, wrench, P);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_contacts_position_vjp(int B, int N, int M, double dt, double now, int phase, long long snap_dt_ns, const double* plan_t,
                                                 const int* plan_n, const double* prev_t, const int* prev_n, const double* list_t, const int* list_n,
                                                 const int* land, const int* ok, const double* g_out, const float* g_p, float* g_x, double* g_prev,
                                                 double* g_plan, int* status, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_contacts_position_vjp_kernel, dim3((2 * B + 127) / 128), dim3(128), 0, stream, B, N, M, dt, now, phase, snap_dt_ns, plan_t, plan_n,
                       prev_t, prev_n, list_t, list_n, land, ok, g_out, g_p, g_x, g_prev, g_plan, status);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_contacts_jvp(int B, int N, int M, int K, double dt, double now, int phase, long long snap_dt_ns, const double* plan_t,
                                        const int* plan_n, const double* prev_t, const int* prev_n, const double* list_t, const int* list_n, const int* land,
                                        const int* ok, const double* d_prev, const double* d_prev_rot, const double* d_plan, const double* d_plan_rot,
                                        const float* d_x, double* d_list, double* d_list_rot, float* d_p, double* d_rot, int* status, hipStream_t stream)
{
    const long long threads = 2LL * B * K;
    hipLaunchKernelGGL(cmpc_contacts_jvp_kernel, dim3((unsigned)((threads + 127) / 128)), dim3(128), 0, stream, B, N, M, K, dt, now, phase, snap_dt_ns, plan_t,
                       plan_n, prev_t, prev_n, list_t, list_n, land, ok, d_prev, d_prev_rot, d_plan, d_plan_rot, d_x, d_list, d_list_rot, d_p, d_rot, status);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_contacts_rotation_vjp(int B, int N, int M, double dt, double now, const double* list_t, const int* list_n, const double* g_rot,
                                                 double* g_list, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_contacts_rotation_vjp_kernel, dim3((2 * B + 127) / 128), dim3(128), 0, stream, B, N, M, dt, now, list_t, list_n, g_rot, g_list);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_contacts_orientation_vjp(int B, int N, int M, double dt, double now, long long snap_dt_ns, const double* plan_t, const int* plan_n,
                                                    const double* prev_t, const int* prev_n, const double* list_t, const int* list_n, const int* land,
                                                    const int* ok, const double* g_out, const double* g_rot, double* g_prev, double* g_plan, int* status,
                                                    hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_contacts_orientation_vjp_kernel, dim3((2 * B + 127) / 128), dim3(128), 0, stream, B, N, M, dt, now, snap_dt_ns, plan_t, plan_n,
                       prev_t, prev_n, list_t, list_n, land, ok, g_out, g_rot, g_prev, g_plan, status);
    return (int)hipGetLastError();
}
