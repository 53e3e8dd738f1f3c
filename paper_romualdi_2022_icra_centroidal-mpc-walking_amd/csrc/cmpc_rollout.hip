// The kernels of the closed-loop roll-out on gfx950 and their launchers: the plant step between two MPC ticks and its JVP / VJP, the front and back
// kernels of a tick (everything in front of the solve, everything behind it, in plain, refill and per-trial form), the record and the outcome arrays of a
// walk, the refill of ended slots and its restore from a snapshot, the cold start, the tape, the snapshot copy, the gates of the reverse and the forward
// walk, the kernels of a tick's derivative chains, the warm shift, and the compact per-problem output.  The per-problem logic they share with the host entry
// points is in cmpc_contacts.h; the entry points that queue them are in cmpc_api.hip, cmpc_api_rollout.hip and cmpc_api_walk_grad.hip.
#include "cmpc_contacts.h"
#include "cmpc_device.h"
#include "cmpc_launch.h"

// ---------------------------------------------------------------------------------------------
// Closed-loop plant between two MPC ticks: what WholeBodyQPBlock does with the MPC
// output -- centroidal dynamics driven by the first-knot corner forces of the active contacts plus
// the external wrench, RK4 with the forces held (src/centroidal-mpc-walking/src/
// WholeBodyQPBlock.cpp:1083-1084, 1150, 1259-1262), and the desired ZMP from the corner forces
// (:805-873: per-foot local ZMP = (-tau_y, tau_x)/f_z clamped to the sole, f_z-weighted mean in the
// world frame).  Everything mass-normalised like the MPC.  One thread per problem (a few hundred
// flops): the kernel is HBM/launch bound and exists so that Monte-Carlo roll-outs never leave HBM.
namespace {

// (problem b, one thread.  state_in / state_out may alias: everything is read before anything is written)
// corners: [2][4][3] of problem 0; problem b's are corners_stride floats further on (0: one set for the batch; per-problem models: the stride of the records)
// MM (cmpc_plant_mismatch, include/cmpc.h): the plant is not the model -- hidden[B][6] (or null: the term is not added) is a wrench the plant feels and dP
// does not hold, gain[B] (or null: 1, no multiply) scales every corner force the plant applies.  Both are loaded up front with the state, whatever the
// contact flags turn out to be, for the reason given at the force load below.  MM = false is the function without either, instruction for instruction.
// PL (the refill walk's per-trial mismatch, cmpc_walk_refill_trials): hidden and gain are this LANE's own -- its trial's row [6] and its trial's word, or
// null -- and not arrays over the batch; the arithmetic is the same statement for statement.
template <bool MM, bool PL = false>
__device__ inline void plant_step_problem(int N, int b, float grav, const float* __restrict__ corners, int corners_stride, const float* __restrict__ X,
                                          const float* __restrict__ P, const float* state_in, float* state_out, float* __restrict__ zmp, float h,
                                          int nsub, float zx, float zy, const float* __restrict__ hidden, const float* __restrict__ gain)
{
    CmpcIdx L{N};
    const float* x = X + (size_t)b * L.nx();
    const float* p = P + (size_t)b * L.np();
    double com[3], v[3], hm[3], fsum[3] = {0, 0, 0}, ext_t[3];
    float hid[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gn = 1.f;
    if (MM) {
        if (hidden)
            for (int i = 0; i < 6; ++i) hid[i] = hidden[(PL ? (size_t)0 : (size_t)b * 6) + i];
        if (gain) gn = gain[PL ? 0 : b];
    }
    for (int i = 0; i < 3; ++i) {
        com[i] = state_in[(size_t)b * 9 + i]; v[i] = state_in[(size_t)b * 9 + 3 + i]; hm[i] = state_in[(size_t)b * 9 + 6 + i];
        ext_t[i] = p[L.pText() + i];
        if (MM && hidden) ext_t[i] += (double)hid[3 + i];   // (tauExt_0 + tauHidden) + sum_q cp_q x f_q
    }
    // contact points (world) and forces of the active contacts at knot 0
    double cp[8][3], cf[8][3];
    double zw[2] = {0, 0}, ztot = 0;
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c);  // col-major vec of knot 0
        const bool on = p[L.pGam(c)] > 0.5f;
        double F[3] = {0, 0, 0}, T[3] = {0, 0, 0};
        for (int j = 0; j < 4; ++j) {
            const float* cn = corners + (size_t)b * corners_stride + 12 * c + 3 * j;
            double fl[3];
            for (int i = 0; i < 3; ++i) {
                cp[4 * c + j][i] = (double)x[L.oPos(c) + i] + (double)R[i] * cn[0] + (double)R[3 + i] * cn[1] + (double)R[6 + i] * cn[2];
                const float fv = x[L.oF(c, j) + i];   // (loaded whatever `on` is: a load behind the contact flag is a second global-memory round trip on this one-thread chain)
                if (MM && gain) cf[4 * c + j][i] = on ? (double)gn * (double)fv : 0.0;   // (the applied force: fsum, tau0 and the ZMP's F, T all see it)
                else cf[4 * c + j][i] = on ? (double)fv : 0.0;
                fsum[i] += cf[4 * c + j][i];
            }
            for (int i = 0; i < 3; ++i) fl[i] = (double)R[3 * i] * cf[4 * c + j][0] + (double)R[3 * i + 1] * cf[4 * c + j][1] + (double)R[3 * i + 2] * cf[4 * c + j][2];
            for (int i = 0; i < 3; ++i) F[i] += cf[4 * c + j][i];
            T[0] += cn[1] * fl[2] - cn[2] * fl[1];
            T[1] += cn[2] * fl[0] - cn[0] * fl[2];
            T[2] += cn[0] * fl[1] - cn[1] * fl[0];
        }
        if (F[2] > 0.001) {
            double lx = fmin((double)zx, fmax(-(double)zx, -T[1] / F[2]));
            double ly = fmin((double)zy, fmax(-(double)zy, T[0] / F[2]));
            ztot += F[2];
            zw[0] += F[2] * ((double)x[L.oPos(c)] + (double)R[0] * lx + (double)R[3] * ly);
            zw[1] += F[2] * ((double)x[L.oPos(c) + 1] + (double)R[1] * lx + (double)R[4] * ly);
        }
    }
    // The forces are held over the step, so the torque about the CoM, sum_q (p_q - c) x f_q, is tau0 - c x fsum with tau0 = sum_q p_q x f_q formed once: one cross
    // product per Runge-Kutta stage instead of eight (this one-thread-per-problem kernel is a dependent chain of float64 operations: 18 us of a tick before,
    // profiles/r04_rollout_tick_overhead.txt).
    double tau0[3] = {ext_t[0], ext_t[1], ext_t[2]}, acc[3];
    for (int q = 0; q < 8; ++q) {
        tau0[0] += cp[q][1] * cf[q][2] - cp[q][2] * cf[q][1];
        tau0[1] += cp[q][2] * cf[q][0] - cp[q][0] * cf[q][2];
        tau0[2] += cp[q][0] * cf[q][1] - cp[q][1] * cf[q][0];
    }
    for (int i = 0; i < 3; ++i) {
        if (MM && hidden) acc[i] = (fsum[i] + (double)p[L.pFext() + i]) + (double)hid[i] - (i == 2 ? (double)grav : 0.0);
        else acc[i] = fsum[i] + (double)p[L.pFext() + i] - (i == 2 ? (double)grav : 0.0);
    }
    auto deriv = [&](const double* cm, const double* vv, double* dcm, double* dv, double* dh) {
        for (int i = 0; i < 3; ++i) { dcm[i] = vv[i]; dv[i] = acc[i]; }
        dh[0] = tau0[0] - (cm[1] * fsum[2] - cm[2] * fsum[1]);
        dh[1] = tau0[1] - (cm[2] * fsum[0] - cm[0] * fsum[2]);
        dh[2] = tau0[2] - (cm[0] * fsum[1] - cm[1] * fsum[0]);
    };
    for (int s = 0; s < nsub; ++s) {
        double k1c[3], k1v[3], k1h[3], k2c[3], k2v[3], k2h[3], k3c[3], k3v[3], k3h[3], k4c[3], k4v[3], k4h[3], tc[3], tv[3];
        deriv(com, v, k1c, k1v, k1h);
        for (int i = 0; i < 3; ++i) { tc[i] = com[i] + 0.5 * h * k1c[i]; tv[i] = v[i] + 0.5 * h * k1v[i]; }
        deriv(tc, tv, k2c, k2v, k2h);
        for (int i = 0; i < 3; ++i) { tc[i] = com[i] + 0.5 * h * k2c[i]; tv[i] = v[i] + 0.5 * h * k2v[i]; }
        deriv(tc, tv, k3c, k3v, k3h);
        for (int i = 0; i < 3; ++i) { tc[i] = com[i] + h * k3c[i]; tv[i] = v[i] + h * k3v[i]; }
        deriv(tc, tv, k4c, k4v, k4h);
        for (int i = 0; i < 3; ++i) {
            com[i] += h / 6.0 * (k1c[i] + 2 * k2c[i] + 2 * k3c[i] + k4c[i]);
            v[i] += h / 6.0 * (k1v[i] + 2 * k2v[i] + 2 * k3v[i] + k4v[i]);
            hm[i] += h / 6.0 * (k1h[i] + 2 * k2h[i] + 2 * k3h[i] + k4h[i]);
        }
    }
    for (int i = 0; i < 3; ++i) {
        state_out[(size_t)b * 9 + i] = (float)com[i]; state_out[(size_t)b * 9 + 3 + i] = (float)v[i]; state_out[(size_t)b * 9 + 6 + i] = (float)hm[i];
    }
    if (zmp) {
        zmp[(size_t)b * 2] = ztot > 0.001 ? (float)(zw[0] / ztot) : nanf("");
        zmp[(size_t)b * 2 + 1] = ztot > 0.001 ? (float)(zw[1] / ztot) : nanf("");
    }
}

template <bool MM>
__global__ __launch_bounds__(256) void cmpc_plant_step_kernel(int N, int B, float grav, const float* __restrict__ corners, int corners_stride,
                                                              const float* __restrict__ X, const float* __restrict__ P,
                                                              const float* state_in, float* state_out,
                                                              float* __restrict__ zmp, float h, int nsub, float zx, float zy,
                                                              const float* __restrict__ hidden, const float* __restrict__ gain)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    plant_step_problem<MM>(N, b, grav, corners, corners_stride, X, P, state_in, state_out, zmp, h, nsub, zx, zy, hidden, gain);
}

// ---- derivatives of the plant step (include/cmpc.h, "plant-step derivatives") ----
// With the forces held the dynamics above are affine and nilpotent (dcom' = a constant, h' = tau0 - com x F), so the Runge-Kutta sweep is exact and equals
// the closed form over T = nsub h:
//     com' = com + T v + T^2/2 a,   v' = v + T a,   h' = h + T tau0 - I x F,     I = T com + T^2/2 v + T^3/6 a,
//     a = F + fExt_0 - g e_z,   F = sum_q f_q,   tau0 = tauExt_0 + sum_q cp_q x f_q,   cp_q = pos_c,0 + R_c,0 cn_q      (f_q = 0 where Gamma_c,0 is off).
// The map is bilinear in (state, pos, corners, wrench) x forces; its partials are the point values below, read ONCE by plant_partials and applied forwards by
// plant_jvp_problem and transposed, term by term in the same order, by plant_vjp_problem -- adjoint by construction.
struct PlantPartials {
    double T, F[3], I[3];      // horizon of the step, total force, time integral of the CoM
    double cp[8][3], cf[8][3]; // contact points and (gated) corner forces
    double cn[8][3];           // the corners themselves (rotation directions: d cp_q = R_c,0 (omega_c x cn_q))
    bool on[2];
    double gain, fr[8][3];     // mismatch (MM): the force gain and the gated forces as the MPC gave them, cf = gain fr
};

// MM: the partials of the mismatched plant -- the same closed form with f_q -> gain f_q and fExt_0 -> fExt_0 + fHidden, so the point values
// are taken at the gained forces and the summed wrench (tauHidden is an additive constant of tau0: no partial holds it).  hidden / gain null: as in the forward.
template <bool MM = false>
__device__ inline void plant_partials(int N, int b, float grav, const float* __restrict__ corners, int corners_stride, const float* __restrict__ X,
                                      const float* __restrict__ P, const float* __restrict__ state_in, float h, int nsub, PlantPartials& q,
                                      const float* __restrict__ hidden = nullptr, const float* __restrict__ gain = nullptr)
{
    const CmpcIdx L{N};
    const float* x = X + (size_t)b * L.nx();
    const float* p = P + (size_t)b * L.np();
    q.T = (double)nsub * (double)h;
    for (int i = 0; i < 3; ++i) q.F[i] = 0;
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c);
        q.on[c] = p[L.pGam(c)] > 0.5f;
        for (int j = 0; j < 4; ++j) {
            const float* cn = corners + (size_t)b * corners_stride + 12 * c + 3 * j;
            for (int i = 0; i < 3; ++i) {
                q.cp[4 * c + j][i] = (double)x[L.oPos(c) + i] + (double)R[i] * cn[0] + (double)R[3 + i] * cn[1] + (double)R[6 + i] * cn[2];
                const float fv = x[L.oF(c, j) + i];
                if (MM) {
                    q.fr[4 * c + j][i] = q.on[c] ? (double)fv : 0.0;
                    if (gain) q.cf[4 * c + j][i] = q.on[c] ? (double)gain[b] * (double)fv : 0.0;
                    else q.cf[4 * c + j][i] = q.on[c] ? (double)fv : 0.0;
                } else q.cf[4 * c + j][i] = q.on[c] ? (double)fv : 0.0;
                q.F[i] += q.cf[4 * c + j][i];
                q.cn[4 * c + j][i] = (double)cn[i];
            }
        }
    }
    const double T = q.T;
    if (MM) q.gain = gain ? (double)gain[b] : 1.0;
    for (int i = 0; i < 3; ++i) {
        double a;
        if (MM && hidden) a = (q.F[i] + (double)p[L.pFext() + i]) + (double)hidden[(size_t)b * 6 + i] - (i == 2 ? (double)grav : 0.0);
        else a = q.F[i] + (double)p[L.pFext() + i] - (i == 2 ? (double)grav : 0.0);
        q.I[i] = T * (double)state_in[(size_t)b * 9 + i] + 0.5 * T * T * (double)state_in[(size_t)b * 9 + 3 + i] + T * T * T / 6.0 * a;
    }
}

__device__ inline void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// forwards: (ds, dx, dp, dtheta, omega_0) -> ds'.  Null direction groups are zero.  ROT: with the rotation direction of knot 0, dir_rot[B][2][3] in the
// body-frame tangent dR_c,0 = R_c,0 [omega_c]x -- the contact points move by R_c,0 (omega_c x cn_q), so only the torque sees it.  ROT = false is the kernel
// without it, instruction for instruction.
// MM: the mismatched plant forwards ("Mismatch, forwards"), q from plant_partials<true>: d cf_q = dgain fr_q + gain df_q on a gated-on foot,
// da gains dfHidden and dtau gains dtauHidden -- plant_vjp_problem<ROT, true> transposed term by term.  dir_hidden[B][6] / dir_gain[B] double, either null =
// zero.  MM = false is the function as it was before the mismatch existed, instruction for instruction.
template <bool ROT, bool MM = false>
__device__ inline void plant_jvp_problem(int N, int b, const float* __restrict__ P, const PlantPartials& q, const double* __restrict__ dir_state,
                                         const float* __restrict__ dir_x, const float* __restrict__ dir_p, const double* __restrict__ dir_model,
                                         const double* __restrict__ dir_rot, double* __restrict__ out, const double* __restrict__ dir_hidden = nullptr,
                                         const double* __restrict__ dir_gain = nullptr)
{
    const CmpcIdx L{N};
    const float* p = P + (size_t)b * L.np();
    const double T = q.T;
    double dc[3], dv[3], dh[3], dF[3] = {0, 0, 0}, dtau[3], da[3], dI[3], t[3];
    for (int i = 0; i < 3; ++i) {
        dc[i] = dir_state[(size_t)b * 9 + i]; dv[i] = dir_state[(size_t)b * 9 + 3 + i]; dh[i] = dir_state[(size_t)b * 9 + 6 + i];
        dtau[i] = dir_p ? (double)dir_p[(size_t)b * L.np() + L.pText() + i] : 0.0;
        if (MM && dir_hidden) dtau[i] += dir_hidden[(size_t)b * 6 + 3 + i];
    }
    const double dgain = (MM && dir_gain) ? dir_gain[b] : 0.0;
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c);
        for (int j = 0; j < 4; ++j) {
            double dcp[3], df[3], wn[3];
            if (ROT) cross3(dir_rot + ((size_t)b * 2 + c) * 3, q.cn[4 * c + j], wn);
            for (int i = 0; i < 3; ++i) {
                dcp[i] = dir_x ? (double)dir_x[(size_t)b * L.nx() + L.oPos(c) + i] : 0.0;
                if (dir_model) {
                    const double* dn = dir_model + (size_t)b * CMPC_MODEL_DOUBLES + 10 + 12 * c + 3 * j;
                    dcp[i] += (double)R[i] * dn[0] + (double)R[3 + i] * dn[1] + (double)R[6 + i] * dn[2];
                }
                if (ROT) dcp[i] += (double)R[i] * wn[0] + (double)R[3 + i] * wn[1] + (double)R[6 + i] * wn[2];
                df[i] = (dir_x && q.on[c]) ? (double)dir_x[(size_t)b * L.nx() + L.oF(c, j) + i] : 0.0;
                if (MM) df[i] = q.on[c] ? dgain * q.fr[4 * c + j][i] + q.gain * df[i] : 0.0;   // d cf_q (fr is zero on a gated-off foot; so is this)
                dF[i] += df[i];
            }
            cross3(dcp, q.cf[4 * c + j], t);
            for (int i = 0; i < 3; ++i) dtau[i] += t[i];
            cross3(q.cp[4 * c + j], df, t);
            for (int i = 0; i < 3; ++i) dtau[i] += t[i];
        }
    }
    for (int i = 0; i < 3; ++i) {
        da[i] = dF[i] + (dir_p ? (double)dir_p[(size_t)b * L.np() + L.pFext() + i] : 0.0);
        if (MM && dir_hidden) da[i] += dir_hidden[(size_t)b * 6 + i];
        dI[i] = T * dc[i] + 0.5 * T * T * dv[i] + T * T * T / 6.0 * da[i];
    }
    double u[3], w[3];
    cross3(dI, q.F, u);
    cross3(q.I, dF, w);
    for (int i = 0; i < 3; ++i) {
        out[(size_t)b * 9 + i] = dc[i] + T * dv[i] + 0.5 * T * T * da[i];
        out[(size_t)b * 9 + 3 + i] = dv[i] + T * da[i];
        out[(size_t)b * 9 + 6 + i] = dh[i] + T * dtau[i] - u[i] - w[i];
    }
}

// transposed: gs' -> (gs, gx (the 30 entries it owns), gp (fExt_0, tauExt_0), gtheta (corners), gomega_0).  grad_state may alias grad_out; null outputs are
// skipped.  ROT: grad_rot[B][2][3], the transpose of the JVP's rotation term: <gcp, R (omega x cn)> = <omega, cn x R^T gcp>, summed over the foot's corners
// in corner order (a gated-off foot has gcp = 0: zeros).
// MM: grad_hidden[B][6] = the plant's own gradient on fExt_0 / tauExt_0, unrounded; grad_x on the 24 forces = gain dl/d(gain f); grad_gain[B] = sum over the
// gated-on corners, in corner order, of <dl/d(gain f_q), f_q> (both written; either may be null).
template <bool ROT, bool MM = false>
__device__ inline void plant_vjp_problem(int N, int b, const float* __restrict__ P, const PlantPartials& q, const double* grad_out, double* grad_state,
                                         float* __restrict__ grad_x, float* __restrict__ grad_p, double* __restrict__ grad_model,
                                         double* __restrict__ grad_rot, double* __restrict__ grad_hidden = nullptr, double* __restrict__ grad_gain = nullptr)
{
    const CmpcIdx L{N};
    const float* p = P + (size_t)b * L.np();
    const double T = q.T;
    double gc[3], gv[3], gh[3], gI[3], gF[3], ga[3];
    for (int i = 0; i < 3; ++i) { gc[i] = grad_out[(size_t)b * 9 + i]; gv[i] = grad_out[(size_t)b * 9 + 3 + i]; gh[i] = grad_out[(size_t)b * 9 + 6 + i]; }
    cross3(gh, q.F, gI);     // -<gh, dI x F> = <dI, gh x F>
    cross3(q.I, gh, gF);     // -<gh, I x dF> = <dF, I x gh>
    for (int i = 0; i < 3; ++i) {
        ga[i] = 0.5 * T * T * gc[i] + T * gv[i] + T * T * T / 6.0 * gI[i];
        gF[i] += ga[i];
        grad_state[(size_t)b * 9 + i] = gc[i] + T * gI[i];
        grad_state[(size_t)b * 9 + 3 + i] = T * gc[i] + gv[i] + 0.5 * T * T * gI[i];
        grad_state[(size_t)b * 9 + 6 + i] = gh[i];
        if (grad_p) { grad_p[(size_t)b * L.np() + L.pFext() + i] = (float)ga[i]; grad_p[(size_t)b * L.np() + L.pText() + i] = (float)(T * gh[i]); }
        if (MM && grad_hidden) { grad_hidden[(size_t)b * 6 + i] = ga[i]; grad_hidden[(size_t)b * 6 + 3 + i] = T * gh[i]; }
    }
    double gtau[3] = {T * gh[0], T * gh[1], T * gh[2]};
    double ggain = 0.0;
    for (int c = 0; c < 2; ++c) {
        const float* R = p + L.pR(c);
        double gpos[3] = {0, 0, 0}, grot[3] = {0, 0, 0};
        for (int j = 0; j < 4; ++j) {
            double gcp[3], gf[3];
            cross3(q.cf[4 * c + j], gtau, gcp);   // <gtau, dcp x f> = <dcp, f x gtau>
            cross3(gtau, q.cp[4 * c + j], gf);    // <gtau, cp x df> = <df, gtau x cp>
            for (int i = 0; i < 3; ++i) {
                gpos[i] += gcp[i];
                if (MM) {
                    const double ga_f = gf[i] + gF[i];   // dl / d(gain f_q)
                    if (grad_x) grad_x[(size_t)b * L.nx() + L.oF(c, j) + i] = q.on[c] ? (float)(q.gain * ga_f) : 0.f;
                    if (q.on[c]) ggain += ga_f * q.fr[4 * c + j][i];
                } else if (grad_x) grad_x[(size_t)b * L.nx() + L.oF(c, j) + i] = q.on[c] ? (float)(gf[i] + gF[i]) : 0.f;
            }
            if (grad_model)
                for (int a = 0; a < 3; ++a)   // R^T gcp: column a of R (col-major) against gcp
                    grad_model[(size_t)b * CMPC_MODEL_DOUBLES + 10 + 12 * c + 3 * j + a] = (double)R[3 * a] * gcp[0] + (double)R[3 * a + 1] * gcp[1] + (double)R[3 * a + 2] * gcp[2];
            if (ROT) {
                double rg[3], t[3];
                for (int a = 0; a < 3; ++a) rg[a] = (double)R[3 * a] * gcp[0] + (double)R[3 * a + 1] * gcp[1] + (double)R[3 * a + 2] * gcp[2];
                cross3(q.cn[4 * c + j], rg, t);
                for (int a = 0; a < 3; ++a) grot[a] += t[a];
            }
        }
        if (grad_x)
            for (int i = 0; i < 3; ++i) grad_x[(size_t)b * L.nx() + L.oPos(c) + i] = (float)gpos[i];
        if (ROT)
            for (int a = 0; a < 3; ++a) grad_rot[((size_t)b * 2 + c) * 3 + a] = grot[a];
    }
    if (grad_model)
        for (int i = 0; i < 10; ++i) grad_model[(size_t)b * CMPC_MODEL_DOUBLES + i] = 0.0;
    if (MM && grad_gain) grad_gain[b] = ggain;
}

template <bool ROT>
__global__ __launch_bounds__(256) void cmpc_plant_jvp_kernel(int N, int B, float grav, const float* __restrict__ corners, int corners_stride,
                                                             const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ state_in,
                                                             float h, int nsub, const double* __restrict__ dir_state, const float* __restrict__ dir_x,
                                                             const float* __restrict__ dir_p, const double* __restrict__ dir_model,
                                                             const double* __restrict__ dir_rot, double* __restrict__ out)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    PlantPartials q;
    plant_partials(N, b, grav, corners, corners_stride, X, P, state_in, h, nsub, q);
    plant_jvp_problem<ROT>(N, b, P, q, dir_state, dir_x, dir_p, dir_model, dir_rot, out);
}

// k columns per problem (include/cmpc.h, cmpc_plant_step_jvp_cols_device): one thread per (problem, column), the same two device functions on direction
// arrays [B][K][...] -- plant_jvp_problem indexes its directions by problem, so column j of problem b is handed over as the array moved by b (K - 1) + j
// rows: entry b of that is entry b K + j of the caller's.  ok (the tick JVP's flags; null otherwise): a problem whose word is 0 gets zeros.
// MM: the mismatched plant -- the partials at this tick's hidden row [B][6] and gain [B] (either null, as in the forward), and the directions
// dir_hidden[B][K][6] / dir_gain[B][K] double, either null = zero.  MM = false reads none of the four.
template <bool ROT, bool MM = false>
__global__ __launch_bounds__(256) void cmpc_plant_jvp_cols_kernel(int N, int B, int K, float grav, const float* __restrict__ corners, int corners_stride,
                                                                  const float* __restrict__ X, const float* __restrict__ P,
                                                                  const float* __restrict__ state_in, float h, int nsub, const double* dir_state,
                                                                  const float* __restrict__ dir_x, const float* __restrict__ dir_p,
                                                                  const double* __restrict__ dir_model, const double* __restrict__ dir_rot,
                                                                  const int* __restrict__ ok, double* out, const float* __restrict__ hidden,
                                                                  const float* __restrict__ gain, const double* __restrict__ dir_hidden,
                                                                  const double* __restrict__ dir_gain)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * K) return;
    const int b = (int)(i / K), j = (int)(i - (long long)b * K);
    const size_t col = (size_t)b * (K - 1) + j;
    if (ok && ok[b] == 0) {
        for (int e = 0; e < 9; ++e) out[((size_t)b * K + j) * 9 + e] = 0.0;
        return;
    }
    const CmpcIdx L{N};
    PlantPartials q;
    if (MM) {
        plant_partials<true>(N, b, grav, corners, corners_stride, X, P, state_in, h, nsub, q, hidden, gain);
        plant_jvp_problem<ROT, true>(N, b, P, q, dir_state + col * 9, dir_x ? dir_x + col * L.nx() : nullptr, dir_p ? dir_p + col * L.np() : nullptr,
                                     dir_model ? dir_model + col * CMPC_MODEL_DOUBLES : nullptr, ROT ? dir_rot + col * 6 : nullptr, out + col * 9,
                                     dir_hidden ? dir_hidden + col * 6 : nullptr, dir_gain ? dir_gain + col : nullptr);
        return;
    }
    plant_partials(N, b, grav, corners, corners_stride, X, P, state_in, h, nsub, q);
    plant_jvp_problem<ROT>(N, b, P, q, dir_state + col * 9, dir_x ? dir_x + col * L.nx() : nullptr, dir_p ? dir_p + col * L.np() : nullptr,
                           dir_model ? dir_model + col * CMPC_MODEL_DOUBLES : nullptr, ROT ? dir_rot + col * 6 : nullptr, out + col * 9);
}

template <bool ROT, bool MM>
__global__ __launch_bounds__(256) void cmpc_plant_vjp_kernel(int N, int B, float grav, const float* __restrict__ corners, int corners_stride,
                                                             const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ state_in,
                                                             float h, int nsub, const double* grad_out, double* grad_state, float* __restrict__ grad_x,
                                                             float* __restrict__ grad_p, double* __restrict__ grad_model, double* __restrict__ grad_rot,
                                                             const float* __restrict__ hidden, const float* __restrict__ gain,
                                                             double* __restrict__ grad_hidden, double* __restrict__ grad_gain)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    PlantPartials q;
    plant_partials<MM>(N, b, grav, corners, corners_stride, X, P, state_in, h, nsub, q, hidden, gain);
    plant_vjp_problem<ROT, MM>(N, b, P, q, grad_out, grad_state, grad_x, grad_p, grad_model, grad_rot, grad_hidden, grad_gain);
}

// ---- the kernels of a tick's derivative chains that run between the plant's and the solve's (cmpc_rollout_tick_vjp_device, cmpc_rollout_tick_jvp_device) ----
// (extern "C": the four keep the unmangled names they have in kernel traces; the enclosing namespace still keeps them out of the symbol table)
extern "C" {
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
}  // extern "C"

// ---- the warm shift (cmpc_shift_solution_device, and the front kernel of a tick below) ----
// warm start: previous solution shifted by one knot (last knot repeated); is_warm_start_enabled of
// the reference (ergoCubGazeboV1/centroidal_mpc.ini:9)
// (one problem: xp -> x0, thread tid of nt)
__device__ inline void warm_shift_problem(int N, const float* __restrict__ xp, float* __restrict__ x0, int tid, int nt)
{
    CmpcLayout L;
    cmpc_layout_init(L, N);
    for (int e = tid; e < L.nx; e += nt) {
        // every block of x is 3 x (N+1) or 3 x N, column = knot: find block start and length
        int start, len;
        if (e < L.o_pos[0]) { start = (e / (3 * (N + 1))) * 3 * (N + 1); len = 3 * (N + 1); }
        else {
            const int c = e < L.o_pos[1] ? 0 : 1, e2 = e - L.o_pos[c];
            if (e2 < 3 * (N + 1)) { start = L.o_pos[c]; len = 3 * (N + 1); }
            else { start = L.o_pos[c] + 3 * (N + 1) + ((e2 - 3 * (N + 1)) / (3 * N)) * 3 * N; len = 3 * N; }
        }
        const int off = e - start;
        const int src = off + 3 < len ? e + 3 : e;  // shift by one knot, repeat the last
        x0[e] = xp[src];
    }
}
__global__ __launch_bounds__(256) void cmpc_warm_shift_kernel(int N, int B, const float* __restrict__ Xp, float* __restrict__ X0)
{
    CmpcLayout L;
    cmpc_layout_init(L, N);
    const int b = blockIdx.x;
    warm_shift_problem(N, Xp + (size_t)b * L.nx, X0 + (size_t)b * L.nx, threadIdx.x, 256);
}

// ---- the two ends of a roll-out tick as ONE launch each (cmpc_rollout_tick_device).  At B <= 256 a tick is a 0.66 ms solve between nine launches of a
// few microseconds of work each, and the dispatch of a kernel behind another costs as much as they do (tools/gpu_rollout_tick_overhead.py): the steps in
// front of the solve touch disjoint entries of P and X0 (contact blocks / state rows / the shifted solution) and so do the two behind it (the lists' poses /
// the state), so each group is one grid whose threads call the SAME per-problem functions as the single kernels -- results identical to the last bit
// (tests/test_gpu_rollout.py).
// pre: one workgroup per problem.  All threads: setState and the warm-start shift; threads 0, 1: merge (updateContactPhaseList) of foot 0 / 1; then one thread per
// (foot, stage): sampling (setContactPhaseList) of the merged lists; threads 0, 1: the landing knots.
// snap_dt_ns > 0 (cmpc_tick_io.force_sample_time): forceSampleTime first -- one thread per list entry (cmpc_snap_contact) on the planner's lists staged in LDS
// (merge ticks) or on the caller's lists (first tick, written back), behind a barrier.  Lists longer than the LDS stage were snapped by
// cmpc_force_sample_time_kernel before this launch: snap_ok[2B] then holds its per-foot status words.  A foot whose snap fails is treated as an empty list:
// its list is emptied, land = -2, ok = 0.
// RF: the refill walk (cmpc_rollout_walk_refill_device), always launched as a merge tick with M <= 16.  The workgroup reads its slot's start tick once: its time
// is its own, now = (tick - start[b]) dt, its wrench row is row tick - start[b] of its trial, and with start[b] == tick this is the problem's FIRST tick -- no
// merge, its lists are the planner's (staged in LDS, snapped there with forceSampleTime) and go out as a merge tick writes them, ok = the snap's status (1
// without), and x0 is the cold start, written behind the barrier after the sampling.  false is the kernel without any of it.
// TR (with RF; cmpc_rollout_walk_refill_trials_device): the per-trial data `tr` -- on its first tick the workgroup writes its slot's record of the handle's
// per-problem table, the base record word for word and then, by one thread behind a barrier (taken by the whole workgroup: `fresh`, the trial and the
// pointer are workgroup-uniform), trial q's model over it (cmpc_refill_trial_model: the statement of cmpc_set_models_device's kernel); the solve and the back
// kernel of this tick are later launches on the stream.  The noise row is row [local tick][q] inside its range -- the same float32 add -- else the plain
// copy.  false is the kernel without any of it: `tr` is not read.
// rf.offset > 0 (trials from a snapshot): a slot spawned at s runs tick t at local tick offset + (t - s) -- one integer sum, converted once -- and its spawn
// tick is NOT a first tick: an ordinary warm merge tick on the lists and the solution the restore launch put there.  What the trial owns -- its wrench and
// noise rows, the model write at its spawn tick -- stays indexed by r = t - s.  With offset 0 every expression is the one it was.
struct CmpcRefillTick {
    const int* start; const int* trial;     // [B]: the slots' start ticks and trials (cmpc_walk_refill)
    int tick;
    int offset;                             // trials from a snapshot (cmpc_walk_refill_snapshot): the pool's tick t_s, the local tick at spawn; else 0
    const float* wrench_trials; int wrench_ticks, trials;   // [wrench_ticks][trials][N][6] or null
    double plan_t_first;
    float g8;                               // the cold start's f_z
};
// local time of a refilled slot and its offset into the planner's trajectories: the host's two roundings, (double)ticks * dt and then the difference
__device__ inline void refill_local_time(int ticks, double dt, double t_first, double* now, double* offset)
{
#pragma clang fp contract(off)
    const double t = (double)ticks * dt;
    *now = t;
    *offset = t - t_first;
}
template <bool RF, bool TR = false>
__global__ __launch_bounds__(256) void cmpc_tick_pre_kernel(int B, int N, int M, double dt, double now, int merge, const double* plan_t, const float* plan_pose,
                                                            const int* plan_n, const double* prev_t, const float* prev_pose, const int* prev_n, double* list_t,
                                                            float* list_pose, int* list_n, int* ok, int* land, const float* __restrict__ box,
                                                            const float* __restrict__ state, const float* __restrict__ wrench, float* P,
                                                            const float* __restrict__ Xprev, float* __restrict__ X0, const float* __restrict__ plan_com,
                                                            const float* __restrict__ plan_h, int plan_knots, double plan_dt, double plan_t_offset,
                                                            double robot_mass, double com_height, long long snap_dt_ns, const int* __restrict__ snap_ok,
                                                            const int* __restrict__ ended, const float* __restrict__ noise, CmpcRefillTick rf,
                                                            CmpcRefillTrialArgs tr)
{
    static_assert(RF || !TR, "the per-trial data belongs to a refill walk");
    const int b = blockIdx.x, tid = threadIdx.x;
    if (ended && ended[b] >= 0) return;   // (cmpc_set_ended_device: the whole workgroup, ahead of its first barrier -- nothing of the problem is written)
    const CmpcIdx L{N};
    float* p = P + (size_t)b * L.np();
    bool fresh = false;                   // (RF: workgroup-uniform, from one scalar load)
    const float* wrench_b = nullptr;      // (RF: the wrench row of this slot's trial, [N][6])
    const float* noise_q = nullptr;       // (TR: the noise row of this slot's trial at its local tick, [9])
    int model_q = -1;                     // (TR: the trial whose model the slot takes on this tick, its first)
    if constexpr (RF) {
        const int local = rf.tick - rf.start[b], q = rf.trial[b];
        fresh = local == 0 && rf.offset == 0;
        refill_local_time(rf.offset + local, dt, rf.plan_t_first, &now, &plan_t_offset);
        if (rf.wrench_trials && local >= 0 && local < rf.wrench_ticks && q >= 0 && q < rf.trials)
            wrench_b = rf.wrench_trials + ((size_t)local * rf.trials + q) * N * 6;
        if (fresh) merge = 0;
        if constexpr (TR) {
            if (tr.noise && local >= 0 && local < tr.noise_ticks && q >= 0 && q < tr.Q) noise_q = tr.noise + ((size_t)local * tr.Q + q) * 9;
            if (tr.models && local == 0 && q >= 0 && q < tr.Q) model_q = q;
        }
    }
    __shared__ int okw;
    __shared__ int foot_ok[2];   // forceSampleTime status of the two feet (1 when the flag is off)
    if (tid == 0) okw = 1;
    if (tid < 2) foot_ok[tid] = snap_ok ? snap_ok[2 * b + tid] : 1;
    __syncthreads();
    // setState and the warm-start shift first (they depend on nothing the kernel computes: their memory traffic runs under the merge of threads 0, 1)
    // (noise: this tick's row [B][9] of cmpc_plant_mismatch.dStateNoise or null -- the MPC measures state + noise, one float32 add; the plant keeps the state)
    if (TR && noise_q) for (int e = tid; e < 9; e += 256) p[L.pCom0() + e] = state[9 * (size_t)b + e] + noise_q[e];
    else if (noise) for (int e = tid; e < 9; e += 256) p[L.pCom0() + e] = state[9 * (size_t)b + e] + noise[9 * (size_t)b + e];
    else for (int e = tid; e < 9; e += 256) p[L.pCom0() + e] = state[9 * (size_t)b + e];
    if constexpr (TR) {
        if (model_q >= 0) {   // (uniform)
            const int* src = reinterpret_cast<const int*>(tr.base);
            int* dst = reinterpret_cast<int*>(tr.table + b);
            for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += 256) dst[e] = src[e];
            __syncthreads();   // (the copy is in the record before the model goes over it)
            if (tid == 64) cmpc_refill_trial_model(tr, model_q, tr.table[b]);
        }
    }
    if constexpr (RF) {
        if (wrench_b)
            for (int e = tid; e < 3 * N; e += 256) {
                const int k = e / 3, i = e % 3;
                p[L.pFext() + e] = wrench_b[k * 6 + i];
                p[L.pText() + e] = wrench_b[k * 6 + 3 + i];
            }
    } else if (wrench)
        for (int e = tid; e < 3 * N; e += 256) {
            const int k = e / 3, i = e % 3;
            p[L.pFext() + e] = wrench[((size_t)b * N + k) * 6 + i];
            p[L.pText() + e] = wrench[((size_t)b * N + k) * 6 + 3 + i];
        }
    if (Xprev && !fresh) warm_shift_problem(N, Xprev + (size_t)b * L.nx(), X0 + (size_t)b * L.nx(), tid, 256);
    if (plan_com)   // setReferenceTrajectory from the planner's trajectories (8f-3), one thread per knot, from the far end of the workgroup
        for (int k = 255 - tid; k <= N; k += 256)
            cmpc_resample_reference_knot(plan_com + (size_t)b * plan_knots * 3, plan_h + (size_t)b * plan_knots * 3, plan_knots, plan_dt, plan_t_offset, dt, k,
                                         robot_mass, com_height, p + L.pComref() + 3 * k, p + L.pHref() + 3 * k);
    // the merge scans its lists entry by entry: from LDS (the workgroup fetches both feet's lists of the planner and of the previous tick in one round trip) when they
    // fit, else from global memory as the single kernel does -- the same function on the same values either way
    constexpr int MS = 16;
    __shared__ double st_[2][2 * 2 * MS];      // [planner | previous][foot][M][2]
    __shared__ float sp_[2][2 * 7 * MS];
    const bool staged = merge && M <= MS;
    if (staged) {
        const size_t o2 = (size_t)(2 * b) * M;
        for (int e = tid; e < 4 * M; e += 256) { st_[0][e] = plan_t[2 * o2 + e]; st_[1][e] = prev_t[2 * o2 + e]; }
        for (int e = tid; e < 14 * M; e += 256) { sp_[0][e] = plan_pose[7 * o2 + e]; sp_[1][e] = prev_pose[7 * o2 + e]; }
        __syncthreads();
        if (snap_dt_ns > 0) {   // forceSampleTime on the staged planner lists ([foot][M][2]: entry e = foot * M + contact); the merge then reads them snapped
            for (int e = tid; e < 2 * M; e += 256) {
                const int c = e / M, pn = plan_n[2 * b + c];
                if (pn >= 0 && pn <= M && e - c * M < pn && !cmpc_snap_contact(st_[0] + 2 * e, snap_dt_ns, st_[0] + 2 * e)) atomicAnd(&foot_ok[c], 0);
            }
            __syncthreads();
        }
    }
    // this tick's lists live in LDS too (so_*): the merge writes them there, the sampling threads scan them there, and the workgroup copies them out
    __shared__ double so_t[2 * 2 * MS];
    __shared__ float so_p[2 * 7 * MS];
    __shared__ int so_n[2];
    const bool lstaged = M <= MS;
    const size_t ob = (size_t)(2 * b) * M;
    if (lstaged && !merge) {   // (first tick: the caller filled the lists; RF: they are the planner's)
        const double* const first_t = RF ? plan_t : list_t;
        const float* const first_p = RF ? plan_pose : list_pose;
        const int* const first_n = RF ? plan_n : list_n;
        for (int e = tid; e < 4 * M; e += 256) so_t[e] = first_t[2 * ob + e];
        for (int e = tid; e < 14 * M; e += 256) so_p[e] = first_p[7 * ob + e];
        if (tid < 2) so_n[tid] = first_n[2 * b + tid];
        if (snap_dt_ns > 0) {   // forceSampleTime on the caller's lists, written back: what the reference passes on (contactPhaseList = mannContactPhaseList)
            __syncthreads();
            for (int e = tid; e < 2 * M; e += 256) {
                const int c = e / M, m = e - c * M, n = so_n[c];
                if (n < 0 || n > M) { if (m == 0) atomicAnd(&foot_ok[c], 0); continue; }
                if (m >= n) continue;
                if (!cmpc_snap_contact(so_t + 2 * e, snap_dt_ns, so_t + 2 * e)) atomicAnd(&foot_ok[c], 0);
                if constexpr (RF) continue;   // (the whole list goes out below)
                list_t[2 * ob + 2 * e] = so_t[2 * e]; list_t[2 * ob + 2 * e + 1] = so_t[2 * e + 1];
            }
            __syncthreads();
        }
    }
    if (tid < 2 && !merge && !foot_ok[tid]) {   // (first tick, a failed snap: the foot's list is empty from here on)
        if (lstaged) so_n[tid] = 0;
        list_n[2 * b + tid] = 0;
    }
    if (tid < 2 && merge) {
        const int e = 2 * b + tid;
        const size_t o = (size_t)e * M;
        const int pn = plan_n[e], mn = prev_n[e];
        const bool sane = pn >= 0 && pn <= M && mn >= 0 && mn <= M;
        int* on = lstaged ? &so_n[tid] : list_n + e;
        const bool snapped = foot_ok[tid] != 0;
        if (!sane || !snapped) *on = 0;
        const double* pt = staged ? st_[0] + 2 * M * tid : plan_t + 2 * o;
        const double* mt = staged ? st_[1] + 2 * M * tid : prev_t + 2 * o;
        const float* pq = staged ? sp_[0] + 7 * M * tid : plan_pose + 7 * o;
        const float* mq = staged ? sp_[1] + 7 * M * tid : prev_pose + 7 * o;
        const bool good = sane && snapped && cmpc_merge_foot(now, pt, pq, pn, mt, mq, mn, M, lstaged ? so_t + 2 * M * tid : list_t + 2 * o,
                                                  lstaged ? so_p + 7 * M * tid : list_pose + 7 * o, on);
        if (!good) atomicAnd(&okw, 0);
    }
    __syncthreads();   // (the merged lists of the two feet are visible to the workgroup: in LDS, or in global memory when they do not fit)
    if (lstaged && (merge || RF)) {   // out to global memory, the entries in use (what the single merge kernel writes)
        for (int e = tid; e < 4 * M; e += 256) { const int c = e / (2 * M); if (e - c * 2 * M < 2 * so_n[c]) list_t[2 * ob + e] = so_t[e]; }
        for (int e = tid; e < 14 * M; e += 256) { const int c = e / (7 * M); if (e - c * 7 * M < 7 * so_n[c]) list_pose[7 * ob + e] = so_p[e]; }
        if (tid < 2) list_n[2 * b + tid] = so_n[tid];
    }
    // sampling: one thread per (foot, stage) -- a single thread walking the N stages of a foot one global-memory round trip at a time was 33 of this kernel's
    // 39 us (rocprofv3, profiles/r04_rollout_tick_overhead.txt); the landing knot then comes from the stages' contact flags in LDS
    __shared__ unsigned char acts[2][CMPC_NMAX];
    for (int e2 = tid; e2 < 2 * N; e2 += 256) {
        const int cft = e2 / N, k = e2 - cft * N, e = 2 * b + cft;
        const size_t o = (size_t)e * M;
        const int n = lstaged ? so_n[cft] : list_n[e];
        if (n >= 1 && n <= M)
            acts[cft][k] = cmpc_sample_stage(N, dt, now, cft, k, lstaged ? so_t + 2 * M * cft : list_t + 2 * o, lstaged ? so_p + 7 * M * cft : list_pose + 7 * o, n, box,
                                             box + 6, p) ? 1 : 0;
    }
    __syncthreads();
    if (tid < 2) {
        const int e = 2 * b + tid, n = lstaged ? so_n[tid] : list_n[e];
        land[e] = (n < 1 || n > M) ? -2 : cmpc_landing_knot(N, [&](int k) { return acts[tid][k] != 0; });
    }
    if ((merge || snap_dt_ns > 0 || RF) && ok && tid == 0) ok[b] = okw && foot_ok[0] && foot_ok[1];
    if constexpr (RF) {   // (the barrier above: the state rows and the sampling's nominal positions of p are the workgroup's to read)
        if (fresh) {
            float* x0 = X0 + (size_t)b * L.nx();
            for (int e = tid; e < L.nx(); e += 256) x0[e] = cmpc_cold_start_entry(N, e, p, rf.g8);
        }
    }
}

// post: one thread per problem -- the plant step, then the step adjustment of its two feet (getOutput().contactPhaseList)
// MM: the mismatched plant (this tick's hidden-wrench row and the force gain, plant_step_problem); false is the kernel without it
// RF: the refill walk -- the step adjustment looks for the next contact at the problem's own time (tick - start[b]) dt
// MM and RF (cmpc_rollout_walk_refill_trials_device): hidden [hidden_ticks][trials][6] and gain [trials] are per TRIAL -- the lane takes row [local
// tick][trial[b]] inside the schedule's range, else none (the term is then not added: a select per lane, no add of zero), and its trial's gain
// offset (RF; trials from a snapshot, else 0): the problem's time is (offset + tick - start[b]) dt; the schedule's row stays tick - start[b]
template <bool MM, bool RF>
__global__ __launch_bounds__(256) void cmpc_tick_post_kernel(int B, int N, int M, double now, float grav, const float* __restrict__ corners, int corners_stride,
                                                             const float* __restrict__ X, const float* __restrict__ P, const float* state_in, float* state_out,
                                                             float* __restrict__ zmp, float h, int nsub, float zx, float zy, const int* __restrict__ land,
                                                             const double* __restrict__ t, float* __restrict__ pose, const int* __restrict__ n,
                                                             const int* __restrict__ ended, const float* __restrict__ hidden,
                                                             const float* __restrict__ gain, const int* __restrict__ start, int tick, double dt,
                                                             const int* __restrict__ trial, int hidden_ticks, int trials, int offset)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    if (ended && ended[b] >= 0) return;   // (cmpc_set_ended_device; per lane, as the line above: nothing behind it needs the whole wave)
    if constexpr (RF) {
        double unused;
        refill_local_time(offset + (tick - start[b]), dt, 0.0, &now, &unused);
        if constexpr (MM) {
            const int local = tick - start[b], q = trial[b];
            const bool known = q >= 0 && q < trials;
            hidden = (hidden && known && local >= 0 && local < hidden_ticks) ? hidden + ((size_t)local * trials + q) * 6 : nullptr;
            gain = (gain && known) ? gain + q : nullptr;
        }
    }
    plant_step_problem<MM, MM && RF>(N, b, grav, corners, corners_stride, X, P, state_in, state_out, zmp, h, nsub, zx, zy, hidden, gain);
    const CmpcIdx L{N};
    for (int c = 0; c < 2; ++c) {
        const int e = 2 * b + c, lk = land[e];
        if (lk < 0 || lk > N || n[e] < 1 || n[e] > M) continue;
        const size_t o = (size_t)e * M;
        const int nx = cmpc_next_contact(t + 2 * o, n[e], now);
        if (nx < 0) continue;
        const float* x = X + (size_t)b * L.nx() + L.oPos(c) + 3 * lk;
        for (int i = 0; i < 3; ++i) pose[7 * (o + nx) + i] = x[i];
    }
}

// ---- the walk (cmpc_rollout_walk_device): the record behind a tick, the outcome arrays at their start, and the cold start in front of a first solve ----
// record: one thread per problem (cmpc_record_problem, the host form's function).  The statistics row: every lane holds its problem's five terms (zeros, the
// identity of the sums and of the max of non-negative counts, for lanes past B and for ended problems), the wave reduces them by butterflies -- all 256 threads
// reach the shuffles: no lane leaves before them -- and lane 0 adds its wave's terms to the row, one integer atomic per non-zero word.
// LIM (cmpc_set_walk_limits): the measures, the codes 6..9 and the sixth word of the row -- the problems whose code is 6..9 -- through the same reduction and
// one more atomic; lm.measures is the tick's row.  LIM = false is the kernel without limits, and lm is not read.
template <bool LIM>
__global__ __launch_bounds__(256) void cmpc_rollout_record_kernel(CmpcRecordArgs a, int* __restrict__ stats, CmpcLimitArgs lm)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    int t[LIM ? 6 : 5] = {0, 0, 0, 0, 0};
    if (b < a.B) cmpc_record_problem<LIM>(a, lm, b, t);
    if (!stats) return;   // (uniform)
    for (int o = warpSize / 2; o > 0; o >>= 1) {
        t[0] += __shfl_xor(t[0], o);
        t[1] += __shfl_xor(t[1], o);
        t[2] += __shfl_xor(t[2], o);
        t[3] = max(t[3], __shfl_xor(t[3], o));
        t[4] += __shfl_xor(t[4], o);
        if (LIM) t[5] += __shfl_xor(t[5], o);
    }
    if ((threadIdx.x & (warpSize - 1)) == 0) {
        if (t[0]) atomicAdd(stats + 0, t[0]);
        if (t[1]) atomicAdd(stats + 1, t[1]);
        if (t[2]) atomicAdd(stats + 2, t[2]);
        if (t[3]) atomicMax(stats + 3, t[3]);
        if (t[4]) atomicAdd(stats + 4, t[4]);
        if (LIM && t[5]) atomicAdd(stats + 5, t[5]);
    }
}

__global__ __launch_bounds__(256) void cmpc_extremes_init_kernel(int B, float* __restrict__ ext)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float inf = __builtin_inff();
    float* e = ext + 5 * (size_t)b;
    e[0] = inf; e[1] = -inf; e[2] = -inf; e[3] = inf; e[4] = -inf;
}

// the measures differentiated (include/cmpc.h, cmpc_walk_measures_vjp_device and its two companions): one thread per (row, problem) -- per (row,
// problem) or (problem, corner word) in the fold -- running the host forms' own functions (cmpc_contacts.h).  No LDS, no barrier, no atomics: a thread
// owns every word it writes, and lanes past the work touch no memory.
__global__ __launch_bounds__(256) void cmpc_walk_measures_vjp_kernel(CmpcMeasureVjpArgs v)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)v.rows * v.B) return;
    cmpc_walk_measures_vjp_entry(v, (int)(e / v.B), (int)(e % v.B));
}

__global__ __launch_bounds__(256) void cmpc_walk_measures_fold_kernel(int N, int B, int rows, const double* __restrict__ direct, float* __restrict__ grad_p,
                                                                      double* __restrict__ grad_model)
{
    cmpc_walk_measures_fold_entry(N, B, rows, direct, grad_p, grad_model, (size_t)blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void cmpc_walk_measures_jvp_kernel(CmpcMeasureJvpArgs v)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)v.rows * v.B) return;
    cmpc_walk_measures_jvp_entry(v, (int)(e / v.B), (int)(e % v.B));
}

// ---- the wrench sensor (include/cmpc.h, cmpc_wrench_sensor): one thread per (row, problem, knot) of the forward and the tangent, one per output element of
// the transpose; the rule is cmpc_contacts.h's, the host forms run the same functions.  No LDS, no atomics. ----
__global__ __launch_bounds__(256) void cmpc_wrench_sense_kernel(CmpcSenseArgs a, int knots, float* __restrict__ wrench_rows, float* __restrict__ plant_rows,
                                                                int* __restrict__ pass_rows)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.rows * a.B * knots) return;
    const size_t rb = e / knots;
    cmpc_wrench_sense_entry(a, wrench_rows, plant_rows, pass_rows, (int)(rb / a.B), (int)(rb % a.B), (int)(e % knots));
}

__global__ __launch_bounds__(256) void cmpc_wrench_sense_vjp_kernel(CmpcSenseVjpArgs v, int out_rows)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)out_rows * v.s.B * 6) return;
    const size_t rb = e / 6;
    cmpc_wrench_sense_vjp_entry(v, (int)(rb / v.s.B), (int)(rb % v.s.B), (int)(e % 6));
}

__global__ __launch_bounds__(256) void cmpc_wrench_sense_jvp_kernel(CmpcSenseJvpArgs v)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)v.s.rows * v.s.B * v.K * v.s.N) return;
    const size_t col = e / v.s.N, rb = col / v.K;
    cmpc_wrench_sense_jvp_entry(v, (int)(rb / v.s.B), (int)(rb % v.s.B), (int)(col % v.K), (int)(e % v.s.N));
}

__global__ __launch_bounds__(256) void cmpc_outcome_init_kernel(int B, const float* __restrict__ state0, int* __restrict__ end_tick, int* __restrict__ end_code,
                                                                int* __restrict__ it_sum, int* __restrict__ it_max, float* __restrict__ final_state,
                                                                float* __restrict__ slack_min)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    end_tick[b] = -1; end_code[b] = 0; it_sum[b] = 0; it_max[b] = 0;
    for (int i = 0; i < 9; ++i) final_state[9 * (size_t)b + i] = state0[9 * (size_t)b + i];
    slack_min[b] = __builtin_inff();
}

// refill (cmpc_rollout_refill_device): ONE workgroup walks the slots in chunks of 256, so that the assignment does not depend on scheduling -- no atomic on the
// counter.  Per chunk: every lane archives its slot and learns whether it is free; a wave64 ballot gives the lane its rank among its wave's free slots, the four
// wave totals go through LDS, and the running base (the queue's counter, read once) is carried from chunk to chunk: free slots take trials base, base + 1, ...
// in ascending slot order.  Every thread reaches the ballot and both barriers of every chunk (lanes past B hold `not free`).  Only this workgroup touches *next.
__global__ __launch_bounds__(256) void cmpc_refill_kernel(CmpcRefillArgs a, int* __restrict__ next)
{
    __shared__ int wave_free[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = a.state_live ? min(max(*next, 0), a.Q) : 0;
    for (int c0 = 0; c0 < a.B; c0 += 256) {
        const int b = c0 + tid;
        const bool is_free = b < a.B && cmpc_refill_archive(a, b);
        const unsigned long long m = __ballot(is_free);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_free[w] = __popcll(m);
        __syncthreads();
        int ahead = 0, total = 0;
        for (int i = 0; i < 4; ++i) {
            const int t = wave_free[i];
            ahead += i < w ? t : 0;
            total += t;
        }
        if (a.state_live && b < a.B) {
            if (is_free) cmpc_refill_assign(a, b, min(base + ahead + rank, a.Q));
            if (a.trial_of) a.trial_of[b] = a.trial[b];
        }
        base = min(base + total, a.Q);
        __syncthreads();   // (wave_free is the next chunk's)
    }
    if (a.state_live && tid == 0) *next = base;
}

// the slots and the queue at their start: every slot empty, every trial not started with the outcome cmpc_outcome_init_kernel gives it, the counter 0
__global__ __launch_bounds__(256) void cmpc_refill_init_kernel(CmpcRefillArgs a, int* __restrict__ next)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e == 0) *next = 0;
    if (e < a.B) { a.start[e] = 0; a.trial[e] = -1; }
    if (e < a.Q) {
        a.q_end_tick[e] = -1; a.q_end_code[e] = 0; a.q_it_sum[e] = 0; a.q_it_max[e] = 0;
        for (int i = 0; i < 9; ++i) a.q_final_state[9 * (size_t)e + i] = a.state0[9 * (size_t)e + i];
        a.q_slack_min[e] = __builtin_inff();
        a.q_ticks[e] = 0; a.q_slot[e] = -1; a.q_start[e] = -1;
    }
}

// cold start: one workgroup per problem, one thread per entry of x (cmpc_cold_start_entry)
__global__ __launch_bounds__(256) void cmpc_cold_start_kernel(int N, float g8, const float* __restrict__ P, float* __restrict__ X0,
                                                              const int* __restrict__ ended)
{
    if (ended && ended[blockIdx.x] >= 0) return;   // (cmpc_set_ended_device)
    const CmpcIdx L{N};
    const float* p = P + (size_t)blockIdx.x * L.np();
    float* x = X0 + (size_t)blockIdx.x * L.nx();
    for (int e = threadIdx.x; e < L.nx(); e += 256) x[e] = cmpc_cold_start_entry(N, e, p, g8);
}

// ---- the device tape (cmpc_rollout_tape_device) and the gate of the reverse walk (cmpc_rollout_walk_vjp_device) ----
// tape: bit copies, grid-stride, one array after the other (every thread walks every array: the arrays are rows of one batch, coalesced).  No barrier.
template <typename T>
__device__ inline void tape_copy(T* __restrict__ dst, const T* __restrict__ src, size_t n, size_t tid, size_t stride)
{
    for (size_t e = tid; e < n; e += stride) dst[e] = src[e];
}
__global__ __launch_bounds__(256) void cmpc_rollout_tape_kernel(CmpcTapeArgs a)
{
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const size_t B = (size_t)a.B, r = (size_t)a.row;
    if (a.parts & 1) tape_copy(a.t_states + r * B * 9, a.state_in, B * 9, tid, stride);
    if (!(a.parts & 2)) return;   // (uniform)
    tape_copy(a.t_X + r * B * a.nx, a.X, B * a.nx, tid, stride);
    tape_copy(a.t_P + r * B * a.np, a.P, B * a.np, tid, stride);
    tape_copy(a.t_info + r * B * CMPC_INFO_N, a.info, B * CMPC_INFO_N, tid, stride);
    tape_copy(a.t_states + (r + 1) * B * 9, a.state_out, B * 9, tid, stride);
    tape_copy(a.t_land + r * B * 2, a.land, B * 2, tid, stride);
    if (a.ok) tape_copy(a.t_ok + r * B, a.ok, B, tid, stride);
    else for (size_t e = tid; e < B; e += stride) a.t_ok[r * B + e] = 1;   // (a first tick without force_sample_time leaves dOk alone: every merge good)
    const size_t nt = B * 4 * a.M;
    if (a.plan_t) tape_copy(a.t_plan_t + r * nt, a.plan_t, nt, tid, stride);
    if (a.plan_n) tape_copy(a.t_plan_n + r * B * 2, a.plan_n, B * 2, tid, stride);
    tape_copy(a.t_list_t + r * nt, a.list_t, nt, tid, stride);
    tape_copy(a.t_list_n + r * B * 2, a.list_n, B * 2, tid, stride);
}

// snapshot (cmpc_rollout_snapshot_device): one workgroup per destination problem, so the source index is one uniform read per row and every array's row
// of that problem is a contiguous piece.  Rows of 64 words and more (x, p, x0, the lists' times and poses from M = 2 on) go as 16-byte pieces aligned on the
// DESTINATION: n_x and n_p are not multiples of four floats at every N, so a row starts 0 .. 3 words short of a 16-byte line -- those words and the tail
// go one by one.  The source row sits at another problem's offset and need not share the alignment: its 16-byte loads are declared 4-byte aligned.
// Bandwidth-bound (13 KB in, 13 KB out per problem): no LDS, no barrier, no atomics.
typedef unsigned snap_u32x4 __attribute__((ext_vector_type(4)));
typedef snap_u32x4 snap_u32x4_a4 __attribute__((aligned(4)));
__device__ inline void snap_row(unsigned* __restrict__ d, const unsigned* __restrict__ s, int w, int tid)
{
    if (w < 64) {
        for (int e = tid; e < w; e += 256) d[e] = s[e];
        return;
    }
    const int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2);   // words in front of the first aligned line
    const int nv = (w - head) >> 2, tail0 = head + 4 * nv;
    if (tid < head) d[tid] = s[tid];
    snap_u32x4* dv = reinterpret_cast<snap_u32x4*>(d + head);
    const snap_u32x4_a4* sv = reinterpret_cast<const snap_u32x4_a4*>(s + head);
    for (int e = tid; e < nv; e += 256) dv[e] = sv[e];
    if (tid < w - tail0) d[tail0 + tid] = s[tail0 + tid];
}
__global__ __launch_bounds__(256) void cmpc_rollout_snapshot_kernel(CmpcSnapshotArgs a)
{
    const int b = blockIdx.x;   // (the grid is B workgroups: nothing runs past B)
    const int s = cmpc_snapshot_source(a, b);
    if (a.ok && threadIdx.x == 0) a.ok[b] = s >= 0 ? 1 : 0;
    if (s < 0) return;          // (uniform) a bad index: the problem stays unwritten
    for (int i = 0; i < a.count; ++i) {
        const size_t w = (size_t)a.words[i];
        snap_row(a.dst[i] + w * b, a.src[i] + w * s, a.words[i], threadIdx.x);
    }
}

// restore (cmpc_rollout_walk_refill_snapshot_device): one workgroup per slot, between the refill launch and the front kernel of a tick.  The gate comes ahead
// of everything and is workgroup-uniform -- blockIdx and kernel arguments only: a slot that was not spawned this tick costs its workgroup one scalar load.
// A spawned slot receives its trial's pool row through the snapshot kernel's row copy (snap_row); an index outside the pool ends the slot at spawn.  The
// flag and the two outcome words are one thread's; on the copy path the outcome words are rows of the table.  No LDS, no barrier, no atomics.
__global__ __launch_bounds__(256) void cmpc_refill_restore_kernel(CmpcRefillRestoreArgs a)
{
    const int b = blockIdx.x;   // (the grid is B workgroups)
    const int q = cmpc_refill_restore_trial(a, b);
    if (q < 0) return;          // (uniform)
    const int s = cmpc_refill_restore_source(a, q);
    if (a.ok && threadIdx.x == 0) a.ok[q] = s >= 0 ? 1 : 0;
    if (s < 0) {                // (uniform)
        if (threadIdx.x == 0) { a.end_tick[b] = a.pool_tick; a.end_code[b] = 0; }
        return;
    }
    for (int i = 0; i < a.copy.count; ++i) {
        const size_t w = (size_t)a.copy.words[i];
        snap_row(a.copy.dst[i] + w * b, a.copy.src[i] + w * s, a.copy.words[i], threadIdx.x);
    }
}

// plan select (cmpc_rollout_walk_refill_plans_device): one workgroup per slot, between the refill launch and the front kernel of a tick.  The gate is the
// restore kernel's -- blockIdx and kernel arguments only, ahead of everything: a slot that was not spawned this tick costs its workgroup one scalar load.
// A spawned slot receives its trial's pool row of the planner's lists (8 M, 14 M and 2 words) and, when the pool has them, of the two planner
// trajectories (3 plan_knots words each) through the snapshot kernel's row copy (snap_row); an index outside the pool ends the slot at spawn, local tick 0.
// The flag and the two outcome words are one thread's.  No LDS, no barrier, no atomics.
__global__ __launch_bounds__(256) void cmpc_refill_plans_kernel(CmpcRefillPlansArgs a)
{
    const int b = blockIdx.x;   // (the grid is B workgroups)
    const int q = cmpc_refill_plans_trial(a, b);
    if (q < 0) return;          // (uniform)
    const int s = cmpc_refill_plans_source(a, q);
    if (a.ok && threadIdx.x == 0) a.ok[q] = s >= 0 ? 1 : 0;
    if (s < 0) {                // (uniform)
        if (threadIdx.x == 0) { a.end_tick[b] = 0; a.end_code[b] = 0; }
        return;
    }
    for (int i = 0; i < a.count; ++i) {
        const size_t w = (size_t)a.words[i];
        snap_row(a.dst[i] + w * b, a.src[i] + w * s, a.words[i], threadIdx.x);
    }
}

// plan fold (cmpc_rollout_plan_fold_device): one thread per entry [p][w] of the pool's gradient, which walks the queue in ascending q and adds the rows of
// its members (cmpc_plan_fold_entry: a select per trial).  Neighbouring threads read neighbouring words of a trial's row; the index word is the same for a
// whole row of the output.  The order is the loop's: no LDS, no barrier, no atomics.
__global__ __launch_bounds__(256) void cmpc_plan_fold_kernel(int Q, int words, const int* __restrict__ index, const double* __restrict__ per, int pool_rows,
                                                             double* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)pool_rows * words) return;
    out[e] = cmpc_plan_fold_entry(Q, words, index, per, (int)(e / words), (int)(e % words));
}

// regroup (cmpc_rollout_tape_regroup_device): one workgroup per (destination row, destination column) of a tape of trial_ticks rows; the column's rule
// (cmpc_regroup_column: the four trial words, read once per workgroup) is workgroup-uniform.  A started column's row r is the bit copy of source row
// t0 + min(r, n - 1), column s, array by array through the snapshot kernel's row copy (snap_row: 16-byte pieces aligned on the destination for the rows of
// 64 words and more); the planner's rows of destination row 0 are written zero.  The workgroup of row 0 also writes the column's words -- the end tick, the
// flag and dStates[0] = dState0[q].  A column without a trial, and every row but 0 of a trial never started, costs its workgroup the index and at most three
// scalar loads.  Bandwidth-bound (about 12 KB in and out per row and column at N = 20): no LDS, no barrier, no atomics.
__global__ __launch_bounds__(256) void cmpc_rollout_tape_regroup_kernel(CmpcRegroupArgs a)
{
    const int j = blockIdx.x, r = blockIdx.y;   // (the grid is B x rows workgroups: nothing runs past either)
    const int tid = threadIdx.x;
    const CmpcRegroupColumn c = cmpc_regroup_column(a, j);
    const size_t B = (size_t)a.B;
    if (r == 0) {
        if (tid == 0) {
            a.end_out[j] = c.kind == 2 ? c.end : 0;
            if (a.ok_out) a.ok_out[j] = c.kind == 0 ? 0 : 1;
        }
        if (c.kind != 0 && tid < 9) a.dst_states[9 * (size_t)j + tid] = a.state0[9 * (size_t)c.q + tid];
    }
    if (c.kind != 2) return;                    // (uniform)
    const size_t sr = (size_t)cmpc_regroup_source_row(c, r);
    for (int i = 0; i < CMPC_REGROUP_ARRAYS; ++i) {
        const int w = a.words[i];
        unsigned* const d = a.dst[i] + (size_t)w * ((size_t)r * B + j);
        if (r == 0 && i >= CMPC_REGROUP_PLAN) {
            for (int e = tid; e < w; e += 256) d[e] = 0u;
        } else {
            snap_row(d, a.src[i] + (size_t)w * (sr * B + c.s), w, tid);
        }
    }
    if (tid < 9) a.dst_states[9 * (((size_t)r + 1) * B + j) + tid] = a.src_states[9 * ((sr + 1) * B + c.s) + tid];
}

// gate: one thread per problem for the small arrays (cmpc_walk_gate_problem; lanes past B do nothing), then every thread strides over the wide rows
// (cmpc_walk_gate_wide).  The two parts touch disjoint arrays: no barrier, no atomics.
__global__ __launch_bounds__(256) void cmpc_walk_vjp_gate_kernel(CmpcGateArgs a, size_t wide)
{
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (tid < (size_t)a.B) cmpc_walk_gate_problem(a, (int)tid);
    for (size_t e = tid; e < wide; e += stride) cmpc_walk_gate_wide(a, e);
}

// gate of the forward walk: one thread per (problem, column) for the small arrays (cmpc_walk_jvp_gate_column; lanes past B k do nothing), then every
// thread strides over the wide row [B][k][n_x] (cmpc_walk_jvp_gate_wide).  The two parts touch disjoint arrays: no LDS, no barrier, no atomics.
__global__ __launch_bounds__(256) void cmpc_walk_jvp_gate_kernel(CmpcJvpGateArgs a, size_t cols, size_t wide)
{
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (tid < cols) cmpc_walk_jvp_gate_column(a, tid);
    for (size_t e = tid; e < wide; e += stride) cmpc_walk_jvp_gate_wide(a, e);
}

}  // namespace

extern "C" int cmpc_launch_warm_shift(const CmpcParams* prm, const float* dXprev, float* dX0, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_warm_shift_kernel, dim3(prm->B), dim3(256), 0, stream, prm->N, prm->B, dXprev, dX0);
    return (int)hipGetLastError();
}

static unsigned stride_blocks(size_t least_threads, size_t work)
{
    size_t nb = (work + 255) / 256;
    if (nb > 2048) nb = 2048;
    const size_t lb = (least_threads + 255) / 256;
    return (unsigned)(nb > lb ? nb : lb);
}

extern "C" int cmpc_launch_rollout_tape(const CmpcTapeArgs* a, hipStream_t stream)
{
    const size_t work = (a->parts & 2) ? (size_t)a->B * (a->nx > a->np ? a->nx : a->np) : (size_t)a->B * 9;
    hipLaunchKernelGGL(cmpc_rollout_tape_kernel, dim3(stride_blocks(1, work)), dim3(256), 0, stream, *a);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_rollout_snapshot(const CmpcSnapshotArgs* a, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_rollout_snapshot_kernel, dim3(a->B), dim3(256), 0, stream, *a);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_refill_restore(const CmpcRefillRestoreArgs* a, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_refill_restore_kernel, dim3(a->copy.B), dim3(256), 0, stream, *a);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_refill_plans(const CmpcRefillPlansArgs* a, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_refill_plans_kernel, dim3(a->B), dim3(256), 0, stream, *a);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_plan_fold(int Q, int words, const int* index, const double* per, int pool_rows, double* out, hipStream_t stream)
{
    const size_t entries = (size_t)pool_rows * words;
    hipLaunchKernelGGL(cmpc_plan_fold_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, Q, words, index, per, pool_rows, out);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_rollout_tape_regroup(const CmpcRegroupArgs* a, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_rollout_tape_regroup_kernel, dim3(a->B, a->rows), dim3(256), 0, stream, *a);
    return (int)hipGetLastError();
}

extern "C" size_t cmpc_walk_gate_wide_entries(const CmpcGateArgs* a)
{
    int w = a->nx > a->np ? a->nx : a->np;   // (6 N < n_p: the wrench row is covered)
    if (a->do_post && a->rot_row && 6 * a->N > w) w = 6 * a->N;
    return (size_t)a->B * w;
}

extern "C" int cmpc_launch_walk_vjp_gate(const CmpcGateArgs* a, hipStream_t stream)
{
    const size_t wide = cmpc_walk_gate_wide_entries(a);
    hipLaunchKernelGGL(cmpc_walk_vjp_gate_kernel, dim3(stride_blocks((size_t)a->B, wide)), dim3(256), 0, stream, *a, wide);
    return (int)hipGetLastError();
}

extern "C" size_t cmpc_walk_jvp_gate_wide_entries(const CmpcJvpGateArgs* a)
{
    return a->do_post && a->x_row ? (size_t)a->B * a->K * a->nx : 0;
}

extern "C" int cmpc_launch_walk_jvp_gate(const CmpcJvpGateArgs* a, hipStream_t stream)
{
    const size_t cols = (size_t)a->B * a->K, wide = cmpc_walk_jvp_gate_wide_entries(a);
    hipLaunchKernelGGL(cmpc_walk_jvp_gate_kernel, dim3(stride_blocks(cols, wide)), dim3(256), 0, stream, *a, cols, wide);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_rollout_record(const CmpcRecordArgs* a, int* stats, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_rollout_record_kernel<false>, dim3((a->B + 255) / 256), dim3(256), 0, stream, *a, stats, CmpcLimitArgs{});
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_rollout_record_limits(const CmpcRecordArgs* a, const CmpcLimitArgs* lm, int* stats, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_rollout_record_kernel<true>, dim3((a->B + 255) / 256), dim3(256), 0, stream, *a, stats, *lm);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_extremes_init(int B, float* ext, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_extremes_init_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, ext);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_walk_measures_vjp(const CmpcMeasureVjpArgs* v, hipStream_t stream)
{
    const size_t n = (size_t)v->rows * v->B;
    hipLaunchKernelGGL(cmpc_walk_measures_vjp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *v);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_walk_measures_fold(int N, int B, int rows, const double* direct, float* grad_p, double* grad_model, hipStream_t stream)
{
    const size_t np = grad_p ? (size_t)rows * B : 0, nm = grad_model ? (size_t)24 * B : 0, n = np > nm ? np : nm;
    if (n == 0) return 0;
    hipLaunchKernelGGL(cmpc_walk_measures_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, N, B, rows, direct, grad_p, grad_model);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_walk_measures_jvp(const CmpcMeasureJvpArgs* v, hipStream_t stream)
{
    const size_t n = (size_t)v->rows * v->B;
    hipLaunchKernelGGL(cmpc_walk_measures_jvp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *v);
    return (int)hipGetLastError();
}

// wrench_rows null: one thread per (row, problem), which writes the plant row and the pass word alone
extern "C" int cmpc_launch_wrench_sense(const CmpcSenseArgs* a, float* wrench_rows, float* plant_rows, int* pass_rows, hipStream_t stream)
{
    const int knots = wrench_rows ? a->N : 1;
    const size_t n = (size_t)a->rows * a->B * knots;
    hipLaunchKernelGGL(cmpc_wrench_sense_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *a, knots, wrench_rows, plant_rows, pass_rows);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_wrench_sense_vjp(const CmpcSenseVjpArgs* v, hipStream_t stream)
{
    const int out_rows = v->grad_noise && v->s.noise_ticks > v->s.hidden_ticks ? v->s.noise_ticks : v->s.hidden_ticks;
    const size_t n = (size_t)out_rows * v->s.B * 6;
    hipLaunchKernelGGL(cmpc_wrench_sense_vjp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *v, out_rows);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_wrench_sense_jvp(const CmpcSenseJvpArgs* v, hipStream_t stream)
{
    const size_t n = (size_t)v->s.rows * v->s.B * v->K * v->s.N;
    hipLaunchKernelGGL(cmpc_wrench_sense_jvp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *v);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_outcome_init(int B, const float* state0, int* end_tick, int* end_code, int* it_sum, int* it_max, float* final_state,
                                        float* slack_min, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_outcome_init_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, state0, end_tick, end_code, it_sum, it_max, final_state,
                       slack_min);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_refill(const CmpcRefillArgs* a, int* next, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_refill_kernel, dim3(1), dim3(256), 0, stream, *a, next);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_refill_init(const CmpcRefillArgs* a, int* next, hipStream_t stream)
{
    const int n = a->B > a->Q ? a->B : a->Q;
    hipLaunchKernelGGL(cmpc_refill_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *a, next);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_cold_start(int N, int B, float g8, const float* dP, float* dX0, const int* ended, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_cold_start_kernel, dim3(B), dim3(256), 0, stream, N, g8, dP, dX0, ended);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_tick_pre(int B, int N, int M, double dt, double now, int merge, const double* plan_t, const float* plan_pose, const int* plan_n,
                                    const double* prev_t, const float* prev_pose, const int* prev_n, double* list_t, float* list_pose, int* list_n, int* ok,
                                    int* land, const float* box, const float* state, const float* wrench, float* P, const float* Xprev, float* X0,
                                    const float* plan_com, const float* plan_h, int plan_knots, double plan_dt, double plan_t_offset, double robot_mass,
                                    double com_height, long long snap_dt_ns, const int* snap_ok, const int* ended, const float* noise, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_tick_pre_kernel<false>, dim3(B), dim3(256), 0, stream, B, N, M, dt, now, merge, plan_t, plan_pose, plan_n, prev_t, prev_pose, prev_n,
                       list_t, list_pose, list_n, ok, land, box, state, wrench, P, Xprev, X0, plan_com, plan_h, plan_knots, plan_dt, plan_t_offset, robot_mass,
                       com_height, snap_dt_ns, snap_ok, ended, noise, CmpcRefillTick{}, CmpcRefillTrialArgs{});
    return (int)hipGetLastError();
}

// the front and back kernels of a refill walk's tick (cmpc_rollout_walk_refill_device): a merge tick with M <= 16 in which every slot runs at its own time
// tr (cmpc_rollout_walk_refill_trials_device; null: the launches of cmpc_rollout_walk_refill_device): the front kernel's per-trial instantiation when it
// holds models or noise, the back kernel's when it holds a hidden wrench or a gain
extern "C" int cmpc_launch_tick_pre_refill(int B, int N, int M, double dt, const double* plan_t, const float* plan_pose, const int* plan_n,
                                           const double* prev_t, const float* prev_pose, const int* prev_n, double* list_t, float* list_pose, int* list_n,
                                           int* ok, int* land, const float* box, const float* state, float* P, const float* Xprev, float* X0,
                                           const float* plan_com, const float* plan_h, int plan_knots, double plan_dt, double robot_mass, double com_height,
                                           long long snap_dt_ns, const int* ended, const int* start, const int* trial, int tick, const float* wrench_trials,
                                           int wrench_ticks, int trials, double plan_t_first, float g8, const CmpcRefillTrialArgs* tr,
                                           int offset, hipStream_t stream)
{
    if (M > 16 || offset < 0) return (int)hipErrorInvalidValue;
    const CmpcRefillTick rf{start, trial, tick, offset, wrench_trials, wrench_ticks, trials, plan_t_first, g8};
    if (tr && (tr->models || tr->noise))
        hipLaunchKernelGGL((cmpc_tick_pre_kernel<true, true>), dim3(B), dim3(256), 0, stream, B, N, M, dt, 0.0, 1, plan_t, plan_pose, plan_n, prev_t, prev_pose,
                           prev_n, list_t, list_pose, list_n, ok, land, box, state, (const float*)nullptr, P, Xprev, X0, plan_com, plan_h, plan_knots, plan_dt,
                           0.0, robot_mass, com_height, snap_dt_ns, (const int*)nullptr, ended, (const float*)nullptr, rf, *tr);
    else
        hipLaunchKernelGGL((cmpc_tick_pre_kernel<true>), dim3(B), dim3(256), 0, stream, B, N, M, dt, 0.0, 1, plan_t, plan_pose, plan_n, prev_t, prev_pose, prev_n,
                           list_t, list_pose, list_n, ok, land, box, state, (const float*)nullptr, P, Xprev, X0, plan_com, plan_h, plan_knots, plan_dt, 0.0,
                           robot_mass, com_height, snap_dt_ns, (const int*)nullptr, ended, (const float*)nullptr, rf, CmpcRefillTrialArgs{});
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_tick_post_refill(int B, int N, int M, double dt, float grav, const float* dCorners, int corners_stride, const float* dX,
                                            const float* dP, const float* dStateIn, float* dStateOut, float* dZmp, float h, int nsub, float zx, float zy,
                                            const int* land, const double* t, float* pose, const int* n, const int* ended, const int* start, int tick,
                                            const int* trial, const CmpcRefillTrialArgs* tr, int offset, hipStream_t stream)
{
    if (tr && (tr->hidden || tr->gain))
        hipLaunchKernelGGL((cmpc_tick_post_kernel<true, true>), dim3((B + 255) / 256), dim3(256), 0, stream, B, N, M, 0.0, grav, dCorners, corners_stride, dX,
                           dP, dStateIn, dStateOut, dZmp, h, nsub, zx, zy, land, t, pose, n, ended, tr->hidden, tr->gain, start, tick, dt, trial,
                           tr->hidden_ticks, tr->Q, offset);
    else
        hipLaunchKernelGGL((cmpc_tick_post_kernel<false, true>), dim3((B + 255) / 256), dim3(256), 0, stream, B, N, M, 0.0, grav, dCorners, corners_stride, dX,
                           dP, dStateIn, dStateOut, dZmp, h, nsub, zx, zy, land, t, pose, n, ended, (const float*)nullptr, (const float*)nullptr, start, tick,
                           dt, (const int*)nullptr, 0, 0, offset);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_tick_post(int B, int N, int M, double now, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                                     const float* dStateIn, float* dStateOut, float* dZmp, float h, int nsub, float zx, float zy, const int* land,
                                     const double* t, float* pose, const int* n, const int* ended, const float* hidden, const float* gain, hipStream_t stream)
{
    if (hidden || gain)
        hipLaunchKernelGGL((cmpc_tick_post_kernel<true, false>), dim3((B + 255) / 256), dim3(256), 0, stream, B, N, M, now, grav, dCorners, corners_stride, dX, dP,
                           dStateIn, dStateOut, dZmp, h, nsub, zx, zy, land, t, pose, n, ended, hidden, gain, (const int*)nullptr, 0, 0.0, (const int*)nullptr, 0, 0, 0);
    else
        hipLaunchKernelGGL((cmpc_tick_post_kernel<false, false>), dim3((B + 255) / 256), dim3(256), 0, stream, B, N, M, now, grav, dCorners, corners_stride, dX, dP,
                           dStateIn, dStateOut, dZmp, h, nsub, zx, zy, land, t, pose, n, ended, hidden, gain, (const int*)nullptr, 0, 0.0, (const int*)nullptr, 0, 0, 0);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_plant_step(int N, int B, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                                      const float* dStateIn, float* dStateOut, float* dZmp, float h, int nsub, float zx, float zy,
                                      const float* dHidden, const float* dGain, hipStream_t stream)
{
    if (dHidden || dGain)   // (both null: the instantiation without the mismatch, which is the kernel as it was before the mismatch existed)
        hipLaunchKernelGGL(cmpc_plant_step_kernel<true>, dim3((B + 255) / 256), dim3(256), 0, stream, N, B, grav, dCorners, corners_stride, dX, dP, dStateIn,
                           dStateOut, dZmp, h, nsub, zx, zy, dHidden, dGain);
    else
        hipLaunchKernelGGL(cmpc_plant_step_kernel<false>, dim3((B + 255) / 256), dim3(256), 0, stream, N, B, grav, dCorners, corners_stride, dX, dP, dStateIn,
                           dStateOut, dZmp, h, nsub, zx, zy, dHidden, dGain);
    return (int)hipGetLastError();
}

// dDirRot0 / dGradRot0 NULL: the instantiation without the rotation term, which is the kernel as it was before that term existed
extern "C" int cmpc_launch_plant_jvp(int N, int B, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                                     const float* dStateIn, float h, int nsub, const double* dDirState, const float* dDirX, const float* dDirP,
                                     const double* dDirModel, const double* dDirRot0, double* dOut, hipStream_t stream)
{
    if (dDirRot0)
        hipLaunchKernelGGL(cmpc_plant_jvp_kernel<true>, dim3((B + 255) / 256), dim3(256), 0, stream, N, B, grav, dCorners, corners_stride, dX, dP, dStateIn, h,
                           nsub, dDirState, dDirX, dDirP, dDirModel, dDirRot0, dOut);
    else
        hipLaunchKernelGGL(cmpc_plant_jvp_kernel<false>, dim3((B + 255) / 256), dim3(256), 0, stream, N, B, grav, dCorners, corners_stride, dX, dP, dStateIn, h,
                           nsub, dDirState, dDirX, dDirP, dDirModel, dDirRot0, dOut);
    return (int)hipGetLastError();
}

// the same with K columns per problem, directions [B][K][...]; dOk [B] or null (a problem whose word is 0 gets zeros)
extern "C" int cmpc_launch_plant_jvp_cols(int N, int B, int K, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                                          const float* dStateIn, float h, int nsub, const double* dDirState, const float* dDirX, const float* dDirP,
                                          const double* dDirModel, const double* dDirRot0, const int* dOk, double* dOut, hipStream_t stream)
{
    return cmpc_launch_plant_jvp_cols_mismatch(N, B, K, grav, dCorners, corners_stride, dX, dP, dStateIn, h, nsub, dDirState, dDirX, dDirP, dDirModel, dDirRot0,
                                               dOk, dOut, 0, nullptr, nullptr, nullptr, nullptr, stream);
}

// mismatch != 0: the instantiations of the mismatched plant (dHidden / dGain / dDirHidden / dDirGain may each be null); 0: the kernels as they were before it
extern "C" int cmpc_launch_plant_jvp_cols_mismatch(int N, int B, int K, float grav, const float* dCorners, int corners_stride, const float* dX,
                                                   const float* dP, const float* dStateIn, float h, int nsub, const double* dDirState, const float* dDirX,
                                                   const float* dDirP, const double* dDirModel, const double* dDirRot0, const int* dOk, double* dOut,
                                                   int mismatch, const float* dHidden, const float* dGain, const double* dDirHidden, const double* dDirGain,
                                                   hipStream_t stream)
{
    const unsigned blocks = (unsigned)(((long long)B * K + 255) / 256);
#define CMPC_PLANT_JVP_COLS(ROT, MM)                                                                                                                          \
    hipLaunchKernelGGL((cmpc_plant_jvp_cols_kernel<ROT, MM>), dim3(blocks), dim3(256), 0, stream, N, B, K, grav, dCorners, corners_stride, dX, dP, dStateIn, h, \
                       nsub, dDirState, dDirX, dDirP, dDirModel, dDirRot0, dOk, dOut, dHidden, dGain, dDirHidden, dDirGain)
    if (mismatch) { if (dDirRot0) CMPC_PLANT_JVP_COLS(true, true); else CMPC_PLANT_JVP_COLS(false, true); }
    else { if (dDirRot0) CMPC_PLANT_JVP_COLS(true, false); else CMPC_PLANT_JVP_COLS(false, false); }
#undef CMPC_PLANT_JVP_COLS
    return (int)hipGetLastError();
}

// dGradX / dGradP: the whole rows are cleared first (the kernel writes the entries the plant reads, nothing else)
extern "C" int cmpc_launch_plant_vjp(int N, int B, float grav, const float* dCorners, int corners_stride, const float* dX, const float* dP,
                                     const float* dStateIn, float h, int nsub, const double* dGradOut, double* dGradState, float* dGradX, float* dGradP,
                                     double* dGradModel, double* dGradRot0, int mismatch, const float* dHidden, const float* dGain, double* dGradHidden,
                                     double* dGradGain, hipStream_t stream)
{
    const CmpcIdx L{N};
    hipError_t e = hipSuccess;
    if (dGradX) e = hipMemsetAsync(dGradX, 0, sizeof(float) * (size_t)B * L.nx(), stream);
    if (e == hipSuccess && dGradP) e = hipMemsetAsync(dGradP, 0, sizeof(float) * (size_t)B * L.np(), stream);
    if (e != hipSuccess) return (int)e;
    // mismatch != 0: the instantiations of the mismatched plant (dHidden / dGain may still be null); 0: the kernels as they were before it existed
#define CMPC_PLANT_VJP(ROT, MM)                                                                                                                              \
    hipLaunchKernelGGL((cmpc_plant_vjp_kernel<ROT, MM>), dim3((B + 255) / 256), dim3(256), 0, stream, N, B, grav, dCorners, corners_stride, dX, dP, dStateIn, h, \
                       nsub, dGradOut, dGradState, dGradX, dGradP, dGradModel, dGradRot0, dHidden, dGain, dGradHidden, dGradGain)
    if (mismatch) { if (dGradRot0) CMPC_PLANT_VJP(true, true); else CMPC_PLANT_VJP(false, true); }
    else { if (dGradRot0) CMPC_PLANT_VJP(true, false); else CMPC_PLANT_VJP(false, false); }
#undef CMPC_PLANT_VJP
    return (int)hipGetLastError();
}

// y[n] += x[n]
extern "C" int cmpc_launch_axpy_float(size_t n, const float* x, float* y, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_axpy_float_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, x, y);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_tick_vjp_combine(int B, int N, const float* info, const int* ok, const float* gp_sol, const float* gp_plant, const double* gm_sol,
                                            const double* gm_plant, double* g_state, float* g_wrench, double* g_model, float* g_p, float* sens, int* ok_out,
                                            const double* g_rot0, double* g_rot, const double* gh_plant, const double* gg_plant, double* g_hidden,
                                            float* g_noise, double* g_gain, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_tick_vjp_combine_kernel, dim3(B), dim3(128), 0, stream, B, N, info, ok, gp_sol, gp_plant, gm_sol, gm_plant, g_state, g_wrench,
                       g_model, g_p, sens, ok_out, g_rot0, g_rot, gh_plant, gg_plant, g_hidden, g_noise, g_gain);
    return (int)hipGetLastError();
}

// cols = B k workgroups
extern "C" int cmpc_launch_tick_jvp_assemble(size_t cols, int N, const double* d_state, const float* d_wrench, const float* d_extra, float* d_p,
                                             const float* d_noise, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_tick_jvp_assemble_kernel, dim3((unsigned)cols), dim3(128), 0, stream, N, d_state, d_wrench, d_extra, d_p, d_noise);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_tick_jvp_flag(int B, int N, int K, const float* info, const int* ok, const float* state_in, float* sens, float* d_x, float* d_p,
                                         double* d_rot, double* d_rot0, int* ok_out, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_tick_jvp_flag_kernel, dim3(B), dim3(128), 0, stream, N, K, info, ok, state_in, sens, d_x, d_p, d_rot, d_rot0, ok_out);
    return (int)hipGetLastError();
}

// ---- compact per-problem output for the all-gather of the multi-GPU path: CoM trajectory 3(N+1), first-knot
// corner forces 24, knot-0 and knot-1 foot positions 12, iterations, status  ->  out[B][3(N+1) + 38] ----
namespace {
__global__ __launch_bounds__(128) void cmpc_compact_kernel(int N, const float* __restrict__ X, const float* __restrict__ info,
                                                           float* __restrict__ out)
{
    const CmpcIdx L{N};
    const int b = blockIdx.x, ncom = 3 * (N + 1), W = ncom + 38;
    const float* x = X + (size_t)b * L.nx();
    for (int c = threadIdx.x; c < W; c += 128) {
        float v;
        if (c < ncom) v = x[L.oCom() + c];
        else if (c < ncom + 24) { const int f = c - ncom; v = x[L.oF(f / 12, (f % 12) / 3) + f % 3]; }
        else if (c < ncom + 36) { const int p = c - ncom - 24; v = x[L.oPos(p / 6) + p % 6]; }
        else v = info[(size_t)b * CMPC_INFO_N + (c == ncom + 36 ? 0 : 5)];
        out[(size_t)b * W + c] = v;
    }
}
}  // namespace

extern "C" int cmpc_launch_compact(int N, int B, const float* dX, const float* dInfo, float* dOut, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_compact_kernel, dim3(B), dim3(128), 0, stream, N, dX, dInfo, dOut);
    return (int)hipGetLastError();
}
