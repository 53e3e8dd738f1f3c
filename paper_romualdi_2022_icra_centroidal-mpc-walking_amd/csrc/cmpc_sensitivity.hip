// Derivatives of the solution map p -> x*(p) at a returned point (include/cmpc.h, "solution sensitivities"; derivation: DESIGN.md 7c).
//
// The barrier form of sIPOPT: [W J_E^T; J_E 0] [dx; dlam_E] = -r(dp), W = grad_xx L + sum_I J_i^T Sigma_i J_i.  It is solved in the solver's
// stage form: state 15 + the 24 previous forces (39), control = 24 forces + 6 landing offsets (30), swing feet land at
// nom + R^-T q, stance vel columns and stance box rows do not exist.  One workgroup of 256 threads per problem, float64 throughout:
//   1. one Riccati factorisation (backward), the control Hessian shifted by SENS_SHIFT on the force diagonal; per stage P_{k+1}, H^-1 and the
//      gain K = -H^-1 G go to a per-handle HBM workspace (the stage matrices are rebuilt from x, p, lam_g wherever they are needed);
//   2. per chunk of up to SENS_KC right-hand sides: a backward and a forward pass, then SENS_NREF steps of iterative refinement against the
//      unshifted operator, then one pass that measures the relative residual.  The right-hand sides of a chunk are JVP directions or -- the cotangent
//      columns of cmpc_solution_vjp_cols_device -- VJP cotangents, each bit for bit the single-column VJP on that cotangent.
// Model directions (include/cmpc.h, "model directions"): the per-problem model theta adds right-hand-side terms (model_q / model_r / model_c) to the
// JVP's columns, and the VJP contracts the same entries with its stored adjoint into 34 sums per problem (model_vjp).
// Rotation directions (include/cmpc.h, "rotation directions"): one omega per foot and stage moves R along R [omega]x; rot_r / rot_c add its terms to the
// JVP's columns, and the VJP contracts the same entries with its stored adjoint into 6 N sums per problem (rot_vjp).
// No atomics: every reduction is a fixed tree or one thread's loop, so a problem's result depends on nothing but its own inputs.
#include "cmpc_device.h"
#include "cmpc_launch.h"

#include <cmath>

namespace {

constexpr int SX = CMPC_NXA;      // 39
constexpr int SU = CMPC_NU;       // 30
constexpr int SENS_KC = 8;        // right-hand sides per chunk
constexpr int CS = 40;            // doubles per column slot in LDS (>= 39)
constexpr int SENS_NREF = 2;      // refinement steps against the unshifted operator
constexpr int SENS_NT = 256;
constexpr double SENS_SMIN = CMPC_SENS_SMIN;
constexpr double SENS_WEAK = CMPC_SENS_WEAK;
constexpr double SENS_SHIFT = CMPC_SENS_SHIFT;

// state / control indices
__host__ __device__ constexpr int sCom() { return 0; }
__host__ __device__ constexpr int sDcom() { return 3; }
__host__ __device__ constexpr int sH() { return 6; }
__host__ __device__ constexpr int sPos(int c) { return 9 + 3 * c; }
__host__ __device__ constexpr int uF(int c, int j) { return 12 * c + 3 * j; }
__host__ __device__ constexpr int uQ(int c) { return 24 + 3 * c; }

#if defined(__HIP_DEVICE_COMPILE__)
#define SENS_SYNC() __syncthreads()
#else
#define SENS_SYNC() ((void)0)
#endif

struct Team {
    int tid, nt;
    double* red;   // 4 doubles (device)
};

// max over the team (256 threads on the device: one wave reduction + four partials; the host team has one thread)
__host__ __device__ inline double team_max(const Team& T, double v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((T.tid & 63) == 0) T.red[T.tid >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(T.red[0], T.red[1]), fmax(T.red[2], T.red[3]));
    __syncthreads();
    return r;
#else
    (void)T;
    return v;
#endif
}

// ---- the geometry of one stage: everything the stage matrices are made of ----
struct Geo {
    double gam[2];
    double R[2][9];        // R(r, c) at 3 r + c
    double Ri[2][9];       // R^-T: a swing foot lands at nom + Ri q
    double rv[2][4][3];    // lever arms r = R corner + pos - com
    double fs[2][4][3];    // corner forces
    double lamh[3];        // lam_g of the angular-momentum rows of the stage
    double afr[2][4][4][3];  // friction row normals a = R (sx, sy, -mu): g = a . f
    double sfr[2][4][4];   // Sigma of the friction rows
    double sU[2][3], sL[2][3];
    int qm[2][3];          // 0: no such control (stance), 1: free offset, 2: fixed offset (lower == upper)
    double hcom[3];        // curvature of the CoM cost at the knot
    double dt, wh, wpos, wsym, D[3];
    int k, N;
    double weak, weak_swing, sigmax;   // (stage build: weakly active rows of loaded feet and box sides, of swing feet, largest Sigma)
};

struct Prob {
    const CmpcConsts* K;
    CmpcIdx L;
    int gh;       // first g row of the angular-momentum dynamics
    int gbox[2], gfric[2];
    const float* x;
    const float* p;
    const float* lam;
};

__host__ __device__ inline double skewm(const double* v, int a, int b)   // [v]x (a, b)
{
    if (a == b) return 0.0;
    const int o = 3 - a - b;
    return ((b - a + 3) % 3 == 1) ? -v[o] : v[o];
}

// Geo of stage k (k == N: only the knot's costs).  Thread 0 does the scalar part; the rows are spread over the team.
__host__ __device__ inline void build_geo(const Team& T, const Prob& P, int k, Geo& g)
{
    const CmpcConsts& K = *P.K;
    const int N = P.L.N;
    const CmpcIdx& L = P.L;
    if (T.tid == 0) {
        g.k = k; g.N = N;
        g.dt = K.dt; g.wh = 2.0 * (double)K.w_h; g.wpos = 2.0 * (double)K.w_pos; g.wsym = 2.0 * (double)K.w_sym;
        for (int i = 0; i < 3; ++i) g.D[i] = K.D[i];
        g.hcom[0] = 2.0 * (double)K.w_com0; g.hcom[1] = 2.0 * (double)K.w_com1; g.hcom[2] = K.wz2[k];
        g.weak = 0.0; g.weak_swing = 0.0; g.sigmax = 0.0;
    }
    if (k == N) { SENS_SYNC(); return; }
    for (int e = T.tid; e < 2; e += T.nt) {
        const int c = e;
        g.gam[c] = P.p[L.pGam(c) + k];
        const float* Rp = P.p + L.pR(c) + 9 * k;
        double R[9];
        for (int r = 0; r < 3; ++r)
            for (int cc = 0; cc < 3; ++cc) R[3 * r + cc] = Rp[3 * cc + r];
        for (int i = 0; i < 9; ++i) g.R[c][i] = R[i];
        // R^-T = cof(R) / det(R)
        double cof[9];
        for (int r = 0; r < 3; ++r)
            for (int cc = 0; cc < 3; ++cc) {
                const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (cc + 1) % 3, c2 = (cc + 2) % 3;
                cof[3 * r + cc] = R[3 * r1 + c1] * R[3 * r2 + c2] - R[3 * r1 + c2] * R[3 * r2 + c1];
            }
        const double det = R[0] * cof[0] + R[1] * cof[1] + R[2] * cof[2];
        for (int i = 0; i < 9; ++i) g.Ri[c][i] = cof[i] / det;
        for (int j = 0; j < 4; ++j) {
            const float* cn = K.corners + 12 * c + 3 * j;
            for (int i = 0; i < 3; ++i) {
                g.rv[c][j][i] = R[3 * i] * cn[0] + R[3 * i + 1] * cn[1] + R[3 * i + 2] * cn[2] + (double)P.x[L.oPos(c) + 3 * k + i] -
                                (double)P.x[L.oCom() + 3 * k + i];
                g.fs[c][j][i] = P.x[L.oF(c, j) + 3 * k + i];
            }
        }
    }
    for (int e = T.tid; e < 3; e += T.nt) g.lamh[e] = P.lam[P.gh + 3 * k + e];
    SENS_SYNC();
    // friction rows: 32 per stage
    for (int e = T.tid; e < 32; e += T.nt) {
        const int c = e >> 4, j = (e >> 2) & 3, f = e & 3;
        const double sx = (f == 0 || f == 3) ? 1.0 : -1.0, sy = (f < 2) ? 1.0 : -1.0, mu = K.mu_fr;
        double a[3], gv = 0.0;
        for (int r = 0; r < 3; ++r) {
            a[r] = g.R[c][3 * r] * sx + g.R[c][3 * r + 1] * sy - mu * g.R[c][3 * r + 2];
            g.afr[c][j][f][r] = a[r];
            gv += a[r] * g.fs[c][j][r];
        }
        const double z = fmax((double)P.lam[P.gfric[c] + 16 * k + 4 * j + f], 0.0);
        const double s = -gv;
        g.sfr[c][j][f] = z / fmax(s, SENS_SMIN);
    }
    // landing offsets of swing feet: 6 per stage
    for (int e = T.tid; e < 6; e += T.nt) {
        const int c = e / 3, i = e % 3;
        const float lo = P.p[L.pLo(c) + 3 * k + i], up = P.p[L.pUp(c) + 3 * k + i];
        g.sU[c][i] = 0.0; g.sL[c][i] = 0.0;
        if (!(P.p[L.pGam(c) + k] < 0.5f)) { g.qm[c][i] = 0; continue; }
        if (!((up - lo) > 1e-9f)) { g.qm[c][i] = 2; continue; }    // (the solver's rule, qfree_compute)
        g.qm[c][i] = 1;
        double v = 0.0;
        for (int r = 0; r < 3; ++r)
            v += g.R[c][3 * r + i] * ((double)P.x[L.oPos(c) + 3 * (k + 1) + r] - (double)P.p[L.pNom(c) + 3 * (k + 1) + r]);
        const double l = P.lam[P.gbox[c] + 3 * k + i];
        const double zU = fmax(l, 0.0), zL = fmax(-l, 0.0), sU = (double)up - v, sL = v - (double)lo;
        g.sU[c][i] = zU / fmax(sU, SENS_SMIN);
        g.sL[c][i] = zL / fmax(sL, SENS_SMIN);
    }
    SENS_SYNC();
    if (T.tid == 0) {   // weakly active rows and the largest Sigma, in a fixed order
        // (friction rows of a swing foot are counted apart: its forces enter no dynamics, and they sit near the apex because the symmetry and rate
        // costs pull them towards zero from inside the pyramid, not because a face binds)
        double w = 0.0, ws = 0.0, sm = 0.0;
        for (int e = 0; e < 32; ++e) {
            const int c = e >> 4, j = (e >> 2) & 3, f = e & 3;
            double gv = 0.0;
            for (int r = 0; r < 3; ++r) gv += g.afr[c][j][f][r] * g.fs[c][j][r];
            const double z = fmax((double)P.lam[P.gfric[c] + 16 * k + 4 * j + f], 0.0);
            if (z < SENS_WEAK && -gv < SENS_WEAK) {
                if (g.gam[c] >= 0.5) w += 1.0;
                else ws += 1.0;
            }
            sm = fmax(sm, g.sfr[c][j][f]);
        }
        for (int e = 0; e < 6; ++e) {
            const int c = e / 3, i = e % 3;
            if (g.qm[c][i] != 1) continue;
            double v = 0.0;
            for (int r = 0; r < 3; ++r)
                v += g.R[c][3 * r + i] * ((double)P.x[L.oPos(c) + 3 * (k + 1) + r] - (double)P.p[L.pNom(c) + 3 * (k + 1) + r]);
            const double l = P.lam[P.gbox[c] + 3 * k + i];
            const double up = P.p[L.pUp(c) + 3 * k + i], lo = P.p[L.pLo(c) + 3 * k + i];
            if (fmax(l, 0.0) < SENS_WEAK && up - v < SENS_WEAK) w += 1.0;
            if (fmax(-l, 0.0) < SENS_WEAK && v - lo < SENS_WEAK) w += 1.0;
            sm = fmax(sm, fmax(g.sU[c][i], g.sL[c][i]));
        }
        g.weak = w; g.weak_swing = ws; g.sigmax = sm;
    }
    SENS_SYNC();
}

// ---- stage matrices as entry functions ----
__host__ __device__ inline double Qe(const Geo& g, int i, int j)   // knot k (k == N: terminal)
{
    if (i != j) return 0.0;
    if (i < 3) return g.hcom[i];
    if (i < 6) return 0.0;
    if (i < 9) return g.wh;
    if (i < 15) return g.wpos;
    return (g.k >= 1 && g.k < g.N) ? g.D[(i - 15) % 3] : 0.0;
}
__host__ __device__ inline double Se(const Geo& g, int i, int j)   // control i, state j
{
    if (i >= 24) return 0.0;
    const int c = i / 12, a = i % 3;
    if (j >= 15) return (g.k >= 1 && j - 15 == i) ? -g.D[a] : 0.0;
    if (j >= 9) {
        if ((j - 9) / 3 != c) return 0.0;
        return -g.dt * g.gam[c] * skewm(g.lamh, a, (j - 9) % 3);
    }
    if (j < 3) return g.dt * g.gam[c] * skewm(g.lamh, a, j);
    return 0.0;
}
__host__ __device__ inline double Re(const Geo& g, int i, int j)   // control i, control j (unshifted)
{
    if (i >= 24 || j >= 24) {
        if (i != j) return 0.0;
        const int c = (i - 24) / 3, a = (i - 24) % 3;
        return g.qm[c][a] == 1 ? g.sU[c][a] + g.sL[c][a] : 1.0;
    }
    const int c1 = i / 12, j1 = (i % 12) / 3, a1 = i % 3, c2 = j / 12, j2 = (j % 12) / 3, a2 = j % 3;
    if (c1 != c2) return 0.0;
    double v = 0.0;
    if (a1 == a2) {
        const double gm = g.gam[c1];
        v += g.wsym * ((j1 == j2 ? 1.0 : 0.0) + (0.25 * gm * gm - 0.5 * gm));
        if (j1 == j2 && g.k >= 1) v += g.D[a1];
    }
    if (j1 == j2)
        for (int f = 0; f < 4; ++f) v += g.sfr[c1][j1][f] * g.afr[c1][j1][f][a1] * g.afr[c1][j1][f][a2];
    return v;
}
__host__ __device__ inline double Ae(const Geo& g, int i, int j)
{
    if (i < 3) return i == j ? 1.0 : (j == 3 + i ? g.dt : 0.0);
    if (i < 6) return i == j ? 1.0 : 0.0;
    if (i < 9) {
        const int a = i - 6;
        if (j == i) return 1.0;
        double v = 0.0;
        if (j < 3) {
            for (int c = 0; c < 2; ++c)
                for (int jj = 0; jj < 4; ++jj) v += g.gam[c] * skewm(g.fs[c][jj], a, j);
            return g.dt * v;
        }
        if (j >= 9 && j < 15) {
            const int c = (j - 9) / 3;
            for (int jj = 0; jj < 4; ++jj) v += skewm(g.fs[c][jj], a, (j - 9) % 3);
            return -g.dt * g.gam[c] * v;
        }
        return 0.0;
    }
    if (i < 15) {
        const int c = (i - 9) / 3;
        return (i == j && g.gam[c] >= 0.5) ? 1.0 : 0.0;
    }
    return 0.0;
}
__host__ __device__ inline double Be(const Geo& g, int i, int j)
{
    if (i < 3) return 0.0;
    if (j < 24) {
        const int c = j / 12, jj = (j % 12) / 3, a = j % 3;
        if (i < 6) return (i - 3 == a) ? g.dt * g.gam[c] : 0.0;
        if (i < 9) return g.dt * g.gam[c] * skewm(g.rv[c][jj], i - 6, a);
        if (i < 15) return 0.0;
        return (i - 15 == j) ? 1.0 : 0.0;
    }
    const int c = (j - 24) / 3, a = (j - 24) % 3;
    if (i >= 9 && i < 15 && (i - 9) / 3 == c && g.qm[c][a] == 1) return g.Ri[c][3 * ((i - 9) % 3) + a];
    return 0.0;
}

// ---- workspace of one problem (doubles) ----
struct Ws {
    double* Pst;   // [N+1][39*39]  P_k
    double* Hi;    // [N][30*30]    H_k^-1
    double* Kg;    // [N][30*39]    K_k = -H_k^-1 G_k
    double* col;   // [KC][colsz]
    int N;
    __host__ __device__ static long long colsz(int N) { return 3LL * SX * (N + 1) + 2LL * SU * N + (long long)SX * N; }
    __host__ __device__ static long long doubles(int N) { return (long long)(N + 1) * SX * SX + (long long)N * (SU * SU + SU * SX) + SENS_KC * colsz(N); }
    // per column: x~ [N+1][39], lam [N+1][39], p [N+1][39], u [N][30], kff [N][30], c [N][39]
    __host__ __device__ double* xs(int j) const { return col + j * colsz(N); }
    __host__ __device__ double* ls(int j) const { return xs(j) + SX * (N + 1); }
    __host__ __device__ double* ps(int j) const { return ls(j) + SX * (N + 1); }
    __host__ __device__ double* us(int j) const { return ps(j) + SX * (N + 1); }
    __host__ __device__ double* kf(int j) const { return us(j) + SU * N; }
    __host__ __device__ double* cs(int j) const { return kf(j) + SU * N; }
};

// LDS of the dense stage work (doubles)
struct Lds {
    double *P, *A, *Bm, *PA, *PB, *H, *G, *Y;   // factorisation
    // column passes (overlay PA.. of the factorisation): per column 64-double slots
    double *q, *r, *c, *pn, *t, *h, *kf, *xk, *uk, *xn, *ln, *lk;
    Geo* g;
    __host__ __device__ static int doubles() { return 3 * SX * SX + 3 * SX * SU + SU * SU + SU * SX; }
};

// ---- the per-problem model as a direction (include/cmpc.h, "model directions") ----
// Fields in cmpc_model's packed order: 0 friction, 1..3 com_weight, 4 angular momentum, 5 contact position, 6..8 force rate, 9 symmetry,
// 10 + 12 c + 3 j + b the corner (c, j), axis b.  The derivative is taken at the problem's float32 record; com_weight[2] enters as
// wz2(k) = 2 w_z(k)^2 = w_cz^2 (1 + e^-k)^2 / 2, so d wz2 / d w_cz = sqrt(2 wz2) (1 + e^-k).
struct MDir {
    const double* d;   // the caller's dtheta[34] (t < 0)
    int t;             // or the unit vector of field t
    __host__ __device__ double operator[](int i) const { return t >= 0 ? (i == t ? 1.0 : 0.0) : d[i]; }
};

__host__ __device__ inline double dwz2(const CmpcConsts& K, int k) { return sqrt(2.0 * (double)K.wz2[k]) * (1.0 + exp(-(double)k)); }

// R(r, cc) of foot c at stage k at 3 r + cc (as build_geo)
__host__ __device__ inline void stage_R(const Prob& P, int c, int k, double* R)
{
    const float* Rp = P.p + P.L.pR(c) + 9 * k;
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) R[3 * r + cc] = Rp[3 * cc + r];
}

// q entry e (state, 39) of the model right-hand side at knot k (k == N: terminal): the weights on com / h / pos, the force rate on the
// previous-force part of the state (stages 1..N-1)
__host__ __device__ inline double model_q(const Prob& P, int k, int e, const MDir& d)
{
    const CmpcConsts& K = *P.K;
    const CmpcIdx& L = P.L;
    if (e < 3) {
        const double dw = e == 0 ? 2.0 * d[1] : e == 1 ? 2.0 * d[2] : dwz2(K, k) * d[3];
        return dw * ((double)P.x[L.oCom() + 3 * k + e] - (double)P.p[L.pComref() + 3 * k + e]);
    }
    if (e < 6) return 0.0;
    if (e < 9) return 2.0 * d[4] * ((double)P.x[L.oH() + 3 * k + e - 6] - (double)P.p[L.pHref() + 3 * k + e - 6]);
    if (e < 15) {
        const int c = (e - 9) / 3, a = (e - 9) % 3;
        return 2.0 * d[5] * ((double)P.x[L.oPos(c) + 3 * k + a] - (double)P.p[L.pNom(c) + 3 * k + a]);
    }
    if (k < 1 || k >= L.N) return 0.0;
    const int i = e - 15, c = i / 12, j = (i % 12) / 3, a = i % 3;
    const float* f = P.x + L.oF(c, j) + 3 * k + a;
    return -2.0 * d[6 + a] * ((double)f[0] - (double)f[-3]);
}

// r entry i (control, 30) of stage k < N: symmetry and force rate on the forces, friction through lam^T dg/dmu and the row's Sigma, the corners
// through the angular-momentum rows' lam_h x (R e_b)
__host__ __device__ inline double model_r(const Prob& P, int k, int i, const MDir& d)
{
    if (i >= 24) return 0.0;
    const CmpcConsts& K = *P.K;
    const CmpcIdx& L = P.L;
    const int c = i / 12, j = (i % 12) / 3, a = i % 3;
    const double gm = P.p[L.pGam(c) + k], dt = K.dt, mu = K.mu_fr;
    double mean = 0.0;
    for (int l = 0; l < 4; ++l) mean += 0.25 * (double)P.x[L.oF(c, l) + 3 * k + a];
    const double fa = P.x[L.oF(c, j) + 3 * k + a];
    const double es = fa - gm * mean, esum = 4.0 * mean * (1.0 - gm);
    double v = 2.0 * d[9] * (es - 0.25 * gm * esum);
    if (k >= 1) v += 2.0 * d[6 + a] * (fa - (double)P.x[L.oF(c, j) + 3 * (k - 1) + a]);
    double R[9], f[3];
    stage_R(P, c, k, R);
    for (int m = 0; m < 3; ++m) f[m] = P.x[L.oF(c, j) + 3 * k + m];
    const double fl2 = R[2] * f[0] + R[5] * f[1] + R[8] * f[2];   // (R^T f)_z
    double fr = 0.0;
    for (int face = 0; face < 4; ++face) {
        const double sx = (face == 0 || face == 3) ? 1.0 : -1.0, sy = (face < 2) ? 1.0 : -1.0;
        double gv = 0.0;   // Sigma of the row, as build_geo
        for (int r = 0; r < 3; ++r) gv += (R[3 * r] * sx + R[3 * r + 1] * sy - mu * R[3 * r + 2]) * f[r];
        const double l = P.lam[P.gfric[c] + 16 * k + 4 * j + face];
        const double sg = fmax(l, 0.0) / fmax(-gv, SENS_SMIN);
        const double aa = R[3 * a] * sx + R[3 * a + 1] * sy - mu * R[3 * a + 2];
        fr += -l * R[3 * a + 2] - sg * aa * fl2;
    }
    v += d[0] * fr;
    double lh[3];
    for (int m = 0; m < 3; ++m) lh[m] = P.lam[P.gh + 3 * k + m];
    const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
    for (int b = 0; b < 3; ++b)   // -dt gam (lam_h x R e_b)_a
        v += d[10 + 12 * c + 3 * j + b] * (-dt * gm * (lh[a1] * R[3 * a2 + b] - lh[a2] * R[3 * a1 + b]));
    return v;
}

// c entry e (39) of stage k < N: the corners in the angular-momentum dynamics, dt gam ((R e_b) x f)
__host__ __device__ inline double model_c(const Prob& P, int k, int e, const MDir& d)
{
    if (e < 6 || e >= 9) return 0.0;
    const CmpcConsts& K = *P.K;
    const CmpcIdx& L = P.L;
    const int a = e - 6, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
    const double dt = K.dt;
    double v = 0.0;
    for (int c = 0; c < 2; ++c) {
        double R[9];
        stage_R(P, c, k, R);
        const double gm = P.p[L.pGam(c) + k];
        for (int j = 0; j < 4; ++j) {
            const float* f = P.x + L.oF(c, j) + 3 * k;
            for (int b = 0; b < 3; ++b)
                v += d[10 + 12 * c + 3 * j + b] * (dt * gm * (R[3 * a1 + b] * (double)f[a2] - R[3 * a2 + b] * (double)f[a1]));
        }
    }
    return v;
}

// one knot's share of the model right-hand side's primal block r_x in the NLP's x layout (the force column of stage k gathers the stage form's
// r_k entry and the force-rate share on x~_{k+1}'s previous forces): sum over the column of n r_x (n: the internal-force direction, e3 scaled as
// internal_dir; null: none) and of r_x^2
__host__ __device__ inline void model_rx_knot(const Prob& P, int k, const MDir& d, const double* e3, double& nr, double& rr)
{
    const int N = P.L.N;
    double s = 0.0, q = 0.0;
    for (int e = 0; e < 15; ++e) { const double v = model_q(P, k, e, d); q += v * v; }
    if (k < N)
        for (int i = 0; i < 24; ++i) {
            const double v = model_r(P, k, i, d) + (k + 1 < N ? model_q(P, k + 1, 15 + i, d) : 0.0);
            q += v * v;
            if (e3) s += (i < 12 ? e3[i % 3] : -e3[i % 3]) * v;
        }
    nr = s; rr = q;
}

// ---- the stage rotations as a direction (include/cmpc.h, "rotation directions") ----
// omega[2][N][3] moves R_{c,k} along dR = R [omega_{c,k}]x.  Every term of the NLP is linear in R's entries, so these are exact.  No state entry (q):
// f does not depend on R, and the lever arm R cn + pos - com enters grad_x L on pos / com through f x lam_h alone.
struct RDir {
    const double* d;   // the caller's omega[2][N][3] (t < 0)
    int t;             // or the unit vector of entry t = 3 (c N + k) + a
    __host__ __device__ void get(int N, int c, int k, double* w) const
    {
        const int o = 3 * (c * N + k);
        for (int a = 0; a < 3; ++a) w[a] = t >= 0 ? (o + a == t ? 1.0 : 0.0) : d[o + a];
    }
};

__host__ __device__ inline void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// r entry i (control, 30) of stage k < N.  Forces: the lever arm in the angular-momentum rows, -dt gam (lam_h x R (omega x cn)); the friction rows
// g = al . R^T f (al = (sx, sy, -mu)) through lam, R (omega x al), and through their Sigma, d g = al . (R^T f x omega) -- swing feet's rows too.
// Free landing offsets: the stage form lands a swing foot at nom + R^-T q and d(R^-T) = R^-T [omega]x, so the position costate R^-T^T lam_pos = -lam_box
// (stationarity in q at the returned point) leaves omega x lam_box
__host__ __device__ inline double rot_r(const Prob& P, int k, int i, const RDir& d)
{
    const CmpcConsts& K = *P.K;
    const CmpcIdx& L = P.L;
    const int c = i < 24 ? i / 12 : (i - 24) / 3;
    double w[3];
    d.get(L.N, c, k, w);
    if (w[0] == 0.0 && w[1] == 0.0 && w[2] == 0.0) return 0.0;
    if (i >= 24) {
        const int a = (i - 24) % 3;
        if (!(P.p[L.pGam(c) + k] < 0.5f) || !((P.p[L.pUp(c) + 3 * k + a] - P.p[L.pLo(c) + 3 * k + a]) > 1e-9f)) return 0.0;
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        return w[a1] * (double)P.lam[P.gbox[c] + 3 * k + a2] - w[a2] * (double)P.lam[P.gbox[c] + 3 * k + a1];
    }
    const int j = (i % 12) / 3, a = i % 3, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
    const double gm = P.p[L.pGam(c) + k], dt = K.dt, mu = K.mu_fr;
    double R[9], f[3], fl[3], flw[3], cn[3], wc[3], lh[3];
    stage_R(P, c, k, R);
    for (int m = 0; m < 3; ++m) { f[m] = P.x[L.oF(c, j) + 3 * k + m]; cn[m] = K.corners[12 * c + 3 * j + m]; lh[m] = P.lam[P.gh + 3 * k + m]; }
    for (int m = 0; m < 3; ++m) fl[m] = R[m] * f[0] + R[3 + m] * f[1] + R[6 + m] * f[2];   // R^T f
    cross3(fl, w, flw);
    cross3(w, cn, wc);
    double rw1 = 0.0, rw2 = 0.0;   // (R (omega x cn)) at a1, a2
    for (int m = 0; m < 3; ++m) { rw1 += R[3 * a1 + m] * wc[m]; rw2 += R[3 * a2 + m] * wc[m]; }
    double v = -dt * gm * (lh[a1] * rw2 - lh[a2] * rw1);
    for (int face = 0; face < 4; ++face) {
        const double al[3] = {(face == 0 || face == 3) ? 1.0 : -1.0, (face < 2) ? 1.0 : -1.0, -mu};
        double wa[3], gv = 0.0, dg = 0.0, ra = 0.0, rwa = 0.0;
        cross3(w, al, wa);
        for (int m = 0; m < 3; ++m) { gv += al[m] * fl[m]; dg += al[m] * flw[m]; ra += R[3 * a + m] * al[m]; rwa += R[3 * a + m] * wa[m]; }
        const double l = P.lam[P.gfric[c] + 16 * k + 4 * j + face];
        const double sg = fmax(l, 0.0) / fmax(-gv, SENS_SMIN);   // Sigma of the row, as build_geo
        v += l * rwa + sg * ra * dg;
    }
    return v;
}

// c entry e (39) of stage k < N: the lever arms in the angular-momentum dynamics, dt gam (R (omega x cn)) x f, and a swing foot's landing
// nom + R^-T q at the returned q = R^T (pos_{k+1} - nom_{k+1}): R^-T (omega x q), free and fixed components alike
__host__ __device__ inline double rot_c(const Prob& P, int k, int e, const RDir& d)
{
    if (e < 6 || e >= 15) return 0.0;
    const CmpcConsts& K = *P.K;
    const CmpcIdx& L = P.L;
    if (e < 9) {
        const int a = e - 6, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        const double dt = K.dt;
        double v = 0.0;
        for (int c = 0; c < 2; ++c) {
            double w[3], R[9];
            d.get(L.N, c, k, w);
            if (w[0] == 0.0 && w[1] == 0.0 && w[2] == 0.0) continue;
            stage_R(P, c, k, R);
            const double gm = P.p[L.pGam(c) + k];
            for (int j = 0; j < 4; ++j) {
                const float* f = P.x + L.oF(c, j) + 3 * k;
                double cn[3], wc[3], rw1 = 0.0, rw2 = 0.0;
                for (int m = 0; m < 3; ++m) cn[m] = K.corners[12 * c + 3 * j + m];
                cross3(w, cn, wc);
                for (int m = 0; m < 3; ++m) { rw1 += R[3 * a1 + m] * wc[m]; rw2 += R[3 * a2 + m] * wc[m]; }
                v += dt * gm * (rw1 * (double)f[a2] - rw2 * (double)f[a1]);
            }
        }
        return v;
    }
    const int c = (e - 9) / 3, a = (e - 9) % 3;
    if (!(P.p[L.pGam(c) + k] < 0.5f)) return 0.0;
    double w[3], R[9], q[3], wq[3], cof[3];
    d.get(L.N, c, k, w);
    if (w[0] == 0.0 && w[1] == 0.0 && w[2] == 0.0) return 0.0;
    stage_R(P, c, k, R);
    for (int i = 0; i < 3; ++i) {
        q[i] = 0.0;
        for (int r = 0; r < 3; ++r) q[i] += R[3 * r + i] * ((double)P.x[L.oPos(c) + 3 * (k + 1) + r] - (double)P.p[L.pNom(c) + 3 * (k + 1) + r]);
    }
    cross3(w, q, wq);
    // row a of R^-T = cof(R) / det(R) (as build_geo)
    const int r1 = (a + 1) % 3, r2 = (a + 2) % 3;
    for (int cc = 0; cc < 3; ++cc) {
        const int c1 = (cc + 1) % 3, c2 = (cc + 2) % 3;
        cof[cc] = R[3 * r1 + c1] * R[3 * r2 + c2] - R[3 * r1 + c2] * R[3 * r2 + c1];
    }
    const double det = R[3 * a] * cof[0] + R[3 * a + 1] * cof[1] + R[3 * a + 2] * cof[2];
    return (cof[0] * wq[0] + cof[1] * wq[1] + cof[2] * wq[2]) / det;
}

// stage k's share of a rotation right-hand side's primal block r_x in the NLP's x layout, with both feet in stance over the whole horizon (the only
// case with an internal-force direction: no landing offsets, r_x sits on the force columns): sum of n r_x (n: e3 scaled as internal_dir) and of r_x^2
__host__ __device__ inline void rot_rx_stage(const Prob& P, int k, const RDir& d, const double* e3, double& nr, double& rr)
{
    double s = 0.0, q = 0.0;
    for (int i = 0; i < 24; ++i) {
        const double v = rot_r(P, k, i, d);
        q += v * v;
        s += (i < 12 ? e3[i % 3] : -e3[i % 3]) * v;
    }
    nr = s; rr = q;
}

// a JVP direction's row of dp, or zeros (dDirP == NULL)
struct PDir {
    const float* d;
    __host__ __device__ float operator[](int i) const { return d ? d[i] : 0.f; }
};

// One column's right-hand side at stage k (k == N: q only) -- the caller's definition
struct Rhs {
    int mode;          // 0: JVP direction dp; 1: VJP gradient v (already projected); 2: VJP cotangent columns (projected where an entry is read)
    const float* dir;  // mode 0: [KC][np] rows of this chunk (stride np); mode 1: [nx]; mode 2: [KC][nx] cotangents of this chunk as the caller gave them (stride nx)
    long long stride;
    const double* dmod;   // mode 0: [KC][34] model directions of this chunk, or null
    const double* drot;   // mode 0: [KC][2][N][3] rotation directions of this chunk, or null
    const double* proj;   // with dmod or drot: e3 (3, as internal_dir) then the KC components n^T r_x removed from the columns' force entries; null: none
                          // mode 2: e3 then the KC components n^T v of the chunk's cotangents; null: no internal-force direction
    double* cres;         // mode 2: per column the largest residual (KC) and the largest right-hand-side entry (KC) of the measuring pass; else null
};

// force entry (i < 24 of the control: foot i / 12, axis i % 3) of one cotangent column without its component s along the internal-force direction, rounded
// to float32 as the single-column path rounds its projected copy of v
__host__ __device__ inline float vjp_force_entry(float gv, double s, const double* e3, int i)
{
    float t = gv;
    t -= s * (i < 12 ? e3[i % 3] : -e3[i % 3]);
    return t;
}

// (q_k, r_k, c_k) of column j, written to q[39], r[30], c[39]; k == N: q only.  x0 (k == 0 only, if non-null): the initial state
__host__ __device__ inline void rhs_entry(const Prob& P, const Geo& g, const Rhs& R, int j, int k, int e, double* q, double* r, double* c, double* x0)
{
    const CmpcIdx& L = P.L;
    const int N = L.N;
    if (R.mode == 0) {
        const PDir d{R.dir ? R.dir + j * R.stride : nullptr};
        if (e < SX) {   // q and c entry e
            double qv = 0.0;
            if (e < 3) qv = -g.hcom[e] * d[L.pComref() + 3 * k + e];
            else if (e >= 6 && e < 9) qv = -g.wh * d[L.pHref() + 3 * k + e - 6];
            else if (e >= 9 && e < 15) qv = -g.wpos * d[L.pNom((e - 9) / 3) + 3 * k + (e - 9) % 3];
            q[e] = qv;
            if (x0) {
                double v = 0.0;
                if (e < 9) v = d[L.pCom0() + e];
                else if (e < 15) v = d[L.pCur((e - 9) / 3) + (e - 9) % 3];
                x0[e] = v;
            }
            if (k < N) {
                double cv = 0.0;
                if (e >= 3 && e < 6) cv = g.dt * d[L.pFext() + 3 * k + e - 3];
                else if (e >= 6 && e < 9) cv = g.dt * d[L.pText() + 3 * k + e - 6];
                else if (e >= 9 && e < 15) {
                    const int cc = (e - 9) / 3, a = (e - 9) % 3;
                    if (g.gam[cc] < 0.5) {
                        cv = d[L.pNom(cc) + 3 * (k + 1) + a];
                        for (int i = 0; i < 3; ++i)
                            if (g.qm[cc][i] == 2)
                                cv += g.Ri[cc][3 * a + i] * 0.5 * ((double)d[L.pLo(cc) + 3 * k + i] + (double)d[L.pUp(cc) + 3 * k + i]);
                    }
                }
                if (R.dmod) cv += model_c(P, k, e, MDir{R.dmod + j * CMPC_MODEL_DOUBLES, -1});
                if (R.drot) cv += rot_c(P, k, e, RDir{R.drot + (size_t)j * 6 * N, -1});
                c[e] = cv;
            }
            if (R.dmod) q[e] = qv + model_q(P, k, e, MDir{R.dmod + j * CMPC_MODEL_DOUBLES, -1});
        } else if (k < N) {   // r entry e - SX
            const int i = e - SX;
            double rv = 0.0;
            if (i >= 24) {
                const int cc = (i - 24) / 3, a = (i - 24) % 3;
                if (g.qm[cc][a] == 1) rv = -(g.sU[cc][a] * d[L.pUp(cc) + 3 * k + a] + g.sL[cc][a] * d[L.pLo(cc) + 3 * k + a]);
            }
            if (R.dmod) rv += model_r(P, k, i, MDir{R.dmod + j * CMPC_MODEL_DOUBLES, -1});
            if (R.drot) rv += rot_r(P, k, i, RDir{R.drot + (size_t)j * 6 * N, -1});
            if (R.proj && i < 24) rv -= R.proj[3 + j] * (i < 12 ? R.proj[i % 3] : -R.proj[i % 3]);   // (no component along n)
            r[i] = rv;
        }
    } else {
        const float* v = R.mode == 1 ? R.dir : R.dir + j * R.stride;
        if (e < SX) {
            double qv = 0.0;
            if (e < 9) qv = -(double)v[3 * (N + 1) * (e / 3) + 3 * k + e % 3];
            else if (e < 15) {
                const int cc = (e - 9) / 3, a = (e - 9) % 3;
                qv = -(double)v[L.oPos(cc) + 3 * k + a];
                // vel_k = (pos_k+1 - pos_k) / dt in swing stages
                if (k < N && P.p[L.pGam(cc) + k] < 0.5f) qv += (double)v[L.oVel(cc) + 3 * k + a] / g.dt;
                if (k >= 1 && P.p[L.pGam(cc) + k - 1] < 0.5f) qv -= (double)v[L.oVel(cc) + 3 * (k - 1) + a] / g.dt;
            }
            q[e] = qv;
            if (x0) x0[e] = 0.0;
            if (k < N) c[e] = 0.0;
        } else if (k < N) {
            const int i = e - SX;
            if (R.mode == 1 || i >= 24) r[i] = i < 24 ? -(double)v[L.oF(i / 12, (i % 12) / 3) + 3 * k + i % 3] : 0.0;
            else {
                const float gv = v[L.oF(i / 12, (i % 12) / 3) + 3 * k + i % 3];
                r[i] = -(double)(R.proj ? vjp_force_entry(gv, R.proj[3 + j], R.proj, i) : gv);
            }
        }
    }
}

// copies n doubles global -> LDS / LDS -> global
__host__ __device__ inline void tcopy(const Team& T, double* dst, const double* src, int n)
{
    for (int e = T.tid; e < n; e += T.nt) dst[e] = src[e];
}

// ---- 1. factorisation ----
// returns 1 (team-uniform) on a non-positive pivot
__host__ __device__ __attribute__((noinline)) int factorise(const Team& T, const Prob& P, const Ws& W, const Lds& S, double& weak, double& weak_swing,
                                                              double& sigmax)
{
    const int N = P.L.N;
    Geo& g = *S.g;
    int bad = 0;
    // P_N = Q_N
    build_geo(T, P, N, g);
    for (int e = T.tid; e < SX * SX; e += T.nt) S.P[e] = Qe(g, e / SX, e % SX);
    SENS_SYNC();
    tcopy(T, W.Pst + (size_t)N * SX * SX, S.P, SX * SX);
    for (int k = N - 1; k >= 0; --k) {
        build_geo(T, P, k, g);
        weak += g.weak; weak_swing += g.weak_swing; sigmax = fmax(sigmax, g.sigmax);   // (every thread: g is shared)
        for (int e = T.tid; e < SX * SX; e += T.nt) S.A[e] = Ae(g, e / SX, e % SX);
        for (int e = T.tid; e < SX * SU; e += T.nt) S.Bm[e] = Be(g, e / SU, e % SU);
        SENS_SYNC();
        for (int e = T.tid; e < SX * SX; e += T.nt) {   // PA = P A
            const int i = e / SX, j = e % SX;
            double v = 0.0;
            for (int m = 0; m < SX; ++m) v += S.P[i * SX + m] * S.A[m * SX + j];
            S.PA[e] = v;
        }
        for (int e = T.tid; e < SX * SU; e += T.nt) {   // PB = P B
            const int i = e / SU, j = e % SU;
            double v = 0.0;
            for (int m = 0; m < SX; ++m) v += S.P[i * SX + m] * S.Bm[m * SU + j];
            S.PB[e] = v;
        }
        SENS_SYNC();
        for (int e = T.tid; e < SU * SU; e += T.nt) {   // H = R + B^T P B + shift on the force diagonal
            const int i = e / SU, j = e % SU;
            double v = Re(g, i, j);
            for (int m = 0; m < SX; ++m) v += S.Bm[m * SU + i] * S.PB[m * SU + j];
            if (i == j && i < 24) v += SENS_SHIFT;
            S.H[e] = v;
        }
        for (int e = T.tid; e < SU * SX; e += T.nt) {   // G = S + B^T P A
            const int i = e / SX, j = e % SX;
            double v = Se(g, i, j);
            for (int m = 0; m < SX; ++m) v += S.Bm[m * SU + i] * S.PA[m * SX + j];
            S.G[e] = v;
        }
        SENS_SYNC();
        // Cholesky H = L L^T in place (lower triangle), column by column
        for (int j = 0; j < SU; ++j) {
            const double d = S.H[j * SU + j];
            if (!(d > 0.0)) bad = 1;
            const double ld = d > 0.0 ? sqrt(d) : 1.0;
            SENS_SYNC();
            for (int i = j + 1 + T.tid; i < SU; i += T.nt) S.H[i * SU + j] /= ld;
            SENS_SYNC();
            if (T.tid == 0) S.H[j * SU + j] = ld;
            for (int e = T.tid; e < (SU - j - 1) * (SU - j - 1); e += T.nt) {
                const int i = j + 1 + e / (SU - j - 1), l = j + 1 + e % (SU - j - 1);
                if (l <= i) S.H[i * SU + l] -= S.H[i * SU + j] * S.H[l * SU + j];
            }
            SENS_SYNC();
        }
        // L^-1 into Y's first 900 entries (one column per thread: forward substitution)
        double* Li = S.Y;
        for (int j = T.tid; j < SU; j += T.nt) {
            for (int i = 0; i < SU; ++i) {
                double v = (i == j) ? 1.0 : 0.0;
                for (int m = j; m < i; ++m) v -= S.H[i * SU + m] * Li[m * SU + j];
                Li[i * SU + j] = i < j ? 0.0 : v / S.H[i * SU + i];
            }
        }
        SENS_SYNC();
        // H^-1 = L^-T L^-1 (into PB's space, which is free now), then K = -H^-1 G (into PA's space after P_k is formed)
        double* Hinv = S.PB;
        for (int e = T.tid; e < SU * SU; e += T.nt) {
            const int i = e / SU, j = e % SU;
            double v = 0.0;
            for (int m = (i > j ? i : j); m < SU; ++m) v += Li[m * SU + i] * Li[m * SU + j];
            Hinv[e] = v;
        }
        SENS_SYNC();
        tcopy(T, W.Hi + (size_t)k * SU * SU, Hinv, SU * SU);
        // P_k = Q + A^T P A + G^T K,  K = -H^-1 G  (written into P after P A is no longer needed below)
        double* Kk = S.Y;   // (L^-1 is dead)
        for (int e = T.tid; e < SU * SX; e += T.nt) {
            const int i = e / SX, j = e % SX;
            double v = 0.0;
            for (int m = 0; m < SU; ++m) v -= Hinv[i * SU + m] * S.G[m * SX + j];
            Kk[e] = v;
        }
        SENS_SYNC();
        tcopy(T, W.Kg + (size_t)k * SU * SX, Kk, SU * SX);
        for (int e = T.tid; e < SX * SX; e += T.nt) {
            const int i = e / SX, j = e % SX;
            double v = Qe(g, i, j);
            for (int m = 0; m < SX; ++m) v += S.A[m * SX + i] * S.PA[m * SX + j];
            for (int m = 0; m < SU; ++m) v += S.G[m * SX + i] * Kk[m * SX + j];
            S.P[e] = v;
        }
        SENS_SYNC();
        for (int e = T.tid; e < SX * SX; e += T.nt) {   // symmetrise
            const int i = e / SX, j = e % SX;
            if (i < j) { const double v = 0.5 * (S.P[e] + S.P[j * SX + i]); S.P[e] = v; S.P[j * SX + i] = v; }
        }
        SENS_SYNC();
        tcopy(T, W.Pst + (size_t)k * SX * SX, S.P, SX * SX);
        SENS_SYNC();
    }
    return bad;
}

// ---- 2. the passes of a chunk of nc columns ----
// pass = 0: solve with the caller's right-hand side (write); 1: refinement step (residual as right-hand side, add the correction);
// 2: measure the residual only.  Returns the largest residual (pass 2) and the largest right-hand side entry (all passes) in rn / bn.
__host__ __device__ __attribute__((noinline)) void chunk_pass(const Team& T, const Prob& P, const Ws& W, const Lds& S, const Rhs& R, int nc, int pass, double& rn,
                                           double& bn)
{
    const int N = P.L.N;
    Geo& g = *S.g;
    double rmax = 0.0, bmax = 0.0;
    const bool colmax = pass == 2 && R.cres != nullptr;   // (every stage starts with build_geo's barriers, which order the slots below too)
    if (colmax) for (int e = T.tid; e < 2 * SENS_KC; e += T.nt) R.cres[e] = 0.0;
    // backward sweep: k = N (terminal), then N-1 .. 0
    for (int k = N; k >= 0; --k) {
        build_geo(T, P, k, g);
        if (k < N) {
            for (int e = T.tid; e < SX * SX; e += T.nt) S.A[e] = Ae(g, e / SX, e % SX);
            for (int e = T.tid; e < SX * SU; e += T.nt) S.Bm[e] = Be(g, e / SU, e % SU);
        }
        // the caller's right-hand side of this stage
        for (int e = T.tid; e < nc * (SX + SU); e += T.nt) {
            const int j = e / (SX + SU), i = e % (SX + SU);
            rhs_entry(P, g, R, j, k, i, S.q + CS * j, S.r + CS * j, S.c + CS * j, k == 0 ? S.lk + CS * j : nullptr);
        }
        SENS_SYNC();
        if (colmax)   // per column: the same entries as bmax below (one thread per column; a maximum does not depend on the order)
            for (int j = T.tid; j < nc; j += T.nt) {
                double b = R.cres[SENS_KC + j];
                for (int i = 0; i < SX; ++i) {
                    b = fmax(b, fabs(S.q[CS * j + i]));
                    if (k < N) b = fmax(b, fabs(S.c[CS * j + i]));
                    if (k == 0) b = fmax(b, fabs(S.lk[CS * j + i]));
                }
                if (k < N) for (int i = 0; i < SU; ++i) b = fmax(b, fabs(S.r[CS * j + i]));
                R.cres[SENS_KC + j] = b;
            }
        for (int e = T.tid; e < nc * (SX + SU); e += T.nt) {
            const int j = e / (SX + SU), i = e % (SX + SU);
            double b = 0.0;
            if (i < SX) {
                b = fabs(S.q[CS * j + i]);
                if (k < N) b = fmax(b, fabs(S.c[CS * j + i]));
                if (k == 0) b = fmax(b, fabs(S.lk[CS * j + i]));
            } else if (k < N) b = fabs(S.r[CS * j + i - SX]);
            bmax = fmax(bmax, b);
        }
        if (pass > 0) {
            // residual of the stored solution: rho_Sx, rho_Su, rho_E (stage k), rho_E0 at k == 0
            for (int e = T.tid; e < nc * SX; e += T.nt) {
                const int j = e / SX, i = e % SX;
                S.xk[CS * j + i] = W.xs(j)[k * SX + i];
                if (k < N) { S.xn[CS * j + i] = W.xs(j)[(k + 1) * SX + i]; S.ln[CS * j + i] = W.ls(j)[(k + 1) * SX + i]; }
            }
            for (int e = T.tid; e < nc * SU; e += T.nt) {
                const int j = e / SU, i = e % SU;
                if (k < N) S.uk[CS * j + i] = W.us(j)[k * SU + i];
            }
            SENS_SYNC();
            for (int e = T.tid; e < nc * (SX + SU + SX); e += T.nt) {
                const int j = e / (2 * SX + SU), i = e % (2 * SX + SU);
                const double* xk = S.xk + CS * j;
                const double* uk = S.uk + CS * j;
                const double* xn = S.xn + CS * j;
                const double* ln = S.ln + CS * j;
                double v;
                if (i < SX) {   // stationarity in x~_k
                    v = S.q[CS * j + i] - W.ls(j)[k * SX + i];
                    for (int m = 0; m < SX; ++m) v += Qe(g, i, m) * xk[m];
                    if (k < N) {
                        for (int m = 0; m < SU; ++m) v += Se(g, m, i) * uk[m];
                        for (int m = 0; m < SX; ++m) v += S.A[m * SX + i] * ln[m];
                    }
                    S.t[CS * j + i] = v;
                } else if (i < SX + SU) {   // stationarity in u_k
                    const int a = i - SX;
                    v = 0.0;
                    if (k < N) {
                        v = S.r[CS * j + a];
                        for (int m = 0; m < SX; ++m) v += Se(g, a, m) * xk[m] + S.Bm[m * SU + a] * ln[m];
                        for (int m = 0; m < SU; ++m) v += Re(g, a, m) * uk[m];
                    }
                    S.h[CS * j + a] = v;
                } else {   // dynamics into k + 1
                    const int a = i - SX - SU;
                    v = 0.0;
                    if (k < N) {
                        v = S.c[CS * j + a] - xn[a];
                        for (int m = 0; m < SX; ++m) v += S.A[a * SX + m] * xk[m];
                        for (int m = 0; m < SU; ++m) v += S.Bm[a * SU + m] * uk[m];
                    }
                    S.kf[CS * j + a] = v;
                }
            }
            SENS_SYNC();
            for (int e = T.tid; e < nc * (2 * SX + SU); e += T.nt) {
                const int j = e / (2 * SX + SU), i = e % (2 * SX + SU);
                double v;
                if (i < SX) { v = S.t[CS * j + i]; S.q[CS * j + i] = v; }
                else if (i < SX + SU) { v = S.h[CS * j + i - SX]; if (k < N) S.r[CS * j + i - SX] = v; }
                else { v = S.kf[CS * j + i - SX - SU]; if (k < N) S.c[CS * j + i - SX - SU] = v; }
                if (k == 0 && i < SX) {   // rho_E0 = x0 - x~_0
                    const double r0 = S.lk[CS * j + i] - S.xk[CS * j + i];
                    S.lk[CS * j + i] = r0;
                    v = fmax(fabs(v), fabs(r0));
                }
                rmax = fmax(rmax, fabs(v));
            }
            SENS_SYNC();
            if (colmax)   // per column: the same entries as rmax above
                for (int j = T.tid; j < nc; j += T.nt) {
                    double r = R.cres[j];
                    for (int i = 0; i < SX; ++i) {
                        r = fmax(r, fabs(S.q[CS * j + i]));
                        if (k < N) r = fmax(r, fabs(S.c[CS * j + i]));
                        if (k == 0) r = fmax(r, fabs(S.lk[CS * j + i]));
                    }
                    if (k < N) for (int i = 0; i < SU; ++i) r = fmax(r, fabs(S.r[CS * j + i]));
                    R.cres[j] = r;
                }
        }
        if (pass == 2) continue;
        // Riccati: t = P_{k+1} c + p_{k+1}; h = r + B^T t; kff = -H^-1 h; p_k = q + A^T t + K^T h
        if (k == N) {
            for (int e = T.tid; e < nc * SX; e += T.nt) {
                const int j = e / SX, i = e % SX;
                S.pn[CS * j + i] = S.q[CS * j + i];
                W.ps(j)[N * SX + i] = S.q[CS * j + i];
            }
            SENS_SYNC();
            continue;
        }
        tcopy(T, S.P, W.Pst + (size_t)(k + 1) * SX * SX, SX * SX);
        tcopy(T, S.H, W.Hi + (size_t)k * SU * SU, SU * SU);
        tcopy(T, S.G, W.Kg + (size_t)k * SU * SX, SU * SX);
        for (int e = T.tid; e < nc * SX; e += T.nt) {
            const int j = e / SX, i = e % SX;
            W.cs(j)[k * SX + i] = S.c[CS * j + i];
        }
        SENS_SYNC();
        for (int e = T.tid; e < nc * SX; e += T.nt) {
            const int j = e / SX, i = e % SX;
            double v = S.pn[CS * j + i];
            for (int m = 0; m < SX; ++m) v += S.P[i * SX + m] * S.c[CS * j + m];
            S.t[CS * j + i] = v;
        }
        SENS_SYNC();
        for (int e = T.tid; e < nc * SU; e += T.nt) {
            const int j = e / SU, i = e % SU;
            double v = S.r[CS * j + i];
            for (int m = 0; m < SX; ++m) v += S.Bm[m * SU + i] * S.t[CS * j + m];
            S.h[CS * j + i] = v;
        }
        SENS_SYNC();
        for (int e = T.tid; e < nc * (SU + SX); e += T.nt) {
            const int j = e / (SU + SX), i = e % (SU + SX);
            if (i < SU) {
                double v = 0.0;
                for (int m = 0; m < SU; ++m) v -= S.H[i * SU + m] * S.h[CS * j + m];
                W.kf(j)[k * SU + i] = v;
            } else {
                const int a = i - SU;
                double v = S.q[CS * j + a];
                for (int m = 0; m < SX; ++m) v += S.A[m * SX + a] * S.t[CS * j + m];
                for (int m = 0; m < SU; ++m) v += S.G[m * SX + a] * S.h[CS * j + m];
                S.xn[CS * j + a] = v;   // p_k (staged)
            }
        }
        SENS_SYNC();
        for (int e = T.tid; e < nc * SX; e += T.nt) {
            const int j = e / SX, i = e % SX;
            S.pn[CS * j + i] = S.xn[CS * j + i];
            W.ps(j)[k * SX + i] = S.xn[CS * j + i];
        }
        SENS_SYNC();
    }
    if (pass == 2) { rn = team_max(T, rmax); bn = team_max(T, bmax); return; }
    bn = team_max(T, bmax);
    // forward sweep: x~_0 = x0 (lk holds it from k == 0 of the backward sweep); u = K x~ + kff; lam = P x~ + p; x~' = A x~ + B u + c
    for (int e = T.tid; e < nc * SX; e += T.nt) S.xk[CS * (e / SX) + e % SX] = S.lk[CS * (e / SX) + e % SX];
    SENS_SYNC();
    for (int k = 0; k <= N; ++k) {
        if (k < N) {
            build_geo(T, P, k, g);
            for (int e = T.tid; e < SX * SX; e += T.nt) S.A[e] = Ae(g, e / SX, e % SX);
            for (int e = T.tid; e < SX * SU; e += T.nt) S.Bm[e] = Be(g, e / SU, e % SU);
            tcopy(T, S.G, W.Kg + (size_t)k * SU * SX, SU * SX);
        }
        tcopy(T, S.P, W.Pst + (size_t)k * SX * SX, SX * SX);
        SENS_SYNC();
        for (int e = T.tid; e < nc * (SX + SU); e += T.nt) {
            const int j = e / (SX + SU), i = e % (SX + SU);
            if (i < SX) {
                double v = W.ps(j)[k * SX + i];
                for (int m = 0; m < SX; ++m) v += S.P[i * SX + m] * S.xk[CS * j + m];
                S.lk[CS * j + i] = v;
            } else if (k < N) {
                const int a = i - SX;
                double v = W.kf(j)[k * SU + a];
                for (int m = 0; m < SX; ++m) v += S.G[a * SX + m] * S.xk[CS * j + m];
                S.uk[CS * j + a] = v;
            }
        }
        SENS_SYNC();
        for (int e = T.tid; e < nc * (2 * SX + SU); e += T.nt) {   // store (or add) x~_k, lam_k, u_k
            const int j = e / (2 * SX + SU), i = e % (2 * SX + SU);
            double* dst;
            double v;
            if (i < SX) { dst = W.xs(j) + k * SX + i; v = S.xk[CS * j + i]; }
            else if (i < 2 * SX) { dst = W.ls(j) + k * SX + i - SX; v = S.lk[CS * j + i - SX]; }
            else { if (k == N) continue; dst = W.us(j) + k * SU + i - 2 * SX; v = S.uk[CS * j + i - 2 * SX]; }
            *dst = pass == 0 ? v : *dst + v;
        }
        if (k == N) break;
        for (int e = T.tid; e < nc * SX; e += T.nt) {
            const int j = e / SX, i = e % SX;
            double v = W.cs(j)[k * SX + i];
            for (int m = 0; m < SX; ++m) v += S.A[i * SX + m] * S.xk[CS * j + m];
            for (int m = 0; m < SU; ++m) v += S.Bm[i * SU + m] * S.uk[CS * j + m];
            S.xn[CS * j + i] = v;
        }
        SENS_SYNC();
        for (int e = T.tid; e < nc * SX; e += T.nt) S.xk[CS * (e / SX) + e % SX] = S.xn[CS * (e / SX) + e % SX];
        SENS_SYNC();
    }
    SENS_SYNC();
}

// the direction along which the NLP does not determine the forces (both feet in stance over the whole horizon): left
// corners +e, right corners -e at every knot, e along currentPos_0 - currentPos_1; returns false when there is none
__host__ __device__ inline bool internal_dir(const Prob& P, double* e)
{
    const CmpcIdx& L = P.L;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < L.N; ++k)
            if (!(P.p[L.pGam(c) + k] > 0.5f)) return false;
    double n2 = 0.0;
    for (int i = 0; i < 3; ++i) { e[i] = (double)P.p[L.pCur(0) + i] - (double)P.p[L.pCur(1) + i]; n2 += e[i] * e[i]; }
    const double s = 1.0 / sqrt(n2 * 8.0 * L.N);   // unit norm over the 24 N force entries
    for (int i = 0; i < 3; ++i) e[i] *= s;
    return n2 > 0.0;
}

// inner product of a force vector in x layout with the internal-force direction (one thread, fixed order)
__host__ __device__ inline double internal_dot(const CmpcIdx& L, const double* e, const float* v)
{
    double s = 0.0;
    for (int c = 0; c < 2; ++c)
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < L.N; ++k)
                for (int i = 0; i < 3; ++i) s += (c == 0 ? e[i] : -e[i]) * (double)v[L.oF(c, j) + 3 * k + i];
    return s;
}

__host__ __device__ inline unsigned fbits(float v)
{
    union { float f; unsigned u; } c;
    c.f = v;
    return c.u;
}

// subset rule of include/cmpc.h (the solver's outside_subset, restated on the staged p)
__host__ __device__ inline bool sens_outside_subset(const Prob& P, int ct, int k)
{
    const CmpcIdx& L = P.L;
    const float* p = P.p;
    const float gm = p[L.pGam(ct) + k];
    if (gm == 0.f) return false;
    if (gm != 1.f) return true;
    int kp = -1;
    for (int j = k - 1; j >= 0 && kp < 0; --j) if (p[L.pGam(ct) + j] < 0.5f) kp = j;
    const float* R = p + L.pR(ct) + 9 * k;
    const float* nom = p + L.pNom(ct) + 3 * (k + 1);
    const float* lo = p + L.pLo(ct) + 3 * k;
    const float* up = p + L.pUp(ct) + 3 * k;
    if (kp < 0) {
        const float* cur = p + L.pCur(ct);
        bool out = false;
        for (int i = 0; i < 3; ++i) {
            float v = 0.f;
            for (int a = 0; a < 3; ++a) v += R[3 * i + a] * (cur[a] - nom[a]);
            out = out || !(v >= lo[i] - 1e-6f && v <= up[i] + 1e-6f);
        }
        return out;
    }
    const float* Rp = p + L.pR(ct) + 9 * kp;
    const float* nomp = p + L.pNom(ct) + 3 * (kp + 1);
    const float* lop = p + L.pLo(ct) + 3 * kp;
    const float* upp = p + L.pUp(ct) + 3 * kp;
    bool diff = false;
    for (int a = 0; a < 9; ++a) diff = diff || fbits(R[a]) != fbits(Rp[a]);
    for (int a = 0; a < 3; ++a) diff = diff || fbits(nom[a]) != fbits(nomp[a]) || fbits(lo[a]) != fbits(lop[a]) || fbits(up[a]) != fbits(upp[a]);
    return diff;
}

// the model part of one problem's VJP after its adjoint solve (W column col): gmod[t] = -w^T r_t for the 34 fields, each a sum over the knots in a
// fixed order.  With the internal-force direction e3 (else null), r_t loses its component along n as the JVP's columns do: -w^T r_t + (n^T w)(n^T r_t)
// (w itself can carry a component along n: v is projected in float32 and the shifted system amplifies what is left by 1 / CMPC_SENS_SHIFT), and the
// largest relative component |n^T r_t| / |r_t| goes to rel.  Items (t, k) spread over the team, partial sums in the free dense area of LDS (part:
// 3 x 34 (N+1) doubles).
__host__ __device__ inline void model_vjp(const Team& T, const Prob& P, const Ws& W, int col, const double* e3, double* part, double* gmod, double& rel,
                                          double& nonfinite)
{
    const int N = P.L.N, nk = N + 1, M = CMPC_MODEL_DOUBLES;
    const double* xs = W.xs(col);
    const double* ls = W.ls(col);
    const double* us = W.us(col);
    for (int e = T.tid; e < M * nk; e += T.nt) {
        const int t = e / nk, k = e % nk;
        const MDir d{nullptr, t};
        double v = 0.0;
        for (int i = 0; i < SX; ++i) v += xs[k * SX + i] * model_q(P, k, i, d);
        if (k < N) {
            for (int i = 0; i < 24; ++i) v += us[k * SU + i] * model_r(P, k, i, d);
            for (int i = 6; i < 9; ++i) v += ls[(k + 1) * SX + i] * model_c(P, k, i, d);
        }
        part[e] = v;
        double nr = 0.0, rr = 0.0;
        if (e3) model_rx_knot(P, k, d, e3, nr, rr);
        part[M * nk + e] = nr;
        part[2 * M * nk + e] = rr;
    }
    SENS_SYNC();
    double r = 0.0;
    for (int t = T.tid; t < M; t += T.nt) {
        double v = 0.0, nr = 0.0, rr = 0.0;
        for (int k = 0; k <= N; ++k) { v += part[t * nk + k]; nr += part[M * nk + t * nk + k]; rr += part[2 * M * nk + t * nk + k]; }
        if (e3) {   // n^T w over the force entries u_k (one thread's loop, the same order in every thread)
            double nw = 0.0;
            for (int k = 0; k < N; ++k)
                for (int i = 0; i < 24; ++i) nw += (i < 12 ? e3[i % 3] : -e3[i % 3]) * us[k * SU + i];
            v -= nw * nr;
        }
        gmod[t] = -v;
        if (!__builtin_isfinite(v)) nonfinite = 1.0;
        if (rr > 0.0) r = fmax(r, fabs(nr) / sqrt(rr));
    }
    rel = team_max(T, r);
}

// the JVP's model columns of one chunk before its passes: proj[3 + j] = n^T r_x of column j's model direction (n: e3, removed from the column's
// force entries by rhs_entry), and the largest relative size |n^T r_x| / |r_x| over the chunk into rel.  part: 2 x KC (N+1) doubles of free LDS.
__host__ __device__ inline void model_jvp_proj(const Team& T, const Prob& P, const double* dmod, int nc, double* proj, double* part, double& rel)
{
    const int N = P.L.N, nk = N + 1;
    for (int e = T.tid; e < nc * nk; e += T.nt) {
        const int j = e / nk, k = e % nk;
        double nr, rr;
        model_rx_knot(P, k, MDir{dmod + j * CMPC_MODEL_DOUBLES, -1}, proj, nr, rr);
        part[e] = nr;
        part[SENS_KC * nk + e] = rr;
    }
    SENS_SYNC();
    double r = 0.0;
    for (int j = T.tid; j < nc; j += T.nt) {
        double nr = 0.0, rr = 0.0;
        for (int k = 0; k <= N; ++k) { nr += part[j * nk + k]; rr += part[SENS_KC * nk + j * nk + k]; }
        proj[3 + j] = nr;
        if (rr > 0.0) r = fmax(r, fabs(nr) / sqrt(rr));
    }
    rel = fmax(rel, team_max(T, r));   // (team_max synchronises: proj is complete for every thread)
}

// the rotation part of one problem's VJP after its adjoint solve (W column col): grot[c][k][a] = -w^T r of the unit direction, one item per (foot, stage,
// axis), each a fixed-order loop over the foot's 12 + 3 control entries and the stage's 9 dynamics entries.  With the internal-force direction e3 (else null) every r loses
// its component along n, as model_vjp's do, and the largest relative component goes to rel.
__host__ __device__ inline void rot_vjp(const Team& T, const Prob& P, const Ws& W, int col, const double* e3, double* grot, double& rel, double& nonfinite)
{
    const int N = P.L.N;
    const double* ls = W.ls(col);
    const double* us = W.us(col);
    double nw = 0.0;
    if (e3)   // n^T w over the force entries u_k (one thread's loop, the same order in every thread)
        for (int k = 0; k < N; ++k)
            for (int i = 0; i < 24; ++i) nw += (i < 12 ? e3[i % 3] : -e3[i % 3]) * us[k * SU + i];
    double r = 0.0;
    for (int e = T.tid; e < 6 * N; e += T.nt) {
        const int c = e / (3 * N), k = (e / 3) % N;
        const RDir d{nullptr, e};
        double v = 0.0, nr = 0.0, rr = 0.0;
        for (int i = 12 * c; i < 12 * c + 12; ++i) {   // (the other foot's entries of a one-foot direction are zero) each r once: contraction, n^T r, |r|^2
            const double rv = rot_r(P, k, i, d);
            v += us[k * SU + i] * rv;
            if (e3) nr += (c == 0 ? e3[i % 3] : -e3[i % 3]) * rv;
            rr += rv * rv;
        }
        for (int i = uQ(c); i < uQ(c) + 3; ++i) v += us[k * SU + i] * rot_r(P, k, i, d);
        for (int i = 6; i < 15; ++i) v += ls[(k + 1) * SX + i] * rot_c(P, k, i, d);
        if (e3) {
            v -= nw * nr;
            if (rr > 0.0) r = fmax(r, fabs(nr) / sqrt(rr));
        }
        grot[e] = -v;
        if (!__builtin_isfinite(v)) nonfinite = 1.0;
    }
    rel = fmax(rel, team_max(T, r));
}

// the JVP's rotation columns of one chunk before its passes: n^T r_x of column j's rotation direction joins proj[3 + j] (add: the model part is
// there already), and the largest relative size |n^T r_x| / |r_x| over the chunk joins rel.  part: 2 x KC N doubles of free LDS.
__host__ __device__ inline void rot_jvp_proj(const Team& T, const Prob& P, const double* drot, int nc, bool add, double* proj, double* part, double& rel)
{
    const int N = P.L.N;
    for (int e = T.tid; e < nc * N; e += T.nt) {
        const int j = e / N, k = e % N;
        double nr, rr;
        rot_rx_stage(P, k, RDir{drot + (size_t)j * 6 * N, -1}, proj, nr, rr);
        part[e] = nr;
        part[SENS_KC * N + e] = rr;
    }
    SENS_SYNC();
    double r = 0.0;
    for (int j = T.tid; j < nc; j += T.nt) {
        double nr = 0.0, rr = 0.0;
        for (int k = 0; k < N; ++k) { nr += part[j * N + k]; rr += part[SENS_KC * N + j * N + k]; }
        proj[3 + j] = add ? proj[3 + j] + nr : nr;
        if (rr > 0.0) r = fmax(r, fabs(nr) / sqrt(rr));
    }
    rel = fmax(rel, team_max(T, r));   // (team_max synchronises: proj is complete for every thread)
}

// ---- one problem: JVP (gx == null: k directions dir[k][np] (and dmod[k][34], or null) -> out[k][nx]) or VJP (k cotangents gx[k][nx] -> out[k][np]
// (or null) and gmod[k][34] (or null)); drot[k][2][N][3] (or null) joins the JVP's columns, grot[k][2][N][3] (or null) comes from the VJP's adjoint
// solves.  The VJP's k == 1 keeps its projected copy of v in LDS (vproj); k > 1 runs in chunks as the JVP does, every column projected where its
// entries are read (Rhs mode 2), and column j's outputs are the k == 1 call's on cotangent j bit for bit.  proj: 3 + 3 KC doubles ----
__host__ __device__ __attribute__((noinline)) void sens_problem(const Team& T, const Prob& P, const Ws& W, const Lds& S, const float* dir, const float* gx, int kdir,
                                            float* out, float* sens, float* vproj, const double* dmod, double* gmod, double* proj,
                                            const double* drot, double* grot)
{
    const CmpcIdx& L = P.L;
    const int N = L.N;
    const bool vjp = gx != nullptr;
    const bool cols = vjp && kdir > 1;
    const long long nout = vjp ? (out ? (long long)kdir * L.np() : 0) : (long long)kdir * L.nx();
    // status 3: outside the supported subset, or a model that broke the model rule; status 2: input not finite
    double flag3 = 0.0, flag2 = 0.0;
    for (int e = T.tid; e < 2 * N; e += T.nt) if (sens_outside_subset(P, e / N, e % N)) flag3 = 1.0;
    if (P.K->model_bad) flag3 = 1.0;
    for (int e = T.tid; e < L.nx(); e += T.nt) if (!__builtin_isfinite(P.x[e])) flag2 = 1.0;
    for (int e = T.tid; e < L.np(); e += T.nt) if (!__builtin_isfinite(P.p[e])) flag2 = 1.0;
    for (int e = T.tid; e < L.ng(); e += T.nt) if (!__builtin_isfinite(P.lam[e])) flag2 = 1.0;
    if (vjp) { for (long long e = T.tid; e < (long long)kdir * L.nx(); e += T.nt) if (!__builtin_isfinite(gx[e])) flag2 = 1.0; }
    else if (dir) { for (long long e = T.tid; e < (long long)kdir * L.np(); e += T.nt) if (!__builtin_isfinite(dir[e])) flag2 = 1.0; }
    if (dmod) for (int e = T.tid; e < kdir * CMPC_MODEL_DOUBLES; e += T.nt) if (!__builtin_isfinite(dmod[e])) flag2 = 1.0;
    if (drot) for (int e = T.tid; e < kdir * 6 * N; e += T.nt) if (!__builtin_isfinite(drot[e])) flag2 = 1.0;
    flag3 = team_max(T, flag3);
    flag2 = team_max(T, flag2);
    double status = flag3 > 0.0 ? 3.0 : (flag2 > 0.0 ? 2.0 : 0.0);
    double weak = 0.0, weak_swing = 0.0, sigmax = 0.0, resid = 0.0;
    if (status == 0.0) {
        if (factorise(T, P, W, S, weak, weak_swing, sigmax)) status = 1.0;
        status = team_max(T, status);
    }
    double e3[3];
    const bool has_e = internal_dir(P, e3);
    double nonfinite = 0.0, mrel = 0.0;
    if (status == 0.0) {
        Rhs R;
        R.dmod = nullptr; R.drot = nullptr; R.proj = nullptr; R.cres = nullptr;
        int nchunks = 1;
        if (cols) {   // the columns lose their component along the internal-force direction where rhs_entry reads them: e3 first, then one n^T v per column
            R.mode = 2; R.stride = L.nx();
            R.cres = proj + 3 + SENS_KC;
            nchunks = (kdir + SENS_KC - 1) / SENS_KC;
            if (has_e) {
                if (T.tid == 0) for (int i = 0; i < 3; ++i) proj[i] = e3[i];
                R.proj = proj;
            }
        } else if (vjp) {   // v with no component along the internal-force direction
            double s = 0.0;
            if (has_e) s = internal_dot(L, e3, gx);
            for (int e = T.tid; e < L.nx(); e += T.nt) vproj[e] = gx[e];
            SENS_SYNC();
            if (has_e)
                for (int e = T.tid; e < 24 * N; e += T.nt) {
                    const int c = e / (12 * N), j = (e / (3 * N)) % 4, r = e % (3 * N);
                    vproj[L.oF(c, j) + r] -= s * (c == 0 ? e3[r % 3] : -e3[r % 3]);
                }
            SENS_SYNC();
            R.mode = 1; R.dir = vproj; R.stride = 0;
        } else {
            R.mode = 0; R.stride = L.np();
            nchunks = (kdir + SENS_KC - 1) / SENS_KC;
            if ((dmod || drot) && has_e) {   // the model and rotation columns lose their component along n: e3 first, then one n^T r_x per column
                if (T.tid == 0) for (int i = 0; i < 3; ++i) proj[i] = e3[i];
                SENS_SYNC();
                R.proj = proj;
            }
        }
        for (int ch = 0; ch < nchunks; ++ch) {
            const int nc = kdir - ch * SENS_KC < SENS_KC ? kdir - ch * SENS_KC : SENS_KC;
            if (cols) {
                R.dir = gx + (size_t)ch * SENS_KC * L.nx();
                SENS_SYNC();   // (the previous chunk's readers of proj are done)
                if (has_e) for (int j = T.tid; j < nc; j += T.nt) proj[3 + j] = internal_dot(L, e3, R.dir + (size_t)j * L.nx());
                SENS_SYNC();
            } else if (!vjp) {
                R.dir = dir ? dir + (size_t)ch * SENS_KC * L.np() : nullptr;
                R.dmod = dmod ? dmod + (size_t)ch * SENS_KC * CMPC_MODEL_DOUBLES : nullptr;
                R.drot = drot ? drot + (size_t)ch * SENS_KC * 6 * N : nullptr;
                if (R.proj && R.dmod) model_jvp_proj(T, P, R.dmod, nc, proj, S.P, mrel);
                if (R.proj && R.drot) rot_jvp_proj(T, P, R.drot, nc, R.dmod != nullptr, proj, S.P, mrel);
            }
            double rn = 0.0, bn = 0.0;
            chunk_pass(T, P, W, S, R, nc, 0, rn, bn);
            for (int it = 0; it < SENS_NREF; ++it) chunk_pass(T, P, W, S, R, nc, 1, rn, bn);
            chunk_pass(T, P, W, S, R, nc, 2, rn, bn);
            if (cols)   // per column, as the single calls measure it
                for (int j = 0; j < nc; ++j) resid = fmax(resid, R.cres[SENS_KC + j] > 0.0 ? R.cres[j] / R.cres[SENS_KC + j] : 0.0);
            else resid = fmax(resid, bn > 0.0 ? rn / bn : 0.0);
            // outputs of the chunk
            if (!vjp) {
                for (int e = T.tid; e < nc * L.nx(); e += T.nt) {
                    const int j = e / L.nx(), o = e % L.nx();
                    const double* xs = W.xs(j);
                    const double* us = W.us(j);
                    double v = 0.0;
                    if (o < 9 * (N + 1)) { const int blk = o / (3 * (N + 1)), r = o % (3 * (N + 1)); v = xs[(r / 3) * SX + 3 * blk + r % 3]; }
                    else {
                        const int c = o < L.oPos(1) ? 0 : 1, r = o - L.oPos(c);
                        if (r < 3 * (N + 1)) v = xs[(r / 3) * SX + sPos(c) + r % 3];
                        else if (r < 3 * (N + 1) + 3 * N) {
                            const int k = (r - 3 * (N + 1)) / 3, a = r % 3;
                            if (P.p[L.pGam(c) + k] < 0.5f) v = (xs[(k + 1) * SX + sPos(c) + a] - xs[k * SX + sPos(c) + a]) / (double)P.K->dt;
                        } else {
                            const int rr = r - 3 * (N + 1) - 3 * N, j4 = rr / (3 * N), k = (rr % (3 * N)) / 3, a = rr % 3;
                            v = us[k * SU + uF(c, j4) + a];
                        }
                    }
                    if (!__builtin_isfinite(v)) nonfinite = 1.0;
                    out[(size_t)(ch * SENS_KC + j) * L.nx() + o] = (float)v;
                }
                SENS_SYNC();
                if (has_e)   // no component along the internal-force direction
                    for (int j = T.tid; j < nc; j += T.nt) {
                        float* o = out + (size_t)(ch * SENS_KC + j) * L.nx();
                        const double s = internal_dot(L, e3, o);
                        for (int c = 0; c < 2; ++c)
                            for (int jj = 0; jj < 4; ++jj)
                                for (int r = 0; r < 3 * N; ++r)
                                    o[L.oF(c, jj) + r] = (float)((double)o[L.oF(c, jj) + r] - s * (c == 0 ? e3[r % 3] : -e3[r % 3]));
                    }
                SENS_SYNC();
            } else for (int jc = 0; jc < nc; ++jc) {   // column jc of the chunk: the contraction with dr/dp, then the model and rotation parts
                const double* xs = W.xs(jc);
                const double* ls = W.ls(jc);
                const double* us = W.us(jc);
                const CmpcConsts& K = *P.K;
                const double dt = K.dt;
                const size_t col = (size_t)ch * SENS_KC + jc;
                float* outc = out ? out + col * L.np() : nullptr;
                for (int e = T.tid; e < L.np(); e += T.nt) {
                    double v = 0.0;
                    if (e >= L.pCom0()) {
                        if (e < L.pComref()) v = -ls[e - L.pCom0()];
                        else if (e < L.pHref()) {
                            const int r = e - L.pComref(), k = r / 3, a = r % 3;
                            const double hc = a == 0 ? 2.0 * (double)K.w_com0 : a == 1 ? 2.0 * (double)K.w_com1 : (double)K.wz2[k];
                            v = hc * xs[k * SX + sCom() + a];
                        } else if (e < L.pFext()) {
                            const int r = e - L.pHref();
                            v = 2.0 * (double)K.w_h * xs[(r / 3) * SX + sH() + r % 3];
                        } else if (e < L.pText()) {
                            const int r = e - L.pFext();
                            v = -dt * ls[(r / 3 + 1) * SX + sDcom() + r % 3];
                        } else {
                            const int r = e - L.pText();
                            v = -dt * ls[(r / 3 + 1) * SX + sH() + r % 3];
                        }
                    } else {
                        const int c = e < L.pR(1) ? 0 : 1, r = e - L.pR(c);
                        if (r >= 16 * N && r < 19 * N + 3) {   // nominalPos, knot kn
                            const int kn = (r - 16 * N) / 3, a = (r - 16 * N) % 3;
                            v = 2.0 * (double)K.w_pos * xs[kn * SX + sPos(c) + a];
                            if (kn >= 1 && P.p[L.pGam(c) + kn - 1] < 0.5f) v -= ls[kn * SX + sPos(c) + a];
                        } else if (r >= 19 * N + 3) v = -ls[sPos(c) + r - (19 * N + 3)];
                        else if (r >= 9 * N && r < 15 * N) {   // upper (9N..12N) / lower (12N..15N)
                            const bool upper = r < 12 * N;
                            const int rr = upper ? r - 9 * N : r - 12 * N, k = rr / 3, i = rr % 3;
                            if (P.p[L.pGam(c) + k] < 0.5f) {
                                const float lo = P.p[L.pLo(c) + 3 * k + i], up = P.p[L.pUp(c) + 3 * k + i];
                                if ((up - lo) > 1e-9f) {
                                    // Sigma of the side (recomputed as build_geo does)
                                    double g = 0.0;
                                    for (int a = 0; a < 3; ++a)
                                        g += (double)P.p[L.pR(c) + 9 * k + 3 * i + a] *
                                             ((double)P.x[L.oPos(c) + 3 * (k + 1) + a] - (double)P.p[L.pNom(c) + 3 * (k + 1) + a]);
                                    const double l = P.lam[P.gbox[c] + 3 * k + i];
                                    const double sg = upper ? fmax(l, 0.0) / fmax((double)up - g, SENS_SMIN) : fmax(-l, 0.0) / fmax(g - (double)lo, SENS_SMIN);
                                    v = sg * us[k * SU + uQ(c) + i];
                                } else {
                                    // fixed component: -1/2 (R^-T e_i) . lam_{k+1, pos}
                                    const float* Rp = P.p + L.pR(c) + 9 * k;
                                    double Rm[9], cof[9];
                                    for (int a = 0; a < 3; ++a)
                                        for (int b2 = 0; b2 < 3; ++b2) Rm[3 * a + b2] = Rp[3 * b2 + a];
                                    for (int a = 0; a < 3; ++a)
                                        for (int b2 = 0; b2 < 3; ++b2) {
                                            const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, c1 = (b2 + 1) % 3, c2 = (b2 + 2) % 3;
                                            cof[3 * a + b2] = Rm[3 * a1 + c1] * Rm[3 * a2 + c2] - Rm[3 * a1 + c2] * Rm[3 * a2 + c1];
                                        }
                                    const double det = Rm[0] * cof[0] + Rm[1] * cof[1] + Rm[2] * cof[2];
                                    for (int a = 0; a < 3; ++a) v -= 0.5 * (cof[3 * a + i] / det) * ls[(k + 1) * SX + sPos(c) + a];
                                }
                            }
                        }
                    }
                    if (!__builtin_isfinite(v)) nonfinite = 1.0;
                    if (outc) outc[e] = (float)v;
                }
                SENS_SYNC();
                if (gmod) {
                    double rel = 0.0;
                    model_vjp(T, P, W, jc, has_e ? e3 : nullptr, S.P, gmod + col * CMPC_MODEL_DOUBLES, rel, nonfinite);
                    mrel = fmax(mrel, rel);
                }
                if (grot) rot_vjp(T, P, W, jc, has_e ? e3 : nullptr, grot + col * 6 * N, mrel, nonfinite);
            }
        }
        if (!__builtin_isfinite(resid)) nonfinite = 1.0;
        nonfinite = team_max(T, nonfinite);
        if (nonfinite > 0.0) status = 2.0;
    }
    if (status != 0.0) {
        for (long long e = T.tid; e < nout; e += T.nt) out[e] = 0.f;
        const int kout = vjp ? kdir : 1;
        if (gmod) for (int e = T.tid; e < kout * CMPC_MODEL_DOUBLES; e += T.nt) gmod[e] = 0.0;
        if (grot) for (int e = T.tid; e < kout * 6 * N; e += T.nt) grot[e] = 0.0;
        resid = 0.0;
        mrel = 0.0;
    }
    if (T.tid == 0 && sens) {
        sens[0] = (float)status; sens[1] = (float)resid; sens[2] = (float)weak; sens[3] = (float)sigmax;
        sens[4] = has_e ? 1.f : 0.f;
        sens[5] = (float)weak_swing;
        sens[6] = (float)mrel;
        for (int i = 7; i < CMPC_SENS; ++i) sens[i] = 0.f;
    }
}

// LDS of the kernel: constants | x | p | lam (floats) | v projected (floats) | Geo | dense doubles | 4 reduction doubles | KC + 3 projection doubles |
// 2 KC doubles of per-column residuals (Rhs::cres)
__host__ __device__ inline size_t sens_lds_floats(int N)
{
    const CmpcIdx L{N};
    return ((sizeof(CmpcConsts) + 15) / 16) * 4 + ((L.nx() + 3) & ~3) + ((L.np() + 3) & ~3) + ((L.ng() + 3) & ~3) + ((L.nx() + 3) & ~3);
}
inline size_t sens_lds_bytes(int N)
{
    return sens_lds_floats(N) * 4 + ((sizeof(Geo) + 15) & ~(size_t)15) + 8 * (size_t)(Lds::doubles() + 4 + 3 * SENS_KC + 3);
}

// carves the dense area: the factorisation's eight matrices; the column slots overlay PA, PB, Y (12 x 40 x 8 = 3840 doubles <= their 3861)
__host__ __device__ inline Lds carve(double* base, Geo* g)
{
    Lds S;
    S.g = g;
    S.P = base; S.A = S.P + SX * SX; S.Bm = S.A + SX * SX; S.G = S.Bm + SX * SU; S.H = S.G + SU * SX;
    S.PA = S.H + SU * SU; S.PB = S.PA + SX * SX; S.Y = S.PB + SX * SU;
    // column slots: [12][KC][CS] over PA | PB | Y, which only the factorisation uses (the passes keep P, A, Bm, G, H)
    double* cs = S.PA;
    S.q = cs; S.r = cs + CS * SENS_KC; S.c = cs + 2 * CS * SENS_KC; S.pn = cs + 3 * CS * SENS_KC; S.t = cs + 4 * CS * SENS_KC;
    S.h = cs + 5 * CS * SENS_KC; S.kf = cs + 6 * CS * SENS_KC; S.xk = cs + 7 * CS * SENS_KC; S.uk = cs + 8 * CS * SENS_KC;
    S.xn = cs + 9 * CS * SENS_KC; S.ln = cs + 10 * CS * SENS_KC; S.lk = cs + 11 * CS * SENS_KC;
    return S;
}

}  // namespace

// ---- the kernel: one workgroup per problem of the sub-batch [b0, b0 + gridDim.x) ----
__global__ __launch_bounds__(256) void cmpc_sensitivity_kernel(const CmpcConsts* __restrict__ kc, int kc_per_problem, int N, int b0,
                                                               const float* __restrict__ X, const float* __restrict__ Pp, const float* __restrict__ LamG,
                                                               const float* __restrict__ Dir, const float* __restrict__ GradX, int kdir,
                                                               float* __restrict__ Out, float* __restrict__ Sens, double* __restrict__ Wsp,
                                                               const double* __restrict__ DirModel, double* __restrict__ GradModel,
                                                               const double* __restrict__ DirRot, double* __restrict__ GradRot)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int bl = blockIdx.x, b = b0 + bl;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kc_per_problem ? kc + b : kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += SENS_NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    float* x = reinterpret_cast<float*>(smem) + ((sizeof(CmpcConsts) + 15) / 16) * 4;
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    float* vproj = lam + ((L.ng() + 3) & ~3);
    Geo* g = reinterpret_cast<Geo*>(smem + sens_lds_floats(N) * 4);
    double* dense = reinterpret_cast<double*>(reinterpret_cast<char*>(g) + ((sizeof(Geo) + 15) & ~(size_t)15));
    double* red = dense + Lds::doubles();
    double* proj = red + 4;
    for (int e = tid; e < L.nx(); e += SENS_NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += SENS_NT) p[e] = Pp[(size_t)b * L.np() + e];
    for (int e = tid; e < L.ng(); e += SENS_NT) lam[e] = LamG[(size_t)b * L.ng() + e];
    __syncthreads();
    Prob P;
    P.K = &K; P.L = L; P.x = x; P.p = p; P.lam = lam;
    P.gh = 15 + 6 * N;
    for (int c = 0; c < 2; ++c) { P.gbox[c] = 15 + 15 * N + c * 19 * N; P.gfric[c] = P.gbox[c] + 3 * N; }
    Ws W;
    W.N = N;
    W.Pst = Wsp + (size_t)bl * Ws::doubles(N);
    W.Hi = W.Pst + (size_t)(N + 1) * SX * SX;
    W.Kg = W.Hi + (size_t)N * SU * SU;
    W.col = W.Kg + (size_t)N * SU * SX;
    const Team T{tid, SENS_NT, red};
    const Lds S = carve(dense, g);
    float* sens = Sens ? Sens + (size_t)b * CMPC_SENS : nullptr;
    if (GradX)
        sens_problem(T, P, W, S, nullptr, GradX + (size_t)b * kdir * L.nx(), kdir, Out ? Out + (size_t)b * kdir * L.np() : nullptr, sens, vproj, nullptr,
                     GradModel ? GradModel + (size_t)b * kdir * CMPC_MODEL_DOUBLES : nullptr, proj, nullptr,
                     GradRot ? GradRot + (size_t)b * kdir * 6 * N : nullptr);
    else
        sens_problem(T, P, W, S, Dir ? Dir + (size_t)b * kdir * L.np() : nullptr, nullptr, kdir, Out + (size_t)b * kdir * L.nx(), sens, vproj,
                     DirModel ? DirModel + (size_t)b * kdir * CMPC_MODEL_DOUBLES : nullptr, nullptr, proj,
                     DirRot ? DirRot + (size_t)b * kdir * 6 * N : nullptr, nullptr);
}

// workspace bytes per problem of the launch below
extern "C" size_t cmpc_sensitivity_workspace_bytes(int N) { return sizeof(double) * (size_t)Ws::doubles(N); }

// problems [b0, b0 + nb) of the batch; the workspace holds nb problems.  JVP (dGradX null): dDir and dDirModel (each may be null), dOut = dx.
// VJP (kdir cotangent columns in dGradX[.][kdir][nx]): dOut = dl/dp (or null), dGradModel = dl/dtheta (or null), dGradRot = dl/domega (or null), each
// [.][kdir][..].  dDirRot: the JVP's rotation directions (or null).
extern "C" int cmpc_launch_sensitivity(const CmpcConsts* kc, int kc_per_problem, int N, int b0, int nb, const float* dX, const float* dP, const float* dLamG,
                                       const float* dDir, const float* dGradX, int kdir, float* dOut, float* dSens, double* dWs, const double* dDirModel,
                                       double* dGradModel, const double* dDirRot, double* dGradRot, hipStream_t stream)
{
    const size_t lds = sens_lds_bytes(N);
    static int configured = 0;
    if (!configured) {
        hipError_t e = hipFuncSetAttribute((const void*)cmpc_sensitivity_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        configured = 1;
    }
    hipLaunchKernelGGL(cmpc_sensitivity_kernel, dim3(nb), dim3(SENS_NT), lds, stream, kc, kc_per_problem, N, b0, dX, dP, dLamG, dDir, dGradX, kdir, dOut,
                       dSens, dWs, dDirModel, dGradModel, dDirRot, dGradRot);
    return (int)hipGetLastError();
}
