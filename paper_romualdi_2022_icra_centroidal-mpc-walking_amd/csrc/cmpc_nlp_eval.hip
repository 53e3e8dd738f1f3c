// Batched evaluation of the reference NLP's callbacks on gfx950: f, g, grad f, jac g, hess L.
//
// These are the five functions IPOPT calls through the reference's CasADi-generated code
// (src/centroidal-mpc-walking/config/robots/ergoCubGazeboV1/tmp.c: nlp_fg :12430, nlp_grad
// :24791, nlp_hess_l :58926, nlp_jac_fg :71962), for a batch and for any horizon N.  Jacobian and
// Hessian non-zeros come out in the reference's CCS order (casadi_s5 / casadi_s4, tmp.c:66-67):
// cmpc_nlp_sparsity() builds that order (sort by column, then row) from the structural pattern.
//
// One workgroup per problem: x, p and lam_g are staged in LDS (12 KB at N=20), every output
// element is one thread's closed-form expression, output rows are written coalesced.  The path is
// HBM-write bound (~45 KB out per problem when the Hessian is requested).
#include "cmpc_contacts.h"
#include "cmpc_device.h"
#include "cmpc_launch.h"

#include <algorithm>
#include <vector>

namespace {

// ---- non-zero descriptors: kind | k<<4 | c<<10 | j<<11 | a<<13 | b<<15 | face<<17 ----
enum : int {
    J_ONE = 0, J_MONE, J_MDT, J_DCOM_F, J_H_F, J_H_POS, J_H_COM, J_POS_VEL, J_BBOX, J_FRIC,
    H_COMX = 0, H_COMY, H_COMZ, H_H, H_POS, H_FF, H_RATE, H_F_POS, H_F_COM
};
__host__ __device__ inline int mk(int kind, int k, int c = 0, int j = 0, int a = 0, int b = 0, int face = 0)
{
    return kind | (k << 4) | (c << 10) | (j << 11) | (a << 13) | (b << 15) | (face << 17);
}

struct GLay {  // g-row offsets (SURVEY 8a-NLP 'Constraints')
    int g_init, g_com, g_dcom, g_h, g_pos[2], g_bbox[2], g_fric[2];
};
__host__ __device__ inline void glay_init(GLay& G, int N)
{
    int o = 0;
    G.g_init = o; o += 15;
    G.g_com = o; o += 3 * N; G.g_dcom = o; o += 3 * N; G.g_h = o; o += 3 * N;
    G.g_pos[0] = o; o += 3 * N; G.g_pos[1] = o; o += 3 * N;
    for (int c = 0; c < 2; ++c) { G.g_bbox[c] = o; o += 3 * N; G.g_fric[c] = o; o += 16 * N; }
}

struct Trip { int row, col, desc; };

// skew-matrix entry [v]x(a,b), a != b
__device__ inline float skew(const float* v, int a, int b)
{
    const int o = 3 - a - b;
    return ((b - a + 3) % 3 == 1) ? -v[o] : v[o];
}

// ---- f, g and the gradient of gamma = lam_f f + lam_g^T g (nlp_grad) of one problem, element by element, on x / p / lam_g staged in LDS.  T is the
// arithmetic: float in the NLP callbacks (cmpc_eval_nlp_device, cmpc_eval_nlp_grad_device), double in the KKT certificate and the value gradient, which
// take differences of large terms.  Stored values (x, p, lam_g, the model's float32 constants) are the same in both. ----
struct NlpView {
    const CmpcConsts& K;
    CmpcIdx L;
    GLay G;
    const float* x;
    const float* p;
    const float* lam;
    __device__ float gam(int c, int k) const { return p[L.pGam(c) + k]; }
    template <typename T>
    __device__ void rvec(int c, int j, int k, T* r) const
    {
        const float* R = p + L.pR(c) + 9 * k;
        const float* cn = K.corners + 12 * c + 3 * j;
        for (int i = 0; i < 3; ++i)
            r[i] = T(R[i]) * T(cn[0]) + T(R[3 + i]) * T(cn[1]) + T(R[6 + i]) * T(cn[2]) + T(x[L.oPos(c) + 3 * k + i]) - T(x[L.oCom() + 3 * k + i]);
    }
    template <typename T>
    __device__ void fcsum(int c, int k, T* Fc) const
    {
        for (int i = 0; i < 3; ++i)
            Fc[i] = T(x[L.oF(c, 0) + 3 * k + i]) + T(x[L.oF(c, 1) + 3 * k + i]) + T(x[L.oF(c, 2) + 3 * k + i]) + T(x[L.oF(c, 3) + 3 * k + i]);
    }
};
template <typename T>
__device__ inline T crossc(const T* a, const T* bb, int i) { return a[(i + 1) % 3] * bb[(i + 2) % 3] - a[(i + 2) % 3] * bb[(i + 1) % 3]; }

// this thread's share (entries tid, tid + nt, ...) of the objective f
template <typename T>
__device__ inline T nlp_f_part(const NlpView& V, int tid, int nt)
{
    const CmpcConsts& K = V.K;
    const CmpcIdx& L = V.L;
    const float *x = V.x, *p = V.p;
    const int N = L.N;
    T acc = T(0);
    for (int e = tid; e < 3 * (N + 1); e += nt) {
        const int k = e / 3, i = e % 3;
        const T ec = T(x[L.oCom() + e]) - T(p[L.pComref() + e]);
        acc += (i == 0 ? T(K.w_com0) : (i == 1 ? T(K.w_com1) : T(0.5f) * T(K.wz2[k]))) * ec * ec;
        const T eh = T(x[L.oH() + e]) - T(p[L.pHref() + e]);
        acc += T(K.w_h) * eh * eh;
        for (int c = 0; c < 2; ++c) {
            const T ep = T(x[L.oPos(c) + e]) - T(p[L.pNom(c) + e]);
            acc += T(K.w_pos) * ep * ep;
        }
    }
    for (int e = tid; e < 2 * N * 3; e += nt) {
        const int c = e / (3 * N), k = (e % (3 * N)) / 3, i = e % 3;
        const T g = T(V.gam(c, k));
        T mean = T(0);
        for (int j = 0; j < 4; ++j) mean += T(0.25f) * T(x[L.oF(c, j) + 3 * k + i]);
        for (int j = 0; j < 4; ++j) {
            const T fv = T(x[L.oF(c, j) + 3 * k + i]);
            const T es = fv - g * mean;
            acc += T(K.w_sym) * es * es;
            if (k + 1 < N) {
                const T d = T(x[L.oF(c, j) + 3 * (k + 1) + i]) - fv;
                acc += T(0.5f) * T(K.D[i]) * d * d;
            }
        }
    }
    return acc;
}

// row r of g
template <typename T>
__device__ inline T nlp_g_row(const NlpView& V, int r)
{
    const CmpcConsts& K = V.K;
    const CmpcIdx& L = V.L;
    const GLay& G = V.G;
    const float *x = V.x, *p = V.p;
    const T dt = T(K.dt);
    T v;
    if (r < 15) {
        const int i = r % 3;
        v = T(r < 3 ? x[L.oCom() + i] : r < 6 ? x[L.oDcom() + i] : r < 9 ? x[L.oH() + i] : r < 12 ? x[L.oPos(0) + i] : x[L.oPos(1) + i]);
    } else if (r < G.g_dcom) {
        const int e = r - G.g_com;
        v = T(x[L.oCom() + e + 3]) - (T(x[L.oCom() + e]) + dt * T(x[L.oDcom() + e]));
    } else if (r < G.g_h) {
        const int e = r - G.g_dcom, k = e / 3, i = e % 3;
        T acc = T(p[L.pFext() + e]) - (i == 2 ? T(K.grav) : T(0));
        for (int c = 0; c < 2; ++c) {
            T Fc[3];
            V.fcsum(c, k, Fc);
            acc += T(V.gam(c, k)) * Fc[i];
        }
        v = T(x[L.oDcom() + e + 3]) - (T(x[L.oDcom() + e]) + dt * acc);
    } else if (r < G.g_pos[0]) {
        const int e = r - G.g_h, k = e / 3, i = e % 3, a1 = (i + 1) % 3, a2 = (i + 2) % 3;
        T tor = T(p[L.pText() + e]);
        for (int c = 0; c < 2; ++c) {
            T t = T(0);
            for (int j = 0; j < 4; ++j) {
                T rr[3];
                V.rvec(c, j, k, rr);
                const float* f = x + L.oF(c, j) + 3 * k;
                t += rr[a1] * T(f[a2]) - rr[a2] * T(f[a1]);
            }
            tor += T(V.gam(c, k)) * t;
        }
        v = T(x[L.oH() + e + 3]) - (T(x[L.oH() + e]) + dt * tor);
    } else if (r < G.g_bbox[0]) {
        const int c = r < G.g_pos[1] ? 0 : 1, e = r - G.g_pos[c], k = e / 3;
        v = T(x[L.oPos(c) + e + 3]) - (T(x[L.oPos(c) + e]) + dt * (T(1) - T(V.gam(c, k))) * T(x[L.oVel(c) + e]));
    } else {
        const int c = r < G.g_bbox[1] ? 0 : 1;
        if (r < G.g_fric[c]) {
            const int e = r - G.g_bbox[c], k = e / 3, i = e % 3;
            const float* R = p + L.pR(c) + 9 * k;
            v = T(0);
            for (int a = 0; a < 3; ++a) v += T(R[3 * i + a]) * (T(x[L.oPos(c) + 3 * (k + 1) + a]) - T(p[L.pNom(c) + 3 * (k + 1) + a]));
        } else {
            const int e = r - G.g_fric[c], k = e / 16, j = (e % 16) / 4, face = e % 4;
            const float* R = p + L.pR(c) + 9 * k;
            const float* f = x + L.oF(c, j) + 3 * k;
            const T sx = (face == 0 || face == 3) ? T(1) : T(-1), sy = face < 2 ? T(1) : T(-1);
            T fl[3];
            for (int m = 0; m < 3; ++m) fl[m] = T(R[3 * m]) * T(f[0]) + T(R[3 * m + 1]) * T(f[1]) + T(R[3 * m + 2]) * T(f[2]);
            v = sx * fl[0] + sy * fl[1] - T(K.mu_fr) * fl[2];
        }
    }
    return v;
}

// d f / d (force component e): symmetry + rate terms (as in the grad f branch of cmpc_nlp_eval_kernel)
template <typename T>
__device__ inline T nlp_gradf_force(const NlpView& V, int c, int k, int i, int e)
{
    const CmpcConsts& K = V.K;
    const float* x = V.x;
    const int N = V.L.N;
    const T g = T(V.gam(c, k));
    T mean = T(0);
    for (int l = 0; l < 4; ++l) mean += T(0.25f) * T(x[V.L.oF(c, l) + 3 * k + i]);
    const T es = T(x[e]) - g * mean, esum = T(4) * mean * (T(1) - g);
    T v = T(2) * T(K.w_sym) * (es - T(0.25f) * g * esum);
    if (k > 0) v += T(K.D[i]) * (T(x[e]) - T(x[e - 3]));
    if (k + 1 < N) v -= T(K.D[i]) * (T(x[e + 3]) - T(x[e]));
    return v;
}

// nlp_grad, x side: d gamma / d x_e
template <typename T>
__device__ inline T nlp_grad_x(const NlpView& V, T lam_f, int e)
{
    const CmpcConsts& K = V.K;
    const CmpcIdx& L = V.L;
    const GLay& G = V.G;
    const float *x = V.x, *p = V.p, *lam = V.lam;
    const int N = L.N;
    const T dt = T(K.dt);
    T v;
    if (e < L.oPos(0)) {  // com | dcom | h : 3 x (N+1) each
        const int blk = e / (3 * (N + 1)), e2 = e % (3 * (N + 1)), k = e2 / 3, i = e2 % 3;
        const int grow = blk == 0 ? G.g_com : (blk == 1 ? G.g_dcom : G.g_h);
        v = T(k == 0 ? lam[G.g_init + 3 * blk + i] : lam[grow + 3 * (k - 1) + i]);
        if (k < N) v -= T(lam[grow + 3 * k + i]);
        if (blk == 0) {
            v += lam_f * (i == 0 ? T(2) * T(K.w_com0) : (i == 1 ? T(2) * T(K.w_com1) : T(K.wz2[k]))) * (T(x[e]) - T(p[L.pComref() + e2]));
            if (k < N) {  // rows g_h: -dt [Fsum]x  ->  -dt (lam_h x Fsum)
                T F0[3], F1[3], Fs[3], lh[3];
                V.fcsum(0, k, F0);
                V.fcsum(1, k, F1);
                for (int a = 0; a < 3; ++a) { Fs[a] = T(V.gam(0, k)) * F0[a] + T(V.gam(1, k)) * F1[a]; lh[a] = T(lam[G.g_h + 3 * k + a]); }
                v -= dt * crossc(lh, Fs, i);
            }
        } else if (blk == 1) {
            if (k < N) v -= dt * T(lam[G.g_com + 3 * k + i]);
        } else v += lam_f * T(2) * T(K.w_h) * (T(x[e]) - T(p[L.pHref() + e2]));
    } else {
        const int c = e < L.oPos(1) ? 0 : 1;
        const int e2 = e - L.oPos(c);
        if (e2 < 3 * (N + 1)) {  // pos
            const int k = e2 / 3, a = e2 % 3;
            v = lam_f * T(2) * T(K.w_pos) * (T(x[e]) - T(p[L.pNom(c) + e2]));
            if (k == 0) v += T(lam[G.g_init + 9 + 3 * c + a]);
            else {
                const float* R = p + L.pR(c) + 9 * (k - 1);
                const float* lb = lam + G.g_bbox[c] + 3 * (k - 1);
                v += T(lam[G.g_pos[c] + 3 * (k - 1) + a]) + T(lb[0]) * T(R[a]) + T(lb[1]) * T(R[3 + a]) + T(lb[2]) * T(R[6 + a]);
            }
            if (k < N) {
                T Fc[3], lh[3];
                V.fcsum(c, k, Fc);
                for (int b = 0; b < 3; ++b) lh[b] = T(lam[G.g_h + 3 * k + b]);
                v += -T(lam[G.g_pos[c] + 3 * k + a]) + dt * T(V.gam(c, k)) * crossc(lh, Fc, a);
            }
        } else if (e2 < 3 * (N + 1) + 3 * N) {  // vel
            const int e3 = e2 - 3 * (N + 1), k = e3 / 3;
            v = -dt * (T(1) - T(V.gam(c, k))) * T(lam[G.g_pos[c] + e3]);
        } else {  // corner forces
            const int e3 = e2 - 3 * (N + 1) - 3 * N, j = e3 / (3 * N), k = (e3 % (3 * N)) / 3, a = e3 % 3;
            const T g = T(V.gam(c, k));
            const float* R = p + L.pR(c) + 9 * k;
            const float* lf = lam + G.g_fric[c] + 16 * k + 4 * j;
            T rr[3], lh[3];
            V.rvec(c, j, k, rr);
            for (int b = 0; b < 3; ++b) lh[b] = T(lam[G.g_h + 3 * k + b]);
            v = lam_f * nlp_gradf_force<T>(V, c, k, a, e) - dt * g * (T(lam[G.g_dcom + 3 * k + a]) + crossc(lh, rr, a));
            const T l0 = T(lf[0]), l1 = T(lf[1]), l2 = T(lf[2]), l3 = T(lf[3]);
            const T cx = l0 - l1 - l2 + l3, cy = l0 + l1 - l2 - l3, cz = -T(K.mu_fr) * (l0 + l1 + l2 + l3);
            v += cx * T(R[a]) + cy * T(R[3 + a]) + cz * T(R[6 + a]);
        }
    }
    return v;
}

// nlp_grad, parameter side: d gamma / d p_e (zero for limA/limB, currentPos, com0/dcom0/h0, which only enter the bounds)
template <typename T>
__device__ inline T nlp_grad_p(const NlpView& V, T lam_f, int e)
{
    const CmpcConsts& K = V.K;
    const CmpcIdx& L = V.L;
    const GLay& G = V.G;
    const float *x = V.x, *p = V.p, *lam = V.lam;
    const int N = L.N;
    const T dt = T(K.dt);
    T v = T(0);
    if (e < L.pCom0()) {
        const int c = e < L.pR(1) ? 0 : 1;
        const int e2 = e - L.pR(c);
        if (e2 < 9 * N) {  // R(a, m) at 9 k + 3 m + a
            const int k = e2 / 9, m = (e2 % 9) / 3, a = e2 % 3;
            const T g = T(V.gam(c, k));
            T lh[3];
            for (int b = 0; b < 3; ++b) lh[b] = T(lam[G.g_h + 3 * k + b]);
            for (int j = 0; j < 4; ++j) {
                T f[3];
                for (int b = 0; b < 3; ++b) f[b] = T(x[L.oF(c, j) + 3 * k + b]);
                const float* lf = lam + G.g_fric[c] + 16 * k + 4 * j;
                const T l0 = T(lf[0]), l1 = T(lf[1]), l2 = T(lf[2]), l3 = T(lf[3]);
                const T coef = m == 0 ? (l0 - l1 - l2 + l3) : (m == 1 ? (l0 + l1 - l2 - l3) : -T(K.mu_fr) * (l0 + l1 + l2 + l3));
                v += -dt * g * T(K.corners[12 * c + 3 * j + m]) * crossc(f, lh, a) + coef * f[a];
            }
            v += T(lam[G.g_bbox[c] + 3 * k + m]) * (T(x[L.oPos(c) + 3 * (k + 1) + a]) - T(p[L.pNom(c) + 3 * (k + 1) + a]));
        } else if (e2 < 15 * N) {
            v = T(0);   // limA, limB
        } else if (e2 < 16 * N) {  // Gamma
            const int k = e2 - 15 * N;
            const T g = T(V.gam(c, k));
            const float* ld = lam + G.g_dcom + 3 * k;
            const float* lh = lam + G.g_h + 3 * k;
            T mean[3] = {T(0), T(0), T(0)}, esum[3];
            for (int j = 0; j < 4; ++j)
                for (int i = 0; i < 3; ++i) mean[i] += T(0.25f) * T(x[L.oF(c, j) + 3 * k + i]);
            for (int i = 0; i < 3; ++i) esum[i] = T(4) * mean[i] * (T(1) - g);
            for (int j = 0; j < 4; ++j) {
                T f[3], rr[3];
                for (int b = 0; b < 3; ++b) f[b] = T(x[L.oF(c, j) + 3 * k + b]);
                V.rvec(c, j, k, rr);
                for (int i = 0; i < 3; ++i) v -= dt * (T(ld[i]) * f[i] + T(lh[i]) * crossc(rr, f, i));
            }
            for (int i = 0; i < 3; ++i)
                v += -lam_f * T(2) * T(K.w_sym) * mean[i] * esum[i] + dt * T(lam[G.g_pos[c] + 3 * k + i]) * T(x[L.oVel(c) + 3 * k + i]);
        } else if (e2 < 16 * N + 3 * (N + 1)) {  // nominalPos
            const int e3 = e2 - 16 * N, k = e3 / 3, a = e3 % 3;
            v = -lam_f * T(2) * T(K.w_pos) * (T(x[L.oPos(c) + e3]) - T(p[e]));
            if (k > 0) {
                const float* R = p + L.pR(c) + 9 * (k - 1);
                const float* lb = lam + G.g_bbox[c] + 3 * (k - 1);
                v -= T(lb[0]) * T(R[a]) + T(lb[1]) * T(R[3 + a]) + T(lb[2]) * T(R[6 + a]);
            }
        }   // currentPos: 0
    } else if (e >= L.pComref() && e < L.pHref()) {
        const int e2 = e - L.pComref(), k = e2 / 3, i = e2 % 3;
        v = -lam_f * (i == 0 ? T(2) * T(K.w_com0) : (i == 1 ? T(2) * T(K.w_com1) : T(K.wz2[k]))) * (T(x[L.oCom() + e2]) - T(p[e]));
    } else if (e >= L.pHref() && e < L.pFext()) {
        v = -lam_f * T(2) * T(K.w_h) * (T(x[L.oH() + e - L.pHref()]) - T(p[e]));
    } else if (e >= L.pFext() && e < L.pText()) {
        v = -dt * T(lam[G.g_dcom + e - L.pFext()]);
    } else if (e >= L.pText()) {
        v = -dt * T(lam[G.g_h + e - L.pText()]);
    }   // com0, dcom0, h0: 0
    return v;
}

__global__ __launch_bounds__(256) void cmpc_nlp_eval_kernel(CmpcParams kp, const float* __restrict__ X, const float* __restrict__ P,
                                                            const float* __restrict__ LamG, float lam_f, float* __restrict__ F,
                                                            float* __restrict__ Gout, float* __restrict__ GradF, float* __restrict__ Jac,
                                                            float* __restrict__ Hess, const int* __restrict__ jdesc,
                                                            const int* __restrict__ hdesc, int nnzj, int nnzh)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, NT = 256;
    const int b = blockIdx.x;
    const int N = kp.N;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kp.kc_per_problem ? kp.kc + b : kp.kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    GLay G;
    glay_init(G, N);
    float* x = reinterpret_cast<float*>(smem + ((sizeof(CmpcConsts) + 15) & ~15));
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    float* red = lam + ((L.ng() + 3) & ~3);
    for (int e = tid; e < L.nx(); e += NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += NT) p[e] = P[(size_t)b * L.np() + e];
    if (LamG) for (int e = tid; e < L.ng(); e += NT) lam[e] = LamG[(size_t)b * L.ng() + e];
    __syncthreads();
    const float dt = K.dt;

    auto gam = [&](int c, int k) { return p[L.pGam(c) + k]; };
    auto rvec = [&](int c, int j, int k, float* r) {
        const float* R = p + L.pR(c) + 9 * k;
        const float* cn = K.corners + 12 * c + 3 * j;
        for (int i = 0; i < 3; ++i)
            r[i] = R[i] * cn[0] + R[3 + i] * cn[1] + R[6 + i] * cn[2] + x[L.oPos(c) + 3 * k + i] - x[L.oCom() + 3 * k + i];
    };
    auto fcsum = [&](int c, int k, float* Fc) {
        for (int i = 0; i < 3; ++i)
            Fc[i] = x[L.oF(c, 0) + 3 * k + i] + x[L.oF(c, 1) + 3 * k + i] + x[L.oF(c, 2) + 3 * k + i] + x[L.oF(c, 3) + 3 * k + i];
    };

    const NlpView V{K, L, G, x, p, lam};
    // ---------------- f ----------------
    if (F) {
        float acc = nlp_f_part<float>(V, tid, NT);
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) F[b] = red[0] + red[1] + red[2] + red[3];
    }
    // ---------------- g ----------------
    if (Gout) {
        float* g = Gout + (size_t)b * L.ng();
        for (int r = tid; r < L.ng(); r += NT) g[r] = nlp_g_row<float>(V, r);
    }
    // ---------------- grad f ----------------
    if (GradF) {
        float* gf = GradF + (size_t)b * L.nx();
        for (int e = tid; e < L.nx(); e += NT) {
            float v = 0.f;
            if (e < L.oDcom()) {
                const int k = e / 3, i = e % 3;
                v = (i == 0 ? 2.f * K.w_com0 : (i == 1 ? 2.f * K.w_com1 : K.wz2[k])) * (x[e] - p[L.pComref() + e]);
            } else if (e < L.oH()) {
                v = 0.f;
            } else if (e < L.oPos(0)) {
                v = 2.f * K.w_h * (x[e] - p[L.pHref() + e - L.oH()]);
            } else {
                const int c = e < L.oPos(1) ? 0 : 1;
                const int e2 = e - L.oPos(c);
                if (e2 < 3 * (N + 1)) v = 2.f * K.w_pos * (x[e] - p[L.pNom(c) + e2]);
                else if (e2 < 3 * (N + 1) + 3 * N) v = 0.f;
                else {
                    const int e3 = e2 - 3 * (N + 1) - 3 * N, j = e3 / (3 * N), k = (e3 % (3 * N)) / 3, i = e3 % 3;
                    const float g = gam(c, k);
                    float mean = 0.f;
                    for (int l = 0; l < 4; ++l) mean += 0.25f * x[L.oF(c, l) + 3 * k + i];
                    const float es = x[e] - g * mean, esum = 4.f * mean * (1.f - g);
                    v = 2.f * K.w_sym * (es - 0.25f * g * esum);
                    if (k > 0) v += K.D[i] * (x[e] - x[e - 3]);
                    if (k + 1 < N) v -= K.D[i] * (x[e + 3] - x[e]);
                    (void)j;
                }
            }
            gf[e] = v;
        }
    }
    // ---------------- jac g (CCS order) ----------------
    if (Jac) {
        float* jo = Jac + (size_t)b * nnzj;
        for (int e = tid; e < nnzj; e += NT) {
            const int d = jdesc[e];
            const int kind = d & 15, k = (d >> 4) & 63, c = (d >> 10) & 1, j = (d >> 11) & 3, a = (d >> 13) & 3, bb = (d >> 15) & 3,
                      face = (d >> 17) & 3;
            float v;
            switch (kind) {
                case J_ONE: v = 1.f; break;
                case J_MONE: v = -1.f; break;
                case J_MDT: v = -dt; break;
                case J_DCOM_F: v = -dt * gam(c, k); break;
                case J_H_F: {
                    float rr[3];
                    rvec(c, j, k, rr);
                    v = -dt * gam(c, k) * skew(rr, a, bb);
                } break;
                case J_H_POS: {
                    float Fc[3];
                    fcsum(c, k, Fc);
                    v = dt * gam(c, k) * skew(Fc, a, bb);
                } break;
                case J_H_COM: {
                    float F0[3], F1[3], Fs[3];
                    fcsum(0, k, F0);
                    fcsum(1, k, F1);
                    for (int i = 0; i < 3; ++i) Fs[i] = gam(0, k) * F0[i] + gam(1, k) * F1[i];
                    v = -dt * skew(Fs, a, bb);
                } break;
                case J_POS_VEL: v = -dt * (1.f - gam(c, k)); break;
                case J_BBOX: v = p[L.pR(c) + 9 * k + 3 * a + bb]; break;  // a = bbox row i, bb = pos component
                default: {  // J_FRIC: bb = force component
                    const float* R = p + L.pR(c) + 9 * k;
                    const float sx = (face == 0 || face == 3) ? 1.f : -1.f, sy = face < 2 ? 1.f : -1.f;
                    v = sx * R[bb] + sy * R[3 + bb] - K.mu_fr * R[6 + bb];
                } break;
            }
            jo[e] = v;
        }
    }
    // ---------------- hess L (CCS order, full symmetric) ----------------
    if (Hess) {
        GLay Gl = G;
        float* ho = Hess + (size_t)b * nnzh;
        for (int e = tid; e < nnzh; e += NT) {
            const int d = hdesc[e];
            const int kind = d & 15, k = (d >> 4) & 63, c = (d >> 10) & 1, j = (d >> 11) & 3, a = (d >> 13) & 3, bb = (d >> 15) & 3,
                      l = (d >> 17) & 3;
            float v;
            switch (kind) {
                case H_COMX: v = lam_f * 2.f * K.w_com0; break;
                case H_COMY: v = lam_f * 2.f * K.w_com1; break;
                case H_COMZ: v = lam_f * K.wz2[k]; break;
                case H_H: v = lam_f * 2.f * K.w_h; break;
                case H_POS: v = lam_f * 2.f * K.w_pos; break;
                case H_FF: {
                    const float g = gam(c, k);
                    v = 2.f * K.w_sym * ((j == l ? 1.f : 0.f) - 0.25f * g * (2.f - g));
                    if (j == l) v += K.D[a] * (float)((k > 0) + (k + 1 < N));
                    v *= lam_f;
                } break;
                case H_RATE: v = -lam_f * K.D[a]; break;
                default: {
                    const float* lh = lam + Gl.g_h + 3 * k;
                    const float s = dt * gam(c, k) * skew(lh, a, bb);
                    v = (kind == H_F_POS) ? -s : s;
                } break;
            }
            ho[e] = v;
        }
    }
}

// nlp_grad (tmp.c:24791-58842): gradient of gamma = lam_f f + lam_g^T g with respect to x and to p, batched.  One
// workgroup per problem, x / p / lam_g staged in LDS, every output element one thread's closed form (J^T lam_g is
// written out per x-block instead of scattering the Jacobian's non-zeros).  Parameter blocks that do not enter f or g
// (limA, limB, currentPos, com0, dcom0, h0: CasADi's Opti turns them into bounds) get zeros, as in the reference.
__global__ __launch_bounds__(256) void cmpc_nlp_grad_kernel(CmpcParams kp, const float* __restrict__ X, const float* __restrict__ P,
                                                            const float* __restrict__ LamG, float lam_f, float* __restrict__ GradX,
                                                            float* __restrict__ GradP)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, NT = 256;
    const int b = blockIdx.x;
    const int N = kp.N;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kp.kc_per_problem ? kp.kc + b : kp.kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    GLay G;
    glay_init(G, N);
    float* x = reinterpret_cast<float*>(smem + ((sizeof(CmpcConsts) + 15) & ~15));
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    for (int e = tid; e < L.nx(); e += NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += NT) p[e] = P[(size_t)b * L.np() + e];
    for (int e = tid; e < L.ng(); e += NT) lam[e] = LamG[(size_t)b * L.ng() + e];
    __syncthreads();
    const NlpView V{K, L, G, x, p, lam};
    if (GradX) {
        float* gx = GradX + (size_t)b * L.nx();
        for (int e = tid; e < L.nx(); e += NT) gx[e] = nlp_grad_x<float>(V, lam_f, e);
    }
    if (GradP) {
        float* gp = GradP + (size_t)b * L.np();
        for (int e = tid; e < L.np(); e += NT) gp[e] = nlp_grad_p<float>(V, lam_f, e);
    }
}

// ---- the solver's dual record -> lam_g in the reference's row order (cmpc_get_multipliers_device; the derivation: DESIGN.md, "Multipliers").  Record of a
// problem (phase_export, cmpc_solver.hip): [NS (N+1) costates | NI N slacks | NI N multipliers], word 0 = status of the solve; the costate lam_{k+1} of
// the solver belongs to L_s = f + sum lam_{k+1}^T (phi_k - s_{k+1}), the reference's rows are s_{k+1} - phi_k: lam_g = -lam_{k+1}.  One workgroup per
// problem: the rows from the record (coalesced), then the 15 initial-condition rows from stationarity at the stage-0 columns, through nlp_grad. ----
__global__ __launch_bounds__(256) void cmpc_multipliers_kernel(CmpcParams kp, const float* __restrict__ X, const float* __restrict__ P,
                                                               const float* __restrict__ D, float* __restrict__ LamG)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, NT = 256;
    const int b = blockIdx.x;
    const int N = kp.N;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kp.kc_per_problem ? kp.kc + b : kp.kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    GLay G;
    glay_init(G, N);
    float* x = reinterpret_cast<float*>(smem + ((sizeof(CmpcConsts) + 15) & ~15));
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    const float* rec = D + (size_t)b * (CMPC_NS * (N + 1) + 2 * CMPC_NI * N);
    const float* lamS = rec;                                        // costates [N+1][NS]
    const float* zr = rec + CMPC_NS * (N + 1) + CMPC_NI * N;        // multipliers [N][NI]
    float* out = LamG + (size_t)b * L.ng();
    if (rec[0] == 3.f) {   // outside the supported subset: not solved, no multipliers
        for (int r = tid; r < L.ng(); r += NT) out[r] = 0.f;
        return;
    }
    for (int e = tid; e < L.nx(); e += NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += NT) p[e] = P[(size_t)b * L.np() + e];
    __syncthreads();
    for (int r = tid; r < L.ng(); r += NT) {
        float v = 0.f;   // (initial-condition rows: below)
        if (r >= G.g_com && r < G.g_pos[0]) {            // g_com | g_dcom | g_h
            const int blk = (r - G.g_com) / (3 * N), e = (r - G.g_com) % (3 * N), k = e / 3, a = e % 3;
            v = -lamS[CMPC_NS * (k + 1) + 3 * blk + a];
        } else if (r >= G.g_pos[0] && r < G.g_bbox[0]) {  // g_pos[c]: the foot's costate in stance; 0 in swing (vel is free and costs nothing)
            const int c = r < G.g_pos[1] ? 0 : 1, e = r - G.g_pos[c], k = e / 3, a = e % 3;
            v = p[L.pGam(c) + k] >= 0.5f ? -lamS[CMPC_NS * (k + 1) + 9 + 3 * c + a] : 0.f;
        } else if (r >= G.g_bbox[0]) {
            const int c = r < G.g_bbox[1] ? 0 : 1;
            if (r < G.g_fric[c]) {                        // g_bbox[c]
                const int e = r - G.g_bbox[c], k = e / 3, i = e % 3;
                const float lo = p[L.pLo(c) + 3 * k + i], hi = p[L.pUp(c) + 3 * k + i];
                if (p[L.pGam(c) + k] >= 0.5f) v = 0.f;   // stance: the multiplier sits on the landing row (convention, include/cmpc.h)
                else if (hi - lo > 1e-9f) v = zr[CMPC_NI * k + 32 + 3 * c + i] - zr[CMPC_NI * k + 38 + 3 * c + i];   // free offset: zU - zL
                else {                                    // lower == upper, eliminated: stationarity in the landing position, lam = -R^T lam_pos
                    const float* R = p + L.pR(c) + 9 * k;
                    const float* lp = lamS + CMPC_NS * (k + 1) + 9 + 3 * c;
                    v = -(R[3 * i] * lp[0] + R[3 * i + 1] * lp[1] + R[3 * i + 2] * lp[2]);
                }
            } else {                                      // g_fric[c]: the same rows, the same order
                const int e = r - G.g_fric[c], k = e / 16;
                v = zr[CMPC_NI * k + 16 * c + e % 16];
            }
        }
        lam[r] = v;
    }
    __syncthreads();
    // initial-condition rows (Jacobian: identity on com_0, dcom_0, h_0, pos_0): lam_init = -d(f + lam'^T g)/dx on those columns, lam' = lam without them
    if (tid < 15) {
        const int e = tid < 9 ? (tid / 3) * 3 * (N + 1) + tid % 3 : L.oPos((tid - 9) / 3) + (tid - 9) % 3;
        const NlpView V{K, L, G, x, p, lam};
        out[tid] = (float)-nlp_grad_x<double>(V, 1.0, e);
    }
    for (int r = 15 + tid; r < L.ng(); r += NT) out[r] = lam[r];
}

// block reductions of the certificate (256 threads): max and sum in double
__device__ inline double blk_max(double v, double* red, int tid)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
__device__ inline double blk_sum(double v, double* red, int tid)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// bounds of row r of g as functions of p (CasADi's Opti turns `param == expr` and `lo <= expr <= hi` into these): init rows = com0 dcom0 h0 currentPos,
// dynamics rows 0, box rows [lower, upper], friction rows (-inf, 0]
__device__ inline void nlp_bounds_row(const CmpcIdx& L, const GLay& G, const float* p, int r, double& lb, double& ub)
{
    if (r < 15) { lb = ub = (double)(r < 9 ? p[L.pCom0() + r] : p[L.pCur((r - 9) / 3) + (r - 9) % 3]); return; }
    if (r < G.g_bbox[0]) { lb = ub = 0.0; return; }
    const int c = r < G.g_bbox[1] ? 0 : 1;
    if (r < G.g_fric[c]) { const int e = r - G.g_bbox[c]; lb = p[L.pLo(c) + e]; ub = p[L.pUp(c) + e]; return; }
    lb = -INFINITY; ub = 0.0;
}

// ---- KKT certificate of the reference NLP at (x, lam_g), one workgroup per problem, residuals in double (kkt_report of tests/golden/
// make_argmin_ref_golden.py, which certified the goldens) -> cert[CMPC_CERT] (include/cmpc.h) ----
__global__ __launch_bounds__(256) void cmpc_kkt_certificate_kernel(CmpcParams kp, const float* __restrict__ X, const float* __restrict__ P,
                                                                   const float* __restrict__ LamG, const float* __restrict__ D, float* __restrict__ Cert)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, NT = 256;
    const int b = blockIdx.x;
    const int N = kp.N;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kp.kc_per_problem ? kp.kc + b : kp.kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    GLay G;
    glay_init(G, N);
    float* x = reinterpret_cast<float*>(smem + ((sizeof(CmpcConsts) + 15) & ~15));
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    double* red = reinterpret_cast<double*>(lam + ((L.ng() + 3) & ~3));
    for (int e = tid; e < L.nx(); e += NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += NT) p[e] = P[(size_t)b * L.np() + e];
    for (int e = tid; e < L.ng(); e += NT) lam[e] = LamG[(size_t)b * L.ng() + e];
    __syncthreads();
    const NlpView V{K, L, G, x, p, lam};
    double lmax = 0.0;
    for (int r = tid; r < L.ng(); r += NT) lmax = fmax(lmax, fabs((double)lam[r]));
    const double scale = fmax(1.0, blk_max(lmax, red, tid));
    double st = 0.0;
    for (int e = tid; e < L.nx(); e += NT) st = fmax(st, fabs(nlp_grad_x<double>(V, 1.0, e)));
    double inf = 0.0, cmp = 0.0, sgn = 0.0;
    for (int r = tid; r < L.ng(); r += NT) {
        double lb, ub;
        nlp_bounds_row(L, G, p, r, lb, ub);
        const double g = nlp_g_row<double>(V, r), l = lam[r];
        inf = fmax(inf, fmax(lb - g, g - ub));
        if (ub - lb > 1e-12) {   // inequality rows
            cmp = fmax(cmp, fabs(l * fmin(g - lb, ub - g)));
            // sign of the multiplier (lam^T g enters the Lagrangian with +): >= 0 on a row bounded above only, <= 0 below only, the sign of the nearer
            // bound on a two-sided row
            const bool up = lb < -1e19 ? true : (ub > 1e19 ? false : (ub - g) < (g - lb));
            sgn = fmax(sgn, up ? -l : l);
        }
    }
    const double f = blk_sum(nlp_f_part<double>(V, tid, NT), red, tid);
    st = blk_max(st, red, tid);
    inf = blk_max(inf, red, tid);
    cmp = blk_max(cmp, red, tid);
    sgn = blk_max(sgn, red, tid);
    if (tid == 0) {
        float* o = Cert + (size_t)b * CMPC_CERT;
        o[0] = (float)(st / scale); o[1] = (float)fmax(inf, 0.0); o[2] = (float)(cmp / scale); o[3] = (float)(fmax(sgn, 0.0) / scale);
        o[4] = (float)f; o[5] = D ? D[(size_t)b * (CMPC_NS * (N + 1) + 2 * CMPC_NI * N)] : -1.f; o[6] = (float)scale; o[7] = (float)st;
    }
}

// ---- dV*/dp = grad_p L(x, lam_g) (nlp_grad) + the terms of the parameters that only enter the bounds: -lam on com0 dcom0 h0 currentPos (initial-
// condition rows), -max(lam, 0) on upper and -min(lam, 0) on lower (box rows).  Double arithmetic, one workgroup per problem. ----
__global__ __launch_bounds__(256) void cmpc_value_gradient_kernel(CmpcParams kp, const float* __restrict__ X, const float* __restrict__ P,
                                                                  const float* __restrict__ LamG, float* __restrict__ GradP)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, NT = 256;
    const int b = blockIdx.x;
    const int N = kp.N;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kp.kc_per_problem ? kp.kc + b : kp.kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    GLay G;
    glay_init(G, N);
    float* x = reinterpret_cast<float*>(smem + ((sizeof(CmpcConsts) + 15) & ~15));
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    for (int e = tid; e < L.nx(); e += NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += NT) p[e] = P[(size_t)b * L.np() + e];
    for (int e = tid; e < L.ng(); e += NT) lam[e] = LamG[(size_t)b * L.ng() + e];
    __syncthreads();
    const NlpView V{K, L, G, x, p, lam};
    float* gp = GradP + (size_t)b * L.np();
    for (int e = tid; e < L.np(); e += NT) {
        double v;
        if (e >= L.pCom0() && e < L.pComref()) v = -(double)lam[G.g_init + e - L.pCom0()];
        else {
            v = nlp_grad_p<double>(V, 1.0, e);
            if (e < L.pCom0()) {
                const int c = e < L.pR(1) ? 0 : 1, e2 = e - L.pR(c);
                if (e2 >= 9 * N && e2 < 12 * N) v = -fmax((double)lam[G.g_bbox[c] + e2 - 9 * N], 0.0);          // upper
                else if (e2 >= 12 * N && e2 < 15 * N) v = -fmin((double)lam[G.g_bbox[c] + e2 - 12 * N], 0.0);   // lower
                else if (e2 >= 19 * N + 3) v = -(double)lam[G.g_init + 9 + 3 * c + e2 - (19 * N + 3)];        // currentPos
            }
        }
        gp[e] = (float)v;
    }
}

// knot k's share of dV*/dtheta_t = d_theta f + lam^T d_theta g for field t of cmpc_model's packed order (include/cmpc.h, "model directions"): the
// weights through f (com_weight[2] as wz2(k) = 2 w_z(k)^2, d wz2 / d w_cz = sqrt(2 wz2) (1 + e^-k), at the problem's float32 record), friction
// through the friction rows (-(R^T f)_z), corner (c, j, b) through the angular-momentum rows (-dt gam (R e_b) x f)
template <typename T>
__device__ inline T nlp_model_grad_knot(const NlpView& V, int t, int k)
{
    const CmpcConsts& K = V.K;
    const CmpcIdx& L = V.L;
    const GLay& G = V.G;
    const float *x = V.x, *p = V.p, *lam = V.lam;
    const int N = L.N;
    T v = T(0);
    if (t >= 1 && t <= 3) {
        const int i = t - 1;
        const T ec = T(x[L.oCom() + 3 * k + i]) - T(p[L.pComref() + 3 * k + i]);
        const T w = i < 2 ? T(1) : T(0.5) * T(sqrt(2.0 * (double)K.wz2[k]) * (1.0 + exp(-(double)k)));
        return w * ec * ec;
    }
    if (t == 4 || t == 5) {
        for (int i = 0; i < 3; ++i) {
            if (t == 4) { const T e = T(x[L.oH() + 3 * k + i]) - T(p[L.pHref() + 3 * k + i]); v += e * e; }
            else
                for (int c = 0; c < 2; ++c) { const T e = T(x[L.oPos(c) + 3 * k + i]) - T(p[L.pNom(c) + 3 * k + i]); v += e * e; }
        }
        return v;
    }
    if (k >= N) return v;
    if (t == 0) {   // lam_fric^T d g_fric / d mu = -sum lam (R^T f)_z
        for (int c = 0; c < 2; ++c) {
            const float* R = p + L.pR(c) + 9 * k;
            for (int j = 0; j < 4; ++j) {
                const float* f = x + L.oF(c, j) + 3 * k;
                const T fl2 = T(R[6]) * T(f[0]) + T(R[7]) * T(f[1]) + T(R[8]) * T(f[2]);
                const float* lf = lam + G.g_fric[c] + 16 * k + 4 * j;
                v -= (T(lf[0]) + T(lf[1]) + T(lf[2]) + T(lf[3])) * fl2;
            }
        }
        return v;
    }
    if (t >= 6 && t <= 9) {
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < 3; ++i) {
                if (t < 9 && i != t - 6) continue;
                T mean = T(0);
                for (int j = 0; j < 4; ++j) mean += T(0.25f) * T(x[L.oF(c, j) + 3 * k + i]);
                for (int j = 0; j < 4; ++j) {
                    const T fv = T(x[L.oF(c, j) + 3 * k + i]);
                    if (t == 9) { const T es = fv - T(V.gam(c, k)) * mean; v += es * es; }
                    else if (k + 1 < N) { const T d = T(x[L.oF(c, j) + 3 * (k + 1) + i]) - fv; v += d * d; }
                }
            }
        return v;
    }
    const int c = (t - 10) / 12, j = ((t - 10) % 12) / 3, b = (t - 10) % 3;   // corner (c, j), axis b
    const float* R = p + L.pR(c) + 9 * k;
    const T rb[3] = {T(R[3 * b]), T(R[3 * b + 1]), T(R[3 * b + 2])}, f[3] = {T(x[L.oF(c, j) + 3 * k]), T(x[L.oF(c, j) + 3 * k + 1]),
                                                                           T(x[L.oF(c, j) + 3 * k + 2])};
    for (int i = 0; i < 3; ++i) v -= T(lam[G.g_h + 3 * k + i]) * T(K.dt) * T(V.gam(c, k)) * crossc(rb, f, i);
    return v;
}

// ---- dV*/dtheta of the per-problem model at (x, lam_g) (envelope theorem), double arithmetic, one workgroup per problem: items (field, knot) spread
// over the team, partial sums in LDS after the staged lam_g, one thread per field adds its knots in order.  A record whose model broke the model rule
// gets zeros. ----
__global__ __launch_bounds__(256) void cmpc_model_value_gradient_kernel(CmpcParams kp, const float* __restrict__ X, const float* __restrict__ P,
                                                                        const float* __restrict__ LamG, double* __restrict__ GradM)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, NT = 256;
    const int b = blockIdx.x;
    const int N = kp.N, M = CMPC_MODEL_DOUBLES, nk = N + 1;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kp.kc_per_problem ? kp.kc + b : kp.kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    GLay G;
    glay_init(G, N);
    float* x = reinterpret_cast<float*>(smem + ((sizeof(CmpcConsts) + 15) & ~15));
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    double* part = reinterpret_cast<double*>(lam + ((L.ng() + 3) & ~3) + 8);
    for (int e = tid; e < L.nx(); e += NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += NT) p[e] = P[(size_t)b * L.np() + e];
    for (int e = tid; e < L.ng(); e += NT) lam[e] = LamG[(size_t)b * L.ng() + e];
    __syncthreads();
    double* out = GradM + (size_t)b * M;
    if (K.model_bad) {
        for (int t = tid; t < M; t += NT) out[t] = 0.0;
        return;
    }
    const NlpView V{K, L, G, x, p, lam};
    for (int e = tid; e < M * nk; e += NT) part[e] = nlp_model_grad_knot<double>(V, e / nk, e % nk);
    __syncthreads();
    for (int t = tid; t < M; t += NT) {
        double v = 0.0;
        for (int k = 0; k < nk; ++k) v += part[t * nk + k];
        out[t] = v;
    }
}

// dV*/domega_{c,k} = lam^T d_omega g (axis a) for the rotation direction dR_{c,k} = R_{c,k} [omega]x (include/cmpc.h, "rotation directions"; f does not
// depend on R).  g is linear in R's entries, so the row's derivative is the row itself with R [e_a]x in R's place: the angular-momentum rows through
// the lever arm, -dt gam (R (e_a x cn)) x f; the friction rows, al . (R^T f x e_a); the box rows (every stage: stance rows carry lam = 0 under the
// export convention), -(e_a x R^T (pos_{k+1} - nom_{k+1}))
template <typename T>
__device__ inline T nlp_rot_grad(const NlpView& V, int c, int k, int a)
{
    const CmpcConsts& K = V.K;
    const CmpcIdx& L = V.L;
    const GLay& G = V.G;
    const float *x = V.x, *p = V.p, *lam = V.lam;
    const float* R = p + L.pR(c) + 9 * k;   // column-major: R(r, m) = R[3 m + r]
    T ea[3] = {T(0), T(0), T(0)};
    ea[a] = T(1);
    T v = T(0);
    T lh[3];
    for (int i = 0; i < 3; ++i) lh[i] = T(lam[G.g_h + 3 * k + i]);
    for (int j = 0; j < 4; ++j) {
        const float* cn = K.corners + 12 * c + 3 * j;
        const float* fp = x + L.oF(c, j) + 3 * k;
        const T f[3] = {T(fp[0]), T(fp[1]), T(fp[2])};
        const T cnT[3] = {T(cn[0]), T(cn[1]), T(cn[2])};
        T wc[3], rw[3], fl[3], flw[3];
        for (int i = 0; i < 3; ++i) wc[i] = crossc(ea, cnT, i);
        for (int i = 0; i < 3; ++i) rw[i] = T(R[i]) * wc[0] + T(R[3 + i]) * wc[1] + T(R[6 + i]) * wc[2];
        for (int i = 0; i < 3; ++i) v -= lh[i] * T(K.dt) * T(V.gam(c, k)) * crossc(rw, f, i);
        for (int m = 0; m < 3; ++m) fl[m] = T(R[3 * m]) * f[0] + T(R[3 * m + 1]) * f[1] + T(R[3 * m + 2]) * f[2];
        for (int i = 0; i < 3; ++i) flw[i] = crossc(fl, ea, i);
        const float* lf = lam + G.g_fric[c] + 16 * k + 4 * j;
        for (int face = 0; face < 4; ++face) {
            const T sx = (face == 0 || face == 3) ? T(1) : T(-1), sy = face < 2 ? T(1) : T(-1);
            v += T(lf[face]) * (sx * flw[0] + sy * flw[1] - T(K.mu_fr) * flw[2]);
        }
    }
    T q[3];
    for (int i = 0; i < 3; ++i) {
        q[i] = T(0);
        for (int r = 0; r < 3; ++r) q[i] += T(R[3 * i + r]) * (T(x[L.oPos(c) + 3 * (k + 1) + r]) - T(p[L.pNom(c) + 3 * (k + 1) + r]));
    }
    for (int i = 0; i < 3; ++i) v -= T(lam[G.g_bbox[c] + 3 * k + i]) * crossc(ea, q, i);
    return v;
}

// ---- dV*/domega of the stage rotations at (x, lam_g) (envelope theorem), double arithmetic, one workgroup per problem, one item per (foot, stage, axis):
// out[2][N][3].  A record whose model broke the model rule gets zeros. ----
__global__ __launch_bounds__(256) void cmpc_rotation_value_gradient_kernel(CmpcParams kp, const float* __restrict__ X, const float* __restrict__ P,
                                                                           const float* __restrict__ LamG, double* __restrict__ GradR)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, NT = 256;
    const int b = blockIdx.x;
    const int N = kp.N;
    CmpcConsts& K = *reinterpret_cast<CmpcConsts*>(smem);
    {
        const int* src = reinterpret_cast<const int*>(kp.kc_per_problem ? kp.kc + b : kp.kc);
        int* dst = reinterpret_cast<int*>(smem);
        for (int e = tid; e < (int)(sizeof(CmpcConsts) / 4); e += NT) dst[e] = src[e];
    }
    const CmpcIdx L{N};
    GLay G;
    glay_init(G, N);
    float* x = reinterpret_cast<float*>(smem + ((sizeof(CmpcConsts) + 15) & ~15));
    float* p = x + ((L.nx() + 3) & ~3);
    float* lam = p + ((L.np() + 3) & ~3);
    for (int e = tid; e < L.nx(); e += NT) x[e] = X[(size_t)b * L.nx() + e];
    for (int e = tid; e < L.np(); e += NT) p[e] = P[(size_t)b * L.np() + e];
    for (int e = tid; e < L.ng(); e += NT) lam[e] = LamG[(size_t)b * L.ng() + e];
    __syncthreads();
    double* out = GradR + (size_t)b * 6 * N;
    const NlpView V{K, L, G, x, p, lam};
    for (int e = tid; e < 6 * N; e += NT) out[e] = K.model_bad ? 0.0 : nlp_rot_grad<double>(V, e / (3 * N), (e / 3) % N, e % 3);
}

void build_sparsity(int N, std::vector<Trip>& J, std::vector<Trip>& H)
{
    CmpcLayout L;
    cmpc_layout_init(L, N);
    GLay G;
    glay_init(G, N);
    J.clear(); H.clear();
    for (int i = 0; i < 3; ++i) {
        J.push_back({G.g_init + i, L.o_com + i, mk(J_ONE, 0)});
        J.push_back({G.g_init + 3 + i, L.o_dcom + i, mk(J_ONE, 0)});
        J.push_back({G.g_init + 6 + i, L.o_h + i, mk(J_ONE, 0)});
        J.push_back({G.g_init + 9 + i, L.o_pos[0] + i, mk(J_ONE, 0)});
        J.push_back({G.g_init + 12 + i, L.o_pos[1] + i, mk(J_ONE, 0)});
    }
    for (int k = 0; k < N; ++k) {
        for (int i = 0; i < 3; ++i) {
            J.push_back({G.g_com + 3 * k + i, L.o_com + 3 * (k + 1) + i, mk(J_ONE, k)});
            J.push_back({G.g_com + 3 * k + i, L.o_com + 3 * k + i, mk(J_MONE, k)});
            J.push_back({G.g_com + 3 * k + i, L.o_dcom + 3 * k + i, mk(J_MDT, k)});
            J.push_back({G.g_dcom + 3 * k + i, L.o_dcom + 3 * (k + 1) + i, mk(J_ONE, k)});
            J.push_back({G.g_dcom + 3 * k + i, L.o_dcom + 3 * k + i, mk(J_MONE, k)});
            J.push_back({G.g_h + 3 * k + i, L.o_h + 3 * (k + 1) + i, mk(J_ONE, k)});
            J.push_back({G.g_h + 3 * k + i, L.o_h + 3 * k + i, mk(J_MONE, k)});
        }
        for (int c = 0; c < 2; ++c) {
            for (int j = 0; j < 4; ++j) {
                for (int i = 0; i < 3; ++i) J.push_back({G.g_dcom + 3 * k + i, L.o_f[c][j] + 3 * k + i, mk(J_DCOM_F, k, c, j)});
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b)
                        if (a != b) J.push_back({G.g_h + 3 * k + a, L.o_f[c][j] + 3 * k + b, mk(J_H_F, k, c, j, a, b)});
                for (int face = 0; face < 4; ++face)
                    for (int b = 0; b < 3; ++b)
                        J.push_back({G.g_fric[c] + 16 * k + 4 * j + face, L.o_f[c][j] + 3 * k + b, mk(J_FRIC, k, c, j, 0, b, face)});
            }
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b)
                    if (a != b) J.push_back({G.g_h + 3 * k + a, L.o_pos[c] + 3 * k + b, mk(J_H_POS, k, c, 0, a, b)});
            for (int i = 0; i < 3; ++i) {
                J.push_back({G.g_pos[c] + 3 * k + i, L.o_pos[c] + 3 * (k + 1) + i, mk(J_ONE, k)});
                J.push_back({G.g_pos[c] + 3 * k + i, L.o_pos[c] + 3 * k + i, mk(J_MONE, k)});
                J.push_back({G.g_pos[c] + 3 * k + i, L.o_vel[c] + 3 * k + i, mk(J_POS_VEL, k, c)});
                for (int a = 0; a < 3; ++a) J.push_back({G.g_bbox[c] + 3 * k + i, L.o_pos[c] + 3 * (k + 1) + a, mk(J_BBOX, k, c, 0, i, a)});
            }
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                if (a != b) J.push_back({G.g_h + 3 * k + a, L.o_com + 3 * k + b, mk(J_H_COM, k, 0, 0, a, b)});
    }
    for (int k = 0; k <= N; ++k) {
        H.push_back({L.o_com + 3 * k, L.o_com + 3 * k, mk(H_COMX, k)});
        H.push_back({L.o_com + 3 * k + 1, L.o_com + 3 * k + 1, mk(H_COMY, k)});
        H.push_back({L.o_com + 3 * k + 2, L.o_com + 3 * k + 2, mk(H_COMZ, k)});
        for (int i = 0; i < 3; ++i) {
            H.push_back({L.o_h + 3 * k + i, L.o_h + 3 * k + i, mk(H_H, k)});
            for (int c = 0; c < 2; ++c) H.push_back({L.o_pos[c] + 3 * k + i, L.o_pos[c] + 3 * k + i, mk(H_POS, k)});
        }
    }
    for (int k = 0; k < N; ++k)
        for (int c = 0; c < 2; ++c)
            for (int j = 0; j < 4; ++j) {
                const int fj = L.o_f[c][j] + 3 * k;
                for (int l = 0; l < 4; ++l)
                    for (int i = 0; i < 3; ++i) H.push_back({fj + i, L.o_f[c][l] + 3 * k + i, mk(H_FF, k, c, j, i, 0, l)});
                if (k + 1 < N)
                    for (int i = 0; i < 3; ++i) {
                        H.push_back({fj + i, fj + 3 + i, mk(H_RATE, k, c, j, i)});
                        H.push_back({fj + 3 + i, fj + i, mk(H_RATE, k, c, j, i)});
                    }
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) {
                        if (a == b) continue;
                        H.push_back({fj + a, L.o_pos[c] + 3 * k + b, mk(H_F_POS, k, c, j, a, b)});
                        H.push_back({L.o_pos[c] + 3 * k + b, fj + a, mk(H_F_POS, k, c, j, a, b)});
                        H.push_back({fj + a, L.o_com + 3 * k + b, mk(H_F_COM, k, c, j, a, b)});
                        H.push_back({L.o_com + 3 * k + b, fj + a, mk(H_F_COM, k, c, j, a, b)});
                    }
            }
    auto ccs = [](const Trip& u, const Trip& v) { return u.col != v.col ? u.col < v.col : u.row < v.row; };
    std::sort(J.begin(), J.end(), ccs);
    std::sort(H.begin(), H.end(), ccs);
}

struct DescCache {
    int N = -1, device = -1;
    int *dJ = nullptr, *dH = nullptr;
    int nnzj = 0, nnzh = 0;
};
DescCache g_cache;

}  // namespace

extern "C" int cmpc_nlp_sparsity(int N, int* jac_row, int* jac_col, int* hess_row, int* hess_col)
{
    if (N < 1 || N > CMPC_NMAX) return -1;
    std::vector<Trip> J, H;
    build_sparsity(N, J, H);
    for (size_t i = 0; i < J.size(); ++i) {
        if (jac_row) jac_row[i] = J[i].row;
        if (jac_col) jac_col[i] = J[i].col;
    }
    for (size_t i = 0; i < H.size(); ++i) {
        if (hess_row) hess_row[i] = H[i].row;
        if (hess_col) hess_col[i] = H[i].col;
    }
    return 0;
}

// dynamic LDS of the NLP kernels: the constants, x, p, lam_g and a 32-byte reduction area (cmpc_nlp_eval_kernel, cmpc_nlp_grad_kernel and the kernels of
// the multiplier interface share the layout)
static size_t nlp_lds_bytes(int N)
{
    CmpcLayout L;
    cmpc_layout_init(L, N);
    return ((sizeof(CmpcConsts) + 15) & ~(size_t)15) + 4 * (size_t)(((L.nx + 3) & ~3) + ((L.np + 3) & ~3) + ((L.ng + 3) & ~3) + 8);
}

extern "C" int cmpc_launch_nlp_eval(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, float lam_f,
                                    float* dF, float* dG, float* dGradF, float* dJac, float* dHess, hipStream_t stream)
{
    const int N = prm->N;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (g_cache.N != N || g_cache.device != dev) {
        std::vector<Trip> J, H;
        build_sparsity(N, J, H);
        std::vector<int> dj(J.size()), dh(H.size());
        for (size_t i = 0; i < J.size(); ++i) dj[i] = J[i].desc;
        for (size_t i = 0; i < H.size(); ++i) dh[i] = H[i].desc;
        if (g_cache.dJ) (void)hipFree(g_cache.dJ);
        if (g_cache.dH) (void)hipFree(g_cache.dH);
        if ((e = hipMalloc(&g_cache.dJ, dj.size() * sizeof(int))) != hipSuccess) return (int)e;
        if ((e = hipMalloc(&g_cache.dH, dh.size() * sizeof(int))) != hipSuccess) return (int)e;
        if ((e = hipMemcpy(g_cache.dJ, dj.data(), dj.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
        if ((e = hipMemcpy(g_cache.dH, dh.data(), dh.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
        g_cache.N = N; g_cache.device = dev; g_cache.nnzj = (int)dj.size(); g_cache.nnzh = (int)dh.size();
    }
    const size_t lds = nlp_lds_bytes(N);
    hipLaunchKernelGGL(cmpc_nlp_eval_kernel, dim3(prm->B), dim3(256), lds, stream, *prm, dX, dP, dLamG, lam_f, dF, dG, dGradF, dJac, dHess,
                       g_cache.dJ, g_cache.dH, g_cache.nnzj, g_cache.nnzh);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_nlp_grad(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, float lam_f, float* dGradX,
                                    float* dGradP, hipStream_t stream)
{
    const size_t lds = nlp_lds_bytes(prm->N);
    hipLaunchKernelGGL(cmpc_nlp_grad_kernel, dim3(prm->B), dim3(256), lds, stream, *prm, dX, dP, dLamG, lam_f, dGradX, dGradP);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_multipliers(const CmpcParams* prm, const float* dX, const float* dP, float* dLamG, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_multipliers_kernel, dim3(prm->B), dim3(256), nlp_lds_bytes(prm->N), stream, *prm, dX, dP, prm->duals, dLamG);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_kkt_certificate(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, float* dCert, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_kkt_certificate_kernel, dim3(prm->B), dim3(256), nlp_lds_bytes(prm->N), stream, *prm, dX, dP, dLamG, prm->duals, dCert);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_value_gradient(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, float* dGradP, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_value_gradient_kernel, dim3(prm->B), dim3(256), nlp_lds_bytes(prm->N), stream, *prm, dX, dP, dLamG, dGradP);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_model_value_gradient(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, double* dGradModel,
                                                hipStream_t stream)
{
    const size_t lds = nlp_lds_bytes(prm->N) + sizeof(double) * CMPC_MODEL_DOUBLES * (size_t)(prm->N + 1);
    hipLaunchKernelGGL(cmpc_model_value_gradient_kernel, dim3(prm->B), dim3(256), lds, stream, *prm, dX, dP, dLamG, dGradModel);
    return (int)hipGetLastError();
}

extern "C" int cmpc_launch_rotation_value_gradient(const CmpcParams* prm, const float* dX, const float* dP, const float* dLamG, double* dGradRot,
                                                   hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_rotation_value_gradient_kernel, dim3(prm->B), dim3(256), nlp_lds_bytes(prm->N), stream, *prm, dX, dP, dLamG, dGradRot);
    return (int)hipGetLastError();
}
