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

extern "C" int cmpc_launch_warm_shift(const CmpcParams* prm, const float* dXprev, float* dX0, hipStream_t stream)
{
    hipLaunchKernelGGL(cmpc_warm_shift_kernel, dim3(prm->B), dim3(256), 0, stream, prm->N, prm->B, dXprev, dX0);
    return (int)hipGetLastError();
}

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
template <bool ROT>
__device__ inline void plant_jvp_problem(int N, int b, const float* __restrict__ P, const PlantPartials& q, const double* __restrict__ dir_state,
                                         const float* __restrict__ dir_x, const float* __restrict__ dir_p, const double* __restrict__ dir_model,
                                         const double* __restrict__ dir_rot, double* __restrict__ out)
{
    const CmpcIdx L{N};
    const float* p = P + (size_t)b * L.np();
    const double T = q.T;
    double dc[3], dv[3], dh[3], dF[3] = {0, 0, 0}, dtau[3], da[3], dI[3], t[3];
    for (int i = 0; i < 3; ++i) {
        dc[i] = dir_state[(size_t)b * 9 + i]; dv[i] = dir_state[(size_t)b * 9 + 3 + i]; dh[i] = dir_state[(size_t)b * 9 + 6 + i];
        dtau[i] = dir_p ? (double)dir_p[(size_t)b * L.np() + L.pText() + i] : 0.0;
    }
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
template <bool ROT>
__global__ __launch_bounds__(256) void cmpc_plant_jvp_cols_kernel(int N, int B, int K, float grav, const float* __restrict__ corners, int corners_stride,
                                                                  const float* __restrict__ X, const float* __restrict__ P,
                                                                  const float* __restrict__ state_in, float h, int nsub, const double* dir_state,
                                                                  const float* __restrict__ dir_x, const float* __restrict__ dir_p,
                                                                  const double* __restrict__ dir_model, const double* __restrict__ dir_rot,
                                                                  const int* __restrict__ ok, double* out)
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
__global__ __launch_bounds__(256) void cmpc_rollout_record_kernel(CmpcRecordArgs a, int* __restrict__ stats)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    int t[5] = {0, 0, 0, 0, 0};
    if (b < a.B) cmpc_record_problem(a, b, t);
    if (!stats) return;   // (uniform)
    for (int o = warpSize / 2; o > 0; o >>= 1) {
        t[0] += __shfl_xor(t[0], o);
        t[1] += __shfl_xor(t[1], o);
        t[2] += __shfl_xor(t[2], o);
        t[3] = max(t[3], __shfl_xor(t[3], o));
        t[4] += __shfl_xor(t[4], o);
    }
    if ((threadIdx.x & (warpSize - 1)) == 0) {
        if (t[0]) atomicAdd(stats + 0, t[0]);
        if (t[1]) atomicAdd(stats + 1, t[1]);
        if (t[2]) atomicAdd(stats + 2, t[2]);
        if (t[3]) atomicMax(stats + 3, t[3]);
        if (t[4]) atomicAdd(stats + 4, t[4]);
    }
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
    hipLaunchKernelGGL(cmpc_rollout_record_kernel, dim3((a->B + 255) / 256), dim3(256), 0, stream, *a, stats);
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
    const unsigned blocks = (unsigned)(((long long)B * K + 255) / 256);
    if (dDirRot0)
        hipLaunchKernelGGL(cmpc_plant_jvp_cols_kernel<true>, dim3(blocks), dim3(256), 0, stream, N, B, K, grav, dCorners, corners_stride, dX, dP, dStateIn, h,
                           nsub, dDirState, dDirX, dDirP, dDirModel, dDirRot0, dOk, dOut);
    else
        hipLaunchKernelGGL(cmpc_plant_jvp_cols_kernel<false>, dim3(blocks), dim3(256), 0, stream, N, B, K, grav, dCorners, corners_stride, dX, dP, dStateIn, h,
                           nsub, dDirState, dDirX, dDirP, dDirModel, dDirRot0, dOk, dOut);
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
