// Stand-alone host program for tests/test_vjp_cols_cpu.py: sens_problem of csrc/cmpc_sensitivity.hip is __host__ __device__ with a one-thread host team,
// so the k-column VJP (Rhs mode 2, the per-column residuals, the column arguments of the contraction, model_vjp and rot_vjp) runs here on the CPU, every
// array allocated at its exact size so that a sanitizer sees a word read or written past an end.  Per input file (one problem: int32 N, double dt,
// 34 doubles of cmpc_model, then x[n_x], p[n_p], lam_g[n_g] float32) it runs k = 9 cotangent columns (two chunks) in one call and the nine
// single-column calls, and prints whether every column's dGradP, dGradModel and dGradRot are the single call's bytes and how dSens compares.
// No HIP call is made: the launch function of the file is linked but never reached.
#include <cstdio>
#include <cstring>
#include <vector>

#include "cmpc_sensitivity.hip"

struct Out {
    std::vector<float> gp, sens;
    std::vector<double> gm, gr;
};

static Out run(const CmpcConsts& K, int N, const std::vector<float>& x, const std::vector<float>& p, const std::vector<float>& lam, const float* gx, int k)
{
    const CmpcIdx L{N};
    Prob P;
    P.K = &K; P.L = L; P.x = x.data(); P.p = p.data(); P.lam = lam.data();
    P.gh = 15 + 6 * N;
    for (int c = 0; c < 2; ++c) { P.gbox[c] = 15 + 15 * N + c * 19 * N; P.gfric[c] = P.gbox[c] + 3 * N; }
    std::vector<double> ws((size_t)Ws::doubles(N)), dense((size_t)Lds::doubles()), red(4), proj(3 + 3 * SENS_KC);
    std::vector<float> vproj((size_t)L.nx());
    Geo geo;
    Ws W;
    W.N = N;
    W.Pst = ws.data();
    W.Hi = W.Pst + (size_t)(N + 1) * SX * SX;
    W.Kg = W.Hi + (size_t)N * SU * SU;
    W.col = W.Kg + (size_t)N * SU * SX;
    const Team T{0, 1, red.data()};
    const Lds S = carve(dense.data(), &geo);
    Out o;
    o.gp.assign((size_t)k * L.np(), -7.f); o.gm.assign((size_t)k * CMPC_MODEL_DOUBLES, -7.0); o.gr.assign((size_t)k * 6 * N, -7.0); o.sens.assign(CMPC_SENS, -7.f);
    sens_problem(T, P, W, S, nullptr, gx, k, o.gp.data(), o.sens.data(), vproj.data(), nullptr, o.gm.data(), proj.data(), nullptr, o.gr.data());
    return o;
}

int main(int argc, char** argv)
{
    const int k = 9;
    for (int a = 1; a < argc; ++a) {
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 2;
        int N = 0;
        double dt = 0.0;
        cmpc_model m;
        if (std::fread(&N, sizeof(int), 1, f) != 1 || std::fread(&dt, sizeof(double), 1, f) != 1 || std::fread(&m, sizeof(m), 1, f) != 1) return 3;
        const CmpcIdx L{N};
        std::vector<float> x((size_t)L.nx()), p((size_t)L.np()), lam((size_t)L.ng());
        if (std::fread(x.data(), 4, x.size(), f) != x.size() || std::fread(p.data(), 4, p.size(), f) != p.size() ||
            std::fread(lam.data(), 4, lam.size(), f) != lam.size())
            return 3;
        std::fclose(f);
        CmpcConsts K;
        std::memset(&K, 0, sizeof(K));
        K.N = N; K.dt = (float)dt; K.grav = 9.80665f;
        std::vector<double> expk((size_t)N + 1);
        for (int i = 0; i <= N; ++i) expk[i] = std::exp(-(double)i);
        cmpc_consts_apply_model(K, m, expk.data());
        // cotangents: a fixed pseudo-random sequence, plus a constant on the left foot's forces (a component along the internal-force direction, if there is one)
        std::vector<float> gx((size_t)k * L.nx());
        unsigned s = 12345u + (unsigned)a;
        for (auto& v : gx) { s = s * 1664525u + 1013904223u; v = (float)((int)(s >> 8) % 2001 - 1000) * 1e-3f; }
        for (int j = 0; j < k; ++j)
            for (int c4 = 0; c4 < 4; ++c4)
                for (int e = 0; e < 3 * N; ++e) gx[(size_t)j * L.nx() + L.oF(0, c4) + e] += 0.5f * (float)(j + 1);
        const Out all = run(K, N, x, p, lam, gx.data(), k);
        int equal = 1;
        float r1 = 0.f, r6 = 0.f;
        int words = 1;
        for (int j = 0; j < k; ++j) {
            const Out one = run(K, N, x, p, lam, gx.data() + (size_t)j * L.nx(), 1);
            equal = equal && !std::memcmp(one.gp.data(), all.gp.data() + (size_t)j * L.np(), 4 * (size_t)L.np()) &&
                    !std::memcmp(one.gm.data(), all.gm.data() + (size_t)j * CMPC_MODEL_DOUBLES, 8 * CMPC_MODEL_DOUBLES) &&
                    !std::memcmp(one.gr.data(), all.gr.data() + (size_t)j * 6 * N, 8 * (size_t)(6 * N));
            r1 = one.sens[1] > r1 ? one.sens[1] : r1;
            r6 = one.sens[6] > r6 ? one.sens[6] : r6;
            for (int w : {0, 2, 3, 4, 5, 7}) words = words && one.sens[w] == all.sens[w];
        }
        float big = 0.f;
        for (float v : all.gp) big = std::fabs(v) > big ? std::fabs(v) : big;
        std::printf("N %d status %d internal %d columns-equal %d sens-words-equal %d residual-is-max %d removed-is-max %d nonzero %d\n", N, (int)all.sens[0],
                    (int)all.sens[4], equal, words, all.sens[1] == r1, all.sens[6] == r6, big > 0.f);
    }
    return 0;
}
