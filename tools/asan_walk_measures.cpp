// Developer tool (CPU only; never loaded into python, never run on a GPU): the per-entry functions behind cmpc_walk_measures_vjp / _vjp_fold / _jvp
// (csrc/cmpc_contacts.h, the kernels' own code) driven over random rows -- every support set, non-finite states, point feet, a sunk CoM, endings, the
// optional directions absent -- as a stand-alone program for the host sanitizers:
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -I paper_romualdi_2022_icra_centroidal-mpc-walking_amd/csrc -I include tools/asan_walk_measures.cpp -o /tmp/asan_walk_measures && /tmp/asan_walk_measures
// prints "ok" and a checksum; a sanitizer report is a bug.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "cmpc_contacts.h"

int main()
{
    const int N = 10, B = 64, rows = 3, K = 2;
    const CmpcIdx L{N};
    std::vector<float> X((size_t)rows * B * L.nx()), P((size_t)rows * B * L.np()), S((size_t)(rows + 1) * B * 9), corners(24 * B);
    srand(5);
    auto rnd = [] { return (float)rand() / RAND_MAX - 0.5f; };
    for (auto& v : X) v = rnd();
    for (auto& v : P) v = rnd();
    for (auto& v : S) v = rnd();
    for (auto& v : corners) v = 0.1f * rnd();
    for (int r = 0; r < rows; ++r)
        for (int b = 0; b < B; ++b) {
            float* p = P.data() + ((size_t)r * B + b) * L.np();
            p[L.pGam(0) + 1] = (b & 1) ? 1.f : 0.f;
            p[L.pGam(1) + 1] = (b & 2) ? 1.f : 0.f;
            if (b % 7 == 3) S[((size_t)(r + 1) * B + b) * 9 + 4] = NAN;
            if (b % 11 == 5) for (int i = 0; i < 24; ++i) corners[24 * b + i] = 0.f;      // point feet
            if (b % 13 == 6) S[((size_t)(r + 1) * B + b) * 9 + 2] = -3.f;                  // sunk
        }
    std::vector<int> end(B);
    for (int b = 0; b < B; ++b) end[b] = (b % 5) - 1;
    std::vector<double> gM((size_t)rows * B * 4, 0.7), gS((size_t)(rows + 1) * B * 9, 0.0), direct((size_t)rows * B * 32), gModel(34 * B, 0.0);
    std::vector<float> gX((size_t)rows * B * L.nx(), 0.f), gP((size_t)rows * B * L.np(), 0.f);
    const CmpcMeasureVjpArgs v{N, B, 0, rows, X.data(), P.data(), S.data(), end.data(), corners.data(), 24, 9.80665, gM.data(), gS.data(), gX.data(), direct.data()};
    for (int r = 0; r < rows; ++r)
        for (int b = 0; b < B; ++b) cmpc_walk_measures_vjp_entry(v, r, b);
    const size_t n = (size_t)rows * B > (size_t)24 * B ? (size_t)rows * B : (size_t)24 * B;
    for (size_t e = 0; e < n + 100; ++e) cmpc_walk_measures_fold_entry(N, B, rows, direct.data(), gP.data(), gModel.data(), e);
    std::vector<double> dS((size_t)(rows + 1) * B * K * 9, 0.3), dModel((size_t)B * K * 34, 0.1), dM((size_t)rows * B * K * 4);
    std::vector<float> dX((size_t)rows * B * K * L.nx(), 0.2f), dP((size_t)rows * B * K * L.np(), 0.1f);
    const CmpcMeasureJvpArgs j{N, B, 0, rows, K, X.data(), P.data(), S.data(), end.data(), corners.data(), 24, 9.80665, dS.data(), dX.data(), dP.data(), dModel.data(), dM.data()};
    const CmpcMeasureJvpArgs j0{N, B, 0, rows, K, X.data(), P.data(), S.data(), nullptr, corners.data(), 24, 9.80665, dS.data(), dX.data(), nullptr, nullptr, dM.data()};
    double sum = 0.0;
    for (int r = 0; r < rows; ++r)
        for (int b = 0; b < B; ++b) { cmpc_walk_measures_jvp_entry(j, r, b); cmpc_walk_measures_jvp_entry(j0, r, b); }
    for (double d : direct) sum += d;
    for (double d : dM) sum += d;
    for (double d : gModel) sum += d;
    printf("ok, checksum %.6e finite %d\n", sum, (int)std::isfinite(sum));
    return std::isfinite(sum) ? 0 : 1;
}
