// Stand-alone host program for tests/test_walk_refill_plans_cpu.py: the host forms of the plan select of a refill walk with plans per trial and of the
// pool's fold (the loops of cmpc_rollout_refill_plans and cmpc_rollout_plan_fold, csrc/cmpc_contacts.h) with every array allocated at its exact size, so
// that a sanitizer sees a word read or written past an end.  The select: B = 5 slots, a pool of 3 rows, M = 5 (rows of 40, 70 and 2 words) and 23 knots (69
// words), the last row of each array ending at the end of its allocation.  Prints what each slot holds after the call; exit status 0.
#include <cstdio>
#include <vector>

#include "cmpc_contacts.h"

int main()
{
    const int B = 5, P = 3, Q = 6, tick = 4;
    const int words[CMPC_PLAN_ARRAYS] = {40, 70, 2, 69, 69};
    std::vector<unsigned> pool[CMPC_PLAN_ARRAYS], live[CMPC_PLAN_ARRAYS];
    CmpcRefillPlansArgs a{};
    a.B = B; a.Q = Q; a.tick = tick; a.pool_plans = P; a.count = CMPC_PLAN_ARRAYS;
    for (int i = 0; i < CMPC_PLAN_ARRAYS; ++i) {
        pool[i].resize((size_t)P * words[i]);
        live[i].assign((size_t)B * words[i], 0xA5A5A5A5u);
        for (size_t e = 0; e < pool[i].size(); ++e) pool[i][e] = 1000u * (unsigned)(i + 1) + (unsigned)e;
        a.src[i] = pool[i].data(); a.dst[i] = live[i].data(); a.words[i] = words[i];
    }
    // slot 0: spawned, row 2 (the pool's last row) | slot 1: walking since tick 2 | slot 2: spawned, index -1 | slot 3: spawned at this tick number but empty
    // | slot 4 (the last slot): spawned, row 2 again -- a repeated index; trial 5 (index P) is never started
    std::vector<int> start = {4, 2, 4, 4, 4}, trial = {1, 0, 2, -1, 4}, index = {0, 2, -1, 1, 2, P}, ok(Q, -7), end_tick(B, -1), end_code(B, 9);
    a.start = start.data(); a.trial = trial.data(); a.index = index.data();
    a.ok = ok.data(); a.end_tick = end_tick.data(); a.end_code = end_code.data();
    cmpc_refill_plans_host(a);
    for (int b = 0; b < B; ++b) {
        std::printf("slot %d end %d code %d first", b, end_tick[b], end_code[b]);
        for (int i = 0; i < CMPC_PLAN_ARRAYS; ++i) std::printf(" %u", live[i][(size_t)b * words[i]]);
        std::printf(" last");
        for (int i = 0; i < CMPC_PLAN_ARRAYS; ++i) std::printf(" %u", live[i][(size_t)(b + 1) * words[i] - 1]);
        std::printf("\n");
    }
    std::printf("ok");
    for (int q = 0; q < Q; ++q) std::printf(" %d", ok[q]);
    std::printf("\n");
    a.ok = nullptr; a.count = 3;         // (without the flags and without trajectories: the lists alone)
    cmpc_refill_plans_host(a);
    std::printf("again %u %u\n", live[1][0], live[1][(size_t)5 * 70 - 1]);

    // the fold: 7 trials of 3 words onto 3 rows; row 1 is empty, trial 3 lies outside the pool, row 0's sum depends on the order
    const int T = 7, W = 3, R = 3;
    std::vector<int> of = {0, 2, 0, R, 0, 2, 0};
    std::vector<double> per((size_t)T * W), out((size_t)R * W, -1.0);
    for (size_t e = 0; e < per.size(); ++e) per[e] = (double)(e + 1);
    per[0 * W] = 1e16; per[2 * W] = 1.0; per[4 * W] = -1e16; per[6 * W] = 1.0;
    for (int p = 0; p < R; ++p)
        for (int w = 0; w < W; ++w) out[(size_t)p * W + w] = cmpc_plan_fold_entry(T, W, of.data(), per.data(), p, w);
    std::printf("fold");
    for (double v : out) std::printf(" %.1f", v);
    std::printf("\n");
    return 0;
}
