// Stand-alone host program for tests/test_walk_refill_cpu.py: the host form of the refill (the loops of cmpc_rollout_refill_init / cmpc_rollout_refill,
// csrc/cmpc_contacts.h) on the crafted B = 5, Q = 7, trial_ticks = 3 case, every array allocated at its exact size so that a sanitizer sees a word read or
// written past an end.  Prints the slots and the queue after each call; exit status 0.
#include <cstdio>
#include <vector>

#include "cmpc_contacts.h"

int main()
{
    const int B = 5, Q = 7, rows = 4;
    std::vector<int> start(B, 77), trial(B, 77), end_tick(B, 9), end_code(B, 9), it_sum(B, 9), it_max(B, 9);
    std::vector<float> final_state(9 * B, 0.5f), slack(B, 0.5f), live(9 * B, 0.25f), state0(9 * Q);
    std::vector<int> q_end_tick(Q), q_end_code(Q), q_it_sum(Q), q_it_max(Q), q_ticks(Q), q_slot(Q), q_start(Q), trial_of(rows * B, 77);
    std::vector<float> q_final(9 * Q), q_slack(Q);
    for (int i = 0; i < 9 * Q; ++i) state0[i] = 0.125f * (float)i;
    int next = 77;
    auto args = [&](int tick_next, float* state_live) {
        return CmpcRefillArgs{B, Q, 3, tick_next, start.data(), trial.data(), state0.data(), q_end_tick.data(), q_end_code.data(), q_it_sum.data(),
                              q_it_max.data(), q_final.data(), q_slack.data(), q_ticks.data(), q_slot.data(), q_start.data(), end_tick.data(),
                              end_code.data(), it_sum.data(), it_max.data(), final_state.data(), slack.data(), state_live,
                              state_live && tick_next < rows ? trial_of.data() + tick_next * B : nullptr};
    };
    auto show = [&](const char* what) {
        std::printf("%s next %d trial", what, next);
        for (int b = 0; b < B; ++b) std::printf(" %d", trial[b]);
        std::printf(" start");
        for (int b = 0; b < B; ++b) std::printf(" %d", start[b]);
        std::printf(" end");
        for (int b = 0; b < B; ++b) std::printf(" %d", end_tick[b]);
        std::printf(" slot");
        for (int q = 0; q < Q; ++q) std::printf(" %d", q_slot[q]);
        std::printf(" ticks");
        for (int q = 0; q < Q; ++q) std::printf(" %d", q_ticks[q]);
        std::printf("\n");
    };
    cmpc_refill_init_host(args(0, nullptr), &next);
    cmpc_refill_host(args(0, live.data()), &next);
    show("fill");
    for (int b = 0; b < 4; ++b) start[b] = 1;                 // (hand-made: slots 0..3 as if spawned at tick 1, slots 1 and 3 ended at local tick 1)
    end_tick[1] = end_tick[3] = 1; end_code[1] = end_code[3] = 3;
    cmpc_refill_host(args(3, live.data()), &next);
    show("refill");
    it_sum[0] += 7;
    cmpc_refill_host(args(3, live.data()), &next);
    show("nothing-free");
    cmpc_refill_host(args(4, nullptr), &next);                // (the archive pass alone)
    show("archive");
    return 0;
}
