// Stand-alone host program for tests/test_walk_refill_tape_cpu.py: the host form of the regroup of a refill walk's tape by trial (the loop of
// cmpc_rollout_tape_regroup, csrc/cmpc_contacts.h) on B = 3 columns, a slot-major source of 5 rows and a destination of trial_ticks = 4 rows, every array
// allocated at its exact size so that a sanitizer sees a word read or written past an end.  The ten arrays have rows of 1, 2, 9 and 70 words (the
// last row of each ending at the end of its allocation).  Source word e of array i holds 1000 (i + 1) + e, source state word e holds 90000 + e.
// Prints what each column holds after the call; exit status 0.
#include <cstdio>
#include <vector>

#include "cmpc_contacts.h"

int main()
{
    const int B = 3, R = 5, TT = 4, Q = 5;
    const int words[CMPC_REGROUP_ARRAYS] = {70, 9, 70, 2, 1, 2, 9, 2, 70, 2};
    std::vector<unsigned> src[CMPC_REGROUP_ARRAYS], dst[CMPC_REGROUP_ARRAYS], src_states((size_t)(R + 1) * B * 9), dst_states((size_t)(TT + 1) * B * 9, 0xA5A5A5A5u);
    CmpcRegroupArgs a{};
    a.B = B; a.rows = TT; a.src_rows = R; a.Q = Q; a.tick_first = 0;
    for (int i = 0; i < CMPC_REGROUP_ARRAYS; ++i) {
        src[i].resize((size_t)R * B * words[i]);
        dst[i].assign((size_t)TT * B * words[i], 0xA5A5A5A5u);
        for (size_t e = 0; e < src[i].size(); ++e) src[i][e] = 1000u * (unsigned)(i + 1) + (unsigned)e;
        a.src[i] = src[i].data(); a.dst[i] = dst[i].data(); a.words[i] = words[i];
    }
    for (size_t e = 0; e < src_states.size(); ++e) src_states[e] = 90000u + (unsigned)e;
    a.src_states = src_states.data(); a.dst_states = dst_states.data();
    // trial 0: slot 2 (the last column), start 1, walked through: source rows 1 .. 4, the tape's last | trial 1: slot 0, start 3, cut off after 2 ticks:
    // rows 3, 4, 4, 4 | trial 2: never started | trial 3: slot 1, start 4, two ticks recorded: its second row lies outside the tape | trial 4: ended at 0
    std::vector<int> slot = {2, 0, -1, 1, 1}, start = {1, 3, -1, 4, 0}, ticks = {4, 2, 0, 2, 1}, end = {-1, -1, -1, -1, 0};
    std::vector<unsigned> state0((size_t)Q * 9);
    for (size_t e = 0; e < state0.size(); ++e) state0[e] = 70000u + (unsigned)e;
    a.slot = slot.data(); a.start = start.data(); a.ticks = ticks.data(); a.end = end.data(); a.state0 = state0.data();
    const int groups[3][3] = {{0, 1, 2}, {3, 4, 4}, {-1, Q, 0}};
    for (int gi = 0; gi < 3; ++gi) {
        std::vector<int> index(groups[gi], groups[gi] + B), end_out(B, -7), ok_out(B, -7);
        a.index = index.data(); a.end_out = end_out.data(); a.ok_out = gi == 2 ? nullptr : ok_out.data();
        for (int i = 0; i < CMPC_REGROUP_ARRAYS; ++i) dst[i].assign(dst[i].size(), 0xA5A5A5A5u);
        dst_states.assign(dst_states.size(), 0xA5A5A5A5u);
        cmpc_regroup_host(a);
        for (int j = 0; j < B; ++j) {
            // the first word of the column's first row of array 0, the last word of its last row of arrays 0 (70 words), 3 (2) and 8 (the planner's), its
            // first state word and the last word of its last state
            std::printf("group %d column %d end %d ok %d first %u last %u %u %u plan0 %u state %u %u\n", gi, j, end_out[j], ok_out[j],
                        dst[0][(size_t)j * 70], dst[0][((size_t)(TT - 1) * B + j + 1) * 70 - 1], dst[3][((size_t)(TT - 1) * B + j + 1) * 2 - 1],
                        dst[8][((size_t)(TT - 1) * B + j + 1) * 70 - 1], dst[8][(size_t)j * 70], dst_states[(size_t)j * 9],
                        dst_states[((size_t)TT * B + j + 1) * 9 - 1]);
        }
    }
    return 0;
}
