// Stand-alone host program for tests/test_walk_refill_snapshot_cpu.py: the host form of the restore step of a refill walk whose trials start from a
// snapshot (the loop of cmpc_rollout_refill_restore, csrc/cmpc_contacts.h) on B = 5 slots and a pool of 3 rows, every array allocated at its exact size so
// that a sanitizer sees a word read or written past an end.  Three arrays of different row widths stand for the snapshot's twenty (a row of 1 word, one
// of 9 and one of 70, the last row of each ending at the end of its allocation).  Prints what each slot holds after the call; exit status 0.
#include <cstdio>
#include <vector>

#include "cmpc_contacts.h"

int main()
{
    const int B = 5, S = 3, Q = 6, tick = 4, pool_tick = 8;
    const int words[3] = {1, 9, 70};
    std::vector<unsigned> pool[3], live[3];
    CmpcRefillRestoreArgs a{};
    a.copy.B = B; a.copy.src_B = S; a.copy.count = 3;
    for (int i = 0; i < 3; ++i) {
        pool[i].resize((size_t)S * words[i]);
        live[i].assign((size_t)B * words[i], 0xA5A5A5A5u);
        for (size_t e = 0; e < pool[i].size(); ++e) pool[i][e] = 1000u * (unsigned)(i + 1) + (unsigned)e;
        a.copy.src[i] = pool[i].data(); a.copy.dst[i] = live[i].data(); a.copy.words[i] = words[i];
    }
    // slot 0: spawned, row 2 (the pool's last row) | slot 1: walking since tick 2 | slot 2: spawned, index -1 | slot 3: spawned at this tick number but empty
    // | slot 4 (the last slot): spawned, row 2 again -- a repeated index; trial 5 (index S) is never started
    std::vector<int> start = {4, 2, 4, 4, 4}, trial = {1, 0, 2, -1, 4}, index = {0, 2, -1, 1, 2, S}, ok(Q, -7), end_tick(B, -1), end_code(B, 9);
    a.copy.index = index.data();
    a.start = start.data(); a.trial = trial.data();
    a.tick = tick; a.Q = Q; a.pool_tick = pool_tick;
    a.ok = ok.data(); a.end_tick = end_tick.data(); a.end_code = end_code.data();
    cmpc_refill_restore_host(a);
    for (int b = 0; b < B; ++b) {
        std::printf("slot %d end %d code %d first", b, end_tick[b], end_code[b]);
        for (int i = 0; i < 3; ++i) std::printf(" %u", live[i][(size_t)b * words[i]]);
        std::printf(" last");
        for (int i = 0; i < 3; ++i) std::printf(" %u", live[i][(size_t)(b + 1) * words[i] - 1]);
        std::printf("\n");
    }
    std::printf("ok");
    for (int q = 0; q < Q; ++q) std::printf(" %d", ok[q]);
    std::printf("\n");
    a.ok = nullptr;                      // (without the flags: the same copy)
    cmpc_refill_restore_host(a);
    std::printf("again %u %u\n", live[2][0], live[2][(size_t)5 * 70 - 1]);
    return 0;
}
