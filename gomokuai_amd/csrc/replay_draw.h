// replay_draw.h -- the draw rule of the replay buffer: element i of the batch of (seed, step) from a population of M samples.
// One definition for the device (replay_kernel.hip, one wavefront per sample) and the host (gmk_replay_draw_host); the rule is stated in
// full in include/gomoku_hip.h ("replay buffer"), and tests/test_replay.py restates it in numpy from that text.
#pragma once
#include "philox.h"

namespace gmk {

constexpr int kReplayFeistelRounds = 4;

// k with 4^(k-1) < M <= 4^k (k = 0 for M = 1); M <= 2^62
GMK_HD int replay_half_bits(uint64_t M) {
    int k = 0;
    while ((static_cast<uint64_t>(1) << (2 * k)) < M) ++k;
    return k;
}

// a bijection of [0, 4^k): balanced Feistel network over 2k bits, round function = word 0 of Philox4x32-10
GMK_HD uint64_t replay_feistel(uint64_t x, int k, uint64_t seed, uint64_t step) {
    const uint32_t mask = static_cast<uint32_t>((static_cast<uint64_t>(1) << k) - 1);
    uint32_t L = static_cast<uint32_t>(x >> k) & mask, R = static_cast<uint32_t>(x) & mask;
    for (uint32_t r = 0; r < static_cast<uint32_t>(kReplayFeistelRounds); ++r) {
        const uint32_t F = philox4x32_10(R, r, static_cast<uint32_t>(step), static_cast<uint32_t>(step >> 32),
                                         static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)).v[0] & mask;
        const uint32_t t = L ^ F;
        L = R;
        R = t;
    }
    return (static_cast<uint64_t>(L) << k) | R;
}

// perm(i) for i < M: cycle walking back into [0, M) (x starts inside, so the walk along its cycle returns there)
GMK_HD uint64_t replay_perm(uint64_t i, uint64_t M, int k, uint64_t seed, uint64_t step) {
    uint64_t x = i;
    do x = replay_feistel(x, k, seed, step); while (x >= M);
    return x;
}

}  // namespace gmk
