/* gomoku_sample.h -- self-play moves drawn in proportion to the root's visit counts ("K20").
 *
 * AlphaZero's self-play plays the first S plies of a game with probability proportional to N_i^(1/tau) over the root's children and the
 * most visited child afterwards (Silver et al., "Mastering the game of Go without human knowledge", Nature 550, 2017, Methods:
 * "Self-play").  The reference's agents always play the most visited child (MCTS::stepForward, core/lib/src/MCTS.cpp:129-134); this
 * header states the rule the K7 self-play loops add to that, ONCE, for the kernels (az_kernel.hip), the host form
 * (gmk_move_sample_host) and any C or C++ caller: it is compiled by hipcc for gfx950 and the host and by g++, and every operation in it
 * is an integer operation, so a choice is the same wherever it is computed.
 *
 * A root with children in child order (ascending cells), S = sample_plies, k = sample_power in 1..3 (temperature 1, 1/2, 1/3) and
 * `stones` stones on the root board (openings included):
 *   - stones >= S (S = 0 included): the greedy choice -- the most visited child, first maximum in child order; with proofs ("K7 + proofs"
 *     of gomoku_hip.h) the first child marked LOSES, otherwise the most visited child not marked WINS that has a visit, otherwise the
 *     rule before.  -1 when no child has a visit and none is marked LOSES.
 *   - otherwise v_i = min(visits_i, 65535), what a record's visit row holds, and w_i = v_i^k as a 64-bit integer (225 children at
 *     k = 3 add up to less than 2^56).  With proofs: a child marked LOSES is played, the first such, and nothing is drawn; children
 *     marked WINS get w_i = 0.
 *   - T = sum of w_i.  T = 0: the greedy choice.
 *   - r = the first two words of gmk_noise_philox(game id, stones, GMK_SAMPLE_TAG, 0; key = seed) as one 64-bit number, low word first;
 *     target = the high 64 bits of r T; the child played is the first i whose inclusive prefix sum w_0 + .. + w_i exceeds target.
 * r is uniform on [0, 2^64) and child i is chosen for the r with target in its w_i consecutive integers, which are w_i 2^64 / T values
 * of r give or take one: its probability is w_i / T within 2^-64, a relative deviation of at most T / (w_i 2^64) <= T / 2^64.  That is
 * below 2^-40 at k = 1 (T <= 225 * 65535 < 2^24) and below 2^-8 at k = 3 (T < 2^56), where it is reached only by a child of one visit
 * beside 224 saturated ones.
 * The game id is the GLOBAL one (first_game_id + the game's number), the one the root noise of gomoku_noise.h is keyed by, so a game's
 * moves do not depend on the slot, handle or loop that plays it, and every sampled move can be derived again from the record's row.
 */
#ifndef GOMOKU_SAMPLE_H_
#define GOMOKU_SAMPLE_H_

#include <stdint.h>

#include "gomoku_noise.h"

#define GMK_SAMPLE_FN GMK_NOISE_FN

#define GMK_SAMPLE_TAG 0x73616d70u /* 'samp' */
#define GMK_SAMPLE_MAX_POWER 3
#define GMK_SAMPLE_SATURATION 65535u
/* a child's proof as the rule reads it: the values of GMK_AZ_PROOF_WINS / GMK_AZ_PROOF_LOSES (gomoku_hip.h) */
#define GMK_SAMPLE_PROOF_WINS 1
#define GMK_SAMPLE_PROOF_LOSES 2

/* w = min(visits, 65535)^power, power in 1..3 */
GMK_SAMPLE_FN uint64_t gmk_sample_weight(uint32_t visits, int power) {
    const uint64_t v = visits < GMK_SAMPLE_SATURATION ? visits : GMK_SAMPLE_SATURATION;
    uint64_t w = v;
    if (power >= 2) w *= v;
    if (power >= 3) w *= v;
    return w;
}

/* the high 64 bits of a b, from 32-bit halves (no 128-bit type: the same text for gcc, g++ and the device) */
GMK_SAMPLE_FN uint64_t gmk_sample_mulhi(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

/* the draw of the root that game `game_id` reaches with `stones` stones, scaled to [0, total) */
GMK_SAMPLE_FN uint64_t gmk_sample_target(uint64_t total, uint32_t game_id, uint32_t stones, uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t w[4];
    gmk_noise_philox(game_id, stones, GMK_SAMPLE_TAG, 0u, seed_lo, seed_hi, w);
    return gmk_sample_mulhi((uint64_t)w[0] | (uint64_t)w[1] << 32, total);
}

/* The greedy choice from a root's visit counts by cell (0: no child or no visit) and, with proofs != NULL, its children's proofs by cell: the
 * serial statement of most_visited_child in az_kernel.hip.  The cell, or -1. */
GMK_SAMPLE_FN int gmk_sample_greedy225(const uint32_t* visits, const int8_t* proofs) {
    int best = -1, open = -1;
    uint32_t best_v = 0, open_v = 0;
    for (int c = 0; c < 225; ++c) {
        if (proofs && proofs[c] == GMK_SAMPLE_PROOF_LOSES) return c;
        if (visits[c] > best_v) { best_v = visits[c]; best = c; }
        if (proofs && proofs[c] != GMK_SAMPLE_PROOF_WINS && visits[c] > open_v) { open_v = visits[c]; open = c; }
    }
    return open >= 0 ? open : best;
}

/* The rule above for one root, from rows by cell: the serial statement of sampled_child in az_kernel.hip.  The cell, or -1. */
GMK_SAMPLE_FN int gmk_sample_choose225(const uint32_t* visits, const int8_t* proofs, uint32_t stones, uint32_t game_id, int sample_plies, int sample_power,
                                       uint32_t seed_lo, uint32_t seed_hi) {
    if (sample_plies <= 0 || stones >= (uint32_t)sample_plies) return gmk_sample_greedy225(visits, proofs);
    uint64_t total = 0;
    for (int c = 0; c < 225; ++c) {
        if (proofs && proofs[c] == GMK_SAMPLE_PROOF_LOSES) return c;
        if (!(proofs && proofs[c] == GMK_SAMPLE_PROOF_WINS)) total += gmk_sample_weight(visits[c], sample_power);
    }
    if (total == 0) return gmk_sample_greedy225(visits, proofs);
    const uint64_t target = gmk_sample_target(total, game_id, stones, seed_lo, seed_hi);
    uint64_t prefix = 0;
    for (int c = 0; c < 225; ++c) {
        if (!(proofs && proofs[c] == GMK_SAMPLE_PROOF_WINS)) prefix += gmk_sample_weight(visits[c], sample_power);
        if (prefix > target) return c;
    }
    return -1;                                                        /* (not reached: target < total) */
}

#endif /* GOMOKU_SAMPLE_H_ */
