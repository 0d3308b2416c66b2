/* gomoku_symmetry.h -- the network asked about a position in the board's eight orientations ("K22").
 *
 * AlphaGo Zero evaluates every leaf under one random dihedral transform of the board (Silver et al., "Mastering the game of Go without
 * human knowledge", Nature 550, 2017, Methods: "Expand and evaluate"); programs that play matches average all eight.  The reference's
 * agents ask the network about the position as it stands (PolicyValueNetwork.eval_state, network/model_tf.py:136-145) although its
 * training augments every sample eight-fold (network/data_helper.py:36-55).  This header states the rule gmk_pvnet_evaluate_sym adds,
 * ONCE, for the kernels (pvnet_sym_kernel.hip), the host form (gmk_pvnet_sym_pick_host) and any C or C++ caller: it is compiled by hipcc
 * for gfx950 and the host, by g++ and by gcc, and every operation in it is an integer operation, so a cell or a pick is the same
 * wherever it is computed.
 *
 * Numbering.  Symmetry a in 0..7 is k = a >> 1 quarter turns followed by a mirror when flip = a & 1: the numbering of the replay
 * buffer's draws (replay_kernel.hip) and of the training augmentation.  A 15 x 15 plane P becomes np.rot90(P, k), then np.fliplr of
 * that if flip.
 *
 * Transform.  T_a(s)[p][j] = s[p][src_a(j)] for all six planes p of Board.encoded_states() (all six are spatial; the colour plane is
 * constant), src_a(j) = gmk_sym_source(j, a) -- the closed form of gmk::augment_source(j, k, flip) in records_access.h (HIP code, which
 * a C caller cannot read); the kernels tabulate augment_source itself and assert at compile time that this header says the same.
 *
 * Back-transform.  A policy row q over the transformed board goes back as p[src_a(j)] = q[j], i.e. p[c] = q[dst_a(c)] with
 * dst_a = gmk_sym_target(c, a), the inverse permutation.
 *
 * The pick of GMK_PVNET_SYM_RANDOM.  A function of the row's CONTENT and the seed only -- never of the row's index, the slot, the handle
 * or the batch, so that (like the draws of gomoku_sample.h) a game is the same game on every loop that plays it:
 *     code(c) = (s[0][c] != 0) + 2 * (s[1][c] != 0)            the stone on cell c: the mover's, the opponent's
 *     colour  = (s[5][0] != 0)
 *     digest  = sum over the cells with code != 0 of splitmix64(4 c + code(c)),  + splitmix64(900 + colour),  mod 2^64
 *     a       = w[0] & 7 of gmk_noise_philox(digest low word, digest high word, GMK_SYM_TAG, 0; key = seed low word, seed high word)
 * The digest is a sum, so a wavefront adds it up in whatever order it likes; planes 2, 3 and 4 (the last moves) do not enter it.
 */
#ifndef GOMOKU_SYMMETRY_H_
#define GOMOKU_SYMMETRY_H_

#include <stdint.h>

#include "gomoku_noise.h"

#if defined(__cplusplus)
#define GMK_SYM_FN constexpr GMK_NOISE_FN
#else
#define GMK_SYM_FN GMK_NOISE_FN
#endif

#define GMK_SYM_TAG 0x73796d6du /* 'symm' */
#define GMK_SYM_COUNT 8
#define GMK_SYM_CELLS 225
#define GMK_SYM_PLANES 6

/* src_a(j): the cell of the position that cell j of the transformed position shows */
GMK_SYM_FN int gmk_sym_source(int j, int a) {
    const int r = j / 15, x = (a & 1) ? 14 - j % 15 : j % 15;         /* fliplr(b)[r][x] = b[r][14 - x] */
    const int k = a >> 1;                                             /* rot90(b)[r][x] = b[x][14 - r], k times */
    return k == 0 ? r * 15 + x : k == 1 ? x * 15 + (14 - r) : k == 2 ? (14 - r) * 15 + (14 - x) : (14 - x) * 15 + r;
}

/* dst_a(c): the cell of the transformed position that shows cell c; gmk_sym_source(gmk_sym_target(c, a), a) = c */
GMK_SYM_FN int gmk_sym_target(int c, int a) {
    const int r = c / 15, x = c % 15, k = a >> 1;
    const int rr = k == 0 ? r : k == 1 ? 14 - x : k == 2 ? 14 - r : x;
    const int xx = k == 0 ? x : k == 1 ? r : k == 2 ? 14 - x : 14 - r;
    return rr * 15 + ((a & 1) ? 14 - xx : xx);
}

/* Steele, Lea & Flood's SplitMix64 output function of x + the golden-ratio increment */
GMK_SYM_FN uint64_t gmk_sym_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* cell c's term of the digest; 0 for an empty cell */
GMK_SYM_FN uint64_t gmk_sym_cell_term(int c, int mine, int theirs) {
    return (mine || theirs) ? gmk_sym_splitmix64((uint64_t)(4 * c + (mine ? 1 : 0) + (theirs ? 2 : 0))) : 0;
}

GMK_SYM_FN uint64_t gmk_sym_colour_term(int colour) { return gmk_sym_splitmix64((uint64_t)(900 + (colour ? 1 : 0))); }

/* the digest of one position, s = float[6][225]: the serial statement of the wavefront sum in pvnet_sym_expand_kernel */
GMK_NOISE_FN uint64_t gmk_sym_digest(const float* s) {
    uint64_t d = gmk_sym_colour_term(s[5 * GMK_SYM_CELLS] != 0.0f);
    for (int c = 0; c < GMK_SYM_CELLS; ++c) d += gmk_sym_cell_term(c, s[c] != 0.0f, s[GMK_SYM_CELLS + c] != 0.0f);
    return d;
}

/* the symmetry GMK_PVNET_SYM_RANDOM evaluates a position with this digest in */
GMK_NOISE_FN int gmk_sym_pick(uint64_t digest, uint64_t seed) {
    uint32_t w[4];
    gmk_noise_philox((uint32_t)digest, (uint32_t)(digest >> 32), GMK_SYM_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return (int)(w[0] & 7u);
}

#endif /* GOMOKU_SYMMETRY_H_ */
