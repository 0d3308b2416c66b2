/* gomoku_pattern_states.h -- the pattern heuristic asked about a position given as network planes ("K23").
 *
 * K10 (gmk_pattern_policy) computes Heuristic::EvaluationProbs, DecisiveFilter and EvaluationValue for a MOVE LIST, because the evaluator's
 * per-cell flag words depend on the order the moves were played in.  K7's leaf batch is the float32 [6][225] planes of
 * Board.encoded_states(), which hold the stones and the last two moves and nothing else of the order.  This header states, ONCE, how a row
 * of planes becomes a move list and how K10's vector becomes the prior K7 expands with -- for the kernel (pattern_kernel.hip), the host
 * forms (gmk_pattern_states_list_host, gmk_pattern_states_finish_host) and any C or C++ caller.  It is compiled by gcc, by g++ and by hipcc
 * for the host and gfx950; its operations are integer operations and IEEE-754 binary64 +, / and conversions, so a list and a prior are the
 * same wherever they are computed.
 *
 * Decoding a row s[6][225].  A cell is SET iff x != 0.0f (NaN is set, -0.0 is not).  own = plane 0, opp = plane 1; plane 2 is not read.
 * Black is to move iff s[5][0] is set (no other cell of plane 5 is read); black's stones are own when black is to move, opp otherwise.
 * The row is a POSITION iff
 *   - own and opp share no cell,
 *   - nb == nw when black is to move and nb == nw + 1 when white is (nb, nw: black's and white's stones),
 *   - plane 3 has at most one set cell, and that cell is in opp              (the last move; gmk_az_set_roots allows none),
 *   - plane 4 has at most one set cell, in own, and only when plane 3 has one (the move before it).
 * Anything else is GMK_PATTERN_ILLEGAL with zero outputs -- the all-zero row K7 writes for a game that is over at the leaf among them
 * ("white to move, no stones").
 *
 * The canonical move list.  THIS PROJECT'S DEFINITION: the position's real order is not in the planes.  T = nb + nw plies, black the even
 * ones (0-based).  The cell of plane 3 is ply T - 1, the cell of plane 4 ply T - 2; the remaining black stones fill the remaining even
 * plies in ascending cell order, the remaining white stones the remaining odd plies in ascending cell order.
 *
 * Finishing.  The list goes through K10's path unchanged (a fresh evaluator, applyMove per ply, EvaluationProbs, DecisiveFilter when
 * `filter`, EvaluationValue): K10's vector v, its value and its status bits 0, 1, 2 -- what gmk_pattern_policy reports for the list.
 *   GMK_PATTERN_NORM_L2   probs = v, K10's L2-normalised vector bit for bit.
 *   GMK_PATTERN_NORM_SUM  S = the sum of (double)v_c in the association of gmk_noise_sum225 (gmk_gumbel_sum225),
 *                         probs_c = (float)((double)v_c / S); when S == 0 on a live row (status 0) with E > 0 empty cells,
 *                         probs_c = (float)(1.0 / (double)E) on the empty cells and 0 elsewhere: a live leaf always has a candidate.
 * The value is K10's in both modes: for the player to move, in [-1, 1].
 */
#ifndef GOMOKU_PATTERN_STATES_H_
#define GOMOKU_PATTERN_STATES_H_

#include <stdint.h>

#include "gomoku_gumbel.h"

#define GMK_PATTERN_FN GMK_NOISE_FN

#define GMK_PATTERN_CELLS 225
#define GMK_PATTERN_PLANES 6
#define GMK_PATTERN_ILLEGAL 4 /* bit 2 of K10's status */
#ifndef GMK_PATTERN_NORM_DEFINED /* (gomoku_hip.h declares the same two) */
#define GMK_PATTERN_NORM_DEFINED
enum { GMK_PATTERN_NORM_L2 = 0, GMK_PATTERN_NORM_SUM = 1 };
#endif

/* the set cells of the four planes that are read, 64 cells per word (cell c = bit c & 63 of word c >> 6), and the side to move */
typedef struct {
    uint64_t own[4], opp[4], last[4], last2[4];
    int black_to_move;
} gmk_pattern_masks;

/* the list as it is walked: the stones not yet played, without the two last moves */
typedef struct {
    uint64_t black[4], white[4];
    int plies, last, last2; /* T; the cells of planes 3 and 4, -1: none */
} gmk_pattern_walk;

GMK_PATTERN_FN int gmk_pattern_count(const uint64_t w[4]) {
    return __builtin_popcountll(w[0]) + __builtin_popcountll(w[1]) + __builtin_popcountll(w[2]) + __builtin_popcountll(w[3]);
}

/* the lowest set cell, -1 when there is none */
GMK_PATTERN_FN int gmk_pattern_lowest(const uint64_t w[4]) {
    if (w[0]) return __builtin_ctzll(w[0]);
    if (w[1]) return 64 + __builtin_ctzll(w[1]);
    if (w[2]) return 128 + __builtin_ctzll(w[2]);
    if (w[3]) return 192 + __builtin_ctzll(w[3]);
    return -1;
}

/* the lowest set cell, taken out of the set; -1 when there is none */
GMK_PATTERN_FN int gmk_pattern_pop(uint64_t w[4]) {
    if (w[0]) { const int c = __builtin_ctzll(w[0]); w[0] &= w[0] - 1; return c; }
    if (w[1]) { const int c = __builtin_ctzll(w[1]); w[1] &= w[1] - 1; return 64 + c; }
    if (w[2]) { const int c = __builtin_ctzll(w[2]); w[2] &= w[2] - 1; return 128 + c; }
    if (w[3]) { const int c = __builtin_ctzll(w[3]); w[3] &= w[3] - 1; return 192 + c; }
    return -1;
}

/* a (a & ~b) != 0 in any word */
GMK_PATTERN_FN int gmk_pattern_outside(const uint64_t a[4], const uint64_t b[4]) {
    return ((a[0] & ~b[0]) | (a[1] & ~b[1]) | (a[2] & ~b[2]) | (a[3] & ~b[3])) != 0;
}

/* 0 when the masks are a position, GMK_PATTERN_ILLEGAL otherwise */
GMK_PATTERN_FN int gmk_pattern_check(const gmk_pattern_masks* m) {
    const int n_own = gmk_pattern_count(m->own), n_opp = gmk_pattern_count(m->opp);
    const int n_last = gmk_pattern_count(m->last), n_last2 = gmk_pattern_count(m->last2);
    int ok = ((m->own[0] & m->opp[0]) | (m->own[1] & m->opp[1]) | (m->own[2] & m->opp[2]) | (m->own[3] & m->opp[3])) == 0;
    ok = ok && (m->black_to_move ? n_own == n_opp : n_opp == n_own + 1);
    ok = ok && n_last <= 1 && !gmk_pattern_outside(m->last, m->opp);
    ok = ok && n_last2 <= 1 && !gmk_pattern_outside(m->last2, m->own) && (n_last2 == 0 || n_last == 1);
    return ok ? 0 : GMK_PATTERN_ILLEGAL;
}

/* the walk of a POSITION's canonical list (gmk_pattern_check said 0) */
GMK_PATTERN_FN void gmk_pattern_walk_begin(const gmk_pattern_masks* m, gmk_pattern_walk* w) {
    const int btm = m->black_to_move;
    w->plies = gmk_pattern_count(m->own) + gmk_pattern_count(m->opp);
    w->last = gmk_pattern_lowest(m->last);
    w->last2 = gmk_pattern_lowest(m->last2);
    /* the mover of ply T - 1 is the opponent of the side to move: opp without plane 3, own without plane 4 */
    w->black[0] = btm ? m->own[0] & ~m->last2[0] : m->opp[0] & ~m->last[0];
    w->black[1] = btm ? m->own[1] & ~m->last2[1] : m->opp[1] & ~m->last[1];
    w->black[2] = btm ? m->own[2] & ~m->last2[2] : m->opp[2] & ~m->last[2];
    w->black[3] = btm ? m->own[3] & ~m->last2[3] : m->opp[3] & ~m->last[3];
    w->white[0] = btm ? m->opp[0] & ~m->last[0] : m->own[0] & ~m->last2[0];
    w->white[1] = btm ? m->opp[1] & ~m->last[1] : m->own[1] & ~m->last2[1];
    w->white[2] = btm ? m->opp[2] & ~m->last[2] : m->own[2] & ~m->last2[2];
    w->white[3] = btm ? m->opp[3] & ~m->last[3] : m->own[3] & ~m->last2[3];
}

/* the cell of ply `ply` (call it for ply = 0, 1, .. T - 1 in order) */
GMK_PATTERN_FN int gmk_pattern_walk_next(gmk_pattern_walk* w, int ply) {
    if (ply == w->plies - 1 && w->last >= 0) return w->last;
    if (ply == w->plies - 2 && w->last2 >= 0) return w->last2;
    return (ply & 1) ? gmk_pattern_pop(w->white) : gmk_pattern_pop(w->black);
}

GMK_PATTERN_FN int gmk_pattern_is_set(float x) { return x != 0.0f; }

/* the masks of a row s[6][225] */
GMK_PATTERN_FN void gmk_pattern_masks_of(const float* s, gmk_pattern_masks* m) {
    for (int j = 0; j < 4; ++j) m->own[j] = m->opp[j] = m->last[j] = m->last2[j] = 0;
    for (int c = 0; c < GMK_PATTERN_CELLS; ++c) {
        const uint64_t bit = (uint64_t)1 << (c & 63);
        if (gmk_pattern_is_set(s[0 * GMK_PATTERN_CELLS + c])) m->own[c >> 6] |= bit;
        if (gmk_pattern_is_set(s[1 * GMK_PATTERN_CELLS + c])) m->opp[c >> 6] |= bit;
        if (gmk_pattern_is_set(s[3 * GMK_PATTERN_CELLS + c])) m->last[c >> 6] |= bit;
        if (gmk_pattern_is_set(s[4 * GMK_PATTERN_CELLS + c])) m->last2[c >> 6] |= bit;
    }
    m->black_to_move = gmk_pattern_is_set(s[5 * GMK_PATTERN_CELLS]);
}

/* The canonical list of a row: moves[0 .. *len), nothing past it is written (moves holds 225).  Returns 0, or GMK_PATTERN_ILLEGAL with
 * *len = 0.  The serial statement of the front of pattern_states_kernel. */
GMK_PATTERN_FN int gmk_pattern_list225(const float* s, uint8_t* moves, int32_t* len) {
    gmk_pattern_masks m;
    gmk_pattern_walk w;
    gmk_pattern_masks_of(s, &m);
    *len = 0;
    if (gmk_pattern_check(&m) != 0) return GMK_PATTERN_ILLEGAL;
    gmk_pattern_walk_begin(&m, &w);
    for (int ply = 0; ply < w.plies; ++ply) moves[ply] = (uint8_t)gmk_pattern_walk_next(&w, ply);
    *len = w.plies;
    return 0;
}

/* K10's vector v[225] of a row into the prior out[225].  `live`: the row is a position and K10's status for its list is 0; a row that is
 * not live gets zeros.  own / opp: the row's stone masks (the empty cells of the uniform fallback).  The serial statement of the back of
 * pattern_states_kernel. */
GMK_PATTERN_FN void gmk_pattern_finish225(const float* v, int norm, int live, const uint64_t own[4], const uint64_t opp[4], float* out) {
    double d[GMK_PATTERN_CELLS];
    if (!live) {
        for (int c = 0; c < GMK_PATTERN_CELLS; ++c) out[c] = 0.0f;
        return;
    }
    if (norm == GMK_PATTERN_NORM_L2) {
        for (int c = 0; c < GMK_PATTERN_CELLS; ++c) out[c] = v[c];
        return;
    }
    for (int c = 0; c < GMK_PATTERN_CELLS; ++c) d[c] = (double)v[c];
    const double sum = gmk_gumbel_sum225(d);
    if (sum == 0.0) {
        const int empty = GMK_PATTERN_CELLS - gmk_pattern_count(own) - gmk_pattern_count(opp);
        const float u = empty > 0 ? (float)(1.0 / (double)empty) : 0.0f;
        for (int c = 0; c < GMK_PATTERN_CELLS; ++c) out[c] = (((own[c >> 6] | opp[c >> 6]) >> (c & 63)) & 1) ? 0.0f : u;
        return;
    }
    for (int c = 0; c < GMK_PATTERN_CELLS; ++c) out[c] = (float)(d[c] / sum);
}

#endif /* GOMOKU_PATTERN_STATES_H_ */
