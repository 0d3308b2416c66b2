/* gomoku_gumbel.h -- Gumbel root search for K7 self-play at few playouts per move, with its policy target ("K21").
 *
 * Danihelka, Guez, Schrittwieser, Silver, "Policy improvement by planning with Gumbel", ICLR 2022: sample a few root actions without
 * replacement (Gumbel-top-m), spend the playouts on them by sequential halving, and learn from the completed-Q improved policy instead of
 * the visit counts.  This header states the rule ONCE, as gomoku_noise.h and gomoku_sample.h state theirs, for the kernels (az_kernel.hip),
 * the host forms (gmk_gumbel_*_host) and any C or C++ caller.  It is C, compiled by gcc, g++ and hipcc (host and gfx950) with
 * -ffp-contract=off, and uses only binary64 + - * /, comparisons, integer operations and gmk_noise_philox / _uniform / _log / _exp: the same
 * bits wherever it is computed.
 *
 * A root is given by cell, as gmk_noise_mix225 takes it: prior[225] (0 = no child; a child's prior is > 0), visits[225], value[225] -- a
 * child's stored mean, which is already from the root mover's side -- and root_value, the root's own stored mean (from the side of the
 * player who moved INTO the root, so the root mover sees -root_value).
 * Parameters: m = max_considered in 1..225, n = n_sims in 1..4096, c_visit and c_scale (the paper's 50 and 1.0 are the defaults of the
 * callers; nothing is tuned here), the 64-bit seed, the GLOBAL game id and the stones on the root board.
 *
 *   draw        g_c = -log(-log(u)), u = gmk_noise_uniform(word 0 of gmk_noise_philox(game id, stones, GMK_GUMBEL_TAG, c; key = seed)); both
 *               logarithms are gmk_noise_log: u lies in [2^-33, 1 - 2^-33] and -log u in [1.1e-10, 22.9], positive normal doubles
 *   logit       l_c = gmk_noise_log((double)prior[c])
 *   base score  s_c = g_c + l_c, from the priors as they stand at set-up
 *   considered  the m_eff = min(m, children) children with the largest s_c, ties to the lower cell; fixed at set-up together with the
 *               snapshot base_c = visits[c].  r_c = visits[c] - base_c: a kept subtree keeps its statistics without distorting the schedule
 *   value term  qhat_c = (value[c] + 1) / 2 for a child with visits[c] > 0, otherwise (-root_value + 1) / 2: the root's own running mean,
 *               seen from the mover, stands in for the paper's v_mix.  sigma_c = ((c_visit + max_b visits[b]) * c_scale) * qhat_c
 *   schedule    seq[0..n): m_eff == 1: seq[t] = t.  Otherwise L = ceil(log2 m_eff), k = m_eff, c = 0, and while fewer than n entries exist:
 *               extra = max(1, n / (L k)); extra times: k copies of c, c += 1; then k = max(2, k / 2).  Truncated to n.
 *   root step   t = sum of r_c over all children.  t < n: among the considered children with r_c == seq[t] the largest s_c + sigma_c, ties to
 *               the lower cell.  No considered child with that count (a playout was dropped for a full arena), or t >= n: the considered
 *               children with the smallest r_c stand in, under the same maximum.  Below the root the search is PUCB, unchanged.
 *   move        among the considered children with the largest r_c the largest s_c + sigma_c, ties to the lower cell; -1 without children
 *   policy row  over ALL children x_c = l_c + sigma_c (from the priors as they stand when the row is taken: the set-up's, unless the caller
 *               changed them in between), e_c = gmk_noise_exp(x_c - max x), Z = the e_c added in the association of gmk_noise_sum225 in
 *               binary64 (gmk_gumbel_sum225), w_c = (uint16) floor(e_c / Z * 65535 + 0.5): what a record's visit row holds for the ply.
 *               The largest entry is 65535 / Z' with Z' <= 225, so at least 291; the row adds up to 65535 within 225 roundings.
 *
 * Out of scope, here and in the kernels: Gumbel below the root, several leaves per step (GMK_OPT_AZ_LEAVES > 1), proofs and the defence
 * solver (GMK_OPT_AZ_PROOF, GMK_OPT_AZ_VCF_DEFEND), evaluation matches and EvaluationSchedule, NetworkAgent, the ensembles, K3, K6 and K8.
 * Playing strength and training benefit are not measured by the project yet.
 */
#ifndef GOMOKU_GUMBEL_H_
#define GOMOKU_GUMBEL_H_

#include <stdint.h>

#include "gomoku_noise.h"

#define GMK_GUMBEL_FN GMK_NOISE_FN

#define GMK_GUMBEL_TAG 0x676d626cu /* 'gmbl' */
#define GMK_GUMBEL_MAX_SIMS 4096
#define GMK_GUMBEL_CELLS 225

/* g_c */
GMK_GUMBEL_FN double gmk_gumbel_draw(uint32_t game_id, uint32_t stones, uint32_t cell, uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t w[4];
    gmk_noise_philox(game_id, stones, GMK_GUMBEL_TAG, cell, seed_lo, seed_hi, w);
    const double inner = -gmk_noise_log(gmk_noise_uniform(w[0]));
    return -gmk_noise_log(inner);
}

/* l_c */
GMK_GUMBEL_FN double gmk_gumbel_logit(float prior) { return gmk_noise_log((double)prior); }

/* s_c */
GMK_GUMBEL_FN double gmk_gumbel_score(float prior, uint32_t game_id, uint32_t stones, uint32_t cell, uint32_t seed_lo, uint32_t seed_hi) {
    return gmk_gumbel_draw(game_id, stones, cell, seed_lo, seed_hi) + gmk_gumbel_logit(prior);
}

/* qhat_c */
GMK_GUMBEL_FN double gmk_gumbel_qhat(uint32_t visits, float value, float root_value) {
    return visits > 0u ? ((double)value + 1.0) / 2.0 : (-(double)root_value + 1.0) / 2.0;
}

/* sigma_c; max_visits = the largest visits[b] over the root's children */
GMK_GUMBEL_FN double gmk_gumbel_sigma(double c_visit, double c_scale, uint32_t max_visits, double qhat) {
    return ((c_visit + (double)max_visits) * c_scale) * qhat;
}

/* b ranks before c: the larger score, ties to the lower cell */
GMK_GUMBEL_FN int gmk_gumbel_before(double score_b, int b, double score_c, int c) { return score_b > score_c || (score_b == score_c && b < c); }

/* ceil(log2 m) for m >= 1 */
GMK_GUMBEL_FN int gmk_gumbel_levels(int m) {
    int levels = 0;
    while ((1 << levels) < m) ++levels;
    return levels;
}

/* seq[t] for 0 <= t < n, without the sequence: the walk over its phases */
GMK_GUMBEL_FN uint32_t gmk_gumbel_sequence_at(int m_eff, int n, int t) {
    if (m_eff <= 1) return (uint32_t)t;
    const int levels = gmk_gumbel_levels(m_eff);
    int k = m_eff, c = 0, at = 0;
    for (;;) {
        int extra = n / (levels * k);
        if (extra < 1) extra = 1;
        if (t < at + extra * k) return (uint32_t)(c + (t - at) / k);
        at += extra * k;
        c += extra;
        k = k / 2 < 2 ? 2 : k / 2;
    }
}

/* seq[0..n), built as it is stated */
GMK_GUMBEL_FN void gmk_gumbel_sequence(int m_eff, int n, uint32_t* seq) {
    if (m_eff <= 1) {
        for (int t = 0; t < n; ++t) seq[t] = (uint32_t)t;
        return;
    }
    const int levels = gmk_gumbel_levels(m_eff);
    int k = m_eff, c = 0, len = 0;
    while (len < n) {
        int extra = n / (levels * k);
        if (extra < 1) extra = 1;
        for (int e = 0; e < extra; ++e, ++c)
            for (int i = 0; i < k; ++i)
                if (len < n) seq[len++] = (uint32_t)c;
        k = k / 2 < 2 ? 2 : k / 2;
    }
}

/* gmk_noise_sum225 in binary64 */
GMK_GUMBEL_FN double gmk_gumbel_sum225(const double* v) {
    double p[64];
    for (int l = 0; l < 64; ++l) {
        p[l] = v[l];
        for (int j = 1; j < 4; ++j) if (l + 64 * j < 225) p[l] += v[l + 64 * j];
    }
    for (int off = 8; off >= 1; off >>= 1)
        for (int l = 0; l < 64; ++l) p[l] = p[l] + (((l & 15) + off < 16) ? p[l + off] : 0.0);
    return (p[0] + p[16]) + (p[32] + p[48]);
}

/* w_c from e_c and Z */
GMK_GUMBEL_FN uint16_t gmk_gumbel_weight(double e, double z) { return (uint16_t)(uint32_t)(e / z * 65535.0 + 0.5); }

/* Set-up of a root: score[225] (s_c; 0 where there is no child), base[225] (the visits), considered[225] (1 / 0).  Returns m_eff, 0 on a root
 * without children.  The serial statement of gumbel_setup in az_kernel.hip. */
GMK_GUMBEL_FN int gmk_gumbel_setup225(const float* prior, const uint32_t* visits, int m, uint32_t game_id, uint32_t stones, uint32_t seed_lo, uint32_t seed_hi,
                                      double* score, uint32_t* base, uint8_t* considered) {
    int children = 0;
    for (int c = 0; c < 225; ++c) {
        score[c] = prior[c] != 0.0f ? gmk_gumbel_score(prior[c], game_id, stones, (uint32_t)c, seed_lo, seed_hi) : 0.0;
        base[c] = visits[c];
        children += prior[c] != 0.0f ? 1 : 0;
    }
    for (int c = 0; c < 225; ++c) {
        int rank = 0;
        for (int b = 0; b < 225; ++b) rank += (prior[b] != 0.0f && gmk_gumbel_before(score[b], b, score[c], c)) ? 1 : 0;
        considered[c] = (uint8_t)((prior[c] != 0.0f && rank < m) ? 1 : 0);
    }
    return children < m ? children : m;
}

/* the largest visits[b] over the children */
GMK_GUMBEL_FN uint32_t gmk_gumbel_max_visits225(const float* prior, const uint32_t* visits) {
    uint32_t most = 0;
    for (int c = 0; c < 225; ++c) if (prior[c] != 0.0f && visits[c] > most) most = visits[c];
    return most;
}

/* among the considered children with r_c == count: the largest s_c + sigma_c, ties to the lower cell; -1 when there is none */
GMK_GUMBEL_FN int gmk_gumbel_best225(const float* prior, const uint32_t* visits, const float* value, float root_value, const double* score, const uint32_t* base,
                                     const uint8_t* considered, double c_visit, double c_scale, uint32_t count) {
    const uint32_t most = gmk_gumbel_max_visits225(prior, visits);
    int best = -1;
    double best_key = 0.0;
    for (int c = 0; c < 225; ++c) {
        if (prior[c] == 0.0f || !considered[c] || visits[c] - base[c] != count) continue;
        const double key = score[c] + gmk_gumbel_sigma(c_visit, c_scale, most, gmk_gumbel_qhat(visits[c], value[c], root_value));
        if (best < 0 || key > best_key) { best = c; best_key = key; }
    }
    return best;
}

/* The root step of a playout: the cell of the child it descends into, -1 on a root without children.  m_eff: what the set-up returned. */
GMK_GUMBEL_FN int gmk_gumbel_pick225(const float* prior, const uint32_t* visits, const float* value, float root_value, const double* score, const uint32_t* base,
                                     const uint8_t* considered, int m_eff, int n, double c_visit, double c_scale) {
    uint64_t t = 0;
    uint32_t least = 0xFFFFFFFFu;
    for (int c = 0; c < 225; ++c) {
        if (prior[c] == 0.0f) continue;
        t += visits[c] - base[c];
        if (considered[c] && visits[c] - base[c] < least) least = visits[c] - base[c];
    }
    if (least == 0xFFFFFFFFu) return -1;
    if (t < (uint64_t)n) {
        const int cell = gmk_gumbel_best225(prior, visits, value, root_value, score, base, considered, c_visit, c_scale, gmk_gumbel_sequence_at(m_eff, n, (int)t));
        if (cell >= 0) return cell;
    }
    return gmk_gumbel_best225(prior, visits, value, root_value, score, base, considered, c_visit, c_scale, least);
}

/* The move: the cell, or -1 on a root without children */
GMK_GUMBEL_FN int gmk_gumbel_move225(const float* prior, const uint32_t* visits, const float* value, float root_value, const double* score, const uint32_t* base,
                                     const uint8_t* considered, double c_visit, double c_scale) {
    uint32_t most = 0;
    int any = 0;
    for (int c = 0; c < 225; ++c)
        if (prior[c] != 0.0f && considered[c]) { any = 1; if (visits[c] - base[c] > most) most = visits[c] - base[c]; }
    if (!any) return -1;
    return gmk_gumbel_best225(prior, visits, value, root_value, score, base, considered, c_visit, c_scale, most);
}

/* The improved-policy row w[225]; all zeros on a root without children */
GMK_GUMBEL_FN void gmk_gumbel_row225(const float* prior, const uint32_t* visits, const float* value, float root_value, double c_visit, double c_scale, uint16_t* w) {
    const uint32_t most = gmk_gumbel_max_visits225(prior, visits);
    double x[225], e[225], top = 0.0;
    int any = 0;
    for (int c = 0; c < 225; ++c) {
        x[c] = 0.0;
        if (prior[c] == 0.0f) continue;
        x[c] = gmk_gumbel_logit(prior[c]) + gmk_gumbel_sigma(c_visit, c_scale, most, gmk_gumbel_qhat(visits[c], value[c], root_value));
        if (!any || x[c] > top) top = x[c];
        any = 1;
    }
    for (int c = 0; c < 225; ++c) e[c] = prior[c] != 0.0f ? gmk_noise_exp(x[c] - top) : 0.0;
    const double z = gmk_gumbel_sum225(e);
    for (int c = 0; c < 225; ++c) w[c] = prior[c] != 0.0f ? gmk_gumbel_weight(e[c], z) : (uint16_t)0;
}

#endif /* GOMOKU_GUMBEL_H_ */
