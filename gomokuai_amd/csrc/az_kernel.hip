// az_kernel.hip -- K7: network-guided tree search, many games per step (BASELINE.json configs[4]).
//
// The reference's AlphaZero-style agent is MCTS with Policy(eval_state = network.eval_state, c_puct)
// (agents/alphazero.py:5-9): Default::Select, a network call at every new leaf instead of rollouts, Default::Expand with
// the returned probabilities and the legality check, Default::BackPropogate (core/lib/include/algorithms/MonteCarlo.hpp:
// 57-95, core/lib/src/MCTS.cpp:158-177).  One game evaluates ONE position per playout, so a GPU batch comes from running
// many games in lock step; a playout of every game is
//     az_select_kernel      descend to a leaf; finished games at the leaf are backed up at once, the others write the
//                           leaf's feature planes (Board.encoded_states, core/py_ext/src/game_ext.hpp:87-104) as one
//                           row of the batch [n_games][6][15][15]
//     the network           any callable on that batch (PyTorch-ROCm PolicyValueNetwork, network/model_tf.py:28-66)
//     az_expand_kernel      children with the returned priors, value backed up to the root
// all on one HIP stream (the three steps can be captured in a hipGraph and replayed per playout).
// With GMK_OPT_AZ_LEAVES = L > 1 a step takes up to L leaves from every game, steered apart by virtual loss, and the batch has live x L rows:
// az_select_leaves_kernel / az_expand_leaves_kernel, for searches of few games.  The two pairs of kernels are callers of one descent, one leaf
// expansion and one view of a pending leaf (descend, leaf_candidates / write_children / leaf_proofs, pending_leaf).
// With GMK_OPT_AZ_VCF_DEPTH = D > 0 the pending leaves are also handed to K14's exact solver of forced wins by fours (az_vcf_leaves_kernel, right
// behind the select kernel), and the expand kernels answer a solved leaf themselves: include/gomoku_hip.h, "K7 + K14".
// With GMK_OPT_AZ_VCF_DEFEND on top of that and of GMK_OPT_AZ_PROOF the leaves the solver did not answer are asked what the opponent threatens
// (az_threat_leaves_kernel) and which replies lose to it (az_defend_leaves_kernel, K15's table), and the expand kernels mark those children as the
// opponent's proven wins: include/gomoku_hip.h, "K7 + K15".  Those three kernels hold no walk of their own: K14's walk is vcf_device.h's, and
// they are its loaders for a leaf and its endings.
// Mapping: one wavefront per game, lanes over the (<= 225) children; the tree is an SoA arena per game in HBM.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <random>
#include <type_traits>
#include <vector>

#include "board_device.h"
#include "capi_common.h"
#include "host_staging.h"
#include "philox.h"
#include "rollout_device.h"
#include "root_noise.h"
#include "noise_device.h"
#include "vcf_device.h"
#include "../../include/gomoku_sample.h"
#include "../../include/gomoku_gumbel.h"

namespace {

using gmk::five_through;

constexpr int kCells = 225;
constexpr uint32_t kNoNode = 0xFFFFFFFFu;
constexpr uint32_t kStatusOver = 1u;

struct AzHeader {                                // 256 B per game, in HBM
    uint32_t rows[16];                           // root position: black | white << 16 per row
    uint32_t leaf_rows[16];                      // position of the pending leaf
    uint32_t n_nodes, stones, last_move, last_move2;           // cells 0..224, 255 = none
    uint32_t status;                             // bit 0: the game is over (az_advance_kernel), bit 1: node arena full, bit 2: a forced step was not a move of the game
    uint32_t leaf, leaf_pending;                 // node waiting for the network's answer (leaf_pending = 1)
    uint32_t leaf_stones;
    uint32_t quota;                              // several leaves per step: the playouts the game still owes (gmk_az_add_playouts)
    uint32_t n_pending;                          //   leaves waiting for the network's answer (AzLeaves::pend), 0 between steps
    uint32_t vcf_leaves, vcf_wins, vcf_cut;      // K7 + K14 (GMK_OPT_AZ_VCF_DEPTH > 0): pending leaves solved, answered WIN, cut by BUDGET or DEPTH
    uint32_t pad0;
    unsigned long long vcf_nodes;                //   and the nodes their walks counted
    uint32_t proof_proved, proof_stops;          // K7 + proofs (GMK_OPT_AZ_PROOF): nodes given a proof, descents ended at a node already proven
    uint32_t def_threatened, def_marked;         // K7 + K15 (GMK_OPT_AZ_VCF_DEFEND): pending leaves under a WIN threat, children marked WINS
    unsigned long long def_nodes;                //   the nodes of the cells' full solves
    uint32_t def_searched;                       //   and the cells solved in full
    uint32_t pad[9];
};
static_assert(sizeof(AzHeader) == 256 && offsetof(AzHeader, vcf_nodes) % 8 == 0 && offsetof(AzHeader, def_nodes) % 8 == 0, "AzHeader layout");

struct AzTree {
    AzHeader* hdr;
    uint2* stat;                                 // [n_games][cap] {visits, value bits}
    uint2* kids;                                 // [n_games][cap] {first child, children | cell << 8}
    float* prior;                                // [n_games][cap]
    uint32_t* parent;                            // [n_games][cap]
    int cap, n_games;
    double c_puct;
    const int32_t* row_of;                       // [n_games] the row of the leaf batch a game writes to and is answered from: the games still
                                                 // played, in slot order (az_compact_kernel); finished games have none
};

// Default::BackPropogate (MonteCarlo.hpp:90-95): one lane walks the parent chain
__device__ __forceinline__ void backup(uint2* stat, const uint32_t* parent, uint32_t node, float value) {
    for (; node != kNoNode; node = parent[node], value = -value) {
        const uint2 s = stat[node];
        const uint32_t visits = s.x + 1u;
        const float q = __uint_as_float(s.y);
        stat[node] = make_uint2(visits, __float_as_uint(q + (value - q) / static_cast<float>(visits)));
    }
}

// K7 + K14: one verdict per row of the leaf batch, written by az_vcf_leaves_kernel and read by the <true> instantiations of the expand kernels
struct AzVcf {
    int4* verdict;                               // [n_games * GMK_AZ_MAX_LEAVES] {status, move, length, nodes}, owned by the handle
    int max_depth;                               // D
    uint32_t budget;                             // B
};

// lane 0 of the game's expand wavefront: the leaf's verdict goes into the game's counters
__device__ __forceinline__ void count_verdict(AzHeader* hdr, const int4& v) {
    hdr->vcf_leaves += 1u;
    hdr->vcf_wins += v.x == GMK_VCF_WIN ? 1u : 0u;
    hdr->vcf_cut += (v.x == GMK_VCF_BUDGET || v.x == GMK_VCF_DEPTH) ? 1u : 0u;
    hdr->vcf_nodes += static_cast<uint32_t>(v.w);
}

// K7 + K15: per row of the leaf batch, written by az_threat_leaves_kernel and az_defend_leaves_kernel and read by the <true, true, true>
// instantiations of the expand kernels
struct AzDefend {
    int4* threat;                                // [n_games * GMK_AZ_MAX_LEAVES] {status, length, nodes, 1 when the leaf was asked}
    uint8_t* pv;                                 // [rows][GMK_VCF_PV] the threat's line, written for a WIN only
    uint16_t* occupied;                          // [rows][16] the leaf's stones of either colour per board row (the read-out's)
    uint32_t* cells;                             // [rows][225] verdict 0..2, "solved in full" 3, nodes 4..: written for the rows under a WIN threat only
};
constexpr uint32_t kCellVerdict = 7u, kCellSearched = 8u;
constexpr int kCellNodesShift = 4;

// ---- K7 + proofs (GMK_OPT_AZ_PROOF; the contract is in include/gomoku_hip.h, "K7 + proofs") ----
// A node's proof (GMK_AZ_PROOF_*) lives in bits 16..17 of its kids.y word, above the child count and the cell: every reader masks the word, and
// az_keep_subtree copies it whole, so the bits travel through re-rooting.  Only the <true> instantiations below read or write them.
constexpr uint32_t kProofShift = 16u, kProofBits = 3u << kProofShift;
__device__ __forceinline__ uint32_t proof_of(uint32_t kids_y) { return (kids_y >> kProofShift) & 3u; }

// prove(X, s), called by all 64 lanes of the game's wavefront with uniform arguments; stones = the stone count of X's position.  Lane 0 writes
// the bit, a workgroup-scope fence and a barrier stand before the lanes read bits again (the next level's children, the next descent).  LOSES
// makes the parent WINS; WINS makes the parent LOSES only when the parent has a child for every free cell and all of them are WINS -- a ballot
// over the children, as select walks them.  Returns the number of nodes that were given a proof.
__device__ uint32_t az_prove(uint2* kids, const uint32_t* parent, uint32_t x, uint32_t s, int stones, int lane) {
    uint32_t proved = 0;
    for (;;) {
        const uint32_t ky = kids[x].y;
        if (ky & kProofBits) break;
        if (lane == 0) kids[x].y = ky | (s << kProofShift);
        ++proved;
        __threadfence_block();
        __syncthreads();
        const uint32_t p = parent[x];
        if (p == kNoNode) break;
        --stones;                                                // of P's position
        if (s == GMK_AZ_PROOF_WINS) {
            const uint2 pk = kids[p];
            const uint32_t n = pk.y & 0xFFu;
            if (n != static_cast<uint32_t>(kCells - stones)) break;                    // Default::Expand dropped a free cell: an untried reply
            bool all = true;
            for (uint32_t i = lane; i < n; i += 64) all = all && proof_of(kids[pk.x + i].y) == GMK_AZ_PROOF_WINS;
            if (__ballot(!all) != 0ull) break;
        }
        s = s == GMK_AZ_PROOF_WINS ? GMK_AZ_PROOF_LOSES : GMK_AZ_PROOF_WINS;
        x = p;
    }
    return proved;
}
// az_prove in the game's arena, with the nodes it proved added to the game's counter; called as az_prove is
__device__ __forceinline__ void prove_counted(const AzTree& t, size_t arena, AzHeader* hdr, uint32_t x, uint32_t s, int stones, int lane) {
    const uint32_t proved = az_prove(t.kids + arena, t.parent + arena, x, s, stones, lane);
    if (lane == 0) hdr->proof_proved += proved;
}

// The children of a node for a descent: the first child marked LOSES in child order (lose_i, 0xFFFFFFFF: none), and whether children marked
// WINS are left out of the PUCB maximum (some child is not marked WINS).  pb: this lane's children's proofs, two bits per round of 64.
__device__ __forceinline__ void proof_children(const uint2* kids, uint32_t first, uint32_t n, int lane, uint32_t& pb, uint32_t& lose_i, bool& filter) {
    pb = 0u;
    lose_i = 0xFFFFFFFFu;
    bool open = false;
    int j = 0;
    for (uint32_t i = lane; i < n; i += 64, ++j) {
        const uint32_t pr = proof_of(kids[first + i].y);
        pb |= pr << (2 * j);
        if (pr == GMK_AZ_PROOF_LOSES) lose_i = min(lose_i, i);
        open = open || pr != GMK_AZ_PROOF_WINS;
    }
    filter = __ballot(open) != 0ull;
    if (__ballot(lose_i != 0xFFFFFFFFu) != 0ull) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) lose_i = min(lose_i, static_cast<uint32_t>(__shfl_xor(lose_i, s)));
    }
}

// The root choice with proofs, after the old rule has left (best_v, best_i): the first child marked LOSES; otherwise the most visited child
// among those not marked WINS that have a visit, first maximum in child order; otherwise the old rule's.  The same in every lane.
__device__ __forceinline__ void proof_choice(const uint2* kids, const uint2* stat, uint32_t first, uint32_t n, int lane, uint32_t& best_v, uint32_t& best_i) {
    uint32_t lose_i = 0xFFFFFFFFu, pv = 0u, pi = 0xFFFFFFFFu;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t pr = proof_of(kids[first + i].y), v = stat[first + i].x;
        if (pr == GMK_AZ_PROOF_LOSES) lose_i = min(lose_i, i);
        else if (pr != GMK_AZ_PROOF_WINS && v > pv) { pv = v; pi = i; }
    }
    for (int s = 32; s > 0; s >>= 1) {
        lose_i = min(lose_i, static_cast<uint32_t>(__shfl_xor(lose_i, s)));
        const uint32_t ov = __shfl_xor(pv, s), oi = __shfl_xor(pi, s);
        if (ov > pv || (ov == pv && oi < pi)) { pv = ov; pi = oi; }
    }
    if (lose_i != 0xFFFFFFFFu) { best_v = 1u; best_i = lose_i; }
    else if (pv != 0u) { best_v = pv; best_i = pi; }
}

// ---- The root's children, for the kernels that move the root or report it ----
// The child MCTS::stepForward() plays (MCTS.cpp:129-134): the most visited one, first maximum in child order, i.e. ascending cells; under kProof
// proof_choice has the last word.  The index among the root's n children, 0xFFFFFFFF when no child has a visit; the same in every lane.
template <bool kProof>
__device__ __forceinline__ uint32_t most_visited_child(const uint2* kids, const uint2* stat, uint32_t first, uint32_t n, int lane) {
    uint32_t best_v = 0, best_i = 0xFFFFFFFFu;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t v = stat[first + i].x;
        if (v > best_v) { best_v = v; best_i = i; }
    }
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t ov = __shfl_down(best_v, s), oi = __shfl_down(best_i, s);
        if (ov > best_v || (ov == best_v && ov != 0u && oi < best_i)) { best_v = ov; best_i = oi; }
    }
    best_v = __shfl(best_v, 0);
    best_i = __shfl(best_i, 0);
    if constexpr (kProof) proof_choice(kids, stat, first, n, lane, best_v, best_i);
    return best_i;
}
// K20: the first sample_plies plies of a self-play game are drawn in proportion to visits^power (include/gomoku_sample.h has the rule and its
// serial statement, gmk_sample_choose225).  The kernels that take it are the instantiations with one AzSample among their arguments.
struct AzSample {
    const int32_t* slot_game;                    // [n_games] the game a slot plays under gmk_az_set_slots, otherwise null and
    const uint32_t* game_ids;                    // [n_games] the game it plays by gmk_az_set_game_ids
    uint32_t first_game_id, seed_lo, seed_hi;
    uint32_t plies;                              // S > 0
    int power;                                   // k in 1..3
};
// The game whose stream a slot draws from, as az_root_noise_kernel names it
__device__ __forceinline__ uint32_t sample_game_id(const AzSample& sm, int slot) {
    return sm.first_game_id + (sm.slot_game ? static_cast<uint32_t>(max(sm.slot_game[slot], 0)) : sm.game_ids[slot]);
}
// The child a sampled ply plays, called as most_visited_child is and with its result: on a root with `stones` >= S stones, or without weight, it
// IS most_visited_child.  Lane l holds the children 4 l .. 4 l + 3, so child order is lane order: the weights stay in registers, one inclusive
// scan of the lanes' 64-bit sums (six shuffles of two words) gives every lane the prefix before its first child, and the first lane with a
// prefix above the target holds the choice.
template <bool kProof>
__device__ __forceinline__ uint32_t sampled_child(const uint2* kids, const uint2* stat, uint32_t first, uint32_t n, int lane, const AzSample& sm, uint32_t game_id,
                                                  uint32_t stones) {
    if (stones >= sm.plies) return most_visited_child<kProof>(kids, stat, first, n, lane);
    uint64_t w[4], sum = 0;
    uint32_t lose_i = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = 4u * lane + j;
        w[j] = 0;
        if (i < n) {
            w[j] = gmk_sample_weight(stat[first + i].x, sm.power);
            if constexpr (kProof) {
                const uint32_t pr = proof_of(kids[first + i].y);
                if (pr == GMK_AZ_PROOF_LOSES) lose_i = min(lose_i, i);
                if (pr == GMK_AZ_PROOF_WINS) w[j] = 0;
            }
        }
        sum += w[j];
    }
    if constexpr (kProof) {                                      // a proven win is played, not drawn: the first one, which the first such lane holds
        const unsigned long long lost = __ballot(lose_i != 0xFFFFFFFFu);
        if (lost != 0ull) return __shfl(lose_i, __ffsll(static_cast<long long>(lost)) - 1);
    }
    uint64_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t below = __shfl_up(static_cast<unsigned long long>(incl), d);
        if (lane >= d) incl += below;
    }
    const uint64_t total = __shfl(static_cast<unsigned long long>(incl), 63);
    if (total == 0) return most_visited_child<kProof>(kids, stat, first, n, lane);
    const uint64_t target = gmk_sample_target(total, game_id, stones, sm.seed_lo, sm.seed_hi);
    uint64_t prefix = incl - sum;
    uint32_t hit = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        prefix += w[j];
        if (hit == 0xFFFFFFFFu && prefix > target) hit = 4u * lane + j;
    }
    const unsigned long long hits = __ballot(hit != 0xFFFFFFFFu);                      // (never empty: target < total)
    return __shfl(hit, __ffsll(static_cast<long long>(hits)) - 1);
}
// The root choice of a kernel instantiated without an AzSample (most_visited_child, and nothing more is read) or with one (sampled_child for
// the game that slot `slot` plays, at the stones of its header)
template <bool kProof, class... Sample>
__device__ __forceinline__ uint32_t root_child(const uint2* kids, const uint2* stat, uint32_t first, uint32_t n, int lane, const AzHeader& hdr, int slot, const Sample&... sm) {
    static_assert(sizeof...(Sample) <= 1 && (std::is_same_v<Sample, AzSample> && ...), "at most one AzSample");
    if constexpr (sizeof...(Sample) == 1) return sampled_child<kProof>(kids, stat, first, n, lane, sm..., sample_game_id(sm..., slot), hdr.stones);
    else return most_visited_child<kProof>(kids, stat, first, n, lane);
}
// The root's child of `cell` (children are in ascending cell order: at most one), 0xFFFFFFFF when there is none; the same in every lane.
__device__ __forceinline__ uint32_t child_of_cell(const uint2* kids, uint32_t first, uint32_t n, uint32_t cell, int lane) {
    uint32_t found = 0xFFFFFFFFu;
    for (uint32_t i = lane; i < n; i += 64)
        if (((kids[first + i].y >> 8) & 0xFFu) == cell) found = i;
    for (int s = 32; s > 0; s >>= 1) found = min(found, static_cast<uint32_t>(__shfl_xor(found, s)));
    return found;
}
// The root children's visit counts by cell into rv[225], saturated to 65 535.  Called by all 64 lanes under uniform control flow: a barrier
// stands between the zeros and the counts.
__device__ __forceinline__ void visits_by_cell(uint16_t* rv, const uint2* kids, const uint2* stat, uint32_t first, uint32_t n, int lane) {
    for (int i = lane; i < kCells; i += 64) rv[i] = 0;
    __syncthreads();
    for (uint32_t i = lane; i < n; i += 64) rv[(kids[first + i].y >> 8) & 0xFFu] = static_cast<uint16_t>(min(stat[first + i].x, 65535u));
}
// A new root at `base` of the arrays of an AzTree or an AzArena (one lane): no visit, no child, kids_y = the cell that led to it << 8, or 0
template <class Arrays>
__device__ __forceinline__ void new_root(const Arrays& a, size_t base, uint32_t kids_y) {
    a.stat[base] = make_uint2(0u, 0u);
    a.kids[base] = make_uint2(0u, kids_y);
    a.prior[base] = 1.0f;
    a.parent[base] = kNoNode;
}

// Default::Expand's candidates at a leaf (leaf_candidates below).  Lane l holds the cells l + 64 j: the probability, whether the cell becomes a
// child, and its place among the children.  The same in every lane: total, the number of children, and win, the solver answered the leaf WIN.
struct Candidates { float pv[4]; bool take[4]; int rank[4], total; bool win; };

// K7 + K15 in the expand kernels, called by all 64 lanes for a pending leaf that is not answered WIN, after the leaf's children were written
// (created: they exist; a leaf whose playout was dropped for a full arena does not get here): the row's threat is WIN -> the game's counters, every child whose
// cell is GMK_VCF_CELL_LOSES gets GMK_AZ_PROOF_WINS with its own word -- the lane that made the child rewrites it --, and when the leaf has a
// child for every free cell and all are marked: prove(leaf, LOSES).  Returns whether the leaf was proven LOSES (+1.0f is then backed up).
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), s));
    return v;
}
__device__ bool az_defend_marks(const AzTree& t, size_t arena, AzHeader* hdr, const AzDefend& df, size_t row, uint32_t leaf, int leaf_stones,
                                uint32_t first_child, const Candidates& c, bool created, int lane) {
    const int4 th = df.threat[row];
    if (th.x != GMK_VCF_WIN || th.w == 0) return false;          // the same in every lane
    const uint32_t* words = df.cells + row * kCells;
    uint32_t searched = 0, nodes = 0, marked = 0;
    bool all = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        const uint32_t w = i < kCells ? words[i] : 0u;
        searched += (w & kCellSearched) ? 1u : 0u;
        nodes += w >> kCellNodesShift;
        if (created && c.take[j]) {
            if ((w & kCellVerdict) == GMK_VCF_CELL_LOSES) {
                t.kids[arena + first_child + c.rank[j]] = make_uint2(0u, (static_cast<uint32_t>(i) << 8) | (static_cast<uint32_t>(GMK_AZ_PROOF_WINS) << kProofShift));
                ++marked;
            } else all = false;
        }
    }
    searched = wave_sum(searched);
    nodes = wave_sum(nodes);
    marked = wave_sum(marked);
    if (lane == 0) {
        hdr->def_threatened += 1u;
        hdr->def_searched += searched;
        hdr->def_nodes += nodes;
        hdr->def_marked += marked;
        hdr->proof_proved += marked;
    }
    if (!created) return false;
    __threadfence_block();
    __syncthreads();                                             // the children's words, before prove's ballot reads them one level up
    if (c.total != kCells - leaf_stones || __ballot(!all) != 0ull) return false;
    prove_counted(t, arena, hdr, leaf, GMK_AZ_PROOF_LOSES, leaf_stones, lane);
    return true;
}

// ---- K21: Gumbel root search (gmk_az_set_gumbel; the rule and its serial statements are in include/gomoku_gumbel.h) ----
// At the root a playout does not take PUCB's child but the one sequential halving schedules among the Gumbel-top-m children; below it the
// descent is descend_from's, unchanged.  One wavefront per game, and the root is handled BY CELL, as the header states it: the root children's
// prior, visits, value and index are scattered into LDS (GumbelLds), lane l owns the cells l + 64 j, and every step of the rule is the header's
// function on a lane's cells plus a reduction over the wavefront.  Per game in HBM (AzGumbelGame): the base scores s_c, the visit snapshot and the
// considered set, valid while ready[game] != 0.  Set-up is lazy: the first root step (or root choice) that finds children and ready == 0 makes
// it -- ranks are counted against the 225 scores in LDS, nothing is sorted.  Whatever moves or replaces a root clears ready.
struct AzGumbelGame {                            // 2936 B
    double score[kCells];                        // s_c by cell
    uint32_t base[kCells];                       // visits[c] at set-up
    uint8_t considered[kCells], pad[3];
    uint32_t m_eff, pad1;
};
static_assert(sizeof(AzGumbelGame) == 2936, "AzGumbelGame layout");
struct AzGumbel {
    AzGumbelGame* st;                            // [n_games]
    uint32_t* ready;                             // [n_games]
    const int32_t* slot_game;                    // as AzSample's
    const uint32_t* game_ids;
    uint32_t first_game_id, seed_lo, seed_hi;
    int m, n;                                    // max_considered, n_sims
    double c_visit, c_scale;
};
struct GumbelLds {
    double score[kCells];
    float prior[kCells];                         // 0: no child
    uint32_t visits[kCells];
    float value[kCells];
    uint16_t child[kCells + 1];                  // the child's index among the root's children
};
__device__ __forceinline__ uint32_t gumbel_game_id(const AzGumbel& gm, int slot) {
    return gm.first_game_id + (gm.slot_game ? static_cast<uint32_t>(max(gm.slot_game[slot], 0)) : gm.game_ids[slot]);
}
// The root's children by cell into L.  All 64 lanes, uniform control flow; L is complete on return.
__device__ __forceinline__ void gumbel_load(GumbelLds& L, const uint2* kids, const uint2* stat, const float* prior, uint32_t first, uint32_t n, int lane) {
    __syncthreads();                                             // nobody reads an older root's L any more
    for (int c = lane; c < kCells; c += 64) { L.prior[c] = 0.0f; L.visits[c] = 0u; L.value[c] = 0.0f; L.child[c] = 0; }
    __syncthreads();
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t cell = (kids[first + i].y >> 8) & 0xFFu;
        const uint2 s = stat[first + i];
        L.prior[cell] = prior[first + i];
        L.visits[cell] = s.x;
        L.value[cell] = __uint_as_float(s.y);
        L.child[cell] = static_cast<uint16_t>(i);
    }
    __syncthreads();
}
// gmk_gumbel_setup225 for the root in L, into st.  All 64 lanes; st is written and visible to the wavefront on return.
__device__ __forceinline__ void gumbel_setup(GumbelLds& L, AzGumbelGame& st, const AzGumbel& gm, uint32_t game_id, uint32_t stones, uint32_t n, int lane) {
#pragma unroll 1
    for (int c = lane; c < kCells; c += 64)
        L.score[c] = L.prior[c] != 0.0f ? gmk_gumbel_score(L.prior[c], game_id, stones, static_cast<uint32_t>(c), gm.seed_lo, gm.seed_hi) : 0.0;
    __syncthreads();
#pragma unroll 1
    for (int c = lane; c < kCells; c += 64) {
        const bool child = L.prior[c] != 0.0f;
        int rank = 0;
        if (child) {
            const double mine = L.score[c];
            for (int b = 0; b < kCells; ++b) rank += (L.prior[b] != 0.0f && gmk_gumbel_before(L.score[b], b, mine, c)) ? 1 : 0;
        }
        st.score[c] = L.score[c];
        st.base[c] = L.visits[c];
        st.considered[c] = (child && rank < gm.m) ? 1 : 0;
    }
    if (lane == 0) st.m_eff = min(n, static_cast<uint32_t>(gm.m));
    __threadfence_block();
    __syncthreads();
}
// What pick and move read of the root: per cell of this lane the key s_c + sigma_c, r_c and whether it is considered; over the wavefront
// t = the sum of r_c, the smallest and the largest r_c of a considered child, and whether there is one.
struct GumbelView { double key[4]; uint32_t r[4]; bool cons[4]; uint32_t t, least, most; bool any; };
__device__ __forceinline__ GumbelView gumbel_view(const GumbelLds& L, const AzGumbelGame& st, const AzGumbel& gm, float root_value, int lane) {
    GumbelView g;
    uint32_t top = 0u;
    g.t = 0u; g.least = 0xFFFFFFFFu; g.most = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        const bool child = c < kCells && L.prior[c] != 0.0f;
        g.cons[j] = child && st.considered[c] != 0;
        g.r[j] = child ? L.visits[c] - st.base[c] : 0u;
        g.t += g.r[j];
        if (child) top = max(top, L.visits[c]);
        if (g.cons[j]) { g.least = min(g.least, g.r[j]); g.most = max(g.most, g.r[j]); }
    }
    g.t = wave_sum(g.t);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        top = max(top, static_cast<uint32_t>(__shfl_xor(static_cast<int>(top), s)));
        g.least = min(g.least, static_cast<uint32_t>(__shfl_xor(static_cast<int>(g.least), s)));
        g.most = max(g.most, static_cast<uint32_t>(__shfl_xor(static_cast<int>(g.most), s)));
    }
    g.any = g.least != 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        g.key[j] = g.cons[j] ? st.score[c] + gmk_gumbel_sigma(gm.c_visit, gm.c_scale, top, gmk_gumbel_qhat(L.visits[c], L.value[c], root_value)) : 0.0;
    }
    return g;
}
// gmk_gumbel_best225: the cell, -1 when no considered child has that count; the same in every lane
__device__ __forceinline__ int gumbel_best(const GumbelView& g, uint32_t count, int lane) {
    constexpr int kNone = 0x7FFFFFFF;
    double best_key = 0.0;
    int best = kNone;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (g.cons[j] && g.r[j] == count && (best == kNone || g.key[j] > best_key)) { best_key = g.key[j]; best = lane + 64 * j; }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double ok = __shfl_xor(best_key, s);
        const int oc = __shfl_xor(best, s);
        if (oc != kNone && (best == kNone || ok > best_key || (ok == best_key && oc < best))) { best_key = ok; best = oc; }
    }
    return best == kNone ? -1 : best;
}
// gmk_gumbel_pick225 / gmk_gumbel_move225
__device__ __forceinline__ int gumbel_pick(const GumbelView& g, const AzGumbelGame& st, const AzGumbel& gm, int lane) {
    if (!g.any) return -1;
    if (g.t < static_cast<uint32_t>(gm.n)) {
        const int cell = gumbel_best(g, gmk_gumbel_sequence_at(static_cast<int>(st.m_eff), gm.n, static_cast<int>(g.t)), lane);
        if (cell >= 0) return cell;
    }
    return gumbel_best(g, g.least, lane);
}
__device__ __forceinline__ int gumbel_move(const GumbelView& g, int lane) { return g.any ? gumbel_best(g, g.most, lane) : -1; }
// gmk_gumbel_row225 into out[225]; all 64 lanes
__device__ __forceinline__ void gumbel_row(const GumbelLds& L, const AzGumbel& gm, float root_value, uint16_t* out, int lane) {
    uint32_t top_v = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        if (c < kCells && L.prior[c] != 0.0f) top_v = max(top_v, L.visits[c]);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) top_v = max(top_v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(top_v), s)));
    double x[4], top = 0.0;
    bool child[4], any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        child[j] = c < kCells && L.prior[c] != 0.0f;
        x[j] = 0.0;
        if (!child[j]) continue;
        x[j] = gmk_gumbel_logit(L.prior[c]) + gmk_gumbel_sigma(gm.c_visit, gm.c_scale, top_v, gmk_gumbel_qhat(L.visits[c], L.value[c], root_value));
        if (!any || x[j] > top) top = x[j];
        any = true;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double ot = __shfl_xor(top, s);
        const bool oa = __shfl_xor(static_cast<int>(any), s) != 0;
        if (oa && (!any || ot > top)) top = ot;
        any = any || oa;
    }
    double e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = child[j] ? gmk_noise_exp(x[j] - top) : 0.0;
    double p = e[0];                                             // gmk_gumbel_sum225: the lane's cells in order, a tree inside every row of 16 lanes, the four rows
#pragma unroll
    for (int j = 1; j < 4; ++j) if (lane + 64 * j < kCells) p += e[j];
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        const double other = __shfl_down(p, off, 16);
        p = p + (((lane & 15) + off < 16) ? other : 0.0);
    }
    const double z = (__shfl(p, 0) + __shfl(p, 16)) + (__shfl(p, 32) + __shfl(p, 48));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        if (c < kCells) out[c] = child[j] ? gmk_gumbel_weight(e[j], z) : static_cast<uint16_t>(0);
    }
}
// The root choice of the Gumbel forms of az_advance_kernel and az_root_choice_kernel: L is loaded, a root whose set-up is missing (was_ready == 0:
// nothing was searched since it became the root) gets it, and the move follows.  The child's index, 0xFFFFFFFF on a root without children.
__device__ __forceinline__ uint32_t gumbel_child(GumbelLds& L, const AzTree& t, size_t base, uint32_t first, uint32_t n, int lane, uint32_t stones, int slot,
                                                 const AzGumbel& gm, uint32_t was_ready) {
    if (n == 0u) return 0xFFFFFFFFu;
    gumbel_load(L, t.kids + base, t.stat + base, t.prior + base, first, n, lane);
    AzGumbelGame& st = gm.st[slot];
    if (was_ready == 0u) gumbel_setup(L, st, gm, gumbel_game_id(gm, slot), stones, n, lane);
    const GumbelView g = gumbel_view(L, st, gm, __uint_as_float(t.stat[base].y), lane);
    const int cell = gumbel_move(g, lane);
    return cell < 0 ? 0xFFFFFFFFu : static_cast<uint32_t>(L.child[cell]);
}
template <class... Extra>
constexpr bool kIsGumbel = (std::is_same_v<Extra, AzGumbel> || ...);

// ---- Several leaves per game per step, with virtual loss (GMK_OPT_AZ_LEAVES = L > 1) ----
// A search of few games gives the network a batch of few rows; with L leaves per game a step carries live x L rows and a search of P playouts
// takes about P / L steps.  The descents of one step are steered apart by a per-node in-flight count v (a side array, all zero between
// steps): a child with real statistics (N, Q) and v descents in flight below it is scored as if each of them had already come back lost,
//     q_eff = v == 0 ? Q : (Q N - v) / (N + v)      n_i = N + v + 1      sqrt_n = sqrt(N_parent + v_parent)      (all in double)
// which is descend<kProof, true> below; with every v zero it is the one-leaf formula.  Every game owes `quota` playouts
// (gmk_az_add_playouts); a step makes min(L, quota) descents, one after the other:
//     the game is over at the leaf   the real value is backed up at once, quota - 1, no row; the next descent sees the new statistics
//     a childless leaf with v > 0    it waits for the network already (a collision): the step's descents end here, nothing is counted
//     otherwise                      v + 1 from the root to the leaf, the leaf is the k-th pending leaf, its planes are row row_of * L + k,
//                                    quota - 1
// and the rows k >= n_pending of the game's L rows are zeros.  The first descent of a step cannot collide, so a game that owes playouts
// completes at least one per step.  az_expand_leaves_kernel answers the pending leaves in their order (which fixes the node numbering):
// Default::Expand from row k, -value[row] backed up -- or status bit 1 and no backup where the children do not fit --, v - 1 from the leaf up.
// Lane 0 writes the marks, the backups and the row words; the 64 lanes read them in the next descent: a workgroup-scope fence and a barrier
// stand between the two (nothing is shared between games).  One wavefront per game, no synchronisation with the host.
struct AzPending {                               // 80 B
    uint32_t node, stones, pad[2];
    uint32_t rows[16];                           // the leaf's position
};
struct AzLeaves {
    uint16_t* inflight;                          // [n_games][cap] v: descents that passed through the node and wait for the network
    AzPending* pend;                             // [n_games][GMK_AZ_MAX_LEAVES]
    int leaves;                                  // L
};

// ---- What the one-leaf kernels and the L > 1 kernels share: a pending leaf, the descent, the game's end, the planes, the expansion ----
// A pending leaf, wherever it is kept: the header's leaf words at L = 1, pend[k] otherwise.  waiting: it waits for an answer; rows: its sixteen words.
struct PendingLeaf { bool waiting; uint32_t node, stones; const uint32_t* rows; };
template <bool kMany>
__device__ __forceinline__ PendingLeaf pending_leaf(const AzHeader* hdr, const AzPending* pend, int k) {
    if constexpr (kMany) return {static_cast<uint32_t>(k) < hdr->n_pending, pend[k].node, pend[k].stones, pend[k].rows};
    else return {hdr->leaf_pending != 0u, hdr->leaf, hdr->leaf_stones, hdr->leaf_rows};
}
__device__ __forceinline__ PendingLeaf pending_leaf(const AzTree& t, const AzLeaves& lv, int game, int k) {
    const AzHeader* hdr = t.hdr + game;
    return lv.leaves > 1 ? pending_leaf<true>(hdr, lv.pend + static_cast<size_t>(game) * GMK_AZ_MAX_LEAVES, k) : pending_leaf<false>(hdr, nullptr, 0);
}

// Default::Select (MonteCarlo.hpp:57-68) from the root down to a leaf.  Called by all 64 lanes of the game's wavefront under uniform control
// flow: lane 0 puts every stone of the path into s_rows (which holds the root position) and a barrier stands behind each.
// kProof: the descent stops at a proven node below the root (stopped: its proof), children marked LOSES are taken and children marked WINS
// avoided.  kInflight: the in-flight counts steer it (the formula above); <.., false> neither loads nor adds them.
struct Descent { uint32_t node; int stones; uint32_t last, last2, stopped; };     // where it ended, with the position's stone count and last two moves
// descend_from: the same from the node d names, whose stones are in s_rows already (K21: the root step is not PUCB's).
template <bool kProof, bool kInflight>
__device__ __forceinline__ Descent descend_from(Descent d, const uint2* stat, const uint2* kids, const float* prior, const uint16_t* inflight, uint32_t* s_rows,
                                                double c_puct, int lane) {
    for (;;) {
        const uint2 k = kids[d.node];
        if constexpr (kProof) {
            if (d.node != 0u && (k.y & kProofBits)) { d.stopped = proof_of(k.y); break; }
        }
        const uint32_t first = k.x, n = k.y & 0xFFu;
        if (n == 0) break;
        uint32_t pb = 0u, lose_i = 0xFFFFFFFFu;
        bool filter = false;
        if constexpr (kProof) proof_children(kids, first, n, lane, pb, lose_i, filter);
        uint32_t n_node = stat[d.node].x;
        if constexpr (kInflight) n_node += static_cast<uint32_t>(inflight[d.node]);
        const double sqrt_n = sqrt(static_cast<double>(n_node));
        double best_score = -1.0;
        uint32_t best_i = 0xFFFFFFFFu;
        int j = 0;
        for (uint32_t i = lane; i < n; i += 64, ++j) {
            if constexpr (kProof) { if (filter && ((pb >> (2 * j)) & 3u) == GMK_AZ_PROOF_WINS) continue; }
            const uint2 cs = stat[first + i];
            double q = static_cast<double>(__uint_as_float(cs.y));
            uint32_t n_child = cs.x + 1u;
            if constexpr (kInflight) {
                const uint32_t v_i = inflight[first + i];
                q = v_i == 0u ? q : (q * static_cast<double>(cs.x) - static_cast<double>(v_i)) / static_cast<double>(cs.x + v_i);
                n_child = cs.x + v_i + 1u;
            }
            const double p_i = prior[first + i], n_i = static_cast<double>(n_child);
            const double score = q + c_puct * p_i * sqrt_n / n_i;                      // Q + PUCB (:23-28)
            if (score > best_score) { best_score = score; best_i = i; }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {                                             // first maximum, strict '>'
            const double os = __shfl_down(best_score, s);
            const uint32_t oi = __shfl_down(best_i, s);
            if (os > best_score || (os == best_score && oi < best_i)) { best_score = os; best_i = oi; }
        }
        best_i = __shfl(best_i, 0);
        if (best_i == 0xFFFFFFFFu) best_i = 0;                                          // nothing beat the initial -1.0: the first child
        if constexpr (kProof) { if (lose_i != 0xFFFFFFFFu) best_i = lose_i; }
        d.node = first + best_i;
        const uint32_t cell = (kids[d.node].y >> 8) & 0xFFu;
        if (lane == 0) s_rows[cell / 15] |= 1u << (cell % 15 + ((d.stones & 1) ? 16 : 0));                          // Policy::applyMove: black moves on even counts
        __syncthreads();
        ++d.stones;
        d.last2 = d.last;
        d.last = cell;
    }
    return d;
}
template <bool kProof, bool kInflight>
__device__ __forceinline__ Descent descend(const uint2* stat, const uint2* kids, const float* prior, const uint16_t* inflight, uint32_t* s_rows, double c_puct,
                                           int stones, uint32_t last, uint32_t last2, int lane) {
    return descend_from<kProof, kInflight>(Descent{0u, stones, last, last2, GMK_AZ_PROOF_NONE}, stat, kids, prior, inflight, s_rows, c_puct, lane);
}

// Board::checkGameEnd (Game.cpp:88-136): five through the last stone (winner: +1 black, -1 white), or a full board
__device__ __forceinline__ bool game_end(const uint32_t* s_rows, int stones, uint32_t last, int& winner) {
    winner = 0;
    if (stones > 0 && last < 225u) {
        const int mover_white = (stones - 1) & 1;
        if (five_through<1>(s_rows, last % 15, last / 15, mover_white ? 16 : 0)) { winner = mover_white ? -1 : 1; return true; }
    }
    return stones == kCells;
}
// Whether the descent's value is known without the network, all 64 lanes: it stopped at a proven node (the exact value is backed up), or the game
// is over at the node: CalcScore(node.player, winner) (Game.h:34-36) is backed up -- the node's player is the one who made the last move --, and
// under kProof a five proves that the side to move at the node has lost.  The proof stop comes before the game-end test.
template <bool kProof>
__device__ __forceinline__ bool settled_at_once(const AzTree& t, size_t arena, AzHeader* hdr, const uint32_t* s_rows, const Descent& d, int lane) {
    if (kProof && d.stopped != GMK_AZ_PROOF_NONE) {
        if (lane == 0) { backup(t.stat + arena, t.parent + arena, d.node, d.stopped == GMK_AZ_PROOF_LOSES ? 1.0f : -1.0f); hdr->proof_stops += 1u; }
        return true;
    }
    int winner;
    if (!game_end(s_rows, d.stones, d.last, winner)) return false;
    const int node_player = (d.stones & 1) ? 1 : -1;
    if (lane == 0) backup(t.stat + arena, t.parent + arena, d.node, static_cast<float>(node_player * winner));
    if constexpr (kProof) { if (winner != 0) prove_counted(t, arena, hdr, d.node, GMK_AZ_PROOF_LOSES, d.stones, lane); }
    return true;
}

// Board.encoded_states (game_ext.hpp:87-104), one row of the batch: own stones, opponent's, empties, last move, the one before, colour to move
__device__ __forceinline__ void write_planes(float* out, const uint32_t* s_rows, int stones, uint32_t last, uint32_t last2, int lane) {
    const int cur_white = stones & 1;
    for (int i = lane; i < kCells; i += 64) {
        const uint32_t row = s_rows[i / 15] >> (i % 15);
        const bool black = row & 1u, white = (row >> 16) & 1u;
        out[0 * kCells + i] = (cur_white ? white : black) ? 1.0f : 0.0f;
        out[1 * kCells + i] = (cur_white ? black : white) ? 1.0f : 0.0f;
        out[2 * kCells + i] = (!black && !white) ? 1.0f : 0.0f;
        out[3 * kCells + i] = static_cast<uint32_t>(i) == last ? 1.0f : 0.0f;
        out[4 * kCells + i] = static_cast<uint32_t>(i) == last2 ? 1.0f : 0.0f;
        out[5 * kCells + i] = cur_white ? 0.0f : 1.0f;
    }
}
// a row of the batch that no leaf fills
__device__ __forceinline__ void zero_row(float* out, int lane) {
    for (int i = lane; i < 6 * kCells; i += 64) out[i] = 0.0f;
}

// Default::Expand with extraCheck (MonteCarlo.hpp:71-80) for the leaf of batch row `row` at position `rows`: probability not 0 and the cell is
// free; ascending cell id.  kVcf: the row's verdict comes first (lane 0 counts it) -- on WIN the answer is one-hot(move), not the network's row.
template <bool kVcf>
__device__ __forceinline__ Candidates leaf_candidates(const AzVcf& vc, AzHeader* hdr, const float* probs, size_t row, const uint32_t* rows, int lane) {
    Candidates c;
    c.win = false;
    c.total = 0;
    int win_cell = -1;
    if constexpr (kVcf) {
        const int4 v = vc.verdict[row];
        c.win = v.x == GMK_VCF_WIN;
        win_cell = v.y;
        if (lane == 0) count_verdict(hdr, v);
    }
    const float* p = probs + row * kCells;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        c.pv[j] = i < kCells ? p[i] : 0.0f;
        if constexpr (kVcf) { if (c.win) c.pv[j] = i == win_cell ? 1.0f : 0.0f; }
        const uint32_t row = i < kCells ? rows[i / 15] >> (i % 15) : 0x10001u;
        c.take[j] = i < kCells && c.pv[j] != 0.0f && !(row & 0x10001u);
        const unsigned long long b = __ballot(c.take[j]);
        c.rank[j] = c.total + static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u)));
        c.total += __popcll(b);
    }
    return c;
}
// The candidates become the leaf's children at n_nodes .. n_nodes + total, and lane 0 writes the leaf's kids word: leaf_proofs' fence and barrier
// stand before the 64 lanes read it.  The caller has checked that they fit.
__device__ __forceinline__ void write_children(const AzTree& t, size_t arena, uint32_t leaf, uint32_t n_nodes, const Candidates& c, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c.take[j]) {
            const uint32_t child = n_nodes + c.rank[j];
            t.stat[arena + child] = make_uint2(0u, 0u);
            t.kids[arena + child] = make_uint2(0u, static_cast<uint32_t>(lane + 64 * j) << 8);
            t.prior[arena + child] = c.pv[j];
            t.parent[arena + child] = leaf;
        }
    if (lane == 0) {
        const uint32_t cell_bits = t.kids[arena + leaf].y & 0xFF00u;
        t.kids[arena + leaf] = make_uint2(n_nodes, static_cast<uint32_t>(c.total) | cell_bits);
    }
}
// Between the children and the backup, called by all 64 lanes under uniform control flow: the fence behind the children's writes and, under kProof,
// the barrier; kProof: a leaf answered WIN whose child exists is proven WINS; kDefend: the children that lose to the opponent's forced win are
// marked (not for a leaf answered WIN or dropped for a full arena).  created: the children at first_child exist.  Returns whether the leaf was
// proven LOSES: +1.0f is then the value to back up.
template <bool kProof, bool kDefend>
__device__ __forceinline__ bool leaf_proofs(const AzTree& t, size_t arena, AzHeader* hdr, const AzDefend& df, size_t row, const PendingLeaf& pl, uint32_t first_child,
                                            const Candidates& c, bool created, bool dropped, int lane) {
    __threadfence_block();
    if constexpr (kProof) {
        __syncthreads();                                         // the leaf's new kids word, before the 64 lanes read it
        if (c.win && created) prove_counted(t, arena, hdr, pl.node, GMK_AZ_PROOF_WINS, static_cast<int>(pl.stones), lane);
    }
    if constexpr (kDefend) {
        if (!c.win && !dropped) return az_defend_marks(t, arena, hdr, df, row, pl.node, static_cast<int>(pl.stones), first_child, c, created, lane);
    }
    return false;
}

// kProof: see descend; a five at the leaf starts a proof.  <false> is the search without the proof bits.
template <bool kProof>
__global__ __launch_bounds__(64)
void az_select_kernel(AzTree t, float* __restrict__ out_states) {
    __shared__ uint32_t s_rows[16];
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    AzHeader* hdr = t.hdr + game;
    if (hdr->status & kStatusOver) return;                       // the game is over (az_advance_kernel): nothing to search, leaf_pending stays 0
    const size_t row = static_cast<size_t>(t.row_of[game]);
    const size_t arena = static_cast<size_t>(game) * t.cap;
    if (lane < 16) s_rows[lane] = hdr->rows[lane];
    __syncthreads();
    const Descent d = descend<kProof, false>(t.stat + arena, t.kids + arena, t.prior + arena, nullptr, s_rows, t.c_puct, static_cast<int>(hdr->stones),
                                             hdr->last_move, hdr->last_move2, lane);
    if (settled_at_once<kProof>(t, arena, hdr, s_rows, d, lane)) {                     // no network row
        if (lane == 0) hdr->leaf_pending = 0;
        if (out_states) zero_row(out_states + row * 6 * kCells, lane);
        return;
    }
    if (lane == 0) { hdr->leaf = d.node; hdr->leaf_pending = 1; hdr->leaf_stones = static_cast<uint32_t>(d.stones); }
    if (lane < 16) hdr->leaf_rows[lane] = s_rows[lane];
    write_planes(out_states + row * 6 * kCells, s_rows, d.stones, d.last, d.last2, lane);
}

// K21: az_select_kernel<false> with the Gumbel root step.  A root without children is the leaf, as it is there: the playout that expands it is
// just a playout, and the next one makes the set-up.
__global__ __launch_bounds__(64)
void az_select_gumbel_kernel(AzTree t, float* __restrict__ out_states, AzGumbel gm) {
    __shared__ uint32_t s_rows[16];
    __shared__ GumbelLds s_g;
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    AzHeader* hdr = t.hdr + game;
    if (hdr->status & kStatusOver) return;
    const size_t row = static_cast<size_t>(t.row_of[game]);
    const size_t arena = static_cast<size_t>(game) * t.cap;
    if (lane < 16) s_rows[lane] = hdr->rows[lane];
    __syncthreads();
    Descent d{0u, static_cast<int>(hdr->stones), hdr->last_move, hdr->last_move2, GMK_AZ_PROOF_NONE};
    const uint2 rk = t.kids[arena];
    const uint32_t first = rk.x, n = rk.y & 0xFFu;
    if (n != 0u) {
        gumbel_load(s_g, t.kids + arena, t.stat + arena, t.prior + arena, first, n, lane);
        AzGumbelGame& st = gm.st[game];
        if (gm.ready[game] == 0u) {
            gumbel_setup(s_g, st, gm, gumbel_game_id(gm, game), hdr->stones, n, lane);
            if (lane == 0) gm.ready[game] = 1u;
        }
        const GumbelView g = gumbel_view(s_g, st, gm, __uint_as_float(t.stat[arena].y), lane);
        const int cell = gumbel_pick(g, st, gm, lane);              // (never -1: a root with children has a considered one)
        if (cell >= 0) {
            d.node = first + s_g.child[cell];
            if (lane == 0) s_rows[cell / 15] |= 1u << (cell % 15 + ((d.stones & 1) ? 16 : 0));
            __syncthreads();
            ++d.stones;
            d.last2 = d.last;
            d.last = static_cast<uint32_t>(cell);
            d = descend_from<false, false>(d, t.stat + arena, t.kids + arena, t.prior + arena, nullptr, s_rows, t.c_puct, lane);
        }
    }
    if (settled_at_once<false>(t, arena, hdr, s_rows, d, lane)) {
        if (lane == 0) hdr->leaf_pending = 0;
        if (out_states) zero_row(out_states + row * 6 * kCells, lane);
        return;
    }
    if (lane == 0) { hdr->leaf = d.node; hdr->leaf_pending = 1; hdr->leaf_stones = static_cast<uint32_t>(d.stones); }
    if (lane < 16) hdr->leaf_rows[lane] = s_rows[lane];
    write_planes(out_states + row * 6 * kCells, s_rows, d.stones, d.last, d.last2, lane);
}

// kVcf: the leaf's verdict comes first (GMK_OPT_AZ_VCF_DEPTH > 0) -- on WIN the answer is (1.0f, one-hot(move)) instead of the network's row
// kProof (with kVcf): a leaf answered WIN whose child was created is proven WINS
// kDefend (with both): the children that lose to the opponent's forced win are marked, and a leaf without a holding reply is proven LOSES
template <bool kVcf, bool kProof, bool kDefend>
__global__ __launch_bounds__(64)
void az_expand_kernel(AzTree t, const float* __restrict__ values, const float* __restrict__ probs, int stages /* bit 0: expand, bit 1: back up */, AzVcf vc,
                      AzDefend df) {
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    AzHeader* hdr = t.hdr + game;
    const PendingLeaf pl = pending_leaf<false>(hdr, nullptr, 0);
    if (!pl.waiting) return;
    const size_t row = static_cast<size_t>(t.row_of[game]);
    const size_t arena = static_cast<size_t>(game) * t.cap;
    const uint32_t n_nodes = hdr->n_nodes;
    const Candidates c = leaf_candidates<kVcf>(vc, hdr, probs, row, pl.rows, lane);
    const bool created = c.total > 0 && (stages & 1);
    if (created) {
        if (n_nodes + c.total > static_cast<uint32_t>(t.cap)) {
            if (lane == 0) { hdr->status |= 2u; hdr->leaf_pending = 0; }               // arena full: this playout is dropped
            return;
        }
        write_children(t, arena, pl.node, n_nodes, c, lane);
        if (lane == 0) hdr->n_nodes = n_nodes + c.total;
    }
    const bool lost = leaf_proofs<kProof, kDefend>(t, arena, hdr, df, row, pl, n_nodes, c, created, false, lane);
    if (lane == 0) {
        if (stages & 2) backup(t.stat + arena, t.parent + arena, pl.node, lost ? 1.0f : c.win ? -1.0f : -values[row]);  // node_value = -state_value (MCTS.cpp:166-168)
        hdr->leaf_pending = 0;
    }
}

template <bool kProof>
__global__ __launch_bounds__(64)
void az_select_leaves_kernel(AzTree t, AzLeaves lv, float* out_states) {
    __shared__ uint32_t s_rows[16];
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    AzHeader* hdr = t.hdr + game;
    if (hdr->status & kStatusOver) return;                       // the game is over: it owes nothing and has no rows
    const size_t row0 = static_cast<size_t>(t.row_of[game]) * lv.leaves;
    const size_t arena = static_cast<size_t>(game) * t.cap;
    const uint32_t* parent = t.parent + arena;
    uint16_t* inflight = lv.inflight + arena;
    AzPending* pend = lv.pend + static_cast<size_t>(game) * GMK_AZ_MAX_LEAVES;
    uint32_t quota = hdr->quota;
    const int descents = static_cast<int>(min(static_cast<uint32_t>(lv.leaves), quota));
    const int root_stones = static_cast<int>(hdr->stones);
    const uint32_t root_last = hdr->last_move, root_last2 = hdr->last_move2;
    int k = 0;                                                   // pending leaves so far
    for (int i = 0; i < descents; ++i) {
        if (lane < 16) s_rows[lane] = hdr->rows[lane];
        __syncthreads();
        const Descent d = descend<kProof, true>(t.stat + arena, t.kids + arena, t.prior + arena, inflight, s_rows, t.c_puct, root_stones, root_last, root_last2, lane);
        bool collided = false;
        if (settled_at_once<kProof>(t, arena, hdr, s_rows, d, lane)) {
            --quota;
        } else if (inflight[d.node] != 0) {
            collided = true;
        } else {
            if (lane == 0) {
                for (uint32_t up = d.node; up != kNoNode; up = parent[up]) inflight[up] = static_cast<uint16_t>(inflight[up] + 1u);
                pend[k].node = d.node;
                pend[k].stones = static_cast<uint32_t>(d.stones);
            }
            if (lane < 16) pend[k].rows[lane] = s_rows[lane];
            write_planes(out_states + (row0 + static_cast<size_t>(k)) * 6 * kCells, s_rows, d.stones, d.last, d.last2, lane);
            ++k;
            --quota;
        }
        __threadfence_block();                                   // lane 0's marks and backups, before the next descent reads them
        __syncthreads();                                         // (and every lane is done with s_rows)
        if (collided) break;
    }
    for (int r = k; r < lv.leaves; ++r) zero_row(out_states + (row0 + static_cast<size_t>(r)) * 6 * kCells, lane);
    if (lane == 0) { hdr->quota = quota; hdr->n_pending = static_cast<uint32_t>(k); hdr->leaf_pending = 0; }
}

template <bool kVcf, bool kProof, bool kDefend>
__global__ __launch_bounds__(64)
void az_expand_leaves_kernel(AzTree t, AzLeaves lv, const float* values, const float* probs, AzVcf vc, AzDefend df) {
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    AzHeader* hdr = t.hdr + game;
    const int n_pending = static_cast<int>(hdr->n_pending);
    if (n_pending == 0) return;
    const size_t row0 = static_cast<size_t>(t.row_of[game]) * lv.leaves;
    const size_t arena = static_cast<size_t>(game) * t.cap;
    uint16_t* inflight = lv.inflight + arena;
    const AzPending* pend = lv.pend + static_cast<size_t>(game) * GMK_AZ_MAX_LEAVES;
    uint32_t n_nodes = hdr->n_nodes;
    bool full = false;
    for (int k = 0; k < n_pending; ++k) {
        const PendingLeaf pl = pending_leaf<true>(hdr, pend, k);
        const size_t row = row0 + static_cast<size_t>(k);
        const Candidates c = leaf_candidates<kVcf>(vc, hdr, probs, row, pl.rows, lane);
        const uint32_t first_child = n_nodes;
        const bool dropped = c.total > 0 && n_nodes + c.total > static_cast<uint32_t>(t.cap);
        if (dropped) {
            full = true;                                         // arena full: this playout is dropped, its marks are taken back below
        } else if (c.total > 0) {
            write_children(t, arena, pl.node, n_nodes, c, lane);
            n_nodes += c.total;
        }
        const bool lost = leaf_proofs<kProof, kDefend>(t, arena, hdr, df, row, pl, first_child, c, c.total > 0 && !dropped, dropped, lane);
        if (lane == 0) {
            if (!dropped) backup(t.stat + arena, t.parent + arena, pl.node, lost ? 1.0f : c.win ? -1.0f : -values[row]);
            for (uint32_t up = pl.node; up != kNoNode; up = t.parent[arena + up]) inflight[up] = static_cast<uint16_t>(inflight[up] - 1u);
        }
    }
    if (lane == 0) {
        hdr->n_nodes = n_nodes;
        if (full) hdr->status |= 2u;
        hdr->n_pending = 0;
    }
}


// ---- K7 + K14: forced wins by fours at the pending leaves (GMK_OPT_AZ_VCF_DEPTH = D > 0) ----
// The three kernels below run K14's walk (the contract in include/gomoku_hip.h "K14"), which is vcf_device.h's: pass, start and step, one board
// ROW per lane, sixteen lanes per leaf.  What stands here is their loaders and their endings.  Lane y reads ONE word of the leaf's sixteen
// (black | white << 16; word 15 is zero) and splits it into attacker and defender by the leaf's stone count: no move list exists and none is
// built.  A pending leaf is a position the select kernel built from legal moves, so K14's BAD cannot arise; OVER can, from a root given with a
// five on it.  The walks are in plain mode (no iterative deepening).  No float, no atomics, no barrier, nothing allocated.

// Row `item` of a launch over n_games * L leaves is game item / L's leaf item % L.  False where there is no such leaf or the game is finished;
// the live games' leaves are found by skipping, which is row_of read forwards: out_row = row_of[game] * L + k is the leaf's row of the batch.
__device__ __forceinline__ bool leaf_of(const AzTree& t, const AzLeaves& lv, long long item, int& game, int& k, size_t& out_row) {
    if (item >= static_cast<long long>(t.n_games) * lv.leaves) return false;
    game = static_cast<int>(item / lv.leaves);
    k = static_cast<int>(item - static_cast<long long>(game) * lv.leaves);
    if (t.hdr[game].status & kStatusOver) return false;
    out_row = static_cast<size_t>(t.row_of[game]) * lv.leaves + static_cast<size_t>(k);
    return true;
}
// This lane's word of a pending leaf: the leaf's row y of black and of white; white is to move on odd stone counts.
struct LeafRow {
    uint32_t black, white;
    bool white_to_move;
};
__device__ __forceinline__ LeafRow leaf_row(const PendingLeaf& pl, int y) {
    const uint32_t word = pl.rows[y];
    return {word & gmk::vcf::kRowMask, (word >> 16) & gmk::vcf::kRowMask, (pl.stones & 1u) != 0};
}

// The side to move attacks.  Four leaves per wavefront, one wavefront per workgroup: group i of the launch takes row i (leaf_of); a leaf that
// is not pending leaves the group idle.  The verdict goes to the leaf's row of the batch; no principal variation is kept beyond the first move.
__global__ __launch_bounds__(64)
void az_vcf_leaves_kernel(AzTree t, AzLeaves lv, AzVcf vc) {
    namespace V = gmk::vcf;
    __shared__ V::Stack stack;
    const V::Lane ln;
    V::Walk w;
    w.limit = vc.max_depth;
    int game = 0, k = 0;
    size_t out_row = 0;

    // ---- the loader ----
    if (leaf_of(t, lv, static_cast<long long>(blockIdx.x) * 4 + ln.group, game, k, out_row)) {
        const PendingLeaf pl = pending_leaf(t, lv, game, k);
        if (pl.waiting) {
            const LeafRow r = leaf_row(pl, ln.y);
            w.reset(r.white_to_move ? r.white : r.black, r.white_to_move ? r.black : r.white, vc.max_depth);
        } else if (ln.y == 0) {
            vc.verdict[out_row] = make_int4(GMK_VCF_NONE, -1, 0, 0);
        }
    }

    // The group's verdict.  first = the cell that ends a winning line at the root (depth 0), else the first move is on the stack.
    const auto finish = [&](int status, int first, int tail) {
        const bool win = status == GMK_VCF_WIN;
        if (ln.y == 0)
            vc.verdict[out_row] = make_int4(status, !win ? -1 : w.depth > 0 ? V::level_c(stack[0][ln.lane]) : first, !win ? 0 : w.depth + tail,
                                            static_cast<int>(w.nodes));
        w.state = V::kIdle;
    };
    // The walk has failed at the root, with every move undone.
    const auto failed = [&]() { finish(w.cut ? GMK_VCF_DEPTH : GMK_VCF_NONE, -1, 0); };

    while (__ballot(w.state != V::kIdle) != 0ull) {
        const V::Pass ps = V::pass(w, ln);
        if (w.state == V::kInit) {
            if (ps.over) finish(GMK_VCF_OVER, -1, 0);
            else if (ps.f1 >= 0) finish(GMK_VCF_WIN, ps.f1, 1);
            else V::start(w, ps, failed);
        } else if (w.state == V::kRun) {
            V::step(w, ln, ps, vc.budget, stack, [&](int c, int, int) { finish(GMK_VCF_WIN, c, 2); }, [&]() { finish(GMK_VCF_BUDGET, -1, 0); }, failed);
        }
    }
}

// ---- K7 + K15: the replies that lose to a forced win by fours, at the pending leaves (GMK_OPT_AZ_VCF_DEFEND; include/gomoku_hip.h "K7 + K15") ----
// Two further links of gmk_az_select's chain behind az_vcf_leaves_kernel, for a handle whose solver and proofs are on.
// az_threat_leaves_kernel is that kernel with the colours swapped -- the side that is NOT to move attacks, as if the side to move had passed
// (K14's GMK_VCF_OPPONENT) -- and the line kept: on WIN every lane writes its four cells of the pv, the levels' (c, r) from the LDS stack and the
// cells that end the line, as vcf_kernel's finish does.  A row whose own verdict (the kernel before, in stream order) is WIN or OVER, or that
// has no pending leaf, reads {NONE, 0, 0, not asked}.  Lane y also leaves the leaf's occupied cells of row y for the read-out.
__global__ __launch_bounds__(64)
void az_threat_leaves_kernel(AzTree t, AzLeaves lv, AzVcf vc, AzDefend df) {
    namespace V = gmk::vcf;
    __shared__ V::Stack stack;
    const V::Lane ln;
    const int y = ln.y;
    V::Walk w;
    w.limit = vc.max_depth;
    int game = 0, k = 0;
    size_t out_row = 0;

    // ---- the loader ----
    if (leaf_of(t, lv, static_cast<long long>(blockIdx.x) * 4 + ln.group, game, k, out_row)) {
        const PendingLeaf pl = pending_leaf(t, lv, game, k);
        bool pending = pl.waiting;
        if (pending) {
            const int own = vc.verdict[out_row].x;
            pending = own != GMK_VCF_WIN && own != GMK_VCF_OVER;
        }
        if (pending) {
            const LeafRow r = leaf_row(pl, y);
            w.reset(r.white_to_move ? r.black : r.white, r.white_to_move ? r.white : r.black, vc.max_depth);      // the side that moved last threatens
            df.occupied[out_row * 16 + y] = static_cast<uint16_t>(r.black | r.white);
        } else if (y == 0) {
            df.threat[out_row] = make_int4(GMK_VCF_NONE, 0, 0, 0);
        }
    }

    // The group's threat.  t0 .. t2 are the cells that end a winning line after the 2 * depth cells on the stack (255: none).
    const auto finish = [&](int status, int t0, int t1, int t2) {
        const bool win = status == GMK_VCF_WIN;
        if (y == 0) df.threat[out_row] = make_int4(status, !win ? 0 : w.depth + (t1 == 255 ? 1 : 2), static_cast<int>(w.nodes), 1);
        if (win) {
            uint32_t line = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) line |= V::line_cell(stack, ln, w.depth, 4 * y + i, t0, t1, t2) << (8 * i);
            reinterpret_cast<uint32_t*>(df.pv + out_row * GMK_VCF_PV)[y] = line;
        }
        w.state = V::kIdle;
    };
    const auto failed = [&]() { finish(w.cut ? GMK_VCF_DEPTH : GMK_VCF_NONE, 255, 255, 255); };

    while (__ballot(w.state != V::kIdle) != 0ull) {
        const V::Pass ps = V::pass(w, ln);
        if (w.state == V::kInit) {
            if (ps.over) finish(GMK_VCF_OVER, 255, 255, 255);
            else if (ps.f1 >= 0) finish(GMK_VCF_WIN, ps.f1, 255, 255);
            else V::start(w, ps, failed);
        } else if (w.state == V::kRun) {
            V::step(w, ln, ps, vc.budget, stack, [&](int c, int f1, int f2) { finish(GMK_VCF_WIN, c, f1, f2); },
                    [&]() { finish(GMK_VCF_BUDGET, 255, 255, 255); }, failed);
        }
    }
}

// az_defend_leaves_kernel is vcf_defend_kernel's launch two around the leaf loader: one job per (row, cell), one 16-lane group per job, follow
// against the threat's line first and K14's full walk of P + c with the whole budget only after FAIL.  Jobs are handed out by ROW: kDefendWaves
// wavefronts per row of the leaf batch, each with a slice of kDefendSlice consecutive cells whose four groups take the next cell of the slice as
// they fall idle.  A wavefront reads its row's threat first and leaves unless it is WIN, so a leaf that is not threatened costs eight wavefronts
// that load one word each; nothing is written for it (the expand kernels do not read its cells, the read-out fills them from the threat's status).
// The position is read once per wavefront.  A leaf with a completing cell of its own is answered WIN by the kernel before the threat's, so
// GMK_VCF_CELL_FIVE cannot arise: follow's init pass has no "over" test.  No float, no atomics, no barrier, nothing allocated.
constexpr int kDefendWaves = 8, kDefendSlice = 29;
static_assert(kDefendWaves * kDefendSlice >= kCells, "the slices cover a row");
__global__ __launch_bounds__(64)
void az_defend_leaves_kernel(AzTree t, AzLeaves lv, AzVcf vc, AzDefend df) {
    namespace V = gmk::vcf;
    enum : int { kSearch = 0, kFollow = 1 };
    __shared__ V::Stack stack;                                   // search mode only
    const V::Lane ln;
    const int y = ln.y;

    // ---- the loader: the same in all 64 lanes ----
    const int slice = static_cast<int>(blockIdx.x % kDefendWaves);
    int game = 0, k = 0;
    size_t out_row = 0;
    if (!leaf_of(t, lv, static_cast<long long>(blockIdx.x) / kDefendWaves, game, k, out_row)) return;
    const int4 th = df.threat[out_row];
    if (th.x != GMK_VCF_WIN || th.w == 0) return;                // only a leaf that was pending and asked has a WIN here
    const LeafRow r = leaf_row(pending_leaf(t, lv, game, k), y);
    const uint32_t base_att = r.white_to_move ? r.black : r.white, base_def = r.white_to_move ? r.white : r.black;
    const int tlen = th.y;
    const uint32_t pvw = reinterpret_cast<const uint32_t*>(df.pv + out_row * GMK_VCF_PV)[y];     // this lane's four pv cells
    uint32_t* out = df.cells + out_row * kCells;
    int next_cell = slice * kDefendSlice;
    int left = next_cell < kCells ? min(kDefendSlice, kCells - next_cell) : 0;

    V::Walk w;
    w.limit = vc.max_depth;
    int mode = kSearch, cell = 0;

    const auto settle = [&](int verdict, bool searched, uint32_t count) {
        if (y == 0) out[cell] = static_cast<uint32_t>(verdict) | (searched ? kCellSearched : 0u) | (count << kCellNodesShift);
        w.state = V::kIdle;
    };
    // P + c, nothing played: where follow starts, and where the search starts after it
    const auto to_root = [&](int new_mode) {
        const int jy = cell / 15;
        mode = new_mode;
        w.reset(base_att, base_def | (y == jy ? 1u << (cell - 15 * jy) : 0u), vc.max_depth);
    };
    // the search's result (K14's finish, without a pv)
    const auto finish = [&](int status) {
        settle(status == GMK_VCF_WIN ? GMK_VCF_CELL_LOSES : status == GMK_VCF_NONE ? GMK_VCF_CELL_HOLDS : GMK_VCF_CELL_UNKNOWN, true, w.nodes);
    };
    const auto failed = [&]() { finish(w.cut ? GMK_VCF_DEPTH : GMK_VCF_NONE); };

    for (;;) {
        // ---- groups without a job take the next cells of this wavefront's slice ----
        const V::HandOut ho = V::hand_out(w.state, ln, left);
        if (w.state == V::kIdle && ho.rank < left) {
            cell = next_cell + ho.rank;
            const int jy = cell / 15;
            const bool taken = V::group_rows(y == jy && (((base_att | base_def) >> (cell - 15 * jy)) & 1u) != 0, ln.gbase) != 0;
            if (taken) settle(GMK_VCF_CELL_NONE, false, 0u);
            else to_root(kFollow);
        }
        left -= ho.taken;
        next_cell += ho.taken;
        if (__ballot(w.state != V::kIdle) == 0ull) {               // nothing to walk: only occupied cells, or the slice is done
            if (left == 0) break;
            continue;
        }

        const V::Pass ps = V::pass(w, ln);
        const V::Follow fo = V::follow_level(w, ln, ps, pvw, tlen);

        // ---- decisions, the same in all sixteen lanes of a group ----
        if (w.state == V::kInit) {
            if (mode == kFollow) {
                if (ps.f1 >= 0) settle(GMK_VCF_CELL_LOSES, false, 0u);
                else if (fo.follows) { w.mask = fo.abit; w.state = V::kRun; }
                else to_root(kSearch);
            } else {
                if (ps.f1 >= 0) finish(GMK_VCF_WIN);               // follow has settled these; kept so that the search is K14's walk whole
                else V::start(w, ps, failed);
            }
        } else if (w.state == V::kRun && mode == kFollow) {
            if (ps.f1 < 0) to_root(kSearch);                       // the threat's move is no four any more
            else if (ps.f2 >= 0) settle(GMK_VCF_CELL_LOSES, false, 0u);
            else if (fo.follows) { ++w.depth; w.mask = fo.abit; }  // a and its forced reply stay on the board
            else to_root(kSearch);
        } else if (w.state == V::kRun) {
            V::step(w, ln, ps, vc.budget, stack, [&](int, int, int) { finish(GMK_VCF_WIN); }, [&]() { finish(GMK_VCF_BUDGET); }, failed);
        }
    }
}

__global__ void az_add_playouts_kernel(AzTree t, uint32_t playouts) {
    const int game = blockIdx.x * blockDim.x + threadIdx.x;
    if (game >= t.n_games) return;
    if (!(t.hdr[game].status & kStatusOver)) t.hdr[game].quota += playouts;
}

__global__ void az_playouts_owed_kernel(AzTree t, int32_t* owed) {
    const int game = blockIdx.x * blockDim.x + threadIdx.x;
    if (game >= t.n_games) return;
    const uint32_t quota = t.hdr[game].quota;
    if (quota != 0u && !(t.hdr[game].status & kStatusOver)) atomicMax(owed, static_cast<int32_t>(min(quota, 0x7FFFFFFFu)));
}

// MCTS::stepForward() / stepForward(move) (MCTS.cpp:129-147): the chosen child's subtree becomes the tree, copied level by
// level into the other arena (root at 0, children consecutive); a move without a child starts a new node.  The move is
// played on the root position.  One wavefront per game.
struct AzArena { uint2* stat; uint2* kids; float* prior; uint32_t* parent; };
// Continuous batching (gmk_az_set_slots): the handle's games are SLOTS that play n_total games between them; slot g plays game slot_game[g]
// (-1: none left), its record goes to that game's rows, and when the game ends the slot takes the next game nobody has started.
struct AzSlots {
    int32_t* slot_game;              // [n_slots], null: slot g plays game g and is not refilled
    int32_t* next_game;              // [1]
    int n_total;
    const uint8_t* open_moves;       // [n_total][open_stride] the moves that lead to a game's first root (black first), may be null
    const int32_t* open_lens;        // [n_total]
    int open_stride;
};

// The subtree of node `src` of arena t becomes the tree of arena b: root at 0, children consecutive, level by level.  All 64 lanes of the
// game's workgroup call it.
__device__ void az_keep_subtree(const AzTree& t, const AzArena& b, size_t base, uint32_t src, int lane, AzHeader& hdr) {
    if (lane == 0) { b.stat[base] = t.stat[base + src]; b.kids[base] = t.kids[base + src]; b.prior[base] = t.prior[base + src]; b.parent[base] = kNoNode; }
    __syncthreads();
    uint32_t next = 1;
    for (uint32_t i0 = 0, chunk = 0; i0 < next; i0 += chunk) {
        chunk = min(64u, next - i0);                            // nodes appended while this chunk is handled come after it
        const uint2 old = static_cast<uint32_t>(lane) < chunk ? b.kids[base + i0 + lane] : make_uint2(0u, 0u);
        unsigned long long todo = __ballot((old.y & 0xFFu) != 0u);
        while (todo) {
            const int j = __ffsll(static_cast<long long>(todo)) - 1;
            todo &= todo - 1ull;
            const uint32_t of = __shfl(old.x, j), oy = __shfl(old.y, j), nk = oy & 0xFFu, node = i0 + static_cast<uint32_t>(j);
            for (uint32_t k = lane; k < nk; k += 64) {
                b.stat[base + next + k] = t.stat[base + of + k];
                b.kids[base + next + k] = t.kids[base + of + k];       // still the OLD child range: rewritten when the scan gets there
                b.prior[base + next + k] = t.prior[base + of + k];
                b.parent[base + next + k] = node;
            }
            if (lane == 0) b.kids[base + node] = make_uint2(next, oy);
            next += nk;
            __syncthreads();
        }
        __syncthreads();
    }
    if (lane == 0) hdr.n_nodes = next;
}

// kProof (here, in az_advance_kernel and in az_root_choice_kernel): where the kernel chooses, proof_choice has the last word
template <bool kProof>
__global__ __launch_bounds__(64)
void az_step_kernel(AzTree t, AzArena b, const int16_t* forced) {
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    AzHeader& hdr = t.hdr[game];
    const size_t base = static_cast<size_t>(game) * t.cap;
    const uint2 rk = t.kids[base];
    const uint32_t first = rk.x, n = rk.y & 0xFFu;
    const int want = forced ? forced[game] : -1;
    uint32_t best_i;
    if (want >= 0) {
        best_i = child_of_cell(t.kids + base, first, n, static_cast<uint32_t>(want), lane);
    } else {
        best_i = most_visited_child<kProof>(t.kids + base, t.stat + base, first, n, lane);
        if (best_i == 0xFFFFFFFFu && n != 0u) best_i = 0u;       // no child has a visit: max_element's first, the first child
    }
    const bool found = best_i != 0xFFFFFFFFu;
    const uint32_t stones = hdr.stones;
    const uint32_t cell = found ? (t.kids[base + first + best_i].y >> 8) & 0xFFu : static_cast<uint32_t>(want);
    const uint32_t row = cell < 225u ? hdr.rows[cell / 15] >> (cell % 15) : 0x10001u;
    const bool legal = (want >= 0 || found) && cell < 225u && !(row & 0x10001u);
    if (!legal) {                                               // nothing to play (childless root) or not a move of this game: the tree is carried over as it is
        if (want >= 0 && lane == 0) hdr.status |= 4u;
    } else if (lane == 0) {
        hdr.rows[cell / 15] |= 1u << (cell % 15 + ((stones & 1u) ? 16 : 0));
        hdr.stones = stones + 1;
        hdr.last_move2 = hdr.last_move;
        hdr.last_move = cell;
        hdr.leaf_pending = 0;
    }
    const uint32_t src = !legal ? 0u : (found ? first + best_i : kNoNode);
    if (src == kNoNode) {                                       // stepForward(move) without such a child: a new node (MCTS.cpp:140-145)
        if (lane == 0) { new_root(b, base, cell << 8); hdr.n_nodes = 1; }
        return;
    }
    az_keep_subtree(t, b, base, src, lane, hdr);
}

// One self-play move for every game that is still played, on the device (what selfplay.play_network_games did with numpy boards, a
// root_stats copy down and a move list up every ply): the most visited child of the root -- first maximum in child order, i.e. ascending
// cells, as MCTS::stepForward()'s max_element (MCTS.cpp:129-134) -- goes into the game's record with the root's visit counts
// (MCTSAgent.eval_state's pi is made from them), Board::applyMove with its victory check (Game.cpp:37-49, 88-136) decides whether the
// game goes on, and the tree is re-rooted: the child's subtree into the other arena (reuse) or a new root.  A root without a visited
// child ends the game where it stands.  Finished games leave a childless root behind in both arenas, so that no kernel ever walks a
// stale tree.  One wavefront per game.
// Sample: nothing, or one AzSample (K20): the plies before its S are drawn by sampled_child, and nothing else changes.  Or one AzGumbel (K21): the
// move is the Gumbel rule's, the row written is the improved-policy row, and the slot's ready word is cleared.
template <bool kProof, class... Sample>
__global__ __launch_bounds__(64)
void az_advance_kernel(AzTree t, AzArena b, uint8_t* __restrict__ rec_moves, uint16_t* __restrict__ rec_visits, int32_t* __restrict__ rec_lens,
                       int8_t* __restrict__ rec_winner, int32_t* __restrict__ unfinished, int reuse, AzSlots sl, Sample... sm) {
    __shared__ uint32_t s_rows[16];
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= t.n_games) return;
    AzHeader& hdr = t.hdr[slot];
    const size_t base = static_cast<size_t>(slot) * t.cap;
    const int game = sl.slot_game ? sl.slot_game[slot] : slot;      // the rows of the records
    GumbelLds* gl = nullptr;
    uint32_t was_ready = 0u;
    if constexpr (kIsGumbel<Sample...>) {
        __shared__ GumbelLds s_g;
        gl = &s_g;
        was_ready = (sm.ready[slot], ...);
        __syncthreads();                                         // every lane has read the word
        if (lane == 0) ((sm.ready[slot] = 0u), ...);
    }
    if ((hdr.status & kStatusOver) || game < 0) {
        if (reuse && lane == 0) new_root(b, base, 0u);
        return;
    }
    const uint2 rk = t.kids[base];
    const uint32_t first = rk.x, n = rk.y & 0xFFu;
    uint32_t best_i;
    if constexpr (kIsGumbel<Sample...>) best_i = gumbel_child(*gl, t, base, first, n, lane, hdr.stones, slot, sm..., was_ready);
    else best_i = root_child<kProof>(t.kids + base, t.stat + base, first, n, lane, hdr, slot, sm...);
    const uint32_t stones = hdr.stones;
    const int len = rec_lens[game];
    bool over = best_i == 0xFFFFFFFFu || stones >= 225u || len >= 225;                 // nothing the search wants to play
    int winner = 0;
    uint32_t cell = 255u;
    if (!over) {
        cell = (t.kids[base + first + best_i].y >> 8) & 0xFFu;
        if constexpr (kIsGumbel<Sample...>) {
            if (rec_visits) gumbel_row(*gl, sm..., __uint_as_float(t.stat[base].y), rec_visits + (static_cast<size_t>(game) * kCells + static_cast<size_t>(len)) * kCells, lane);
        } else {
            if (rec_visits) visits_by_cell(rec_visits + (static_cast<size_t>(game) * kCells + static_cast<size_t>(len)) * kCells, t.kids + base, t.stat + base, first, n, lane);
        }
        const int shift = (stones & 1u) ? 16 : 0;                // black moves on even stone counts
        if (lane < 16) s_rows[lane] = hdr.rows[lane] | ((lane == static_cast<int>(cell / 15u)) ? 1u << (cell % 15u + shift) : 0u);
        __syncthreads();
        const bool five = five_through<1>(s_rows, static_cast<int>(cell % 15u), static_cast<int>(cell / 15u), shift);
        if (lane == 0) {
            hdr.rows[cell / 15u] = s_rows[cell / 15u];
            hdr.stones = stones + 1u;
            hdr.last_move2 = hdr.last_move;
            hdr.last_move = cell;
            hdr.leaf_pending = 0;
            rec_moves[static_cast<size_t>(game) * kCells + len] = static_cast<uint8_t>(cell);
            rec_lens[game] = len + 1;
        }
        winner = five ? (shift ? -1 : 1) : 0;
        over = five || len + 1 == 225;
    }
    if (over) {
        if (lane == 0) {
            rec_winner[game] = static_cast<int8_t>(winner);
            const int next = sl.slot_game ? atomicAdd(sl.next_game, 1) : 0x7FFFFFFF;
            uint32_t root_cell = 0u;
            if (next < sl.n_total) {                            // the slot goes on with the next unstarted game: its opening is the root position
                const int n_open = sl.open_moves ? sl.open_lens[next] : 0;
                for (int y = 0; y < 16; ++y) hdr.rows[y] = 0u;
                uint32_t last = 255u, last2 = 255u;
                for (int i = 0; i < n_open; ++i) {
                    const uint32_t c = sl.open_moves[static_cast<size_t>(next) * sl.open_stride + i];
                    hdr.rows[c / 15u] |= 1u << (c % 15u + ((i & 1) ? 16 : 0));
                    last2 = last;
                    last = c;
                }
                hdr.stones = static_cast<uint32_t>(n_open);
                hdr.last_move = last;
                hdr.last_move2 = last2;
                sl.slot_game[slot] = next;
                root_cell = (last & 0xFFu) << 8;                // as az_init_roots_kernel
                atomicAdd(unfinished, 1);
            } else {
                if (sl.slot_game) sl.slot_game[slot] = -1;
                hdr.status |= kStatusOver;
            }
            hdr.leaf_pending = 0;
            hdr.quota = 0;                                       // a refilled slot owes nothing until the next gmk_az_add_playouts
            hdr.n_nodes = 1;
            new_root(t, base, root_cell);
            if (reuse) new_root(b, base, root_cell);
        }
        return;
    }
    if (lane == 0) atomicAdd(unfinished, 1);
    if (reuse) {
        az_keep_subtree(t, b, base, first + best_i, lane, hdr);
    } else if (lane == 0) {                                      // a new root, as gmk_az_set_roots makes it
        new_root(t, base, cell << 8);
        hdr.n_nodes = 1;
    }
}

// The leaf batch holds the games that are still played, and nothing else: row_of[g] = the number of live games before g.  The network's
// work per playout then follows the number of live games instead of the number of slots (the end of a batch of games is long: lengths
// run from 9 to 225 plies).  One workgroup.
__global__ __launch_bounds__(1024)
void az_compact_kernel(const AzHeader* __restrict__ hdr, int n_games, int32_t* __restrict__ row_of, int32_t* __restrict__ n_live) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int g0 = 0; g0 < n_games; g0 += 1024) {
        const int g = g0 + tid;
        const bool live = g < n_games && !(hdr[g].status & kStatusOver);
        const unsigned long long b = __ballot(live);
        const int before = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u)));
        if ((tid & 63) == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int waves_before = 0, total = 0;
        for (int w = 0; w < 16; ++w) { if (w < wave) waves_before += s_wave[w]; total += s_wave[w]; }
        if (g < n_games) row_of[g] = live ? s_base + waves_before + before : -1;
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
    if (tid == 0) *n_live = s_base;
}

// Default::AddNoise (MonteCarlo.hpp:97-108): the root children's priors, by cell, as the host computed them
__global__ __launch_bounds__(64)
void az_set_root_priors_kernel(AzTree t, const float* priors) {
    const int game = blockIdx.x, lane = threadIdx.x;
    const size_t base = static_cast<size_t>(game) * t.cap;
    const uint2 rk = t.kids[base];
    for (uint32_t i = lane; i < (rk.y & 0xFFu); i += 64)
        t.prior[base + rk.x + i] = priors[static_cast<size_t>(game) * kCells + ((t.kids[base + rk.x + i].y >> 8) & 0xFFu)];
}

// Default::AddNoise with the counter-based sampler (include/gomoku_noise.h), one wavefront per game, on the device: the root children's priors travel
// through 225 words of LDS into by-cell order, lane l mixes the cells l + 64 j (noise_device.h), and back.  The stream belongs to the GAME a slot
// plays (slot_game under continuous batching, game_ids otherwise) and to the stones on its root board.
__global__ __launch_bounds__(64)
void az_root_noise_kernel(AzTree t, const int32_t* __restrict__ slot_game, const uint32_t* __restrict__ game_ids, uint32_t first_game_id,
                          float alpha, float epsilon, uint32_t seed_lo, uint32_t seed_hi) {
    __shared__ uint32_t s_cells[kCells];
    const int game = blockIdx.x, lane = threadIdx.x;
    const AzHeader& hdr = t.hdr[game];
    if (hdr.status & kStatusOver) return;
    const size_t base = static_cast<size_t>(game) * t.cap;
    const uint2 rk = t.kids[base];
    const uint32_t first = rk.x, n = rk.y & 0xFFu;
    if (n == 0u) return;                                         // a root without children takes no noise (the loop over node->children is empty)
    const uint32_t gid = first_game_id + (slot_game ? static_cast<uint32_t>(max(slot_game[game], 0)) : game_ids[game]);
    for (int i = lane; i < kCells; i += 64) s_cells[i] = 0u;
    __syncthreads();
    uint32_t cell[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = lane + 64 * k;
        cell[k] = i < n ? (t.kids[base + first + i].y >> 8) & 0xFFu : 0u;
        if (i < n) s_cells[cell[k]] = __float_as_uint(t.prior[base + first + i]);
    }
    __syncthreads();
    float p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = lane + 64 * j < kCells ? __uint_as_float(s_cells[lane + 64 * j]) : 0.0f;
    gmk::noise::mix_root_priors(p, lane, alpha, epsilon, gid, hdr.stones, seed_lo, seed_hi);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) if (lane + 64 * j < kCells) s_cells[lane + 64 * j] = __float_as_uint(p[j]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = lane + 64 * k;
        if (i < n) t.prior[base + first + i] = __uint_as_float(s_cells[cell[k]]);
    }
}

// The cell MCTS::stepForward() would play for every game, left ON THE DEVICE for the match referee (match_kernel.hip): the most visited root
// child, first maximum in child (= cell) order, exactly az_advance_kernel's choice; -1 for a root without a visited child.  visits (may be
// null): the root children's visit counts by cell, saturated like the records' rows.  One wavefront per game.
// Sample: nothing, or one AzSample (K20): az_advance_kernel's sampled choice.  Or one AzGumbel (K21): its Gumbel choice, `visits` gets the
// improved-policy row (zeros for a root without children), and the game's ready word is cleared.
template <bool kProof, class... Sample>
__global__ __launch_bounds__(64)
void az_root_choice_kernel(AzTree t, int16_t* __restrict__ cells, uint16_t* __restrict__ visits, Sample... sm) {
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    const size_t base = static_cast<size_t>(game) * t.cap;
    const uint2 rk = t.kids[base];
    const uint32_t first = rk.x, n = rk.y & 0xFFu;
    if constexpr (kIsGumbel<Sample...>) {
        __shared__ GumbelLds s_g;
        const uint32_t was_ready = (sm.ready[game], ...);
        __syncthreads();                                         // every lane has read the word
        if (lane == 0) ((sm.ready[game] = 0u), ...);
        const uint32_t best_i = gumbel_child(s_g, t, base, first, n, lane, t.hdr[game].stones, game, sm..., was_ready);
        if (lane == 0) cells[game] = best_i == 0xFFFFFFFFu ? static_cast<int16_t>(-1) : static_cast<int16_t>((t.kids[base + first + best_i].y >> 8) & 0xFFu);
        if (visits) {
            if (n != 0u) gumbel_row(s_g, sm..., __uint_as_float(t.stat[base].y), visits + static_cast<size_t>(game) * kCells, lane);
            else for (int i = lane; i < kCells; i += 64) visits[static_cast<size_t>(game) * kCells + i] = 0;
        }
    } else {
        const uint32_t best_i = root_child<kProof>(t.kids + base, t.stat + base, first, n, lane, t.hdr[game], game, sm...);
        if (lane == 0) cells[game] = best_i == 0xFFFFFFFFu ? static_cast<int16_t>(-1) : static_cast<int16_t>((t.kids[base + first + best_i].y >> 8) & 0xFFu);
        if (visits) visits_by_cell(visits + static_cast<size_t>(game) * kCells, t.kids + base, t.stat + base, first, n, lane);
    }
}

// gmk_az_step with the cells and the referee's verdicts (GMK_MATCH_*) read from device memory.  A game that moved follows the move -- the
// child's subtree into the other arena (fresh == 0, as az_step_kernel) or a new root in place (fresh != 0, what gmk_az_set_roots makes for
// the position after the move); a game that ended on this ply is closed as az_advance_kernel closes one (status bit 0, a childless root in
// both arenas); a game that did not move or was over before keeps its tree (copied over as it is when the arenas flip: a closed game's
// childless root is in both already).  One wavefront per game.
__global__ __launch_bounds__(64)
void az_step_device_kernel(AzTree t, AzArena b, const int16_t* __restrict__ cells, const int32_t* __restrict__ verdict, int fresh) {
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    AzHeader& hdr = t.hdr[game];
    const size_t base = static_cast<size_t>(game) * t.cap;
    const int v = verdict[game];
    if (hdr.status & kStatusOver) return;                        // closed on an earlier ply
    const uint32_t cell = static_cast<uint32_t>(static_cast<int>(cells[game]));
    const uint32_t stones = hdr.stones;
    bool moved = v == GMK_MATCH_MOVED || v == GMK_MATCH_ENDED;
    if (moved) {                                                 // the referee judged the RECORD; the handle's own position must agree
        const uint32_t row = cell < 225u ? hdr.rows[cell / 15u] >> (cell % 15u) : 0x10001u;
        if (row & 0x10001u) { moved = false; if (lane == 0) hdr.status |= 4u; }
    }
    if (!moved) {
        if (!fresh) az_keep_subtree(t, b, base, 0u, lane, hdr);
        return;
    }
    const uint2 rk = t.kids[base];
    uint32_t best_i = 0xFFFFFFFFu;                               // the child of that cell
    if (!fresh && v == GMK_MATCH_MOVED) best_i = child_of_cell(t.kids + base, rk.x, rk.y & 0xFFu, cell, lane);
    __syncthreads();                                             // every lane has read the old header
    if (lane == 0) {
        hdr.rows[cell / 15u] |= 1u << (cell % 15u + ((stones & 1u) ? 16 : 0));
        hdr.stones = stones + 1u;
        hdr.last_move2 = hdr.last_move;
        hdr.last_move = cell;
        hdr.leaf_pending = 0;
    }
    if (v == GMK_MATCH_ENDED) {
        if (lane == 0) {
            hdr.status |= kStatusOver;
            hdr.quota = 0;
            hdr.n_nodes = 1;
            new_root(t, base, 0u);
            if (!fresh) new_root(b, base, 0u);
        }
        return;
    }
    if (fresh) {                                                 // a new root, as az_init_roots_kernel makes it
        if (lane == 0) { new_root(t, base, cell << 8); hdr.n_nodes = 1; }
        return;
    }
    if (best_i == 0xFFFFFFFFu) {                                 // stepForward(move) without such a child: a new node (MCTS.cpp:140-145)
        if (lane == 0) { new_root(b, base, cell << 8); hdr.n_nodes = 1; }
        return;
    }
    az_keep_subtree(t, b, base, rk.x + best_i, lane, hdr);
}

__global__ void az_init_roots_kernel(AzTree t) {
    const int game = blockIdx.x * blockDim.x + threadIdx.x;
    if (game >= t.n_games) return;
    new_root(t, static_cast<size_t>(game) * t.cap, (t.hdr[game].last_move & 0xFFu) << 8);
}

__global__ __launch_bounds__(64)
void az_root_stats_kernel(AzTree t, uint32_t* visits, float* values, float* priors, uint32_t* root_visits, float* root_value) {
    const int game = blockIdx.x, lane = threadIdx.x;
    const size_t arena = static_cast<size_t>(game) * t.cap;
    const uint2 k = t.kids[arena];
    for (uint32_t i = lane; i < (k.y & 0xFFu); i += 64) {
        const uint32_t child = k.x + i, cell = (t.kids[arena + child].y >> 8) & 0xFFu;
        const uint2 cs = t.stat[arena + child];
        if (visits) visits[static_cast<size_t>(game) * kCells + cell] = cs.x;
        if (values) values[static_cast<size_t>(game) * kCells + cell] = __uint_as_float(cs.y);
        if (priors) priors[static_cast<size_t>(game) * kCells + cell] = t.prior[arena + child];
    }
    if (lane == 0) {
        if (root_visits) root_visits[game] = t.stat[arena].x;
        if (root_value) root_value[game] = __uint_as_float(t.stat[arena].y);
    }
}

// K7 + proofs: the root's proof and its children's by cell (0 where there is no child)
__global__ __launch_bounds__(64)
void az_root_proofs_kernel(AzTree t, int8_t* __restrict__ root, int8_t* __restrict__ children) {
    const int game = blockIdx.x, lane = threadIdx.x;
    if (game >= t.n_games) return;
    const size_t arena = static_cast<size_t>(game) * t.cap;
    const uint2 k = t.kids[arena];
    int8_t* out = children + static_cast<size_t>(game) * kCells;
    for (int i = lane; i < kCells; i += 64) out[i] = 0;
    __syncthreads();
    for (uint32_t i = lane; i < (k.y & 0xFFu); i += 64) {
        const uint32_t ky = t.kids[arena + k.x + i].y;
        out[(ky >> 8) & 0xFFu] = static_cast<int8_t>(proof_of(ky));
    }
    if (lane == 0) root[game] = static_cast<int8_t>(proof_of(k.y));
}

}  // namespace

struct gmk_az {
    AzTree t{};
    bool rooted = false;
    AzArena other{};                                             // second arena, allocated by the first gmk_az_step
    int16_t* d_forced = nullptr;
    float* d_noise_priors = nullptr;
    int32_t* d_unfinished = nullptr;                             // gmk_az_advance's counter
    int32_t* d_row_of = nullptr;                                 // [n_games] + the number of live games (AzTree::row_of)
    int n_live = 0;
    AzSlots slots{};                                             // gmk_az_set_slots (device memory owned by the handle)
    uint8_t* d_open_moves = nullptr;
    int32_t* d_open_lens = nullptr;
    std::vector<uint32_t> game_ids;                              // the game a slot is playing, relative to the callers' first_game_id (default: the slot number)
    bool second_arena = false;
    int noise_sampler = GMK_NOISE_SAMPLER_STD;                   // gmk_az_set_option
    uint32_t* d_game_ids = nullptr;                              // the device copy of game_ids for az_root_noise_kernel
    AzLeaves lv{nullptr, nullptr, 1};                            // GMK_OPT_AZ_LEAVES; the side buffers come with the first L > 1
    int32_t* d_owed = nullptr;                                   // gmk_az_playouts_owed's word
    bool select_issued = false;                                  // L > 1: gmk_az_select has marked its leaves, gmk_az_expand has not answered yet
    bool leaf_waiting = false;                                   // any L: a gmk_az_select has not been answered yet (asked by the GMK_OPT_AZ_VCF_* options only)
    AzVcf vcf{nullptr, 0, 64u};                                  // GMK_OPT_AZ_VCF_DEPTH / _BUDGET; the verdict buffer comes with the first D > 0
    bool proof = false;                                          // GMK_OPT_AZ_PROOF: the <true> proof instantiations are launched
    bool defend = false;                                         // GMK_OPT_AZ_VCF_DEFEND; it acts only with D > 0 and proof (az_defend_active)
    AzDefend df{};                                               //   its buffers come when it first acts
    bool gumbel = false;                                         // K21: gmk_az_set_gumbel with max_considered > 0
    AzGumbel gm{};                                               //   its parameters; st and ready come with the first use
    // device scratch of the host-driven form (gmk_az_select_host / gmk_az_expand_host)
    float *h_states = nullptr, *h_values = nullptr, *h_probs = nullptr;
    int16_t* h_paths = nullptr;
    int32_t* h_lens = nullptr;
};

extern "C" int gmk_az_destroy(gmk_az* a) {
    if (!a) return GMK_OK;
    (void)gmk::device_free(a->t.hdr); (void)gmk::device_free(a->t.stat); (void)gmk::device_free(a->t.kids); (void)gmk::device_free(a->t.prior); (void)gmk::device_free(a->t.parent);
    (void)gmk::device_free(a->other.stat); (void)gmk::device_free(a->other.kids); (void)gmk::device_free(a->other.prior); (void)gmk::device_free(a->other.parent);
    (void)gmk::device_free(a->d_forced); (void)gmk::device_free(a->d_game_ids); (void)gmk::device_free(a->d_noise_priors); (void)gmk::device_free(a->d_unfinished); (void)gmk::device_free(a->d_row_of);
    (void)gmk::device_free(a->slots.slot_game); (void)gmk::device_free(a->d_open_moves); (void)gmk::device_free(a->d_open_lens);
    (void)gmk::device_free(a->h_states); (void)gmk::device_free(a->h_values); (void)gmk::device_free(a->h_probs); (void)gmk::device_free(a->h_paths); (void)gmk::device_free(a->h_lens);
    (void)gmk::device_free(a->lv.inflight); (void)gmk::device_free(a->lv.pend); (void)gmk::device_free(a->d_owed);
    (void)gmk::device_free(a->vcf.verdict);
    (void)gmk::device_free(a->gm.st); (void)gmk::device_free(a->gm.ready);
    (void)gmk::device_free(a->df.threat); (void)gmk::device_free(a->df.pv); (void)gmk::device_free(a->df.occupied); (void)gmk::device_free(a->df.cells);
    delete a;
    return GMK_OK;
}

extern "C" int gmk_az_create(int n_games, int node_capacity, double c_puct, gmk_az** out) {
    GMK_NEED_INIT();
    if (!out || n_games <= 0 || node_capacity < 256) { gmk::set_error("gmk_az_create: bad arguments"); return GMK_ERR_ARG; }
    gmk_az* a = new gmk_az;
    a->t.n_games = n_games; a->t.cap = node_capacity; a->t.c_puct = c_puct;
    const size_t nodes = static_cast<size_t>(n_games) * node_capacity;
    const bool ok = gmk::device_malloc(&a->t.hdr, static_cast<size_t>(n_games) * sizeof(AzHeader)) == hipSuccess &&
                    gmk::device_malloc(&a->t.stat, nodes * 8) == hipSuccess && gmk::device_malloc(&a->t.kids, nodes * 8) == hipSuccess &&
                    gmk::device_malloc(&a->t.prior, nodes * 4) == hipSuccess && gmk::device_malloc(&a->t.parent, nodes * 4) == hipSuccess;
    if (!ok || gmk::device_malloc(&a->d_row_of, (static_cast<size_t>(n_games) + 1) * 4) != hipSuccess) { gmk_az_destroy(a); gmk::set_error("gmk_az_create: device allocation failed"); return GMK_ERR_HIP; }
    a->t.row_of = a->d_row_of;
    a->game_ids.resize(static_cast<size_t>(n_games));
    for (int g = 0; g < n_games; ++g) a->game_ids[static_cast<size_t>(g)] = static_cast<uint32_t>(g);
    if (gmk::device_malloc(&a->d_game_ids, static_cast<size_t>(n_games) * 4) != hipSuccess ||
        hipMemcpy(a->d_game_ids, a->game_ids.data(), static_cast<size_t>(n_games) * 4, hipMemcpyHostToDevice) != hipSuccess) {
        gmk_az_destroy(a); gmk::set_error("gmk_az_create: device allocation failed"); return GMK_ERR_HIP;
    }
    *out = a;
    return GMK_OK;
}

// d_game_ids mirrors game_ids, so that gmk_az_add_root_noise's kernel needs nothing from the host: after every change of game_ids, once the
// device is idle (a noise kernel may still be reading the old ones on a stream of the caller's)
static int az_upload_game_ids(gmk_az* a) {
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(a->d_game_ids, a->game_ids.data(), a->game_ids.size() * 4, hipMemcpyHostToDevice));
    return GMK_OK;
}

// row_of and the number of live games, after anything that changes which games are played
static int az_compact(gmk_az* a, hipStream_t s) {
    hipLaunchKernelGGL(az_compact_kernel, dim3(1), dim3(1024), 0, s, a->t.hdr, a->t.n_games, a->d_row_of, a->d_row_of + a->t.n_games);
    GMK_HIP_CHECK(hipGetLastError());
    int32_t n = 0;
    GMK_HIP_CHECK(hipMemcpyAsync(&n, a->d_row_of + a->t.n_games, 4, hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    a->n_live = n;
    return GMK_OK;
}

// L > 1 and a select is waiting for its expand: the in-flight marks are up, so nothing may move the trees or change how they are read
static bool az_marks_up(const gmk_az* a, const char* who) {
    if (a->lv.leaves > 1 && a->select_issued) { gmk::set_error("%s: gmk_az_select is waiting for its gmk_az_expand (GMK_OPT_AZ_LEAVES = %d)", who, a->lv.leaves); return true; }
    return false;
}
// the host-driven entries serve one leaf per game, evaluated by the host alone
static bool az_many_leaves(const gmk_az* a, const char* who) {
    if (a->vcf.max_depth > 0) { gmk::set_error("%s: the host-driven form does not solve its leaves (GMK_OPT_AZ_VCF_DEPTH = %d)", who, a->vcf.max_depth); return true; }
    if (a->proof) { gmk::set_error("%s: the host-driven form does not carry proofs (GMK_OPT_AZ_PROOF = 1)", who); return true; }
    if (a->defend) { gmk::set_error("%s: the host-driven form does not ask the defence solver (GMK_OPT_AZ_VCF_DEFEND = 1)", who); return true; }
    if (a->lv.leaves > 1) { gmk::set_error("%s: the host-driven form takes one leaf per step (GMK_OPT_AZ_LEAVES = %d)", who, a->lv.leaves); return true; }
    return false;
}
// new roots: no leaf is pending and nothing is in flight (the headers are rewritten by the caller: quota 0, n_pending 0)
static int az_reset_leaves(gmk_az* a) {
    a->select_issued = false;
    a->leaf_waiting = false;
    if (a->lv.inflight) GMK_HIP_CHECK(hipMemset(a->lv.inflight, 0, static_cast<size_t>(a->t.n_games) * static_cast<size_t>(a->t.cap) * 2));
    return GMK_OK;
}

// K21: the roots have moved or been replaced, so every set-up is void: a clear of the ready words behind the caller's launches, on their stream.
// With Gumbel off nothing is issued.
static int az_gumbel_clear(gmk_az* a, hipStream_t s) {
    if (!a->gumbel) return GMK_OK;
    GMK_HIP_CHECK(hipMemsetAsync(a->gm.ready, 0, static_cast<size_t>(a->t.n_games) * 4, s));
    return GMK_OK;
}
// the kernels' AzGumbel: the handle's parameters and the games its slots play now
static AzGumbel az_gumbel_args(const gmk_az* a) {
    AzGumbel g = a->gm;
    g.slot_game = a->slots.slot_game;
    g.game_ids = a->d_game_ids;
    return g;
}

extern "C" int gmk_az_live_games(gmk_az* a, int32_t* n_live) {
    if (!a || !n_live) { gmk::set_error("gmk_az_live_games: bad arguments"); return GMK_ERR_ARG; }
    *n_live = a->n_live;
    return GMK_OK;
}

extern "C" int gmk_az_set_game_ids(gmk_az* a, const uint32_t* h_ids) {
    if (!a || !h_ids) { gmk::set_error("gmk_az_set_game_ids: bad arguments"); return GMK_ERR_ARG; }
    a->game_ids.assign(h_ids, h_ids + a->t.n_games);
    return az_upload_game_ids(a);
}

extern "C" int gmk_az_set_roots(gmk_az* a, const uint16_t* h_planes, const int16_t* h_last_moves) {
    if (!a || !h_planes || !h_last_moves) { gmk::set_error("gmk_az_set_roots: bad arguments"); return GMK_ERR_ARG; }
    std::vector<AzHeader> hdr(a->t.n_games);
    for (int g = 0; g < a->t.n_games; ++g) {
        AzHeader& h = hdr[g];
        std::memset(&h, 0, sizeof h);
        const uint16_t* p = h_planes + static_cast<size_t>(g) * 32;
        int stones = 0;
        for (int y = 0; y < 15; ++y) {
            if ((p[y] & p[16 + y]) || ((p[y] | p[16 + y]) & 0x8000u)) { gmk::set_error("gmk_az_set_roots: game %d has an invalid position", g); return GMK_ERR_ARG; }
            h.rows[y] = static_cast<uint32_t>(p[y]) | (static_cast<uint32_t>(p[16 + y]) << 16);
            stones += __builtin_popcount(h.rows[y]);
        }
        h.n_nodes = 1;
        h.stones = static_cast<uint32_t>(stones);
        const int16_t l1 = h_last_moves[2 * g], l2 = h_last_moves[2 * g + 1];
        h.last_move = l1 >= 0 && l1 < 225 ? static_cast<uint32_t>(l1) : 255u;
        h.last_move2 = l2 >= 0 && l2 < 225 ? static_cast<uint32_t>(l2) : 255u;
    }
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(a->t.hdr, hdr.data(), hdr.size() * sizeof(AzHeader), hipMemcpyHostToDevice));
    if (const int rc = az_reset_leaves(a); rc != GMK_OK) return rc;
    hipLaunchKernelGGL(az_init_roots_kernel, dim3((a->t.n_games + 255) / 256), dim3(256), 0, nullptr, a->t);
    GMK_HIP_CHECK(hipGetLastError());
    if (const int rc = az_gumbel_clear(a, nullptr); rc != GMK_OK) return rc;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    a->rooted = true;
    if (const int rc = az_compact(a, nullptr); rc != GMK_OK) return rc;
    (void)gmk::device_free(a->slots.slot_game); (void)gmk::device_free(a->d_open_moves); (void)gmk::device_free(a->d_open_lens);       // slot g plays game g again
    a->slots = AzSlots{}; a->d_open_moves = nullptr; a->d_open_lens = nullptr;
    return GMK_OK;
}

// Continuous batching for whole-game self-play: the handle's n_games slots play n_total games between them.  The first min(n_games,
// n_total) games start in the slots, from their openings (this call makes the roots: it takes gmk_az_set_roots's place); gmk_az_advance
// then writes a slot's move into the record rows of the GAME it plays and hands a finished game's slot to the next unstarted game.
extern "C" int gmk_az_set_slots(gmk_az* a, int n_total, const uint8_t* h_open_moves, int open_stride, const int32_t* h_open_lens) {
    if (!a || n_total <= 0 || (h_open_moves && (!h_open_lens || open_stride <= 0))) { gmk::set_error("gmk_az_set_slots: bad arguments"); return GMK_ERR_ARG; }
    const int n_slots = a->t.n_games, started = std::min(n_slots, n_total);
    const size_t ns = static_cast<size_t>(n_slots), nt = static_cast<size_t>(n_total);
    std::vector<int32_t> open_lens(nt, 0);
    if (h_open_moves)
        for (size_t g = 0; g < nt; ++g) {
            if (h_open_lens[g] < 0 || h_open_lens[g] > 8 || h_open_lens[g] > open_stride) { gmk::set_error("gmk_az_set_slots: opening of game %zu has %d moves (at most 8: an opening cannot be a finished game)", g, h_open_lens[g]); return GMK_ERR_ARG; }
            open_lens[g] = h_open_lens[g];
            uint32_t seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};           // every opening is checked here: the device plays the later ones unseen
            for (int i = 0; i < open_lens[g]; ++i) {
                const uint32_t c = h_open_moves[g * static_cast<size_t>(open_stride) + i];
                if (c >= 225u || ((seen[c >> 5] >> (c & 31u)) & 1u)) { gmk::set_error("gmk_az_set_slots: opening of game %zu is not a sequence of moves", g); return GMK_ERR_ARG; }
                seen[c >> 5] |= 1u << (c & 31u);
            }
        }
    std::vector<AzHeader> hdr(ns);
    std::vector<int32_t> state(ns + 1, -1);
    for (size_t g = 0; g < ns; ++g) {
        AzHeader& h = hdr[g];
        std::memset(&h, 0, sizeof h);
        h.n_nodes = 1;
        h.last_move = h.last_move2 = 255u;
        if (g >= static_cast<size_t>(started)) { h.status = kStatusOver; continue; }
        state[g] = static_cast<int32_t>(g);
        for (int i = 0; i < open_lens[g]; ++i) {
            const uint32_t c = h_open_moves[g * static_cast<size_t>(open_stride) + i];
            if (c >= 225u || ((h.rows[c / 15u] | (h.rows[c / 15u] >> 16)) >> (c % 15u)) & 1u) { gmk::set_error("gmk_az_set_slots: opening of game %zu is not a sequence of moves", g); return GMK_ERR_ARG; }
            h.rows[c / 15u] |= 1u << (c % 15u + ((i & 1) ? 16 : 0));
            h.last_move2 = h.last_move;
            h.last_move = c;
        }
        h.stones = static_cast<uint32_t>(open_lens[g]);
    }
    state[ns] = started;                                         // next_game
    GMK_HIP_CHECK(hipDeviceSynchronize());
    (void)gmk::device_free(a->slots.slot_game); (void)gmk::device_free(a->d_open_moves); (void)gmk::device_free(a->d_open_lens);
    a->slots = AzSlots{}; a->d_open_moves = nullptr; a->d_open_lens = nullptr;
    GMK_HIP_CHECK(gmk::device_malloc(&a->slots.slot_game, state.size() * 4));
    GMK_HIP_CHECK(hipMemcpy(a->slots.slot_game, state.data(), state.size() * 4, hipMemcpyHostToDevice));
    GMK_HIP_CHECK(gmk::device_malloc(&a->d_open_lens, nt * 4));
    GMK_HIP_CHECK(hipMemcpy(a->d_open_lens, open_lens.data(), nt * 4, hipMemcpyHostToDevice));
    if (h_open_moves) {
        GMK_HIP_CHECK(gmk::device_malloc(&a->d_open_moves, nt * static_cast<size_t>(open_stride)));
        GMK_HIP_CHECK(hipMemcpy(a->d_open_moves, h_open_moves, nt * static_cast<size_t>(open_stride), hipMemcpyHostToDevice));
    }
    a->slots.next_game = a->slots.slot_game + ns;
    a->slots.n_total = n_total;
    a->slots.open_moves = a->d_open_moves; a->slots.open_lens = a->d_open_lens; a->slots.open_stride = open_stride;
    GMK_HIP_CHECK(hipMemcpy(a->t.hdr, hdr.data(), hdr.size() * sizeof(AzHeader), hipMemcpyHostToDevice));
    if (const int rc = az_reset_leaves(a); rc != GMK_OK) return rc;
    hipLaunchKernelGGL(az_init_roots_kernel, dim3((a->t.n_games + 255) / 256), dim3(256), 0, nullptr, a->t);
    GMK_HIP_CHECK(hipGetLastError());
    if (const int rc = az_gumbel_clear(a, nullptr); rc != GMK_OK) return rc;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    for (size_t g = 0; g < ns; ++g) a->game_ids[g] = state[g] >= 0 ? static_cast<uint32_t>(state[g]) : 0u;
    if (const int rc = az_upload_game_ids(a); rc != GMK_OK) return rc;
    a->rooted = true;
    return az_compact(a, nullptr);
}

// K7 + K15 acts: the option, the solver and the proofs are all on, and its buffers are there (an option call whose allocation failed has
// said so, and the block stays inert)
static bool az_defend_wanted(const gmk_az* a) { return a->defend && a->proof && a->vcf.max_depth > 0; }
static bool az_defend_active(const gmk_az* a) { return az_defend_wanted(a) && a->df.threat != nullptr; }

// The instantiation of a kernel for the handle's options: f is handed them as std::bool_constants and returns the kernel.  f(kVcf, kProof,
// kDefend) for the expand kernels: proofs start there only at a leaf answered WIN, so without the solver the proof option launches what it
// launches when off.  f(kProof) for the others.
template <class F>
static auto az_expand_variant(const gmk_az* a, F f) {
    if (az_defend_active(a)) return f(std::true_type{}, std::true_type{}, std::true_type{});
    if (a->vcf.max_depth > 0 && a->proof) return f(std::true_type{}, std::true_type{}, std::false_type{});
    if (a->vcf.max_depth > 0) return f(std::true_type{}, std::false_type{}, std::false_type{});
    return f(std::false_type{}, std::false_type{}, std::false_type{});
}
template <class F>
static auto az_proof_variant(const gmk_az* a, F f) {
    return a->proof ? f(std::true_type{}) : f(std::false_type{});
}
// the second arena holds the trees now
static void az_flip_arenas(gmk_az* a) {
    std::swap(a->t.stat, a->other.stat); std::swap(a->t.kids, a->other.kids); std::swap(a->t.prior, a->other.prior); std::swap(a->t.parent, a->other.parent);
}

// The buffers of K7 + K15, when an option call makes it act for the first time: per row of the largest leaf batch the threat (every row reads
// "not asked" until a select writes it), its line, the occupied cells and one word per cell.
static int az_defend_buffers(gmk_az* a) {
    if (!az_defend_wanted(a) || a->df.threat) return GMK_OK;
    const size_t rows = static_cast<size_t>(a->t.n_games) * GMK_AZ_MAX_LEAVES;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    const bool ok = gmk::device_malloc(&a->df.threat, rows * sizeof(int4)) == hipSuccess && gmk::device_malloc(&a->df.pv, rows * GMK_VCF_PV) == hipSuccess &&
                    gmk::device_malloc(&a->df.occupied, rows * 16 * 2) == hipSuccess && gmk::device_malloc(&a->df.cells, rows * kCells * 4) == hipSuccess &&
                    hipMemset(a->df.threat, 0, rows * sizeof(int4)) == hipSuccess && hipMemset(a->df.pv, 0xFF, rows * GMK_VCF_PV) == hipSuccess &&
                    hipMemset(a->df.occupied, 0, rows * 16 * 2) == hipSuccess && hipMemset(a->df.cells, 0, rows * kCells * 4) == hipSuccess;
    if (!ok) {                                                   // all or nothing
        (void)gmk::device_free(a->df.threat); (void)gmk::device_free(a->df.pv); (void)gmk::device_free(a->df.occupied); (void)gmk::device_free(a->df.cells);
        a->df = AzDefend{};
        (void)hipGetLastError();
        gmk::set_error("gmk_az_set_option: hipMalloc of the defence buffers (%zu rows) failed", rows);
        return GMK_ERR_HIP;
    }
    return GMK_OK;
}

// D > 0: the pending leaves go through the solver, on the same stream, right behind the select kernel; with K7 + K15 the threat against each
// and the replies that lose to it follow, as two more links of the same chain
static int az_vcf_leaves(gmk_az* a, void* stream) {
    a->leaf_waiting = true;
    if (a->vcf.max_depth == 0) return GMK_OK;
    const long long groups = static_cast<long long>(a->t.n_games) * a->lv.leaves;
    hipLaunchKernelGGL(az_vcf_leaves_kernel, dim3(static_cast<unsigned>((groups + 3) / 4)), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, a->lv, a->vcf);
    GMK_HIP_CHECK(hipGetLastError());
    if (!az_defend_active(a)) return GMK_OK;
    hipLaunchKernelGGL(az_threat_leaves_kernel, dim3(static_cast<unsigned>((groups + 3) / 4)), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, a->lv, a->vcf, a->df);
    GMK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(az_defend_leaves_kernel, dim3(static_cast<unsigned>(groups * kDefendWaves)), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, a->lv, a->vcf, a->df);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_az_select(gmk_az* a, float* d_states, void* stream) {
    if (!a || !d_states) { gmk::set_error("gmk_az_select: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_select: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (a->lv.leaves > 1) {                                      // d_states has gmk_az_live_games x L rows
        if (az_marks_up(a, "gmk_az_select")) return GMK_ERR_STATE;
        const auto kernel = az_proof_variant(a, [](auto proof) { return &az_select_leaves_kernel<proof>; });
        hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, a->lv, d_states);
        GMK_HIP_CHECK(hipGetLastError());
        a->select_issued = true;
        return az_vcf_leaves(a, stream);
    }
    if (a->gumbel) {                                             // K21 (one leaf, no proofs: gmk_az_set_gumbel and gmk_az_set_option see to it)
        hipLaunchKernelGGL(az_select_gumbel_kernel, dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, d_states, az_gumbel_args(a));
        GMK_HIP_CHECK(hipGetLastError());
        return az_vcf_leaves(a, stream);
    }
    const auto kernel = az_proof_variant(a, [](auto proof) { return &az_select_kernel<proof>; });
    hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, d_states);
    GMK_HIP_CHECK(hipGetLastError());
    return az_vcf_leaves(a, stream);
}

extern "C" int gmk_az_expand(gmk_az* a, const float* d_values, const float* d_probs, void* stream) {
    if (!a || !d_values || !d_probs) { gmk::set_error("gmk_az_expand: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_expand: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (a->lv.leaves > 1) {                                      // d_values and d_probs have gmk_az_live_games x L rows
        const auto kernel = az_expand_variant(a, [](auto vcf, auto proof, auto defend) { return &az_expand_leaves_kernel<vcf, proof, defend>; });
        hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, a->lv, d_values, d_probs, a->vcf, a->df);
        GMK_HIP_CHECK(hipGetLastError());
        a->select_issued = false;
        a->leaf_waiting = false;
        return GMK_OK;
    }
    const auto kernel = az_expand_variant(a, [](auto vcf, auto proof, auto defend) { return &az_expand_kernel<vcf, proof, defend>; });
    hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, d_values, d_probs, 3, a->vcf, a->df);
    GMK_HIP_CHECK(hipGetLastError());
    a->leaf_waiting = false;
    return GMK_OK;
}

// Every game that is not over owes `playouts` more (several leaves per step: az_select_leaves_kernel takes them off as it completes them)
extern "C" int gmk_az_add_playouts(gmk_az* a, int playouts, void* stream) {
    if (!a || playouts < 0) { gmk::set_error("gmk_az_add_playouts: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_add_playouts: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    hipLaunchKernelGGL(az_add_playouts_kernel, dim3((a->t.n_games + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a->t, static_cast<uint32_t>(playouts));
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

// The largest number of playouts a game of the handle still owes (synchronises the stream)
extern "C" int gmk_az_playouts_owed(gmk_az* a, int32_t* h_max, void* stream) {
    if (!a || !h_max) { gmk::set_error("gmk_az_playouts_owed: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_playouts_owed: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (!a->d_owed) GMK_HIP_CHECK(gmk::device_malloc(&a->d_owed, 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
    GMK_HIP_CHECK(hipMemsetAsync(a->d_owed, 0, 4, s));
    hipLaunchKernelGGL(az_playouts_owed_kernel, dim3((a->t.n_games + 255) / 256), dim3(256), 0, s, a->t, a->d_owed);
    GMK_HIP_CHECK(hipGetLastError());
    int32_t owed = 0;
    GMK_HIP_CHECK(hipMemcpyAsync(&owed, a->d_owed, 4, hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    *h_max = owed;
    return GMK_OK;
}

extern "C" int gmk_az_root_stats(gmk_az* a, uint32_t* h_visits, float* h_values, float* h_priors, uint32_t* h_root_visits,
                                 float* h_root_value, int32_t* h_n_nodes, int32_t* h_status);

static int az_second_arena(gmk_az* a) {
    if (a->second_arena) return GMK_OK;
    const size_t n = static_cast<size_t>(a->t.n_games), nodes = n * static_cast<size_t>(a->t.cap);
    const bool ok = gmk::device_malloc(&a->other.stat, nodes * 8) == hipSuccess && gmk::device_malloc(&a->other.kids, nodes * 8) == hipSuccess &&
                    gmk::device_malloc(&a->other.prior, nodes * 4) == hipSuccess && gmk::device_malloc(&a->other.parent, nodes * 4) == hipSuccess &&
                    gmk::device_malloc(&a->d_forced, n * 2) == hipSuccess;
    if (!ok) {                                                      // all or nothing: a later call must not find half an arena
        (void)gmk::device_free(a->other.stat); (void)gmk::device_free(a->other.kids); (void)gmk::device_free(a->other.prior); (void)gmk::device_free(a->other.parent); (void)gmk::device_free(a->d_forced);
        a->other = AzArena{}; a->d_forced = nullptr;
        (void)hipGetLastError();
        gmk::set_error("gmk_az: hipMalloc of the second arena (%zu nodes) failed", nodes);
        return GMK_ERR_HIP;
    }
    a->second_arena = true;
    return GMK_OK;
}

extern "C" int gmk_az_step(gmk_az* a, const int16_t* h_moves) {
    if (!a) { gmk::set_error("gmk_az_step: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_step: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (az_marks_up(a, "gmk_az_step")) return GMK_ERR_STATE;
    const size_t n = static_cast<size_t>(a->t.n_games);
    if (const int rc = az_second_arena(a); rc != GMK_OK) return rc;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    if (h_moves) GMK_HIP_CHECK(hipMemcpy(a->d_forced, h_moves, n * 2, hipMemcpyHostToDevice));
    const auto kernel = az_proof_variant(a, [](auto proof) { return &az_step_kernel<proof>; });
    hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, nullptr, a->t, a->other, h_moves ? a->d_forced : nullptr);
    GMK_HIP_CHECK(hipGetLastError());
    if (const int rc = az_gumbel_clear(a, nullptr); rc != GMK_OK) return rc;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    az_flip_arenas(a);
    return GMK_OK;
}

// K20: the arguments of the two sampled entries, checked, as the kernels take them; plies == 0 when nothing is to be sampled
static int az_sample_args(const gmk_az* a, const char* who, int sample_plies, int sample_power, uint64_t seed, uint32_t first_game_id, AzSample* sm) {
    if (sample_plies < 0 || sample_plies > kCells || sample_power < 1 || sample_power > GMK_SAMPLE_MAX_POWER) {
        gmk::set_error("%s: sample_plies takes 0 .. 225 and sample_power 1 .. %d, not %d and %d", who, GMK_SAMPLE_MAX_POWER, sample_plies, sample_power);
        return GMK_ERR_ARG;
    }
    *sm = AzSample{a->slots.slot_game, a->d_game_ids, first_game_id, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(sample_plies), sample_power};
    return GMK_OK;
}

// gmk_az_root_choice and gmk_az_root_choice_sampled (sm: null, or what is to be sampled): one launch on `stream`
static int az_root_choice(gmk_az* a, const char* who, int16_t* d_cells, uint16_t* d_visits, const AzSample* sm, void* stream, const AzGumbel* gm = nullptr) {
    if (!a->rooted) { gmk::set_error("%s: gmk_az_set_roots has not been called", who); return GMK_ERR_STATE; }
    if (gm) {
        hipLaunchKernelGGL((az_root_choice_kernel<false, AzGumbel>), dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, d_cells, d_visits, *gm);
    } else if (sm && sm->plies != 0u) {
        const auto kernel = az_proof_variant(a, [](auto proof) { return &az_root_choice_kernel<proof, AzSample>; });
        hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, d_cells, d_visits, *sm);
    } else {
        const auto kernel = az_proof_variant(a, [](auto proof) { return &az_root_choice_kernel<proof>; });
        hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, static_cast<hipStream_t>(stream), a->t, d_cells, d_visits);
    }
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_az_root_choice(gmk_az* a, int16_t* d_cells, uint16_t* d_visits, void* stream) {
    if (!a || !d_cells) { gmk::set_error("gmk_az_root_choice: bad arguments"); return GMK_ERR_ARG; }
    return az_root_choice(a, "gmk_az_root_choice", d_cells, d_visits, nullptr, stream);
}

extern "C" int gmk_az_root_choice_sampled(gmk_az* a, int16_t* d_cells, uint16_t* d_visits, int sample_plies, int sample_power, uint64_t seed, uint32_t first_game_id,
                                          void* stream) {
    if (!a || !d_cells) { gmk::set_error("gmk_az_root_choice_sampled: bad arguments"); return GMK_ERR_ARG; }
    AzSample sm{};
    if (const int rc = az_sample_args(a, "gmk_az_root_choice_sampled", sample_plies, sample_power, seed, first_game_id, &sm); rc != GMK_OK) return rc;
    return az_root_choice(a, "gmk_az_root_choice_sampled", d_cells, d_visits, &sm, stream);
}

// gmk_az_step from device memory, on the caller's stream (az_step_device_kernel), then the leaf batch is compacted as gmk_az_advance
// compacts it.  The one synchronisation of a match ply is here: the number of live games (4 bytes) and, if asked for, the referee's count.
extern "C" int gmk_az_step_device(gmk_az* a, const int16_t* d_cells, const int32_t* d_verdict, int fresh_root, const int32_t* d_unfinished, int32_t* h_unfinished,
                                  void* stream) {
    if (!a || !d_cells || !d_verdict || (h_unfinished && !d_unfinished)) { gmk::set_error("gmk_az_step_device: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_step_device: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (az_marks_up(a, "gmk_az_step_device")) return GMK_ERR_STATE;
    if (a->slots.slot_game) { gmk::set_error("gmk_az_step_device: the handle plays through slots (gmk_az_set_slots): a match wants one game per slot"); return GMK_ERR_STATE; }
    if (!fresh_root)
        if (const int rc = az_second_arena(a); rc != GMK_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(az_step_device_kernel, dim3(a->t.n_games), dim3(64), 0, s, a->t, a->other, d_cells, d_verdict, fresh_root ? 1 : 0);
    GMK_HIP_CHECK(hipGetLastError());
    if (const int rc = az_gumbel_clear(a, s); rc != GMK_OK) return rc;
    int32_t unfinished = 0;
    if (h_unfinished) GMK_HIP_CHECK(hipMemcpyAsync(&unfinished, d_unfinished, 4, hipMemcpyDeviceToHost, s));
    if (const int rc = az_compact(a, s); rc != GMK_OK) return rc;   // (synchronises)
    if (!fresh_root) az_flip_arenas(a);
    if (h_unfinished) *h_unfinished = unfinished;
    return GMK_OK;
}

// One self-play move of every game still played (az_advance_kernel).  h_unfinished: the games that go on.  sm: null (gmk_az_advance), or what
// gmk_az_advance_sampled is to sample.
static int az_advance(gmk_az* a, const char* who, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int reuse_subtree, const AzSample* sm,
                      int32_t* h_unfinished, void* stream, const AzGumbel* gm = nullptr) {
    if (!a->rooted) { gmk::set_error("%s: gmk_az_set_roots has not been called", who); return GMK_ERR_STATE; }
    if (az_marks_up(a, who)) return GMK_ERR_STATE;
    if (reuse_subtree)
        if (const int rc = az_second_arena(a); rc != GMK_OK) return rc;
    if (!a->d_unfinished) GMK_HIP_CHECK(gmk::device_malloc(&a->d_unfinished, 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
    GMK_HIP_CHECK(hipMemsetAsync(a->d_unfinished, 0, 4, s));
    if (gm) {                                                    // K21: the kernel clears the ready words itself
        hipLaunchKernelGGL((az_advance_kernel<false, AzGumbel>), dim3(a->t.n_games), dim3(64), 0, s, a->t, a->other, d_moves, d_visits, d_lens, d_winner, a->d_unfinished,
                           reuse_subtree ? 1 : 0, a->slots, *gm);
    } else if (sm && sm->plies != 0u) {
        const auto kernel = az_proof_variant(a, [](auto proof) { return &az_advance_kernel<proof, AzSample>; });
        hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, s, a->t, a->other, d_moves, d_visits, d_lens, d_winner, a->d_unfinished, reuse_subtree ? 1 : 0, a->slots, *sm);
    } else {
        const auto kernel = az_proof_variant(a, [](auto proof) { return &az_advance_kernel<proof>; });
        hipLaunchKernelGGL(kernel, dim3(a->t.n_games), dim3(64), 0, s, a->t, a->other, d_moves, d_visits, d_lens, d_winner, a->d_unfinished, reuse_subtree ? 1 : 0, a->slots);
    }
    GMK_HIP_CHECK(hipGetLastError());
    if (!gm)
        if (const int rc = az_gumbel_clear(a, s); rc != GMK_OK) return rc;
    int32_t unfinished = 0;
    GMK_HIP_CHECK(hipMemcpyAsync(&unfinished, a->d_unfinished, 4, hipMemcpyDeviceToHost, s));
    if (const int rc = az_compact(a, s); rc != GMK_OK) return rc;   // (synchronises: both numbers are here now, and they agree)
    if (reuse_subtree) az_flip_arenas(a);
    if (h_unfinished) *h_unfinished = unfinished;
    return GMK_OK;
}

extern "C" int gmk_az_advance(gmk_az* a, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int reuse_subtree, int32_t* h_unfinished,
                              void* stream) {
    if (!a || !d_moves || !d_lens || !d_winner) { gmk::set_error("gmk_az_advance: bad arguments"); return GMK_ERR_ARG; }
    return az_advance(a, "gmk_az_advance", d_moves, d_visits, d_lens, d_winner, reuse_subtree, nullptr, h_unfinished, stream);
}

extern "C" int gmk_az_advance_sampled(gmk_az* a, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int reuse_subtree, int sample_plies,
                                      int sample_power, uint64_t seed, uint32_t first_game_id, int32_t* h_unfinished, void* stream) {
    if (!a || !d_moves || !d_lens || !d_winner) { gmk::set_error("gmk_az_advance_sampled: bad arguments"); return GMK_ERR_ARG; }
    AzSample sm{};
    if (const int rc = az_sample_args(a, "gmk_az_advance_sampled", sample_plies, sample_power, seed, first_game_id, &sm); rc != GMK_OK) return rc;
    return az_advance(a, "gmk_az_advance_sampled", d_moves, d_visits, d_lens, d_winner, reuse_subtree, &sm, h_unfinished, stream);
}

// The rule of include/gomoku_sample.h for n roots given by rows, on the host: needs no GPU and no gmk_init
extern "C" int gmk_move_sample_host(const uint32_t* h_visits, const int8_t* h_proofs, const int32_t* h_stones, const uint32_t* h_game_ids, int n, int sample_plies,
                                    int sample_power, uint64_t seed, int16_t* h_cells) {
    static_assert(GMK_SAMPLE_PROOF_WINS == GMK_AZ_PROOF_WINS && GMK_SAMPLE_PROOF_LOSES == GMK_AZ_PROOF_LOSES, "gomoku_sample.h reads the proofs of gomoku_hip.h");
    if (n < 0 || (n > 0 && (!h_visits || !h_stones || !h_game_ids || !h_cells)) || sample_plies < 0 || sample_plies > kCells || sample_power < 1 ||
        sample_power > GMK_SAMPLE_MAX_POWER) {
        gmk::set_error("gmk_move_sample_host: bad arguments (sample_plies 0 .. 225, sample_power 1 .. %d)", GMK_SAMPLE_MAX_POWER);
        return GMK_ERR_ARG;
    }
    for (int g = 0; g < n; ++g)
        if (h_stones[g] < 0 || h_stones[g] > kCells) { gmk::set_error("gmk_move_sample_host: row %d has %d stones", g, h_stones[g]); return GMK_ERR_ARG; }
    for (int g = 0; g < n; ++g) {
        h_cells[g] = static_cast<int16_t>(gmk_sample_choose225(h_visits + static_cast<size_t>(g) * kCells, h_proofs ? h_proofs + static_cast<size_t>(g) * kCells : nullptr,
                                                               static_cast<uint32_t>(h_stones[g]), h_game_ids[g], sample_plies, sample_power, static_cast<uint32_t>(seed),
                                                               static_cast<uint32_t>(seed >> 32)));
    }
    return GMK_OK;
}

// ---- K21: the option, the two entries that move by the rule, and the header's statements on the host ----
extern "C" int gmk_az_set_gumbel(gmk_az* a, int max_considered, int n_sims, double c_visit, double c_scale, uint64_t seed, uint32_t first_game_id) {
    if (!a) { gmk::set_error("gmk_az_set_gumbel: bad arguments"); return GMK_ERR_ARG; }
    if (max_considered == 0) {                                   // off: every entry launches what it launched before
        a->gumbel = false;
        return GMK_OK;
    }
    if (max_considered < 1 || max_considered > kCells || n_sims < 1 || n_sims > GMK_GUMBEL_MAX_SIMS || !(c_visit >= 0.0 && c_visit <= 1e300) || !(c_scale >= 0.0 && c_scale <= 1e300)) {
        gmk::set_error("gmk_az_set_gumbel: max_considered takes 0 (off) .. 225, n_sims 1 .. %d, c_visit and c_scale finite values >= 0; not %d, %d, %g, %g", GMK_GUMBEL_MAX_SIMS,
                       max_considered, n_sims, c_visit, c_scale);
        return GMK_ERR_ARG;
    }
    if (a->lv.leaves > 1) { gmk::set_error("gmk_az_set_gumbel: the Gumbel root search takes one leaf per step (GMK_OPT_AZ_LEAVES = %d)", a->lv.leaves); return GMK_ERR_STATE; }
    if (a->proof) { gmk::set_error("gmk_az_set_gumbel: the Gumbel root search does not carry proofs (GMK_OPT_AZ_PROOF = 1)"); return GMK_ERR_STATE; }
    const size_t n = static_cast<size_t>(a->t.n_games);
    GMK_HIP_CHECK(hipDeviceSynchronize());
    if (!a->gm.st) {
        if (gmk::device_malloc(&a->gm.st, n * sizeof(AzGumbelGame)) != hipSuccess || gmk::device_malloc(&a->gm.ready, n * 4) != hipSuccess) {
            (void)gmk::device_free(a->gm.st); (void)gmk::device_free(a->gm.ready);
            a->gm.st = nullptr; a->gm.ready = nullptr;
            (void)hipGetLastError();
            gmk::set_error("gmk_az_set_gumbel: hipMalloc of the per-game state (%zu games) failed", n);
            return GMK_ERR_HIP;
        }
    }
    GMK_HIP_CHECK(hipMemset(a->gm.ready, 0, n * 4));             // other parameters, other set-ups
    a->gm.first_game_id = first_game_id;
    a->gm.seed_lo = static_cast<uint32_t>(seed);
    a->gm.seed_hi = static_cast<uint32_t>(seed >> 32);
    a->gm.m = max_considered;
    a->gm.n = n_sims;
    a->gm.c_visit = c_visit;
    a->gm.c_scale = c_scale;
    a->gumbel = true;
    return GMK_OK;
}

extern "C" int gmk_az_root_choice_gumbel(gmk_az* a, int16_t* d_cells, uint16_t* d_visits, void* stream) {
    if (!a || !d_cells) { gmk::set_error("gmk_az_root_choice_gumbel: bad arguments"); return GMK_ERR_ARG; }
    if (!a->gumbel) { gmk::set_error("gmk_az_root_choice_gumbel: the Gumbel root search is off (gmk_az_set_gumbel)"); return GMK_ERR_STATE; }
    const AzGumbel gm = az_gumbel_args(a);
    return az_root_choice(a, "gmk_az_root_choice_gumbel", d_cells, d_visits, nullptr, stream, &gm);
}

extern "C" int gmk_az_advance_gumbel(gmk_az* a, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int reuse_subtree, int32_t* h_unfinished,
                                     void* stream) {
    if (!a || !d_moves || !d_lens || !d_winner) { gmk::set_error("gmk_az_advance_gumbel: bad arguments"); return GMK_ERR_ARG; }
    if (!a->gumbel) { gmk::set_error("gmk_az_advance_gumbel: the Gumbel root search is off (gmk_az_set_gumbel)"); return GMK_ERR_STATE; }
    const AzGumbel gm = az_gumbel_args(a);
    return az_advance(a, "gmk_az_advance_gumbel", d_moves, d_visits, d_lens, d_winner, reuse_subtree, nullptr, h_unfinished, stream, &gm);
}

// The statements of include/gomoku_gumbel.h for n roots given by rows, on the host: they need no GPU and no gmk_init
static bool gumbel_rule_args(const char* who, int n, bool pointers, double c_visit, double c_scale) {
    if (n < 0 || (n > 0 && !pointers) || !(c_visit >= 0.0 && c_visit <= 1e300) || !(c_scale >= 0.0 && c_scale <= 1e300)) {
        gmk::set_error("%s: bad arguments (n >= 0, no NULL row with n > 0, c_visit and c_scale finite and >= 0)", who);
        return false;
    }
    return true;
}
extern "C" int gmk_gumbel_sequence_host(int m_eff, int n_sims, uint32_t* h_seq) {
    if (m_eff < 1 || m_eff > kCells || n_sims < 1 || n_sims > GMK_GUMBEL_MAX_SIMS || !h_seq) {
        gmk::set_error("gmk_gumbel_sequence_host: bad arguments (m_eff 1 .. 225, n_sims 1 .. %d)", GMK_GUMBEL_MAX_SIMS);
        return GMK_ERR_ARG;
    }
    gmk_gumbel_sequence(m_eff, n_sims, h_seq);
    for (int t = 0; t < n_sims; ++t)                             // the kernels walk the phases instead of keeping the sequence: the two must agree
        if (gmk_gumbel_sequence_at(m_eff, n_sims, t) != h_seq[t]) { gmk::set_error("gmk_gumbel_sequence_host: the walk disagrees with the sequence at %d", t); return GMK_ERR_STATE; }
    return GMK_OK;
}
extern "C" int gmk_gumbel_setup_host(const float* h_prior, const uint32_t* h_visits, const int32_t* h_stones, const uint32_t* h_game_ids, int n, int max_considered,
                                     uint64_t seed, double* h_draws, double* h_score, uint32_t* h_base, uint8_t* h_considered, int32_t* h_m_eff) {
    if (n < 0 || (n > 0 && (!h_prior || !h_visits || !h_stones || !h_game_ids || !h_score || !h_base || !h_considered || !h_m_eff)) || max_considered < 1 ||
        max_considered > kCells) {
        gmk::set_error("gmk_gumbel_setup_host: bad arguments (max_considered 1 .. 225)");
        return GMK_ERR_ARG;
    }
    for (int g = 0; g < n; ++g)
        if (h_stones[g] < 0 || h_stones[g] > kCells) { gmk::set_error("gmk_gumbel_setup_host: row %d has %d stones", g, h_stones[g]); return GMK_ERR_ARG; }
    const uint32_t lo = static_cast<uint32_t>(seed), hi = static_cast<uint32_t>(seed >> 32);
    for (int g = 0; g < n; ++g) {
        const size_t at = static_cast<size_t>(g) * kCells;
        h_m_eff[g] = gmk_gumbel_setup225(h_prior + at, h_visits + at, max_considered, h_game_ids[g], static_cast<uint32_t>(h_stones[g]), lo, hi, h_score + at, h_base + at,
                                         h_considered + at);
        if (h_draws)
            for (int c = 0; c < kCells; ++c) h_draws[at + c] = gmk_gumbel_draw(h_game_ids[g], static_cast<uint32_t>(h_stones[g]), static_cast<uint32_t>(c), lo, hi);
    }
    return GMK_OK;
}
extern "C" int gmk_gumbel_pick_host(const float* h_prior, const uint32_t* h_visits, const float* h_value, const float* h_root_value, const double* h_score,
                                    const uint32_t* h_base, const uint8_t* h_considered, const int32_t* h_m_eff, int n, int n_sims, double c_visit, double c_scale,
                                    int16_t* h_cells) {
    if (!gumbel_rule_args("gmk_gumbel_pick_host", n, h_prior && h_visits && h_value && h_root_value && h_score && h_base && h_considered && h_m_eff && h_cells, c_visit, c_scale))
        return GMK_ERR_ARG;
    if (n_sims < 1 || n_sims > GMK_GUMBEL_MAX_SIMS) { gmk::set_error("gmk_gumbel_pick_host: n_sims takes 1 .. %d, not %d", GMK_GUMBEL_MAX_SIMS, n_sims); return GMK_ERR_ARG; }
    for (int g = 0; g < n; ++g)
        if (h_m_eff[g] < 0 || h_m_eff[g] > kCells) { gmk::set_error("gmk_gumbel_pick_host: row %d has m_eff = %d", g, h_m_eff[g]); return GMK_ERR_ARG; }
    for (int g = 0; g < n; ++g) {
        const size_t at = static_cast<size_t>(g) * kCells;
        h_cells[g] = static_cast<int16_t>(gmk_gumbel_pick225(h_prior + at, h_visits + at, h_value + at, h_root_value[g], h_score + at, h_base + at, h_considered + at,
                                                             h_m_eff[g], n_sims, c_visit, c_scale));
    }
    return GMK_OK;
}
extern "C" int gmk_gumbel_move_host(const float* h_prior, const uint32_t* h_visits, const float* h_value, const float* h_root_value, const double* h_score,
                                    const uint32_t* h_base, const uint8_t* h_considered, int n, double c_visit, double c_scale, int16_t* h_cells) {
    if (!gumbel_rule_args("gmk_gumbel_move_host", n, h_prior && h_visits && h_value && h_root_value && h_score && h_base && h_considered && h_cells, c_visit, c_scale))
        return GMK_ERR_ARG;
    for (int g = 0; g < n; ++g) {
        const size_t at = static_cast<size_t>(g) * kCells;
        h_cells[g] = static_cast<int16_t>(gmk_gumbel_move225(h_prior + at, h_visits + at, h_value + at, h_root_value[g], h_score + at, h_base + at, h_considered + at, c_visit,
                                                             c_scale));
    }
    return GMK_OK;
}
extern "C" int gmk_gumbel_row_host(const float* h_prior, const uint32_t* h_visits, const float* h_value, const float* h_root_value, int n, double c_visit, double c_scale,
                                   uint16_t* h_rows) {
    if (!gumbel_rule_args("gmk_gumbel_row_host", n, h_prior && h_visits && h_value && h_root_value && h_rows, c_visit, c_scale)) return GMK_ERR_ARG;
    for (int g = 0; g < n; ++g) {
        const size_t at = static_cast<size_t>(g) * kCells;
        gmk_gumbel_row225(h_prior + at, h_visits + at, h_value + at, h_root_value[g], c_visit, c_scale, h_rows + at);
    }
    return GMK_OK;
}

extern "C" int gmk_az_set_option(gmk_az* a, int option, int value) {
    if (a && az_marks_up(a, "gmk_az_set_option")) return GMK_ERR_STATE;
    if (a && a->gumbel && ((option == GMK_OPT_AZ_LEAVES && value > 1 && value <= GMK_AZ_MAX_LEAVES) || (option == GMK_OPT_AZ_PROOF && value == 1))) {
        gmk::set_error("gmk_az_set_option: the Gumbel root search (gmk_az_set_gumbel) takes one leaf per step and carries no proofs; switch it off first");
        return GMK_ERR_STATE;
    }
    if (a && option == GMK_OPT_AZ_LEAVES && value >= 1 && value <= GMK_AZ_MAX_LEAVES) {
        if (value > 1 && !a->lv.inflight) {                      // the side buffers: in-flight counts (all zero between steps) and the pending leaves
            const size_t n = static_cast<size_t>(a->t.n_games), nodes = n * static_cast<size_t>(a->t.cap);
            GMK_HIP_CHECK(hipDeviceSynchronize());
            if (gmk::device_malloc(&a->lv.inflight, nodes * 2) != hipSuccess || gmk::device_malloc(&a->lv.pend, n * GMK_AZ_MAX_LEAVES * sizeof(AzPending)) != hipSuccess) {
                (void)gmk::device_free(a->lv.inflight); (void)gmk::device_free(a->lv.pend);
                a->lv.inflight = nullptr; a->lv.pend = nullptr;
                (void)hipGetLastError();
                gmk::set_error("gmk_az_set_option: hipMalloc of the in-flight counts (%zu nodes) failed", nodes);
                return GMK_ERR_HIP;
            }
            GMK_HIP_CHECK(hipMemset(a->lv.inflight, 0, nodes * 2));
            GMK_HIP_CHECK(hipMemset(a->lv.pend, 0, n * GMK_AZ_MAX_LEAVES * sizeof(AzPending)));
        }
        a->lv.leaves = value;
        return GMK_OK;
    }
    if (a && (option == GMK_OPT_AZ_VCF_DEPTH || option == GMK_OPT_AZ_VCF_BUDGET)) {
        const bool depth = option == GMK_OPT_AZ_VCF_DEPTH;
        if (depth ? (value < 0 || value > GMK_VCF_MAX_DEPTH) : (value < 1 || value > (1 << 20))) {
            gmk::set_error("gmk_az_set_option: GMK_OPT_AZ_VCF_DEPTH takes 0 .. %d and GMK_OPT_AZ_VCF_BUDGET 1 .. 2^20, not %d", GMK_VCF_MAX_DEPTH, value);
            return GMK_ERR_ARG;
        }
        if (a->leaf_waiting) { gmk::set_error("gmk_az_set_option: gmk_az_select is waiting for its gmk_az_expand; the leaves' verdicts belong to the old setting"); return GMK_ERR_STATE; }
        if (!depth) { a->vcf.budget = static_cast<uint32_t>(value); return GMK_OK; }
        if (value > 0 && !a->vcf.verdict) {                      // one verdict per row of the largest leaf batch; every row reads "no leaf" until a select writes it
            const size_t rows = static_cast<size_t>(a->t.n_games) * GMK_AZ_MAX_LEAVES;
            const std::vector<int4> none(rows, make_int4(GMK_VCF_NONE, -1, 0, 0));
            GMK_HIP_CHECK(hipDeviceSynchronize());
            if (gmk::device_malloc(&a->vcf.verdict, rows * sizeof(int4)) != hipSuccess) {
                a->vcf.verdict = nullptr;
                (void)hipGetLastError();
                gmk::set_error("gmk_az_set_option: hipMalloc of the verdict buffer (%zu rows) failed", rows);
                return GMK_ERR_HIP;
            }
            GMK_HIP_CHECK(hipMemcpy(a->vcf.verdict, none.data(), rows * sizeof(int4), hipMemcpyHostToDevice));
        }
        a->vcf.max_depth = value;
        return az_defend_buffers(a);
    }
    if (a && option == GMK_OPT_AZ_PROOF && (value == 0 || value == 1)) {
        if (a->leaf_waiting) { gmk::set_error("gmk_az_set_option: gmk_az_select is waiting for its gmk_az_expand; GMK_OPT_AZ_PROOF changes how it is answered"); return GMK_ERR_STATE; }
        a->proof = value == 1;                                   // the bits stay where they are: facts about positions, ignored while the option is off
        return az_defend_buffers(a);
    }
    if (a && option == GMK_OPT_AZ_VCF_DEFEND && (value == 0 || value == 1)) {
        if (a->leaf_waiting) { gmk::set_error("gmk_az_set_option: gmk_az_select is waiting for its gmk_az_expand; GMK_OPT_AZ_VCF_DEFEND changes how it is answered"); return GMK_ERR_STATE; }
        a->defend = value == 1;                                  // inert unless the solver and the proofs are on as well
        return az_defend_buffers(a);
    }
    if (a && option == GMK_OPT_NOISE_SAMPLER && (value == GMK_NOISE_SAMPLER_STD || value == GMK_NOISE_SAMPLER_COUNTER)) { a->noise_sampler = value; return GMK_OK; }
    gmk::set_error("gmk_az_set_option: bad handle, unknown option %d or value %d", option, value);
    return GMK_ERR_ARG;
}

// Default::AddNoise on every root with children, seeded like gmk_mcts_add_root_noise / gmk_trad_add_root_noise.  The counter sampler is one
// launch on `stream` and does not wait.  The std sampler draws on the host: it waits for `stream`, then for the device, and returns finished.
extern "C" int gmk_az_add_root_noise(gmk_az* a, float alpha, float epsilon, uint64_t seed, uint32_t first_game_id, void* stream) {
    if (!a) { gmk::set_error("gmk_az_add_root_noise: bad arguments"); return GMK_ERR_ARG; }
    if (!gmk::noise_args_ok("gmk_az_add_root_noise", alpha, epsilon)) return GMK_ERR_ARG;
    if (!a->rooted) { gmk::set_error("gmk_az_add_root_noise: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (az_marks_up(a, "gmk_az_add_root_noise")) return GMK_ERR_STATE;
    const size_t n = static_cast<size_t>(a->t.n_games);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->noise_sampler == GMK_NOISE_SAMPLER_COUNTER) {         // drawn on the device, one wavefront per game: nothing comes back to the host
        hipLaunchKernelGGL(az_root_noise_kernel, dim3(a->t.n_games), dim3(64), 0, s, a->t, a->slots.slot_game, a->d_game_ids, first_game_id, alpha, epsilon,
                           static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
        GMK_HIP_CHECK(hipGetLastError());
        return GMK_OK;
    }
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    if (a->slots.slot_game) {                                    // continuous batching: the random stream belongs to the GAME a slot plays
        std::vector<int32_t> slot_game(n);
        GMK_HIP_CHECK(hipMemcpy(slot_game.data(), a->slots.slot_game, n * 4, hipMemcpyDeviceToHost));
        for (size_t g = 0; g < n; ++g) a->game_ids[g] = slot_game[g] >= 0 ? static_cast<uint32_t>(slot_game[g]) : 0u;
        if (const int rc = az_upload_game_ids(a); rc != GMK_OK) return rc;
    }
    std::vector<float> priors(n * 225);
    int rc = gmk_az_root_stats(a, nullptr, nullptr, priors.data(), nullptr, nullptr, nullptr, nullptr);
    if (rc != GMK_OK) return rc;
    std::vector<AzHeader> hdr(n);
    GMK_HIP_CHECK(hipMemcpy(hdr.data(), a->t.hdr, n * sizeof(AzHeader), hipMemcpyDeviceToHost));
    gmk::for_each_game(n, [&](size_t g) {
        float* p = &priors[g * 225];
        bool any = false;
        for (int i = 0; i < 225; ++i) any |= p[i] != 0.0f;
        if (any) gmk::mix_root_noise(p, 225, alpha, epsilon, gmk::root_noise_engine_seed(seed, first_game_id + a->game_ids[g], hdr[g].stones));
    });
    if (!a->d_noise_priors) GMK_HIP_CHECK(gmk::device_malloc(&a->d_noise_priors, n * 225 * 4));
    GMK_HIP_CHECK(hipMemcpy(a->d_noise_priors, priors.data(), n * 225 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(az_set_root_priors_kernel, dim3(a->t.n_games), dim3(64), 0, nullptr, a->t, a->d_noise_priors);
    GMK_HIP_CHECK(hipGetLastError());
    GMK_HIP_CHECK(hipDeviceSynchronize());
    return GMK_OK;
}

// ---- host-driven form for callers that evaluate leaves on the host (one game behind CorePyExt: the evaluator is a Python
// callable that wants a Board): the moves from the root to each pending leaf, and value / probabilities from host memory ----
namespace {
__global__ void az_leaf_path_kernel(AzTree t, int16_t* paths, int32_t* lens) {
    const int game = blockIdx.x * blockDim.x + threadIdx.x;
    if (game >= t.n_games) return;
    const AzHeader& hdr = t.hdr[game];
    int16_t* out = paths + static_cast<size_t>(game) * 226;
    if (!hdr.leaf_pending) { lens[game] = -1; return; }
    const size_t arena = static_cast<size_t>(game) * t.cap;
    int depth = 0;
    for (uint32_t node = hdr.leaf; node != 0u && node != kNoNode; node = t.parent[arena + node]) ++depth;
    lens[game] = depth;
    int i = depth;
    for (uint32_t node = hdr.leaf; node != 0u && node != kNoNode; node = t.parent[arena + node])
        out[--i] = static_cast<int16_t>((t.kids[arena + node].y >> 8) & 0xFFu);
}
}  // namespace

static bool az_host_scratch(gmk_az* a) {
    if (a->h_states) return true;
    const size_t n = static_cast<size_t>(a->t.n_games);
    return gmk::device_malloc(&a->h_states, n * 6 * 225 * 4) == hipSuccess && gmk::device_malloc(&a->h_values, n * 4) == hipSuccess &&
           gmk::device_malloc(&a->h_probs, n * 225 * 4) == hipSuccess && gmk::device_malloc(&a->h_paths, n * 226 * 2) == hipSuccess &&
           gmk::device_malloc(&a->h_lens, n * 4) == hipSuccess;
}

// gmk_az_select, then for every game the moves from the root to its pending leaf: h_paths int16[n][226], h_lens int32[n]
// (-1 = the playout ended at a finished game and is already backed up: nothing to evaluate)
extern "C" int gmk_az_select_host(gmk_az* a, int16_t* h_paths, int32_t* h_lens) {
    if (!a || !h_paths || !h_lens) { gmk::set_error("gmk_az_select_host: bad arguments"); return GMK_ERR_ARG; }
    if (az_many_leaves(a, "gmk_az_select_host")) return GMK_ERR_STATE;
    if (!az_host_scratch(a)) { gmk::set_error("gmk_az_select_host: device allocation failed"); return GMK_ERR_HIP; }
    const int rc = gmk_az_select(a, a->h_states, nullptr);
    if (rc != GMK_OK) return rc;
    hipLaunchKernelGGL(az_leaf_path_kernel, dim3((a->t.n_games + 63) / 64), dim3(64), 0, nullptr, a->t, a->h_paths, a->h_lens);
    GMK_HIP_CHECK(hipGetLastError());
    GMK_HIP_CHECK(hipMemcpy(h_paths, a->h_paths, static_cast<size_t>(a->t.n_games) * 226 * 2, hipMemcpyDeviceToHost));
    GMK_HIP_CHECK(hipMemcpy(h_lens, a->h_lens, static_cast<size_t>(a->t.n_games) * 4, hipMemcpyDeviceToHost));
    return GMK_OK;
}

extern "C" int gmk_az_expand_host(gmk_az* a, const float* h_values, const float* h_probs) {
    if (!a || !h_values || !h_probs) { gmk::set_error("gmk_az_expand_host: bad arguments"); return GMK_ERR_ARG; }
    if (az_many_leaves(a, "gmk_az_expand_host")) return GMK_ERR_STATE;
    if (!az_host_scratch(a)) { gmk::set_error("gmk_az_expand_host: device allocation failed"); return GMK_ERR_HIP; }
    GMK_HIP_CHECK(hipMemcpy(a->h_values, h_values, static_cast<size_t>(a->t.n_games) * 4, hipMemcpyHostToDevice));
    GMK_HIP_CHECK(hipMemcpy(a->h_probs, h_probs, static_cast<size_t>(a->t.n_games) * 225 * 4, hipMemcpyHostToDevice));
    const int rc = gmk_az_expand(a, a->h_values, a->h_probs, nullptr);
    if (rc != GMK_OK) return rc;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    return GMK_OK;
}

// ---- Host-driven stages: Policy(select=, expand=, back_prop=) hands Python callables to MCTS::playout
// (core/py_ext/src/mcts_ext.hpp:43-61, core/lib/include/MCTS.h:74-101).  A Python callable runs on the host by definition; the tree stays on the
// device and the host reads the node it is asked about, decides, and tells the device: a node and its children out, the chosen leaf in, expand
// and / or back up as separate steps, statistics of a path written back, and Default::Simulate's random rollout (MonteCarlo.hpp:83-88) from the
// pending leaf as a one-wavefront kernel on the rollout code of K3.  One game of the handle at a time; synchronous; for CorePyExt's one-game MCTS.
namespace {
__global__ __launch_bounds__(64)
void az_leaf_rollout_kernel(AzTree t, int game, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1, int32_t* winner) {
    using namespace gmk::rollout;
    __shared__ uint32_t s_lines[kLineWords];
    __shared__ uint2 s_cells[30];
    const int lane = threadIdx.x;
    const AzHeader& hdr = t.hdr[game];
    const int stones = static_cast<int>(hdr.leaf_stones);
    for (int w = lane; w < kLineWords; w += 64) s_lines[w] = 0u;
    __syncthreads();
    if (lane < 15) {
        const uint32_t row = hdr.leaf_rows[lane];
        s_lines[lane] = row;
        for (uint32_t m = (row | (row >> 16)) & 0x7FFFu; m; m &= m - 1u) {
            const int x = __ffs(m) - 1, y = lane;
            const uint32_t cb = ((row >> x) & 1u) ? 0u : 16u;
            atomicOr(&s_lines[kColBase + x], 1u << (y + cb));
            atomicOr(&s_lines[kDiagBase + x - y + 14], 1u << (x + cb));
            atomicOr(&s_lines[kAntiBase + x + y], 1u << (x + cb));
        }
    }
    if (lane < 30 && 8 * lane < 225 - stones) s_cells[lane] = rollout_cells(c0, c1, c2, static_cast<uint32_t>(lane), k0, k1);
    __syncthreads();
    if (lane == 0) *winner = random_rollout_blocks(s_lines, 1u, (stones & 1) ? -1 : 1, stones, 0, [&](uint32_t b) { return s_cells[b]; });
}
}  // namespace

extern "C" int gmk_az_read_node_host(gmk_az* a, int game, uint32_t node, uint32_t* h_visits, float* h_value, float* h_prior, int32_t* h_cell, uint32_t* h_parent,
                                     uint32_t* h_first_child, int32_t* h_n_children) {
    if (!a || game < 0 || game >= a->t.n_games || node >= static_cast<uint32_t>(a->t.cap)) { gmk::set_error("gmk_az_read_node_host: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_read_node_host: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    const size_t at = static_cast<size_t>(game) * a->t.cap + node;
    uint2 st, kd;
    float pr;
    uint32_t par;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(&st, a->t.stat + at, 8, hipMemcpyDeviceToHost));
    GMK_HIP_CHECK(hipMemcpy(&kd, a->t.kids + at, 8, hipMemcpyDeviceToHost));
    GMK_HIP_CHECK(hipMemcpy(&pr, a->t.prior + at, 4, hipMemcpyDeviceToHost));
    GMK_HIP_CHECK(hipMemcpy(&par, a->t.parent + at, 4, hipMemcpyDeviceToHost));
    if (h_visits) *h_visits = st.x;
    if (h_value) std::memcpy(h_value, &st.y, 4);
    if (h_prior) *h_prior = pr;
    if (h_cell) *h_cell = static_cast<int32_t>((kd.y >> 8) & 0xFFu);
    if (h_parent) *h_parent = par;
    if (h_first_child) *h_first_child = kd.x;
    if (h_n_children) *h_n_children = static_cast<int32_t>(kd.y & 0xFFu);
    return GMK_OK;
}

extern "C" int gmk_az_read_children_host(gmk_az* a, int game, uint32_t first_child, int n, int16_t* h_cells, uint32_t* h_visits, float* h_values, float* h_priors,
                                         int32_t* h_n_children) {
    if (!a || game < 0 || game >= a->t.n_games || n < 0 || n > 225 || static_cast<size_t>(first_child) + n > static_cast<size_t>(a->t.cap)) { gmk::set_error("gmk_az_read_children_host: bad arguments"); return GMK_ERR_ARG; }
    if (n == 0) return GMK_OK;
    const size_t at = static_cast<size_t>(game) * a->t.cap + first_child;
    uint2 st[225], kd[225];
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(st, a->t.stat + at, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost));
    GMK_HIP_CHECK(hipMemcpy(kd, a->t.kids + at, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost));
    if (h_priors) GMK_HIP_CHECK(hipMemcpy(h_priors, a->t.prior + at, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        if (h_cells) h_cells[i] = static_cast<int16_t>((kd[i].y >> 8) & 0xFFu);
        if (h_visits) h_visits[i] = st[i].x;
        if (h_values) std::memcpy(&h_values[i], &st[i].y, 4);
        if (h_n_children) h_n_children[i] = static_cast<int32_t>(kd[i].y & 0xFFu);
    }
    return GMK_OK;
}

// the leaf the host's descent ended at: node `leaf`, reached from the root over h_path[0 .. depth): it becomes the pending leaf of the next
// gmk_az_expand_stages_host / gmk_az_rollout_host (what az_select_kernel leaves behind for a device-side descent)
extern "C" int gmk_az_set_leaf_host(gmk_az* a, int game, uint32_t leaf, const int16_t* h_path, int depth) {
    if (!a || game < 0 || game >= a->t.n_games || depth < 0 || depth > 225 || (depth > 0 && !h_path) || leaf >= static_cast<uint32_t>(a->t.cap)) { gmk::set_error("gmk_az_set_leaf_host: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_set_leaf_host: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (az_many_leaves(a, "gmk_az_set_leaf_host")) return GMK_ERR_STATE;
    AzHeader h;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(&h, a->t.hdr + game, sizeof h, hipMemcpyDeviceToHost));
    for (int y = 0; y < 16; ++y) h.leaf_rows[y] = h.rows[y];
    uint32_t stones = h.stones;
    for (int i = 0; i < depth; ++i, ++stones) {
        const int c = h_path[i];
        if (c < 0 || c >= 225 || ((h.leaf_rows[c / 15] | (h.leaf_rows[c / 15] >> 16)) >> (c % 15)) & 1u) { gmk::set_error("gmk_az_set_leaf_host: the path is not a sequence of moves"); return GMK_ERR_ARG; }
        h.leaf_rows[c / 15] |= 1u << (c % 15 + ((stones & 1u) ? 16 : 0));
    }
    h.leaf = leaf; h.leaf_pending = 1; h.leaf_stones = stones;
    GMK_HIP_CHECK(hipMemcpy(a->t.hdr + game, &h, sizeof h, hipMemcpyHostToDevice));
    return GMK_OK;
}

// gmk_az_expand_host with the two halves of az_expand_kernel switched separately: expand (children with h_probs, Default::Expand) and / or
// back up (-h_values along the parent chain, Default::BackPropogate); the pending leaves are done either way
extern "C" int gmk_az_expand_stages_host(gmk_az* a, const float* h_values, const float* h_probs, int do_expand, int do_backup) {
    if (!a || (do_backup && !h_values) || (do_expand && !h_probs)) { gmk::set_error("gmk_az_expand_stages_host: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_expand_stages_host: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (az_many_leaves(a, "gmk_az_expand_stages_host")) return GMK_ERR_STATE;
    if (!az_host_scratch(a)) { gmk::set_error("gmk_az_expand_stages_host: device allocation failed"); return GMK_ERR_HIP; }
    if (h_values) GMK_HIP_CHECK(hipMemcpy(a->h_values, h_values, static_cast<size_t>(a->t.n_games) * 4, hipMemcpyHostToDevice));
    if (h_probs) GMK_HIP_CHECK(hipMemcpy(a->h_probs, h_probs, static_cast<size_t>(a->t.n_games) * 225 * 4, hipMemcpyHostToDevice));
    else GMK_HIP_CHECK(hipMemset(a->h_probs, 0, static_cast<size_t>(a->t.n_games) * 225 * 4));
    hipLaunchKernelGGL((az_expand_kernel<false, false, false>), dim3(a->t.n_games), dim3(64), 0, nullptr, a->t, a->h_values, a->h_probs, (do_expand ? 1 : 0) | (do_backup ? 2 : 0), a->vcf, a->df);
    GMK_HIP_CHECK(hipGetLastError());
    a->leaf_waiting = false;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    return GMK_OK;
}

// node statistics as a Python back_prop left them: h_nodes[i] gets {h_visits[i], h_values[i]}
extern "C" int gmk_az_write_stats_host(gmk_az* a, int game, const uint32_t* h_nodes, const uint32_t* h_visits, const float* h_values, int n) {
    if (!a || game < 0 || game >= a->t.n_games || n < 0 || (n > 0 && (!h_nodes || !h_visits || !h_values))) { gmk::set_error("gmk_az_write_stats_host: bad arguments"); return GMK_ERR_ARG; }
    if (az_many_leaves(a, "gmk_az_write_stats_host")) return GMK_ERR_STATE;
    GMK_HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < n; ++i) {
        if (h_nodes[i] >= static_cast<uint32_t>(a->t.cap)) { gmk::set_error("gmk_az_write_stats_host: node %u outside the arena", h_nodes[i]); return GMK_ERR_ARG; }
        uint2 st;
        st.x = h_visits[i];
        std::memcpy(&st.y, &h_values[i], 4);
        GMK_HIP_CHECK(hipMemcpy(a->t.stat + static_cast<size_t>(game) * a->t.cap + h_nodes[i], &st, 8, hipMemcpyHostToDevice));
    }
    return GMK_OK;
}

// Default::Simulate's random rollout from the pending leaf of `game` (one wavefront, the rollout of K3): the winner (+1 black, -1 white, 0 tie).
// The cell draws are Philox(seed; counter0, counter1, counter2, block of eight plies): with (global game id, playout number, root stones << 8)
// they are the draws of K3's first rollout lane, i.e. MCTS(RandomPolicy(c_puct, 1)) of gmk_mcts_*.
extern "C" int gmk_az_rollout_host(gmk_az* a, int game, uint64_t seed, uint32_t counter0, uint32_t counter1, uint32_t counter2, int32_t* h_winner) {
    if (!a || game < 0 || game >= a->t.n_games || !h_winner) { gmk::set_error("gmk_az_rollout_host: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_rollout_host: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    if (az_many_leaves(a, "gmk_az_rollout_host")) return GMK_ERR_STATE;
    if (!a->d_unfinished) GMK_HIP_CHECK(gmk::device_malloc(&a->d_unfinished, 4));
    hipLaunchKernelGGL(az_leaf_rollout_kernel, dim3(1), dim3(64), 0, nullptr, a->t, game, counter0, counter1, counter2, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), a->d_unfinished);
    GMK_HIP_CHECK(hipGetLastError());
    GMK_HIP_CHECK(hipMemcpy(h_winner, a->d_unfinished, 4, hipMemcpyDeviceToHost));
    return GMK_OK;
}

extern "C" int gmk_az_root_stats(gmk_az* a, uint32_t* h_visits, float* h_values, float* h_priors, uint32_t* h_root_visits,
                                 float* h_root_value, int32_t* h_n_nodes, int32_t* h_status) {
    if (!a) { gmk::set_error("gmk_az_root_stats: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_root_stats: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    const size_t n = static_cast<size_t>(a->t.n_games);
    // One block, the pool's at any size: the host-driven loops read the roots once per ply.  The kernel writes visits, values and priors only where
    // the root has a child, and a block that comes back from the pool is not cleared: the clear of the three is what makes the other cells read 0.
    gmk::Staging st("gmk_az_root_stats", gmk::kPoolKeeps);
    uint32_t *d_visits, *d_root_visits;
    float *d_values, *d_priors, *d_root_value;
    st.out(d_visits, h_visits, n * 225, true); st.out(d_values, h_values, n * 225, true); st.out(d_priors, h_priors, n * 225, true);
    st.out(d_root_visits, h_root_visits, n, true); st.out(d_root_value, h_root_value, n, true);
    if (const int rc = st.take(); rc != GMK_OK) return rc;
    GMK_STAGED(st, hipMemset(d_visits, 0, reinterpret_cast<char*>(d_priors + n * 225) - reinterpret_cast<char*>(d_visits)));      // visits | values | priors lie side by side
    GMK_STAGED(st, hipDeviceSynchronize());
    hipLaunchKernelGGL(az_root_stats_kernel, dim3(a->t.n_games), dim3(64), 0, nullptr, a->t, d_visits, d_values, d_priors, d_root_visits, d_root_value);
    GMK_STAGED(st, hipGetLastError());
    GMK_STAGED(st, hipDeviceSynchronize());
    if (const int rc = st.download(); rc != GMK_OK) return rc;
    std::vector<AzHeader> hdr(n);
    GMK_STAGED(st, hipMemcpy(hdr.data(), a->t.hdr, n * sizeof(AzHeader), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < n; ++g) {
        if (h_n_nodes) h_n_nodes[g] = static_cast<int32_t>(hdr[g].n_nodes);
        if (h_status) h_status[g] = static_cast<int32_t>(hdr[g].status);
    }
    return GMK_OK;
}

// ---- K7 + K14: the read-out ----
extern "C" int gmk_az_vcf_stats(gmk_az* a, uint32_t* h_leaves, uint32_t* h_wins, uint32_t* h_cut, uint64_t* h_nodes) {
    GMK_NEED_INIT();
    if (!a) { gmk::set_error("gmk_az_vcf_stats: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_vcf_stats: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    const size_t n = static_cast<size_t>(a->t.n_games);
    std::vector<AzHeader> hdr(n);
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(hdr.data(), a->t.hdr, n * sizeof(AzHeader), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < n; ++g) {
        if (h_leaves) h_leaves[g] = hdr[g].vcf_leaves;
        if (h_wins) h_wins[g] = hdr[g].vcf_wins;
        if (h_cut) h_cut[g] = hdr[g].vcf_cut;
        if (h_nodes) h_nodes[g] = hdr[g].vcf_nodes;
    }
    return GMK_OK;
}

extern "C" int gmk_az_vcf_verdicts_host(gmk_az* a, int32_t* h_status, int32_t* h_move, int32_t* h_length, uint32_t* h_nodes) {
    GMK_NEED_INIT();
    if (!a) { gmk::set_error("gmk_az_vcf_verdicts_host: bad arguments"); return GMK_ERR_ARG; }
    if (a->vcf.max_depth == 0 || !a->vcf.verdict) { gmk::set_error("gmk_az_vcf_verdicts_host: the leaves are not solved (GMK_OPT_AZ_VCF_DEPTH = 0)"); return GMK_ERR_STATE; }
    const size_t rows = static_cast<size_t>(a->n_live) * static_cast<size_t>(a->lv.leaves);
    std::vector<int4> v(rows);
    GMK_HIP_CHECK(hipDeviceSynchronize());
    if (rows) GMK_HIP_CHECK(hipMemcpy(v.data(), a->vcf.verdict, rows * sizeof(int4), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        if (h_status) h_status[r] = v[r].x;
        if (h_move) h_move[r] = v[r].y;
        if (h_length) h_length[r] = v[r].z;
        if (h_nodes) h_nodes[r] = static_cast<uint32_t>(v[r].w);
    }
    return GMK_OK;
}

// ---- K7 + proofs: the read-outs ----
extern "C" int gmk_az_root_proofs(gmk_az* a, int8_t* h_root, int8_t* h_children) {
    GMK_NEED_INIT();
    if (!a) { gmk::set_error("gmk_az_root_proofs: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_root_proofs: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    const size_t n = static_cast<size_t>(a->t.n_games);
    gmk::Staging st("gmk_az_root_proofs");                        // one block: the children's rows | the roots; the kernel writes both
    int8_t *d_children, *d_root;
    st.out(d_children, h_children, n * 225, true); st.out(d_root, h_root, n, true);
    GMK_STAGED(st, hipDeviceSynchronize());
    if (const int rc = st.take(); rc != GMK_OK) return rc;
    hipLaunchKernelGGL(az_root_proofs_kernel, dim3(a->t.n_games), dim3(64), 0, nullptr, a->t, d_root, d_children);
    GMK_STAGED(st, hipGetLastError());
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}

extern "C" int gmk_az_proof_stats(gmk_az* a, uint32_t* h_proved, uint32_t* h_stops) {
    GMK_NEED_INIT();
    if (!a) { gmk::set_error("gmk_az_proof_stats: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_proof_stats: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    const size_t n = static_cast<size_t>(a->t.n_games);
    std::vector<AzHeader> hdr(n);
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(hdr.data(), a->t.hdr, n * sizeof(AzHeader), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < n; ++g) {
        if (h_proved) h_proved[g] = hdr[g].proof_proved;
        if (h_stops) h_stops[g] = hdr[g].proof_stops;
    }
    return GMK_OK;
}

// ---- K7 + K15: the read-outs ----
extern "C" int gmk_az_defend_stats(gmk_az* a, uint32_t* h_threatened, uint32_t* h_marked, uint32_t* h_searched, uint64_t* h_nodes) {
    GMK_NEED_INIT();
    if (!a) { gmk::set_error("gmk_az_defend_stats: bad arguments"); return GMK_ERR_ARG; }
    if (!a->rooted) { gmk::set_error("gmk_az_defend_stats: gmk_az_set_roots has not been called"); return GMK_ERR_STATE; }
    const size_t n = static_cast<size_t>(a->t.n_games);
    std::vector<AzHeader> hdr(n);
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(hdr.data(), a->t.hdr, n * sizeof(AzHeader), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < n; ++g) {
        if (h_threatened) h_threatened[g] = hdr[g].def_threatened;
        if (h_marked) h_marked[g] = hdr[g].def_marked;
        if (h_searched) h_searched[g] = hdr[g].def_searched;
        if (h_nodes) h_nodes[g] = hdr[g].def_nodes;
    }
    return GMK_OK;
}

extern "C" int gmk_az_defend_verdicts_host(gmk_az* a, int32_t* h_threat_status, int32_t* h_threat_length, int8_t* h_verdict, uint32_t* h_nodes) {
    GMK_NEED_INIT();
    if (!a) { gmk::set_error("gmk_az_defend_verdicts_host: bad arguments"); return GMK_ERR_ARG; }
    if (!az_defend_active(a) || !a->df.threat) { gmk::set_error("gmk_az_defend_verdicts_host: the defence solver is not asked (GMK_OPT_AZ_VCF_DEFEND with GMK_OPT_AZ_VCF_DEPTH > 0 and GMK_OPT_AZ_PROOF)"); return GMK_ERR_STATE; }
    const size_t rows = static_cast<size_t>(a->n_live) * static_cast<size_t>(a->lv.leaves);
    std::vector<int4> th(rows);
    std::vector<uint16_t> occupied(rows * 16);
    std::vector<uint32_t> cells(rows * kCells);
    GMK_HIP_CHECK(hipDeviceSynchronize());
    if (rows) {
        GMK_HIP_CHECK(hipMemcpy(th.data(), a->df.threat, rows * sizeof(int4), hipMemcpyDeviceToHost));
        GMK_HIP_CHECK(hipMemcpy(occupied.data(), a->df.occupied, rows * 16 * 2, hipMemcpyDeviceToHost));
        GMK_HIP_CHECK(hipMemcpy(cells.data(), a->df.cells, rows * kCells * 4, hipMemcpyDeviceToHost));
    }
    for (size_t r = 0; r < rows; ++r) {
        const bool asked = th[r].w != 0, win = asked && th[r].x == GMK_VCF_WIN;
        if (h_threat_status) h_threat_status[r] = th[r].x;
        if (h_threat_length) h_threat_length[r] = th[r].y;
        // the cells of a row that is not under a WIN threat were never written: K15's table for them follows from the threat's status alone
        const int other = !asked || th[r].x == GMK_VCF_OVER ? GMK_VCF_CELL_NONE : th[r].x == GMK_VCF_NONE ? GMK_VCF_CELL_HOLDS : GMK_VCF_CELL_UNKNOWN;
        for (int c = 0; c < kCells; ++c) {
            const uint32_t w = cells[r * kCells + c];
            const bool taken = (occupied[r * 16 + c / 15] >> (c % 15)) & 1u;
            if (h_verdict) h_verdict[r * kCells + c] = static_cast<int8_t>(win ? (w & kCellVerdict) : taken ? GMK_VCF_CELL_NONE : other);
            if (h_nodes) h_nodes[r * kCells + c] = win ? w >> kCellNodesShift : 0u;
        }
    }
    return GMK_OK;
}
