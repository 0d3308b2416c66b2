// trad_tree.h -- the "first child" search tree shared by the kernels whose select stage is RAVE::Select
// (core/lib/include/algorithms/MonteCarlo.hpp:149-152): K6 (trad_kernel.hip, TraditionalPolicy) and K8 (rave_kernel.hip,
// PoolRAVEPolicy).  One arena of `cap` nodes per game in HBM, the root at index 0, children of a node consecutive;
// what RAVE::BackPropogate's swaps change is kept as the node's position in its parent's order (`ord`) and the parent's
// record of its current first child (`front`).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/gomoku_sample.h"
#include "board_device.h"
#include "wave_fence.h"

namespace gmk {
namespace tree {

using gmk::wave_phase_fence;

constexpr uint32_t kNoParent = 0xFFFFFFu;
constexpr uint32_t kNoChild = 0xFFFFFFFFu;       // most_visited_child / child_of_cell: the node has no such child

constexpr uint32_t kStatusIdleSlot = 16u;        // continuous batching (gmk_trad_selfplay_run): the slot's games have run out, the searches skip it

struct TradHeader {                              // 64 B per game in HBM
    uint32_t n_nodes, init_acts, status, fresh;  // status: bit 0 node capacity reached, bit 1 evaluator error, bit 2 board-only revert met, bit 3 illegal step, bit 4 idle slot
                                                 // fresh: 1 = new root + evaluator sync, 2 = the tree was re-rooted (kept): evaluator sync only
    uint32_t playouts_done, root_black, pad0, pad1;
    unsigned long long evaluator_updates, pad2;
    uint32_t prof[4];                            // GMK_TRAD_PROFILE: shader clocks (>> 10) in select + evaluator moves, simulate + expand, backup, all
};
static_assert(sizeof(TradHeader) == 64, "TradHeader layout");

struct TradArena {
    uint2* stat;                                 // [n_games][cap] {visits, value bits}
    uint2* info;                                 // [n_games][cap] {parent | cell << 24, prior bits}
    uint32_t* link;                              // [n_games][cap] first child | children << 24
    uint2* front;                                // [n_games][cap] the child that is first in the CURRENT order: {id | cell << 24, its link word}
    uint8_t* ord;                                // [n_games][cap] the node's position in its parent's current child order
    uint2* amaf;                                 // [n_games][cap] {amaf_visits, amaf_value bits} (AMAFNode, MonteCarlo.hpp:113-122); null for K6 without RAVE
};

// What the device-resident self-play loop (gmk_trad_selfplay_run) hands its step kernel: the game a slot plays and the hand-over of a
// finished game's slot to the next unstarted game, the openings, and the records by GAME (not by slot).
struct TradSelfPlay {
    int32_t* slot_game;                          // [n_slots] the game (0 .. n_total-1) a slot plays, -1: none
    int32_t* next_game;                          // the next unstarted game
    int n_total;
    const uint8_t* open_moves;                   // [n_total][open_stride], may be null
    const int32_t* open_lens;                    // [n_total]
    int open_stride;
    uint32_t* game_ids;                          // [n_slots] = slot_game as the searches and the root noise key their streams
    uint8_t* rec_moves;                          // [n_total][225]
    int32_t* rec_lens;                           // [n_total]
    uint16_t* rec_visits;                        // [n_total][225][225] or null: root visit counts of every searched ply
    int8_t* rec_winner;                          // [n_total]
    int32_t* unfinished;                         // slots that still have a game after this step
    int32_t* overflow;                           // set when a search stopped at its node capacity
    // the persistent loop with the reference agent's per-move semantics (MCTS.cpp:129-147, 179-183): the chosen child's subtree is kept -- compacted
    // into the slot's OTHER arena, arena_stride nodes further on, inside the launch -- and Default::AddNoise runs before every search, drawn by the
    // wavefront itself from the counter-based sampler (include/gomoku_noise.h), keyed by (seed; first_game_id + game, stones, cell)
    int reuse;
    float noise_alpha, noise_epsilon;            // alpha == 0: no noise
    size_t arena_stride;                         // nodes between a slot's two arenas (0: one arena)
    uint32_t seed_lo, seed_hi, first_game_id;
};

// ---- wave-wide reductions without LDS round trips ----
// DPP row_shl by N lanes for 64-bit and unsigned values; a lane without a source inside its row of 16 keeps its own value
template <int N>
__device__ __forceinline__ double row_down_keep(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, 0x100 + N, 0xF, 0xF, false), __builtin_amdgcn_update_dpp(lo, lo, 0x100 + N, 0xF, 0xF, false));
}
template <int N>
__device__ __forceinline__ uint32_t row_down_keep(uint32_t v) {
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(v), static_cast<int>(v), 0x100 + N, 0xF, 0xF, false));
}
__device__ __forceinline__ double lane_value(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// wave-wide maximum of doubles that are never NaN / minimum of unsigned values: DPP inside the rows, the four row leaders by readlane
__device__ __forceinline__ double wave_max(double v) {
    v = fmax(v, row_down_keep<8>(v)); v = fmax(v, row_down_keep<4>(v)); v = fmax(v, row_down_keep<2>(v)); v = fmax(v, row_down_keep<1>(v));
    return fmax(fmax(lane_value(v, 0), lane_value(v, 16)), fmax(lane_value(v, 32), lane_value(v, 48)));
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = min(v, row_down_keep<8>(v)); v = min(v, row_down_keep<4>(v)); v = min(v, row_down_keep<2>(v)); v = min(v, row_down_keep<1>(v));
    const uint32_t a = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 0)), b = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 16));
    const uint32_t c = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 32)), d = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 48));
    return min(min(a, b), min(c, d));
}

// ---- the root's move, once: what the searches' step, advance, statistics and self-play kernels share ----
// All of it is one wavefront's work on ONE game: the pointers are offset to the game's arena, `first` and `n` are the root's child range.
// Where a piece has two phases that hand data to each other, the caller passes how ITS lanes meet -- the scopes differ and stay as they
// are: the persistent turn of trad_playouts_kernel is one wavefront of a 512-thread workgroup (SyncWave; copy_sync<true> around
// copy_subtree), the one-wavefront kernels are whole workgroups (SyncBlock; copy_sync<false>).
struct SyncWave { __device__ __forceinline__ void operator()() const { wave_phase_fence(); } };
struct SyncBlock { __device__ __forceinline__ void operator()() const { __syncthreads(); } };

// MCTS::stepForward()'s choice (MCTS.cpp:129-134): the most visited child, among equals the one that is first in the CURRENT child order
// (a child without visits counts: of unvisited children the first is taken).  The node id, kNoChild when n == 0.
__device__ __forceinline__ uint32_t most_visited_child(const uint2* stat, const uint8_t* ord, uint32_t first, uint32_t n, int lane) {
    uint32_t best = 0u, best_ord = 0u, best_id = kNoChild;      // best: visits + 1, 0 = no child yet
    const auto take_if_better = [&](uint32_t v, uint32_t o, uint32_t id) {
        if (v > best || (v == best && v != 0u && o < best_ord)) { best = v; best_ord = o; best_id = id; }
    };
    for (uint32_t i = lane; i < n; i += 64) take_if_better(stat[first + i].x + 1u, ord[first + i], first + i);
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t v = __shfl_down(best, s), o = __shfl_down(best_ord, s), id = __shfl_down(best_id, s);
        take_if_better(v, o, id);
    }
    return __shfl(best_id, 0);
}

// MCTS::stepForward(move)'s search (MCTS.cpp:136-139): the child of that cell (a cell has at most one), kNoChild without one
__device__ __forceinline__ uint32_t child_of_cell(const uint2* info, uint32_t first, uint32_t n, uint32_t cell, int lane) {
    uint32_t id = kNoChild;
    for (uint32_t i = lane; i < n; i += 64) if ((info[first + i].x >> 24) == cell) id = first + i;
    for (int s = 32; s > 0; s >>= 1) id = min(id, static_cast<uint32_t>(__shfl_xor(id, s)));
    return id;
}

// the children's visit counts by cell, saturated at 65 535: a searched ply's row of a game's record, the referee's row
template <class Sync>
__device__ __forceinline__ void visits_by_cell(uint16_t* row, const uint2* stat, const uint2* info, uint32_t first, uint32_t n, int lane, Sync sync) {
    for (int i = lane; i < 225; i += 64) row[i] = 0;
    sync();
    for (uint32_t i = lane; i < n; i += 64) row[info[first + i].x >> 24] = static_cast<uint16_t>(min(stat[first + i].x, 65535u));
}

// K20: the first `plies` plies of a self-play game are drawn in proportion to visits^power (include/gomoku_sample.h has the rule and its
// serial statement, gmk_sample_choose225 without proofs).  The kernels that take it are the instantiations with one TradSample among their
// arguments; the game id is the GLOBAL one, the id the root noise is keyed by.
struct TradSample {
    uint32_t seed_lo, seed_hi, first_game_id;
    uint32_t plies;                              // S > 0
    int power;                                   // k in 1..3
};

// The cell the rule draws from a root's visit counts BY CELL (`row`: what visits_by_cell wrote, in LDS or in the game's record; the caller's
// lanes have met since), -1 for a row without weight.  The children are not kept in cell order, so the choice is a function of the row and
// not of them: lane l holds the cells 4 l .. 4 l + 3, cell order is lane order, the weights stay in registers, one inclusive scan of the
// lanes' 64-bit sums gives every lane the prefix before its first cell, and the first lane with a prefix above the target holds the choice.
__device__ __forceinline__ int sampled_cell(const uint16_t* row, int lane, const TradSample& sm, uint32_t game_id, uint32_t stones) {
    uint64_t w[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * lane + j;
        w[j] = c < 225 ? gmk_sample_weight(row[c], sm.power) : 0;
        sum += w[j];
    }
    uint64_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t below = __shfl_up(static_cast<unsigned long long>(incl), d);
        if (lane >= d) incl += below;
    }
    const uint64_t total = __shfl(static_cast<unsigned long long>(incl), 63);
    if (total == 0) return -1;
    const uint64_t target = gmk_sample_target(total, game_id, stones, sm.seed_lo, sm.seed_hi);
    uint64_t prefix = incl - sum;
    int hit = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        prefix += w[j];
        if (hit < 0 && prefix > target) hit = 4 * lane + j;
    }
    const unsigned long long hits = __ballot(hit >= 0);                                // (never empty: target < total)
    return __shfl(hit, __ffsll(static_cast<long long>(hits)) - 1);
}

// The child a sampled ply plays, called where most_visited_child is and with its result: on a root with `stones` >= S stones, without
// children or without weight it IS most_visited_child.  Otherwise the root's row by cell is written first -- into `record_row` (the searched
// ply's row of the game's record; *row_written says so and the caller does not write it again) or, without one, into `lds_row` (225
// uint16_t of the caller's LDS) -- and the drawn cell's child is looked up.
template <class Sync>
__device__ __forceinline__ uint32_t sampled_child(const uint2* stat, const uint2* info, const uint8_t* ord, uint32_t first, uint32_t n, int lane, const TradSample& sm,
                                                  uint32_t game_id, uint32_t stones, uint16_t* record_row, uint16_t* lds_row, bool* row_written, Sync sync) {
    *row_written = false;
    if (stones >= sm.plies || n == 0u) return most_visited_child(stat, ord, first, n, lane);
    int cell;
    if (record_row) {
        visits_by_cell(record_row, stat, info, first, n, lane, sync);
        sync();
        cell = sampled_cell(record_row, lane, sm, game_id, stones);
        *row_written = true;
    } else {
        visits_by_cell(lds_row, stat, info, first, n, lane, sync);
        sync();
        cell = sampled_cell(lds_row, lane, sm, game_id, stones);
    }
    if (cell < 0) return most_visited_child(stat, ord, first, n, lane);
    return child_of_cell(info, first, n, static_cast<uint32_t>(cell), lane);
}

// The root choice of a kernel instantiated without a TradSample (most_visited_child, and nothing more is read or written) or with one
// (sampled_child for the game `game` -- relative to the sample's first_game_id -- at `stones` stones)
template <class Sync, class... Sample>
__device__ __forceinline__ uint32_t root_child(const uint2* stat, const uint2* info, const uint8_t* ord, uint32_t first, uint32_t n, int lane, uint32_t game, uint32_t stones,
                                               uint16_t* record_row, uint16_t* lds_row, bool* row_written, Sync sync, const Sample&... sm) {
    static_assert(sizeof...(Sample) <= 1 && (std::is_same_v<Sample, TradSample> && ...), "at most one TradSample");
    if constexpr (sizeof...(Sample) == 1) {
        const TradSample& one = (sm, ...);
        return sampled_child(stat, info, ord, first, n, lane, one, one.first_game_id + game, stones, record_row, lds_row, row_written, sync);
    } else {
        *row_written = false;
        return most_visited_child(stat, ord, first, n, lane);
    }
}

// Board::applyMove's victory check (Game.cpp:37-49, 88-136) for `cell` played after moves[0 .. len): the board after the move as row
// words in rows[0 .. 16) (the caller's LDS; move i is black's when i is even, white's stones 16 bits up), five or more through the cell
// win.  The winner: +1 black, -1 white, 0 nobody (yet).
template <class Sync>
__device__ __forceinline__ int play_cell(const uint8_t* moves, int len, uint32_t cell, uint32_t* rows, int lane, Sync sync) {
    if (lane < 16) rows[lane] = 0u;
    sync();
    for (int i = lane; i < len; i += 64) atomicOr(&rows[moves[i] / 15u], 1u << (moves[i] % 15u + ((i & 1) ? 16u : 0u)));
    const int shift = (len & 1) ? 16 : 0;
    if (lane == 0) atomicOr(&rows[cell / 15u], 1u << (cell % 15u + shift));
    sync();
    const bool five = gmk::five_through<1>(rows, static_cast<int>(cell % 15u), static_cast<int>(cell / 15u), shift);
    return five ? (shift ? -1 : 1) : 0;
}

// is `cell` a move that moves[0 .. len) allows: on the board, the board not full, the cell not taken (one answer for the wavefront)
__device__ __forceinline__ bool legal_reply(const uint8_t* moves, int len, uint32_t cell, int lane) {
    bool legal = cell < 225u && len < 225;
    for (int i = lane; i < len; i += 64) legal &= moves[i] != cell;
    return __all(legal);
}

// MCTS::reset / stepForward(move) without such a child (MCTS.cpp:140-145): the game's tree is one childless root behind `cell` (255: the
// empty board), written by ONE lane; amaf: the nodes carry AMAF statistics.  A root's `ord` is never read (the backup and the root choice read their CHILDREN's) and a childless
// node's `front` is not either (select follows it only where link >> 24 != 0): `ord` is written because some callers always did, `front` by none.
__device__ __forceinline__ void new_root(const TradArena& a, size_t base, uint32_t cell, bool amaf) {
    a.stat[base] = make_uint2(0u, 0u);
    a.info[base] = make_uint2(kNoParent | (cell << 24), __float_as_uint(1.0f));
    a.link[base] = 0u;
    a.ord[base] = 0;
    if (amaf) a.amaf[base] = make_uint2(0u, 0u);
}

// MCTS::stepForward() / stepForward(move) (MCTS.cpp:129-147): the chosen child's subtree becomes the tree.  The reference
// frees the siblings; here the kept subtree is copied level by level into the other arena so that node indices stay dense
// (children consecutive, the root at 0).  A copied node carries its OLD child range and OLD first-child record until the
// scan reaches it, copies its children and rewrites both.  One wavefront per game.
// kWaveOnly: the caller is one wavefront of a larger workgroup (the persistent self-play loop of trad_playouts_kernel): its lanes meet at a
// wavefront barrier with workgroup-scope fences (the CU's L1 is shared by the workgroup) instead of __syncthreads().
template <bool kWaveOnly>
__device__ __forceinline__ void copy_sync() {
    if constexpr (kWaveOnly) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// The subtree of node src_root of arena a becomes the tree of arena b, level by level (see above); one wavefront.  Returns the node count.
template <bool kWaveOnly>
__device__ uint32_t copy_subtree(const TradArena& a, const TradArena& b, size_t base, uint32_t src_root, int lane) {
    if (lane == 0) {
        b.stat[base] = a.stat[base + src_root];
        b.info[base] = make_uint2(kNoParent | (a.info[base + src_root].x & 0xFF000000u), a.info[base + src_root].y);
        b.link[base] = a.link[base + src_root];
        b.front[base] = a.front[base + src_root];
        b.ord[base] = 0;
        if (a.amaf) b.amaf[base] = a.amaf[base + src_root];
    }
    copy_sync<kWaveOnly>();
    uint32_t next = 1;
    for (uint32_t i0 = 0, chunk = 0; i0 < next; i0 += chunk) {
        chunk = min(64u, next - i0);                            // nodes appended while this chunk is handled come after it
        const uint32_t old_link = static_cast<uint32_t>(lane) < chunk ? b.link[base + i0 + lane] : 0u;
        unsigned long long todo = __ballot((old_link >> 24) != 0u);
        while (todo) {
            const int j = __ffsll(static_cast<long long>(todo)) - 1;
            todo &= todo - 1ull;
            const uint32_t ol = __shfl(old_link, j), of = ol & 0xFFFFFFu, nk = ol >> 24, node = i0 + static_cast<uint32_t>(j);
            for (uint32_t k = lane; k < nk; k += 64) {
                const uint2 inf = a.info[base + of + k];
                b.stat[base + next + k] = a.stat[base + of + k];
                b.info[base + next + k] = make_uint2(node | (inf.x & 0xFF000000u), inf.y);
                b.link[base + next + k] = a.link[base + of + k];
                b.front[base + next + k] = a.front[base + of + k];
                b.ord[base + next + k] = a.ord[base + of + k];
                if (a.amaf) b.amaf[base + next + k] = a.amaf[base + of + k];
            }
            if (lane == 0) {
                const uint32_t new_link = next | (nk << 24);
                b.link[base + node] = new_link;
                const uint2 fr = b.front[base + node];              // still the OLD id of the first child in the current order
                b.front[base + node] = make_uint2((next + ((fr.x & 0xFFFFFFu) - of)) | (fr.x & 0xFF000000u), fr.y);
                if (node != 0u) {                                   // am I my parent's first child?  then its record of me carries my child range
                    const uint32_t p = b.info[base + node].x & 0xFFFFFFu;
                    const uint2 pf = b.front[base + p];
                    if ((pf.x & 0xFFFFFFu) == node) b.front[base + p] = make_uint2(pf.x, new_link);
                }
            }
            next += nk;
            copy_sync<kWaveOnly>();
        }
        copy_sync<kWaveOnly>();                                        // children written above are scanned below
    }
    return next;
}

}  // namespace tree
}  // namespace gmk

struct gmk_trad {
    int n_games = 0, cap = 0;
    uint32_t* d_states = nullptr;
    gmk::tree::TradArena a{}, b{};               // the arena that holds the trees; the other one (trad_second_arena: the step kernels copy the kept subtrees into it, then the two flip)
                                                 // a.amaf: made by the first gmk_trad_run_poolrave / gmk_trad_run_rave; b.amaf follows it
    int16_t* d_forced = nullptr;
    float* d_priors = nullptr;
    gmk::tree::TradHeader* d_hdr = nullptr;
    uint8_t* d_moves = nullptr;
    int32_t* d_lens = nullptr;
    std::vector<uint32_t> game_ids;                                         // the game a slot is playing, relative to the callers' first_game_id (default: the slot number)
    uint32_t* d_game_ids = nullptr;
    uint32_t* d_path_spill = nullptr;            // [n_games][kPathSpill] K6: the child ranges of path levels the LDS copy has no room for
    bool attr_set = false, attr_set_selfplay = false, attr_set_rave = false, attr_set_selfplay_rave = false, attr_set_sampled = false, attr_set_sampled_rave = false, positioned = false, second_arena = false;
    // gmk_trad_set_option
    int noise_sampler = 0;                       // GMK_NOISE_SAMPLER_STD: where Default::AddNoise draws from
    int lockstep = 0;
    // the persistent loop with kept subtrees wants a slot's two arenas a fixed distance apart: both halves of ONE allocation per array
    bool paired = false;
    gmk::tree::TradArena block{};                // a and b are its halves then; block.amaf (TraditionalPolicy + RAVE handles): ensure_amaf, trad_kernel.hip
    void* d_ensemble = nullptr;                                             // accumulators of gmk_trad_ensemble_merge (ensemble_kernel.hip), [ensemble_capacity] ensembles
    int ensemble_capacity = 0;
    size_t arena_stride() const { return (paired && b.stat > a.stat) ? static_cast<size_t>(b.stat - a.stat) : 0; }
    int policy = 0;                                                          // 0 not searched yet, 1 TraditionalPolicy (gmk_trad_run), 2 PoolRAVEPolicy (gmk_trad_run_poolrave),
                                                                             // 3 TraditionalPolicy + RAVE (gmk_trad_run_rave): one per handle
};
