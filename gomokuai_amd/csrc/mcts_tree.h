// mcts_tree.h -- the K3 handle and the per-game header of its trees (mcts_kernel.hip), for the kernels outside that file that read a
// root: the tree lives in HBM, one arena of node_capacity nodes per game, structure-of-arrays: stats {visits u32, value f32}, link
// {first child << 8 | cell} (the children of a node are consecutive, in ascending cell order) and parent.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/gomoku_hip.h"

namespace gmk {
namespace mcts {

struct GameHeader {                 // 128 B per game, in HBM
    uint32_t rows[16];              // root position: black | white << 16 per row
    uint32_t root;                  // node index of the root inside the arena
    uint32_t n_nodes;               // nodes in use (MCTS::m_size)
    uint32_t stones;                // stones on the root board (= Policy::m_initActs)
    uint32_t last_move;             // cell of the last move, 255 if none
    uint32_t game_id;               // global game id (RNG counter word 0)
    uint32_t status;                // bit 0: the game is over, bit 1: an arena of this slot filled up (sticky over a slot's games), bit 2: illegal move requested
    uint64_t alg_bytes;             // algorithmic tree bytes of the last run
    uint32_t playouts_done;         // playouts already run from this root (RNG counter word 1 continues across launches)
    uint32_t noise;                 // 1: the root's children take their priors from root_prior[] (Default::AddNoise ran)
    uint32_t root_expanded;         // scratch for gmk_mcts_add_root_noise
    uint32_t pad[4];                // (diagnostic build: clock sums of the four phases)
    uint32_t arena;                 // the persistent self-play loop with kept subtrees: which of the game's two arenas holds its tree (0 / 1); 0 everywhere else
};
static_assert(sizeof(GameHeader) == 128, "GameHeader layout");

// Continuous batching for whole-game self-play (gmk_selfplay_run): the handle's games are SLOTS; slot g plays game slot_game[g] of
// n_total, its records go to that game's rows, and when the game ends the slot takes the next game nobody has started (a counter in
// device memory): its opening position becomes the slot's root, its global id the slot's random-number key.  So the search
// launches stay full until fewer games than slots remain, instead of waiting for the longest game of a fixed batch.
struct SlotRefill {
    int32_t* slot_game;             // [n_slots] game played by each slot, -1 = none (null: slot g plays game g and is not refilled)
    int32_t* next_game;             // [1] first game not started yet
    int n_total;
    const uint8_t* open_moves;      // [n_total][open_stride] opening moves (black first), may be null
    const int32_t* open_lens;       // [n_total] (<= 8: an opening cannot be a finished game)
    int open_stride;
    uint32_t first_game_id;
};

}  // namespace mcts
}  // namespace gmk

struct gmk_mcts {
    int n_games = 0, node_capacity = 0, c_rollouts = 5, games_per_block = 12;
    double c_puct = 5.0;
    uint64_t seed = 0;
    gmk::mcts::GameHeader* d_headers = nullptr;
    uint2* d_stats = nullptr;          // live arena
    uint32_t* d_link = nullptr;
    uint32_t* d_parent = nullptr;
    uint2* d_stats2 = nullptr;         // second arena, allocated by the first advance() that keeps subtrees
    uint32_t* d_link2 = nullptr;
    uint32_t* d_parent2 = nullptr;
    float* d_root_prior = nullptr;     // [n_games][225] by child index, used while GameHeader::noise is set
    float* d_value = nullptr;          // [2 * c_rollouts + 1] rollout sum -> state value
    gmk::mcts::SlotRefill slots{};                // continuous batching (gmk_selfplay_run); all null otherwise
    struct { uint8_t* moves; uint16_t* visits; int32_t* lens; int8_t* winner; int32_t* unfinished; int reuse; float noise_alpha, noise_epsilon; int sample_plies, sample_power; } persistent_rec{};     // set while gmk_selfplay_run's ONE launch is issued
    int32_t* d_slot_state = nullptr;   // [n_games + 1] slot_game, next_game
    int32_t* d_step_counters = nullptr; // [2] mcts_advance_kernel's own (zero between launches)
    uint8_t* d_open_moves = nullptr;
    int32_t* d_open_lens = nullptr;
    void* d_step_scratch = nullptr;    // record outputs of gmk_mcts_step_host
    hipStream_t last_stream = nullptr;
    bool rooted = false;               // gmk_mcts_set_roots has run: headers and arenas hold trees
    // gmk_mcts_set_option
    int noise_sampler = GMK_NOISE_SAMPLER_STD;   // where Default::AddNoise draws from
    int lockstep = 0;                  // 1: gmk_selfplay_run alternates search and step launches even where ONE persistent launch could play the games
    // the persistent loop with kept subtrees wants a game's two arenas a fixed distance apart: both halves of ONE allocation per array
    bool paired = false;
    uint2* block_stats = nullptr;
    uint32_t *block_link = nullptr, *block_parent = nullptr;
    void* d_ensemble = nullptr;        // accumulators of gmk_mcts_ensemble_merge (ensemble_kernel.hip), [ensemble_capacity] ensembles
    int ensemble_capacity = 0;
    size_t arena_stride() const { return (paired && d_stats2 > d_stats) ? static_cast<size_t>(d_stats2 - d_stats) : 0; }
};
