/*
 * gomoku_hip.h -- C-ABI of libgomoku_hip.so, the MI355X (gfx950) implementation of the GomokuAI
 * self-play hot path: the Aho-Corasick line-pattern evaluator and the MCTS playout loop.
 *
 * This is the drop-in boundary underneath the reference's pybind11 module `CorePyExt`
 * (core/py_ext/src/module.cpp:7-13): the C++ binding layer (gomokuai_amd/csrc/core_pyext.cpp, or the
 * stub shown in INTEGRATION.md for the reference tree) is the only code that touches Python objects;
 * everything below is plain pointers and sizes.  Paths in comments are relative to the reference root.
 *
 * Conventions
 *   - every function returns 0 on success, a negative gmk_status otherwise; gmk_last_error() has text;
 *   - `d_` pointers are DEVICE (HBM) pointers, `h_` pointers are host pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are asynchronous on it: an entry that takes a
 *     `stream` does all of its device work on that stream, and one that returns host values waits for that stream first;
 *   - an entry WITHOUT a `stream` that reads or writes a handle is ordered after everything already enqueued for that handle, on any
 *     stream (it waits for the device at its head), and has finished when it returns (gmk_mcts_root_stats and gmk_mcts_alg_bytes
 *     wait for the stream of the handle's last call instead);
 *   - there is no CPU fallback: without a usable HIP device every compute entry returns GMK_ERR_NO_DEVICE.
 *
 * Board encoding (replaces Board::m_moveStates, core/lib/include/Game.h:146-150)
 *   planes: uint16_t[n][2][16]   plane 0 = black stones, plane 1 = white stones,
 *           word y = row y, bit x = column x (x,y in 0..14), word 15 and bit 15 are zero.  64 B per board.
 *   Position id = y*15 + x (Game.h:45-56).  Player: -1 white, 0 none, +1 black (Game.h:19-21).
 *
 * Move choice in self-play
 *   Every searcher plays its most visited root child, as MCTS::stepForward does (core/lib/src/MCTS.cpp:129-134).  The K7 self-play
 *   entries can instead draw the first plies of a game in proportion to the visit counts (AlphaZero's temperature schedule):
 *   gmk_az_advance_sampled, gmk_az_root_choice_sampled and, on the host, gmk_move_sample_host, see "K20" below.  The rule is integer
 *   arithmetic on a counter-based stream keyed by the game and its stone count (gomoku_sample.h), so every loop plays the same games
 *   and a record's visit row reproduces its move.  The unsampled entries, the K3 / K6 / K8 self-play loops and matches are unchanged.
 *   K7 self-play at few playouts per move can instead run Gumbel AlphaZero at the root (gmk_az_set_gumbel, gmk_az_advance_gumbel,
 *   gmk_az_root_choice_gumbel; gomoku_gumbel.h states the rule, see "K21" below): the record's row is then the improved policy, read
 *   back with GMK_TARGET_POLICY.
 */
#ifndef GOMOKU_HIP_H_
#define GOMOKU_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GMK_OK = 0,
    GMK_ERR_NO_DEVICE = -1,     /* no HIP device / HIP runtime error at init */
    GMK_ERR_HIP = -2,           /* a HIP call failed */
    GMK_ERR_ARG = -3,           /* invalid argument */
    GMK_ERR_STATE = -4,         /* library not initialised / handle invalid */
    GMK_ERR_CAPACITY = -5       /* a fixed capacity (tree arena, queue) was exceeded */
} gmk_status;

enum { GMK_BOARD_CELLS = 225, GMK_PLANE_WORDS = 16, GMK_TOTALS = 11 };

/* ---- library ---- */
int gmk_init(int device);                 /* builds the pattern automaton on the host and uploads it */
int gmk_shutdown(void);
/* Large device blocks (the tree arenas: tens of GB per handle) that a destroyed handle gives up are kept by the library for the next handle
 * (the driver clears memory before it hands it out again: seconds per 24 GB); at most 224 GB idle (the longest-idle blocks go first), and never more than three quarters of what the
 * device could hand out if the pool gave everything back (the idle blocks are invisible to other allocators of the process).  This returns the idle ones to the
 * driver, e.g. before another allocator in the process needs the memory; gmk_shutdown does it too. */
int gmk_pool_release(void);
/* Diagnostic switch of that pool (off by default): a block that is handed out again is first filled with 0xA5, so that a kernel which reads a
 * node nobody wrote since meets garbage instead of the previous handle's (plausible) tree.  The pool never clears a block otherwise: the driver's
 * clear is 1.5 s per 24 GB, and no kernel reads what it has not written -- tests/test_pool_gpu.py searches on poisoned blocks to hold that. */
int gmk_pool_poison(int on);
const char *gmk_last_error(void);
int gmk_device_info(int *cu_count, size_t *hbm_bytes, char *name, int name_cap);

/* ---- pattern tables (host side; usable without a GPU) ----
 * Replaces the static `Evaluator::Patterns` (core/lib/src/Pattern.cpp:554-596) and its builder
 * (core/lib/src/utils/ACAutomata.cpp:15-274). */
typedef struct {
    int32_t n_patterns;        /* 294 */
    int32_t n_states;          /* dense DFA states */
    int32_t dat_size;          /* length of base/check/fail (1024) */
    int32_t max_emissions;     /* longest emission list of one transition */
    int32_t trans_words;       /* n_states*4 */
    int32_t emit_words;        /* uint16 entries */
    int32_t invariants[5];
} gmk_table_info;
int gmk_tables_info(gmk_table_info *info);
/* pattern i: rich string (<=7 chars + NUL), favour (+1/-1), type (Pattern::Type, Pattern.h:33-39), score */
int gmk_tables_pattern(int i, char str[8], int *favour, int *type, int *score);
/* copies of the GPU tables (see gomokuai_amd/csrc/pattern_tables.h for the bit layout) */
int gmk_tables_copy(uint32_t *trans, uint16_t *emit_lists, uint32_t *pattern_info);
/* copies of the reference-shaped double array (PatternSearch::m_base/m_check/m_fail, Pattern.h:89-92) */
int gmk_tables_copy_dat(int32_t *base, int32_t *check, int32_t *fail);
/* Table self-check: runs the flattened DFA on the host over codes[n] (1=x 2=o 3=? 4=blank) and writes the
 * (pattern, end offset) stream; returns the number of matches.  Not used by any compute entry. */
int gmk_tables_scan(const uint8_t *codes, int n, int32_t *patterns, int32_t *offsets, int cap);

/* ---- synthetic workloads (host side) ----
 * kind 0 "random-opening": L = 8 + u32 % 53 plies, each ply r = u32 % 225 then the reference probe rule
 *        (core/lib/src/Game.cpp:68-72); stops early on five-in-row.
 * kind 1 "clustered": 90 % of plies land within Chebyshev distance 2 of a random earlier stone.
 * Philox4x32-10, key = seed, counter = (first_board + i, draw, kind, 0).
 * moves: uint8[n][stride] (stride >= 64), lens: int32[n], planes (optional): uint16[n][2][16]. */
int gmk_synth_boards(uint64_t seed, uint32_t first_board, int n, int kind,
                     uint8_t *h_moves, int stride, int32_t *h_lens, uint16_t *h_planes);
/* move list -> planes (black moves first, alternating), host side */
int gmk_moves_to_planes(const uint8_t *h_moves, int stride, const int32_t *h_lens, int n, uint16_t *h_planes);

/* ---- K1: batched position evaluation ----
 * Computes, from the stones alone, what the reference's incrementally maintained Evaluator
 * (core/lib/src/Pattern.cpp:111-386) holds after those stones were played:
 *   scores  int32[n][4][225]     Evaluator::m_scores, group = (favour==black)<<1 | (perspective==black)   (Pattern.h:159-161,219)
 *   density int32[n][2][2][225]  Evaluator::m_density [white,black][count,weight]; occupied cells hold -v-1 (Pattern.cpp:236-272)
 *   totals  uint32[n][11]        m_patternDist[225][0..7] then m_compoundDist[225][0..2]: white count in the low,
 *                                black in the high 16 bits (Pattern.cpp:390-393)
 *   status  int32[n]             bit0 game over, bit1 evaluator error (the reference would read out of bounds,
 *                                Pattern.cpp:484-485, or the board queues 384 or more emitting transitions: no legal position
 *                                found so far does, DESIGN.md "K1's fixed capacities"), bits 8..15 winner, bits 16..23 player to move
 * Any output pointer may be NULL.  All pointers are device pointers; n boards; asynchronous on stream. */
int gmk_eval_batch(const uint16_t *d_planes, int n,
                   int32_t *d_scores, int32_t *d_density, uint32_t *d_totals, int32_t *d_status,
                   void *stream);
/* same with host buffers (allocates, copies in, runs, copies out, synchronises) */
int gmk_eval_batch_host(const uint16_t *h_planes, int n,
                        int32_t *h_scores, int32_t *h_density, uint32_t *h_totals, int32_t *h_status);
/* launch geometry the library chose for gmk_eval_batch (for profiling reports) */
int gmk_eval_launch_info(int n, int *grid, int *block, int *lds_bytes);
/* for tests and diagnostics only (no caller needs it to evaluate): the 64 lane records of gmk_eval_batch's scan as the host builds and checks them (8 words each; [0] the lines word, [1] the place word: eval_kernel.hip,
 * "Lane -> lines").  Host only: needs neither a device nor gmk_init. */
int gmk_eval_lane_records(uint32_t *records /* 64 * 8 words */);

/* ---- K2: incrementally maintained evaluator states ----
 * One handle = n_games Evaluator objects (core/lib/include/Pattern.h:142-220) living in HBM, 17 792 B each.  Unlike K1 it keeps
 * everything the reference keeps, including the per-cell 2-bit flag words of m_patternDist / m_compoundDist, which are
 * order-dependent shift registers (Pattern.cpp:395-400) and can only be reproduced by replaying the update rule.
 * gmk_evalstate_update applies moves_per_game entries per game in one launch, entry m of game g at d_moves[g*moves_per_game+m]:
 *   >= 0  Evaluator::applyMove(cell)   (Pattern.cpp:310-335; an illegal or post-game move is ignored, as there)
 *   -1    nothing
 *   -2    Evaluator::revertMove(1)     (Pattern.cpp:337-342)
 * gmk_evalstate_read copies the members out: scores int32[n][4][225], density int32[n][2][2][225], pattern_dist uint32[n][226][8]
 * (row 225 = totals), compound_dist uint32[n][226][3], meta int32[n][4] = {moves played, player to move, winner, error bits},
 * record uint8[n][228] (m_moveRecord).  Any pointer may be NULL. */
typedef struct gmk_evalstate gmk_evalstate;
int gmk_evalstate_create(int n_games, gmk_evalstate **out);
int gmk_evalstate_destroy(gmk_evalstate *e);
int gmk_evalstate_reset(gmk_evalstate *e);                                   /* Evaluator::reset (Pattern.cpp:371-386) */
int gmk_evalstate_update(gmk_evalstate *e, const int16_t *d_moves, int moves_per_game, void *stream);
int gmk_evalstate_update_host(gmk_evalstate *e, const int16_t *h_moves, int moves_per_game);
int gmk_evalstate_read(gmk_evalstate *e, int32_t *h_scores, int32_t *h_density, uint32_t *h_pattern_dist, uint32_t *h_compound_dist,
                       int32_t *h_meta, uint8_t *h_record);

/* ---- K3: batched MCTS with the reference's default RandomPolicy ----
 * One handle = n_games independent searches, each with its own tree arena in HBM.  Replaces, per game,
 * Gomoku::MCTS + Policies::RandomPolicy (core/lib/include/MCTS.h:135-180, core/lib/src/MCTS.cpp:99-198,
 * core/lib/include/algorithms/MonteCarlo.hpp:13-110, core/lib/include/policies/Random.h:22-35):
 *   select   argmax_i Q_i + c_puct * P_i * sqrt(N) / (n_i + 1) in double, first maximum wins
 *   expand   one child per empty cell in ascending id, prior 1/float(#empty)
 *   simulate c_rollouts uniform-probe random games (Game.cpp:64-73), value = float(sum / c_rollouts)
 *   backup   visits += 1; value += (v - value) / float(visits); v = -v, up to the root
 * The reference's random_device-seeded mt19937 is replaced by Philox4x32-10 with
 *   key = seed, counter = (global game id, playout index, (stones on the root board << 8) | rollout, ply >> 3);
 *   ply p uses the 16-bit half (p & 1) of output word (p >> 1) & 3, cell draw = (half * 225) >> 16
 * so results do not depend on how games are spread over GPUs.
 * Node capacity per game: at most 225 - stones new nodes per playout; exceeding it sets bit 1 of status. */
typedef struct gmk_mcts gmk_mcts;
int gmk_mcts_create(int n_games, int node_capacity, double c_puct, int c_rollouts, uint64_t seed, gmk_mcts **out);
int gmk_mcts_destroy(gmk_mcts *m);
/* Fresh roots (MCTS::reset + syncWithBoard on a tree without the position, MCTS.cpp:119-125,149-156):
 * h_planes uint16[n][2][16]; h_last_move int16[n] (-1 for an empty board).  first_game_id = global id of game 0. */
int gmk_mcts_set_roots(gmk_mcts *m, const uint16_t *h_planes, const int16_t *h_last_move, uint32_t first_game_id);
/* The global id of every game (uint32[n], host), overriding first_game_id + g of the last gmk_mcts_set_roots: for callers whose
 * handle plays a changing or non-contiguous set of games (slots handed from finished games to new ones, the groups of a match).
 * The id is word 0 of every random-number counter of the game (rollouts, root noise). */
int gmk_mcts_set_game_ids(gmk_mcts *m, const uint32_t *h_ids);
/* MCTS::runPlayouts with the iteration constraint (MCTS.cpp:179-198): `playouts` playouts for every game, one launch. */
int gmk_mcts_run(gmk_mcts *m, int playouts, void *stream);
/* One self-play move for every unfinished game, to be called after gmk_mcts_run (replaces the loop body of
 * agents/utils.py:29-47 around MCTSAgent.eval_state, agents/mcts.py:17-21):
 *   the most visited root child (first maximum: MCTS::stepForward, MCTS.cpp:129-134) is played on the root position,
 *   (move, root child visit counts by cell) is appended to the game record, the game is closed when the move makes
 *   five or fills the board (Board::checkGameEnd, Game.cpp:88-136), and the tree is re-rooted: reuse_subtree = 0
 *   starts the next search from a fresh one-node tree (MCTS::reset), 1 keeps the subtree of the move.
 * Device buffers: d_moves uint8[n][225], d_visits uint16[n][225][225] (may be NULL), d_lens int32[n] (zero before the
 * first move), d_winner int8[n] (valid once the game is over), d_unfinished int32[1] = games still running afterwards.
 * Finished games are skipped by later gmk_mcts_run calls. */
int gmk_mcts_advance(gmk_mcts *m, uint8_t *d_moves, uint16_t *d_visits, int32_t *d_lens, int8_t *d_winner,
                     int32_t *d_unfinished, int reuse_subtree, void *stream);
/* Whole self-play games, resident on the device with CONTINUOUS BATCHING (replaces the data generation loop of
 * network/data_helper.py:58-83 around agents/utils.py:29-63 for MCTS(RandomPolicy) on both sides): the handle's n_games are slots
 * that play n_total games between them.  Every move of the slots is one gmk_mcts_run (`playouts` playouts) and one gmk_mcts_advance;
 * a slot whose game ends takes the next game nobody has started -- its opening becomes the slot's root, its global id
 * first_game_id + index the slot's random-number key -- so the searches stay full until fewer games than slots remain, and game g's
 * record is the same whichever slot played it and however many slots there are.
 * h_open_moves uint8[n_total][open_stride] / h_open_lens int32[n_total]: opening moves per game, black first, 0 .. 8 of them (NULL: empty boards).
 * Device outputs, indexed by GAME: d_moves uint8[n_total][225] (openings included), d_visits uint16[n_total][225][225] or NULL,
 * d_lens int32[n_total], d_winner int8[n_total].  noise_alpha > 0 with reuse_subtree applies Default::AddNoise before every search.
 * ONE persistent launch plays all games (every wavefront searches and steps its slots' games turn by turn at its own pace; with
 * reuse_subtree the chosen child's subtree is compacted into the game's second arena inside the launch) unless the noise has to be drawn
 * on the host (GMK_NOISE_SAMPLER_STD with noise_alpha > 0) or GMK_OPT_LOCKSTEP is set; the records are the same bytes either way.
 * playouts >= 1 (a root that was never searched has no child to play).  A slot whose game can never move -- a node capacity too small for one
 * expansion -- stops and is reported through status bit 1 (arena full) instead of keeping the launch alive.
 * Synchronous; *h_steps (optional) = search launches it took (lock step: each one move for every busy slot; persistent: 1). */
int gmk_selfplay_run(gmk_mcts *m, int n_total, uint32_t first_game_id, int playouts, int reuse_subtree, float noise_alpha, float noise_epsilon,
                     const uint8_t *h_open_moves, int open_stride, const int32_t *h_open_lens,
                     uint8_t *d_moves, uint16_t *d_visits, int32_t *d_lens, int8_t *d_winner, int32_t *h_steps, void *stream);
/* The same step with the move given: MCTS::stepForward(next_move) (core/lib/src/MCTS.cpp:136-147), e.g. the opponent's
 * reply.  d_forced_moves int16[n] (device): the cell to step to, or -1 for the most visited child (= gmk_mcts_advance).
 * A root that was never expanded simply moves on; with reuse_subtree the child's subtree is kept.  An illegal cell
 * sets status bit 2 of that game and plays nothing. */
int gmk_mcts_step(gmk_mcts* m, const int16_t* d_forced_moves, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens,
                  int8_t* d_winner, int32_t* d_unfinished, int reuse_subtree, void* stream);
/* the same from host memory, synchronous, without game records: h_moves int16[n] */
int gmk_mcts_step_host(gmk_mcts* m, const int16_t* h_moves, int reuse_subtree);
/* The two calls a device-resident match makes of a K3 handle (K12, see gmk_match_referee below).
 * gmk_mcts_root_choice: the cell gmk_mcts_step would play with a forced move of -1 -- the most visited root child, first maximum in its
 * order, -1 for a root without a visited child or a finished game -- as d_cells int16[n], and the root children's visit counts by cell
 * saturated at 65 535 as d_visits uint16[n][225] (may be NULL; a finished game's row is zero), both in device memory, on `stream`; nothing
 * is copied to the host.  It reads the arena the game's tree is in now (after a step that kept subtrees: the other one).
 * gmk_mcts_step_device: gmk_mcts_step with the cells read from d_cells and the launch on `stream`, steered by the referee's verdicts
 * d_verdict int32[n] (GMK_MATCH_*): a game that MOVED follows the move, one that ENDED takes the move and is finished (status bit 0: later
 * gmk_mcts_run calls skip it), one that was REFUSED or OVER keeps its tree, its position and its status whatever d_cells holds (-1 is
 * "nothing" here, not "the most visited child").  An illegal cell under MOVED sets status bit 2 and plays nothing.  fresh_root = 0 keeps
 * the subtree as gmk_mcts_step with reuse_subtree does (a move without a child starts a new node); fresh_root != 0 leaves a moved game a
 * one-node root at the position after the move.
 * Both return GMK_ERR_STATE for a handle without roots or one that plays through slots (gmk_selfplay_run). */
int gmk_mcts_root_choice(gmk_mcts* m, int16_t* d_cells, uint16_t* d_visits, void* stream);
int gmk_mcts_step_device(gmk_mcts* m, const int16_t* d_cells, const int32_t* d_verdict, int fresh_root, void* stream);
/* Root noise parameters -- the ONE rule for every entry that takes Default::AddNoise's alpha and epsilon:
 *   gmk_mcts_add_root_noise, gmk_trad_add_root_noise, gmk_az_add_root_noise, gmk_noise_mix_rows:
 *     alpha is finite and > 0, and 0 <= epsilon <= 1 (tested as comparisons, so a NaN is refused).
 *   gmk_selfplay_run, gmk_selfplay_run_sampled, gmk_trad_selfplay_run, gmk_trad_selfplay_run_sampled:
 *     noise_alpha == 0 means "no noise" and noise_epsilon is then ignored; any other noise_alpha follows the rule above.
 * Anything else returns GMK_ERR_ARG with a message that names the argument, before anything is launched and before anything on the handle
 * changes.  (alpha = +inf or epsilon = NaN would make every mixed prior NaN, epsilon > 1 some of them negative, and the searches would go on.)
 * epsilon == 0 leaves the priors as they are; epsilon == 1 leaves none (AddNoise scales the priors by 1 - epsilon FIRST and draws only for the
 * entries that are not 0 then: every entry is masked and ends at 0, in the serial statement too); alpha >= 1 draws without the boost. */
/* Default::AddNoise (MonteCarlo.hpp:97-108, Statistical.hpp:29-34) on every unfinished game whose root has children:
 * P <- (1-epsilon) P + epsilon * normalized(gamma(alpha,1)); the reference calls it at the start of every runPlayouts
 * (MCTS.cpp:182) with alpha 0.05, epsilon 0.25.  No-op for childless (fresh) roots.  The priors stay in force until the
 * next gmk_mcts_advance / gmk_mcts_set_roots.  Synchronises `stream`. */
int gmk_mcts_add_root_noise(gmk_mcts *m, float alpha, float epsilon, void *stream);
/* Handle options (K3 gmk_mcts_set_option, K6 / K8 gmk_trad_set_option).
 * GMK_OPT_NOISE_SAMPLER: where Default::AddNoise draws its gamma variates from (the reference: std::gamma_distribution<float> over a
 *   random_device-seeded std::mt19937, Statistical.hpp:22-34 -- a stream without a seed API, unpinned by construction):
 *     GMK_NOISE_SAMPLER_STD (default)  the toolchain's std::gamma_distribution<float> over std::mt19937, seeded per (game, stones) through
 *                                      Philox; drawn on the HOST, so the self-play loops run in lock step (search, step, noise, search ...);
 *     GMK_NOISE_SAMPLER_COUNTER        the counter-based sampler of include/gomoku_noise.h (Philox-keyed Marsaglia-Tsang, one stream per
 *                                      (game, stones, cell)), drawn by the searching wavefront itself: the reference agent's per-move
 *                                      semantics -- kept subtree + noise before every search -- then run inside ONE persistent launch.
 * GMK_OPT_LOCKSTEP: 1 = gmk_selfplay_run / gmk_trad_selfplay_run alternate search and step launches even where one persistent launch could play
 *   the games (the second form the tests hold the persistent one to); 0 (default) = persistent wherever the configuration allows. */
enum { GMK_OPT_NOISE_SAMPLER = 1, GMK_OPT_LOCKSTEP = 2, GMK_OPT_AZ_LEAVES = 3 /* K7 only: see gmk_az_set_option */,
       GMK_OPT_AZ_VCF_DEPTH = 4, GMK_OPT_AZ_VCF_BUDGET = 5 /* K7 only: see "K7 + K14" */,
       GMK_OPT_AZ_PROOF = 6 /* K7 only: see "K7 + proofs" */,
       GMK_OPT_AZ_VCF_DEFEND = 7 /* K7 only: see "K7 + K15" */ };
#define GMK_AZ_MAX_LEAVES 8
enum { GMK_NOISE_SAMPLER_STD = 0, GMK_NOISE_SAMPLER_COUNTER = 1 };
int gmk_mcts_set_option(gmk_mcts *m, int option, int value);
/* Diagnostic: the mixing of GMK_NOISE_SAMPLER_COUNTER on rows of priors the CALLER supplies -- the device function every search kernel inlines
 * around its own child-to-cell gather, keyed and shaped as a test chooses (tests/test_noise_rows_gpu.py holds it to the serial statement in
 * include/gomoku_noise.h, gmk_noise_mix225, bit for bit).  One wavefront per row; lane l owns the cells l, l + 64, l + 128, l + 192.
 *   d_priors   float[n][225] by cell, mixed IN PLACE; an entry equal to 0 is "no child": it takes no draw and stays 0 (so does an entry that
 *              the scaling by 1 - epsilon rounds to 0)
 *   d_draws    NULL, or float[n][225]: the gamma(alpha, 1) variate of every entry that took a draw, before the normalisation; 0 elsewhere
 *   d_game_ids, d_stones   uint32[n]: words 0 and 1 of row i's counter (the GLOBAL game id and the stones on the root board); seed: the key
 * n >= 0 (0: nothing happens); for n > 0 the pointers other than d_draws are non-null; every pointer is 4-byte aligned; alpha and epsilon as
 * "Root noise parameters" above.  One launch on `stream`; the call does not wait. */
int gmk_noise_mix_rows(float *d_priors, float *d_draws, const uint32_t *d_game_ids, const uint32_t *d_stones,
                       int n, float alpha, float epsilon, uint64_t seed, void *stream);
/* The handle's tree arenas, now: one arena per game (what the first gmk_mcts_set_roots allocates) or, two_arenas != 0, the two arenas per game of
 * the persistent loop with kept subtrees (what gmk_selfplay_run allocates).  Tens of GB, and the driver clears memory it has handed out before
 * (seconds per 24 GB): for callers that want that outside a region they time, or want the blocks in the library's pool before a batch starts
 * (create, reserve, destroy: the next handle of that shape finds them there).  two_arenas != 0 loses the trees, also on a handle that has its
 * two arenas already (a lock-step gmk_mcts_step with reuse_subtree may have left the live trees in the other half): gmk_mcts_run,
 * gmk_mcts_root_stats and the other calls that want roots return GMK_ERR_STATE until the next gmk_mcts_set_roots. */
int gmk_mcts_reserve(gmk_mcts *m, int two_arenas);
/* Root statistics after a run (synchronises the stream used by the last run):
 *   h_visits uint32[n][225] child visit counts by cell (MCTS::evalState, MCTS.cpp:104-110),
 *   h_root_value float[n], h_root_visits uint32[n], h_nodes uint32[n] (MCTS::m_size), h_status int32[n] (bit1: arena full). */
int gmk_mcts_root_stats(gmk_mcts *m, uint32_t *h_visits, float *h_root_value, uint32_t *h_root_visits,
                        uint32_t *h_nodes, int32_t *h_status);
/* algorithmic tree bytes moved by the last run, summed over games (select 8 B/child, expand 16 B/node, backup 16 B/level) */
int gmk_mcts_alg_bytes(gmk_mcts *m, uint64_t *bytes);
int gmk_mcts_launch_info(gmk_mcts *m, int *grid, int *block, int *lds_bytes);
/* pi from visit counts exactly as MCTS::evalState does (MCTS.cpp:112-116, Statistical.hpp:37-42); host side.
 * visits uint32[225], stones = moves on the board (temperature 1 below 15 stones, else 0.01). */
int gmk_visits_to_pi(const uint32_t *visits, int stones, float *pi);

/* ---- K4 + K5: game records -> training tuples, on the device ----
 * Sample s = move d_sample_move[s] of game d_sample_game[s] of the records written by gmk_mcts_advance:
 *   d_states uint8[S][6][225]  Board::encoded_states (core/py_ext/src/game_ext.hpp:87-104) of the position BEFORE that move,
 *   d_values float[S]          Player::calc_score(player to move, winner) (agents/utils.py:55-59),
 *   d_pi     float[S][225]     MCTS::evalState's action probabilities from the recorded visit counts (MCTS.cpp:104-117).
 * augment != 0 writes the eight symmetric copies of every sample (network/data_helper.py:36-55: rot90^i, then fliplr of it):
 * the outputs then hold 8*S samples, copy a of sample s at index 8*s + a.  All pointers are device pointers. */
int gmk_samples_from_records(const uint8_t *d_moves, const int32_t *d_lens, const uint16_t *d_visits, const int8_t *d_winner,
                             const int32_t *d_sample_game, const int32_t *d_sample_move, int n_samples, int augment,
                             uint8_t *d_states, float *d_values, float *d_pi, void *stream);
/* The policy target's mode (K21).  A row written by gmk_az_advance_gumbel / gmk_az_root_choice_gumbel is a distribution, not visit counts:
 *   GMK_TARGET_VISITS  MCTS::evalState's transform of the row, what the entries without `target` compute (their outputs stay bit for bit);
 *   GMK_TARGET_POLICY  pi_c = (float)((double)w_c / (double)sum of w): the sum is an integer below 2^24, so no order of adding enters; a row
 *                      of zeros gives zeros.
 * The mode is a property of the draw, not of the stored bytes: records, the wire form, the replay image and its checkpoints do not change, and
 * a resumed run passes the same mode again.  gmk_samples_from_records_target, gmk_samples_from_packed_target (below) and
 * gmk_replay_sample_target are their plain forms with `target` behind `augment`; any other value is GMK_ERR_ARG, and nothing is launched. */
enum { GMK_TARGET_VISITS = 0, GMK_TARGET_POLICY = 1 };
int gmk_samples_from_records_target(const uint8_t *d_moves, const int32_t *d_lens, const uint16_t *d_visits, const int8_t *d_winner,
                                    const int32_t *d_sample_game, const int32_t *d_sample_move, int n_samples, int augment, int target,
                                    uint8_t *d_states, float *d_values, float *d_pi, void *stream);

/* ---- game records on the wire (the exchange step: selfplay.pack_records / unpack_records, on the device) ----
 * Wire form of n games, one byte block:  lens int32[n] | winner int8[n] | moves uint8[T] | visits uint16[T][225] (optional),
 * T = sum(lens): only the played plies, in game order; the visit section starts at byte 5n + T and is odd-addressed when that is odd.
 * The fixed-stride records are those of gmk_samples_from_records (moves uint8[n][225], visits uint16[n][225][225]).
 * Every launch goes on `stream`; only gmk_records_packed_bytes synchronises (it).  n = 0 is a no-op that returns GMK_OK.
 * gmk_records_scan: d_offsets int64[n+1] = exclusive prefix sum of d_lens, d_offsets[n] = T.  A length outside [0, 225] is not clamped:
 *   d_offsets[n] becomes -1 (and so do the offsets after it).
 * gmk_records_packed_bytes: *h_bytes = 5n + T (1 + 450 has_visits) from d_offsets[n]; GMK_ERR_ARG if a length was outside [0, 225].
 * gmk_records_pack: the bytes of selfplay.pack_records into d_out[0, size) (d_visits NULL = no visit section); d_offsets from
 *   gmk_records_scan of d_lens.  The size is checked on the device: *d_status = GMK_WIRE_BAD_LENGTH or GMK_WIRE_BAD_SIZE (out_bytes
 *   below the wire size), and then nothing is written to d_out; 0 when packed.  Bytes of d_out past the wire size are not touched.
 * gmk_records_unpack: the inverse, d_buf[0, n_bytes) -> the fixed-stride rows of n games.  It writes EVERY byte of those rows -- the
 *   played plies from the block, zeros after a game's length -- so the destination needs no clearing first (selfplay.unpack_records_into
 *   does need it).  d_offsets int64[n+1] is filled as scratch (the scan of the block's lens).  *d_status = GMK_WIRE_BAD_LENGTH or
 *   GMK_WIRE_BAD_SIZE (n_bytes is not the wire size of those lens), and then the records are untouched; 0 when unpacked.
 * gmk_samples_from_packed: K4 + K5 on the wire form (with visits): the same outputs as gmk_samples_from_records on the unpacked
 *   records, for the same sample lists; d_offsets from gmk_records_scan of the block's lens.
 * Alignment: d_lens, d_out, d_buf and d_status 4 bytes, d_offsets 8 bytes, d_visits 2 bytes (GMK_ERR_ARG otherwise). */
enum { GMK_WIRE_BAD_LENGTH = 1, GMK_WIRE_BAD_SIZE = 2 };
int gmk_records_scan(const int32_t *d_lens, int n, int64_t *d_offsets, void *stream);
int gmk_records_packed_bytes(const int64_t *d_offsets, int n, int has_visits, uint64_t *h_bytes, void *stream);
int gmk_records_pack(const uint8_t *d_moves, const int32_t *d_lens, const int8_t *d_winner, const uint16_t *d_visits, int n,
                     const int64_t *d_offsets, uint8_t *d_out, uint64_t out_bytes, int32_t *d_status, void *stream);
int gmk_records_unpack(const uint8_t *d_buf, uint64_t n_bytes, int n, int has_visits, int64_t *d_offsets, uint8_t *d_moves,
                       int32_t *d_lens, int8_t *d_winner, uint16_t *d_visits, int32_t *d_status, void *stream);
int gmk_samples_from_packed(const uint8_t *d_buf, int n, const int64_t *d_offsets, const int32_t *d_sample_game,
                            const int32_t *d_sample_move, int n_samples, int augment, uint8_t *d_states, float *d_values,
                            float *d_pi, void *stream);
int gmk_samples_from_packed_target(const uint8_t *d_buf, int n, const int64_t *d_offsets, const int32_t *d_sample_game,
                                   const int32_t *d_sample_move, int n_samples, int augment, int target, uint8_t *d_states, float *d_values,
                                   float *d_pi, void *stream);

/* ---- replay buffer: game records kept in HBM, training minibatches drawn from them ----
 * Takes the place of DataHelper.buffer + DataHelper.generate_batch (network/data_helper.py:67-83, 97-139).  The handle keeps RECORDS, not
 * tuples: one byte per stored ply, one 450-byte visit row per sampled ply, 32 bytes per game; a minibatch is built from them when it is
 * drawn (K4 + K5 for one sample and one symmetry per wavefront; states, value and pi are the bits gmk_samples_from_records writes).
 * Append and draw are asynchronous on `stream` and make no host round trip; gmk_replay_size and the image calls below synchronise.  One handle serves one
 * stream at a time.  The device memory comes from the library's block pool (gmk_pool_release) and is not cleared.
 *
 * Capacity and eviction.  The buffer holds at most capacity_plies stored plies and max_games games.  An append of n games gives them the
 * serial numbers tail .. tail + n - 1 (tail = games appended since create / reset), then the oldest whole games leave until everything
 * held fits both limits; if the n games alone exceed a limit, the oldest of THEM leave too (the buffer keeps the newest games that fit).
 * The reference trims its list to maxlen BEFORE it extends it (data_helper.py:79-81), so its buffer may overshoot maxlen by one
 * extension; here the capacity is an allocation, so it is hard: the trim comes with the append.
 * first_move (per append): plies below it are stored -- the position before a later ply contains them -- but they are not in the
 * population and carry no visit row; a game with len <= first_move adds nothing to the population.  A length outside [0, 225] sets
 * *d_status = GMK_REPLAY_BAD_LENGTH and appends nothing (no byte of the buffer's state changes); otherwise *d_status = 0.
 * gmk_replay_append reads the fixed-stride records of gmk_samples_from_records, gmk_replay_append_packed a wire block with visits and the
 * d_offsets that gmk_records_scan made of its lens.  An append that brings more games than any before it (and more than
 * min(max_games, 65536)) drains `stream` once and regrows a scratch row; no other append waits for the device.
 *
 * Population order.  P = sampled plies held.  Sampled ply s in [0, P), oldest first: the held games in serial order, within a game the
 * plies first_move .. len - 1.  Without augmentation M = P and sample p is ply p, symmetry 0; with augmentation M = 8 P and sample p is
 * ply p / 8 under symmetry a = p % 8 = 2 k + flip, the numbering of gmk_samples_from_records (np.rot90 k times, then np.fliplr if flip):
 * the tuple is row 8 s + a of that call's augmented output.
 *
 * Draw rule.  Element i of the batch of (seed, step), 0 <= i < batch <= M, is sample perm(i); perm is a bijection of [0, M), so a
 * batch holds distinct samples (random.sample, data_helper.py:137-139).  Let k be the integer with 4^(k-1) < M <= 4^k (k = 0 for M = 1)
 * and mask = 2^k - 1.  E is a balanced Feistel network on 2k-bit numbers x:  L = x >> k, R = x & mask;  four rounds r = 0, 1, 2, 3 of
 *       F = philox4x32_10(counter = {R, r, step & 0xFFFFFFFF, step >> 32}, key = {seed & 0xFFFFFFFF, seed >> 32}).v[0] & mask
 *       (L, R) <- (R, L ^ F)
 * then E(x) = (L << k) | R.  (philox4x32_10 is Philox4x32 with ten rounds, gomokuai_amd/csrc/philox.h; v[0] is its first output word;
 * step is taken as an unsigned 64-bit number.)  perm(i) = E applied to i once, and again while the result is >= M (cycle walking).
 * gmk_replay_draw_host evaluates perm(0 .. batch-1) on the host: it needs no GPU and no gmk_init, and no compute entry uses it.
 *
 * gmk_replay_sample writes the batch: d_states [B][6][225], uint8 (states_float = 0) or float32 0.0 / 1.0 (states_float != 0: what
 * gmk_pvnet_forward and the PyTorch module take), d_values float[B], d_pi float[B][225], and, unless NULL, d_picked int64[B][3] =
 * (game serial, ply, symmetry).  If M < batch, *d_status = GMK_REPLAY_TOO_FEW and no output byte is written; otherwise *d_status = 0.
 * gmk_replay_size: games and stored plies held, population = P (sampled plies held, not multiplied by 8), evicted_games = games that have
 * left or never fitted = the serial of the oldest game held; any of the four pointers may be NULL.  gmk_replay_reset empties the buffer
 * (serials start at 0 again).  GMK_ERR_ARG: a NULL handle or pointer, a misaligned pointer (d_lens, d_buf, d_status and float outputs
 * 4 bytes; d_offsets and d_picked 8; d_visits 2), n < 0, batch < 0, first_move outside [0, 225], capacity_plies outside [225, 2^40],
 * max_games outside [1, capacity_plies]; in gmk_replay_draw_host also batch > population.  n = 0 and batch = 0 are no-ops.
 *
 * The image (checkpoints).  gmk_replay_snapshot writes, and gmk_replay_restore reads, a position-independent byte image of what the handle
 * holds: the same bytes for the same held games, wherever the rings stand and whatever the capacities are.  Little-endian, every section
 * 8-byte aligned:
 *     0  8 bytes   "GMKRPLY1"
 *     8  uint64    n      games held
 *    16  uint64    T      stored plies  = sum len
 *    24  uint64    S      sampled plies = sum max(0, len - first)
 *    32  uint64    head   serial of the oldest game held (= evicted_games)
 *    40  uint64    bytes  size of the whole image
 *    48  uint64 0, uint64 0   (reserved, must be zero)
 *    64  n descriptors, oldest game first, 8 bytes each: uint16 len, uint16 first, int8 winner, three zero bytes
 *    ..  uint8  moves[T], the games back to back, zero bytes up to a multiple of 8
 *    ..  uint16 visits[S][225], in population order, zero bytes up to a multiple of 8
 *   bytes = 64 + 8 n + roundup8(T) + roundup8(450 S); an empty buffer is the 64-byte header.
 * Valid (gomokuai_amd/csrc/replay_image.h, one text for the host and the device): the magic; the reserved words zero; the bytes field
 * equal to the `bytes` argument and to the formula; n <= 2^40 and head <= 2^62; every len <= 225 and every first <= 225; the descriptors'
 * pad bytes zero; the descriptors' sums equal to T and S.  The device checks all of that before it reads a move or a visit row, so a
 * damaged image makes it neither read past `bytes` nor write past the rings; like gmk_replay_append it trusts the move bytes themselves.
 * gmk_replay_image_check_host checks the same and also that every move byte is below 225 and that the sections' padding is zero; it
 * needs no GPU and no gmk_init.  It returns GMK_OK and info = {n, T, S, head, 0} (info may be NULL), or GMK_REPLAY_BAD_IMAGE -- as its
 * return value, the one positive one of this header -- with the broken rule in gmk_last_error.  The winner byte is copied, not judged.
 * gmk_replay_image_bytes: the size of the image of what is held now.
 * gmk_replay_snapshot writes that image to d_image and *d_status = 0; the handle does not change.  If capacity_bytes is too small,
 * *d_status = GMK_REPLAY_NO_ROOM and no byte of d_image is written.
 * gmk_replay_restore replaces whatever the handle holds by the image's games.  They keep their serials head .. head + n - 1: afterwards
 * evicted_games = head, the next append gets serial head + n, and gmk_replay_size, every output of gmk_replay_sample (d_picked included)
 * and which games every later append evicts are those of the handle the image was taken from (the same games leave when the capacities
 * are equal).  Where the games stand in the rings is not kept: they are laid down from the rings' start.  *d_status = GMK_REPLAY_BAD_IMAGE
 * if the image is not valid, else GMK_REPLAY_NO_ROOM if T > capacity_plies or n > max_games, else 0; a refusal changes no byte of the
 * handle's state, descriptors or rings.
 * Synchronisation: gmk_replay_image_bytes, gmk_replay_snapshot and gmk_replay_restore each drain `stream` once (a checkpoint is not a
 * step); snapshot and restore then leave their copies queued on it.  The descriptors go through a kernel each way (restore: one workgroup
 * that validates, takes the prefix sums and writes descriptors and state words last); the plies and the visit rows are one contiguous run
 * of each ring modulo the capacity and move as at most two device-to-device copies each.
 * GMK_ERR_ARG here: a NULL handle or pointer (info excepted), d_image not 8-byte or d_status not 4-byte aligned, bytes < 64,
 * capacity_bytes < 0. */
enum { GMK_REPLAY_BAD_LENGTH = 1, GMK_REPLAY_TOO_FEW = 2, GMK_REPLAY_BAD_IMAGE = 3, GMK_REPLAY_NO_ROOM = 4 };
typedef struct gmk_replay gmk_replay;
int gmk_replay_create(int64_t capacity_plies, int64_t max_games, uint64_t seed, gmk_replay **out);
int gmk_replay_destroy(gmk_replay *h);
int gmk_replay_reset(gmk_replay *h, void *stream);
int gmk_replay_append(gmk_replay *h, const uint8_t *d_moves, const int32_t *d_lens, const int8_t *d_winner, const uint16_t *d_visits,
                      int n, int first_move, int32_t *d_status, void *stream);
int gmk_replay_append_packed(gmk_replay *h, const uint8_t *d_buf, int n, const int64_t *d_offsets, int first_move, int32_t *d_status,
                             void *stream);
int gmk_replay_size(gmk_replay *h, int64_t *games, int64_t *plies, int64_t *population, int64_t *evicted_games, void *stream);
int gmk_replay_sample(gmk_replay *h, int batch, int64_t step, int augment, int states_float, void *d_states, float *d_values, float *d_pi,
                      int64_t *d_picked, int32_t *d_status, void *stream);
/* gmk_replay_sample with the policy target's mode (GMK_TARGET_*, above); GMK_TARGET_VISITS is gmk_replay_sample */
int gmk_replay_sample_target(gmk_replay *h, int batch, int64_t step, int augment, int target, int states_float, void *d_states, float *d_values,
                             float *d_pi, int64_t *d_picked, int32_t *d_status, void *stream);
int gmk_replay_draw_host(uint64_t seed, int64_t step, int64_t population, int64_t batch, int64_t *h_index);
int gmk_replay_image_bytes(gmk_replay *h, int64_t *bytes, void *stream);
int gmk_replay_snapshot(gmk_replay *h, uint8_t *d_image, int64_t capacity_bytes, int32_t *d_status, void *stream);
int gmk_replay_restore(gmk_replay *h, const uint8_t *d_image, int64_t bytes, int32_t *d_status, void *stream);
int gmk_replay_image_check_host(const uint8_t *image, int64_t bytes, int64_t info[5]);

/* ---- K6: pattern-guided tree search, the reference's self-play supervisor ("traditional_mcts", config.py:9-12) ----
 * Replaces MCTS(policy = TraditionalPolicy(c_puct)) : core/lib/include/policies/Traditional.h:17-69 on top of
 * Heuristic (core/lib/include/algorithms/Heuristic.hpp:16-45, 94-200), RAVE::Select / BackPropogate<false>
 * (core/lib/include/algorithms/MonteCarlo.hpp:149-184), Default::Expand (:71-80), MCTS::playout (core/lib/src/MCTS.cpp:158-177).
 * One search per game and launch, every game with its own tree and its own persistent Evaluator (the policy object's
 * m_evaluator): gmk_trad_set_positions = MCTS(c_iterations, last_move, last_player) + Policy::prepare, gmk_trad_run =
 * that many MCTS::playout iterations (further calls continue the same tree), gmk_trad_root_stats = what
 * MCTS::stepForward / evalState read from the root. */
typedef struct gmk_trad gmk_trad;
int gmk_trad_create(int n_games, int node_capacity /* nodes per game, 256 .. 2^24-1 */, gmk_trad** out);
int gmk_trad_destroy(gmk_trad* t);
int gmk_trad_reset_evaluators(gmk_trad* t);                       /* Evaluator::reset for every game */
/* The game each slot of the handle is playing, relative to the first_game_id the noise / PoolRAVE entry points take (uint32[n], host;
 * default: the slot number).  A caller that hands the slot of a finished game to a new one sets the new game's number here, so that
 * the game's random streams (root noise, PoolRAVE rollouts) belong to the GAME, not to the slot it happens to run in. */
int gmk_trad_set_game_ids(gmk_trad* t, const uint32_t* h_ids);
int gmk_trad_set_positions(gmk_trad* t, const uint8_t* h_moves /* [n][225] */, const int32_t* h_lens /* [n]; < 0: this game keeps its position and tree */);
int gmk_trad_run(gmk_trad* t, int playouts, double c_puct, void* stream);
/* host outputs, any may be NULL: per-cell root child visits / values / priors [n][225], the move stepForward() would
 * play (-1 without children), root visits and value, nodes in the tree, status (bit 0 node capacity reached, bit 1
 * evaluator error, bit 2 unsupported board-only revert), evaluator updates (applied + reverted moves) so far */
int gmk_trad_root_stats(gmk_trad* t, uint32_t* h_visits, float* h_values, float* h_priors, int32_t* h_best,
                        uint32_t* h_root_visits, float* h_root_value, int32_t* h_n_nodes, int32_t* h_status,
                        uint64_t* h_evaluator_updates);
/* MCTS::stepForward() / stepForward(move) (core/lib/src/MCTS.cpp:129-147) for every game: h_moves int16[n] = the cell to step
 * to, or -1 for the most visited child (first in the current child order); h_moves == NULL = -1 for all.  The child's
 * subtree is kept (compacted into a second arena), a move without a child starts a new node; the move is appended to the
 * game's position and the next gmk_trad_run synchronises the evaluator (Policy::prepare).  Status bit 3 = not a legal move. */
int gmk_trad_step(gmk_trad* t, const int16_t* h_moves);
/* The two calls a device-resident match makes of a K6 / K8 handle (K12, see gmk_match_referee below).
 * gmk_trad_root_choice: what gmk_trad_root_stats reports as `best` -- the cell MCTS::stepForward() would play, -1 for a root without
 * children -- as d_cells int16[n], and the root children's visit counts by cell saturated at 65 535 as d_visits uint16[n][225] (may be
 * NULL), both in device memory, on `stream`; nothing is copied to the host.
 * gmk_trad_step_device: gmk_trad_step with the cells read from d_cells and the launch on `stream`, steered by the referee's verdicts
 * d_verdict int32[n] (GMK_MATCH_*): a game that MOVED follows the move, one that ENDED takes the move and goes idle (status bit 4: the
 * searches skip it), one that was REFUSED or OVER keeps its tree and status.  fresh_root = 0 keeps the subtree as gmk_trad_step does;
 * fresh_root != 0 leaves a moved game as gmk_trad_set_positions would leave it for the position after the move (a new root at the next search). */
int gmk_trad_root_choice(gmk_trad* t, int16_t* d_cells, uint16_t* d_visits, void* stream);
int gmk_trad_step_device(gmk_trad* t, const int16_t* d_cells, const int32_t* d_verdict, int fresh_root, void* stream);
/* Default::AddNoise on every root with children (the reference does this at the start of every search, MCTS.cpp:182).
 * GMK_NOISE_SAMPLER_COUNTER: one launch on `stream`, behind the search or step that made the root's children; the call does not wait.
 * GMK_NOISE_SAMPLER_STD: the draws are the host's, so the call waits for `stream`, reads the priors back and returns with the new ones
 * written (synchronises `stream` and the device). */
int gmk_trad_add_root_noise(gmk_trad* t, float alpha, float epsilon, uint64_t seed, uint32_t first_game_id, void* stream);
/* TraditionalPolicy(c_puct, use_rave = true) (agents/mcts.py:44-47): gmk_trad_run's playout with RAVE::BackPropogate<true> in place of
 * <false> (MonteCarlo.hpp:113-184).  At every level of the backup each child whose cell the LEAF position holds for the child's player
 * (the root position plus the path; there is no rollout) takes -value into its all-moves-as-first statistics, and the children are ranked
 * by PUCB + the HandSelect-weighted value, (1 - w) Q + w Q_amaf with w = sqrt(800 / (3 n + 800)).  c_bias only reaches RAVE::MinMSE,
 * which the reference leaves unused: no argument.  The first call allocates the handle's AMAF statistics; gmk_trad_root_amaf reads the
 * root children's, and set_positions, step, add_root_noise and root_stats work as for gmk_trad_run.  A handle searches with ONE policy:
 * mixing this call with gmk_trad_run or gmk_trad_run_poolrave on it returns GMK_ERR_STATE, whichever came first. */
int gmk_trad_run_rave(gmk_trad* t, int playouts, double c_puct, void* stream);
/* GMK_OPT_NOISE_SAMPLER / GMK_OPT_LOCKSTEP for a K6 / K8 handle (see gmk_mcts_set_option) */
int gmk_trad_set_option(gmk_trad* t, int option, int value);
/* gmk_mcts_reserve for a K6 / K8 handle (two_arenas = 0: nothing to do, gmk_trad_create allocates the one arena).  The AMAF statistics
 * of a TraditionalPolicy + RAVE handle are left to the run itself (gmk_trad_run_rave, gmk_trad_selfplay_run with policy 2). */
int gmk_trad_reserve(gmk_trad* t, int two_arenas);
/* The self-play loop of the pattern-guided searchers, resident on the device (replaces the host loop of network/data_helper.py:56-83
 * around agents/mcts.py:17-21 for config.py:9-12's supervisor): n_total games (global ids first_game_id ..) are played through the
 * handle's n_games SLOTS with continuous batching -- every move = Default::AddNoise (noise_alpha > 0; MCTS.cpp:182) + one search of
 * `playouts` playouts (policy = 0: TraditionalPolicy as gmk_trad_run, 1: PoolRAVEPolicy as gmk_trad_run_poolrave, 2: TraditionalPolicy
 * with RAVE as gmk_trad_run_rave) + a step kernel
 * that plays MCTS::stepForward()'s choice, checks the end of the game (Game.cpp:88-136) and hands a finished game's slot to the next
 * unstarted game (reuse_subtree = 1 keeps the chosen child's subtree as gmk_trad_step does, 0 starts every search from a new root as
 * gmk_trad_set_positions does).  Records by GAME, on the device: d_moves uint8[n_total][225], d_lens int32[n_total], d_winner
 * int8[n_total], d_visits uint16[n_total][225][225] (may be NULL).  h_open_moves / h_open_lens: the games' openings, or NULL.
 * persistent = 1 (TraditionalPolicy with or without RAVE, whole games): ONE launch in which every slot's wavefront plays game after game at its own pace -- a
 * search no longer waits for the slowest one of the batch -- taking the next unstarted game from a counter when its game ends; a game then
 * starts on a fresh evaluator (Evaluator::reset), so its record does not depend on the slot it landed in and equals the one the
 * all-games-at-once loop plays.  With reuse_subtree the chosen child's subtree is compacted into the slot's second arena inside the launch
 * (MCTS::stepForward, MCTS.cpp:129-134); root noise inside the launch is drawn by the wavefront from the counter-based sampler
 * (gmk_trad_set_option(GMK_OPT_NOISE_SAMPLER, GMK_NOISE_SAMPLER_COUNTER); with the host-drawn std sampler the call is refused).
 * persistent = 0, or GMK_OPT_LOCKSTEP: the lock-step loop described above (a slot's evaluator carries over from game to game, as the
 * reference's policy object does within a worker).
 * max_steps > 0 ends the loop after that many moves per slot (games still running keep the moves they have, winner 0): what a
 * throughput measurement with every slot busy needs; 0 = play every game to its end.
 * *h_overflow != 0: some search stopped at its node capacity.  Afterwards the handle must be positioned again before other use. */
int gmk_trad_selfplay_run(gmk_trad* t, int policy, int n_total, uint32_t first_game_id, int playouts, double c_puct, uint64_t seed,
                          int reuse_subtree, float noise_alpha, float noise_epsilon,
                          const uint8_t* h_open_moves, int open_stride, const int32_t* h_open_lens,
                          uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int persistent, int max_steps, int32_t* h_overflow, int32_t* h_steps, void* stream);
/* the games' evaluator states, laid out as gmk_evalstate_read */
int gmk_trad_read_evaluators(gmk_trad* t, int32_t* h_scores, int32_t* h_density, uint32_t* h_pattern_dist,
                             uint32_t* h_compound_dist, int32_t* h_meta, uint8_t* h_record);

/* ---- K8: PoolRAVE tree search on the K6 handle ----
 * Replaces MCTS(policy = PoolRAVEPolicy(c_puct, c_bias)) : core/lib/include/policies/PoolRAVE.h:7-52 = RAVE::Select,
 * Default::Expand with AMAFNodes, one Default::RandomRollout per playout that stays on the board, and
 * RAVE::BackPropogate<true> (core/lib/include/algorithms/MonteCarlo.hpp:113-184).  The tree is the one of K6: create,
 * set_positions, step, add_root_noise and root_stats are the gmk_trad_* entry points above (the handle's evaluators are
 * not used); this call runs `playouts` MCTS::playout iterations per game with PoolRAVE's stages.  Rollout draws: Philox4x32-10,
 * key = seed, counter = (first_game_id + game, playout since the root last changed, stones on the root board << 8, ply >> 3),
 * as K3 with rollout number 0.  c_bias only reaches RAVE::MinMSE, which the reference leaves unused (:130-139): no argument.
 * A handle searches with ONE policy: mixing gmk_trad_run, gmk_trad_run_rave and gmk_trad_run_poolrave on it returns GMK_ERR_STATE. */
int gmk_trad_run_poolrave(gmk_trad* t, int playouts, double c_puct, uint64_t seed, uint32_t first_game_id, void* stream);
/* the root children's all-moves-as-first statistics by cell (AMAFNode::amaf_visits / amaf_value), host [n][225] each (K8 and
 * gmk_trad_run_rave handles) */
int gmk_trad_root_amaf(gmk_trad* t, uint32_t* h_amaf_visits, float* h_amaf_values);

/* ---- K7: network-guided tree search, many games in lock step (BASELINE.json configs[4]) ----
 * Replaces MCTS(policy = Policy(eval_state = network.eval_state, c_puct)) (agents/alphazero.py:5-9): Default::Select
 * (core/lib/include/algorithms/MonteCarlo.hpp:57-68), the evaluator call at a new leaf (core/lib/src/MCTS.cpp:164-168),
 * Default::Expand with extraCheck = true (:71-80), Default::BackPropogate (:90-95).  One playout of every game =
 * gmk_az_select (writes the leaves' Board.encoded_states planes, core/py_ext/src/game_ext.hpp:87-104, as float32
 * [n][6][15][15]; games that are over at the leaf are backed up at once and get a zero row), the caller's network on that
 * batch, gmk_az_expand with its value [n] and probabilities [n][225] (device pointers, same stream).
 * The batch holds the games that are still PLAYED, in slot order: n = gmk_az_live_games, which is n_games until gmk_az_advance ends a
 * game (or gmk_az_set_slots leaves slots idle); a finished game has no row, so the network's work follows the live games. */
typedef struct gmk_az gmk_az;
int gmk_az_create(int n_games, int node_capacity, double c_puct, gmk_az** out);
int gmk_az_destroy(gmk_az* a);
/* fresh roots; h_planes uint16[n][2][16] as gmk_eval_batch, h_last_moves int16[n][2] = {last move, the one before} or -1 */
int gmk_az_set_roots(gmk_az* a, const uint16_t* h_planes, const int16_t* h_last_moves);
int gmk_az_live_games(gmk_az* a, int32_t* n_live);            /* rows of the leaf batch; changed by gmk_az_set_roots / _set_slots / _advance only */
int gmk_az_select(gmk_az* a, float* d_states, void* stream);
int gmk_az_expand(gmk_az* a, const float* d_values, const float* d_probs, void* stream);
/* MCTS::stepForward() / stepForward(move) (core/lib/src/MCTS.cpp:129-147) for every game, subtree kept (as gmk_trad_step): h_moves
 * int16[n] = the cell to step to, -1 = the most visited child, NULL = -1 for all; status bit 2 = not a legal move. */
int gmk_az_step(gmk_az* a, const int16_t* h_moves);
/* The two calls a device-resident match makes of a K7 handle (K12, see gmk_match_referee below).
 * gmk_az_root_choice: the most visited root child, first maximum in cell order as gmk_az_advance picks it (-1: no visited child), as
 * d_cells int16[n], and the root children's visit counts by cell saturated at 65 535 as d_visits uint16[n][225] (may be NULL), both in
 * device memory, on `stream`; nothing is copied to the host.
 * gmk_az_step_device: gmk_az_step with the cells read from d_cells and the launch on `stream`, steered by the referee's verdicts
 * d_verdict int32[n] (GMK_MATCH_*): a game that MOVED follows the move, one that ENDED is closed as gmk_az_advance closes one (status
 * bit 0; the leaf batch is compacted, so gmk_az_live_games drops), one that was REFUSED or OVER keeps its tree and status.  fresh_root = 0
 * keeps the subtree as gmk_az_step does; fresh_root != 0 makes the root gmk_az_set_roots makes for the position after the move.
 * The call waits for the stream once, for the number of live games; with h_unfinished it brings the referee's count d_unfinished
 * (int32[1], device) along in the same wait -- the four bytes the host sees of a match ply. */
int gmk_az_root_choice(gmk_az* a, int16_t* d_cells, uint16_t* d_visits, void* stream);
int gmk_az_step_device(gmk_az* a, const int16_t* d_cells, const int32_t* d_verdict, int fresh_root, const int32_t* d_unfinished, int32_t* h_unfinished,
                       void* stream);
/* One self-play move for every game still played, on the device (replaces the per-ply host work of the reference's self-play loop,
 * network/data_helper.py:56-83 with agents/alphazero.py:5-9 on both sides, as gmk_mcts_advance does for K3): the most visited child of
 * the root (first maximum in cell order, MCTS.cpp:129-134) is appended to the game's record with the root's visit counts, played on the
 * root position with Board::applyMove's victory check (Game.cpp:37-49, 88-136), and the tree is re-rooted (reuse_subtree: the child's
 * subtree is kept as gmk_az_step keeps it; otherwise a new root).  A root without a visited child ends its game where it stands.
 * Finished games (status bit 0) are skipped by gmk_az_select / gmk_az_expand from then on.
 * Records on the device, row g = game g: d_moves uint8[n][225] and d_lens int32[n] must hold the moves that led to the roots (the
 * openings), d_winner int8[n] zero; d_visits uint16[n][225][225] may be NULL.  h_unfinished: the games that go on.  Synchronises `stream`. */
/* Continuous batching for whole-game self-play (as gmk_selfplay_run / gmk_trad_selfplay_run have it): the handle's n_games slots play
 * n_total games between them.  This call takes gmk_az_set_roots's place: the first min(n_games, n_total) games start in the slots from
 * their openings (h_open_moves uint8[n_total][open_stride], h_open_lens int32[n_total], at most 8 moves each; NULL: empty boards);
 * gmk_az_advance then writes a slot's move to the record rows of the GAME it plays (rows = n_total) and hands a finished game's slot to
 * the next unstarted game; gmk_az_add_root_noise keys a slot's draws by that game.  gmk_az_set_roots ends the mode. */
int gmk_az_set_slots(gmk_az* a, int n_total, const uint8_t* h_open_moves, int open_stride, const int32_t* h_open_lens);
int gmk_az_advance(gmk_az* a, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int reuse_subtree, int32_t* h_unfinished,
                   void* stream);
/* Default::AddNoise on every root with children (core/lib/include/algorithms/MonteCarlo.hpp:97-108); the random stream of slot g is keyed
 * by first_game_id + ids[g], ids as set by gmk_az_set_game_ids (uint32[n], host; default: the slot number; the call waits for the device
 * and uploads them).
 * GMK_NOISE_SAMPLER_COUNTER: one launch on `stream`, behind the gmk_az_expand / gmk_az_advance that made the root's children and before
 * the next gmk_az_select on it; the call does not wait.  GMK_NOISE_SAMPLER_STD: the draws are the host's, so the call waits for `stream`,
 * reads the priors back and returns with the new ones written (synchronises `stream` and the device). */
int gmk_az_set_game_ids(gmk_az* a, const uint32_t* h_ids);
int gmk_az_add_root_noise(gmk_az* a, float alpha, float epsilon, uint64_t seed, uint32_t first_game_id, void* stream);
/* GMK_OPT_NOISE_SAMPLER for a K7 handle (see gmk_mcts_set_option): GMK_NOISE_SAMPLER_COUNTER draws the noise on the device, one wavefront per game.
 * GMK_OPT_AZ_LEAVES = L in 1 .. GMK_AZ_MAX_LEAVES (GMK_ERR_ARG otherwise; default 1): leaves per game per step, with virtual loss.
 *   L = 1: gmk_az_select / gmk_az_expand are the one-leaf kernels, one playout per step.
 *   L > 1: every game owes a quota of playouts (gmk_az_add_playouts).  gmk_az_select makes min(L, quota) descents per game, one after the
 *   other; each counts the descents still in flight below a node as lost playouts (per child: mean (Q N - v) / (N + v), count N + v + 1,
 *   parent count N + v under the square root, in double), so that they spread.  A descent that ends at a finished game is backed up at once;
 *   one that reaches a leaf already waiting for the network ends the game's descents for this step and is not counted; any other marks its
 *   path, becomes the game's k-th pending leaf and takes one off the quota.  d_states, d_values and d_probs then have
 *   gmk_az_live_games x L rows: game g's k-th leaf is row row(g) * L + k, rows past the game's pending leaves are zeros on the way out and
 *   ignored on the way in.  gmk_az_expand answers the pending leaves in that order and takes the marks back; a leaf whose children do not
 *   fit the arena sets status bit 1 and its playout is dropped.  Neither call waits for the host: a step can be captured in a hipGraph.
 *   The first L > 1 allocates two bytes per node and 640 bytes per game.  Between a gmk_az_select and its gmk_az_expand the marks are up:
 *   gmk_az_select, gmk_az_step, gmk_az_step_device, gmk_az_advance, gmk_az_add_root_noise and gmk_az_set_option return GMK_ERR_STATE then.
 *   The host-driven entries below (one game behind a Python evaluator) return GMK_ERR_STATE on a handle whose L > 1.
 * gmk_az_add_playouts: every game that is not over owes `playouts` more (finished games keep 0); gmk_az_set_roots and gmk_az_set_slots
 *   reset the quota, the pending leaves and the marks, and a slot refilled by gmk_az_advance starts with 0.
 * gmk_az_playouts_owed: *h_max = the largest quota over the handle; synchronises `stream`.  A game that owes playouts completes at least
 *   one per step, so `playouts` steps always suffice and about playouts / L do. */
int gmk_az_set_option(gmk_az* a, int option, int value);
int gmk_az_add_playouts(gmk_az* a, int playouts, void* stream);
int gmk_az_playouts_owed(gmk_az* a, int32_t* h_max, void* stream);
/* The same two steps for an evaluator that runs on the host and wants positions, not planes (the Python callable of
 * Policy(eval_state=...)): select, then the moves from the root to every pending leaf (h_paths int16[n][226], h_lens int32[n],
 * -1 = nothing to evaluate); expand from host memory.  Synchronous. */
int gmk_az_select_host(gmk_az* a, int16_t* h_paths, int32_t* h_lens);
int gmk_az_expand_host(gmk_az* a, const float* h_values, const float* h_probs);
/* Host-driven STAGES: `Policy(select=, expand=, eval_state=, back_prop=)` hands Python callables to the four stages of
 * MCTS::playout (core/py_ext/src/mcts_ext.hpp:43-61, core/lib/include/MCTS.h:74-101).  The callables run on the host; the tree stays on the
 * device, and the host reads what it is asked about and tells the device what was decided.  One game (`game`) of the handle; synchronous.
 *   gmk_az_read_node_host / _read_children_host   a node (visits, value, prior, cell, parent, child range) and the nodes of a child range
 *   gmk_az_set_leaf_host            the leaf a host-side descent ended at (node, the moves from the root): it becomes the pending leaf
 *   gmk_az_rollout_host             Default::Simulate's random rollout (MonteCarlo.hpp:37-47, 83-88) from the pending leaf, on the device;
 *                                   counters (global game id, playout number, root stones << 8) = the draws of gmk_mcts_*'s first rollout
 *   gmk_az_expand_stages_host       gmk_az_expand_host with Default::Expand and Default::BackPropogate switched separately
 *   gmk_az_write_stats_host         {visits, value} of nodes as a Python back_prop left them */
int gmk_az_read_node_host(gmk_az* a, int game, uint32_t node, uint32_t* h_visits, float* h_value, float* h_prior, int32_t* h_cell, uint32_t* h_parent,
                          uint32_t* h_first_child, int32_t* h_n_children);
int gmk_az_read_children_host(gmk_az* a, int game, uint32_t first_child, int n, int16_t* h_cells, uint32_t* h_visits, float* h_values, float* h_priors,
                              int32_t* h_n_children);
int gmk_az_set_leaf_host(gmk_az* a, int game, uint32_t leaf, const int16_t* h_path, int depth);
int gmk_az_rollout_host(gmk_az* a, int game, uint64_t seed, uint32_t counter0, uint32_t counter1, uint32_t counter2, int32_t* h_winner);
int gmk_az_expand_stages_host(gmk_az* a, const float* h_values, const float* h_probs, int do_expand, int do_backup);
int gmk_az_write_stats_host(gmk_az* a, int game, const uint32_t* h_nodes, const uint32_t* h_visits, const float* h_values, int n);
/* host outputs, any may be NULL; status bit 0 = the game is over (gmk_az_advance), bit 1 = node arena full (playouts of that game were dropped) */
int gmk_az_root_stats(gmk_az* a, uint32_t* h_visits, float* h_values, float* h_priors, uint32_t* h_root_visits,
                      float* h_root_value, int32_t* h_n_nodes, int32_t* h_status);
/* ---- K7 + K14: forced wins by fours solved at the leaves of the network search (az_vcf_leaves_kernel) ----
 * Two options of gmk_az_set_option:
 *   GMK_OPT_AZ_VCF_DEPTH  = D in 0 .. GMK_VCF_MAX_DEPTH, default 0 = off
 *   GMK_OPT_AZ_VCF_BUDGET = B in 1 .. 2^20, default 64 (not tuned; DESIGN.md K16 has the timing table)
 * GMK_ERR_ARG outside these ranges; GMK_ERR_STATE while a gmk_az_select waits for its gmk_az_expand.  The first D > 0 allocates the verdict
 * buffer, 16 bytes x n_games x GMK_AZ_MAX_LEAVES.  With D = 0 every entry launches exactly the kernels it launches without this block.
 * With D > 0 a step is the same step with another evaluator.  For every pending leaf -- its stones and its side to move, white when the
 * leaf's stone count is odd -- gmk_az_select computes, in a kernel of its own right behind the select kernel on the same stream,
 *     r = K14's walk (below, "K14") on that position, max_depth = D, budget = B, plain mode (flags 0), the side to move attacks
 * and gmk_az_expand answers the leaf
 *     r.status == GMK_VCF_WIN     as if the network had returned value = +1.0f and probs = one-hot(r.move): one child, cell pv[0], prior 1.0f,
 *                                 and -1.0f is backed up
 *     NONE, DEPTH, BUDGET, OVER   from its row of d_values / d_probs, unchanged
 * so the search equals the search with the evaluator E'(pos) = WIN ? (1, one-hot) : E(pos), bit for bit.  Default::Expand's legality check, the
 * arena-full rule (status bit 1, the playout dropped), virtual loss, quota and the order of the pending leaves are as they are.  Terminal
 * leaves, collided descents and rows k >= n_pending have no leaf and are not solved.  d_values and d_probs are read, never written.  Nothing
 * waits for the host: a captured step stays one chain of kernels.
 * Per game the handle counts the leaves solved, those answered WIN, those cut by BUDGET or DEPTH, and the nodes the walks counted;
 * gmk_az_set_roots and gmk_az_set_slots clear the counters (a slot refilled by gmk_az_advance keeps them: they belong to the slot).
 * gmk_az_vcf_stats: the counters, per-game host arrays uint32[n_games] x 3 and uint64[n_games]; any pointer may be NULL.  Synchronises.
 * gmk_az_vcf_verdicts_host: the verdicts of the last gmk_az_select for the gmk_az_live_games x L rows of the leaf batch: status, move, length
 *   (int32 each) and nodes (uint32), as gmk_vcf_solve writes them; a row without a pending leaf reads GMK_VCF_NONE / -1 / 0 / 0.
 *   GMK_ERR_STATE when D = 0.  Synchronises.
 * The host-driven one-leaf entries gmk_az_select_host, gmk_az_expand_host, gmk_az_set_leaf_host and gmk_az_expand_stages_host return
 * GMK_ERR_STATE on a handle whose D > 0, as they do when L > 1. */
int gmk_az_vcf_stats(gmk_az* a, uint32_t* h_leaves, uint32_t* h_wins, uint32_t* h_cut, uint64_t* h_nodes);
int gmk_az_vcf_verdicts_host(gmk_az* a, int32_t* h_status, int32_t* h_move, int32_t* h_length, uint32_t* h_nodes);
/* ---- K7 + proofs: proven wins and losses carried up the tree (MCTS-Solver, Winands et al. 2008) ----
 * GMK_OPT_AZ_PROOF of gmk_az_set_option: 0 (default) or 1, anything else GMK_ERR_ARG; GMK_ERR_STATE while the marks are up (L > 1) or a
 * gmk_az_select waits for its gmk_az_expand.  With 0 every entry launches exactly the kernels it launches without this block.
 * A node carries a proof in bits 16..17 of its child word (no memory of its own; the bits travel through re-rooting with the word):
 *     GMK_AZ_PROOF_NONE  = 0   no proof
 *     GMK_AZ_PROOF_WINS  = 1   the side to move at the node has a forced win
 *     GMK_AZ_PROOF_LOSES = 2   the side to move at the node loses against every move
 * A node whose last stone completed a five is LOSES.  A full board is not a proof.  Switching the option off leaves the bits where they are and
 * the off-path ignores them; they are facts about positions, so switching it on again may use them.  gmk_az_set_roots, gmk_az_set_slots, a slot
 * refilled by gmk_az_advance and every fresh root start with NONE.
 * prove(X, s), run by the game's own wavefront; stones(X) = the stone count of X's position:
 *     1. if X already has a proof, stop          2. proof(X) = s, and the game's `proved` counter + 1
 *     3. P = X's parent; none: stop              4. s == LOSES: prove(P, WINS)
 *     5. s == WINS: prove(P, LOSES) only when children(P) == 225 - stones(P) (Default::Expand dropped no free cell for a zero probability)
 *        and every child of P is WINS; otherwise stop
 * Proofs start (a) in gmk_az_select, at a descent that ends at a terminal node with a five: prove(node, LOSES), the +1 backed up as before;
 * (b) in gmk_az_expand, at a pending leaf whose "K7 + K14" verdict is WIN and whose child was created (not dropped by a full arena):
 * prove(leaf, WINS), the -1.0f backup and the one-hot child as before.  (b) needs GMK_OPT_AZ_VCF_DEPTH > 0; without it only (a) starts proofs.
 * Descent (every descent of a step, any L).  On arriving at a node that is not the root and has a proof, before its children are read, the
 * descent ends: +1.0f is backed up from it for LOSES, -1.0f for WINS, and the game's `stops` counter + 1.  With L > 1 this is the "game is
 * over at the leaf" case (quota - 1, no mark, no row, no collision test); with L = 1 nothing is pending and the game's row is zeros.  The root
 * always descends.  Among the children of a node: if any is LOSES the first such in child order (ascending cell) is taken; otherwise children
 * marked WINS are left out of the PUCB maximum unless all are marked, then none is.  The expression, the double arithmetic, the strict '>' from
 * -1.0 (nothing beats it: the first child, marked or not) and the virtual-loss terms are as they are.
 * Root choice (gmk_az_advance, gmk_az_root_choice, and gmk_az_step for a game whose move is not forced; gmk_az_step_device chooses nothing):
 *     1. the first child marked LOSES, if there is one
 *     2. otherwise the most visited child among those not marked WINS that have at least one visit, first maximum in cell order
 *     3. otherwise the old rule
 * The recorded visit rows and gmk_az_root_stats are the raw counts, unchanged.
 * gmk_az_root_proofs: the root's proof int8[n_games] and its children's by cell int8[n_games][225], 0 where there is no child; either may be
 *   NULL.  gmk_az_proof_stats: per game, uint32[n_games] each, either may be NULL: nodes given a proof, and descents ended at a node already
 *   proven; cleared where the "K7 + K14" counters are cleared.  Both synchronise.
 * The host-driven one-leaf entries that refuse a handle whose D > 0 refuse one whose GMK_OPT_AZ_PROOF is 1 in the same way. */
enum { GMK_AZ_PROOF_NONE = 0, GMK_AZ_PROOF_WINS = 1, GMK_AZ_PROOF_LOSES = 2 };
int gmk_az_root_proofs(gmk_az* a, int8_t* h_root, int8_t* h_children);
int gmk_az_proof_stats(gmk_az* a, uint32_t* h_proved, uint32_t* h_stops);
/* ---- K7 + K15: the replies that lose to a forced win by fours, proven at the leaves of the network search ----
 * GMK_OPT_AZ_VCF_DEFEND of gmk_az_set_option: 0 (default) or 1, anything else GMK_ERR_ARG; GMK_ERR_STATE in the states in which options 4 to 6
 * are refused (the marks are up, or a gmk_az_select waits for its gmk_az_expand).  The option ACTS only on a handle that also has
 * GMK_OPT_AZ_VCF_DEPTH = D > 0 and GMK_OPT_AZ_PROOF = 1; with either of them off it is accepted and inert: every entry launches exactly the
 * kernels it launches without this block and the search is bit for bit that handle's without the option.  The option call that makes it act
 * for the first time allocates, per row of the largest leaf batch (n_games x GMK_AZ_MAX_LEAVES), 16 + GMK_VCF_PV + 32 + 900 bytes; nothing is
 * allocated inside a step.  If that allocation fails the call returns GMK_ERR_HIP and the block stays inert.
 * While it acts, gmk_az_select computes for every pending leaf P whose "K7 + K14" verdict is neither WIN nor OVER, in two more kernels behind
 * that block's on the same stream (one linear chain):
 *   1. threat = K14's walk on P with the side that is NOT to move attacking (GMK_VCF_OPPONENT), plain mode, max_depth = D, budget = B, the
 *      handle's "K7 + K14" settings; its principal variation is kept.
 *   2. threat.status == GMK_VCF_WIN: for every cell c the verdict of "K15"'s table (below) in plain mode for P: occupied NONE; otherwise
 *      follow(0) against the threat's pv with a stone of the side to move on c, and only on FAIL solve(P + [c]) with the whole budget B.
 *      GMK_VCF_CELL_FIVE cannot occur: a leaf with a completing cell of its own is a "K7 + K14" WIN (K14 answers it before any limit).
 *   3. Any other threat status (NONE, DEPTH, BUDGET) marks nothing.
 * The threat and the table equal gmk_vcf_defend's for the leaf's move list with (D, B, flags 0), bit for bit: threat status and length, and
 * verdict and nodes per cell.
 * gmk_az_expand then, for such a leaf under a WIN threat, once its children exist and unless the playout was dropped for a full arena:
 *   every child whose cell is GMK_VCF_CELL_LOSES gets GMK_AZ_PROOF_WINS -- the opponent, to move there, has a forced win.  The bit is written
 *   with the child's word, not through prove: one WINS child proves nothing about its parent.  Each such child counts once in `proved`.
 *   If the leaf has a child for every free cell (children == 225 - stones) and every child is now WINS: prove(leaf, GMK_AZ_PROOF_LOSES), which
 *   climbs by "K7 + proofs"'s rule, and +1.0f is backed up from the leaf in place of -value.
 *   Otherwise the network's value and row are used as they are.  Priors are never changed: the descent already leaves WINS children out of
 *   the maximum and stops at a marked child without a network row.
 * A dropped leaf gets no mark and counts nowhere.  Virtual loss, quota, the order of the pending leaves, d_values and d_probs are untouched.
 * Everything is exact integer work: no float, no atomics; a captured step stays one chain of kernels.
 * gmk_az_defend_stats: per game, uint32[n_games] x 3 and uint64[n_games], any pointer may be NULL: the leaves expanded under a WIN threat, the
 *   children marked, the cells solved in full (step 2's solve) and the nodes of those solves; cleared where the "K7 + K14" counters are
 *   cleared.  Synchronises.
 * gmk_az_defend_verdicts_host: for the gmk_az_live_games x L rows of the last gmk_az_select: h_threat_status int32[rows], h_threat_length
 *   int32[rows], h_verdict int8[rows][225] (GMK_VCF_CELL_*), h_nodes uint32[rows][225]; any pointer may be NULL.  A row without a pending leaf,
 *   or whose "K7 + K14" verdict is WIN or OVER, reads threat NONE, length 0 and all-zero cells; a pending leaf whose threat is NONE reads HOLDS
 *   on its free cells, one whose threat is DEPTH or BUDGET reads UNKNOWN there, as K15's table has them.  GMK_ERR_STATE unless the option
 *   acts.  Synchronises.
 * The host-driven one-leaf entries that refuse a handle whose D > 0 refuse one whose GMK_OPT_AZ_VCF_DEFEND is 1 in the same way. */
int gmk_az_defend_stats(gmk_az* a, uint32_t* h_threatened, uint32_t* h_marked, uint32_t* h_searched, uint64_t* h_nodes);
int gmk_az_defend_verdicts_host(gmk_az* a, int32_t* h_threat_status, int32_t* h_threat_length, int8_t* h_verdict, uint32_t* h_nodes);
/* ---- K20: self-play moves drawn from the root's visit counts, on the device ----
 * The rule is stated once, in gomoku_sample.h: a root with fewer than sample_plies stones (openings included) plays child i with probability
 * w_i / T, w_i = min(visits_i, 65535)^sample_power, through one draw of the counter-based stream keyed by (seed; global game id, stones,
 * 'samp'); with GMK_OPT_AZ_PROOF the first child marked LOSES is played without a draw and children marked WINS weigh nothing; a root with
 * sample_plies stones or more, or without weight, plays what gmk_az_advance plays.  sample_power 1, 2, 3 is temperature 1, 1/2, 1/3.
 * The global game id of slot g is first_game_id + what gmk_az_add_root_noise's counter sampler uses: the game the slot plays under
 * gmk_az_set_slots, otherwise ids[g] of gmk_az_set_game_ids (default g).
 * gmk_az_advance_sampled / gmk_az_root_choice_sampled: gmk_az_advance / gmk_az_root_choice with that choice; everything else (records, visit
 *   rows, re-rooting, the synchronisation of gmk_az_advance) is theirs, and so is GMK_ERR_STATE.  One launch on `stream`, nothing on any other.
 *   sample_plies outside 0 .. 225 or sample_power outside 1 .. 3: GMK_ERR_ARG, and nothing is launched.  sample_plies = 0 launches exactly the
 *   kernel the unsampled entry launches.
 * gmk_move_sample_host: the rule for n roots given by rows, on the host (no GPU, no gmk_init): h_visits uint32[n][225] by cell, not saturated
 *   (gmk_az_root_stats' visits), h_proofs int8[n][225] (gmk_az_root_proofs' children) or NULL, h_stones int32[n] in 0 .. 225, h_game_ids
 *   uint32[n] GLOBAL ids; h_cells int16[n], -1 for a root that has nothing to play.  It equals the device entries cell for cell.
 * K3 and K6 / K8 (the searches whose games bootstrap the training loop) draw by the same rule, without proofs, from the root's visit counts BY CELL:
 * gmk_mcts_advance_sampled / gmk_selfplay_run_sampled: gmk_mcts_advance / gmk_selfplay_run with that choice, keyed by the HANDLE's seed
 *   (gmk_mcts_create) and the game's global id (first_game_id + index, or gmk_mcts_set_game_ids); a ply at or past sample_plies, or a root
 *   without weight, plays gmk_mcts_advance's first maximum in cell order.  The persistent launch, GMK_OPT_LOCKSTEP and the host-drawn noise
 *   sampler play the same games.
 * gmk_trad_selfplay_run_sampled: gmk_trad_selfplay_run with that choice for all three policies, keyed by that call's seed and first_game_id,
 *   in the persistent launch and in the lock-step loop alike; gmk_trad_root_choice_sampled: gmk_trad_root_choice with it, the game of slot g
 *   being first_game_id + ids[g] of gmk_trad_set_game_ids (default g) and its stones the length of its position.  A ply at or past
 *   sample_plies, or a root without weight, plays MCTS::stepForward()'s choice as before: the most visited child, among equals the first in
 *   the CURRENT child order (not gmk_sample_greedy225's first in cell order).
 *   All four: sample_plies outside 0 .. 225 or sample_power outside 1 .. 3 is GMK_ERR_ARG, nothing is launched and the handle stays usable;
 *   sample_plies = 0 launches exactly the kernels of the unsampled entry.  The two run entries are synchronous like their unsampled forms; the
 *   other two are one launch on `stream`.
 * Not sampled: gmk_mcts_step with forced moves, gmk_trad_step, gmk_az_step, the ensembles (gmk_*_ensemble_merge) and evaluation matches, which play
 * the most visited child; the policy target (gmk_visits_to_pi) is unchanged. */
int gmk_az_advance_sampled(gmk_az* a, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int reuse_subtree,
                           int sample_plies, int sample_power, uint64_t seed, uint32_t first_game_id, int32_t* h_unfinished, void* stream);
int gmk_az_root_choice_sampled(gmk_az* a, int16_t* d_cells, uint16_t* d_visits, int sample_plies, int sample_power,
                               uint64_t seed, uint32_t first_game_id, void* stream);
int gmk_move_sample_host(const uint32_t* h_visits /*[n][225], unsaturated*/, const int8_t* h_proofs /*[n][225] or NULL*/,
                         const int32_t* h_stones, const uint32_t* h_game_ids /* already global */, int n,
                         int sample_plies, int sample_power, uint64_t seed, int16_t* h_cells /* -1: none */);
int gmk_mcts_advance_sampled(gmk_mcts* m, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int32_t* d_unfinished, int reuse_subtree,
                             int sample_plies, int sample_power, void* stream);
int gmk_selfplay_run_sampled(gmk_mcts* m, int n_total, uint32_t first_game_id, int playouts, int reuse_subtree, float noise_alpha, float noise_epsilon,
                             int sample_plies, int sample_power, const uint8_t* h_open_moves, int open_stride, const int32_t* h_open_lens,
                             uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int32_t* h_steps, void* stream);
int gmk_trad_selfplay_run_sampled(gmk_trad* t, int policy, int n_total, uint32_t first_game_id, int playouts, double c_puct, uint64_t seed,
                                  int reuse_subtree, float noise_alpha, float noise_epsilon, int sample_plies, int sample_power,
                                  const uint8_t* h_open_moves, int open_stride, const int32_t* h_open_lens,
                                  uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int persistent, int max_steps, int32_t* h_overflow, int32_t* h_steps, void* stream);
int gmk_trad_root_choice_sampled(gmk_trad* t, int16_t* d_cells, uint16_t* d_visits, int sample_plies, int sample_power, uint64_t seed, uint32_t first_game_id, void* stream);

/* ---- K21: Gumbel root search for K7 self-play, with its policy target ----
 * At few playouts per move (32 .. 64 over up to 225 children) PUCB spreads the playouts thinly, the most visited child is a noisy choice and the
 * visit row carries little policy improvement.  Gumbel AlphaZero (Danihelka et al., ICLR 2022) samples m root children without replacement
 * (Gumbel-top-m), spends the playouts on them by sequential halving and learns from the completed-Q improved policy.  The rule -- draws, considered
 * set, schedule, root step, move, policy row -- is stated once, in gomoku_gumbel.h, in binary64 operations that are the same bits on the host and on
 * gfx950.  It acts at the ROOT only: below it the descent is PUCB's, unchanged.
 * gmk_az_set_gumbel(a, max_considered, n_sims, c_visit, c_scale, seed, first_game_id): max_considered = 0 switches it off (the default: every
 *   entry then launches exactly what it launched before); otherwise max_considered in 1 .. 225, n_sims in 1 .. 4096, c_visit and c_scale finite
 *   and >= 0 (the paper's 50 and 1.0 are parameters, not tuned here), else GMK_ERR_ARG.  GMK_ERR_STATE while GMK_OPT_AZ_LEAVES > 1 or
 *   GMK_OPT_AZ_PROOF = 1; while it is on, gmk_az_set_option returns GMK_ERR_STATE for those two values.  GMK_OPT_AZ_VCF_DEPTH composes: it
 *   changes the expand kernels only.  The first use allocates 2940 B per game.  Synchronises.  The draws of slot g are keyed by (seed; first_game_id +
 *   the game the slot plays, as K20 names it; the stones on the root board; 'gmbl'; the cell).
 *   While it is on, gmk_az_select's root step is the rule's: the first root step that finds children makes the set-up for that root (the playout
 *   that expands a childless root is just a playout), and every entry that moves or replaces a root -- gmk_az_set_roots, gmk_az_set_slots,
 *   gmk_az_step, gmk_az_step_device, gmk_az_advance, gmk_az_advance_sampled, and this call -- voids the set-ups, behind its launches on its stream.
 *   gmk_az_add_root_noise stays callable: the rule reads whatever priors stand at set-up.
 * gmk_az_advance_gumbel / gmk_az_root_choice_gumbel: gmk_az_advance / gmk_az_root_choice with the rule's move, and with the improved-policy row
 *   (uint16, adds up to 65535 within 225) where they write the visit counts: the record, wire and replay formats stay what they are, and the
 *   row is read with GMK_TARGET_POLICY below.  A root that was not searched since it became the root gets its set-up here (every r_c is 0: the
 *   move is the considered child with the largest s_c + sigma_c).  Both void the set-up of every root they read, so the choice is taken once per
 *   root.  GMK_ERR_STATE while the option is off; otherwise as their plain forms.  One launch on `stream`.
 * gmk_gumbel_*_host: the header's serial statements for n roots given by rows [n][225] by cell, on the host (no GPU, no gmk_init; they are the
 *   tests' and a binder's view of the rule): _sequence_host the schedule seq[0 .. n_sims) for m_eff; _setup_host the draws g_c (h_draws, of all
 *   225 cells, may be NULL), s_c, the visit snapshot, the considered set and m_eff; _pick_host the cell of the next playout's root step;
 *   _move_host the move; _row_host the improved-policy row.  -1 where a root has no children.  h_stones in 0 .. 225, h_game_ids GLOBAL.
 * Out of scope: Gumbel below the root, GMK_OPT_AZ_LEAVES > 1, proofs and the defence solver, evaluation matches, the ensembles, K3, K6 and K8.
 * Playing strength and training benefit are not measured yet. */
int gmk_az_set_gumbel(gmk_az* a, int max_considered, int n_sims, double c_visit, double c_scale, uint64_t seed, uint32_t first_game_id);
int gmk_az_advance_gumbel(gmk_az* a, uint8_t* d_moves, uint16_t* d_visits, int32_t* d_lens, int8_t* d_winner, int reuse_subtree, int32_t* h_unfinished, void* stream);
int gmk_az_root_choice_gumbel(gmk_az* a, int16_t* d_cells, uint16_t* d_visits, void* stream);
int gmk_gumbel_sequence_host(int m_eff, int n_sims, uint32_t* h_seq);
int gmk_gumbel_setup_host(const float* h_prior, const uint32_t* h_visits, const int32_t* h_stones, const uint32_t* h_game_ids /* already global */, int n,
                          int max_considered, uint64_t seed, double* h_draws /* or NULL */, double* h_score, uint32_t* h_base, uint8_t* h_considered, int32_t* h_m_eff);
int gmk_gumbel_pick_host(const float* h_prior, const uint32_t* h_visits, const float* h_value, const float* h_root_value /*[n]*/, const double* h_score,
                         const uint32_t* h_base, const uint8_t* h_considered, const int32_t* h_m_eff, int n, int n_sims, double c_visit, double c_scale,
                         int16_t* h_cells);
int gmk_gumbel_move_host(const float* h_prior, const uint32_t* h_visits, const float* h_value, const float* h_root_value, const double* h_score,
                         const uint32_t* h_base, const uint8_t* h_considered, int n, double c_visit, double c_scale, int16_t* h_cells);
int gmk_gumbel_row_host(const float* h_prior, const uint32_t* h_visits, const float* h_value, const float* h_root_value, int n, double c_visit, double c_scale,
                        uint16_t* h_rows);

/* ---- K12: the referee of a match between two search handles, on the device (match_kernel.hip) ----
 * One ply of n two-agent games without the host in the loop (agents/utils.py:13-63 dual_play, :66-100 eval_agents): the side to move has
 * searched; gmk_az_root_choice or gmk_trad_root_choice leaves its cells and visit rows in device memory; gmk_match_referee plays them on
 * the game records; gmk_trad_step_device and gmk_az_step_device make both trees follow.
 * The referee, one wavefront per game: slot g plays the record row d_row_of[g] (int32[n], NULL: row g; rows = the records' row count) of
 * d_moves uint8[rows][225], d_lens int32[rows], d_winner int8[rows], d_visits uint16[rows][225][225] (may be NULL).  For every game that
 * is still running it rebuilds the position from the record, refuses a cell that is off the board or occupied (the record stays as it is
 * and bit 0 of d_status[g] is set; bit 1: d_row_of[g] is not a row), and otherwise plays it with Board::applyMove's end test (Game.cpp:37-49,
 * 88-136: five or more through the new stone, or a full board as a tie), appends the move and the visit row d_visit_rows[g] (uint16[n][225],
 * NULL: zeros) to the record and writes the winner of a game that ended.
 * d_verdict int32[n] is the state of the games and the referee's word to the step calls; the caller zeroes it (GMK_MATCH_MOVED) before
 * the first ply, or sets GMK_MATCH_OVER for a game that is not to be played, and zeroes d_status:
 *   GMK_MATCH_MOVED 0    the cell was played, the game goes on          GMK_MATCH_REFUSED 1   the game did not move and goes on
 *   GMK_MATCH_ENDED 2    the cell was played and ended the game         GMK_MATCH_OVER 3      the game was over before this ply
 * d_unfinished int32[1]: the games that go on (MOVED or REFUSED) after this ply. */
#define GMK_MATCH_MOVED 0
#define GMK_MATCH_REFUSED 1
#define GMK_MATCH_ENDED 2
#define GMK_MATCH_OVER 3
int gmk_match_referee(int n, int rows, const int16_t* d_cells, const uint16_t* d_visit_rows, const int32_t* d_row_of, uint8_t* d_moves, int32_t* d_lens,
                      int8_t* d_winner, uint16_t* d_visits, int32_t* d_verdict, int32_t* d_status, int32_t* d_unfinished, void* stream);

/* ---- K13: root-parallel tree ensembles: one position searched by many replicas, their root tables merged on the device ----
 * The n_games of a K3 handle (gmk_mcts) or a K6 / K6 + RAVE / K8 handle (gmk_trad) are read as E = n_games / group ensembles of `group`
 * consecutive games: ensemble e = games e*group .. e*group + group - 1, the REPLICAS of one position, each with its own arena and its own
 * random streams (its game id).  The merge calls read the replicas' roots after a search and write one table per ensemble; they touch no
 * tree, so the searches can go on afterwards.  Outputs are device memory, written on `stream`; nothing is copied to the host and the call
 * does not wait; any output may be NULL:
 *   d_visits uint32[E][225], d_values float[E][225], d_cells int16[E], d_cells_per_game int16[n_games] (the ensemble's cell once per
 *   replica: what gmk_mcts_step takes as d_forced_moves and gmk_trad_step_device as d_cells), d_root_visits uint32[E], d_root_value
 *   float[E], d_status int32[E].
 * The merge.  With n_r[c], q_r[c] replica r's root child visits and value at cell c (zero without a child) and N_r, V_r its root's, as the
 * root statistics calls report them:
 *   visits[c] = sum_r n_r[c]
 *   S[c]      = sum_r llrint(double(n_r[c]) * double(q_r[c]) * 2^24)     int64; every product rounded on its own, no fused multiply-add
 *   values[c] = float(double(S[c]) / 2^24 / double(visits[c])), 0 where visits[c] = 0
 *   root_visits, root_value: the same over (N_r, V_r)
 *   cell      = the first maximum of visits in ascending cell order (MCTS::stepForward, core/lib/src/MCTS.cpp:129-134), -1 without a visit.
 * Every sum is a sum of integers, so the result is the same bits for any launch geometry and any order of the replicas.
 * Status bits: GMK_ENSEMBLE_MISMATCH -- a replica does not stand at the position of replica 0 of its ensemble (the same stones, hence the
 *   same player to move): the ensemble's visit and value rows and root pair are zeros and its cell is -1 in both cell outputs; other
 *   ensembles are unaffected.  GMK_ENSEMBLE_RANGE -- a replica holds a count of 2^24 or more: it adds nothing (so |S| < 2^60 always).
 *   GMK_ENSEMBLE_SATURATED -- a sum of counts passed 2^32 - 1 (possible from 257 replicas on): that uint32 output holds 2^32 - 1; the sums
 *   themselves are kept in 64 bits, so values, root_value and the cell are those of the exact sums.
 * A finished or idle replica adds nothing (K3: status bit 0; K6 / K8: status bit 4), nor does one that was positioned and never searched.
 * GMK_ERR_ARG unless 1 <= group <= 4096 and group divides n_games.
 * gmk_ensemble_merge_host: the same merge of host tables h_visits uint32[E*group][225], h_values float[E*group][225], h_root_visits
 *   uint32[E*group], h_root_values float[E*group] (the root pair may be NULL: zeros) into host outputs (any may be NULL); there are no
 *   positions to compare, so GMK_ENSEMBLE_MISMATCH is never set.  Needs no GPU and no gmk_init. */
enum { GMK_ENSEMBLE_MISMATCH = 1, GMK_ENSEMBLE_RANGE = 2, GMK_ENSEMBLE_SATURATED = 4 };
int gmk_mcts_ensemble_merge(gmk_mcts* m, int group, uint32_t* d_visits, float* d_values, int16_t* d_cells, int16_t* d_cells_per_game,
                            uint32_t* d_root_visits, float* d_root_value, int32_t* d_status, void* stream);
int gmk_trad_ensemble_merge(gmk_trad* t, int group, uint32_t* d_visits, float* d_values, int16_t* d_cells, int16_t* d_cells_per_game,
                            uint32_t* d_root_visits, float* d_root_value, int32_t* d_status, void* stream);
int gmk_ensemble_merge_host(int n_ensembles, int group, const uint32_t* h_visits, const float* h_values, const uint32_t* h_root_visits,
                            const float* h_root_values, uint32_t* out_visits, float* out_values, int16_t* out_cells,
                            uint32_t* out_root_visits, float* out_root_value, int32_t* out_status);

/* ---- K9: the convolutional trunk of the policy-value network (the evaluator K7 calls at every leaf) as one fused kernel ----
 * Replaces the convolution layers of PolicyValueNetwork (network/model_tf.py:28-66: conv3x3 6->32->64->128 with ReLU, the 1x1
 * policy head 128->4 and the 1x1 value head 128->2, both with ReLU) for a batch of positions, in float32 on the f32 matrix cores.
 * Weights are host arrays in PyTorch's conv layout [cout][cin][3][3] ([cout][cin] for the 1x1 heads), packed once at creation.
 * gmk_pvnet_forward: d_states float32 [n][6][225] (Board.encoded_states(), game_ext.hpp:87-104) ->
 *   d_pflat float32 [n][900] = relu(policy conv) flattened (pixel, channel), d_vflat float32 [n][450] likewise for the value head:
 * the inputs of the network's dense layers (tf.layers.flatten of the NHWC tensors).
 * gmk_pvnet_set_dense: the three dense layers behind them (network/model_tf.py:53-54 policy_logits / policy_output, :64-66 value_hidden /
 *   value_logits / value_output), host arrays in [out][in] order over the (pixel, channel) flattening: w_policy [225][900], b_policy [225],
 *   w_hidden [64][450], b_hidden [64], w_out [64], b_out; packed once, may be called again with new weights (a blocking copy: not while a
 *   gmk_pvnet_evaluate of this handle is in flight on another stream).
 * gmk_pvnet_evaluate: the whole PolicyValueNetwork.eval_state forward (network/model_tf.py:136-145) for a batch, two kernels on `stream`:
 *   d_states float32 [n][6][225] -> d_value float32 [n] = tanh(...), d_probs float32 [n][225] = softmax(...).  The head activations between
 *   the kernels live in the handle (grown on demand, which synchronises `stream`: let a batch size's first call happen outside a stream
 *   capture; one handle serves one stream at a time).  GMK_ERR_STATE before gmk_pvnet_set_dense. */
typedef struct gmk_pvnet gmk_pvnet;
int gmk_pvnet_create(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                     const float* w_policy, const float* b_policy, const float* w_value, const float* b_value, gmk_pvnet** out);
int gmk_pvnet_destroy(gmk_pvnet* net);
int gmk_pvnet_forward(gmk_pvnet* net, const float* d_states, int n, float* d_pflat, float* d_vflat, void* stream);
int gmk_pvnet_set_dense(gmk_pvnet* net, const float* w_policy, const float* b_policy, const float* w_hidden, const float* b_hidden,
                        const float* w_out, float b_out);
int gmk_pvnet_evaluate(gmk_pvnet* net, const float* d_states, int n, float* d_value, float* d_probs, void* stream);

/* ---- K9 in bf16: the same trunk on the bf16 matrix cores, opt-in per handle ----
 * A handle evaluates in GMK_PVNET_F32 (the default: exactly the kernels above) or GMK_PVNET_BF16.  Precision GMK_PVNET_BF16 evaluates the same
 * network under these rules, and nothing else changes:
 *   - the five convolution weight tensors (three 3x3 layers, two 1x1 heads) are rounded once to bf16, round to nearest, ties to even; biases
 *     and the three dense layers stay float32;
 *   - the input planes are rounded to bf16 on load (the 0/1 planes K7 feeds are exact);
 *   - every convolution accumulates in float32 on the matrix cores (v_mfma_f32_32x32x16_bf16), the 3x3 layers starting from their float32 bias;
 *   - after ReLU the activations of layers 1, 2 and 3 are rounded to bf16 (nearest even): they feed the next matrix instruction;
 *   - the 1x1 heads take the bf16 layer-3 activations and bf16 weights; each of the four wavefronts sums its 32 channels, the four partial
 *     sums are added in float32 in wavefront order, then the float32 head bias and ReLU: d_pflat / d_vflat are float32;
 *   - the dense kernel is the float32 one, unchanged, on those rows;
 *   - no float atomics: the same inputs give the same bits, and a row's outputs depend neither on the batch nor on where the row sits in it.
 * gmk_pvnet_set_precision: blocking (it synchronises the device and, for GMK_PVNET_BF16, packs the bf16 weights from the handle's current ones);
 *   not while a call on this handle is in flight on another stream, as for gmk_pvnet_set_dense.  GMK_ERR_ARG for a NULL handle or any other
 *   precision.  gmk_pvnet_forward and gmk_pvnet_evaluate run the trunk of the handle's precision; gmk_train_export also refreshes the bf16
 *   weights of a handle that is in GMK_PVNET_BF16, on its stream.  A handle switched back to GMK_PVNET_F32 gives the float32 bits again.
 * gmk_pvnet_get_precision: *precision = the handle's.  GMK_ERR_ARG for a NULL argument.
 * gmk_bf16_round_host: dst[i] = the bf16 bits of src[i] as the packer rounds them (nearest even; NaN -> 0x7FC0; beyond the largest bf16 -> Inf).
 *   Needs no GPU and no gmk_init.  GMK_ERR_ARG for a NULL pointer with n > 0. */
enum { GMK_PVNET_F32 = 0, GMK_PVNET_BF16 = 1 };
int gmk_pvnet_set_precision(gmk_pvnet* net, int precision);
int gmk_pvnet_get_precision(gmk_pvnet* net, int* precision);
int gmk_bf16_round_host(const float* src, size_t n, uint16_t* dst);

/* ---- K22: the network evaluated over the board's eight symmetries ----
 * The rule -- the numbering of the symmetries, the transform T_a of a position, the back-transform of a policy row and the pick of
 * GMK_PVNET_SYM_RANDOM -- is stated once, in gomoku_symmetry.h.  gmk_pvnet_evaluate_sym takes gmk_pvnet_evaluate's arguments plus a mode:
 *   GMK_PVNET_SYM_NONE    exactly the launches of gmk_pvnet_evaluate.
 *   GMK_PVNET_SYM_ALL     per row: (v_a, q_a) = gmk_pvnet_evaluate(T_a(s)) for a = 0 .. 7, p_a = q_a back-transformed;
 *                         value = (v_0 + v_1 + .. + v_7) * 0.125f, probs[c] = (p_0[c] + .. + p_7[c]) * 0.125f, float32 sums in this order
 *                         (the library is built with -ffp-contract=off): the result is defined bit for bit by gmk_pvnet_evaluate, which is
 *                         isolated by row in both precisions.
 *   GMK_PVNET_SYM_RANDOM  value = v_a, probs = p_a with a = the pick: a function of the row's content and `seed` only, never of the row's
 *                         index or the batch.  `seed` is ignored by the other two modes.
 * Launches: one expand kernel (n rows -> 8n or n transformed rows, and the picks), gmk_pvnet_evaluate's two kernels on those rows in the
 * handle's precision, one reduce kernel; all on `stream`, nothing on any other stream.  d_states is not written and nothing past row n of
 * the outputs is written.  n = 0 is a no-op.  GMK_ERR_ARG for a NULL handle, a NULL pointer with n > 0, n < 0 or another mode -- before
 * anything touches a GPU --, GMK_ERR_STATE before gmk_init or gmk_pvnet_set_dense.
 * The handle owns the workspace (the expanded states, their 8n or n rows of outputs, the picks) and the head activations of those rows.
 * Both grow on demand and never shrink; growth synchronises `stream` and allocates, so it must not happen during a stream capture: let
 * the first call of a batch size and mode happen eagerly.  AlphaZeroMCTS.search(graph=True) does: its first step runs eagerly with the
 * full batch and sizes the workspace, the captured step only launches.  One handle serves one stream at a time, as for gmk_pvnet_evaluate.
 * gmk_pvnet_sym_pick_host: h_sym[i] = the pick of GMK_PVNET_SYM_RANDOM for row i of h_states float32 [n][6][225].  Needs no GPU and no
 *   gmk_init.  GMK_ERR_ARG for n < 0 or a NULL pointer with n > 0. */
enum { GMK_PVNET_SYM_NONE = 0, GMK_PVNET_SYM_ALL = 1, GMK_PVNET_SYM_RANDOM = 2 };
int gmk_pvnet_evaluate_sym(gmk_pvnet* net, const float* d_states, int n, int mode, uint64_t seed, float* d_value, float* d_probs,
                           void* stream);
int gmk_pvnet_sym_pick_host(const float* h_states, int n, uint64_t seed, int32_t* h_sym);

/* ---- K10: the pattern heuristic on its own, per position and for whole greedy games ----
 * Heuristic::EvaluationProbs, DecisiveFilter and EvaluationValue (core/lib/include/algorithms/Heuristic.hpp:16-45, 94-161) for a batch, outside
 * any tree.  filter: 1 = EvaluationProbs + DecisiveFilter (PatternEvalAgent::getAction, core/interface/src/Agent.h:107-160, and
 * TraditionalPolicy::hybridSimulate); 0 = EvaluationProbs alone (Heuristic::MaxEvaluatedRollout, Heuristic.hpp:61-83).
 * gmk_pattern_policy: position g is the move list d_moves[g*stride .. + d_lens[g]), black first and alternating, replayed in order on a fresh
 *   evaluator (Evaluator::applyMove, as gmk_evalstate_update: the heuristic reads the order-dependent flag words).  For the player to move:
 *   d_probs float32[n][225] (an empty list: 1.0 on the centre cell, Heuristic.hpp:22-25), d_value float32[n] = EvaluationValue, d_best int32[n] =
 *   the first maximum of probs (maxCoeff).  Any output pointer may be NULL.  d_status int32[n]:
 *     bit 0  the game is over at this position: probs all zero, value 0, best -1 (the reference never asks)
 *     bit 1  evaluator error, as in K1 and K2
 *     bit 2  not a position: a cell >= 225, an occupied cell, a move after the end or a length outside [0, 225]; outputs as for bit 0, and
 *            nothing outside the list is read
 *   Asynchronous on `stream`; n = 0 does nothing.  The work counter of a launch comes from a ring the first call allocates: let that call
 *   happen outside a stream capture.
 * gmk_pattern_policy_host: the same with host buffers (allocates, copies in, runs, copies out, synchronises).
 * gmk_pattern_play: whole games in ONE launch.  On entry d_moves uint8[n][225] / d_lens int32[n] hold every game's opening (0 .. 225 moves), on
 *   exit the whole game: every ply is the policy above on the live evaluator and applyMove of `best`, until Evaluator::checkGameEnd
 *   (Pattern.cpp:344-354) or until max_moves > 0 plies were added (0: no limit).  d_winner int8[n] = -1, 0 or 1; d_values float32[n][225] (or NULL):
 *   entry i = the EvaluationValue the player of move i saw, 0 for the opening's plies and past the end.  d_status: bits 0 (the game is finished), 1
 *   and 2 as above -- an opening that is not a position is left as it was given, winner 0 -- and
 *     bit 3  stalled: the chosen cell was not empty, where the reference would ask again for ever (Heuristic.hpp:65-68); the game stops where
 *            it stands, winner 0.
 *   d_winner, d_values and d_status may be NULL. */
int gmk_pattern_policy(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int filter,
                       float* d_probs, float* d_value, int32_t* d_best, int32_t* d_status, void* stream);
int gmk_pattern_policy_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int filter,
                            float* h_probs, float* h_value, int32_t* h_best, int32_t* h_status);
int gmk_pattern_play(uint8_t* d_moves, int32_t* d_lens, int n, int filter, int max_moves,
                     int8_t* d_winner, float* d_values, int32_t* d_status, void* stream);

/* ---- K23: the pattern heuristic for rows of network planes: K10 as K7's leaf evaluator ----
 * The rule is include/gomoku_pattern_states.h, which the kernel and the host forms compile: row g of d_states float32 [n][6][225] (the planes
 * of Board.encoded_states / gmk_az_select) is decoded (a cell is set iff x != 0), checked, turned into its CANONICAL move list and put through
 * gmk_pattern_policy's path with `filter`.  The canonical order is this project's definition -- the real order of a position's moves is not
 * in the planes -- so a K7 leaf need not get the bits K6 gets for the same game.
 * gmk_pattern_evaluate_states: d_value float32[n] (EvaluationValue for the player to move, in [-1, 1]: what gmk_az_expand takes), d_probs
 *   float32[n][225], d_status int32[n] or NULL: gmk_pattern_policy's bits 0, 1, 2 for the canonical list; bit 2 (GMK_PATTERN_ILLEGAL) also for
 *   a row that is not a position, the all-zero row of a finished K7 leaf among them.  Rows with bit 0 or 2 get zero outputs.
 *   norm GMK_PATTERN_NORM_L2: probs = K10's L2-normalised vector, bit for bit.  GMK_PATTERN_NORM_SUM: probs_c = (float)((double)v_c / S), S
 *   the binary64 sum in gmk_noise_sum225's order; S == 0 on a live row: uniform over the empty cells.
 *   Asynchronous on `stream`, nothing runs on any other stream; d_states is not written and nothing past row n of an output is.  n = 0
 *   does nothing.  GMK_ERR_ARG, before anything touches a GPU, for n < 0, a NULL d_states / d_value / d_probs with n > 0, a filter other than
 *   0 or 1 or an unknown norm; GMK_ERR_STATE before gmk_init (no CPU fallback).  The work counter of a launch comes from gmk_pattern_policy's
 *   ring, which the first call of either allocates: let that call happen outside a stream capture; afterwards the entry can be captured.
 * gmk_pattern_evaluate_states_host: the same with host buffers (stages, runs, synchronises); h_status may be NULL.
 * gmk_pattern_states_list_host: the decode and the canonical list alone: h_moves uint8[n][225] (entries past the length are not written),
 *   h_lens int32[n], h_status int32[n] = 0 or GMK_PATTERN_ILLEGAL (length 0).  Needs no GPU and no gmk_init.
 * gmk_pattern_states_finish_host: h_probs float32[n][225] from h_vec float32[n][225] (K10's vectors of the rows' lists) under `norm`.  It
 *   knows no evaluator status: a row that decodes as a position counts as live, any other row gets zeros.  Needs no GPU and no gmk_init. */
#ifndef GMK_PATTERN_NORM_DEFINED
#define GMK_PATTERN_NORM_DEFINED
enum { GMK_PATTERN_NORM_L2 = 0, GMK_PATTERN_NORM_SUM = 1 };
#endif
int gmk_pattern_evaluate_states(const float* d_states, int n, int filter, int norm,
                                float* d_value, float* d_probs, int32_t* d_status, void* stream);
int gmk_pattern_evaluate_states_host(const float* h_states, int n, int filter, int norm,
                                     float* h_value, float* h_probs, int32_t* h_status);
int gmk_pattern_states_list_host(const float* h_states, int n, uint8_t* h_moves, int32_t* h_lens, int32_t* h_status);
int gmk_pattern_states_finish_host(const float* h_vec, const float* h_states, int n, int norm, float* h_probs);

/* ---- K14: the forced-win solver by continuous fours (VCF), exact, per position and in batch ----
 * No counterpart in the reference; the contract is this block.  All of it is geometry on the 15 x 15 board, the pattern automaton is not involved.
 * Position g is the move list d_moves[g*stride .. + d_lens[g]), black first and alternating; a cell is y * 15 + x.  The ATTACKER is the side to
 * move, or with GMK_VCF_OPPONENT the other side, moving first as if the side to move had passed ("what threatens me?"); the defender is the
 * other colour.  completing(S) = the empty cells whose occupation by colour S makes a run of five OR MORE through that cell (freestyle, as
 * Board::checkGameEnd; runs do not wrap from one row into the next).  L limits the attacker's moves, the one that makes five included.
 *
 *   attack(depth):                                  the attacker is to move and has made `depth` moves
 *     W = completing(attacker);  if W: pv += [min W]; return WIN
 *     T = completing(defender);  if |T| >= 2: return FAIL
 *     if depth + 2 > L: cut = true; return FAIL
 *     for c in (T if T else all empty cells), ascending:
 *         F = completing(attacker) with c played;  if F is empty: continue            (not a four: no candidate, no node)
 *         if nodes == budget: stop everything with BUDGET
 *         nodes += 1
 *         if |F| >= 2: pv += [c, F's lowest, F's second lowest]; return WIN
 *         r = F's only cell; play c and r
 *         if attack(depth + 1) == WIN: pv = [c, r] + the rest; return WIN
 *         undo both
 *     return FAIL
 *
 * Plain mode runs attack(0) with L = max_depth.  GMK_VCF_ITERATIVE runs L = 1, 2, .. max_depth in turn, `cut` cleared before each, and stops
 * at the first WIN or at the first limit that fails without a cut; nodes add up over the limits and the budget is on the total.
 * Per position (any output pointer may be NULL): d_status int32[n], d_move int32[n], d_length int32[n], d_nodes uint32[n],
 * d_pv uint8[n][GMK_VCF_PV]:
 *     GMK_VCF_NONE    FAIL with cut false: no forced win by fours at any depth
 *     GMK_VCF_WIN     move = pv[0], length = the attacker's moves in pv, which has 2 * length - 1 cells, attacker and defender alternating
 *     GMK_VCF_DEPTH   no win found and some branch was cut by the limit
 *     GMK_VCF_BUDGET  nodes == budget and another candidate was due
 *     GMK_VCF_OVER    a colour already has five or more; nothing is searched
 *     GMK_VCF_BAD     not a position: a length outside [0, 225] or above stride, a cell >= 225 or a repeated cell; nothing is searched and
 *                     nothing outside the list is read
 *   move is -1 and length 0 unless WIN; nodes is 0 for OVER and BAD, else the count when the search stopped; pv cells past the end are 255.
 *   Every output is an exact function of the list, max_depth, budget and flags.
 * gmk_vcf_solve: asynchronous on `stream`, allocates nothing; n = 0 does nothing.  GMK_ERR_ARG: a NULL input with n > 0, n < 0, stride < 1,
 *   max_depth outside [1, GMK_VCF_MAX_DEPTH], unknown flag bits, d_lens or an int32 output not 4-byte aligned.  GMK_ERR_STATE without a device.
 * gmk_vcf_solve_host: the same with host buffers (allocates, copies in, runs on the GPU, copies out, synchronises). */
enum { GMK_VCF_MAX_DEPTH = 32, GMK_VCF_PV = 64 };
enum { GMK_VCF_OPPONENT = 1, GMK_VCF_ITERATIVE = 2 };
enum { GMK_VCF_NONE = 0, GMK_VCF_WIN = 1, GMK_VCF_DEPTH = 2, GMK_VCF_BUDGET = 3, GMK_VCF_OVER = 4, GMK_VCF_BAD = 5 };
int gmk_vcf_solve(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                  int32_t* d_status, int32_t* d_move, int32_t* d_length, uint32_t* d_nodes, uint8_t* d_pv, void* stream);
int gmk_vcf_solve_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                       int32_t* h_status, int32_t* h_move, int32_t* h_length, uint32_t* h_nodes, uint8_t* h_pv);

/* ---- K15: the moves that refute a forced win by continuous fours, exact, per position and in batch ----
 * No counterpart in the reference; the contract is this block, on top of K14's.  A position is the move list, as for K14.  D is the side to
 * move, A the other colour: the threat's attacker.  attack, completing, L and budget are K14's; solve(list, flags) is gmk_vcf_solve's result
 * for that list with the same max_depth and budget.  flags: 0 or GMK_VCF_ITERATIVE.
 *
 *   1. threat = solve(P, GMK_VCF_OPPONENT | (flags & GMK_VCF_ITERATIVE)): d_threat_status int32[n], d_threat_length int32[n],
 *      d_threat_pv uint8[n][GMK_VCF_PV], d_threat_nodes uint32[n], equal bit for bit to what gmk_vcf_solve writes.
 *   2. threat OVER or BAD: every cell's verdict is GMK_VCF_CELL_NONE; nothing is searched.
 *   3. Otherwise each cell c has a verdict (d_verdict uint8[n][225]), a length (d_cell_length uint8[n][225]) and nodes (d_cell_nodes
 *      uint32[n][225]); length and nodes are 0 unless said otherwise:
 *        c occupied                                   GMK_VCF_CELL_NONE
 *        c in completing(D) on P                      GMK_VCF_CELL_FIVE     D wins at once
 *        else, threat NONE                            GMK_VCF_CELL_HOLDS    not searched: a defender stone never gives the attacker a line of
 *                                                                           fours he did not have
 *        else, threat DEPTH or BUDGET                 GMK_VCF_CELL_UNKNOWN  not searched: the caller raises the limits
 *        else (threat WIN with pv): follow(0) on P with a D stone on c -- the walk of attack with exactly one candidate per level, pv's
 *        attacker move of that level:
 *
 *          follow(i):                       the board is P, the D stone on c, then i attacker moves of pv and their i forced replies
 *            if completing(A): return LOSES, length i + 1
 *            T = completing(D);  if |T| >= 2: return FAIL
 *            if 2 i >= |pv|: return FAIL
 *            a = pv[2 i];  if a is occupied, or T is not empty and a is not in T: return FAIL
 *            F = completing(A) with a played;  if F is empty: return FAIL
 *            if |F| >= 2: return LOSES, length i + 2
 *            play a and F's only cell;  return follow(i + 1)
 *
 *          LOSES                                      GMK_VCF_CELL_LOSES with that length, nodes 0
 *          FAIL: s = solve(P + [c], flags & GMK_VCF_ITERATIVE), each such cell with the whole budget; nodes = s.nodes
 *            s WIN                                    GMK_VCF_CELL_LOSES, length = s.length
 *            s NONE                                   GMK_VCF_CELL_HOLDS
 *            s DEPTH or BUDGET                        GMK_VCF_CELL_UNKNOWN
 *   4. Every output is an exact function of the list, max_depth, budget and flags.
 *
 * gmk_vcf_defend: asynchronous on `stream` (two launches), allocates nothing; n = 0 does nothing.  d_threat_nodes, d_cell_length and
 *   d_cell_nodes may be NULL; the other four outputs are required, and the second launch reads the three required threat outputs.
 *   GMK_ERR_ARG as for gmk_vcf_solve, and for a NULL required output with n > 0, GMK_VCF_OPPONENT or an unknown bit in flags, a 4-byte output
 *   that is not 4-byte aligned.  GMK_ERR_STATE without a device.  Nothing outside a list's len cells is read; the stone on c is added in
 *   registers, never written to the list.
 * gmk_vcf_defend_host: the same with host buffers (allocates, copies in, runs on the GPU, copies out, synchronises). */
enum { GMK_VCF_CELL_NONE = 0, GMK_VCF_CELL_HOLDS = 1, GMK_VCF_CELL_LOSES = 2, GMK_VCF_CELL_UNKNOWN = 3, GMK_VCF_CELL_FIVE = 4 };
int gmk_vcf_defend(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                   int32_t* d_threat_status, int32_t* d_threat_length, uint8_t* d_threat_pv, uint32_t* d_threat_nodes,
                   uint8_t* d_verdict, uint8_t* d_cell_length, uint32_t* d_cell_nodes, void* stream);
int gmk_vcf_defend_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                        int32_t* h_threat_status, int32_t* h_threat_length, uint8_t* h_threat_pv, uint32_t* h_threat_nodes,
                        uint8_t* h_verdict, uint8_t* h_cell_length, uint32_t* h_cell_nodes);

/* ---- K17: what a stone of the side to move threatens, for every cell, exact, per position and in batch ----
 * No counterpart in the reference; the contract is this block, on top of K14's.  A position is the move list, as for K14.  A is the side to
 * move, D the other colour.  attack, completing, L and budget are K14's; solve(list, flags) is gmk_vcf_solve's result for that list with the
 * same max_depth and budget.  flags: 0 or GMK_VCF_ITERATIVE.
 *
 *   1. own = solve(P, flags & GMK_VCF_ITERATIVE): d_own_status int32[n], d_own_move int32[n], d_own_length int32[n], d_own_nodes uint32[n],
 *      d_own_pv uint8[n][GMK_VCF_PV], equal bit for bit to what gmk_vcf_solve writes.
 *   2. own OVER or BAD: every cell's verdict is GMK_VCF_THREAT_NONE; nothing is searched.
 *   3. Otherwise (own WIN, NONE, DEPTH or BUDGET alike) each cell c has a verdict (d_verdict uint8[n][225]), a length (d_cell_length
 *      uint8[n][225]) and nodes (d_cell_nodes uint32[n][225]); length and nodes are 0 unless said otherwise.  Tested in this order:
 *        c occupied                                   GMK_VCF_THREAT_NONE
 *        c in completing(A) on P                      GMK_VCF_THREAT_FIVE     A wins at once
 *        completing(D) on P + [c] is not empty        GMK_VCF_THREAT_IGNORES  D makes five next
 *        completing(A) on P + [c] is not empty        GMK_VCF_THREAT_FOUR     length = 1 with one completing cell, 2 with several; not searched
 *        else s = solve(P + [c], GMK_VCF_OPPONENT | (flags & GMK_VCF_ITERATIVE)): A, having played c, attacks again as if D had passed;
 *        each such cell with the whole budget; nodes = s.nodes
 *          s WIN                                      GMK_VCF_THREAT_WINS, length = s.length: c threatens a win by fours in that many moves
 *          s NONE                                     GMK_VCF_THREAT_QUIET
 *          s DEPTH or BUDGET                          GMK_VCF_THREAT_UNKNOWN  the caller raises the limits
 *   4. Every output is an exact function of the list, max_depth, budget and flags.
 *
 * gmk_vcf_threats: asynchronous on `stream` (two launches), allocates nothing; n = 0 does nothing.  d_own_status and d_verdict are required
 *   (the second launch reads the first); the other own outputs, d_cell_length and d_cell_nodes may be NULL.  GMK_ERR_ARG as for
 *   gmk_vcf_defend.  GMK_ERR_STATE without a device.  Nothing outside a list's len cells is read; the stone on c is added in registers, never
 *   written to the list.
 * gmk_vcf_threats_host: the same with host buffers (allocates, copies in, runs on the GPU, copies out, synchronises). */
enum { GMK_VCF_THREAT_NONE = 0, GMK_VCF_THREAT_QUIET = 1, GMK_VCF_THREAT_WINS = 2, GMK_VCF_THREAT_UNKNOWN = 3, GMK_VCF_THREAT_FIVE = 4,
       GMK_VCF_THREAT_FOUR = 5, GMK_VCF_THREAT_IGNORES = 6 };
int gmk_vcf_threats(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                    int32_t* d_own_status, int32_t* d_own_move, int32_t* d_own_length, uint32_t* d_own_nodes, uint8_t* d_own_pv,
                    uint8_t* d_verdict, uint8_t* d_cell_length, uint32_t* d_cell_nodes, void* stream);
int gmk_vcf_threats_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                         int32_t* h_own_status, int32_t* h_own_move, int32_t* h_own_length, uint32_t* h_own_nodes, uint8_t* h_own_pv,
                         uint8_t* h_verdict, uint8_t* h_cell_length, uint32_t* h_cell_nodes);

/* ---- K17: the forced win by continuous threats (fours and threes, VCT), exact, per position and in batch ----
 * No counterpart in the reference; the contract is this block, on top of K14's, K15's and the one above.  A root is a move list; A is its
 * side to move, D the other colour.  solve, threats and defend are gmk_vcf_solve, gmk_vcf_threats and gmk_vcf_defend with this call's
 * max_depth, budget and flags (0 or GMK_VCF_ITERATIVE).  max_threats = T in 1 .. GMK_VCT_MAX_THREATS limits A's threat moves, the moves that
 * are answered by a reply of D's choice; max_positions = M >= 1 caps the positions of one root on one level.
 * The search is level-synchronous.  Level 0 is the root; the positions of level t have A to move after t threat moves and their replies.
 *
 *   for t = 0, 1, .. T:
 *     every position Q of level t: o = solve(Q).  At the root OVER and BAD are the result.  o WIN: Q is won, with depth 0 and line o.pv.
 *       o DEPTH or BUDGET: cut = true.  t = T and Q not won: cut = true (level T is never expanded).
 *     resolve, levels t - 1 .. 0: depth(Q) = 0 if Q is won, else 1 + min over Q's candidates c of (max over c's children of their depth,
 *       0 without children), over the candidates whose children all have a depth; none: no depth yet.
 *     the root has a depth: WIN.  Nothing of it is expanded further.
 *     t < T, every Q of the level that is not won, in order:
 *       the candidates are the cells of threats(Q) with verdict WINS or FOUR, ascending.  A cell UNKNOWN: cut = true; it is no candidate.
 *       candidate c: d = defend(Q + [c]).  A cell UNKNOWN: cut = true and c is dropped.  A cell FIVE: c is dropped (the IGNORES verdict
 *       already excludes it).  Otherwise c's children are the positions Q + [c, r], r over the HOLDS cells, ascending; they join level t + 1.
 *     level t + 1 has more than M positions: GMK_VCT_BUDGET, and the level is discarded.
 *   no win when the levels run out: GMK_VCF_DEPTH if cut, else GMK_VCF_NONE.
 *
 * Nothing is pruned: a position is expanded whether or not its branch can still win, so `positions` is a function of the contract alone.
 * Per root (any output pointer may be NULL): d_status int32[n] (GMK_VCF_NONE, WIN, DEPTH, OVER, BAD, or GMK_VCT_BUDGET), d_move int32[n],
 * d_threats int32[n], d_positions uint32[n], d_pv uint8[n][GMK_VCT_PV]:
 *     move       WIN: pv[0] -- o.move at depth 0, else the lowest cell among the candidates of minimal depth; -1 otherwise
 *     threats    WIN: the root's depth, A's threat moves before the win by fours; 0 otherwise
 *     positions  the sizes of the root's levels added up, the root itself included, up to the level it ended at; a discarded level is not counted
 *     pv         WIN: c, the lowest candidate of minimal depth, then its child r of greatest depth (the lowest r on ties), and so on down; the
 *                line ends with the o.pv of a won position, or with c alone when no reply holds.  Cells past the end, and every cell of
 *                another status, are 255.
 * A root's outputs are an exact function of its list and the six parameters; they do not depend on the other roots of the batch.
 * gmk_vct_solve: the driver is host code.  It allocates its workspace on the device (and frees it), launches the three solvers and small
 *   kernels of its own on `stream`, and SYNCHRONISES `stream` several times per level to read per-root counts; when it returns the outputs are
 *   written.  n = 0 does nothing.  GMK_ERR_ARG: as gmk_vcf_solve, GMK_VCF_OPPONENT in flags, max_threats or max_positions out of range.
 *   GMK_ERR_HIP when a level does not fit in device or host memory; GMK_ERR_CAPACITY when a level, the roots' (n) included, has more than 2^22
 *   positions over the batch.  The workspace is a few blocks per level.
 * gmk_vct_solve_host: the same with host buffers. */
enum { GMK_VCT_MAX_THREATS = 8, GMK_VCT_PV = 80 };
enum { GMK_VCT_BUDGET = 6 };
int gmk_vct_solve(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                  int max_threats, int max_positions, int32_t* d_status, int32_t* d_move, int32_t* d_threats, uint32_t* d_positions,
                  uint8_t* d_pv, void* stream);
int gmk_vct_solve_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                       int max_threats, int max_positions, int32_t* h_status, int32_t* h_move, int32_t* h_threats, uint32_t* h_positions,
                       uint8_t* h_pv);

/* ---- K11: training the policy-value network on the device (network/train.py:62-86, network/model_tf.py:73-135) ----
 * A gmk_trainer holds the network's sixteen parameter tensors in float32 in their canonical layouts (those gmk_pvnet_create and
 * gmk_pvnet_set_dense take), Adam's two moments, a gradient block and the activations of up to max_batch positions.  One step = forward
 * with kept activations, loss, backward, TF1's Adam (tf.train.AdamOptimizer: lr_t = lr sqrt(1 - 0.999^t) / (1 - 0.9^t),
 * w -= lr_t m / (sqrt(v) + 1e-8)); float32 parameters, activations, gradients and moments (Adam's few operations per element run in
 * float64 between float32 loads and stores), no floating-point atomics: the same inputs give the same bits.
 * loss = mean (value - z)^2 + mean softmax cross-entropy(pi, logits) + 1e-4 sum(w^2) / 2 over every tensor that is not a bias.
 * All pointers are device pointers unless named h_; n in [1, max_batch]; everything is asynchronous on `stream` unless said otherwise.
 *
 * The host arrays h_w1 .. h_b_out are gmk_pvnet_create's ten followed by gmk_pvnet_set_dense's six (h_b_out points at one float).
 * BLOCK ORDER -- the order of d_grads and of gmk_train_get_block / gmk_train_set_block, 326 540 floats:
 *   w1 [32][6][3][3], b1 [32], w2 [64][32][3][3], b2 [64], w3 [128][64][3][3], b3 [128], w_policy_conv [4][128], w_value_conv [2][128],
 *   b_policy_conv [4], b_value_conv [2], w_policy [225][900], b_policy [225], w_hidden [64][450], b_hidden [64], w_out [64], b_out [1]
 *   (the two 1x1 heads sit side by side because they run as one GEMM).
 *
 * gmk_train_create: moments zero, step count 0.  max_batch in [1, 4096].
 * gmk_train_forward: d_states float32 [n][6][225] -> d_value [n], d_probs [n][225] (the training path's forward; activations are kept).
 * gmk_train_grads: forward, loss and backward, no update.  d_grads: one block in BLOCK ORDER, the gradient of the data loss (WITHOUT the L2
 *   term).  d_metrics float[4] = loss including L2, entropy mean(-sum p log(p + 1e-10)), value loss, policy loss.
 * gmk_train_step: the same, then Adam on every tensor (weights with the L2 gradient 1e-4 w).  d_probs_out (or NULL) [n][225]: the policy
 *   output from BEFORE the update, as session.run([policy_output, loss, entropy, opt]) fetches it.  d_metrics float[5]: the four above and
 *   [4] = mean sum (old + 1e-10) log((old + 1e-10) / (p + 1e-10)) against d_old_probs [n][225], or 0 if d_old_probs is NULL.
 * gmk_train_params / gmk_train_set_params: the sixteen tensors to / from host arrays (blocking; they synchronise the device).
 * gmk_train_get_block / gmk_train_set_block: a whole block in BLOCK ORDER to / from the host (blocking): which = 0 parameters, 1 first
 *   moments, 2 second moments, 3 (get only) the update the last step applied: w_new = w_old - update, exactly.  Block 3 is a diagnostic: the
 *   difference of two stored float32 parameters carries half an ulp of the PARAMETER, several 1e-6 of a step of lr, so the optimiser's
 *   arithmetic can be checked to 1e-6 only against the update itself (tests/test_train_gpu.py).  It costs a fifth parameter-sized block
 *   (1.3 MB) and one 4-byte store per element and step; nothing in the training path reads it.
 * gmk_train_set_step_count: Adam's t (what a restored state continues from).
 * gmk_train_export: writes the parameters into an existing gmk_pvnet's device buffers, in the layouts gmk_pvnet_create / gmk_pvnet_set_dense
 *   give them, with one kernel on `stream` (GMK_ERR_STATE before gmk_pvnet_set_dense).  The network's output bias is a host scalar in the
 *   handle: its four bytes are read back, so this call returns after `stream` has reached it.  It must not run while a
 *   gmk_pvnet_evaluate of `net` is in flight on another stream.
 * gmk_train_info: the number of steps taken, the scratch bytes (activations, columns, split-K slabs), max_batch, the floats of a block; any
 *   pointer may be NULL. */
typedef struct gmk_trainer gmk_trainer;
int gmk_train_create(const float* h_w1, const float* h_b1, const float* h_w2, const float* h_b2, const float* h_w3, const float* h_b3,
                     const float* h_w_policy_conv, const float* h_b_policy_conv, const float* h_w_value_conv, const float* h_b_value_conv,
                     const float* h_w_policy, const float* h_b_policy, const float* h_w_hidden, const float* h_b_hidden,
                     const float* h_w_out, const float* h_b_out, int max_batch, gmk_trainer** out);
int gmk_train_destroy(gmk_trainer* trainer);
int gmk_train_forward(gmk_trainer* trainer, const float* d_states, int n, float* d_value, float* d_probs, void* stream);
int gmk_train_grads(gmk_trainer* trainer, const float* d_states, const float* d_values, const float* d_pi, int n, float* d_grads,
                    float* d_metrics, void* stream);
int gmk_train_step(gmk_trainer* trainer, const float* d_states, const float* d_values, const float* d_pi, int n, float lr,
                   const float* d_old_probs, float* d_probs_out, float* d_metrics, void* stream);
int gmk_train_params(gmk_trainer* trainer, float* h_w1, float* h_b1, float* h_w2, float* h_b2, float* h_w3, float* h_b3,
                     float* h_w_policy_conv, float* h_b_policy_conv, float* h_w_value_conv, float* h_b_value_conv,
                     float* h_w_policy, float* h_b_policy, float* h_w_hidden, float* h_b_hidden, float* h_w_out, float* h_b_out);
int gmk_train_set_params(gmk_trainer* trainer, const float* h_w1, const float* h_b1, const float* h_w2, const float* h_b2, const float* h_w3,
                         const float* h_b3, const float* h_w_policy_conv, const float* h_b_policy_conv, const float* h_w_value_conv,
                         const float* h_b_value_conv, const float* h_w_policy, const float* h_b_policy, const float* h_w_hidden,
                         const float* h_b_hidden, const float* h_w_out, const float* h_b_out);
int gmk_train_get_block(gmk_trainer* trainer, int which, float* h_block);
int gmk_train_set_block(gmk_trainer* trainer, int which, const float* h_block);
int gmk_train_set_step_count(gmk_trainer* trainer, int64_t step);
int gmk_train_export(gmk_trainer* trainer, gmk_pvnet* net, void* stream);
int gmk_train_info(gmk_trainer* trainer, int64_t* h_step, int64_t* h_scratch_bytes, int32_t* h_max_batch, int32_t* h_param_floats);

/* ---- K11's kernels on their own: the GEMM, its split-K reduction, im2col and col2im on caller-supplied operands ----
 * For tests of the kernels.  Each entry goes through the launcher the trainer itself uses, so the tile variant a shape gets (N <= 32,
 * N <= 64, N > 64) is the trainer's choice.  All pointers are device pointers of float32, strides and extents count floats, everything is
 * asynchronous on `stream`.  The strides are the caller's, so the host checks the addressing in 64-bit integers BEFORE the launch: a
 * descriptor whose largest index leaves a buffer it names, or whose store map writes one float twice, returns GMK_ERR_ARG, nothing is
 * launched and gmk_last_error() names the field.
 *
 * gmk_train_gemm_desc, field by field (the kernel's own argument block plus the extent of every buffer):
 *   A, sam, sak, a_floats    A(m, k) = A[m * sam + k * sak], m < M, k < K.  Strides in [0, 2^31); 0 repeats one element along that axis.
 *   B, sbk, sbn, b_floats    B(k, n) = B[k * sbk + n * sbn], n < N.  An operand whose k stride is 1 is loaded k-fastest; the sums are the same.
 *   M, N, K                  all >= 1.  The result is S(m, n) = sum over k of A(m, k) B(k, n), float32 products accumulated in float32 in an
 *                            order that depends on (M, N, K, kslab, the two "k stride is 1" facts) only, never on the data or on other rows.
 *   kslab, nz, z0, part, part_floats
 *                            part != NULL is the SPLIT-K form: slab z < nz holds the raw sums over k in [z * kslab, min(K, (z + 1) * kslab))
 *                            at part[((z0 + z) * M + m) * N + n]; no epilogue -- bias, relu, mask, C and C2 are not read or written.
 *                            kslab >= 1, z0 >= 0, (z0 + nz) * M * N <= part_floats, and nz is EXACTLY ceil(K / kslab): a slab that would hold
 *                            no k at all is refused, not written as zeros.  nz * kslab < 2^31.
 *                            part == NULL is the DIRECT form: nz must be 1 and kslab >= K (anything else would drop terms silently).
 *   C, ldc, cq, cs, c_floats the direct form's output for columns n < min(N, nsplit): v = S(m, n) + bias[n], then max(v, 0) if relu, then 0
 *                            unless mask(m, n) > 0, stored at C[m * ldc + (n / cq) * cs + n % cq].  cq >= N is "no grouping" (cs is then
 *                            not used; the trainer passes cq = INT_MAX, cs = 0).  With cq < N, cs >= cq; ldc >= one row's extent under the map.
 *   nsplit, C2, ldc2, c2_floats
 *                            columns n >= nsplit go to C2[m * ldc2 + n - nsplit] instead (same epilogue); nsplit >= N is "no split"
 *                            (INT_MAX in the trainer, C2 may be NULL); nsplit = 0 sends every column to C2 and C is not touched.
 *   bias, bias_floats        NULL, or [N].
 *   relu                     0 or 1.
 *   mask, ldm, mask_floats   NULL, or mask(m, n) = mask[m * ldm + n]: only `> 0` keeps (0, -0, negatives and NaN all give 0).
 * gmk_train_kernel_reduce: out[i] = part[0 * mn + i] + part[1 * mn + i] + ... + part[(nz - 1) * mn + i], float32, in that order, i < mn.
 * gmk_train_kernel_im2col: 3x3 'same' columns of npos 15x15 positions of C channels: the input element (position b, pixel p, channel c) is
 *   in[b * sb + p * sp + c * sc] (largest index < in_floats), col[(b * 225 + p) * 9 C + c * 9 + tap] is the pixel tap / 3 - 1 rows and
 *   tap % 3 - 1 columns away, or 0.0f outside the board.  col holds npos * 225 * 9 C floats.
 * gmk_train_kernel_col2im: out[row][c] (row = b * 225 + p, channels-last, npos * 225 * C floats) = the float32 sum, in tap order 0..8, of
 *   the dcol[row'][c * 9 + tap] whose tap reads pixel p -- or 0 unless mask[row][c] > 0.  dcol holds npos * 225 * 9 C floats. */
typedef struct gmk_train_gemm_desc {
    const float* A; int64_t sam, sak, a_floats;
    const float* B; int64_t sbk, sbn, b_floats;
    int32_t M, N, K;
    int32_t kslab, nz, z0;
    float* part; int64_t part_floats;
    float* C; int64_t ldc, cs, c_floats;
    float* C2; int64_t ldc2, c2_floats;
    int32_t cq, nsplit;
    const float* bias; int64_t bias_floats;
    const float* mask; int64_t ldm, mask_floats;
    int32_t relu;
} gmk_train_gemm_desc;
int gmk_train_kernel_gemm(const gmk_train_gemm_desc* desc, void* stream);
int gmk_train_kernel_reduce(const float* part, int nz, int64_t mn, float* out, void* stream);
int gmk_train_kernel_im2col(const float* in, int64_t in_floats, int64_t sb, int64_t sp, int64_t sc, int C, int npos, float* col, void* stream);
int gmk_train_kernel_col2im(const float* dcol, int C, int npos, const float* mask, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOMOKU_HIP_H_ */
