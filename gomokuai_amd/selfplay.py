"""Batched self-play on the GPU and the one exchange step of the path: gathering finished game records.

Replaces the reference's data generation loop -- `network/data_helper.py:58-83` (`simulate_game_data` ->
`dual_play(..., verbose=True)`) run by `DATA_CONFIG["process_num"]` = 2 Python processes that append to a
`multiprocessing.Manager().list()` (`data_helper.py:97-113, 152-169`) -- by thousands of concurrent games per
GPU (K3 + `gmk_mcts_advance`) sharded over ranks by global game id, and ONE gather of the compact records
(moves, per-move root visit counts, winner) to rank 0 over `torch.distributed` (RCCL on MI355X, gloo on CPU).
"""
import contextlib
import os

import numpy as np
import torch

from . import lib as G

N = 225


class GameRecords:
    """Fixed-stride game records: moves u8[n,225], lens i32[n], winner i8[n], visits u16[n,225,225] (optional)."""

    def __init__(self, moves, lens, winner, visits=None, first_game_id=0, overflow=False):
        self.moves, self.lens, self.winner, self.visits, self.first_game_id = moves, lens, winner, visits, first_game_id
        self.overflow = overflow            # a tree arena filled up during some search (results then deviate)

    def __len__(self):
        return int(self.lens.shape[0])

    def cpu(self):
        return GameRecords(self.moves.cpu(), self.lens.cpu(), self.winner.cpu(),
                           None if self.visits is None else self.visits.cpu(), self.first_game_id, self.overflow)

    def to_samples(self, augment=False, first_move=0, target=None):
        """All training tuples of all games, built ON THE GPU (K4 + K5, optionally with the eight-fold augmentation of
        network/data_helper.py:36-55): -> (states uint8[S,6,15,15], values float32[S], pi float32[S,225]) as torch
        tensors on the records' device, samples ordered by (game, move[, symmetry]).  first_move skips opening plies
        that were not searched.  target = "policy": the rows are improved-policy rows (play_network_games(gumbel=)), pi = row / sum(row);
        "visits" or None: MCTS::evalState's transform of visit counts."""
        assert self.visits is not None and self.moves.is_cuda
        dev = self.moves.device
        game, move = _sample_lists(self.lens.cpu().numpy(), first_move)
        n = int(game.shape[0])
        copies = 8 if augment else 1
        d_game, d_move = torch.from_numpy(game).to(dev), torch.from_numpy(move).to(dev)
        states = torch.empty((n * copies, 6, 15, 15), dtype=torch.uint8, device=dev)
        values = torch.empty(n * copies, dtype=torch.float32, device=dev)
        pi = torch.empty((n * copies, N), dtype=torch.float32, device=dev)
        G.samples_from_records(self.moves.data_ptr(), self.lens.data_ptr(), self.visits.data_ptr(), self.winner.data_ptr(),
                               d_game.data_ptr(), d_move.data_ptr(), n, augment, states.data_ptr(), values.data_ptr(), pi.data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream, target=target)
        return states, values, pi

    def samples(self, game):
        """The training tuples of one game as `dual_play(verbose=True)` returns them (agents/utils.py:36-40, 55-59):
        [(uint8[6,15,15] encoded states, float score for the player to move, float32[225] pi)]."""
        assert self.visits is not None
        rec = self.cpu()
        L = int(rec.lens[game])
        winner = int(rec.winner[game])
        cell = np.zeros(N, dtype=np.int8)
        out = []
        for t in range(L):
            cur = 1 if t % 2 == 0 else -1
            states = np.zeros((6, N), dtype=np.uint8)
            states[0] = cell == cur
            states[1] = cell == -cur
            states[2] = cell == 0
            if t >= 1:
                states[3, int(rec.moves[game, t - 1])] = 1
            if t >= 2:
                states[4, int(rec.moves[game, t - 2])] = 1
            states[5] = cur == 1
            counts = rec.visits[game, t].contiguous().view(torch.int16).numpy().view(np.uint16)     # uint16 carried as int16: 32 768 and above are not negative
            pi = G.visits_to_pi(counts.astype(np.uint32), t)
            out.append((states.reshape(6, 15, 15), np.array(float(cur * winner)), pi))
            cell[int(rec.moves[game, t])] = cur
        return out


def _sample_lists(lens, first_move):
    """(game, move) int32 lists of every sample, ordered by (game, move): moves first_move .. len - 1 of each game."""
    game = np.concatenate([np.full(max(int(l) - first_move, 0), g, dtype=np.int32) for g, l in enumerate(lens)] or [np.zeros(0, np.int32)])
    move = np.concatenate([np.arange(first_move, int(l), dtype=np.int32) for l in lens] or [np.zeros(0, np.int32)])
    return game, move


# Games in flight per MI355X for whole-game RandomPolicy self-play, and the number of search handles they are split over.  The loop is ONE
# persistent launch per handle: 8 192 slots are the 2 048 wavefronts (four games each, two per SIMD) the chip holds, so one handle of 8 192 slots fills
# it and keeps it filled until the games run out.  Measured in one process, alternating (tools/k3_handles_ab.py, 32 768 games x 800 playouts, M playouts/s):
# one handle x 8 192 slots 134.9 / 135.5; one x 16 384 (the second half of the wavefronts queues behind the first) 127.3 / 126.9; two handles x 8 192 on
# two streams and host threads -- round 3's default, the best plan of the LOCK-STEP loop, where two handles filled each other's ends of launches --
# 127.9 / 112.4 (and the run-to-run spread VERDICT r3 noted); two x 4 096: 91.
# With kept subtrees a slot owns TWO arenas of three times the nodes (the kept subtree + the new search; 17 MB per slot at 800 playouts per move):
# 8 192 slots are 142 GB of the 288.
SLOTS_PER_GPU = 8192
HANDLES_FROM_GAMES = 1 << 30        # (no longer a default: handles="auto" is one handle; handles=k is still honoured)
SLOTS_PER_GPU_KEPT = 8192


def plan_games(n_games, slots="auto", handles="auto", opening_plies=0, reuse_subtree=False):
    """How play_games spreads n_games over search handles and slots: a list of (first game, one past the last game, slots) per handle,
    or None for the plain lock-step loop (one handle, every game in flight from the start).  Pure bookkeeping, no GPU."""
    if n_games <= 0:
        raise ValueError("play_games: n_games must be positive")
    if handles == "auto":
        handles = 1
    if slots == "auto":
        per_gpu = SLOTS_PER_GPU_KEPT if reuse_subtree else SLOTS_PER_GPU
        slots = per_gpu if n_games > per_gpu and opening_plies <= 8 else None
    handles = max(1, min(int(handles), n_games))
    if not ((slots is not None and slots < n_games) or handles > 1):
        return None
    if opening_plies > 8:
        raise ValueError("play_games: slots and handles take openings of at most 8 plies")
    total_slots = n_games if slots is None else max(handles, min(int(slots), n_games))
    blocks = [((n_games * i) // handles, (n_games * (i + 1)) // handles) for i in range(handles)]
    return [(lo, hi, min(hi - lo, -(-total_slots // handles))) for lo, hi in blocks]


# ---- the rules every game loop below shares, each defined once ("Host-side pieces") ----
def _device(device):
    """(torch device, the handle of its current stream) of a game loop, the library initialised on it; None = the current device."""
    G.init(torch.cuda.current_device() if device is None else device.index)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return dev, torch.cuda.current_stream(dev).cuda_stream


def _opening(n_games, seed, first_game_id, opening_plies):
    """(moves uint8[n, 225], lens int32[n]): game g opens with the first opening_plies plies of the synthetic game first_game_id + g
    (fewer where that game is shorter); zeros past an opening's end."""
    moves, lens = np.zeros((n_games, N), dtype=np.uint8), np.zeros(n_games, dtype=np.int32)
    if opening_plies > 0 and n_games > 0:
        m, l, _ = G.synth_boards(n_games, 0, seed=seed, first_board=first_game_id)
        lens = np.minimum(l, opening_plies).astype(np.int32)
        moves[:, :m.shape[1]] = np.where(np.arange(m.shape[1])[None, :] < lens[:, None], m, 0)
    return moves, lens


def _last_two(moves, lens):
    """int16[n, 2]: the last move of every row and the one before it, -1 where there is none"""
    last = np.full((len(lens), 2), -1, dtype=np.int16)
    g = np.arange(len(lens))
    has1, has2 = lens > 0, lens > 1
    last[has1, 0] = moves[g[has1], lens[has1] - 1]
    last[has2, 1] = moves[g[has2], lens[has2] - 2]
    return last


# Default nodes per game of a searcher, by entry point: (nodes a playout can add, spare nodes, clamped to the 24-bit node index).  The spellings
# differ for no recorded reason (K3 expands 225 children and is not clamped, K6 / K8 count the root's 226th); they are kept as they were.
_ARENA = {"games": (N, 1, False), "supervisor": (226, 1, True), "network": (N, 1, True), "match": (226, 256, True)}


def _arena_nodes(entry, playouts, kept_subtree=False, node_capacity=None):
    """node_capacity if given, else the default of `entry` (_ARENA) for searches of `playouts` playouts: one search's worth of nodes, three
    with kept subtrees."""
    if node_capacity is not None:
        return node_capacity
    per_playout, spare, clamped = _ARENA[entry]
    nodes = (3 if kept_subtree else 1) * playouts * per_playout + spare
    return min(nodes, (1 << 24) - 1) if clamped else nodes


def _arena_full(status, bit):
    """Whether a tree arena filled up in some search: `bit` (the handle class's STATUS_ARENA_FULL) in root_stats()' status words."""
    return bool((status & bit).any())


def _record_tensors(n_games, dev, opening=None, visits=True):
    """(moves uint8[n, 225], lens int32[n], winner int8[n], visits int16[n, 225, 225] or None) on the device for a device-resident loop
    to fill: zeros, or the games' openings = host arrays (moves, lens) as _opening returns and _HostGames holds them."""
    d_moves = torch.zeros((n_games, N), dtype=torch.uint8, device=dev) if opening is None else torch.from_numpy(opening[0]).to(dev)
    d_lens = torch.zeros(n_games, dtype=torch.int32, device=dev) if opening is None else torch.from_numpy(opening[1]).to(dev)
    d_winner = torch.zeros(n_games, dtype=torch.int8, device=dev)
    return d_moves, d_lens, d_winner, torch.zeros((n_games, N, N), dtype=torch.int16, device=dev) if visits else None


def _records_from_host(games, visits, dev, first_game_id, overflow):
    """The GameRecords of a host-driven loop: its _HostGames and its ledger visits uint16[n, 225, 225], carried as int16 like the device's"""
    return GameRecords(torch.from_numpy(games.moves).to(dev), torch.from_numpy(games.lens).to(dev), torch.from_numpy(games.winner).to(dev),
                       torch.from_numpy(visits.view(np.int16)).to(dev), first_game_id, overflow)


def _hand_over(active, over, waiting):
    """Continuous batching on the host: active int[slots] = the game in each slot, over bool[n], waiting = the games not started yet, a list in
    game order.  The lowest slots whose game is over take the next waiting games (both changed in place); returns bool[slots], the slots
    that changed hands."""
    take = np.nonzero(over[active])[0][:len(waiting)]
    active[take] = waiting[:len(take)]
    del waiting[:len(take)]
    fresh = np.zeros(len(active), dtype=bool)
    fresh[take] = True
    return fresh


def _agent_tree(kind, kw, n, cap, seed, first_game_id):
    """The lib handle of n searches by an agent of the reference's schedule (agents/__init__.py AGENT_MAP, config.py:9-19): kind
    "traditional_mcts" (K6; with kw["use_rave"] K6 + RAVE, TraditionalAgent(c_puct, c_bias, use_rave=True), agents/mcts.py:44-47), "rave_mcts" (K8)
    or "random_mcts" (K3), kw its c_puct / c_bias / c_rollouts, cap its nodes per game.  None for a name it does not know."""
    c_puct = float(kw.get("c_puct", 5.0))
    if kind == "traditional_mcts" and kw.get("use_rave"):
        return G.TraditionalRAVEMCTS(n, node_capacity=cap, c_puct=c_puct, c_bias=float(kw.get("c_bias", 0.0)))
    if kind == "traditional_mcts":
        return G.TraditionalMCTS(n, node_capacity=cap, c_puct=c_puct)
    if kind == "rave_mcts":
        return G.PoolRAVEMCTS(n, node_capacity=cap, c_puct=c_puct, seed=seed, first_game_id=first_game_id)
    if kind == "random_mcts":
        return G.BatchedMCTS(n, c_puct=c_puct, c_rollouts=int(kw.get("c_rollouts", 5)), seed=seed, node_capacity=cap)
    return None


def play_games(n_games, playouts, seed=G.DEFAULT_SEED, first_game_id=0, c_puct=5.0, c_rollouts=5,
               opening_plies=0, record_visits=True, reuse_subtree=False, root_noise=None, max_moves=N, device=None,
               node_capacity=None, slots="auto", handles="auto", noise_sampler="counter", lockstep=False, prepare_only=False,
               sample_plies=0, sample_power=1):
    """Plays n_games complete games on the current GPU: every move = one K3 search of `playouts` playouts for all
    unfinished games, then `gmk_mcts_advance`.  Game g uses the global id first_game_id + g for its RNG streams, so
    the records do not depend on how games are spread over GPUs, slots or handles.
    slots: at most that many games in flight, with CONTINUOUS BATCHING on the device (gmk_selfplay_run): a slot whose game ends takes
    the next unstarted game inside the step kernel, so the searches stay full instead of waiting for the longest game of the batch.
    "auto" = SLOTS_PER_GPU when there are more games than that, else all games at once; None = all games at once.
    handles: the games are split into that many contiguous blocks, each with its own search handle, HIP stream and host thread
    (the slots are shared out between them); "auto" = 1 (one persistent launch fills the chip, see SLOTS_PER_GPU).
    reuse_subtree + root_noise=(alpha, epsilon) are the reference agent's per-move semantics (agents/mcts.py:17-21: the chosen child's subtree is
    the next search's tree, MCTS.cpp:129-147, and Default::AddNoise runs before every search, MCTS.cpp:182).  noise_sampler: "counter" = the
    counter-based Dirichlet sampler of include/gomoku_noise.h, drawn inside the searching kernel, so that the whole run is ONE persistent launch
    (slots / handles != None); "std" = std::gamma_distribution on the host, which needs a launch boundary per move (lock step).  lockstep=True
    forces the search-by-search loop (the form the tests hold the persistent one to).
    prepare_only: create the search handles this call would create, allocate their tree arenas and give them back -- to the library's block pool,
    where the same call without prepare_only finds them (the arenas are tens of GB, and the driver clears memory it has handed out before at seconds
    per 24 GB: a self-play job pays that once, not per batch; a measurement keeps it out of its timed region this way).  Returns None.
    sample_plies = S > 0: a game plays its first S plies (openings count) in proportion to visits^sample_power (1, 2, 3 = temperature 1, 1/2, 1/3)
    and the most visited child afterwards (lib.BatchedMCTS.advance(sample=), include/gomoku_sample.h): the draw is keyed by seed, the game's
    global id and its stone count, so the records are the same on every path and a ply's visit row gives its move again."""
    sample = _sample_schedule("play_games", sample_plies, sample_power)
    dev, stream = _device(device)
    cap = _arena_nodes("games", playouts, reuse_subtree, node_capacity)
    # (the device-resident loop plays whole games: a cap on the moves per game takes the lock-step path below, which honours it)
    plan = plan_games(n_games, slots, handles, opening_plies, reuse_subtree) if max_moves >= N else None
    if plan is None and max_moves >= N and opening_plies <= 8 and not lockstep:
        plan = [(0, n_games, n_games)]                  # all games at once, the loop on the device all the same (gmk_selfplay_run: ONE launch where it can)
    if plan is None and prepare_only:
        return None
    open_moves, open_lens = _opening(n_games, seed, first_game_id, opening_plies)
    d_moves, d_lens, d_winner, d_visits = _record_tensors(n_games, dev, (open_moves, open_lens) if plan is None else None, record_visits)
    noise = root_noise if reuse_subtree else None       # Default::AddNoise at the start of every search (MCTS.cpp:182)
    trees = []
    try:
        for _, _, n_slots in plan or [(0, n_games, n_games)]:
            trees.append(G.BatchedMCTS(n_slots, c_puct=c_puct, c_rollouts=c_rollouts, seed=seed, node_capacity=cap))
            trees[-1].set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS[noise_sampler])
        if plan is None:
            tree = trees[0]
            tree.set_roots(G.moves_to_planes(open_moves, open_lens), _last_two(open_moves, open_lens)[:, 0], first_game_id)
            d_unfinished = torch.ones(1, dtype=torch.int32, device=dev)
            for _ in range(max_moves):
                if noise is not None:
                    tree.add_root_noise(noise[0], noise[1], stream)
                tree.run(playouts, stream)
                tree.advance(d_moves.data_ptr(), d_visits.data_ptr() if record_visits else None, d_lens.data_ptr(),
                             d_winner.data_ptr(), d_unfinished.data_ptr(), reuse_subtree, stream, sample)
                if int(d_unfinished.item()) == 0:             # 4-byte readback per move: the only host sync in the loop
                    break
        else:
            for tree in trees:
                tree.set_option(G.OPT_LOCKSTEP, int(bool(lockstep)))
            if prepare_only:
                persistent = not lockstep and not (noise is not None and noise_sampler != "counter")
                for tree in trees:
                    tree.reserve(two_arenas=reuse_subtree and persistent)
                return None
            if opening_plies <= 0:                       # (the records stay zero: the loop is handed no opening at all)
                open_moves = open_lens = None

            def run_block(i, hip_stream):
                lo, hi, _ = plan[i]
                trees[i].selfplay_run(hi - lo, first_game_id + lo, playouts, d_moves[lo:].data_ptr(), d_visits[lo:].data_ptr() if record_visits else None,
                                      d_lens[lo:].data_ptr(), d_winner[lo:].data_ptr(), None if open_moves is None else open_moves[lo:hi],
                                      None if open_lens is None else open_lens[lo:hi], reuse_subtree, noise, hip_stream, sample)

            _on_streams(run_block, len(trees), dev, stream)
        overflow = any([_arena_full(tree.root_stats()[4], G.BatchedMCTS.STATUS_ARENA_FULL) for tree in trees])
    finally:
        for tree in trees:
            tree.close()
    return GameRecords(d_moves, d_lens, d_winner, d_visits, first_game_id, overflow)


def _sample_schedule(who, sample_plies, sample_power):
    """(plies, power) of a self-play loop's sampled plies, None for sample_plies = 0; the bounds are the C-ABI's"""
    if not (0 <= int(sample_plies) <= N and 1 <= int(sample_power) <= 3):
        raise ValueError("%s: sample_plies takes 0 .. 225 and sample_power 1, 2 or 3" % who)
    return (int(sample_plies), int(sample_power)) if int(sample_plies) > 0 else None


def _on_streams(run, n, dev, stream):
    """run(i, hip_stream) for i < n: on `stream` when n is 1, otherwise each on a HIP stream and a host thread of its own (run returns with
    its stream drained); a failure of any is raised."""
    if n == 1:
        return run(0, stream)
    import threading
    torch.cuda.current_stream(dev).synchronize()          # what the caller zeroed on its stream is there before another stream writes it
    side = [torch.cuda.Stream(dev) for _ in range(n)]
    failed = [None] * n

    def worker(i):
        try:
            torch.cuda.set_device(dev)                     # the HIP device is a property of the thread
            run(i, side[i].cuda_stream)
        except BaseException as exc:
            failed[i] = exc

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for exc in failed:
        if exc is not None:
            raise exc


class _HostGames:
    """The boards of n games on the host, all games handled at once with numpy (no Python loop per game): Board::applyMove with
    its victory check (Game.cpp:37-49, 88-136: five or more through the new stone wins, a full board is a tie) for the moves a
    batched searcher just chose.  The searchers only propose legal moves; `over` games take none."""

    def __init__(self, n):
        self.n = n
        self.moves = np.zeros((n, N), dtype=np.uint8)
        self.lens = np.zeros(n, dtype=np.int32)
        self.stones = np.zeros((n, 15, 15), dtype=np.int8)      # +1 black, -1 white
        self.over = np.zeros(n, dtype=bool)
        self.winner = np.zeros(n, dtype=np.int8)

    def apply(self, played):
        """played int[n]: the cell each game plays, -1 for none; returns the indices of the games that moved."""
        played = np.asarray(played)
        idx = np.nonzero((played >= 0) & ~self.over)[0]
        if len(idx) == 0:
            return idx
        cells = played[idx].astype(np.int64)
        y, x = cells // 15, cells % 15
        colour = np.where(self.lens[idx] % 2 == 0, 1, -1).astype(np.int8)      # black moves on even stone counts
        assert (self.stones[idx, y, x] == 0).all(), "a searcher proposed an occupied cell"
        self.stones[idx, y, x] = colour
        self.moves[idx, self.lens[idx]] = cells
        self.lens[idx] += 1
        five = np.zeros(len(idx), dtype=bool)
        for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
            run = np.ones(len(idx), dtype=np.int32)
            for sign in (1, -1):
                alive = np.ones(len(idx), dtype=bool)
                for k in range(1, 5):
                    yy, xx = y + sign * k * dy, x + sign * k * dx
                    inside = (yy >= 0) & (yy < 15) & (xx >= 0) & (xx < 15)
                    alive &= inside
                    alive[alive] = self.stones[idx[alive], yy[alive], xx[alive]] == colour[alive]
                    run += alive
            five |= run >= 5
        self.winner[idx[five]] = colour[five]
        self.over[idx] = five | (self.lens[idx] == N)
        return idx

    @classmethod
    def opened(cls, n_games, seed, first_game_id, opening_plies):
        """n_games boards after their openings (_opening), played ply by ply: an opening that ends its game stops there"""
        return cls.from_opening(*_opening(n_games, seed, first_game_id, opening_plies))

    @classmethod
    def from_opening(cls, moves, lens):
        """The boards after the openings (moves uint8[n, 225], lens int32[n]), played ply by ply: an opening that ends its game stops there"""
        games = cls(len(lens))
        for i in range(int(lens.max()) if len(lens) else 0):
            games.apply(np.where(lens > i, moves[:, i].astype(np.int64), -1))
        return games

    def last_two(self, rows=None):
        """int16[len(rows), 2]: the last move and the one before it of the games `rows` (default: all of them), -1 where there is none"""
        return _last_two(self.moves, self.lens) if rows is None else _last_two(self.moves[rows], self.lens[rows])

    def play(self, active, best, rows, visits, stall_ends_game=True, movers=None):
        """The ledger step of a host-driven loop.  active int[k]: the game in each slot of a searcher; best int[k]: the cell the searcher
        chose per slot, -1 for none; rows [k, 225]: its root visit counts per slot; movers bool[k] or None: the slots whose side is to move
        (the others neither play nor stall).  Games that are over take nothing.  A mover without a cell has nothing to play: its game is
        marked over, or left standing with stall_ends_game=False.  The moves are applied and each mover's row, saturated at 65 535, goes to
        visits uint16[n, 225, 225] at the ply its move was made.  Returns int16[k]: the cell that went in per slot, -1 where nothing moved."""
        active = np.asarray(active)
        live = ~self.over[active] if movers is None else movers & ~self.over[active]
        step = np.where(live, best, -1)
        if stall_ends_game:
            self.over[active[live & (step < 0)]] = True
        played = np.full(self.n, -1, dtype=np.int64)
        played[active] = step
        at = self.lens.copy()                                    # a row belongs to the position it was searched from
        moved = self.apply(played)
        slot_of = np.full(self.n, -1, dtype=np.int64)
        slot_of[active] = np.arange(len(active))
        visits[moved, at[moved]] = np.minimum(rows[slot_of[moved]], 65535)
        return step.astype(np.int16)


# play_supervisor_games' policy names: the reference agent (name, kwargs) each stands for, in the vocabulary of _agent_tree
_POLICY_AGENTS = {"traditional": ("traditional_mcts", {}), "poolrave": ("rave_mcts", {}), "traditional_rave": ("traditional_mcts", {"use_rave": True})}
_POLICIES = tuple(_POLICY_AGENTS)


def _supervisor_tree(policy, n, playouts, c_puct, seed, first_game_id, reuse_subtree, node_capacity, noise_sampler):
    """The batched searcher of play_supervisor_games' policy: MCTS(TraditionalPolicy) (K6), MCTS(PoolRAVEPolicy) (K8) or
    MCTS(TraditionalPolicy(use_rave=True)) (K6 with RAVE::BackPropogate<true>).  PoolRAVE games draw their root noise with "std"."""
    if policy not in _POLICY_AGENTS:
        raise ValueError("play_supervisor_games: policy must be one of %s" % (_POLICIES,))
    kind, kw = _POLICY_AGENTS[policy]
    tree = _agent_tree(kind, dict(kw, c_puct=c_puct), n, _arena_nodes("supervisor", playouts, reuse_subtree, node_capacity), seed, first_game_id)
    try:
        tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["std" if policy == "poolrave" else noise_sampler])
    except BaseException:
        tree.close()
        raise
    return tree


def _play_supervisor_on_device(n_games, n_slots, playouts, c_puct, seed, first_game_id, opening_plies, device, node_capacity, policy, reuse_subtree, root_noise, max_steps=0,
                               persistent=False, noise_sampler="std", prepare_only=False, sample=None):
    """play_supervisor_games with the loop resident on the device (gmk_trad_selfplay_run): the searches, MCTS::stepForward's move, the
    end-of-game check and the hand-over of a finished game's slot are kernels; the host reads four bytes per move.  Same games, same
    records as the host-driven loops below (tests/test_selfplay_gpu.py holds them to each other)."""
    dev, stream = _device(device)
    open_moves, open_lens = _opening(n_games, seed, first_game_id, opening_plies) if opening_plies > 0 else (None, None)
    tree = _supervisor_tree(policy, n_slots, playouts, c_puct, seed, first_game_id, reuse_subtree, node_capacity, noise_sampler)
    try:
        if prepare_only:                                         # the arenas this run would allocate go to the library's pool (see play_games)
            tree.reserve(two_arenas=bool(reuse_subtree and persistent))
            return None
        d_moves, d_lens, d_winner, d_visits = _record_tensors(n_games, dev)
        torch.cuda.current_stream(dev).synchronize()
        _, overflow = tree.selfplay_run(n_games, first_game_id, playouts, d_moves.data_ptr(), d_visits.data_ptr(), d_lens.data_ptr(), d_winner.data_ptr(),
                                        open_moves, open_lens, reuse_subtree, root_noise, seed, stream, max_steps, persistent, sample)
    finally:
        tree.close()
    return GameRecords(d_moves, d_lens, d_winner, d_visits, first_game_id, overflow)


def play_supervisor_games(n_games, playouts, c_puct=5.0, seed=G.DEFAULT_SEED, first_game_id=0, opening_plies=0, max_moves=N,
                          device=None, node_capacity=None, reuse_subtree=False, root_noise=None, policy="traditional", slots=None, device_loop=True, max_steps=0,
                          noise_sampler="counter", prepare_only=False, sample_plies=0, sample_power=1):
    """n_games complete games of the reference's self-play SUPERVISOR against itself (config.py:9-12: "traditional_mcts",
    MCTS(TraditionalPolicy) on both sides), all games side by side on the current GPU: every move = one K6 search of
    `playouts` playouts per unfinished game (the games' evaluators are kept and synchronised like the policy objects of
    the reference; with reuse_subtree the chosen child's subtree is kept too, MCTS::stepForward, and root_noise =
    (alpha, epsilon) mixes Default::AddNoise into the root priors before every search), then MCTS::stepForward's choice
    is played.  Without noise the search is deterministic; variety then comes from the openings (synthetic generator,
    `opening_plies` plies of game first_game_id + g).  policy="poolrave" plays the same loop with MCTS(PoolRAVEPolicy)
    (agents/mcts.py:36-40) on both sides: K8 searches, random rollouts seeded by (seed, first_game_id + g).  policy="traditional_rave"
    plays it with MCTS(TraditionalPolicy(use_rave=True)) (agents/mcts.py:44-47): K6 searches with RAVE::BackPropogate<true>, on every loop.
    slots: at most that many games are in flight; a game that ends hands its slot -- tree arena, evaluator,
    wavefront -- to the next unstarted game, so the GPU stays full instead of waiting for the longest game of the batch (a search
    costs the same time however many of its games are still alive: one wavefront per game, latency bound).
    device_loop (default): the loop runs on the device (gmk_trad_selfplay_run; whole games only, so a max_moves cap takes the host loop);
    device_loop=False: the host drives it ply by ply with numpy boards (root_stats down, positions up every ply) -- the same games.
    Known gap: through slots (slots < n_games) the host-driven loop plays every game to its end and does not look at max_moves.
    max_steps > 0 (device loop only): stop after that many moves per slot, whatever is unfinished (throughput measurements with every slot busy).
    noise_sampler: "counter" (default) = the counter-based Dirichlet sampler of include/gomoku_noise.h, drawn on the device -- inside the ONE launch of the
    persistent loop, so that the reference agent's semantics (reuse_subtree + root_noise) run at the pace of the plain loop; "std" = std::gamma_distribution
    over std::mt19937 on the host (lock step).  PoolRAVE games draw "std" whatever is asked (their loop is lock step anyway).
    sample_plies = S > 0: a game plays its first S plies (openings count) in proportion to visits^sample_power and MCTS::stepForward()'s choice
    afterwards, for every policy and on every loop (lib.TraditionalMCTS.selfplay_run(sample=), include/gomoku_sample.h); in the host-driven loop
    the host makes the same choice from the root's row (lib.move_sample_host) and steps the trees to it.
    Returns the same GameRecords as play_games (moves, per-move root visit counts, winner), so to_samples() / gather_records() apply."""
    if policy not in _POLICIES:
        raise ValueError("play_supervisor_games: policy must be one of %s" % (_POLICIES,))
    sample = _sample_schedule("play_supervisor_games", sample_plies, sample_power)
    if device_loop and max_moves >= N:
        n_slots = n_games if slots is None else max(1, min(int(slots), n_games))
        # "persistent": one launch, every slot plays game after game at its own pace (TraditionalPolicy, whole games; kept subtrees are compacted
        # inside the launch, root noise comes from the counter-based sampler); each game on a fresh evaluator, so the records equal the all-at-once
        # loop's whatever the slots.  Chosen by itself when games outnumber slots or the reference agent's semantics are asked for and the
        # configuration allows it; device_loop="lockstep" keeps the search-by-search loop (a slot's evaluator carries over).
        if policy == "poolrave":
            noise_sampler = "std"
        noisy = root_noise is not None and reuse_subtree
        can_persist = policy in ("traditional", "traditional_rave") and not max_steps and not (noisy and noise_sampler != "counter")
        if device_loop == "persistent" and not can_persist:
            raise ValueError("play_supervisor_games: the persistent loop plays TraditionalPolicy (+ RAVE) games to their end, with root noise from the counter-based sampler only")
        persistent = can_persist and (device_loop == "persistent" or (device_loop is True and (n_slots < n_games or reuse_subtree)))
        return _play_supervisor_on_device(n_games, n_slots, playouts, c_puct, seed, first_game_id,
                                          opening_plies, device, node_capacity, policy, reuse_subtree, root_noise, max_steps, persistent, noise_sampler, prepare_only, sample)
    if prepare_only:
        return None
    if max_steps:
        raise ValueError("play_supervisor_games: max_steps is a switch of the device-resident loop")
    # One host-driven loop: all games at once are n_games slots that never change hands, for at most max_moves searches.  Through fewer
    # slots the bound is what it takes to play every game out -- max_moves is not looked at there (a known gap).
    n_slots = int(slots) if slots is not None and slots < n_games else n_games
    steps = max_moves if n_slots == n_games else (n_games // n_slots + 2) * N
    dev, stream = _device(device)
    games = _HostGames.opened(n_games, seed, first_game_id, opening_plies)      # host boards: Board::applyMove / checkGameEnd for all games at once
    tree = _supervisor_tree(policy, n_slots, playouts, c_puct, seed, first_game_id, reuse_subtree, node_capacity, noise_sampler)
    try:
        visits, overflow = _supervisor_host_loop(tree, games, n_slots, steps, playouts, reuse_subtree, root_noise, seed, first_game_id, stream, sample)
    finally:
        tree.close()
    return _records_from_host(games, visits, dev, first_game_id, overflow)


def _supervisor_choice(st, stones, games, sample, seed, first_game_id):
    """The cell every slot of a K6 / K8 searcher plays from its root_stats() `st`: MCTS::stepForward()'s choice (st["best"]), or with sample =
    (plies, power) the cell the sampled step kernels draw (lib.move_sample_host) where the root has fewer than `plies` stones and its row has
    weight.  stones int[k], games int[k]: the stones on the slots' root boards and the numbers of their games."""
    if sample is None:
        return st["best"]
    plies, power = sample
    ids = (first_game_id + np.asarray(games, dtype=np.int64)) & 0xFFFFFFFF
    drawn = G.move_sample_host(st["visits"], stones, ids, plies, power, seed)
    return np.where((np.asarray(stones) < plies) & (st["visits"].max(1) > 0), drawn, st["best"]).astype(st["best"].dtype)


def _supervisor_host_loop(tree, games, slots, steps, playouts, reuse_subtree, root_noise, seed, first_game_id, stream, sample=None):
    """The host-driven loop of play_supervisor_games: the games of `games` (a _HostGames) through `slots` slots of `tree`, at most `steps`
    searches; a finished game hands its slot to the next unstarted one.  sample = (plies, power): the host chooses the sampled plies' moves
    (_supervisor_choice) and the trees step to them.  Returns (visits uint16[n, 225, 225], whether an arena filled up)."""
    visits = np.zeros((games.n, N, N), dtype=np.uint16)
    active, waiting = np.arange(slots), list(range(slots, games.n))      # the game in each slot, the games not started yet
    fresh = np.ones(slots, dtype=bool)                           # slots whose game starts from a new root at the next search
    overflow = False
    for _ in range(steps):
        fresh |= _hand_over(active, games.over, waiting)
        if games.over[active].all():
            break
        tree.set_game_ids(active)                                # root noise and rollout streams are the GAME's (first_game_id + its number), whatever slot it runs in
        if not reuse_subtree:
            tree.set_positions(games.moves[active], games.lens[active])
        elif fresh.any():                                        # the others keep the subtree gmk_trad_step left them
            tree.set_positions(games.moves[active], np.where(fresh, games.lens[active], -1))
        fresh[:] = False
        if root_noise is not None:
            tree.add_root_noise(root_noise[0], root_noise[1], seed=seed, first_game_id=first_game_id, stream=stream)
        tree.run(playouts, stream)
        st = tree.root_stats()
        overflow |= _arena_full(st["status"], G.TraditionalMCTS.STATUS_ARENA_FULL)
        best = _supervisor_choice(st, games.lens[active], active, sample, seed, first_game_id)
        step = games.play(active, best, st["visits"], visits)          # a root without a child: nothing the policy wants to play (cannot happen on a live board)
        if reuse_subtree:
            tree.step(step)                                      # finished games ask for -1 on a childless root: nothing moves
    return visits, overflow


def _vcf_options(vcf):
    """vcf = (depth, budget) or None -> the keywords of lib.AlphaZeroMCTS that switch the solver at the leaves on"""
    if vcf is None:
        return {}
    depth, budget = vcf
    return {"vcf_depth": int(depth), "vcf_budget": int(budget)}


def _root_choice(visits, proofs=None):
    """The cell every game plays from its root's visit counts [n, 225] (-1: none): the most visited child, first maximum in cell order
    (MCTS::stepForward()'s max_element).  proofs int8[n, 225] (lib.AlphaZeroMCTS.root_proofs()["children"]): the root-choice rule of "K7 + proofs",
    as the kernels apply it -- the first child that is a proven loss for its mover; otherwise the most visited child that is not a proven win
    for its mover and has a visit; otherwise the rule above."""
    best = np.where(visits.max(1) > 0, visits.argmax(1), -1)
    if proofs is not None:
        unproven = np.where(proofs == G.AZ_PROOF_WINS, 0, visits)
        best = np.where(unproven.max(1) > 0, unproven.argmax(1), best)
        loses = proofs == G.AZ_PROOF_LOSES
        best = np.where(loses.any(1), loses.argmax(1), best)
    return best


def _sampled_choice(visits, proofs, stones, games, sample):
    """_root_choice for the host-driven loops of play_network_games: with sample = (plies, power, seed, first_game_id) the choice
    gmk_az_advance_sampled makes on the device (lib.move_sample_host), for roots with `stones` stones that belong to the games numbered `games`."""
    if sample is None:
        return _root_choice(visits, proofs)
    plies, power, seed, first_game_id = sample
    ids = (first_game_id + np.asarray(games, dtype=np.int64)) & 0xFFFFFFFF
    return G.move_sample_host(visits, stones, ids, plies, power, seed, proofs).astype(np.int64)


def _symmetric(who, network, symmetry, seed):
    """`network` as the loops of `who` call it: itself for symmetry None, network.symmetric(symmetry, seed) for "random" or "all" (K22)."""
    if symmetry is None:
        return network
    if symmetry not in ("random", "all"):
        raise ValueError("%s: symmetry is None, \"random\" or \"all\", not %r" % (who, symmetry))
    if not hasattr(network, "symmetric"):
        raise ValueError("%s: symmetry needs a network with symmetric(mode, seed) (network.FusedPolicyValueNetwork)" % who)
    return network.symmetric(symmetry, seed)


def _gumbel_goes_with(who, root_noise, leaves, proof, vcf_defend, sample_plies):
    """ValueError for what the Gumbel root search (K21) of a loop `who` does not go with: root noise, leaves > 1, proofs, sampled plies."""
    if root_noise is not None:
        raise ValueError("%s: gumbel does not go with root noise -- pass root_noise=None, the Gumbel noise is the exploration" % who)
    for name, bad in (("leaves > 1", leaves != 1), ("proof", proof), ("vcf_defend", vcf_defend), ("sample_plies > 0", int(sample_plies) > 0)):
        if bad:
            raise ValueError("%s: gumbel does not go with %s (the Gumbel root search takes one leaf per step, carries no proofs "
                             "and chooses its moves itself)" % (who, name))


def play_network_games(n_games, network, playouts, c_puct=5.0, seed=G.DEFAULT_SEED, first_game_id=0, opening_plies=0, max_moves=N,
                       device=None, node_capacity=None, reuse_subtree=True, root_noise=(0.05, 0.25), slots=None, device_loop=True, noise_sampler="counter", leaves=1,
                       vcf=None, proof=False, vcf_defend=False, sample_plies=0, sample_power=1, symmetry=None, gumbel=None):
    """n_games complete games of the network-guided searcher against itself (agents/alphazero.py:5-9 on both sides: the
    reference's AlphaZero self-play), all games in lock step on the current GPU: every move = `playouts` lock-step playouts of
    K7 with `network(states [n,6,15,15]) -> (value [n], probs [n,225])` at the leaves (network.FusedPolicyValueNetwork = K9),
    then every game plays its most visited child (MCTSAgent.eval_state -> MCTS::stepForward); with reuse_subtree the child's
    subtree is kept and root_noise = (alpha, epsilon) is mixed into the root priors before every search (MCTS.cpp:182).
    slots: at most that many games in flight, a finished game hands its slot to the next one (see play_supervisor_games; on the
    host-driven loop with fresh roots only).  device_loop (all games at once): the move, the record, the end-of-game check and the re-rooting are one
    kernel per ply (gmk_az_advance) and the host sees four bytes per move; noise_sampler "counter" (default) draws the root noise on the device
    (az_root_noise_kernel, include/gomoku_noise.h), "std" on the host with std::gamma_distribution (priors down and up every ply); False = the host-driven loop it replaced (numpy boards, root statistics down and moves up every ply), kept for the
    tests that compare the two.  leaves > 1: every search step takes up to that many leaves from each game, with virtual loss
    (lib.AlphaZeroMCTS(leaves=)): the network's batch is live games x leaves rows and a move takes about playouts / leaves steps; the games differ
    from those of leaves = 1, and are the same games on every loop of this function.  vcf = (depth, budget): the searches solve forced wins by
    fours at their leaves (lib.AlphaZeroMCTS(vcf_depth=, vcf_budget=)); None: they do not.  proof: the searches carry proven wins and losses up
    their trees and every loop chooses its moves by them (lib.AlphaZeroMCTS(proof=), _root_choice).  vcf_defend (with vcf and proof): the replies
    that lose to the opponent's forced win by fours are proven at the leaves (lib.AlphaZeroMCTS(vcf_defend=)); such a search spends its playouts
    below the few replies that hold, so a kept subtree stays nearly whole while the replies are forced: give node_capacity room (the records'
    overflow says when an arena filled).  sample_plies = S > 0: a game plays its first S plies (openings count) in proportion to
    visits^sample_power (1, 2, 3: temperature 1, 1/2, 1/3) and its most visited child afterwards, AlphaZero's self-play schedule
    (lib.AlphaZeroMCTS.advance(sample=), include/gomoku_sample.h): the draw is keyed by seed, the game's global id and its stone count, so
    these too are the same games on every loop, and a record's visit row gives its move again.  symmetry = "random" or "all": the leaves are
    evaluated through network.symmetric(symmetry, seed) -- one orientation of the board per leaf, picked from the leaf's position and `seed`, or
    the average over all eight (K22, include/gomoku_symmetry.h); the pick does not depend on a row's place in the batch, so these are the same
    games on every loop as well.  None: `network` as it is.
    gumbel = (max_considered, c_visit, c_scale): Gumbel AlphaZero at the root (K21, include/gomoku_gumbel.h; lib.AlphaZeroMCTS(gumbel=)) with
    n_sims = playouts -- the playouts of a move go to the Gumbel-top-m root children by sequential halving, the move is the rule's, and the
    records' rows are improved-policy rows, to be read with target="policy" (GameRecords.to_samples, ReplayBuffer).  The draws are keyed by seed,
    the game's global id and its stone count, so every loop plays the same games, rows included.  The Gumbel noise is the exploration:
    root_noise must be None, and leaves > 1, proof, vcf_defend and sample_plies > 0 do not go with it (ValueError).  Playing strength against
    the plain search: first figures in profiles/agent_match.json (play_agent_match).  Returns GameRecords like play_games."""
    if not (0 <= int(sample_plies) <= N and 1 <= int(sample_power) <= 3):
        raise ValueError("play_network_games: sample_plies takes 0 .. 225 and sample_power 1, 2 or 3")
    gumbel_args = None
    if gumbel is not None:
        _gumbel_goes_with("play_network_games", root_noise, leaves, proof, vcf_defend, sample_plies)
        m, c_visit, c_scale = gumbel
        gumbel_args = (int(m), int(playouts), float(c_visit), float(c_scale), seed, first_game_id)
    network = _symmetric("play_network_games", network, symmetry, seed)
    sample = (int(sample_plies), int(sample_power), seed, first_game_id) if int(sample_plies) > 0 else None
    if slots is not None and slots < n_games and (max_moves < N or (device_loop and opening_plies > 8)):
        # (the slot loops play whole games, the device-resident one from openings of at most 8 plies -- gmk_az_set_slots' limit: say so instead of
        # ignoring the cap or failing inside the library)
        raise ValueError("play_network_games: with slots, games are played to their end (max_moves >= 225)" +
                         (" from openings of at most 8 plies on the device loop" if device_loop else "") + "; play all games at once (slots=None) for a move cap")
    slotted = slots is not None and slots < n_games
    if slotted and not device_loop and reuse_subtree:
        raise ValueError("play_network_games: slots on the host-driven loop need fresh roots (reuse_subtree=False)")
    n_slots = int(slots) if slotted else n_games
    steps = (n_games // n_slots + 2) * N if slotted else max_moves
    dev, _ = _device(device)
    games = _HostGames.opened(n_games, seed, first_game_id, opening_plies)
    tree = G.AlphaZeroMCTS(n_slots, node_capacity=_arena_nodes("network", playouts, reuse_subtree, node_capacity), c_puct=c_puct, leaves=leaves, proof=proof,
                           vcf_defend=vcf_defend, gumbel=gumbel_args, **_vcf_options(vcf))
    try:
        tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS[noise_sampler])
        with torch.no_grad():
            if not device_loop:
                # (through slots the host-driven loop has never mixed noise into its fresh roots: kept as it is)
                visits, overflow = _network_host_loop(tree, games, n_slots, steps, network, playouts, reuse_subtree, None if slotted else root_noise,
                                                      proof, sample, seed, first_game_id, gumbel is not None)
                return _records_from_host(games, visits, dev, first_game_id, overflow)
            if slotted:
                # continuous batching on the device (gmk_az_set_slots + gmk_az_advance): the batch the network sees stays full of live games
                # until fewer games than slots remain, with kept subtrees and root noise as well
                tree.set_slots(n_games, games.moves[:, :max(int(games.lens.max()), 1)], games.lens)
            else:
                tree.set_roots(G.moves_to_planes(games.moves, games.lens), games.last_two())
            d_moves, d_lens, d_winner, d_visits = _record_tensors(n_games, dev, (games.moves, games.lens))
            for _ in range(steps):
                if root_noise is not None:
                    tree.add_root_noise(root_noise[0], root_noise[1], seed=seed, first_game_id=first_game_id)
                tree.search(network, playouts)
                if tree.advance(d_moves, d_visits, d_lens, d_winner, reuse_subtree, sample=sample, gumbel=gumbel is not None) == 0:
                    break
        overflow = _arena_full(tree.root_stats()["status"], G.AlphaZeroMCTS.STATUS_ARENA_FULL)
    finally:
        tree.close()
    return GameRecords(d_moves, d_lens, d_winner, d_visits, first_game_id, overflow)


def _network_host_loop(tree, games, slots, steps, network, playouts, reuse_subtree, root_noise, proof, sample, seed, first_game_id, gumbel=False):
    """The host-driven loop of play_network_games: the games of `games` (a _HostGames) through `slots` slots of the K7 handle `tree`, at
    most `steps` searches.  With kept subtrees every slot keeps its game (slots == games.n: K7 has no way to give one slot a new root and
    leave the others their trees).  gumbel: the handle's Gumbel root search is on -- the move and the row come from root_choice(gumbel=True), and
    the row recorded is its improved-policy row.  Returns (visits uint16[n, 225, 225], whether an arena filled up)."""
    visits = np.zeros((games.n, N, N), dtype=np.uint16)
    if gumbel:
        d_cells = torch.zeros(slots, dtype=torch.int16, device="cuda")
        d_rows = torch.zeros((slots, N), dtype=torch.int16, device="cuda")
    active, waiting = np.arange(slots), list(range(slots, games.n))
    overflow = False
    for i in range(steps):
        _hand_over(active, games.over, waiting)
        if games.over[active].all():
            break
        if i == 0 or not reuse_subtree:
            tree.set_game_ids(active)
            tree.set_roots(G.moves_to_planes(games.moves[active], games.lens[active]), games.last_two(active))
        if root_noise is not None:
            tree.add_root_noise(root_noise[0], root_noise[1], seed=seed, first_game_id=first_game_id)
        tree.search(network, playouts)
        st = tree.root_stats()
        overflow |= _arena_full(st["status"], G.AlphaZeroMCTS.STATUS_ARENA_FULL)
        if gumbel:
            tree.root_choice(d_cells, d_rows, gumbel=True)
            choice, rows = d_cells.cpu().numpy().astype(np.int64), d_rows.cpu().numpy().view(np.uint16)
            step = games.play(active, choice, rows, visits)
            if reuse_subtree:
                tree.step(step)
            continue
        choice = _sampled_choice(st["visits"], tree.root_proofs()["children"] if proof else None, games.lens[active], active, sample)
        visited = st["visits"].max(1) > 0                        # no child was visited: nothing to play (cannot happen on a live board)
        step = games.play(active, np.where(visited, choice, -1), st["visits"], visits)
        if reuse_subtree:
            tree.step(step)
    return visits, overflow


class _Searcher:
    """One side of play_match_games: a batched searcher for a fixed set of games, fresh roots every move."""

    def __init__(self, spec, n, playouts, seed, first_game_id):
        kind, kw = spec
        self.kind, self.n, self.playouts = kind, n, int(kw.get("c_iterations", playouts))
        self.first_game_id = first_game_id
        cap = _arena_nodes("games" if kind == "random_mcts" else "match", self.playouts)
        self.tree = _agent_tree(kind, kw, n, cap, seed, first_game_id)
        if self.tree is None:
            raise ValueError("play_match_games: unknown agent '%s' (traditional_mcts, rave_mcts, random_mcts)" % kind)

    def search(self, moves, lens, games, stream):
        """Root visit counts [n, 225] and the move MCTS::stepForward() would make per game (-1: none), from fresh roots.
        games int[n]: the number of the game in each slot; its random streams are keyed by first_game_id + that number."""
        if self.kind == "random_mcts":
            self.tree.set_roots(G.moves_to_planes(moves, lens), _last_two(moves, lens)[:, 0], self.first_game_id)
            self.tree.set_game_ids((self.first_game_id + np.asarray(games)).astype(np.uint32))
            self.tree.run(self.playouts, stream)
            stats = self.tree.root_stats()
            return stats[0], _root_choice(stats[0]).astype(np.int32), _arena_full(stats[4], G.BatchedMCTS.STATUS_ARENA_FULL)
        self.tree.set_game_ids(np.asarray(games, dtype=np.uint32))
        self.tree.set_positions(moves, lens)
        self.tree.run(self.playouts, stream)
        st = self.tree.root_stats()
        return st["visits"], st["best"], _arena_full(st["status"], G.TraditionalMCTS.STATUS_ARENA_FULL)

    def close(self):
        self.tree.close()


def play_match_games(n_games, supervisor, candidate, playouts=400, seed=G.DEFAULT_SEED, first_game_id=0, opening_plies=0,
                     max_moves=N, device=None, slots=None):
    """The reference's data generation pairing (network/data_helper.py:15-22, 56-63; config.py:6-20): every game is played by
    the SUPERVISOR against a CANDIDATE, sides drawn at random per game, and both players' searches are recorded.  supervisor /
    candidate = (name, kwargs) as in DATA_CONFIG["schedule"]: ("traditional_mcts" | "rave_mcts" | "random_mcts", {"c_puct": ..,
    "c_iterations": .., "c_rollouts": ..}); "traditional_mcts" with {"use_rave": True, "c_bias": ..} searches with TraditionalRAVEMCTS.  All games run side by side on the current GPU: the games in which the supervisor
    has black and the games in which it has white form two groups, each with one batched searcher per agent (K6 / K8 / K3), so
    that every ply is two searches (one per group) covering all unfinished games; roots are fresh at every move and every
    game's random streams are keyed by its own global id first_game_id + g, whatever group and slot it runs in.  slots: games in flight per group (default: all of them); a
    finished game hands its slot to the next unstarted game of its group, which keeps the searches full (see play_supervisor_games).
    Returns (GameRecords, supervisor_is_black bool[n]); the records' visit counts at move i are those of the player who made it."""
    dev, stream = _device(device)
    rng = np.random.RandomState(int((seed ^ (seed >> 32) ^ first_game_id) & 0xFFFFFFFF))
    sup_black = rng.randint(0, 2, n_games).astype(bool)           # random.shuffle(players) per game (data_helper.py:57-58)
    games = _HostGames.opened(n_games, seed, first_game_id, opening_plies)
    visits = np.zeros((n_games, N, N), dtype=np.uint16)
    active, waiting, searchers = [], [], []                      # per group: the game in each slot, the games not started yet, [supervisor, candidate]
    overflow = False
    with contextlib.ExitStack() as handles:
        for idx in (np.nonzero(sup_black)[0], np.nonzero(~sup_black)[0]):
            k = len(idx) if slots is None else min(int(slots), len(idx))
            active.append(idx[:k].copy())
            waiting.append(list(idx[k:]))
            searchers.append([handles.enter_context(contextlib.closing(_Searcher(spec, k, playouts, seed, first_game_id))) if k else None
                              for spec in (supervisor, candidate)])
        for _ in range((2 + (0 if slots is None else n_games // max(1, int(slots)))) * max_moves):
            if games.over.all():
                break
            for gi, act in enumerate(active):
                _hand_over(act, games.over, waiting[gi])          # a finished game hands its slot to the next one of the group
                if games.over[act].all():                         # (an empty group too)
                    continue
                for who in (0, 1):                                # normally one of the two: the games of a group move in lock step
                    # group 0: the supervisor has black, i.e. it moves on even stone counts
                    sel = (((games.lens[act] % 2 == 0) == (gi == 0)) == (who == 0)) & ~games.over[act]
                    if not sel.any():
                        continue
                    v, best, full = searchers[gi][who].search(games.moves[act], games.lens[act], act, stream)
                    overflow |= full
                    games.play(act, best, v, visits, movers=sel)
    return _records_from_host(games, visits, dev, first_game_id, overflow), sup_black


def evaluation_sides(n_games):
    """network_is_black bool[n]: eval_agents exchanges the start player after every game (agents/utils.py:82-93), so the first agent --
    the network -- has black in game i iff i is even."""
    return np.arange(int(n_games)) % 2 == 0


def evaluation_scores(winner, network_is_black):
    """eval_agents' count (agents/utils.py:84-89) per game: 1 for a win of the network, 0 for a loss, 0.5 for a tie; winner +1 black, -1 white,
    0 tie.  The win rate is their mean."""
    winner, black = np.asarray(winner).astype(np.int64), np.asarray(network_is_black, dtype=bool)
    return np.where(winner == 0, 0.5, np.where((winner > 0) == black, 1.0, 0.0))


_EVAL_OPPONENTS = ("traditional_mcts", "rave_mcts", "random_mcts")


class _EvalOpponent:
    """The opponent's side of one group of play_evaluation_games: a K6 / K8 handle that keeps its trees (or gets fresh roots), or -- on the
    host loop only -- the K3 searcher of play_match_games, which starts every search from fresh roots."""

    def __init__(self, spec, idx, moves, lens, seed, first_game_id, reuse_subtree):
        kind, kw = spec
        self.kind, self.idx, self.reuse, self.seed, self.first = kind, idx, reuse_subtree, seed, first_game_id
        self.playouts = int(kw.get("c_iterations", 400))
        self.searcher = self.tree = None
        if kind == "random_mcts":
            self.searcher = _Searcher(spec, len(idx), self.playouts, seed, first_game_id)
            return
        self.tree = _agent_tree(kind, kw, len(idx), _arena_nodes("match", self.playouts, reuse_subtree), seed, first_game_id)
        try:
            self.tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
            self.tree.set_game_ids(np.asarray(idx, dtype=np.uint32))
            self.tree.set_positions(moves, lens)
        except BaseException:
            self.tree.close()
            raise

    def add_root_noise(self, root_noise, stream=None):
        if root_noise is not None and self.tree is not None:
            self.tree.add_root_noise(root_noise[0], root_noise[1], seed=self.seed, first_game_id=self.first, stream=stream)

    def overflow(self):
        return self.tree is not None and _arena_full(self.tree.root_stats()["status"], G.TraditionalMCTS.STATUS_ARENA_FULL)

    def close(self):
        (self.tree if self.tree is not None else self.searcher).close()


def play_evaluation_games(n_games, network, opponent, playouts=400, c_puct=5.0, seed=G.DEFAULT_SEED, first_game_id=0, opening_plies=0, max_moves=N,
                          reuse_subtree=True, root_noise=(0.05, 0.25), device_loop=None, device=None, leaves=1, vcf=None, proof=False, vcf_defend=False, node_capacity=None,
                          symmetry=None):
    """The reference's evaluation match (network/train.py:88-126 evaluate_network -> agents/utils.py:66-100 eval_agents): n_games games of the
    network-guided searcher (K7 with `network` = network.FusedPolicyValueNetwork at the leaves, `playouts` playouts a move) against
    `opponent` = (name, kwargs) as in DATA_CONFIG["schedule"] ("traditional_mcts" -- with {"use_rave": True} TraditionalPolicy + RAVE --,
    "rave_mcts" or "random_mcts"; kwargs["c_iterations"] is its playout budget).  The network has black in game i iff i is even.  The games
    with the network as black and the others form two groups, each with one K7 handle and one opponent handle; every ply of a group is one
    search by the side to move, whose choice both trees follow.  reuse_subtree: each agent keeps its own tree through the game and follows the
    opponent's move by stepForward(move) (MCTS.cpp:119-147), and root_noise = (alpha, epsilon) is mixed into the mover's root priors before
    every search (MCTS.cpp:182) by the counter-based sampler keyed by first_game_id + i; otherwise every search starts from a fresh root.
    device_loop=True: root choice, referee (K12: the record, the end-of-game test) and both steps are kernels on the current stream and the
    host sees the count of unfinished games per ply; False: the same match through the host (root_stats down, numpy boards, moves up);
    None: the device loop, except for "random_mcts" (the gmk_mcts handle), which the host loop serves, from fresh roots at every move.
    A mover whose root has no child to play leaves its game where it stands (it cannot happen on a board with an empty cell).
    leaves > 1: the network's searches take up to that many leaves per game per step, with virtual loss (lib.AlphaZeroMCTS(leaves=)) -- a
    match has few games, so this is what fills the network's batch; both loops play the same games.
    vcf = (depth, budget): the network's searches -- not the opponent's -- solve forced wins by fours at their leaves
    (lib.AlphaZeroMCTS(vcf_depth=, vcf_budget=)); None: they do not.  proof: they carry proven wins and losses up their trees, and the
    network's moves are chosen by them on both loops (lib.AlphaZeroMCTS(proof=)).  vcf_defend (with vcf and proof): they also prove the
    replies that lose to the opponent's forced win by fours (lib.AlphaZeroMCTS(vcf_defend=)); it applies to the K7 handle only.  Such a search
    spends its playouts below the few replies that hold, so a kept subtree stays nearly whole while the replies are forced: node_capacity (the K7
    handle's nodes per game; None: three searches' worth with kept subtrees) makes room, and the records' overflow says when an arena filled.
    symmetry = "random" or "all": the network's leaves are evaluated through network.symmetric(symmetry, seed) (K22: one orientation per leaf, or
    the average over all eight -- a match's batch is small enough for the eight to ride on the network's launch cost); None: `network` as it is.
    Returns (GameRecords, network_is_black bool[n], scores float[n]); the records' visit counts at move i are the mover's, and
    records.groups lists per group the games, the unfinished count and the K7 handle's live games after the loop."""
    network = _symmetric("play_evaluation_games", network, symmetry, seed)
    kind = opponent[0]
    if kind not in _EVAL_OPPONENTS:
        raise ValueError("play_evaluation_games: unknown opponent '%s' (%s)" % (kind, ", ".join(_EVAL_OPPONENTS)))
    if device_loop and kind == "random_mcts":
        raise ValueError("play_evaluation_games: random_mcts (the gmk_mcts handle) is served by the host loop only: device_loop=False or None")
    if device_loop is None:
        device_loop = kind != "random_mcts"
    if opening_plies > 8:
        raise ValueError("play_evaluation_games: openings of at most 8 plies (an opening cannot be a finished game)")
    dev, stream = _device(device)
    black = evaluation_sides(n_games)
    games = _HostGames.opened(n_games, seed, first_game_id, opening_plies)
    start = int(games.lens[0]) if n_games else 0
    assert (games.lens == start).all() and not games.over.any()
    if device_loop:
        d_moves, d_lens, d_winner, d_visits = _record_tensors(n_games, dev, (games.moves, games.lens))
    else:
        visits = np.zeros((n_games, N, N), dtype=np.uint16)
    overflow, groups = False, []
    net_cap = _arena_nodes("network", playouts, reuse_subtree, node_capacity)
    for gi, idx in enumerate((np.nonzero(black)[0], np.nonzero(~black)[0])):
        k = len(idx)
        if k == 0:
            groups.append({"games": idx, "unfinished": 0, "live_games": 0})
            continue
        with contextlib.ExitStack() as handles, torch.no_grad():
            net = handles.enter_context(contextlib.closing(
                G.AlphaZeroMCTS(k, node_capacity=net_cap, c_puct=c_puct, leaves=leaves, proof=proof, vcf_defend=vcf_defend, **_vcf_options(vcf))))
            net.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
            net.set_game_ids(np.asarray(idx, dtype=np.uint32))
            net.set_roots(G.moves_to_planes(games.moves[idx], games.lens[idx]), games.last_two(idx))
            opp = handles.enter_context(contextlib.closing(_EvalOpponent(opponent, idx, games.moves[idx], games.lens[idx], seed, first_game_id, reuse_subtree)))
            unfinished = k
            if device_loop:
                d_idx = torch.from_numpy(idx.astype(np.int32)).to(dev)
                d_cells, d_rows = torch.full((k,), -1, dtype=torch.int16, device=dev), torch.zeros((k, N), dtype=torch.int16, device=dev)
                d_verdict, d_status, d_unfinished = torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            for ply in range(max_moves):
                if not device_loop and games.over[idx].all():
                    break
                net_moves = ((start + ply) % 2 == 0) == (gi == 0)             # group 0: the network has black, i.e. it moves on even stone counts
                fresh = not device_loop and ply > 0 and not reuse_subtree     # (on the device loop step_device leaves the fresh roots)
                if net_moves:
                    if fresh:
                        net.set_roots(G.moves_to_planes(games.moves[idx], games.lens[idx]), games.last_two(idx))
                    if root_noise is not None:
                        net.add_root_noise(root_noise[0], root_noise[1], seed=seed, first_game_id=first_game_id)
                    net.search(network, playouts)
                elif opp.tree is not None:
                    if fresh:
                        opp.tree.set_positions(games.moves[idx], games.lens[idx])
                    opp.add_root_noise(root_noise, stream)
                    opp.tree.run(opp.playouts, stream)
                if device_loop:
                    (net if net_moves else opp.tree).root_choice(d_cells, d_rows)
                    G.match_referee(d_cells, d_rows, d_idx, d_moves, d_lens, d_winner, d_visits, d_verdict, d_status, d_unfinished)
                    opp.tree.step_device(d_cells, d_verdict, fresh_root=not reuse_subtree)
                    unfinished = net.step_device(d_cells, d_verdict, fresh_root=not reuse_subtree, unfinished=d_unfinished)
                    if unfinished == 0:
                        break
                else:
                    if net_moves:
                        st = net.root_stats()
                        overflow |= _arena_full(st["status"], G.AlphaZeroMCTS.STATUS_ARENA_FULL)
                        v, best = st["visits"], _root_choice(st["visits"], net.root_proofs()["children"] if proof else None)
                    elif opp.tree is None:
                        v, best, full = opp.searcher.search(games.moves[idx], games.lens[idx], idx, stream)
                        overflow |= full
                    else:
                        st = opp.tree.root_stats()
                        v, best = st["visits"], st["best"]
                    step = games.play(idx, best, v, visits, stall_ends_game=False)      # a mover without a child leaves its game where it stands
                    if reuse_subtree:
                        net.step(step)
                        if opp.tree is not None:
                            opp.tree.step(step)
            if device_loop:
                overflow |= _arena_full(net.root_stats()["status"], G.AlphaZeroMCTS.STATUS_ARENA_FULL)
            else:
                unfinished = int((~games.over[idx]).sum())
            overflow |= opp.overflow()
            groups.append({"games": idx, "unfinished": unfinished, "live_games": net.live})
    if device_loop:
        rec = GameRecords(d_moves, d_lens, d_winner, d_visits, first_game_id, overflow)
        winner = d_winner.cpu().numpy()
    else:
        rec = _records_from_host(games, visits, dev, first_game_id, overflow)
        winner = games.winner
    rec.groups = groups
    return rec, black, evaluation_scores(winner, black)


_MATCH_AGENTS = _EVAL_OPPONENTS + ("network",)
_NETWORK_AGENT_KEYS = ("network", "playouts", "c_puct", "leaves", "vcf", "proof", "vcf_defend", "symmetry", "gumbel", "sample_plies", "sample_power", "node_capacity")


def _match_agent(spec, root_noise):
    """An agent spec of play_agent_match, checked without the library: (kind, kwargs), kwargs a copy.  ValueError names what is wrong."""
    who = "play_agent_match"
    try:
        kind, kw = spec
        kw = dict(kw)
    except (TypeError, ValueError):
        raise ValueError("%s: an agent is (kind, kwargs), not %r" % (who, spec)) from None
    if kind not in _MATCH_AGENTS:
        raise ValueError("%s: unknown agent '%s' (%s)" % (who, kind, ", ".join(_MATCH_AGENTS)))
    if kind == "random_mcts" and int(kw.get("c_iterations", 400)) < 2:
        raise ValueError("%s: random_mcts needs c_iterations >= 2 (the first playout only expands the root: there is no child to play)" % who)
    if kind != "network":
        return kind, kw
    unknown = sorted(set(kw) - set(_NETWORK_AGENT_KEYS))
    if unknown:
        raise ValueError("%s: a network agent takes %s, not %s" % (who, ", ".join(_NETWORK_AGENT_KEYS), ", ".join(unknown)))
    if kw.get("network") is None:
        raise ValueError("%s: a network agent needs its network (network.FusedPolicyValueNetwork)" % who)
    if kw.get("symmetry") not in (None, "random", "all"):
        raise ValueError("%s: symmetry is None, \"random\" or \"all\", not %r" % (who, kw["symmetry"]))
    _sample_schedule(who, kw.get("sample_plies", 0), kw.get("sample_power", 1))
    if kw.get("gumbel") is not None:
        _gumbel_goes_with(who, root_noise, kw.get("leaves", 1), kw.get("proof", False), kw.get("vcf_defend", False), kw.get("sample_plies", 0))
        if len(tuple(kw["gumbel"])) != 3:
            raise ValueError("%s: gumbel = (max_considered, c_visit, c_scale)" % who)
    return kind, kw


class _MatchSide:
    """One agent's side of one group of play_agent_match: its own handle over the group's games `idx`, rooted at their positions in `games`
    (a _HostGames), and the calls both loops make of it whatever the handle is -- K7 with its network and options, K6 / K6 + RAVE / K8, or K3."""

    def __init__(self, spec, idx, games, seed, first_game_id, reuse_subtree, dev):
        self.kind, kw = spec
        self.idx, self.seed, self.first = idx, seed, first_game_id
        k = len(idx)
        self.sample = self.network = None
        self.gumbel = self.proof = False
        if self.kind == "network":
            self.playouts = int(kw.get("playouts", 400))
            self.network = _symmetric("play_agent_match", kw["network"], kw.get("symmetry"), seed)
            self.proof = bool(kw.get("proof", False))
            plies = _sample_schedule("play_agent_match", kw.get("sample_plies", 0), kw.get("sample_power", 1))
            self.sample = None if plies is None else plies + (seed, first_game_id)
            gumbel_args = None
            if kw.get("gumbel") is not None:
                m, c_visit, c_scale = kw["gumbel"]
                gumbel_args, self.gumbel = (int(m), self.playouts, float(c_visit), float(c_scale), seed, first_game_id), True
            self.tree = G.AlphaZeroMCTS(k, node_capacity=_arena_nodes("network", self.playouts, reuse_subtree, kw.get("node_capacity")), c_puct=float(kw.get("c_puct", 5.0)),
                                        leaves=int(kw.get("leaves", 1)), proof=self.proof, vcf_defend=bool(kw.get("vcf_defend", False)), gumbel=gumbel_args,
                                        **_vcf_options(kw.get("vcf")))
            self.full = G.AlphaZeroMCTS.STATUS_ARENA_FULL
        else:
            self.playouts = int(kw.get("c_iterations", 400))
            k3 = self.kind == "random_mcts"
            self.tree = _agent_tree(self.kind, kw, k, _arena_nodes("games" if k3 else "match", self.playouts, reuse_subtree), seed, first_game_id)
            self.full = G.BatchedMCTS.STATUS_ARENA_FULL if k3 else G.TraditionalMCTS.STATUS_ARENA_FULL
        try:
            self.tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
            self.set_position(games, first=True)
            if self.gumbel or self.sample is not None:           # the host loop's root_choice lands here
                self.d_cells, self.d_rows = torch.zeros(k, dtype=torch.int16, device=dev), torch.zeros((k, N), dtype=torch.int16, device=dev)
        except BaseException:
            self.tree.close()
            raise

    def set_position(self, games, first=False):
        """Fresh roots at the games' positions; the games' numbers key every random stream of the handle (first: they are told once)."""
        idx = self.idx
        if self.kind == "network":
            if first:
                self.tree.set_game_ids(np.asarray(idx, dtype=np.uint32))
            self.tree.set_roots(G.moves_to_planes(games.moves[idx], games.lens[idx]), games.last_two(idx))
        elif self.kind == "random_mcts":                         # (gmk_mcts_set_roots numbers the games itself: their ids follow it every time)
            self.tree.set_roots(G.moves_to_planes(games.moves[idx], games.lens[idx]), games.last_two(idx)[:, 0], self.first)
            self.tree.set_game_ids(((self.first + np.asarray(idx, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32))
        else:
            if first:
                self.tree.set_game_ids(np.asarray(idx, dtype=np.uint32))
            self.tree.set_positions(games.moves[idx], games.lens[idx])

    def search(self, root_noise, stream):
        """Default::AddNoise on the roots that have children, if asked for, then the agent's playouts"""
        if self.kind == "network":
            if root_noise is not None:
                self.tree.add_root_noise(root_noise[0], root_noise[1], seed=self.seed, first_game_id=self.first)
            self.tree.search(self.network, self.playouts)
        elif self.kind == "random_mcts":
            if root_noise is not None:
                self.tree.add_root_noise(root_noise[0], root_noise[1], stream)
            self.tree.run(self.playouts, stream)
        else:
            if root_noise is not None:
                self.tree.add_root_noise(root_noise[0], root_noise[1], seed=self.seed, first_game_id=self.first, stream=stream)
            self.tree.run(self.playouts, stream)

    def choose_device(self, d_cells, d_rows):
        """The move of every game and its record row into device memory: greedy, sampled or the Gumbel rule's, by the spec"""
        if self.gumbel:
            self.tree.root_choice(d_cells, d_rows, gumbel=True)
        elif self.sample is not None:
            self.tree.root_choice(d_cells, d_rows, sample=self.sample)
        else:
            self.tree.root_choice(d_cells, d_rows)

    def status(self):
        st = self.tree.root_stats()
        return st[4] if self.kind == "random_mcts" else st["status"]

    def overflow(self):
        return _arena_full(self.status(), self.full)

    def choose_host(self, stones):
        """(cells int[k], -1: none; rows [k, 225]; whether an arena filled) of the same choice through the host; stones int[k] on the root boards"""
        st = self.tree.root_stats()
        if self.kind == "random_mcts":
            return _root_choice(st[0]), st[0], _arena_full(st[4], self.full)
        full = _arena_full(st["status"], self.full)
        if self.kind != "network":
            return st["best"], st["visits"], full
        if self.gumbel:
            self.tree.root_choice(self.d_cells, self.d_rows, gumbel=True)
            return self.d_cells.cpu().numpy().astype(np.int64), self.d_rows.cpu().numpy().view(np.uint16), full
        proofs = self.tree.root_proofs()["children"] if self.proof else None
        if self.sample is None:
            return _root_choice(st["visits"], proofs), st["visits"], full
        choice = _sampled_choice(st["visits"], proofs, stones, self.idx, self.sample)
        return np.where(st["visits"].max(1) > 0, choice, -1), st["visits"], full

    def step_host(self, step):
        """Both trees follow the move with their subtrees kept: step int16[k], the cell that went in"""
        if self.kind == "random_mcts":
            self.tree.step_host(step, reuse_subtree=True)
        else:
            self.tree.step(step)

    @property
    def live(self):
        return self.tree.live if self.kind == "network" else None

    def close(self):
        self.tree.close()


def play_agent_match(n_games, first, second, seed=G.DEFAULT_SEED, first_game_id=0, opening_plies=4, paired=True, max_moves=N, reuse_subtree=True,
                     root_noise=None, device_loop=True, device=None):
    """A match between any two agents the project has: n_games games of `first` against `second`, each an agent spec (kind, kwargs).
    kind "traditional_mcts" (K6; {"use_rave": True}: K6 + RAVE), "rave_mcts" (K8) and "random_mcts" (K3) as in DATA_CONFIG["schedule"] -- kwargs c_puct,
    c_bias, c_rollouts, and c_iterations, the playout budget -- or "network": K7 with kwargs network (a network.FusedPolicyValueNetwork, required),
    playouts, c_puct, leaves, vcf = (depth, budget), proof, vcf_defend, symmetry (None, "random", "all"), gumbel = (max_considered, c_visit, c_scale)
    with n_sims = playouts, sample_plies, sample_power and node_capacity, each as play_network_games reads it.  Each side has its own handle with its own
    options and its own network, so K7 plays K7 with any two sets of them.  gumbel does not go with leaves > 1, proof, vcf_defend or sample_plies > 0 on
    its side, nor with root_noise (ValueError, checked before the library is touched).
    `first` has black in even games (evaluation_sides).  paired (n_games even): the games 2p and 2p + 1 start from the same opening -- the first
    opening_plies plies (at most 8) of synthetic game first_game_id + 2p -- with the colours exchanged, so an opening's bias cancels within the
    pair (rating.summary(paired=True) reads the scores that way); paired=False: every game has its own opening, as in play_evaluation_games.
    Every random stream (root noise, sampled plies, Gumbel draws, K3 and K8 rollouts) is keyed by the game's global id first_game_id + g.
    The games in which `first` has black and the others form two groups, each with one handle per side; every ply of a group is the mover's root
    noise (root_noise = (alpha, epsilon); None, the default: a strength match explores nothing -- variety comes from the openings and sample_plies),
    its search, its root choice, the referee (K12) and the step of both handles -- the subtree kept (reuse_subtree) or a fresh root.
    device_loop: all of that is kernels on the current stream and the host reads the unfinished count once per ply and group; False: the same
    match through the host (root_stats down, numpy boards, moves up), kept for the tests: both play the same games byte for byte.
    Returns (GameRecords, first_is_black bool[n], scores float[n]: 1 / 0.5 / 0 for `first`); the records' visit rows are the mover's,
    records.groups lists per group the games, the unfinished count and "live_games": per side the K7 handle's live games (None for another
    handle), and records.overflow says whether an arena of any of the four handles filled up."""
    first, second = _match_agent(first, root_noise), _match_agent(second, root_noise)
    if paired and n_games % 2:
        raise ValueError("play_agent_match: a paired match has an even number of games")
    if not 0 <= opening_plies <= 8:
        raise ValueError("play_agent_match: openings of at most 8 plies (an opening cannot be a finished game)")
    dev, stream = _device(device)
    black = evaluation_sides(n_games)
    open_moves, open_lens = _opening(n_games, seed, first_game_id, opening_plies)
    if paired:
        open_moves[1::2], open_lens[1::2] = open_moves[0::2], open_lens[0::2]
    games = _HostGames.from_opening(open_moves, open_lens)
    start = int(games.lens[0]) if n_games else 0
    assert (games.lens == start).all() and not games.over.any()
    if device_loop:
        d_moves, d_lens, d_winner, d_visits = _record_tensors(n_games, dev, (games.moves, games.lens))
    else:
        visits = np.zeros((n_games, N, N), dtype=np.uint16)
    overflow, groups = False, []
    for gi, idx in enumerate((np.nonzero(black)[0], np.nonzero(~black)[0])):
        k = len(idx)
        if k == 0:
            groups.append({"games": idx, "unfinished": 0, "live_games": (None, None)})
            continue
        with contextlib.ExitStack() as handles, torch.no_grad():
            sides = [handles.enter_context(contextlib.closing(_MatchSide(spec, idx, games, seed, first_game_id, reuse_subtree, dev))) for spec in (first, second)]
            unfinished = k
            if device_loop:
                d_idx = torch.from_numpy(idx.astype(np.int32)).to(dev)
                d_cells, d_rows = torch.full((k,), -1, dtype=torch.int16, device=dev), torch.zeros((k, N), dtype=torch.int16, device=dev)
                d_verdict, d_status, d_unfinished = torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            for ply in range(max_moves):
                if not device_loop and games.over[idx].all():
                    break
                mover = sides[0 if ((start + ply) % 2 == 0) == (gi == 0) else 1]      # group 0: `first` has black, i.e. it moves on even stone counts
                if not device_loop and ply > 0 and not reuse_subtree:                   # (on the device loop step_device leaves the fresh roots)
                    mover.set_position(games)
                mover.search(root_noise, stream)
                if device_loop:
                    mover.choose_device(d_cells, d_rows)
                    G.match_referee(d_cells, d_rows, d_idx, d_moves, d_lens, d_winner, d_visits, d_verdict, d_status, d_unfinished)
                    for side in sides:
                        side.tree.step_device(d_cells, d_verdict, fresh_root=not reuse_subtree)
                    unfinished = int(d_unfinished.item())             # four bytes per ply and group: the only host sync of the loop
                    if unfinished == 0:
                        break
                else:
                    best, rows, full = mover.choose_host(games.lens[idx])
                    overflow |= full
                    step = games.play(idx, best, rows, visits, stall_ends_game=False)      # a mover without a child leaves its game where it stands
                    if reuse_subtree:
                        for side in sides:
                            side.step_host(step)
            if device_loop:
                overflow |= any([side.overflow() for side in sides])
            else:
                unfinished = int((~games.over[idx]).sum())
            groups.append({"games": idx, "unfinished": unfinished, "live_games": tuple(side.live for side in sides)})
    if device_loop:
        rec = GameRecords(d_moves, d_lens, d_winner, d_visits, first_game_id, overflow)
        winner = d_winner.cpu().numpy()
    else:
        rec = _records_from_host(games, visits, dev, first_game_id, overflow)
        winner = games.winner
    rec.groups = groups
    return rec, black, evaluation_scores(winner, black)


def play_pattern_games(n_games, opening_plies=4, seed=G.DEFAULT_SEED, first_game_id=0, filter=True, max_moves=N, device=None):
    """n_games whole games of the search-free pattern policy against itself (K10, gmk_pattern_play): every ply is the first maximum of
    Heuristic::EvaluationProbs -- after DecisiveFilter with filter=True (PatternEvalAgent), without it Heuristic::MaxEvaluatedRollout -- on the
    game's live evaluator, all games in ONE launch on the current stream; nothing comes back to the host between plies.  The policy is
    deterministic: variety comes from the openings (synthetic generator, `opening_plies` plies of game first_game_id + g), so a game's record
    depends only on its global id.  max_moves < 225: at most that many plies are added to an opening.
    Returns (GameRecords without visit counts, values float32[n, 225] on the device: entry i of a row = the EvaluationValue the player of
    move i saw, 0 for opening plies and past the end); the records carry the kernel's status words as `.status` (int32[n], lib.PATTERN_*)."""
    if max_moves < 1:
        raise ValueError("play_pattern_games: max_moves must be at least 1")
    dev, stream = _device(device)
    with torch.cuda.device(dev):
        d_moves, d_lens, d_winner, _ = _record_tensors(n_games, dev, _opening(n_games, seed, first_game_id, opening_plies), visits=False)
        d_values = torch.zeros((n_games, N), dtype=torch.float32, device=dev)
        d_status = torch.zeros(n_games, dtype=torch.int32, device=dev)
        G.pattern_play(d_moves.data_ptr(), d_lens.data_ptr(), n_games, filter, max_moves if max_moves < N else 0,
                       d_winner.data_ptr(), d_values.data_ptr(), d_status.data_ptr(), stream)
    rec = GameRecords(d_moves, d_lens, d_winner, None, first_game_id)
    rec.status = d_status
    return rec, d_values


def dump_batches(samples, path, batch_size=512):
    """The reference appends mini-batches to `latest.train.hdf5` as three growing datasets `state_batch`, `value_batch`,
    `probs_batch` of shape (batches, batch_size, ...) (network/data_helper.py:176-194).  h5py is written when it can be
    imported; otherwise the same three arrays go to `<path>.npz` (numpy's archive), with the same names and shapes.
    `samples` = (states, values, pi) as GameRecords.to_samples() returns them; a trailing partial batch is dropped like
    the reference's generator does.  Returns the number of batches written."""
    states, values, pi = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in samples)
    n_batches = states.shape[0] // batch_size
    if n_batches == 0:
        return 0
    cut = n_batches * batch_size
    arrays = {"state_batch": states[:cut].reshape(n_batches, batch_size, *states.shape[1:]).astype(np.float32),
              "value_batch": values[:cut].reshape(n_batches, batch_size).astype(np.float32),
              "probs_batch": pi[:cut].reshape(n_batches, batch_size, pi.shape[1]).astype(np.float32)}
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None and not path.endswith(".npz"):
        with h5py.File(path, "a") as hf:
            for name, arr in arrays.items():
                if name not in hf:
                    hf.create_dataset(name, (0, *arr.shape[1:]), maxshape=(None, *arr.shape[1:]))
                hf[name].resize(hf[name].shape[0] + arr.shape[0], axis=0)
                hf[name][-arr.shape[0]:] = arr
    else:
        path = path if path.endswith(".npz") else path + ".npz"
        if os.path.exists(path):
            with np.load(path) as old:
                arrays = {name: np.concatenate([old[name], arr]) for name, arr in arrays.items()}
        np.savez(path, **arrays)
    return n_batches


def pack_records(rec):
    """The wire form of a rank's records, ONE uint8 tensor on the records' device: lens int32[n], winner int8[n],
    then only what was played: moves uint8[sum(lens)] and, if visits were recorded, uint16[sum(lens)][225] (the root visit counts
    of the searched plies; plies that were not searched -- openings -- carry their zero rows).  ~27 KB per game instead of the
    fixed-stride 101 KB."""
    lens = rec.lens.to(torch.int32).contiguous()
    n = int(lens.shape[0])
    if n == 0:
        return torch.zeros(0, dtype=torch.uint8, device=lens.device)
    played = torch.arange(N, device=lens.device)[None, :] < lens[:, None]            # [n, 225]
    parts = [lens.view(torch.uint8).reshape(-1), rec.winner.to(torch.int8).contiguous().view(torch.uint8).reshape(-1),
             rec.moves.contiguous().view(torch.uint8).reshape(n, N)[played]]
    if rec.visits is not None:
        parts.append(rec.visits.contiguous().view(torch.int16).reshape(n, N, N)[played].contiguous().view(torch.uint8).reshape(-1))
    return torch.cat(parts)


def unpack_records_into(buf, n, has_visits, moves, lens, winner, visits, at):
    """pack_records undone into rows [at, at + n) of preallocated fixed-stride arrays (rows beyond a game's length must be zero already)."""
    dev = buf.device
    lens[at:at + n] = buf[:4 * n].view(torch.int32)
    winner[at:at + n] = buf[4 * n:5 * n].view(torch.int8)
    my_lens = lens[at:at + n]
    total = int(my_lens.sum()) if n else 0
    played = torch.arange(N, device=dev)[None, :] < my_lens[:, None]
    moves[at:at + n][played] = buf[5 * n:5 * n + total]
    if has_visits and visits is not None:
        flat = buf[5 * n + total:5 * n + total + total * N * 2]
        if (5 * n + total) % 2:                                  # int16 views need an even byte offset
            flat = flat.clone()
        visits[at:at + n][played] = flat.view(torch.int16).reshape(total, N)


def unpack_records(buf, n, has_visits, first_game_id=0, overflow=False):
    """pack_records undone: fixed-stride GameRecords on buf's device (what to_samples() / K4 + K5 read)."""
    dev = buf.device
    moves = torch.zeros((n, N), dtype=torch.uint8, device=dev)
    lens = torch.zeros((n,), dtype=torch.int32, device=dev)
    winner = torch.zeros((n,), dtype=torch.int8, device=dev)
    visits = torch.zeros((n, N, N), dtype=torch.int16, device=dev) if has_visits else None
    unpack_records_into(buf, n, has_visits, moves, lens, winner, visits, 0)
    return GameRecords(moves, lens, winner, visits, first_game_id, overflow)


# The same three steps through the C-ABI (gmk_records_*, records_wire.hip): what a binder without torch calls.
def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def pack_records_device(rec):
    """pack_records on the device: the same uint8 tensor, from a prefix sum of the lengths and one pack kernel.  It synchronises once, for
    the size.  Raises GmkError if a length is outside [0, 225] (pack_records does not check)."""
    lens = rec.lens.to(torch.int32).contiguous()
    n = int(lens.shape[0])
    dev = lens.device
    if n == 0:
        return torch.zeros(0, dtype=torch.uint8, device=dev)
    moves = rec.moves.contiguous().view(torch.uint8)
    winner = rec.winner.to(torch.int8).contiguous()
    visits = None if rec.visits is None else rec.visits.contiguous()
    assert moves.shape == (n, N) and winner.shape == (n,) and (visits is None or (visits.shape == (n, N, N) and visits.element_size() == 2))
    stream = _stream(dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    G.records_scan(lens.data_ptr(), n, offsets.data_ptr(), stream)
    size = G.records_packed_bytes(offsets.data_ptr(), n, visits is not None, stream)
    out = torch.empty(size, dtype=torch.uint8, device=dev)
    # status can only be set on a bad length or a short buffer, and records_packed_bytes has ruled out both: it is not read back
    G.records_pack(moves.data_ptr(), lens.data_ptr(), winner.data_ptr(), None if visits is None else visits.data_ptr(), n, offsets.data_ptr(),
                   out.data_ptr(), size, status.data_ptr(), stream)
    return out


def unpack_records_device(buf, n, has_visits, first_game_id=0, overflow=False):
    """unpack_records on the device: the same GameRecords.  The kernel writes every byte of the fixed-stride rows (zeros past a game's
    length), so they are allocated uncleared.  Raises ValueError if a length in buf is outside [0, 225] or buf's size is not the wire size
    of its lengths."""
    dev = buf.device
    buf = buf.contiguous()
    moves = torch.empty((n, N), dtype=torch.uint8, device=dev)
    lens = torch.empty((n,), dtype=torch.int32, device=dev)
    winner = torch.empty((n,), dtype=torch.int8, device=dev)
    visits = torch.empty((n, N, N), dtype=torch.int16, device=dev) if has_visits else None
    if n > 0:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        G.records_unpack(buf.data_ptr(), buf.numel(), n, has_visits, offsets.data_ptr(), moves.data_ptr(), lens.data_ptr(), winner.data_ptr(),
                         None if visits is None else visits.data_ptr(), status.data_ptr(), _stream(dev))
        code = int(status.item())
        if code:
            raise ValueError("unpack_records_device: %s" % ("a game length is outside [0, 225]" if code == G.WIRE_BAD_LENGTH else
                                                            "%d bytes are not the wire size of these %d games" % (buf.numel(), n)))
    return GameRecords(moves, lens, winner, visits, first_game_id, overflow)


def samples_from_packed(buf, n, augment=False, first_move=0):
    """The training tuples of the n games of a wire-form block with visits, read from the block itself (K4 + K5, no fixed-stride copy):
    the same (states, values, pi) as unpack_records(buf, n, True).to_samples(augment, first_move)."""
    dev = buf.device
    buf = buf.contiguous()
    copies = 8 if augment else 1
    if n == 0:
        return (torch.empty((0, 6, 15, 15), dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
                torch.empty((0, N), dtype=torch.float32, device=dev))
    stream = _stream(dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    G.records_scan(buf.data_ptr(), n, offsets.data_ptr(), stream)
    size = G.records_packed_bytes(offsets.data_ptr(), n, True, stream)
    if size != buf.numel():
        raise ValueError("samples_from_packed: %d bytes are not the wire size (%d) of these %d games with visits" % (buf.numel(), size, n))
    game, move = _sample_lists(buf[:4 * n].view(torch.int32).cpu().numpy(), first_move)
    s = int(game.shape[0])
    d_game, d_move = torch.from_numpy(game).to(dev), torch.from_numpy(move).to(dev)
    states = torch.empty((s * copies, 6, 15, 15), dtype=torch.uint8, device=dev)
    values = torch.empty(s * copies, dtype=torch.float32, device=dev)
    pi = torch.empty((s * copies, N), dtype=torch.float32, device=dev)
    G.samples_from_packed(buf.data_ptr(), n, offsets.data_ptr(), d_game.data_ptr(), d_move.data_ptr(), s, augment, states.data_ptr(),
                          values.data_ptr(), pi.data_ptr(), stream)
    return states, values, pi


class ReplayBuffer:
    """The trainer's side of self-play: DataHelper.buffer + DataHelper.generate_batch (network/data_helper.py:67-83, 97-139) in HBM
    (gmk_replay_*, replay_kernel.hip).  It keeps game RECORDS -- a byte per stored ply, a 450-byte visit row per sampled ply -- and builds
    the tuples of a minibatch when it is drawn: `batch_size` distinct samples per step (random.sample), a sample = one sampled ply under
    one of the eight symmetries.  At most capacity_plies stored plies and max_games games are held; an append makes the oldest whole
    games leave until the new ones fit (the reference trims before it extends and may overshoot; this capacity is an allocation).
    extend / extend_packed / sample are asynchronous on the current stream of the buffer's device; len(), stats() and status() synchronise it.
    target = "policy": the rows held are improved-policy rows (play_network_games(gumbel=)) and sample() / batches() read them as distributions
    (lib.TARGET_POLICY); "visits": visit counts through MCTS::evalState's transform, as before.  The stored bytes and state_dict() do not depend on it."""

    def __init__(self, capacity_plies, max_games=None, seed=G.DEFAULT_SEED, device=None, target="visits"):
        if target not in G.TARGETS:
            raise ValueError("ReplayBuffer: target is \"visits\" or \"policy\", not %r" % (target,))
        self.target = target                                   # how sample() reads a row: a property of the draw, not of what is stored or checkpointed
        capacity_plies = int(capacity_plies)
        if capacity_plies < N:
            raise ValueError("ReplayBuffer: capacity_plies must be at least 225 (one full game)")
        if max_games is None:
            max_games = max(1, capacity_plies // 8)          # (32 bytes per game: no game of self-play is shorter than nine plies)
        max_games = int(max_games)
        if not 1 <= max_games <= capacity_plies:
            raise ValueError("ReplayBuffer: max_games must be in [1, capacity_plies]")
        G.init(torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.capacity_plies, self.max_games, self.seed = capacity_plies, max_games, int(seed)
        self._h = G.ReplayHandle(capacity_plies, max_games, seed)
        self._status = torch.zeros(2, dtype=torch.int32, device=self.device)      # [0] the last append's code, [1] the last draw's
        self._step = 0

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._h.close()
            self._h = None

    def reset(self):
        self._h.reset(_stream(self.device))

    def extend(self, records, first_move=0):
        """Appends the games of a GameRecords on this device (with visits).  Plies below first_move are kept for the positions after them
        but are never drawn.  A length outside [0, 225] appends nothing and leaves lib.REPLAY_BAD_LENGTH in status()[0]."""
        if records.visits is None:
            raise ValueError("ReplayBuffer.extend: the records carry no visit counts")
        if not 0 <= int(first_move) <= N:
            raise ValueError("ReplayBuffer.extend: first_move must be in [0, 225]")
        n = len(records)
        if n == 0:
            return
        if not records.moves.is_cuda or records.moves.device != self.device:
            raise ValueError("ReplayBuffer.extend: the records must be on %s" % (self.device,))
        moves = records.moves.contiguous().view(torch.uint8)
        lens = records.lens.to(torch.int32).contiguous()
        winner = records.winner.to(torch.int8).contiguous()
        visits = records.visits.contiguous()
        assert moves.shape == (n, N) and winner.shape == (n,) and visits.shape == (n, N, N) and visits.element_size() == 2
        self._h.append(moves.data_ptr(), lens.data_ptr(), winner.data_ptr(), visits.data_ptr(), n, first_move, self._status.data_ptr(),
                       _stream(self.device))

    def extend_packed(self, buf, n, first_move=0):
        """Appends the n games of a wire-form block with visits (pack_records / pack_records_device; what a rank sends to gather_records)."""
        if not 0 <= int(first_move) <= N:
            raise ValueError("ReplayBuffer.extend_packed: first_move must be in [0, 225]")
        n = int(n)
        if n == 0:
            return
        if not buf.is_cuda or buf.device != self.device or buf.dtype != torch.uint8 or buf.numel() < 5 * n:
            raise ValueError("ReplayBuffer.extend_packed: buf must be a uint8 tensor of at least 5 n bytes on %s" % (self.device,))
        buf = buf.contiguous()
        stream = _stream(self.device)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        G.records_scan(buf.data_ptr(), n, offsets.data_ptr(), stream)
        self._h.append_packed(buf.data_ptr(), n, offsets.data_ptr(), first_move, self._status[0:].data_ptr(), stream)

    def sample(self, batch_size, step=None, augment=True, dtype=torch.float32, return_picked=False):
        """-> (states [B,6,15,15] of `dtype` (torch.float32 or torch.uint8), values float32[B], pi float32[B,225][, picked int64[B,3] =
        (game serial, ply, symmetry)]): the batch of (seed, step), B distinct samples; the same (seed, step) and contents give the same
        batch.  step=None counts the draws of this object.  With fewer than B samples held nothing is written and status()[1] is
        lib.REPLAY_TOO_FEW (the tensors are returned uninitialised): ask len() first, as batches() does."""
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError("ReplayBuffer.sample: dtype must be torch.float32 or torch.uint8")
        batch_size = int(batch_size)
        if batch_size < 0:
            raise ValueError("ReplayBuffer.sample: batch_size must not be negative")
        if step is None:
            step = self._step
            self._step += 1
        dev = self.device
        states = torch.empty((batch_size, 6, 15, 15), dtype=dtype, device=dev)
        values = torch.empty(batch_size, dtype=torch.float32, device=dev)
        pi = torch.empty((batch_size, N), dtype=torch.float32, device=dev)
        picked = torch.empty((batch_size, 3), dtype=torch.int64, device=dev) if return_picked else None
        self._h.sample(batch_size, step, augment, dtype == torch.float32, states.data_ptr(), values.data_ptr(), pi.data_ptr(),
                       None if picked is None else picked.data_ptr(), self._status[1:].data_ptr(), _stream(dev),
                       target=None if self.target == "visits" else self.target)
        return (states, values, pi, picked) if return_picked else (states, values, pi)

    def stats(self):
        """{"games", "plies", "population" (sampled plies held), "evicted_games", "capacity_plies", "max_games"}; synchronises."""
        games, plies, population, evicted = self._h.size(_stream(self.device))
        return {"games": games, "plies": plies, "population": population, "evicted_games": evicted,
                "capacity_plies": self.capacity_plies, "max_games": self.max_games}

    def status(self):
        """(code of the last append, code of the last draw): 0, lib.REPLAY_BAD_LENGTH, lib.REPLAY_TOO_FEW; synchronises."""
        a, d = self._status.tolist()
        return a, d

    def state_dict(self):
        """What a checkpoint keeps of the buffer: {"image": the held games as a uint8 CPU tensor (gmk_replay_snapshot; the format is in
        include/gomoku_hip.h), "seed", "step" (the draw counter of sample(step=None)), "capacity_plies", "max_games"}.  Synchronises."""
        stream = _stream(self.device)
        size = self._h.image_bytes(stream)
        image = torch.empty(size, dtype=torch.uint8, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._h.snapshot(image.data_ptr(), size, status.data_ptr(), stream)
        code = int(status.item())
        if code:
            raise RuntimeError("ReplayBuffer.state_dict: gmk_replay_snapshot refused an image of its own size (status %d)" % code)
        return {"image": image.cpu(), "seed": self.seed, "step": self._step, "capacity_plies": self.capacity_plies, "max_games": self.max_games}

    def load_state_dict(self, state):
        """The games, their serials and the draw counter of a state_dict() replace what this buffer holds, so that its draws and evictions
        go on as the saved buffer's would have.  Raises ValueError -- and leaves the buffer as it was -- if the seeds differ (the draws
        would silently differ), if the image is not valid, or if its games do not fit capacity_plies and max_games."""
        mask = 0xFFFFFFFFFFFFFFFF
        if int(state["seed"]) & mask != self.seed & mask:
            raise ValueError("ReplayBuffer.load_state_dict: the state was saved with seed %d, this buffer draws with seed %d" % (int(state["seed"]), self.seed))
        image = state["image"]
        if not torch.is_tensor(image) or image.dtype != torch.uint8 or image.dim() != 1 or image.numel() < 64:
            raise ValueError("ReplayBuffer.load_state_dict: the image must be a flat uint8 tensor of at least 64 bytes")
        step = int(state["step"])
        G.replay_image_check_host(image.cpu().contiguous().numpy())          # ValueError names the broken rule
        d_image = image.to(self.device).contiguous()
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._h.restore(d_image.data_ptr(), d_image.numel(), status.data_ptr(), _stream(self.device))
        code = int(status.item())
        if code == G.REPLAY_NO_ROOM:
            raise ValueError("ReplayBuffer.load_state_dict: the saved games do not fit capacity_plies = %d and max_games = %d"
                             % (self.capacity_plies, self.max_games))
        if code:
            raise ValueError("ReplayBuffer.load_state_dict: the device refused the image (status %d)" % code)
        self._step = step

    @classmethod
    def from_state_dict(cls, state, capacity_plies=None, max_games=None, device=None, target="visits"):
        """A new buffer with the saved seed that holds the saved games; the sizes default to the saved ones.  target is not saved (the stored
        bytes do not depend on it): a resumed run passes the one it was started with."""
        buf = cls(state["capacity_plies"] if capacity_plies is None else capacity_plies, state["max_games"] if max_games is None else max_games,
                  seed=state["seed"], device=device, target=target)
        try:
            buf.load_state_dict(state)
        except Exception:
            buf.close()
            raise
        return buf

    def __len__(self):
        """The population of an augmented draw: 8 x the sampled plies held -- what len(DataHelper.buffer) counts."""
        return 8 * self._h.size(_stream(self.device))[2]

    def batches(self, batch_size):
        """generate_batch (data_helper.py:133-139): yields augmented float32 minibatches while len(self) > batch_size."""
        while len(self) > batch_size:
            yield self.sample(batch_size)


class GatherError(RuntimeError):
    """Raised on EVERY rank when any rank could not contribute to gather_records."""


def gather_records(rec, dst=0, group=None):
    """The one exchange step of the path (network/data_helper.py:97-113: the worker processes' `Manager().list()`): every rank
    contributes its records in the compact wire form of pack_records, rank `dst` receives them with one grouped batch of
    point-to-point transfers -- every other rank posts ONE send, dst posts world - 1 receives (RCCL has no native gather; over xGMI
    the 7 peers send concurrently on their own links) -- and unpacks the concatenation in rank order (= global game id order).
    The same code runs on every torch.distributed backend (RCCL on the GPU box, gloo in the CPU tests); with world size 1 it is the
    identity.  Returns the gathered GameRecords on dst, None elsewhere."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return rec
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    dev = rec.lens.device
    # Packing is local work that can fail on one rank alone (memory): the ranks agree on it BEFORE the first collective, so that a failure
    # is raised on every rank (GatherError) instead of leaving the others waiting in all_gather for a rank that has left.
    mine, failure = None, None
    try:
        mine = pack_records(rec)
    except Exception as exc:                                    # noqa: BLE001
        failure = exc
    ok = torch.tensor([0 if failure is not None else 1], dtype=torch.int32, device=dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
    if int(ok[0]) == 0:
        raise GatherError("gather_records: packing failed on %s" % ("this rank: %s: %s" % (type(failure).__name__, failure) if failure is not None else "another rank"))
    # sizes first: [games, bytes, first game id, arena overflow seen, visits recorded]
    meta = torch.tensor([len(rec), int(mine.numel()), int(rec.first_game_id), int(bool(rec.overflow)), int(rec.visits is not None)], dtype=torch.int64, device=dev)
    metas = [torch.zeros_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta, group=group)
    metas = [[int(v) for v in m] for m in metas]
    if rank == dst:
        bufs = [mine if r == dst else torch.empty(metas[r][1], dtype=torch.uint8, device=dev) for r in range(world)]
        ops = [dist.P2POp(dist.irecv, bufs[r], r, group) for r in range(world) if r != dst and metas[r][1] > 0]
    else:
        ops = [dist.P2POp(dist.isend, mine, dst, group)] if mine.numel() > 0 else []
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    if rank != dst:
        return None
    has_visits = all(m[4] for m in metas if m[0] > 0) and any(m[0] > 0 for m in metas)
    overflow = any(m[3] for m in metas)                          # a rank whose arenas overflowed must not be reported as clean
    first = min((m[2] for m in metas if m[0] > 0), default=rec.first_game_id)
    n_all = sum(m[0] for m in metas)
    if n_all == 0:
        return GameRecords(rec.moves[:0], rec.lens[:0], rec.winner[:0], None if rec.visits is None else rec.visits[:0], first, overflow)
    # The fixed-stride form is allocated ONCE for all ranks and every rank's bytes are unpacked into their rows, the wire buffer of a rank
    # freed as soon as it has been read: 32 768 games are 3.3 GB of visit rows, and per-rank parts plus a concatenation would hold them twice.
    moves = torch.zeros((n_all, N), dtype=torch.uint8, device=dev)
    lens = torch.zeros((n_all,), dtype=torch.int32, device=dev)
    winner = torch.zeros((n_all,), dtype=torch.int8, device=dev)
    visits = torch.zeros((n_all, N, N), dtype=torch.int16, device=dev) if has_visits else None
    at = 0
    for r in range(world):                                       # rank order = global game id order
        if metas[r][0] > 0:
            unpack_records_into(bufs[r], metas[r][0], bool(metas[r][4]), moves, lens, winner, visits, at)
            at += metas[r][0]
        bufs[r] = None
    del mine
    return GameRecords(moves, lens, winner, visits, first, overflow)


def shard(n_total, rank, world):
    """Contiguous id blocks: game g lives on rank g * world // n_total."""
    lo = (n_total * rank) // world
    hi = (n_total * (rank + 1)) // world
    return lo, hi - lo
