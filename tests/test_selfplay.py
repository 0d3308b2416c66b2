"""Self-play records and the multi-rank gather (CPU part).  The gather is the only exchange step of the path
(SURVEY.md 8e); it is exercised here with world_size 2 on gloo, the GPU box uses the same code over RCCL."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gomokuai_amd import core, selfplay


def _fake_records(n, first, seed):
    rng = np.random.RandomState(seed)
    moves = np.zeros((n, 225), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    winner = np.zeros(n, dtype=np.int8)
    visits = np.zeros((n, 225, 225), dtype=np.int16)
    for g in range(n):
        b = core.Board()
        t = 0
        while not b.status["is_end"]:
            mv = b.random_move()
            empties = [i for i in range(225) if b.check_move(core.Position(i))]
            visits[g, t, empties] = rng.randint(0, 50, size=len(empties))
            visits[g, t, mv.id] = 60
            moves[g, t] = mv.id
            b.apply_move(mv)
            t += 1
        lens[g] = t
        winner[g] = int(float(b.status["winner"]))
    return selfplay.GameRecords(torch.from_numpy(moves), torch.from_numpy(lens), torch.from_numpy(winner), torch.from_numpy(visits), first)


def test_samples_match_dual_play_tuples():
    """GameRecords.samples == what agents/utils.py:29-63 builds move by move from Board.encoded_states()."""
    rec = _fake_records(2, 0, 1)
    for g in range(2):
        samples = rec.samples(g)
        b = core.Board()
        L = int(rec.lens[g])
        assert len(samples) == L
        for t in range(L):
            states, score, pi = samples[t]
            assert (states == b.encoded_states()).all()
            cur = b.status["cur_player"]
            b.apply_move(core.Position(int(rec.moves[g, t])))
            assert pi.shape == (225,) and abs(float(pi.sum()) - 1.0) < 1e-3
            assert float(score) == core.Player.calc_score(cur, core.Player.black if rec.winner[g] == 1 else core.Player.white if rec.winner[g] == -1 else core.Player.none)
        assert b.status["is_end"]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tuples.npz")


def test_host_tuples_match_the_reference_loop():
    """tests/golden/reference_tuples.npz holds what the REFERENCE's dual_play(verbose=True) (agents/utils.py:29-63) produced on
    this CorePyExt for six games of its random agent (made by tests/golden/make_reference_tuples.py in the build container).
    GameRecords.samples rebuilds the tuples from the move lists alone: encoded states and values must be identical."""
    ref = np.load(GOLDEN)
    n = int(ref["lens"].shape[0])
    rec = selfplay.GameRecords(torch.from_numpy(ref["moves"]), torch.from_numpy(ref["lens"]), torch.from_numpy(ref["winner"]),
                               torch.zeros((n, 225, 225), dtype=torch.int16), 0)
    k = 0
    for g in range(n):
        for states, value, pi in rec.samples(g):
            assert int(ref["game"][k]) == g
            assert (states == ref["states"][k]).all(), "game %d tuple %d" % (g, k)
            assert float(value) == float(ref["values"][k])
            assert pi.shape == ref["probs"][k].shape
            k += 1
    assert k == int(ref["values"].shape[0]) == int(ref["lens"].sum())
    assert np.allclose(ref["probs"], 1.0 / 225)                # the reference's random agent reports the uniform distribution


def test_shard_blocks_cover_everything():
    for total, world in ((32768, 8), (4096, 3), (10, 4)):
        blocks = [selfplay.shard(total, r, world) for r in range(world)]
        assert blocks[0][0] == 0 and sum(n for _, n in blocks) == total
        for (lo, n), (lo2, _) in zip(blocks, blocks[1:]):
            assert lo + n == lo2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, out_dir, total, dst):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, n = selfplay.shard(total, rank, world)
    rec = _fake_records(n, lo, 100 + rank)
    rec.overflow = rank == world - 1                       # one rank saw an arena overflow: rank dst must hear of it
    got = selfplay.gather_records(rec, dst=dst)
    torch.save({"moves": rec.moves, "lens": rec.lens, "winner": rec.winner, "visits": rec.visits}, os.path.join(out_dir, "part%d.pt" % rank))
    if rank == dst:
        assert got is not None and len(got) == total and got.first_game_id == 0 and got.overflow
        torch.save({"moves": got.moves, "lens": got.lens, "winner": got.winner, "visits": got.visits}, os.path.join(out_dir, "all.pt"))
    else:
        assert got is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,total,dst", [(2, 7, 0), (3, 7, 1), (3, 2, 0)])      # even-ish shards; uneven shards to a non-zero root; a rank without a game
def test_gather_gloo(tmp_path, world, total, dst):
    """The exchange step with world size 2 and 3 on gloo: ONE code path for every backend (grouped point-to-point transfers of
    the compact wire form), so this is what RCCL runs on the GPU box."""
    mp.spawn(_gather_worker, args=(world, _free_port(), str(tmp_path), total, dst), nprocs=world, join=True)
    parts = [torch.load(os.path.join(tmp_path, "part%d.pt" % r)) for r in range(world)]
    allrec = torch.load(os.path.join(tmp_path, "all.pt"))
    for key in ("moves", "lens", "winner", "visits"):
        assert torch.equal(allrec[key], torch.cat([p[key] for p in parts], dim=0)), key


def _failing_gather_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import datetime
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    lo, n = selfplay.shard(6, rank, world)
    rec = _fake_records(n, lo, 7 + rank)
    if rank == 1:
        rec.moves = None                                   # packing this rank's records raises before the first collective
    try:
        selfplay.gather_records(rec, dst=0)
        outcome = "returned"
    except selfplay.GatherError as exc:
        outcome = "GatherError: %s" % exc
    open(os.path.join(out_dir, "outcome%d.txt" % rank), "w").write(outcome)
    dist.barrier()                                         # every rank is still in step with the others
    dist.destroy_process_group()


def test_gather_fails_on_every_rank_when_one_cannot_pack(tmp_path):
    """A rank that fails before all_gather must not leave the others waiting in it: the ranks agree first, all raise GatherError."""
    import time
    t0 = time.monotonic()
    mp.spawn(_failing_gather_worker, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True)
    assert time.monotonic() - t0 < 45.0
    outcomes = [open(os.path.join(tmp_path, "outcome%d.txt" % r)).read() for r in range(3)]
    assert all(o.startswith("GatherError") for o in outcomes), outcomes
    assert "this rank" in outcomes[1] and "another rank" in outcomes[0]


def test_wire_form_is_compact_and_round_trips():
    """pack_records carries only what was played (moves u8[L], visits u16[L][225], winner, length per game)."""
    rec = _fake_records(3, 9, 5)
    buf = selfplay.pack_records(rec)
    total = int(rec.lens.sum())
    assert buf.dtype == torch.uint8 and buf.numel() == 3 * 5 + total + total * 225 * 2
    assert buf.numel() < 0.6 * (rec.moves.numel() + rec.visits.numel() * 2)
    back = selfplay.unpack_records(buf, 3, True, first_game_id=9)
    for key in ("moves", "lens", "winner", "visits"):
        assert torch.equal(getattr(back, key), getattr(rec, key)), key
    no_visits = selfplay.GameRecords(rec.moves, rec.lens, rec.winner, None, 9)
    back = selfplay.unpack_records(selfplay.pack_records(no_visits), 3, False)
    assert back.visits is None and torch.equal(back.moves, rec.moves)


def test_gather_single_process_is_identity():
    rec = _fake_records(2, 5, 3)
    assert selfplay.gather_records(rec) is rec


def test_host_games_match_the_board():
    """selfplay._HostGames (all games of a batch at once, numpy) against CorePyExt.Board move by move: end detection and winner
    (Game.cpp:37-49, 88-136), including overlines and a full board without a five (the reference's tie order)."""
    from gomokuai_amd import core
    from gomokuai_amd.selfplay import _HostGames
    rng = np.random.RandomState(7)
    n = 120
    hg = _HostGames(n)
    boards = [core.Board() for _ in range(n)]
    for ply in range(225):
        played = np.full(n, -1)
        for g in range(n):
            if boards[g].status["is_end"]:
                continue
            free = [c for c in range(225) if boards[g].check_move(core.Position(c))]
            played[g] = free[rng.randint(len(free))] if (g % 3 and rng.rand() < 0.6) else free[0]
        moved = hg.apply(played)
        assert sorted(moved) == [g for g in range(n) if played[g] >= 0]
        for g in range(n):
            if played[g] >= 0:
                boards[g].apply_move(core.Position(int(played[g])))
        assert all(bool(hg.over[g]) == bool(boards[g].status["is_end"]) for g in range(n)), ply
        if hg.over.all():
            break
    assert all(int(hg.winner[g]) == int(boards[g].status["winner"]) for g in range(n))
    assert (hg.winner == 1).any() and (hg.winner == -1).any()
    # the tie: a full board without five in a row (the pattern of core/test/integration/board_integrationtest.cpp)
    tie = _HostGames(1)
    b = core.Board()
    order = [y * 15 + x for y in range(15) for x in range(15)]
    cells = sorted(order, key=lambda c: (((c % 15) // 2 + (c // 15)) % 2, c))      # colour classes that never line up five
    blacks, whites = [c for c in cells if ((c % 15) // 2 + c // 15) % 2 == 0], [c for c in cells if ((c % 15) // 2 + c // 15) % 2 == 1]
    seq = []
    while blacks or whites:
        if blacks: seq.append(blacks.pop())
        if whites: seq.append(whites.pop())
    ok = True
    for c in seq:
        if b.status["is_end"]:
            ok = False
            break
        tie.apply(np.array([c]))
        b.apply_move(core.Position(c))
        assert bool(tie.over[0]) == bool(b.status["is_end"])
    assert int(tie.winner[0]) == int(b.status["winner"])


def test_plan_games_spreads_games_over_handles_and_slots():
    """selfplay.plan_games: the bookkeeping behind play_games(slots=, handles=) -- contiguous blocks that cover every game once, the
    slots shared out between the handles, the lock-step loop when neither is asked for."""
    assert selfplay.plan_games(4096) is None                                    # one handle, all games at once
    assert selfplay.plan_games(23, slots=64) is None                            # more slots than games
    assert selfplay.plan_games(32768) == [(0, 32768, 8192)]                     # one handle: its persistent launch fills the chip
    assert selfplay.plan_games(8192) is None                                    # every game in flight from the start
    assert selfplay.plan_games(8192, handles=2) == [(0, 4096, 4096), (4096, 8192, 4096)]   # two handles on request
    assert selfplay.plan_games(23, slots=5) == [(0, 23, 5)]
    for n, slots, handles in [(23, 6, 3), (23, None, 2), (7, 100, 7), (5, 1, 9), (40000, "auto", "auto"), (16385, "auto", 1)]:
        plan = selfplay.plan_games(n, slots, handles)
        assert plan[0][0] == 0 and plan[-1][1] == n and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
        assert all(1 <= s <= hi - lo for lo, hi, s in plan)
        if isinstance(slots, int):
            assert sum(s for _, _, s in plan) <= max(len(plan), min(slots, n)) + len(plan) - 1
    assert selfplay.plan_games(20000, opening_plies=12) is None                 # long openings: the lock-step loop
    with pytest.raises(ValueError):
        selfplay.plan_games(20000, slots=100, opening_plies=12)
    with pytest.raises(ValueError):
        selfplay.plan_games(0)


def test_network_slot_loops_refuse_what_they_would_ignore():
    """play_network_games: the slot loops play whole games (and the device-resident one takes openings of at most 8 plies): a move cap or a longer
    opening is refused up front, not silently ignored (no GPU needed: the check comes first)."""
    import pytest
    from gomokuai_amd import selfplay
    with pytest.raises(ValueError):
        selfplay.play_network_games(8, None, 4, slots=2, max_moves=10)
    with pytest.raises(ValueError):
        selfplay.play_network_games(8, None, 4, slots=2, opening_plies=12)


# ---- the shared pieces of the game loops (selfplay._HostGames.play, _hand_over, _supervisor_host_loop, _arena_nodes, _opening) ----
def _ledger_script():
    """Steps (active, best, rows, stall_ends_game, movers) for 6 games: game 0 is won by black at its ninth ply and stays in its slot,
    a mover stalls with the flag both ways, one step masks a side as the match loop does, and rows carry counts of 32 768 and above and
    counts above 65 535."""
    rng = np.random.RandomState(3)

    def rows(k):
        r = rng.randint(0, 50, size=(k, 225)).astype(np.uint32)
        r[:, 7] = 32768 + rng.randint(0, 1000, size=k)              # not negative behind the int16 view
        r[0, 9], r[-1, 11] = 65535, 70000                           # saturates
        return r

    steps = []
    for t in range(9):                                              # black: cells 0..4 of row 0, white: row 1 -- five in a row at ply 9
        cell0 = t // 2 if t % 2 == 0 else 15 + t // 2
        steps.append((np.array([0, 1, 2]), np.array([cell0, 100 + t, 200 + t]), rows(3), True, None))
    steps.append((np.array([0, 1, 2]), np.array([30, -1, 209]), rows(3), False, None))          # finished game 0; game 1 stalls and stays
    steps.append((np.array([0, 1, 2]), np.array([31, 109, -1]), rows(3), True, None))           # game 1 goes on; game 2 stalls and is over
    steps.append((np.array([3, 2, 4, 5]), np.array([40, 41, -1, 42]), rows(4), True, np.array([True, True, False, False])))   # masked: neither play nor stall
    steps.append((np.array([3, 2, 4, 5]), np.array([-1, 50, 51, 52]), rows(4), True, np.array([False, False, True, True])))
    steps.append((np.array([5, 4]), np.array([-1, 60]), rows(2), True, np.array([True, True])))  # a mover of the masked form stalls: over
    steps.append((np.array([5, 4, 1]), np.array([61, 62, 110]), rows(3), True, None))
    return steps


def test_ledger_matches_a_move_by_move_restatement_on_the_board():
    """_HostGames.play -- the one ledger step of every host-driven loop -- against core.Board, game by game: who moves, who is marked over,
    which row lands at which ply (the ply the move was made at), saturation at 65 535, and the step handed back for tree.step."""
    from gomokuai_amd.selfplay import _HostGames, _records_from_host
    n = 6
    hg, visits = _HostGames(n), np.zeros((n, 225, 225), dtype=np.uint16)
    boards, over, moves, want = [core.Board() for _ in range(n)], [False] * n, [[] for _ in range(n)], np.zeros((n, 225, 225), dtype=np.int64)
    for active, best, rows, stall, movers in _ledger_script():
        step = hg.play(active, best, rows, visits, stall_ends_game=stall, movers=movers)
        expect = np.full(len(active), -1)
        for s, g in enumerate(active):
            if over[g] or (movers is not None and not movers[s]):
                continue
            if best[s] < 0:
                over[g] = stall
                continue
            want[g, len(moves[g])] = np.minimum(rows[s], 65535)
            moves[g].append(int(best[s]))
            boards[g].apply_move(core.Position(int(best[s])))
            over[g] = bool(boards[g].status["is_end"])
            expect[s] = best[s]
        assert step.dtype == np.int16 and (step == expect).all()
        assert [bool(o) for o in hg.over] == over
        assert all(list(hg.moves[g, :hg.lens[g]]) == moves[g] for g in range(n))
    assert int(hg.winner[0]) == 1 == int(boards[0].status["winner"]) and hg.lens[0] == 9 and not hg.winner[1:].any()
    assert (visits.astype(np.int64) == want).all() and want.max() == 65535 and ((want >= 32768) & (want < 65535)).any()
    rec = _records_from_host(hg, visits, torch.device("cpu"), 4, True)
    assert rec.visits.dtype == torch.int16 and (rec.visits.numpy().view(np.uint16).astype(np.int64) == want).all()
    assert rec.first_game_id == 4 and rec.overflow and (rec.lens.numpy() == [len(m) for m in moves]).all()
    pi = rec.samples(1)[2][2]                                       # a count of 32 768 and above is the row's weight, not a negative one
    assert pi.argmax() == 7 and abs(float(pi.sum()) - 1) < 1e-3 and (pi >= 0).all()


def test_hand_over_fills_the_lowest_finished_slots_in_game_order():
    from gomokuai_amd.selfplay import _hand_over
    over, active, waiting, started = np.zeros(7, dtype=bool), np.arange(3), list(range(3, 7)), [0, 1, 2]
    for ending in ([], [1], [0, 2], [], [3, 4, 1], [5], [0, 2, 3, 4], [6], []):        # the order in which games end
        over[ending] = True
        want_active, want_waiting, want_fresh = active.copy(), list(waiting), np.zeros(3, dtype=bool)
        for slot in range(3):                                       # the rule, slot by slot
            if over[want_active[slot]] and want_waiting:
                want_active[slot], want_fresh[slot] = want_waiting.pop(0), True
        fresh = _hand_over(active, over, waiting)
        assert fresh.dtype == bool and (fresh == want_fresh).all() and (active == want_active).all() and waiting == want_waiting
        started += list(active[fresh])
    assert started == list(range(7)) and waiting == [] and over.all()
    # fewer waiting games than finished slots: the lowest slots get them
    over, active, waiting = np.array([True, True, True, False, False]), np.array([2, 0, 1]), [4]
    assert list(_hand_over(active, over, waiting)) == [True, False, False] and list(active) == [4, 0, 1] and waiting == []
    # an empty group
    active = np.zeros(0, dtype=np.int64)
    assert _hand_over(active, over, []).shape == (0,) and _hand_over(active, over, [3]).shape == (0,)


class _ScriptedTree:
    """A stand-in for lib.TraditionalMCTS in _supervisor_host_loop: root_stats() is a pure function of the position each slot was given
    (set_positions, then step), so the games it plays do not depend on slots -- if the loop hands it the right positions."""

    def __init__(self, n):
        self.n, self.positions, self.ids = n, [None] * n, None

    def set_game_ids(self, ids):
        self.ids = np.array(ids)

    def set_positions(self, moves, lens):
        assert moves.shape == (self.n, 225) and lens.shape == (self.n,)
        for s in range(self.n):
            if lens[s] >= 0:
                self.positions[s] = [int(c) for c in moves[s, :lens[s]]]

    def add_root_noise(self, alpha, epsilon, seed, first_game_id, stream):
        pass

    def run(self, playouts, stream):
        pass

    def root_stats(self):
        visits, best = np.zeros((self.n, 225), dtype=np.uint32), np.full(self.n, -1, dtype=np.int32)
        for s, pos in enumerate(self.positions):
            empty = [c for c in range(225) if c not in pos]
            row = (len(pos) % 2) * 7 + pos[0] % 7                   # black and white each fill a row of their own: a five after nine plies or so
            target = next((c for c in range(15 * row, 15 * row + 15) if c in empty), empty[0])
            visits[s, empty] = [(c * 7 + len(pos)) % 50 for c in empty]
            visits[s, target] = 40000 + len(pos)
            best[s] = target
        return {"visits": visits, "best": best, "status": np.zeros(self.n, dtype=np.int32)}

    def step(self, cells):
        assert cells.dtype == np.int16 and cells.shape == (self.n,)
        for s, c in enumerate(cells):
            if c >= 0:
                self.positions[s].append(int(c))


@pytest.mark.parametrize("reuse_subtree", [False, True])
def test_supervisor_host_loop_plays_the_same_games_through_any_slots(reuse_subtree):
    """The one host-driven loop of play_supervisor_games with a scripted searcher: 9 games through 3 slots give the records of 9 slots,
    with fresh roots and with kept trees (where only a slot that changed hands gets a new position)."""
    from gomokuai_amd.selfplay import _HostGames, _supervisor_host_loop
    out = []
    for slots, steps in ((9, 225), (3, (9 // 3 + 2) * 225)):
        games = _HostGames(9)
        games.apply(np.arange(9) * 16 + 20)                         # a different first stone per game
        tree = _ScriptedTree(slots)
        visits, overflow = _supervisor_host_loop(tree, games, slots, steps, 10, reuse_subtree, None, 1, 0, None)
        assert games.over.all() and not overflow and len(set(tree.ids)) == slots
        out.append((games.moves, games.lens, games.winner, visits))
    assert all((a == b).all() for a, b in zip(*out))
    assert (out[0][2] != 0).all() and int(out[0][1].max()) < 40 and int(out[0][3].max()) >= 40000


def test_arena_nodes_are_what_each_entry_point_asked_for():
    """selfplay._arena_nodes against the expressions of the entry points it replaced, written out: the four spellings, with the clamp to the
    24-bit node index and without it (play_games)."""
    from gomokuai_amd.selfplay import _arena_nodes
    top = (1 << 24) - 1
    for p in (1, 400, 100000):
        for kept, k in ((False, 1), (True, 3)):
            assert _arena_nodes("games", p, kept) == p * 225 * k + 1                              # play_games: not clamped
            assert _arena_nodes("supervisor", p, kept) == min(k * p * 226 + 1, top)               # play_supervisor_games, all three loops
            assert _arena_nodes("network", p, kept) == min(k * p * 225 + 1, top)                  # play_network_games, the K7 handle of play_evaluation_games
            assert _arena_nodes("match", p, kept) == min(k * p * 226 + 256, top)                  # the opponent of play_evaluation_games
            assert _arena_nodes("network", p, kept, node_capacity=777) == 777
        assert _arena_nodes("match", p) == min(p * 226 + 256, top)                                # the K6 / K8 searchers of play_match_games
        assert _arena_nodes("games", p) == p * 225 + 1                                            # its K3 searcher: BatchedMCTS(playouts_capacity=p)
    assert _arena_nodes("games", 100000, True) == 67500001 > top == _arena_nodes("network", 100000, True)


@pytest.mark.parametrize("plies", [0, 1, 4, 12])
def test_opening_is_the_synthetic_game_cut_to_its_plies(plies):
    from gomokuai_amd import lib as G
    from gomokuai_amd.selfplay import _HostGames, _last_two, _opening
    n, seed, first = 40, 11, 7
    m, l, _ = G.synth_boards(n, 0, seed=seed, first_board=first)
    moves, lens = _opening(n, seed, first, plies)
    assert moves.shape == (n, 225) and moves.dtype == np.uint8 and lens.dtype == np.int32
    assert (lens == np.minimum(l, plies)).all() and (plies == 0 or (lens == plies).any())
    last = _last_two(moves, lens)
    for g in range(n):
        assert (moves[g, :lens[g]] == m[g, :lens[g]]).all() and not moves[g, lens[g]:].any()
        assert last[g, 0] == (m[g, lens[g] - 1] if lens[g] > 0 else -1) and last[g, 1] == (m[g, lens[g] - 2] if lens[g] > 1 else -1)
    games, old = _HostGames.opened(n, seed, first, plies), _HostGames(n)
    for i in range(plies):                                          # the loop it replaces
        old.apply(np.where(l > i, m[:, i].astype(np.int64), -1))
    assert (games.moves == old.moves).all() and (games.lens == old.lens).all() and (games.over == old.over).all() and (games.stones == old.stones).all()
    assert (games.last_two() == _last_two(old.moves, old.lens)).all() and (games.last_two(np.array([5, 2])) == games.last_two()[[5, 2]]).all()
