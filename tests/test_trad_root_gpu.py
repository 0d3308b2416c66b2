"""K6: what happens at the ROOT between two searches -- MCTS::stepForward()'s choice, the visit row of a record, the move, the new root
(trad_tree.h: most_visited_child, child_of_cell, visits_by_cell, play_cell, legal_reply, new_root, copy_subtree) -- through every kernel
that does it: trad_root_stats_kernel, trad_root_choice_kernel, trad_step_kernel, trad_step_device_kernel, trad_advance_kernel and the
persistent turn of trad_playouts_kernel.  The expected values are the oracle's (oracle/go_trad.c) wherever it has the operation.

Searches of a few playouts, so that many root children share a visit count: the rule is "most visited, first in the CURRENT child order",
which is not "lowest cell"."""
import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

N = 225
CAP = 4096
DEV = torch.device("cuda", 0)
c = lambda y, x: y * 15 + x
# black has five in a row: a searched root of this position has no children
FIVE = [c(7, 7), c(0, 0), c(7, 8), c(0, 2), c(7, 9), c(0, 4), c(7, 10), c(0, 6), c(7, 11)]


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def _tie_positions():
    """0, 1, 2, 3, 4, 6, 9 and 12 distinct stones in the 7x7 block around the centre, one generator"""
    rng = np.random.RandomState(7)
    out = []
    for k in (0, 1, 2, 3, 4, 6, 9, 12):
        cells = []
        while len(cells) < k:
            y = 7 + rng.randint(-3, 4)
            x = 7 + rng.randint(-3, 4)
            if y * 15 + x not in cells:
                cells.append(y * 15 + x)
        out.append(cells)
    return out


POSITIONS = _tie_positions()
PLAYOUTS = (1, 3, 9, 33)


@pytest.fixture(scope="module")
def expected(oracle):
    """per playout count: the oracle's visits [8, 225], best cell [8], root children [8] and the lowest cell among the most visited [8]"""
    out = {}
    for p in PLAYOUTS:
        visits, best, kids, lowest = np.zeros((len(POSITIONS), N), np.uint32), [], [], []
        for g, pos in enumerate(POSITIONS):
            orc = oracle.TraditionalMCTS(5.0)
            orc.search(pos, p)
            v, _, pr, b = orc.root_children()
            visits[g] = v
            best.append(b)
            kids.append(int((pr != 0).sum()))
            lowest.append(int(np.nonzero((pr != 0) & (v == v[b]))[0][0]))
        out[p] = (visits, np.array(best), np.array(kids), np.array(lowest))
    return out


def _records(n):
    return (torch.zeros((n, N), dtype=torch.uint8, device=DEV), torch.full((n, N, N), 9, dtype=torch.int16, device=DEV),
            torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int8, device=DEV))


def _root_choice(t):
    cells = torch.full((t.n,), 99, dtype=torch.int16, device=DEV)
    rows = torch.full((t.n, N), 9, dtype=torch.int16, device=DEV)
    t.root_choice(cells, rows)
    torch.cuda.synchronize()
    return cells.cpu().numpy(), rows.cpu().numpy().view(np.uint16)


def _position_of(t, g, length):
    """the first `length` moves of the evaluator's record: the position the last search synchronised it with"""
    return [int(m) for m in t.read_evaluators()["record"][g][:length]]


def test_the_fixture_has_ties_that_the_lowest_cell_does_not_win(expected):
    visits, best, kids, lowest = expected[3]
    assert (best != lowest).sum() >= 3 and (kids > 64).any()
    assert list(best[[4, 5, 6]]) == [78, 115, 81] and list(lowest[[4, 5, 6]]) == [19, 16, 17]
    assert list(kids) == [1, 24, 47, 77, 81, 95, 119, 1]
    assert (expected[9][1] != expected[9][3]).sum() == 3 and (expected[33][1] != expected[33][3]).sum() == 2
    assert not expected[1][0].any() and (expected[1][1] == expected[1][3]).all()        # one playout: no child is visited, the first one is taken


@pytest.mark.parametrize("playouts", PLAYOUTS)
def test_ties_go_by_the_current_child_order_everywhere(gmk, expected, playouts):
    """root_stats, root_choice, step(), the lock-step loop's and the persistent loop's first move all name the oracle's child."""
    G = gmk
    visits, best, _, _ = expected[playouts]
    n = len(POSITIONS)
    t = G.TraditionalMCTS(n, node_capacity=CAP)
    t.set_positions(POSITIONS)
    t.run(playouts)
    st = t.root_stats()
    assert (st["status"] == 0).all()
    np.testing.assert_array_equal(st["visits"], visits)
    np.testing.assert_array_equal(st["best"], best)
    cells, rows = _root_choice(t)
    np.testing.assert_array_equal(cells, best)
    np.testing.assert_array_equal(rows, np.minimum(visits, 65535))
    t.step()                                                    # no forced move: the most visited child's cell is appended
    t.run(playouts)
    for g, pos in enumerate(POSITIONS):
        assert _position_of(t, g, len(pos) + 1) == pos + [int(best[g])], g
    t.close()

    open_moves = np.zeros((n, 16), np.uint8)
    open_lens = np.array([len(p) for p in POSITIONS], np.int32)
    for g, pos in enumerate(POSITIONS):
        open_moves[g, :len(pos)] = pos
    for persistent, reuse in ((False, False), (False, True), (True, False), (True, True)):
        where = "persistent %d, kept subtrees %d" % (persistent, reuse)
        t = G.TraditionalMCTS(n, node_capacity=CAP)
        d_moves, d_visits, d_lens, d_winner = _records(n)
        t.selfplay_run(n, 0, playouts, d_moves.data_ptr(), d_visits.data_ptr(), d_lens.data_ptr(), d_winner.data_ptr(), open_moves, open_lens,
                       reuse_subtree=reuse, max_steps=0 if persistent else 1, persistent=persistent)
        torch.cuda.synchronize()
        moves, lens, rec = d_moves.cpu().numpy(), d_lens.cpu().numpy(), d_visits.cpu().numpy().view(np.uint16)
        for g, pos in enumerate(POSITIONS):
            assert lens[g] > len(pos) and [int(m) for m in moves[g, :len(pos) + 1]] == pos + [int(best[g])], (where, g)
            np.testing.assert_array_equal(rec[g, len(pos)], np.minimum(visits[g], 65535), where)
        t.close()


def _two_roots(G, oracle, other):
    """game 0: FIVE, searched: a root without children; game 1: `other`, searched and then positioned again: a root that does not exist yet.
    The oracles have made the same searches (their evaluators persist like the handle's)."""
    t = G.TraditionalMCTS(2, node_capacity=CAP)
    t.set_positions([FIVE, other])
    t.run(8)
    lens = np.array([-1, len(other)], np.int32)
    moves = np.zeros((2, N), np.uint8)
    moves[1, :len(other)] = other
    t.set_positions(moves, lens)
    orcs = [oracle.TraditionalMCTS(5.0), oracle.TraditionalMCTS(5.0)]
    orcs[0].search(FIVE, 8)
    orcs[1].search(other, 8)
    return t, orcs


def _same_search(st, g, orc, nodes=True):
    """nodes=False: the oracle was driven with run(): its node count includes the moves it stepped through from the empty board"""
    v, q, p, best = orc.root_children()
    np.testing.assert_array_equal(st["visits"][g], v)
    np.testing.assert_array_equal(st["values"][g].view(np.uint32), q.view(np.uint32))
    np.testing.assert_array_equal(st["priors"][g].view(np.uint32), p.view(np.uint32))
    assert st["best"][g] == best and st["root_visits"][g] == orc.root_visits and st["status"][g] == 0
    assert not nodes or st["n_nodes"][g] == orc.n_nodes


def test_roots_without_children_and_roots_that_do_not_exist(gmk, oracle):
    G = gmk
    other = POSITIONS[4]
    free = [m for m in range(N) if m not in FIVE and m not in other]

    # ---- nothing to choose: -1, an all-zero visit row; a step without a move changes nothing ----
    t, orcs = _two_roots(G, oracle, other)
    st = t.root_stats()
    assert list(st["best"]) == [-1, -1] and st["root_visits"][0] == orcs[0].root_visits == 8 and st["root_visits"][1] == 0
    assert not st["visits"].any()
    cells, rows = _root_choice(t)
    assert list(cells) == [-1, -1] and not rows.any()
    t.step()
    st = t.root_stats()
    assert list(st["n_nodes"]) == [1, 1] and list(st["status"]) == [0, 0] and list(st["best"]) == [-1, -1]
    assert st["root_visits"][0] == 8 and st["root_visits"][1] == 0
    t.run(12)
    orcs[1].search(other, 12)
    st = t.root_stats()
    _same_search(st, 1, orcs[1])
    # the finished game's root was kept (MCTS.cpp:133: nothing moves) and is visited on: 8 + 12 visits, still no child
    assert st["best"][0] == -1 and st["n_nodes"][0] == 1 and st["status"][0] == 0 and st["root_visits"][0] == 20 and not st["visits"][0].any()
    assert _position_of(t, 0, len(FIVE)) == FIVE and _position_of(t, 1, len(other)) == other
    assert t.read_evaluators()["meta"][0][0] == len(FIVE)
    t.close()

    # ---- a forced step: one node, the move appended; through gmk_trad_step and through gmk_trad_step_device ----
    for device in (False, True):
        t, orcs = _two_roots(G, oracle, other)
        mv = np.array([free[0], free[40]], np.int16)
        if device:
            t.step_device(torch.from_numpy(mv).to(DEV), torch.full((2,), G.MATCH_MOVED, dtype=torch.int32, device=DEV), fresh_root=False)
            torch.cuda.synchronize()
        else:
            t.step(mv)
        st = t.root_stats()
        assert list(st["n_nodes"]) == [1, 1] and list(st["status"]) == [0, 0] and list(st["best"]) == [-1, -1] and not st["visits"].any(), device
        assert list(st["root_visits"]) == [0, 0], device
        # the finished game leaves (a move after the end is nothing the evaluator plays); the other one is searched from its new position
        moves = np.zeros((2, N), np.uint8)
        t.set_positions(moves, np.array([0, -1], np.int32))
        t.run(12)
        orcs[1].search(other + [int(mv[1])], 12)
        st = t.root_stats()
        _same_search(st, 1, orcs[1])
        assert _position_of(t, 1, len(other) + 1) == other + [int(mv[1])], device
        t.close()
    # ... and both lists took the move: the same cell again is no move of these games
    t, _ = _two_roots(G, oracle, other)
    t.step(mv)
    assert list(t.root_stats()["status"]) == [0, 0]
    t.step(mv)
    assert list(t.root_stats()["status"]) == [t.STATUS_ILLEGAL_STEP, t.STATUS_ILLEGAL_STEP]
    t.close()


@pytest.mark.parametrize("device", (False, True), ids=("step", "step_device"))
def test_forced_steps_without_a_child_and_illegal_ones(gmk, oracle, device):
    """game 0 steps to a free cell that has no child, game 1 to an occupied cell, game 2 to no cell of the board"""
    G = gmk
    pos = POSITIONS[5]                                          # six stones, 95 root children
    t = G.TraditionalMCTS(3, node_capacity=CAP)
    t.set_positions([pos, pos, pos])
    t.run(17)                                                   # (17 + 9 playouts of at most 119 children each stay below CAP nodes)
    orcs = [oracle.TraditionalMCTS(5.0), oracle.TraditionalMCTS(5.0)]
    orcs[0].search(pos, 17)
    orcs[1].run(pos, 17)                                        # (the oracle keeps a tree between run() calls only; no noise was set)
    before = t.root_stats()
    _same_search(before, 0, orcs[0])
    _same_search(before, 1, orcs[1], nodes=False)
    childless = [m for m in range(N) if m not in pos and before["priors"][0][m] == 0.0]
    assert childless and before["visits"][0][childless[0]] == 0
    cells = np.array([childless[0], pos[2], 225], np.int16)
    if device:
        t.step_device(torch.from_numpy(cells).to(DEV), torch.full((3,), G.MATCH_MOVED, dtype=torch.int32, device=DEV), fresh_root=False)
        torch.cuda.synchronize()
    else:
        t.step(cells)
    after = t.root_stats()
    assert after["n_nodes"][0] == 1 and after["status"][0] == 0 and after["best"][0] == -1 and after["root_visits"][0] == 0
    for g in (1, 2):
        assert after["status"][g] == t.STATUS_ILLEGAL_STEP
        for k in ("visits", "values", "priors"):                # the whole tree went through copy_subtree from node 0
            np.testing.assert_array_equal(after[k][g].view(np.uint32), before[k][g].view(np.uint32))
        for k in ("best", "n_nodes", "root_visits", "root_value"):
            assert after[k][g] == before[k][g], k
    t.run(9)
    orcs[0].search(pos + [childless[0]], 9)
    orcs[1].run(pos, 9)                                         # the kept tree is searched on
    st = t.root_stats()
    _same_search(st, 0, orcs[0])
    for g in (1, 2):
        assert st["status"][g] == t.STATUS_ILLEGAL_STEP
        st["status"][g] = 0
        _same_search(st, g, orcs[1], nodes=False)
        assert _position_of(t, g, len(pos)) == pos
    assert _position_of(t, 0, len(pos) + 1) == pos + [childless[0]]
    t.close()


@pytest.mark.parametrize("persistent", (False, True), ids=("lockstep", "persistent"))
def test_a_self_play_game_whose_root_has_no_child_ends_where_it_stands(gmk, persistent):
    """An opening that is a finished game: the search finds nothing to play; the record keeps the opening, the
    slot goes on to the next game."""
    G = gmk
    openings = [FIVE, POSITIONS[3], FIVE]
    open_moves = np.zeros((3, 16), np.uint8)
    for g, o in enumerate(openings):
        open_moves[g, :len(o)] = o
    open_lens = np.array([len(o) for o in openings], np.int32)
    t = G.TraditionalMCTS(2, node_capacity=CAP)                 # two slots: the third game waits for one
    d_moves, d_visits, d_lens, d_winner = _records(3)
    t.selfplay_run(3, 0, 3, d_moves.data_ptr(), d_visits.data_ptr(), d_lens.data_ptr(), d_winner.data_ptr(), open_moves, open_lens, persistent=persistent)
    torch.cuda.synchronize()
    lens, winner, moves, rec = d_lens.cpu().numpy(), d_winner.cpu().numpy(), d_moves.cpu().numpy(), d_visits.cpu().numpy()
    assert list(lens[[0, 2]]) == [len(FIVE), len(FIVE)]
    assert [int(m) for m in moves[0, :len(FIVE)]] == FIVE and [int(m) for m in moves[2, :len(FIVE)]] == FIVE
    assert (rec[0] == 9).all() and (rec[2] == 9).all()          # no searched ply: no visit row written
    assert lens[1] > len(POSITIONS[3]) and (winner[1] != 0 or lens[1] == N)
    t.close()
