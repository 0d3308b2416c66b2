"""The two calls a device-resident match makes of a K3 handle, on the GPU: gmk_mcts_root_choice against root_stats and against the move
gmk_mcts_step makes with -1, in either arena, with games that were never searched and games that are finished; gmk_mcts_step_device against
gmk_mcts_step_host on a twin handle (the games that moved), against a handle that was left alone (the games that did not) and against
itself (the game that ended, the illegal requests)."""
import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

N = 225
DEV = "cuda"
PLAYOUTS = 30
FOUR = [15 * 3 + 3, 0, 15 * 3 + 4, 2, 15 * 3 + 5, 4, 15 * 3 + 6, 6]      # black has four in row 3 and the move: (7, 3) or (2, 3) wins
WINS = 15 * 3 + 7


def _positions(n, four_first=False, with_moves=False):
    """n short openings of the synthetic generator (0 .. 8 plies, game g's cut at (3 g + 2) % 9) -> planes, last moves, stones"""
    moves, lens, _ = G.synth_boards(n, 0, seed=21, first_board=100, stride=N)
    lens = np.minimum(lens, (3 * np.arange(n) + 2) % 9).astype(np.int32)
    if four_first:
        moves[0, :8], lens[0] = FOUR, 8
    last = np.array([moves[g, lens[g] - 1] if lens[g] else -1 for g in range(n)], dtype=np.int16)
    return (G.moves_to_planes(moves, lens), last, lens) + ((moves,) if with_moves else ())


def _tree(n, planes, last, seed=13):
    tree = G.BatchedMCTS(n, playouts_capacity=4 * PLAYOUTS, seed=seed)
    tree.set_roots(planes, last, first_game_id=50)
    return tree


def _choice(tree):
    cells, rows = torch.full((tree.n,), 99, dtype=torch.int16, device=DEV), torch.full((tree.n, N), 9, dtype=torch.int16, device=DEV)
    tree.root_choice(cells, rows)
    bare = torch.full((tree.n,), 99, dtype=torch.int16, device=DEV)
    tree.root_choice(bare, None)
    assert bare.tolist() == cells.tolist()
    return cells.cpu().numpy(), rows.cpu().numpy().view(np.uint16)


def _holds_root_stats(tree, finished=()):
    """root_choice is what root_stats reports: the first maximum in child (= cell) order, the counts saturated; -1 and a zero row for a
    finished game"""
    visits, _, _, _, status = tree.root_stats()
    cells, rows = _choice(tree)
    live = np.ones(tree.n, dtype=bool)
    live[list(finished)] = False
    assert ((status & 1) == 0).tolist() == live.tolist()
    expect = np.where(live & (visits.max(1) > 0), visits.argmax(1), -1)
    assert cells.tolist() == expect.tolist()
    assert (rows == np.where(live[:, None], np.minimum(visits, 65535), 0)).all()
    assert (cells[live] >= 0).all() and (rows[live].astype(np.int64).sum(1) == visits[live].sum(1)).all()
    return cells


@pytest.mark.parametrize("n", [1, 3, 70])
def test_root_choice_is_root_stats_and_the_step_with_minus_one(n):
    G.init(0)
    planes, last, _ = _positions(n)
    tree, twin = _tree(n, planes, last), _tree(n, planes, last)
    try:
        cells, rows = _choice(tree)                                   # rooted, never searched: no child to play
        assert cells.tolist() == [-1] * n and not rows.any()
        tree.run(PLAYOUTS)
        twin.run(PLAYOUTS)
        cells = _holds_root_stats(tree)
        # the twin plays gmk_mcts_step's own choice (-1) into a record: the same cell
        forced = torch.full((n,), -1, dtype=torch.int16, device=DEV)
        d_moves, d_lens = torch.zeros((n, N), dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        d_winner, d_unfinished = torch.zeros(n, dtype=torch.int8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        twin.step(forced.data_ptr(), d_moves.data_ptr(), None, d_lens.data_ptr(), d_winner.data_ptr(), d_unfinished.data_ptr(), True, None)
        torch.cuda.synchronize()
        assert d_lens.tolist() == [1] * n and d_moves[:, 0].tolist() == cells.tolist()
        # the kept subtree is in the other arena now: the second search's roots are read there
        tree.step_host(cells, reuse_subtree=True)
        kept, _ = _choice(tree)                                       # (the kept subtree's counts, before any new playout)
        visits = tree.root_stats()[0]
        assert kept.tolist() == np.where(visits.max(1) > 0, visits.argmax(1), -1).tolist()
        tree.run(PLAYOUTS)
        twin.run(PLAYOUTS)
        again = _holds_root_stats(tree)
        assert (tree.root_stats()[0] == twin.root_stats()[0]).all() and again.tolist() == _choice(twin)[0].tolist()
    finally:
        tree.close()
        twin.close()


@pytest.mark.parametrize("n", [1, 3, 70])
def test_root_choice_of_a_finished_game(n):
    G.init(0)
    planes, last, _ = _positions(n, four_first=True)
    tree = _tree(n, planes, last)
    try:
        tree.run(PLAYOUTS)
        moves = np.full(n, -1, dtype=np.int16)
        moves[0] = WINS                                               # game 0 completes its five: finished, status bit 0
        tree.step_host(moves, reuse_subtree=True)
        tree.run(PLAYOUTS)
        _holds_root_stats(tree, finished=(0,))
    finally:
        tree.close()


def _stats(tree):
    visits, q, rv, nodes, status = tree.root_stats()
    return {"visits": visits, "q": q.view(np.uint32), "root_visits": rv, "nodes": nodes, "status": status}


def _same(a, b, games, but=()):
    return all((a[k][games] == b[k][games]).all() for k in a if k not in but)


@pytest.mark.parametrize("fresh", [False, True], ids=["kept", "fresh"])
def test_step_device_against_step_host(fresh):
    """Five games after the same search.  Games 0 and 1 MOVED (the handle's choice; a legal cell whose child was never visited), game 2
    ENDED on its choice, game 3 was REFUSED (its cell: -1, which must mean nothing), game 4 was OVER (its cell: an occupied one)."""
    G.init(0)
    n = 5
    planes, last, lens, moves = _positions(n, with_moves=True)
    assert lens[4] > 0
    dev, host, still = (_tree(n, planes, last) for _ in range(3))
    try:
        for tree in (dev, host, still):
            tree.run(PLAYOUTS)
        before = _stats(dev)
        choice, _ = _choice(dev)
        stones = {int(c) for c in moves[1, :lens[1]]}
        unvisited = max(c for c in range(N) if c not in stones and before["visits"][1][c] == 0)      # an empty cell of game 1 whose child no playout took
        taken = int(last[4])
        cells = np.array([choice[0], unvisited, choice[2], -1, taken], dtype=np.int16)
        verdict = np.array([G.MATCH_MOVED, G.MATCH_MOVED, G.MATCH_ENDED, G.MATCH_REFUSED, G.MATCH_OVER], dtype=np.int32)
        dev.step_device(torch.from_numpy(cells).to(DEV), torch.from_numpy(verdict).to(DEV), fresh_root=fresh)
        host.step_host(np.array([choice[0], unvisited, choice[2], -1, -1], dtype=np.int16), reuse_subtree=not fresh)
        after, twin = _stats(dev), _stats(host)
        assert _same(after, twin, [0, 1]) and _same(after, before, [3, 4])
        assert after["status"].tolist() == [0, 0, 1, 0, 0] and after["nodes"][2] == 1 and not after["visits"][2].any()
        if fresh:
            assert after["nodes"][:2].tolist() == [1, 1] and not after["visits"][:2].any()
        else:
            assert after["root_visits"][0] == before["visits"][0][choice[0]] > 0 and after["nodes"][0] > 1 and after["nodes"][1] == 1
        for tree in (dev, host, still):
            tree.run(PLAYOUTS)
        after, twin, alone = _stats(dev), _stats(host), _stats(still)
        assert _same(after, twin, [0, 1])                            # the games that moved: the twin's trees, bit for bit
        assert (after["root_visits"][:2] >= PLAYOUTS).all() and (after["visits"][[0, 1], [cells[0], cells[1]]] == 0).all()
        assert after["root_visits"][2] == 0 and after["status"][2] == 1 and not after["visits"][2].any()      # the game that ended: not searched again
        assert _same(after, alone, [3, 4])                           # the games that did not move: as if nothing had been called
        assert (after["root_visits"][3:] == 2 * PLAYOUTS).all()
        # an illegal cell under MOVED: status bit 2, the tree stays (occupied, off the board, -1)
        for bad in (int(cells[0]), 225, -1):
            was = _stats(dev)
            cells2 = np.array([bad, -1, -1, -1, -1], dtype=np.int16)
            verdict2 = np.array([G.MATCH_MOVED] + [G.MATCH_REFUSED] * 4, dtype=np.int32)
            dev.step_device(torch.from_numpy(cells2).to(DEV), torch.from_numpy(verdict2).to(DEV), fresh_root=fresh)
            now = _stats(dev)
            assert _same(now, was, [0, 1, 2, 3, 4], but=("status",)) and now["status"].tolist() == [G.BatchedMCTS.STATUS_ILLEGAL_STEP, 0, 1, 0, 0]
        cells_dev, _ = _choice(dev)
        assert cells_dev[2] == -1 and (cells_dev[[0, 1, 3, 4]] >= 0).all()
    finally:
        for tree in (dev, host, still):
            tree.close()


def test_the_entries_refuse_what_they_cannot_serve():
    G.init(0)
    tree = G.BatchedMCTS(2, playouts_capacity=PLAYOUTS, seed=1)
    cells, verdict = torch.zeros(2, dtype=torch.int16, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    try:
        with pytest.raises(G.GmkError, match="gmk_mcts_set_roots has not been called"):      # GMK_ERR_STATE: no roots
            tree.root_choice(cells)
        with pytest.raises(G.GmkError, match="gmk_mcts_set_roots has not been called"):
            tree.step_device(cells, verdict)
        L = G.load()
        assert L.gmk_mcts_root_choice(tree.h, None, None, None) != 0 and L.gmk_mcts_step_device(tree.h, cells.data_ptr(), None, 0, None) != 0
        assert L.gmk_mcts_root_choice(None, cells.data_ptr(), None, None) != 0 and L.gmk_mcts_step_device(None, cells.data_ptr(), verdict.data_ptr(), 0, None) != 0
    finally:
        tree.close()
