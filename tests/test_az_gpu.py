"""K7 parity: the lock-step network-guided search (gmk_az_*) against the oracle's MCTS with an external evaluator
(Policy(eval_state=f), agents/alphazero.py:5-9; Default::Select / Expand(extraCheck) / BackPropogate).  The evaluator of the
parity test is a pure function of the feature planes that both sides compute on the host with the same numpy code, so
the search itself is compared exactly (visit counts, value and prior bits, tree size); the real network is run end to end
in a second test and checked against a float64 forward pass (tests/pvnet_reference.py) with a tolerance."""
import ctypes as C

import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu


def surrogate(states):
    """states uint8/float [6, 15, 15] -> (value, probs): deterministic, exactly reproducible, with zero probabilities on some
    empty cells and non-zero ones on some occupied cells (so that both halves of Default::Expand's test matter)."""
    s = np.asarray(states).reshape(6, 225).astype(np.int64)
    code = s[0] * 3 + s[1] * 5 + s[3] * 7 + s[4] * 11 + s[5]
    idx = np.arange(225, dtype=np.int64)
    h = (int((code * (idx + 1)).sum()) * 2654435761 + idx * 40503 * (int(code.sum()) + 1)) % 65536
    probs = ((h % 1021) + 1).astype(np.float32) / np.float32(1024.0)
    probs[h % 7 == 0] = 0.0
    value = np.float32((int(h.sum()) % 2001) - 1000) / np.float32(1000.0)
    return value, probs


def _roots(n, max_len):
    moves, lens, _ = G.synth_boards(n, 1, first_board=500)
    lens = np.array([min(int(lens[g]), (3 * g) % (max_len + 1)) for g in range(n)], dtype=np.int32)
    planes = G.moves_to_planes(moves, lens)
    last = np.full((n, 2), -1, np.int16)
    for g in range(n):
        if lens[g] >= 1: last[g, 0] = moves[g, lens[g] - 1]
        if lens[g] >= 2: last[g, 1] = moves[g, lens[g] - 2]
    return moves, lens, planes, last


def test_search_matches_oracle(oracle):
    import torch
    O = oracle
    G.init()
    n, playouts = 12, 160
    moves, lens, planes, last = _roots(n, 30)
    tree = G.AlphaZeroMCTS(n, node_capacity=1 << 16, c_puct=5.0)
    tree.set_roots(planes, last)

    def host_network(states):                                   # the batch goes to the host, through the surrogate, and back
        s = states.cpu().numpy()
        vp = [surrogate(s[g]) for g in range(n)]
        return (torch.tensor([v for v, _ in vp], dtype=torch.float32, device="cuda"),
                torch.from_numpy(np.stack([p for _, p in vp])).cuda())
    tree.search(host_network, playouts)
    st = tree.root_stats()
    assert (st["status"] == 0).all()
    for g in range(n):
        b = O.new_board()
        for i in range(int(lens[g])):
            O.lib().go_board_apply(C.byref(b), int(moves[g, i]), 1)
        om = O.MCTS(playouts, 5.0, 5, 0, 0)
        om.set_evaluator(surrogate)
        om.run_playouts(b)
        v, q, p = om.root_children()
        np.testing.assert_array_equal(st["visits"][g], v)
        np.testing.assert_array_equal(st["values"][g].view(np.uint32), q.view(np.uint32))
        np.testing.assert_array_equal(st["priors"][g].view(np.uint32), p.view(np.uint32))
        assert st["root_visits"][g] == om.root_visits and st["n_nodes"][g] == om.size
        assert np.float32(st["root_value"][g]).view(np.uint32) == np.float32(om.root_value).view(np.uint32)
    tree.close()


def test_finished_games_and_full_arena():
    import torch
    G.init()
    c = lambda y, x: y * 15 + x
    won = [c(7, 7), c(0, 0), c(7, 8), c(0, 2), c(7, 9), c(0, 4), c(7, 10), c(0, 6), c(7, 11)]          # black has five: the root is terminal
    moves = np.zeros((2, 64), np.uint8); moves[0, :9] = won; moves[1, :3] = [112, 113, 127]
    lens = np.array([9, 3], np.int32)
    planes = G.moves_to_planes(moves, lens)
    tree = G.AlphaZeroMCTS(2, node_capacity=256, c_puct=5.0)
    tree.set_roots(planes, np.array([[won[-1], won[-2]], [127, 113]], np.int16))
    uniform = lambda s: (torch.zeros(2, device="cuda"), torch.full((2, 225), 1.0 / 225, device="cuda"))
    tree.search(uniform, 40)
    st = tree.root_stats()
    assert st["root_visits"][0] == 40 and st["root_value"][0] == 1.0 and st["n_nodes"][0] == 1        # every playout ends at the root: its player won
    assert st["status"][1] & 2 and st["n_nodes"][1] <= 256                                             # 222 children per node: the second expansion does not fit
    tree.close()


def test_policy_value_network_end_to_end():
    import torch
    from gomokuai_amd.network import PolicyValueNetwork
    G.init()
    torch.manual_seed(0)
    net = PolicyValueNetwork(seed=3).cuda().eval()
    n, playouts = 64, 48
    _, lens, planes, last = _roots(n, 20)
    tree = G.AlphaZeroMCTS(n, node_capacity=1 << 15, c_puct=5.0)
    tree.set_roots(planes, last)
    with torch.no_grad():
        tree.search(net, playouts)
        st = tree.root_stats()
        states = tree.select().clone()                          # one more batch of leaves, for the numerics check below
        value, probs = net(states)
    assert (st["status"] == 0).all() and (st["root_visits"] == playouts).all()
    assert (st["visits"].sum(1) == playouts - 1).all()
    assert ((st["priors"] > 0).sum(1) == 225 - lens).all()     # softmax never returns 0: one child per empty cell
    assert float(probs.sum(1).sub(1).abs().max()) < 1e-5 and float(value.abs().max()) <= 1.0
    # float64 forward pass of the same weights (model_tf.py:28-66, tests/pvnet_reference.py) on a few rows
    import pvnet_reference
    ref = pvnet_reference.forward(pvnet_reference.weights(net), states[:4])
    assert np.abs(probs[:4].cpu().numpy() - ref["probs"]).max() < 1e-4      # float32 convolutions vs float64: tolerance
    assert np.abs(value[:4].cpu().numpy() - ref["value"]).max() < 1e-4
    tree.close()


@pytest.mark.parametrize("sampler", [0, 1])
def test_step_keeps_the_subtree_and_noise(oracle, sampler):
    """gmk_az_step + gmk_az_add_root_noise: search, step to the most visited child, step to the opponent's reply (a child or
    not), search again from the kept subtree with fresh root noise: equal to the oracle's persistent MCTS object -- with the noise drawn on the
    host (sampler 0: std::gamma_distribution) and on the device (sampler 1: the counter-based sampler of include/gomoku_noise.h, az_root_noise_kernel)."""
    import torch
    O = oracle
    G.init()
    n, playouts = 6, 90
    moves, lens, planes, last = _roots(n, 12)
    tree = G.AlphaZeroMCTS(n, node_capacity=1 << 17, c_puct=5.0)
    tree.set_option(G.OPT_NOISE_SAMPLER, sampler)
    tree.set_roots(planes, last)

    def host_network(states):
        s = states.cpu().numpy()
        vp = [surrogate(s[g]) for g in range(n)]
        return (torch.tensor([v for v, _ in vp], dtype=torch.float32, device="cuda"), torch.from_numpy(np.stack([p for _, p in vp])).cuda())
    boards, orcs = [], []
    for g in range(n):
        b = O.new_board()
        for i in range(int(lens[g])):
            O.lib().go_board_apply(C.byref(b), int(moves[g, i]), 1)
        om = O.MCTS(playouts, 5.0, 5, 777, 20 + g)
        om.set_evaluator(surrogate)
        om.set_noise(0.05, 0.25, sampler=sampler)
        boards.append(b); orcs.append(om)
    kept = 0
    for rnd in range(3):
        tree.add_root_noise(0.05, 0.25, seed=777, first_game_id=20)
        tree.search(host_network, playouts)
        st = tree.root_stats()
        assert (st["status"] == 0).all()
        best = np.full(n, -1, np.int16); reply = np.full(n, -1, np.int16)
        for g in range(n):
            if boards[g].cur_player == 0:
                continue
            orcs[g].run_playouts(boards[g])
            v, q, p = orcs[g].root_children()
            where = "round %d game %d" % (rnd, g)
            np.testing.assert_array_equal(st["priors"][g].view(np.uint32), p.view(np.uint32), where)
            np.testing.assert_array_equal(st["visits"][g], v, where)
            np.testing.assert_array_equal(st["values"][g].view(np.uint32), q.view(np.uint32), where)
            assert st["root_visits"][g] == orcs[g].root_visits, where
            kept = max(kept, int(st["root_visits"][g]) - playouts)
            best[g] = orcs[g].step_forward()
            O.lib().go_board_apply(C.byref(boards[g]), int(best[g]), 1)
        tree.step(best)
        for g in range(n):
            if boards[g].cur_player == 0:
                continue
            free = [c for c in range(225) if boards[g].states[1][c]]
            kv = orcs[g].root_children()[0]
            reply[g] = int(np.argmax(kv)) if (g % 2 == 0 and kv.any()) else free[g]
            O.lib().go_board_apply(C.byref(boards[g]), int(reply[g]), 1)
        tree.step(reply)
    assert kept > 0
    tree.close()


def test_nearly_full_boards(oracle):
    """Roots with 1 .. 12 empty cells (shuffled tie games): leaves at full boards (ties) inside the tree, priors on occupied
    cells dropped by Default::Expand's legality check, trees that run out of leaves."""
    import torch
    O = oracle
    G.init()
    rng = np.random.RandomState(17)
    cls = lambda c: ((c % 15) // 2 + c // 15) % 2             # two colour classes that never line up five
    blacks, whites = [c for c in range(225) if cls(c) == 0], [c for c in range(225) if cls(c) == 1]
    n, playouts = 8, 200
    moves = np.zeros((n, 225), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    for g in range(n):
        b, w = list(rng.permutation(blacks)), list(rng.permutation(whites))
        seq = []
        while b or w:
            if b:
                seq.append(b.pop())
            if w:
                seq.append(w.pop())
        moves[g] = seq
        lens[g] = rng.randint(213, 225)
    planes = G.moves_to_planes(moves, lens)
    last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
    tree = G.AlphaZeroMCTS(n, node_capacity=1 << 14, c_puct=5.0)
    tree.set_roots(planes, last)

    def host_network(states):
        s = states.cpu().numpy()
        vp = [surrogate(s[g]) for g in range(n)]
        return (torch.tensor([v for v, _ in vp], dtype=torch.float32, device="cuda"), torch.from_numpy(np.stack([p for _, p in vp])).cuda())
    tree.search(host_network, playouts)
    st = tree.root_stats()
    assert (st["status"] == 0).all()
    for g in range(n):
        b = O.new_board()
        for i in range(int(lens[g])):
            O.lib().go_board_apply(C.byref(b), int(moves[g, i]), 1)
        om = O.MCTS(playouts, 5.0, 5, 0, 0)
        om.set_evaluator(surrogate)
        om.run_playouts(b)
        v, q, p = om.root_children()
        np.testing.assert_array_equal(st["visits"][g], v)
        np.testing.assert_array_equal(st["values"][g].view(np.uint32), q.view(np.uint32))
        assert st["root_visits"][g] == om.root_visits and st["n_nodes"][g] == om.size
    tree.close()


def test_set_slots_checks_every_opening():
    """gmk_az_set_slots: the openings of ALL games are checked on the host (the later ones are played by the device, unseen): a cell
    outside the board, a cell played twice and an opening of more than eight moves are refused, for a game that starts in a slot and for
    one that waits."""
    t = G.AlphaZeroMCTS(2, node_capacity=4096)
    good = np.array([[112, 113, 0], [0, 1, 2], [7, 8, 9], [30, 31, 32]], dtype=np.uint8)
    t.set_slots(4, good, np.array([2, 3, 3, 1], dtype=np.int32))
    assert t.live == 2
    for bad_game in (0, 3):
        for bad in ([230, 1, 2], [5, 5, 6]):
            m = good.copy()
            m[bad_game] = bad
            with pytest.raises(G.GmkError):
                t.set_slots(4, m, np.array([3, 3, 3, 3], dtype=np.int32))
    with pytest.raises(G.GmkError):
        t.set_slots(4, np.zeros((4, 12), dtype=np.uint8) + np.arange(12, dtype=np.uint8), np.array([9, 1, 1, 1], dtype=np.int32))
    t.close()


def test_advance_plays_late_positions_to_their_end(oracle):
    """gmk_az_advance from positions with 2 .. 20 empty cells (no five on the board yet): every ply's recorded move is the root's most
    visited child (first maximum in cell order), its visit counts are the root's, the records replay on the oracle's board to a finished
    game with the recorded winner (five in a row, or the tie of a full board), and the leaf batch shrinks with the games (live rows only)."""
    import torch
    O = oracle
    G.init()
    rng = np.random.RandomState(23)
    cls = lambda c: ((c % 15) // 2 + c // 15) % 2
    blacks, whites = [c for c in range(225) if cls(c) == 0], [c for c in range(225) if cls(c) == 1]
    n, playouts = 10, 40
    moves = np.zeros((n, 225), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    for g in range(n):
        b, w = list(rng.permutation(blacks)), list(rng.permutation(whites))
        seq = []
        while b or w:
            if b:
                seq.append(b.pop())
            if w:
                seq.append(w.pop())
        rng.shuffle(seq[205:])                                   # the tail in any order: fives become possible
        moves[g] = seq
        lens[g] = 205 + 2 * g
    start = lens.copy()
    planes = G.moves_to_planes(moves, lens)
    last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
    tree = G.AlphaZeroMCTS(n, node_capacity=1 << 15, c_puct=5.0)
    tree.set_roots(planes, last)
    d_moves = torch.from_numpy(np.where(np.arange(225)[None, :] < lens[:, None], moves, 0).astype(np.uint8)).cuda()
    d_lens, d_winner = torch.from_numpy(lens.copy()).cuda(), torch.zeros(n, dtype=torch.int8, device="cuda")
    d_visits = torch.zeros((n, 225, 225), dtype=torch.int16, device="cuda")

    def host_network(states):
        s = states.cpu().numpy()
        vp = [surrogate(s[g]) for g in range(s.shape[0])]
        return (torch.tensor([v for v, _ in vp], dtype=torch.float32, device="cuda"), torch.from_numpy(np.stack([p for _, p in vp])).cuda())

    live_rows = []
    stalled = np.zeros(n, dtype=bool)                             # the search had nothing to play: the evaluator gave every empty cell probability 0
    for _ in range(30):
        live_rows.append(tree.live)
        tree.search(host_network, playouts)
        st = tree.root_stats()
        before = d_lens.cpu().numpy().copy()
        over_before = (st["status"] & G.AlphaZeroMCTS.STATUS_OVER) != 0
        left = tree.advance(d_moves, d_visits, d_lens, d_winner, reuse_subtree=True)
        after, rec, vis = d_lens.cpu().numpy(), d_moves.cpu().numpy(), d_visits.cpu().numpy()
        for g in range(n):
            if over_before[g] or st["visits"][g].max() == 0:
                assert after[g] == before[g]
                stalled[g] |= not over_before[g]
                continue
            assert after[g] == before[g] + 1 and rec[g, before[g]] == int(st["visits"][g].argmax())
            assert (vis[g, before[g]].astype(np.int64) == np.minimum(st["visits"][g], 65535)).all()
        assert left == tree.live
        if left == 0:
            break
    assert tree.live == 0 and live_rows[0] == n and live_rows == sorted(live_rows, reverse=True) and live_rows[-1] < n
    rec, rl, rw = d_moves.cpu().numpy(), d_lens.cpu().numpy(), d_winner.cpu().numpy()
    ties = 0
    for g in range(n):
        b = O.new_board()
        for i in range(int(rl[g])):
            assert O.lib().go_board_check_move(C.byref(b), int(rec[g, i])), "game %d move %d" % (g, i)
            assert b.cur_player != 0 or i < start[g]
            O.lib().go_board_apply(C.byref(b), int(rec[g, i]), 1)
        assert (rec[g, :start[g]] == moves[g, :start[g]]).all()
        if stalled[g]:                                            # ended where it stood (as the host-driven loop ends it): no winner
            assert b.cur_player != 0 and rw[g] == 0, "game %d" % g
        else:
            assert b.cur_player == 0 and b.winner == int(rw[g]), "game %d" % g
        ties += int(rw[g] == 0 and rl[g] == 225)
    assert int((~stalled).sum()) >= n // 2
    tree.close()
