"""K7 with the network evaluated over the board's symmetries ("K22"): AlphaZeroMCTS.search through FusedPolicyValueNetwork.symmetric against the
same search through a callable composed in torch (index operations, the plain fused network, ordered float32 sums), the captured step against
the eager one, the self-play and match loops against each other, and the front end's NetworkAgent against a direct search."""
import numpy as np
import pytest

import pvnet_sym_reference as S
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from test_az_leaves_gpu import _roots

pytestmark = pytest.mark.gpu

N = 225
SEED = 0x9E3779B97F4A7C15
cell = lambda y, x: 15 * y + x
# four asymmetric positions (no symmetry of the board maps any of them to itself), black or white to move
OPENINGS = [[cell(7, 7), cell(7, 8), cell(8, 9)], [cell(3, 4), cell(4, 4), cell(5, 6), cell(2, 9)], [cell(7, 7), cell(6, 8), cell(9, 8), cell(8, 6), cell(5, 5)],
            [cell(10, 3), cell(11, 5)]]
SIX_PLIES = [cell(7, 7), cell(7, 8), cell(8, 8), cell(6, 6), cell(8, 9), cell(9, 7)]


@pytest.fixture(scope="module")
def fused():
    import torch
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=8).cuda().eval())
    torch.cuda.synchronize()
    yield net
    net.close()


def composed(fused, mode, seed=SEED):
    """network(states) -> (value, probs) built from torch index operations around the plain fused network: the statement of
    include/gomoku_symmetry.h a second time, with tests/pvnet_sym_reference.py's tables (np.rot90 of the cell numbers)"""
    import torch
    src = [torch.from_numpy(S.transform(np.arange(N).reshape(1, 15, 15), a).reshape(N).astype(np.int64)).cuda() for a in range(8)]

    def one(states, a):
        n = states.shape[0]
        v, q = fused(states.reshape(n, 6, N)[:, :, src[a]].reshape(n, 6, 15, 15).contiguous())
        p = torch.empty_like(q)
        p[:, src[a]] = q                                         # p[src_a(j)] = q[j]
        return v, p

    def network(states):
        if mode == "all":
            v, p = one(states, 0)
            for a in range(1, 8):
                va, pa = one(states, a)
                v, p = v + va, p + pa
            return v * 0.125, p * 0.125
        pick = S.pick(states.cpu().numpy(), seed)
        v, p = torch.empty(states.shape[0], device="cuda"), torch.empty((states.shape[0], N), device="cuda")
        for a in range(8):
            rows = torch.from_numpy(np.nonzero(pick == a)[0]).cuda()
            if len(rows):
                v[rows], p[rows] = one(states[rows].contiguous(), a)
        return v, p
    return network


def _tree(leaves):
    tree = G.AlphaZeroMCTS(len(OPENINGS), node_capacity=1 << 14, c_puct=5.0, leaves=leaves)
    tree.set_roots(*_roots(OPENINGS))
    return tree


def _same_stats(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = (a[k].view(np.uint32), b[k].view(np.uint32)) if a[k].dtype == np.float32 else (a[k], b[k])
        np.testing.assert_array_equal(x, y, "%s: %s" % (what, k))


@pytest.mark.parametrize("leaves", [1, 4])
@pytest.mark.parametrize("mode", ["all", "random"])
def test_search_equals_the_torch_composition_and_the_captured_step(fused, mode, leaves):
    trees = [_tree(leaves) for _ in range(4)]
    try:
        sym = fused.symmetric(mode, SEED)
        trees[0].search(sym, 32)
        trees[1].search(composed(fused, mode), 32)
        trees[2].search(sym, 32, graph=True)
        trees[3].search(fused, 32)
        stats = [t.root_stats() for t in trees]
        assert (stats[0]["root_visits"] == 32).all() and (stats[0]["status"] == 0).all()
        _same_stats(stats[0], stats[1], "symmetric(%r) against the composition" % mode)
        _same_stats(stats[0], stats[2], "graph=True against the eager search")
        assert (stats[0]["priors"].view(np.uint32) != stats[3]["priors"].view(np.uint32)).any()      # (not the plain network's search)
    finally:
        for t in trees:
            t.close()


def _same_records(a, b):
    assert not a.overflow and not b.overflow
    assert (a.lens == b.lens).all() and (a.winner == b.winner).all()
    for g in range(len(a.lens)):
        n = int(a.lens[g])
        assert (a.moves[g, :n] == b.moves[g, :n]).all() and (a.visits[g, :n] == b.visits[g, :n]).all(), g


def test_self_play_is_one_set_of_games_on_every_loop(fused):
    """the pick of "random" is keyed by a leaf's position and the seed, not by its row: live-only batches, slots and the host loop play the
    same games"""
    kw = dict(opening_plies=2, first_game_id=70, seed=2, root_noise=(0.05, 0.25), symmetry="random")
    full = selfplay.play_network_games(6, fused, 8, **kw).cpu()
    few = selfplay.play_network_games(6, fused, 8, slots=4, **kw).cpu()
    host = selfplay.play_network_games(6, fused, 8, device_loop=False, **kw).cpu()
    _same_records(full, few)
    _same_records(full, host)
    assert int(full.lens.min()) >= 9 and all(int(full.lens[g]) == N or int(full.winner[g]) != 0 for g in range(6))
    kw["symmetry"] = None
    plain = selfplay.play_network_games(6, fused, 8, **kw).cpu()
    assert any(int(plain.lens[g]) != int(full.lens[g]) or (plain.moves[g] != full.moves[g]).any() for g in range(6))


def test_the_match_runs_on_both_loops(fused):
    opponent = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 50})
    kw = dict(playouts=16, seed=9, first_game_id=40, leaves=4, symmetry="all")
    (rd, bd, sd), (rh, bh, sh) = (selfplay.play_evaluation_games(4, fused, opponent, device_loop=loop, **kw) for loop in (True, False))
    assert (bd == bh).all() and (sd == sh).all()
    _same_records(rd.cpu(), rh.cpu())
    plain = selfplay.play_evaluation_games(4, fused, opponent, device_loop=True, **dict(kw, symmetry=None))[0].cpu()
    assert any((plain.moves[g] != rd.cpu().moves[g]).any() for g in range(4))


@pytest.mark.parametrize("symmetry", ["all", None])
def test_network_agent_plays_the_direct_searchs_cell(fused, symmetry):
    from gomokuai_amd import core
    from gomokuai_amd.interface import NetworkAgent, VCFAgent
    board = core.Board()
    for c in SIX_PLIES:
        board.apply_move(core.Position(c))
    agent = NetworkAgent(fused, iterations=48, leaves=4, symmetry=symmetry, c_puct=5.0, quiet=True)
    try:
        agent.sync_with_board(board)
        move = agent.get_action(board)

        def direct(moves):
            tree = G.AlphaZeroMCTS(1, node_capacity=1 << 14, c_puct=5.0, leaves=4)
            try:
                tree.set_roots(*_roots([moves]))
                tree.search(fused.symmetric("all") if symmetry else fused, 48)
                st = tree.root_stats()
                return int(st["visits"][0].argmax()), st
            finally:
                tree.close()
        want, st = direct(SIX_PLIES)
        assert int(move.id) == want and st["visits"][0, want] > 0
        assert agent.debug_message()["playouts"] == 48 and agent.debug_message()["symmetry"] == (symmetry or "none")
        board.apply_move(move)
        reply = next(c for c in range(N) if c not in SIX_PLIES and c != want)
        board.apply_move(core.Position(reply))
        agent.sync_with_board(board)                             # after a reply it follows the board
        assert int(agent.get_action(board).id) == direct(SIX_PLIES + [want, reply])[0]
        if symmetry:
            front = VCFAgent(agent, depth=4)                      # the solver in front of it, as for the other agents
            front.sync_with_board(board)
            played = int(front.get_action(board).id)
            assert "vcf" in front.debug_message() and front.own["status"] in ("WIN", "NONE", "BUDGET", "DEPTH")
            assert played == (front.own["move"] if front.own["status"] == "WIN" else direct(SIX_PLIES + [want, reply])[0])
    finally:
        agent.close()
    with pytest.raises(ValueError):
        NetworkAgent(fused, iterations=8, symmetry="mean")
    with pytest.raises(ValueError):
        NetworkAgent(lambda s: None, iterations=8, symmetry="all")


def test_make_agent_reads_the_weights_and_the_time_budget(fused, tmp_path):
    import torch
    from gomokuai_amd import core
    from gomokuai_amd.interface import NetworkAgent, make_agent
    torch.save(fused.net.state_dict(), tmp_path / "w.pt")
    agent = make_agent("network:%s:3.5" % (tmp_path / "w.pt"), milliseconds=30, quiet=True, leaves=2, symmetry="random")
    try:
        assert isinstance(agent, NetworkAgent) and agent.c_puct == 3.5 and agent.leaves == 2 and agent.symmetry == "random" and agent.ms == 30
        board = core.Board()
        board.apply_move(core.Position(cell(7, 7)))
        agent.sync_with_board(board)
        move = agent.get_action(board)
        assert 0 <= int(move.id) < N and int(move.id) != cell(7, 7)
        assert agent.playouts >= agent.chunk and agent.playouts % agent.chunk == 0 and agent.playouts <= agent.max_playouts
    finally:
        agent.close()
        agent.network.fused.close()
    with pytest.raises(ValueError):
        make_agent("network", quiet=True)
    with pytest.raises(ValueError):
        make_agent("network:%s" % (tmp_path / "w.pt"), quiet=True, symmetry="mean")
