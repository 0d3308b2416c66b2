"""K21 on the device: K7's search under gmk_az_set_gumbel, gmk_az_root_choice_gumbel and gmk_az_advance_gumbel against tests/az_gumbel_reference.py,
bit for bit -- the root and its children's visits, values and priors, the tree size and status after every search (the moves on kept subtrees bring
the levels below the root up to where they are compared), the chosen cell and the improved-policy row.  The network is a host function of the
batch, the one the reference calls, so nothing but the search is compared."""
import functools

import numpy as np
import pytest

import az_gumbel_reference as AR
import az_leaves_reference as R
from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

N = 225
SEED, FIRST_ID = 0x5EED0123456789AB, 1000
GAMES = R.OPENINGS + [R.WON, R.OPEN_FOUR]
EVALUATORS = {"surrogate": R.surrogate, "sharpened": R.sharpened, "uniform": R.uniform}


def _roots(openings):
    moves, lens = np.zeros((len(openings), N), np.uint8), np.array([len(p) for p in openings], np.int32)
    last = np.full((len(openings), 2), -1, np.int16)
    for g, p in enumerate(openings):
        moves[g, :len(p)] = p
        last[g, :min(2, len(p))] = p[::-1][:2]
    return G.moves_to_planes(moves, lens), last


def _host_network(evaluator):
    import torch

    def network(states):
        s = states.cpu().numpy()
        vp = [evaluator(s[r]) for r in range(s.shape[0])]
        return (torch.tensor([float(v) for v, _ in vp], dtype=torch.float32, device="cuda"), torch.from_numpy(np.stack([p for _, p in vp])).cuda())
    return network


def _tree(openings, m, n, node_capacity=1 << 14, **kw):
    G.init()
    tree = G.AlphaZeroMCTS(len(openings), node_capacity=node_capacity, c_puct=5.0, gumbel=(m, n, 50.0, 1.0, SEED, FIRST_ID), **kw)
    tree.set_roots(*_roots(openings))
    return tree


def _refs(openings, evaluator, m, n, node_capacity=1 << 14, **kw):
    return [AR.GumbelSearch(moves, EVALUATORS[evaluator], m, n, FIRST_ID + g, SEED, c_puct=5.0, node_capacity=node_capacity, **kw) for g, moves in enumerate(openings)]


def _same(st, refs, where=""):
    for g, ref in enumerate(refs):
        rs, at = ref.root_stats(), "%s game %d" % (where, g)
        np.testing.assert_array_equal(st["visits"][g], rs["visits"], at)
        np.testing.assert_array_equal(st["values"][g].view(np.uint32), rs["values"].view(np.uint32), at)
        np.testing.assert_array_equal(st["priors"][g].view(np.uint32), rs["priors"].view(np.uint32), at)
        assert st["root_visits"][g] == rs["root_visits"] and st["n_nodes"][g] == rs["n_nodes"] and st["status"][g] == rs["status"], at
        assert np.float32(st["root_value"][g]).view(np.uint32) == np.float32(rs["root_value"]).view(np.uint32), at


def _choice(tree):
    import torch
    cells = torch.full((tree.n,), -7, dtype=torch.int16, device="cuda")
    rows = torch.full((tree.n, N), 12345, dtype=torch.int16, device="cuda")
    tree.root_choice(cells, rows, gumbel=True)
    torch.cuda.synchronize()
    return cells.cpu().numpy(), rows.cpu().numpy().view(np.uint16)


def _same_choice(tree, refs, where=""):
    cells, rows = _choice(tree)
    for g, ref in enumerate(refs):
        move, row = ref.choice()
        assert cells[g] == move, "%s game %d" % (where, g)
        np.testing.assert_array_equal(rows[g], row, "%s game %d" % (where, g))
    return cells


@functools.lru_cache(maxsize=None)
def _three_moves(evaluator, m, n):
    """The reference's side of test_three_moves_on_kept_subtrees: per move (statistics after the search, move, row)"""
    refs = _refs(GAMES, evaluator, m, n)
    out = []
    for _ in range(3):
        for ref in refs:
            ref.search(n)
        stats = [ref.root_stats() for ref in refs]
        choices = [ref.choice() for ref in refs]
        for ref, (move, _) in zip(refs, choices):
            if move >= 0:
                ref.reroot(move)
        out.append((stats, choices))
    return out


@pytest.mark.parametrize("evaluator", ["surrogate", "sharpened"])
@pytest.mark.parametrize("m,n", [(4, 16), (16, 32), (225, 8)])
def test_three_moves_on_kept_subtrees(evaluator, m, n):
    want = _three_moves(evaluator, m, n)
    tree = _tree(GAMES, m, n)
    network = _host_network(EVALUATORS[evaluator])
    for ply, (stats, choices) in enumerate(want):
        tree.search(network, n)
        st = tree.root_stats()
        for g, rs in enumerate(stats):
            at = "move %d game %d" % (ply, g)
            np.testing.assert_array_equal(st["visits"][g], rs["visits"], at)
            np.testing.assert_array_equal(st["values"][g].view(np.uint32), rs["values"].view(np.uint32), at)
            np.testing.assert_array_equal(st["priors"][g].view(np.uint32), rs["priors"].view(np.uint32), at)
            assert st["root_visits"][g] == rs["root_visits"] and st["n_nodes"][g] == rs["n_nodes"] and st["status"][g] == rs["status"], at
            assert np.float32(st["root_value"][g]).view(np.uint32) == np.float32(rs["root_value"]).view(np.uint32), at
        cells, rows = _choice(tree)
        for g, (move, row) in enumerate(choices):
            assert cells[g] == move, "move %d game %d" % (ply, g)
            np.testing.assert_array_equal(rows[g], row, "move %d game %d" % (ply, g))
        assert cells[len(R.OPENINGS)] == -1 and not rows[len(R.OPENINGS)].any()          # WON: a root without children
        tree.step(cells)                                         # the subtrees are kept; the won root has nothing to play
    tree.close()


def test_more_playouts_than_scheduled_then_a_fresh_root():
    m, n = 4, 16
    refs = _refs(R.OPENINGS, "surrogate", m, n)
    tree = _tree(R.OPENINGS, m, n)
    network = _host_network(R.surrogate)
    tree.search(network, n + 8)
    for ref in refs:
        ref.search(n + 8)
    _same(tree.root_stats(), refs, "n + 8")
    cells = _same_choice(tree, refs, "n + 8")
    after = [list(p) + [int(c)] for p, c in zip(R.OPENINGS, cells)]
    tree.set_roots(*_roots(after))                               # a fresh root below the move
    fresh = _refs(after, "surrogate", m, n)
    tree.search(network, n)
    for ref in fresh:
        ref.search(n)
    _same(tree.root_stats(), fresh, "fresh")
    _same_choice(tree, fresh, "fresh")
    tree.close()


def test_set_roots_voids_the_set_up():
    """Other positions with the same stone counts (the openings turned by 180 degrees): a set-up that survived gmk_az_set_roots would steer them"""
    m, n = 4, 16
    turned = [[224 - c for c in p] for p in R.OPENINGS]
    tree = _tree(R.OPENINGS, m, n)
    network = _host_network(R.sharpened)
    tree.search(network, n)
    tree.set_roots(*_roots(turned))
    refs = _refs(turned, "sharpened", m, n)
    tree.search(network, n)
    for ref in refs:
        ref.search(n)
    assert all(ref.setups == 1 for ref in refs)
    _same(tree.root_stats(), refs)
    _same_choice(tree, refs)
    tree.close()


def test_a_full_arena_drops_playouts():
    m, n = 16, 32
    refs = _refs(R.OPENINGS, "surrogate", m, n, node_capacity=256)
    tree = _tree(R.OPENINGS, m, n, node_capacity=256)
    tree.search(_host_network(R.surrogate), n)
    for ref in refs:
        ref.search(n)
    st = tree.root_stats()
    assert any(ref.status & R.STATUS_ARENA_FULL for ref in refs)  # the case is there: the reference dropped playouts
    _same(st, refs)
    _same_choice(tree, refs)
    tree.close()


def test_the_solver_at_the_leaves_composes():
    m, n = 4, 16
    refs = _refs([R.OPEN_FOUR], "uniform", m, n, vcf_depth=8, vcf_budget=64)
    tree = _tree([R.OPEN_FOUR], m, n, vcf_depth=8, vcf_budget=64)
    tree.search(_host_network(R.uniform), n)
    refs[0].search(n)
    assert refs[0].wins > 0
    _same(tree.root_stats(), refs)
    _same_choice(tree, refs)
    tree.close()


def test_advance_gumbel_writes_the_move_and_the_row():
    import torch
    m, n = 16, 32
    refs = _refs(R.OPENINGS, "sharpened", m, n)
    tree = _tree(R.OPENINGS, m, n)
    games = len(R.OPENINGS)
    moves, lens = torch.zeros((games, N), dtype=torch.uint8, device="cuda"), torch.tensor([len(p) for p in R.OPENINGS], dtype=torch.int32, device="cuda")
    for g, p in enumerate(R.OPENINGS):
        moves[g, :len(p)] = torch.tensor(p, dtype=torch.uint8)
    rows = torch.zeros((games, N, N), dtype=torch.int16, device="cuda")
    winner = torch.zeros(games, dtype=torch.int8, device="cuda")
    network = _host_network(R.sharpened)
    for ply in range(2):
        tree.search(network, n)
        assert tree.advance(moves, rows, lens, winner, reuse_subtree=True, gumbel=True) == games
        for g, ref in enumerate(refs):
            ref.search(n)
            move, row = ref.choice()
            at = len(R.OPENINGS[g]) + ply
            assert int(moves[g, at]) == move and int(lens[g]) == at + 1
            np.testing.assert_array_equal(rows[g, at].cpu().numpy().view(np.uint16), row)
            ref.reroot(move)
    tree.close()


def test_off_after_on_is_the_handle_that_never_was_on():
    network = _host_network(R.surrogate)
    stats = []
    for on in (True, False):
        G.init()
        tree = G.AlphaZeroMCTS(len(R.OPENINGS), node_capacity=1 << 14, c_puct=5.0)
        if on:
            tree.set_gumbel(4, 16, 50.0, 1.0, SEED, FIRST_ID)
            tree.set_roots(*_roots(R.OPENINGS))
            tree.search(network, 5)
            tree.set_gumbel(0)
        tree.set_roots(*_roots(R.OPENINGS))
        tree.search(network, 24)
        stats.append(tree.root_stats())
        tree.close()
    for k in stats[0]:
        assert (stats[0][k].view(np.uint32) == stats[1][k].view(np.uint32)).all(), k
    assert (stats[0]["root_visits"] == 24).all()


@pytest.fixture(scope="module")
def fused():
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    from helpers import PaddedNetwork
    G.init()
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=8).cuda().eval())
    yield PaddedNetwork(net, 6)                                  # the same shapes whatever the number of live games or slots
    net.close()


def _same_records(one, other):
    assert not one.overflow and not other.overflow
    assert (one.lens == other.lens).all() and (one.winner == other.winner).all() and int(one.lens.min()) >= 9
    for g in range(len(one)):
        n = int(one.lens[g])
        assert n == N or int(one.winner[g]) != 0
        assert (one.moves[g, :n] == other.moves[g, :n]).all() and (one.visits[g, :n] == other.visits[g, :n]).all()


@pytest.mark.parametrize("reuse", [True, False], ids=["kept", "fresh"])
def test_one_set_of_games_on_every_loop(fused, reuse):
    """Six whole games at eight playouts a move: all at once and through two slots, on the device loop and on the host-driven one.  With kept
    subtrees the host-driven loop has no slots (K7 cannot re-root one slot alone), with fresh roots it has: each loop is held to the device loop of
    its kind.  Every row is an improved-policy row, and the games are not the games of the plain search."""
    from gomokuai_amd import selfplay
    kw = dict(opening_plies=2, first_game_id=70, seed=2, root_noise=None, reuse_subtree=reuse, gumbel=(4, 50.0, 1.0))
    full = selfplay.play_network_games(6, fused, 8, **kw).cpu()
    others = [selfplay.play_network_games(6, fused, 8, slots=2, **kw).cpu(), selfplay.play_network_games(6, fused, 8, device_loop=False, **kw).cpu()]
    if not reuse:
        others.append(selfplay.play_network_games(6, fused, 8, slots=2, device_loop=False, **kw).cpu())
    for other in others:
        _same_records(full, other)
    rows = full.visits.numpy().view(np.uint16)
    for g in range(6):
        sums = rows[g, 2:int(full.lens[g])].astype(np.int64).sum(1)
        assert (np.abs(sums - 65535) <= 225).all(), g            # distributions, not visit counts (eight playouts would add up to eight)
    kw.pop("gumbel")
    plain = selfplay.play_network_games(6, fused, 8, **kw).cpu()
    assert any(int(plain.lens[g]) != int(full.lens[g]) or (plain.moves[g] != full.moves[g]).any() for g in range(6))


def test_the_entries_want_the_option():
    import torch
    tree = G.AlphaZeroMCTS(2, node_capacity=256)
    tree.set_roots(*_roots([[], [112]]))
    cells = torch.zeros(2, dtype=torch.int16, device="cuda")
    with pytest.raises(G.GmkError, match="off"):
        tree.root_choice(cells, gumbel=True)
    tree.close()
