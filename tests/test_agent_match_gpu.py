"""selfplay.play_agent_match on the GPU: the device loop against the same match through the host for every kind of pairing, the plies of a
K7-against-K7 match against single searches of the mover's own configuration, a deterministic agent against itself, and the bookkeeping."""
import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd import rating, selfplay
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
from helpers import PaddedNetwork

pytestmark = pytest.mark.gpu

N = 225
ROWS = 16                     # every batch a network sees is padded to this many rows (helpers.PaddedNetwork): 3 games x 4 leaves fit


@pytest.fixture(scope="module")
def nets():
    fused = [FusedPolicyValueNetwork(PolicyValueNetwork(seed=s).cuda().eval()) for s in (0, 1)]
    yield [PaddedNetwork(f, ROWS) for f in fused]
    for f in fused:
        f.close()


def net(network, playouts=24, **kw):
    return ("network", dict(network=network, playouts=playouts, **kw))


TRAD = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 40})
RANDOM = ("random_mcts", {"c_puct": 5.0, "c_iterations": 40})


def _same_match(dev, host):
    (rd, bd, sd), (rh, bh, sh) = dev, host
    n = len(rd)
    cd, ch = rd.cpu(), rh.cpu()
    assert (bd == bh).all() and (bd == (np.arange(n) % 2 == 0)).all() and (sd == sh).all()
    assert (cd.lens == ch.lens).all() and (cd.winner == ch.winner).all() and rd.overflow == rh.overflow and not rd.overflow
    assert (cd.moves == ch.moves).all()
    for g in range(n):
        k = int(cd.lens[g])
        assert (cd.visits[g, :k] == ch.visits[g, :k]).all(), g
        assert int(cd.visits[g, k:].abs().sum()) == 0 and int(ch.visits[g, k:].abs().sum()) == 0 and int(cd.moves[g, k:].sum()) == 0
    for gd, gh in zip(rd.groups, rh.groups):
        assert gd["games"].tolist() == gh["games"].tolist() and gd["unfinished"] == gh["unfinished"]
        assert all(live is None or live == gd["unfinished"] for live in gd["live_games"])      # a K7 handle closed exactly the games that ended
    assert (sd == selfplay.evaluation_scores(cd.winner.numpy(), bd)).all()
    return cd


def _pairings(nets):
    a, b = nets
    short = dict(n_games=6, max_moves=12)
    return {
        "k7-k7-kept": (net(a), net(b, 12, leaves=4), dict(short, paired=True, opening_plies=2, reuse_subtree=True)),
        "k7-k7-fresh": (net(a), net(b, 12, leaves=4), dict(short, paired=True, opening_plies=2, reuse_subtree=False)),
        "proof-k7": (net(a, vcf=(8, 32), proof=True), net(b), dict(short, paired=True, opening_plies=3)),
        "gumbel-k7": (net(a, 16, gumbel=(8, 50.0, 1.0)), net(b), dict(short, paired=True, opening_plies=3)),
        "k7-k6": (net(a), TRAD, dict(short, paired=True, opening_plies=3)),
        "k3-k7": (RANDOM, net(a), dict(short, paired=True, opening_plies=3)),
        "k3-k6": (RANDOM, TRAD, dict(short, paired=True, opening_plies=3)),
        "k7-k3-whole": (net(a), RANDOM, dict(n_games=2, max_moves=N, paired=True, opening_plies=0)),
    }


@pytest.mark.parametrize("name", ["k7-k7-kept", "k7-k7-fresh", "proof-k7", "gumbel-k7", "k7-k6", "k3-k7", "k3-k6", "k7-k3-whole"])
def test_both_loops_play_the_same_match(nets, name):
    first, second, kw = _pairings(nets)[name]
    kw = dict(kw, seed=9, first_game_id=40)
    n_games = kw.pop("n_games")
    dev = selfplay.play_agent_match(n_games, first, second, device_loop=True, **kw)
    host = selfplay.play_agent_match(n_games, first, second, device_loop=False, **kw)
    rec = _same_match(dev, host)
    assert [len(g["games"]) for g in dev[0].groups] == [n_games // 2, n_games // 2]
    opening = kw["opening_plies"]
    if kw["max_moves"] < N:
        assert int(rec.lens.max()) <= opening + kw["max_moves"] and int(rec.lens.min()) >= min(9, opening + kw["max_moves"])
    else:                                                            # played to their end
        assert all(g["unfinished"] == 0 for g in dev[0].groups)
        assert all(int(rec.lens[g]) == N or int(rec.winner[g]) != 0 for g in range(n_games))
    for g in range(n_games):                                         # every searched ply left a row with weight
        assert all(int(rec.visits[g, i].to(torch.int32).abs().sum()) > 0 for i in range(opening, int(rec.lens[g])))


def _roots(lists):
    moves, lens = np.zeros((len(lists), N), np.uint8), np.array([len(p) for p in lists], np.int32)
    last = np.full((len(lists), 2), -1, np.int16)
    for g, p in enumerate(lists):
        moves[g, :len(p)] = p
        last[g, :min(2, len(p))] = p[::-1][:2]
    return G.moves_to_planes(moves, lens), last


def _single_searches(network, playouts, positions):
    """(move, visit row saturated) of a fresh AlphaZeroMCTS.search from each position"""
    out = []
    for at in range(0, len(positions), ROWS):
        chunk = positions[at:at + ROWS]
        az = G.AlphaZeroMCTS(len(chunk), node_capacity=playouts * N + 1)
        az.set_roots(*_roots(chunk))
        with torch.no_grad():
            az.search(network, playouts)
        v = az.root_stats()["visits"]
        az.close()
        out += [(int(v[k].argmax()), np.minimum(v[k], 65535).astype(np.uint16)) for k in range(len(chunk))]
    return out


def test_every_ply_is_the_movers_own_search(nets):
    """Fresh roots, no noise: every recorded ply -- move and visit row -- is what a fresh AlphaZeroMCTS.search gives from the position before it
    with the MOVER's network at the mover's budget; and the other side's configuration gives something else on some ply of the match,
    otherwise this could not tell the sides apart."""
    a, b = nets
    rec, black, _ = selfplay.play_agent_match(4, net(a, 24), net(b, 12), seed=3, first_game_id=5, opening_plies=2, paired=True, max_moves=10,
                                              reuse_subtree=False, root_noise=None, device_loop=True)
    rec = rec.cpu()
    moves, lens, visits = rec.moves.numpy(), rec.lens.numpy(), rec.visits.numpy().view(np.uint16)
    plies = [[], []]                                                 # of `first`, of `second`
    for g in range(4):
        for i in range(2, int(lens[g])):
            plies[0 if (i % 2 == 0) == bool(black[g]) else 1].append((g, i))
    assert len(plies[0]) >= 12 and len(plies[1]) >= 12
    told_apart = 0
    for side, (own, other) in enumerate((((a, 24), (b, 12)), ((b, 12), (a, 24)))):
        positions = [[int(x) for x in moves[g, :i]] for g, i in plies[side]]
        for (g, i), (move, row) in zip(plies[side], _single_searches(*own, positions)):
            assert move == moves[g, i] and (row == visits[g, i]).all(), (side, g, i)
        told_apart += sum(move != moves[g, i] or (row != visits[g, i]).any() for (g, i), (move, row) in zip(plies[side], _single_searches(*other, positions)))
    assert told_apart > 0


def test_a_deterministic_side_against_itself_scores_one_half(nets):
    """The same plain agent on both sides of paired openings, no noise: game 2p + 1 is game 2p again with the handles exchanged, so every pair
    scores exactly one point and the paired standard error is exactly 0."""
    spec = net(nets[0], 16)
    rec, black, scores = selfplay.play_agent_match(6, spec, spec, seed=12, first_game_id=20, opening_plies=4, paired=True, max_moves=N, root_noise=None)
    groups, rec = rec.groups, rec.cpu()
    assert all(g["unfinished"] == 0 for g in groups) and not rec.overflow
    for p in range(3):
        assert int(rec.lens[2 * p]) == int(rec.lens[2 * p + 1]) and (rec.moves[2 * p] == rec.moves[2 * p + 1]).all()
        assert (rec.visits[2 * p] == rec.visits[2 * p + 1]).all() and int(rec.winner[2 * p]) == int(rec.winner[2 * p + 1])
        assert scores[2 * p] + scores[2 * p + 1] == 1.0
    s = rating.summary(scores, paired=True)
    assert s["pairs"] == [0, 0, 3, 0, 0] and s["stderr"] == 0.0 and s["score"] == 0.5 and rating.sprt(scores, 0.0, 10.0)["llr"] == 0.0


@pytest.mark.parametrize("paired", [True, False])
def test_bookkeeping(nets, paired):
    n = 6 if paired else 5
    rec, black, scores = selfplay.play_agent_match(n, net(nets[0], 12), TRAD, seed=7, first_game_id=30, opening_plies=4, paired=paired, max_moves=8)
    groups, rec = rec.groups, rec.cpu()
    assert black.tolist() == (np.arange(n) % 2 == 0).tolist()
    own_moves, own_lens = selfplay._opening(n, 7, 30, 4)
    assert (own_lens == 4).all()
    for g in range(n):
        source = g - g % 2 if paired else g                           # a pair shares the opening of its even game
        assert rec.moves[g, :4].tolist() == own_moves[source, :4].tolist(), g
        assert int(rec.visits[g, :4].abs().sum()) == 0                # opening plies were not searched
    if paired:
        assert (rec.moves[0::2, :4] == rec.moves[1::2, :4]).all()
    assert (scores == selfplay.evaluation_scores(rec.winner.numpy(), black)).all()
    assert [g["games"].tolist() for g in groups] == [list(range(0, n, 2)), list(range(1, n, 2))]
    for g in groups:
        assert g["live_games"] == (g["unfinished"], None)             # the K7 handle's live games, and a handle that has no such count
        assert g["unfinished"] == int((rec.lens[g["games"]] == 12).sum() - ((rec.winner[g["games"]] != 0) & (rec.lens[g["games"]] == 12)).sum())
