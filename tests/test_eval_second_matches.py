"""Boards on which transitions report two matches (tests/golden/k1_second_matches.npz, chosen by tools/k1_second_matches_fixture.py), on the
CPU: the fixture holds every way a board's second matches can lie against K1's 64-lane deposit rounds, and no board the suite knows has more
MATCHES than the transition queue has room for entries (384).  K1 as it stands deposits a second match inline, by the lane of its transition,
so its queue counts transitions; the bound on matches is what a kernel that queues second matches as entries of their own would need (that form
was built in round 10, measured and dropped) and is kept as the margin it is.

With T emitting transitions and M matches on a board (oracle.scratch_load), 64 lanes a round:
  more      M > T
  new_round ceil(M / 64) > ceil(T / 64): the second matches would open a round of their own
  lane0     T % 64 == 0 and M > T: the rounds are full and a second match would be lane 0 of a new one
  crowded   M - T > ceil(T / 64): two or more second matches come from one round (pigeonhole)
  none      M == T
  heaviest  the boards of k1_saturated.npz with the most matches"""
import os

import numpy as np

from gomokuai_amd import lib as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "k1_second_matches.npz")
QUEUE_ROOM = 384                   # kQueueCap - 64 of eval_kernel.hip: queue entries below the copies of the totals


def load_fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def counts(oracle, load):
    F = oracle.LOAD_FIELDS
    return load[:, F.index("transitions")].astype(np.int64), load[:, F.index("matches")].astype(np.int64)


def test_fixture_is_as_recorded_and_holds_every_case(oracle):
    fx = load_fixture()
    moves, lens, load = fx["moves"], fx["lens"], fx["load"]
    n = len(lens)
    assert 0 < n <= 400 and moves.shape == (n, 232) and moves.dtype == np.uint8 and lens.dtype == np.int32
    assert os.path.getsize(FIXTURE) < 256 * 1024
    assert tuple(fx["fields"]) == oracle.LOAD_FIELDS
    for i in range(n):
        played = moves[i, :lens[i]]
        assert played.max() < 225 and len(set(played.tolist())) == lens[i] and not moves[i, lens[i]:].any(), i
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    assert legal.all() and ((end_ply < 0) | (end_ply == lens)).all()
    np.testing.assert_array_equal(oracle.scratch_load(moves, lens), load)
    t, m = counts(oracle, load)
    rounds = lambda v: (v + 63) // 64
    cases = {"more": m > t, "new_round": rounds(m) > rounds(t), "lane0": (t % 64 == 0) & (t > 0) & (m > t), "crowded": m - t > rounds(t),
             "none": (m == t) & (t > 0), "heaviest": fx["heaviest"]}
    for name, mask in cases.items():
        print("%-10s %d boards" % (name, int(mask.sum())))
    assert cases["more"].sum() >= 100
    for name in ("new_round", "lane0", "crowded", "none", "heaviest"):
        assert cases[name].sum() >= 4, name
    # the heaviest boards are the heaviest of the saturated set
    with np.load(os.path.join(GOLDEN, "k1_saturated.npz")) as f:
        sat_matches = np.sort(f["load"][:, oracle.LOAD_FIELDS.index("matches")])[::-1]
    k = int(cases["heaviest"].sum())
    assert sorted(m[cases["heaviest"]].tolist(), reverse=True) == sat_matches[:k].tolist()


def test_no_known_board_has_more_matches_than_the_queue_holds(oracle):
    """No more than 384 matches on a board of the fixture, of 6 000 boards of each synthetic kind or of the saturated set."""
    worst = {}
    worst["fixture"] = int(counts(oracle, load_fixture()["load"])[1].max())
    for kind in (0, 1):
        moves, lens, _ = G.synth_boards(6000, kind, first_board=100000)
        worst["synthetic kind %d" % kind] = int(counts(oracle, oracle.scratch_load(moves, lens))[1].max())
    with np.load(os.path.join(GOLDEN, "k1_saturated.npz")) as f:
        worst["k1_saturated"] = int(counts(oracle, oracle.scratch_load(f["moves"], f["lens"]))[1].max())
    print("most matches on a board:", worst)
    for name, v in worst.items():
        assert v <= QUEUE_ROOM, "%s: a board with %d matches" % (name, v)
