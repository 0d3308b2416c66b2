"""The board sets of tests/test_eval_compound_quads_gpu.py hold what they claim, by the oracle's load counts (oracle.scratch_load), on the CPU.

Phase 3b of K1 takes sixteen (candidate cell, colour) pairs per round, pair v = 2 * candidate + colour.  2 * n_cand is even, so a round's end
(a multiple of sixteen) never falls between the two colours of a candidate, and the pair counts next to a round's end are 14, 16, 18 and
30, 32, 34: boards with 7, 8, 9 and 15, 16, 17 candidate cells.  The set has every count from 1 to 20.

A candidate whose colour's density count is below two does not exist (tests/test_eval_density_gate.py), so no board can make phase 3b's
former density gate fail; what is left of that case are candidates in the board's first and last three rows, whose neighbourhood is cut
by the edge, and those are here."""
import os

import numpy as np

import eval_compound_quads_boards as B

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_compound_quads.npz")


def load_fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_has_every_candidate_count_and_colour_mix(oracle):
    F = oracle.LOAD_FIELDS
    fx = load_fixture()
    moves, lens = fx["moves"], fx["lens"]
    assert moves.shape == (len(lens), B.STRIDE) and moves.dtype == np.uint8 and os.path.getsize(FIXTURE) < 64 * 1024
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    assert legal.all() and (end_ply < 0).all(), "legal positions of unfinished games"
    load = oracle.scratch_load(moves, lens)
    np.testing.assert_array_equal(load[:, F.index("candidates")], fx["candidates"])
    assert (load[:, F.index("fives")] == 0).all()
    mixed = fx["mode"] == "mixed"
    print("candidate counts: white only %s, black only %s, mixed %s" % (fx["candidates"][fx["mode"] == "white"].tolist(),
                                                                       fx["candidates"][fx["mode"] == "black"].tolist(), fx["candidates"][mixed].tolist()))
    assert sorted(fx["candidates"][mixed].tolist()) == list(range(1, 21)), "every count from 1 to 20, the round boundaries 7 8 9 and 15 16 17 among them"
    for mode in ("white", "black"):
        assert (fx["mode"] == mode).sum() >= 3
    # one colour only: the other colour's stones are fillers, five or more cells from each other: it has no pattern, hence no counters and no flag
    totals = oracle.scratch_batch(moves, lens)[2]
    for i in np.nonzero(~mixed)[0]:
        other = totals[i, :8] & 0xFFFF if fx["mode"][i] == "black" else totals[i, :8] >> 16           # (totals: white in the low, black in the high half word)
        assert not other[3:6].any(), "board %d (%s only): the other colour has a LiveTwo, DeadThree or LiveThree" % (i, fx["mode"][i])
        own = totals[i, :8] >> 16 if fx["mode"][i] == "black" else totals[i, :8] & 0xFFFF
        assert own[3:6].any()
    # both colours on ONE cell: a (cell, colour) pair makes at most one compound, so more compounds than candidate cells means a cell with both flags
    both = load[:, F.index("compounds")] > load[:, F.index("candidates")]
    print("%d boards have more compounds than candidate cells" % int(both.sum()))
    assert both[mixed].sum() >= 3


def test_edge_rows_and_direction_pairs_hold_compounds(oracle):
    F = oracle.LOAD_FIELDS
    edge = B.edge_row_boards()
    load = oracle.scratch_load(*B.pack(edge))
    with_compound = load[:, F.index("compounds")] > 0
    print("edge rows: %d boards, %d with a compound, %d with two" % (len(edge), int(with_compound.sum()), int((load[:, F.index("compounds")] > 1).sum())))
    assert with_compound.sum() >= 40 and (load[:, F.index("compounds")] > 1).sum() >= 2 and (load[:, F.index("fives")] == 0).all()
    order = B.direction_order_boards()
    load = oracle.scratch_load(*B.pack(order))
    print("direction pairs: %d boards, queued components per board %s" % (len(order), np.bincount(load[:, F.index("queued")]).tolist()))
    assert len(order) >= 40 and (load[:, F.index("candidates")] == 1).all() and (load[:, F.index("queued")] == 1).all()


def test_saturated_positions_reach_the_flush_level():
    """phase 4 runs early once more than 192 rescan entries (96 compounds of two components) are queued: tests/golden/k1_saturated.npz has such positions"""
    with np.load(os.path.join(os.path.dirname(FIXTURE), "k1_saturated.npz")) as f:
        queued = f["load"][:, list(f["fields"]).index("queued")]
    print("%d of %d saturated positions queue more than 96 compounds, the most %d" % (int((queued > 96).sum()), len(queued), int(queued.max())))
    assert (queued > 96).sum() >= 8
