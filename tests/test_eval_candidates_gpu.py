"""K1's compound candidates (phase 3: which cells' LiveThree / DeadThree / LiveTwo counters, clipped to 2 and summed over the directions, reach
two; phase 3b reads which colour made a cell a candidate from the entry) against the oracle's from-scratch evaluator, on every small
arrangement of stones along one line and on crossing lines.  Integer outputs and the whole status word: exact, every board compared.

A position is a move list (black first, colours alternate).  Whatever a window leaves the two colours apart is made up by filler stones of
the colour that is short: more than three cells from every cell of the window, no two of them next to each other on any line."""
import itertools

import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

NAMES = ("scores", "density", "totals", "status")
STRIDE = 232
DIRS = ((1, 0), (0, 1), (1, 1), (-1, 1))          # the kernel's directions 0..3: row, column, diagonal (x - y fixed), anti-diagonal (x + y fixed)


def cell(x, y):
    assert 0 <= x < 15 and 0 <= y < 15, (x, y)
    return 15 * y + x


def position(black, white):
    black, white = list(black), list(white)
    assert len(set(black) | set(white)) == len(black) + len(white), "a cell is used twice"
    assert len(black) - len(white) in (0, 1), "black %d, white %d stones: not a position of alternating moves" % (len(black), len(white))
    moves = [0] * (len(black) + len(white))
    moves[0::2] = black
    moves[1::2] = white
    return moves


def pack(positions):
    moves = np.zeros((len(positions), STRIDE), dtype=np.uint8)
    lens = np.zeros(len(positions), dtype=np.int32)
    for i, p in enumerate(positions):
        moves[i, :len(p)] = p
        lens[i] = len(p)
    return moves, lens


def compare(ref, got, what):
    for name, a, b in zip(NAMES, ref, got):
        bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
        print("%s %s: %d of %d boards differ" % (what, name, len(bad), len(a)))
        assert len(bad) == 0, "%s: %s differs on %d boards, first %d" % (what, name, len(bad), bad[0])


FILLINGS = [f for f in itertools.product((0, 1, -1), repeat=9) if sum(v != 0 for v in f) <= 5]      # 0 empty, 1 black, -1 white


def fillers_for(window):
    """Five cells for filler stones: more than three cells (in x or in y) from every cell of the window, and as far from each other as
    the board allows: at least three cells apart, so that two fillers are neither next to each other nor one blank apart on a line (X_X would be
    a pattern of the fillers' own)."""
    far = [(x, y) for y in range(15) for x in range(15) if all(max(abs(x - wx), abs(y - wy)) > 3 for (wx, wy) in window)]
    for apart in (5, 4, 3):
        out = []
        for p in far:
            if all(max(abs(p[0] - o[0]), abs(p[1] - o[1])) >= apart for o in out):
                out.append(p)
        if len(out) >= 5:
            # spread over the choice, not its first five: the colours' fillers come from both ends of the board where there are two
            return [cell(*p) for p in out[::max(1, len(out) // 5)][:5]]
    raise AssertionError("no room for five filler stones around %s" % (window,))


def window_positions(window):
    """Every filling of the window's nine cells with at most five stones (6 883 positions), made legal by filler stones."""
    assert len(FILLINGS) == 6883
    cells = [cell(x, y) for (x, y) in window]
    spare = fillers_for(window)
    out = []
    for f in FILLINGS:
        black = [c for c, v in zip(cells, f) if v > 0]
        white = [c for c, v in zip(cells, f) if v < 0]
        if len(black) > len(white):
            white += spare[:len(black) - len(white) - 1]
        else:
            black += spare[:len(white) - len(black)]
        out.append(position(black, white))
    return out


def line_window(d, centre):
    dx, dy = DIRS[d]
    return [(centre[0] + k * dx, centre[1] + k * dy) for k in range(-4, 5)]


def check(oracle, positions, what):
    moves, lens = pack(positions)
    ref = oracle.scratch_batch(moves, lens)
    compare(ref, G.eval_batch_host(G.moves_to_planes(moves, lens)), what)
    return ref


@pytest.mark.parametrize("centre", [(7, 7), (7, 14), (10, 14)], ids=["centre", "row14", "row14-cell224"])
def test_every_filling_of_a_row_window(oracle, centre):
    """Nine consecutive cells of a row: at the board's centre, and on row 14 -- the cells of the kernel's fourth pass over the board -- once
    in the middle of the row and once ending in cell 224."""
    positions = window_positions(line_window(0, centre))
    moves, lens = pack(positions)
    load = oracle.scratch_load(moves, lens)
    print("%s: %d positions, %d with a candidate, %d with a compound" % (centre, len(positions), int((load[:, oracle.LOAD_FIELDS.index("candidates")] > 0).sum()),
                                                                     int((load[:, oracle.LOAD_FIELDS.index("compounds")] > 0).sum())))
    assert (load[:, oracle.LOAD_FIELDS.index("candidates")] > 0).sum() >= 100, "the windows are meant to hold candidates"
    check(oracle, positions, "row window at %s" % (centre,))


@pytest.mark.parametrize("d, centre", [(1, (7, 7)), (1, (14, 10)), (2, (7, 7)), (2, (10, 10)), (3, (7, 7)), (3, (4, 10))],
                         ids=["column", "column14-cell224", "diagonal", "diagonal-cell224", "anti-diagonal", "anti-diagonal-corner"])
def test_candidate_fillings_of_the_other_directions(oracle, d, centre):
    """The same windows along a column, a diagonal and an anti-diagonal (the counters of directions 1..3: the other nibbles of a colour's
    half word), at the centre and ending on the board's last row; only the fillings on which the oracle finds a candidate."""
    positions = window_positions(line_window(d, centre))
    moves, lens = pack(positions)
    with_candidate = np.nonzero(oracle.scratch_load(moves, lens)[:, oracle.LOAD_FIELDS.index("candidates")] > 0)[0]
    print("direction %d at %s: %d of %d positions hold a candidate" % (d, centre, len(with_candidate), len(positions)))
    assert len(with_candidate) >= 100
    check(oracle, [positions[i] for i in with_candidate], "direction %d window at %s" % (d, centre))


def compound_positions():
    """Two open twos of one colour that cross in an empty cell q: a compound of two components (a double two): one counter in each of two
    direction nibbles of the colour's half word.  q x every pair of directions x both colours, at the board's centre, and with one component
    on the longest diagonal / anti-diagonal and on the shortest ones that can hold an open two (the constructions of test_eval_frame_gpu.py)."""
    out = []

    def cross(q, d1, d2, colour, s1=1, s2=1):
        (qx, qy), own = q, []
        for (dx, dy), s in ((DIRS[d1], s1), (DIRS[d2], s2)):
            own += [cell(qx + s * k * dx, qy + s * k * dy) for k in (1, 2)]
        used = set(own) | {cell(qx, qy)}
        spare = [c for c in (cell(x, y) for y in (0, 14) for x in range(0, 15, 2)) if c not in used and all(abs(c % 15 - u % 15) > 3 or abs(c // 15 - u // 15) > 3 for u in used)]
        other = spare[:4]
        assert len(other) == 4, "no room for the other colour's stones"
        return position(own, other) if colour > 0 else position(other + [spare[4]], own)

    for colour in (1, -1):
        for d1 in range(4):
            for d2 in range(d1 + 1, 4):
                out.append(cross((7, 7), d1, d2, colour))
        out.append(cross((6, 6), 2, 0, colour))
        out.append(cross((6, 6), 2, 1, colour))
        out.append(cross((6, 8), 3, 0, colour))
        out.append(cross((8, 6), 3, 1, colour, s1=-1))
        out.append(cross((10, 2), 2, 1, colour))
        out.append(cross((2, 10), 2, 0, colour))
        out.append(cross((4, 2), 3, 1, colour))
        out.append(cross((12, 10), 3, 0, colour, s2=-1))
    return out


def test_crossing_twos_in_every_pair_of_directions(oracle):
    positions = compound_positions()
    ref = check(oracle, positions, "crossing twos")
    compounds = (ref[2][:, 8:11] != 0).any(axis=1)
    assert compounds.all(), "positions %s hold no compound by the oracle: the construction is wrong" % np.nonzero(~compounds)[0].tolist()
