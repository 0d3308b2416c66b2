"""K1's scan takes a lane's first four symbols with one read of a prefix table and queues nothing for them; its first ordinary lookup is the
fifth symbol (eval_kernel.hip, phase 1).  Here every line's first five cells -- the four the prefix swallows and the first one behind it --
carry every filling there is.

Boards, generated from a seed (legal positions: black on the even plies): for each of the 72 lines of five or more cells, all 243 fillings
{empty, black, white} of its first five cells; the colours are balanced and three stones per colour are added, all off the line; a filling
of five equal stones is a five, ordered so that the last ply completes it.  17 496 boards, none left out: the fixture asserts that all are
legal, that every (line, filling) class is there, that 144 end with a five and that none asks for more than the kernel's queues hold.
The lines are restated from lane_tables (eval_kernel.hip): rows, columns, diagonals, anti-diagonals, from the cell the lane's stream starts at.

Against oracle.scratch_batch: scores, density, totals and the WHOLE status word, every board in one launch; the five boards and every
50th other board again in launches of one.  Integer outputs: exact."""
import itertools

import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

NAMES = ("scores", "density", "totals", "status")
STRIDE = 32
BLACK, WHITE = 0, 1
EMPTY = 2


def lines_of_the_board():
    lines = [[15 * y + x for x in range(15)] for y in range(15)] + [[15 * y + x for y in range(15)] for x in range(15)]
    for d in range(-10, 11):
        x0, y0 = (d, 0) if d > 0 else (0, -d)
        lines.append([15 * (y0 + i) + x0 + i for i in range(15 - abs(d))])
    for k in range(4, 25):
        x0 = min(k, 14)
        y0 = k - x0
        lines.append([15 * (y0 + i) + x0 - i for i in range(min(k, 28 - k) + 1)])
    lines.sort(key=lambda l: -len(l))                                       # (stable, like the host's sort)
    assert len(lines) == 72 and min(len(l) for l in lines) == 5
    return lines


def build_boards():
    rng = np.random.default_rng(1121)
    boards = []                                                             # (black cells, white cells, line, filling, is a five)
    for li, line in enumerate(lines_of_the_board()):
        for fi, filling in enumerate(itertools.product((EMPTY, BLACK, WHITE), repeat=5)):
            stones = {line[i]: col for i, col in enumerate(filling) if col != EMPTY}
            five = filling[0] != EMPTY and len(set(filling)) == 1
            side = [[c for c, col in stones.items() if col == BLACK], [c for c, col in stones.items() if col == WHITE]]
            free = [c for c in rng.permutation(225).tolist() if c not in line]
            ahead = (1 if filling[0] == BLACK else 0) if five else int(rng.integers(0, 2))      # black's lead behind the last ply
            while len(side[BLACK]) - len(side[WHITE]) != ahead:
                side[BLACK if len(side[BLACK]) - len(side[WHITE]) < ahead else WHITE].insert(0, free.pop())
            for _ in range(3):
                side[BLACK].insert(0, free.pop())
                side[WHITE].insert(0, free.pop())
            boards.append((side[BLACK], side[WHITE], li, fi, five))         # (the line's stones stay last in their list: a five is completed by the last ply)
    moves = np.zeros((len(boards), STRIDE), np.uint8)
    lens = np.zeros(len(boards), np.int32)
    for i, (black, white, _, _, _) in enumerate(boards):
        assert len(black) - len(white) in (0, 1) and len(black) + len(white) <= STRIDE
        seq = [0] * (len(black) + len(white))
        seq[0::2] = black
        seq[1::2] = white
        moves[i, :len(seq)] = seq
        lens[i] = len(seq)
    return moves, lens, boards


@pytest.fixture(scope="module")
def prefix_boards(oracle):
    moves, lens, boards = build_boards()
    assert len(boards) == 72 * 243 == 17496
    assert {(b[2], b[3]) for b in boards} == {(li, fi) for li in range(72) for fi in range(243)}
    # legal positions, all of them: no stone twice, nothing played behind a five, and a five only where the filling is one
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    ok = legal & ((end_ply < 0) | (end_ply == lens))
    is_five = np.array([b[4] for b in boards])
    ends = end_ply == lens
    print("boards: %d built, %d legal; %d end with a five, %d fillings are fives" % (len(lens), int(ok.sum()), int(ends.sum()), int(is_five.sum())))
    assert ok.all(), "board %d (line %d, filling %d) is not a legal position" % ((int(np.nonzero(~ok)[0][0]),) + boards[int(np.nonzero(~ok)[0][0])][2:4])
    assert int(is_five.sum()) == 144 and (ends == is_five).all()
    ref = oracle.scratch_batch(moves, lens)
    for a in ref:
        a.setflags(write=False)
    assert int(((ref[3] & 2) != 0).sum()) == 0                              # (no board of these asks for more than the kernel's queues hold)
    return G.moves_to_planes(moves, lens), ref, is_five


def compare(ref, got, rows, what):
    for name, a, b in zip(NAMES, ref, got):
        a = a[rows]
        bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
        print("%s %s: %d of %d boards differ" % (what, name, len(bad), len(a)))
        assert len(bad) == 0, "%s: %s differs on %d of %d boards, first %d" % (what, name, len(bad), len(a), bad[0])


def test_all_boards_in_one_launch(prefix_boards):
    planes, ref, _ = prefix_boards
    got = G.eval_batch_host(planes)
    assert len(got[3]) == len(planes) == 17496
    compare(ref, got, slice(None), "all %d boards" % len(planes))


def test_launches_of_one_board(prefix_boards):
    """one board, one wavefront at work: the 144 five boards and every 50th of the others"""
    planes, ref, is_five = prefix_boards
    others = np.nonzero(~is_five)[0]
    rows = np.sort(np.concatenate([np.nonzero(is_five)[0], others[::50]]))
    assert len(rows) == 144 + (len(others) + 49) // 50
    got = [np.concatenate(parts) for parts in zip(*(G.eval_batch_host(planes[i:i + 1]) for i in rows))]
    compare(ref, got, rows, "launches of 1 (%d boards)" % len(rows))
