"""K1's counter-move rescans (eval_kernel.hip, phase 4) take the first four symbols of a lane's window with one read of the root's prefix
table (DeviceTables::dev_prefix4) and walk the remaining three or four; the window may hold '?' there, wherever the cell lies near an end of
its line.

Boards, generated from a seed: eight plies, black's four stones two pairs -- `q + 1, q + 2` or `q + 1, q + 3` steps from an empty cell q,
the same shape for both -- along two different directions that cross at q: a compound of two twos at q, whose counter-move cells phase 4
looks for.  Every cell q, the six pairs of directions, both signs of each direction, both shapes, wherever the stones lie on the board:
6 768 boards.  White's four stones lie more than five cells from q and more than two cells from each other (no pattern of their own, none
of black's touched).  The fixture asserts on the CPU, before anything runs on the GPU, that all boards are legal, that 4 320 of them queue a
rescan (oracle.scratch_load), and that among those q lies one to six cells from either end of its line in each of the four directions, 48
classes with at least 40 boards each: the windows whose leading or trailing symbols are '?'.

Against oracle.scratch_batch: scores, density, totals and the WHOLE status word, every board.  Integer outputs: exact."""
import itertools

import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

NAMES = ("scores", "density", "totals", "status")
DIRS = ((1, 0), (0, 1), (1, 1), (-1, 1))                                    # row, column, diagonal, anti-diagonal, as (dx, dy)
STRIDE = 8


def on_board(x, y):
    return 0 <= x < 15 and 0 <= y < 15


def to_line_ends(x, y, d):
    """cells between (x, y) and the two ends of its line along d: (towards -d, towards +d)"""
    back = fwd = 0
    while on_board(x - (back + 1) * d[0], y - (back + 1) * d[1]):
        back += 1
    while on_board(x + (fwd + 1) * d[0], y + (fwd + 1) * d[1]):
        fwd += 1
    return back, fwd


def build_boards():
    rng = np.random.default_rng(1123)
    boards = []                                                             # (black cells, white cells, q, (direction a, direction b))
    for qy, qx in itertools.product(range(15), repeat=2):
        for a, b in itertools.combinations(range(4), 2):
            for sa, sb, gap in itertools.product((1, -1), (1, -1), (2, 3)):
                black = [(qx + sa * k * DIRS[a][0], qy + sa * k * DIRS[a][1]) for k in (1, gap)] + [(qx + sb * k * DIRS[b][0], qy + sb * k * DIRS[b][1]) for k in (1, gap)]
                if not all(on_board(x, y) for x, y in black):
                    continue
                white = []
                for c in rng.permutation(225).tolist():
                    x, y = c % 15, c // 15
                    if max(abs(x - qx), abs(y - qy)) > 5 and all(max(abs(x - wx), abs(y - wy)) > 2 for wx, wy in white):
                        white.append((x, y))
                        if len(white) == 4:
                            break
                assert len(white) == 4
                boards.append(([15 * y + x for x, y in black], [15 * y + x for x, y in white], (qx, qy), (a, b)))
    moves = np.zeros((len(boards), STRIDE), np.uint8)
    for i, (black, white, _, _) in enumerate(boards):
        moves[i, 0::2] = black
        moves[i, 1::2] = white
    return moves, np.full(len(boards), STRIDE, np.int32), boards


@pytest.fixture(scope="module")
def rescan_boards(oracle):
    moves, lens, boards = build_boards()
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    queued = oracle.scratch_load(moves, lens)[:, oracle.LOAD_FIELDS.index("queued")] > 0
    print("boards: %d built, %d legal and unfinished, %d queue a rescan" % (len(boards), int((legal & (end_ply < 0)).sum()), int(queued.sum())))
    assert len(boards) == 6768 and (legal & (end_ply < 0)).all()
    assert int(queued.sum()) == 4320
    # q one to six cells from a line's end, per direction of the board's pair and per side: the windows that run off the line
    classes = {}
    for (_, _, (qx, qy), pair), rescans in zip(boards, queued):
        if not rescans:
            continue
        for d in pair:
            for side, dist in enumerate(to_line_ends(qx, qy, DIRS[d])):
                if 1 <= dist <= 6:
                    classes[(d, side, dist)] = classes.get((d, side, dist), 0) + 1
    print("boards with a rescan per (direction, side, cells to the line's end): least %d of %d classes" % (min(classes.values()), len(classes)))
    assert set(classes) == {(d, side, dist) for d in range(4) for side in (0, 1) for dist in range(1, 7)} and min(classes.values()) >= 40
    ref = oracle.scratch_batch(moves, lens)
    for a in ref:
        a.setflags(write=False)
    assert int(((ref[3] & 2) != 0).sum()) == 0                              # (no board of these asks for more than the kernel's queues hold)
    return G.moves_to_planes(moves, lens), ref


def test_every_board_against_the_oracle(rescan_boards):
    planes, ref = rescan_boards
    got = G.eval_batch_host(planes)
    assert len(got[3]) == len(planes) == 6768
    for name, a, b in zip(NAMES, ref, got):
        bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
        print("%s: %d of %d boards differ" % (name, len(bad), len(a)))
        assert len(bad) == 0, "%s differs on %d of %d boards, first %d" % (name, len(bad), len(a), bad[0])
