"""K1's scan at the ends of its lines and at the seam between a lane's two lines.  A lane walks its one or two lines as one symbol stream
without leading pads, `cellsA ? ? cellsB ? ? ...` (eval_kernel.hip, phase 1): a match that begins on a line's first cell is the first thing
the automaton sees after its start state or after the two pads of the line before, a match that ends on a line's last cell is reported on
the pads behind it, and where a lane carries two lines the late reports of the first and the early cells of the second lie two symbols apart.

Boards, generated here from a seed (legal positions: black on the even plies, a five completed by the last ply):
  edges  every one of the 72 lines of five or more cells carries, in turn, each form -- five, four, split four, three, two -- from its first
         cell on and up to its last cell, the colours alternating from board to board (72 x 2 x 5 boards);
  seams  the eight lanes with two lines -- the 8- and 7-cell diagonals with the 5- and 6-cell diagonals of the corners behind them -- with a
         form up to the last cell of the first line AND a form from the first cell of the second, every pair of colours.
The lines and the lanes are restated from lane_tables (eval_kernel.hip): rows, columns, diagonals, anti-diagonals, sorted by length, the
longest first; lane l < 64 walks line l, and line 64 + k rides behind lane 63 - k.

Against oracle.scratch_batch: scores, density, totals and the WHOLE status word, every board, in launches of 1 board, of 17 and of all.
Integer outputs: exact."""
import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

NAMES = ("scores", "density", "totals", "status")
STRIDE = 64
FORMS = {"five": (0, 1, 2, 3, 4), "four": (0, 1, 2, 3), "split four": (0, 2, 3, 4), "three": (0, 1, 2), "two": (0, 1)}   # cells from the line's end inwards
BLACK, WHITE = 0, 1


def lines_and_lanes():
    """-> (lines: list of cell lists, pairs: [(first line, second line)] of the lanes that walk two)"""
    lines = [[15 * y + x for x in range(15)] for y in range(15)] + [[15 * y + x for y in range(15)] for x in range(15)]
    for d in range(-10, 11):
        x0, y0 = (d, 0) if d > 0 else (0, -d)
        lines.append([15 * (y0 + i) + x0 + i for i in range(15 - abs(d))])
    for k in range(4, 25):
        x0 = min(k, 14)
        y0 = k - x0
        lines.append([15 * (y0 + i) + x0 - i for i in range(min(k, 28 - k) + 1)])
    lines.sort(key=lambda l: -len(l))                                       # (stable, like the host's sort)
    assert len(lines) == 72 and [len(l) for l in lines[56:]] == [8] * 4 + [7] * 4 + [6] * 4 + [5] * 4
    pairs = [(lines[63 - k], lines[64 + k]) for k in range(8)]
    assert sorted(len(a) + len(b) for a, b in pairs) == [13] * 8          # 8 + 5 and 7 + 6 cells: with two pads each, seventeen symbols
    return lines, pairs


def build_boards():
    rng = np.random.default_rng(1117)
    lines, pairs = lines_and_lanes()
    boards = []                                                             # (black cells, white cells, kind, key)

    def finish(stones, keep_off, five_colour, kind, key):
        """stones: {cell: colour}; balances the colours with stones off the lines at hand, adds three more of each, orders the plies"""
        side = [[c for c, col in stones.items() if col == BLACK], [c for c, col in stones.items() if col == WHITE]]
        free = [c for c in rng.permutation(225).tolist() if c not in keep_off and c not in stones]
        ahead = 1 if five_colour == BLACK else 0 if five_colour == WHITE else int(rng.integers(0, 2))      # black's lead behind the last ply
        while len(side[BLACK]) - len(side[WHITE]) != ahead:
            side[BLACK if len(side[BLACK]) - len(side[WHITE]) < ahead else WHITE].insert(0, free.pop())
        for _ in range(3):
            side[BLACK].insert(0, free.pop())
            side[WHITE].insert(0, free.pop())
        boards.append((side[BLACK], side[WHITE], kind, key))                # (a form's cells stay last in their list: a five is completed by the last ply)

    for li, line in enumerate(lines):
        for end in (0, 1):
            cells = line if end == 0 else line[::-1]
            for fi, (name, form) in enumerate(FORMS.items()):
                colour = (li + end + fi) & 1
                finish({cells[i]: colour for i in form}, set(line), colour if name == "five" else None, "edge", (li, end))
    for pi, (first, second) in enumerate(pairs):
        for fa in ("five", "four", "three"):
            for fb in ("four", "three", "five"):
                if fa == fb == "five":
                    continue
                for ca in (BLACK, WHITE):
                    for cb in (BLACK, WHITE):
                        stones = {first[::-1][i]: ca for i in FORMS[fa]}
                        theirs = {second[i]: cb for i in FORMS[fb]}
                        if any(stones.get(c, col) != col for c, col in theirs.items()):
                            continue                                        # (the two lines cross in a cell both forms want)
                        # the five's stones last in their colour's list
                        merged = dict(list(theirs.items()) + list(stones.items())) if fa == "five" else dict(list(stones.items()) + list(theirs.items()))
                        finish(merged, set(first) | set(second), ca if fa == "five" else cb if fb == "five" else None, "seam", pi)
    moves = np.zeros((len(boards), STRIDE), np.uint8)
    lens = np.zeros(len(boards), np.int32)
    for i, (black, white, _, _) in enumerate(boards):
        assert len(black) - len(white) in (0, 1) and len(black) + len(white) <= STRIDE
        seq = [0] * (len(black) + len(white))
        seq[0::2] = black
        seq[1::2] = white
        moves[i, :len(seq)] = seq
        lens[i] = len(seq)
    return moves, lens, boards


@pytest.fixture(scope="module")
def edge_boards(oracle):
    moves, lens, boards = build_boards()
    # legal positions only: no stone twice, nothing played behind a five (a filler stone can complete one by chance: that board leaves, and
    # what has to stay covered is asserted)
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    ok = legal & ((end_ply < 0) | (end_ply == lens))
    print("boards: %d built, %d legal; %d end with a five" % (len(lens), int(ok.sum()), int((end_ply[ok] == lens[ok]).sum())))
    kept = [b for b, good in zip(boards, ok) if good]
    edges = {b[3] for b in kept if b[2] == "edge"}
    assert edges == {(li, end) for li in range(72) for end in (0, 1)}, "a line's end is left without a board"
    per_lane = [sum(1 for b in kept if b[2] == "seam" and b[3] == pi) for pi in range(8)]
    print("seam boards per two-line lane:", per_lane)
    assert min(per_lane) >= 16 and int(ok.sum()) >= 0.95 * len(ok)
    moves, lens = moves[ok], lens[ok]
    fives = int((end_ply[ok] == lens).sum())
    assert fives >= 100
    ref = oracle.scratch_batch(moves, lens)
    for a in ref:
        a.setflags(write=False)
    assert int(((ref[3] & 2) != 0).sum()) == 0                              # (no board of these asks for more than the kernel's queues hold)
    seam = np.array([b[2] == "seam" for b in kept])
    return G.moves_to_planes(moves, lens), ref, seam


def compare(ref, got, rows, what):
    for name, a, b in zip(NAMES, ref, got):
        a = a[rows]
        bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
        print("%s %s: %d of %d boards differ" % (what, name, len(bad), len(a)))
        assert len(bad) == 0, "%s: %s differs on %d of %d boards, first %d" % (what, name, len(bad), len(a), bad[0])


def test_all_boards_in_one_launch(edge_boards):
    planes, ref, _ = edge_boards
    got = G.eval_batch_host(planes)
    assert len(got[3]) == len(planes)
    compare(ref, got, slice(None), "all %d boards" % len(planes))


def test_launches_of_17_boards(edge_boards):
    """a group and a board: the second group is partial; every board of the set, launch after launch"""
    planes, ref, _ = edge_boards
    n = len(planes)
    got = [np.concatenate(parts) for parts in zip(*(G.eval_batch_host(planes[i:i + 17]) for i in range(0, n - 16, 17)))]
    done = (n // 17) * 17
    assert done >= n - 16
    compare(ref, got, slice(0, done), "launches of 17")
    last = G.eval_batch_host(planes[n - 17:])                               # (the set's tail, which the strides of 17 may leave out)
    compare(ref, last, slice(n - 17, n), "the last 17")


def test_launches_of_one_board(edge_boards):
    """one board, one wavefront at work: every seam board and every fourth edge board"""
    planes, ref, seam = edge_boards
    n = len(planes)
    rows = np.nonzero(seam | (np.arange(n) % 4 == 0))[0]
    got = [np.concatenate(parts) for parts in zip(*(G.eval_batch_host(planes[i:i + 1]) for i in rows))]
    compare(ref, got, rows, "launches of 1 (%d boards)" % len(rows))
