"""K1's queue entries carry the place of the consumed symbol -- cell, direction, minus the stride -- kept as a running value by the scan lane, and
a lane's two lines lie in one direction (eval_kernel.hip, phases 1 and 2; the lane table is restated in tests/eval_place_reference.py and held
against the host's on the CPU by tests/test_eval_place_entries.py).  The boards on which a wrong place would show:

  one stone   the 225 boards with one stone: every cell on each of its lines, so a wrong first cell, direction or stride of any line;
  seams       the eight lanes with two lines -- an 8-cell (anti-)diagonal with the 5-cell one of the same direction behind it, 7 cells with 6 --
              with a form (five, four, three) up to the last cell of the first line AND a form from the first cell of the second, every pair of
              colours: the jump, and the late reports of the first line two symbols in front of the second;
  ends        forms ending on the last cell of the main diagonal, the main anti-diagonal, row 14 and column 14, both colours, and main-diagonal
              boards whose filling reports a match on step 16, the second trailing pad, "cell" 256: the place's ninth cell bit;
  heavy       the positions of tests/golden/k1_saturated.npz that queue more than 320 transitions (at most 44 of them): six deposit rounds, each
              reading the next round's entry ahead without a clamp.

Boards are legal positions (black on the even plies, a five completed by the last ply).  Against oracle.scratch_batch: scores, density, totals and
the WHOLE status word, every board, each set in launches of 1 board, of 17 and of all.  Integer outputs: exact."""
import itertools
import os

import numpy as np
import pytest

import eval_place_reference as R
from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_saturated.npz")
NAMES = ("scores", "density", "totals", "status")
STRIDE = 232                                                                # (the fixture's)
FORMS = {"five": (0, 1, 2, 3, 4), "four": (0, 1, 2, 3), "split four": (0, 2, 3, 4), "three": (0, 1, 2), "two": (0, 1)}   # cells from the line's end inwards
BLACK, WHITE = 0, 1
SETS = ("one stone", "seams", "ends", "heavy")


def has_five(tail):
    return any(len(set(tail[i:i + 5])) == 1 and tail[i] != 3 for i in range(len(tail) - 4))


def build_boards():
    """-> [(black cells, white cells, set, key)]"""
    rng = np.random.default_rng(1421)
    boards = []

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

    for pi, (_, (_, first), (_, second)) in enumerate(R.pairs()):
        for fa in ("five", "four", "three"):
            for fb in ("four", "three", "five"):
                if fa == fb == "five":
                    continue
                for ca in (BLACK, WHITE):
                    for cb in (BLACK, WHITE):
                        stones = {first[::-1][i]: ca for i in FORMS[fa]}
                        theirs = {second[i]: cb for i in FORMS[fb]}
                        # the five's stones last in their colour's list
                        merged = dict(list(theirs.items()) + list(stones.items())) if fa == "five" else dict(list(stones.items()) + list(theirs.items()))
                        finish(merged, set(first) | set(second), ca if fa == "five" else cb if fb == "five" else None, "seams", pi)
    ls = R.lines()
    main_diagonal, main_anti = ls[R.MAIN_DIAGONAL_LANE][1], ls[R.MAIN_DIAGONAL_LANE + 1][1]
    assert main_diagonal == [16 * i for i in range(15)] and main_anti == [14 + 14 * i for i in range(15)]
    for li, line in enumerate((main_diagonal, main_anti, [210 + x for x in range(15)], [15 * y + 14 for y in range(15)])):
        for fi, (name, form) in enumerate(FORMS.items()):
            for colour in (BLACK, WHITE):
                finish({line[::-1][i]: colour for i in form}, set(line), colour if name == "five" else None, "ends", (li, name, colour))
    # fillings of the main diagonal's last six cells (the rest blank) that report a match on the stream's last symbol, walked on the CPU
    trans, _, _ = G.tables_copy()
    late = [t for t in itertools.product((0, 1, 3), repeat=6) if not has_five(t) and R.reports_on_last_pad(trans, t)]
    assert len(late) > 0, "no filling of the main diagonal reports on step 16"
    for t in late[:8]:
        finish({main_diagonal[9 + i]: sym for i, sym in enumerate(t) if sym != 3}, set(main_diagonal), None, "ends", ("step 16", t))
    return boards, len(late)


def to_moves(boards):
    moves = np.zeros((len(boards), STRIDE), np.uint8)
    lens = np.zeros(len(boards), np.int32)
    for i, (black, white, _, _) in enumerate(boards):
        assert len(black) - len(white) in (0, 1) and len(black) + len(white) <= STRIDE
        seq = [0] * (len(black) + len(white))
        seq[0::2] = black
        seq[1::2] = white
        moves[i, :len(seq)] = seq
        lens[i] = len(seq)
    return moves, lens


@pytest.fixture(scope="module")
def place_boards(oracle):
    """-> (planes, reference, the set of every board)"""
    built, n_late = build_boards()
    moves, lens = to_moves(built)
    # legal positions only: nothing played behind a five (a filler stone can complete one by chance: that board leaves, and what has to stay
    # covered is asserted)
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    ok = legal & ((end_ply < 0) | (end_ply == lens))
    kept = [b for b, good in zip(built, ok) if good]
    per_lane = [sum(1 for b in kept if b[2] == "seams" and b[3] == pi) for pi in range(8)]
    print("built %d boards, %d legal; seam boards per two-line lane: %s; %d fillings report on step 16" % (len(ok), int(ok.sum()), per_lane, n_late))
    assert min(per_lane) >= 16 and int(ok.sum()) >= 0.95 * len(ok)
    assert {b[3][0] for b in kept if b[2] == "ends"} == {0, 1, 2, 3, "step 16"}, "a line's end is left without a board"
    parts = [(moves[ok], lens[ok], [b[2] for b in kept])]
    ones = np.zeros((225, STRIDE), np.uint8)
    ones[:, 0] = np.arange(225)
    parts.append((ones, np.ones(225, np.int32), ["one stone"] * 225))
    T = oracle.LOAD_FIELDS.index("transitions")
    with np.load(FIXTURE) as f:
        sat_moves, sat_lens = f["moves"], f["lens"]
    assert sat_moves.shape[1] == STRIDE
    heavy = np.nonzero(oracle.scratch_load(sat_moves, sat_lens)[:, T] > 320)[0][:44]
    assert len(heavy) > 0
    parts.append((sat_moves[heavy], sat_lens[heavy], ["heavy"] * len(heavy)))
    moves = np.concatenate([p[0] for p in parts])
    lens = np.concatenate([p[1] for p in parts])
    kinds = np.array(sum((p[2] for p in parts), []))
    legal, end_ply, _ = oracle.replay_games(moves, lens)
    assert legal.all() and ((end_ply < 0) | (end_ply == lens)).all()
    ref = oracle.scratch_batch(moves, lens)
    for a in ref:
        a.setflags(write=False)
    assert int(((ref[3] & 2) != 0).sum()) == 0                              # (no board of these asks for more than the kernel's queues hold)
    print("boards per set: %s" % {s: int((kinds == s).sum()) for s in SETS})
    assert all((kinds == s).any() for s in SETS)
    return G.moves_to_planes(moves, lens), ref, kinds


def compare(ref, got, rows, what):
    for name, a, b in zip(NAMES, ref, got):
        a = a[rows]
        bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0]
        print("%s %s: %d of %d boards differ" % (what, name, len(bad), len(a)))
        assert len(bad) == 0, "%s: %s differs on %d of %d boards, first %d" % (what, name, len(bad), len(a), bad[0])


def launches_of(planes, n):
    parts = [G.eval_batch_host(planes[i:i + n]) for i in range(0, len(planes), n)]
    return [np.concatenate(p) for p in zip(*parts)]


@pytest.mark.parametrize("which", SETS)
def test_set_in_one_launch(place_boards, which):
    planes, ref, kinds = place_boards
    rows = np.nonzero(kinds == which)[0]
    got = G.eval_batch_host(planes[rows])
    assert len(got[3]) == len(rows)
    compare(ref, got, rows, "%s, one launch of %d" % (which, len(rows)))


@pytest.mark.parametrize("which", SETS)
def test_set_in_launches_of_17(place_boards, which):
    """a group and a board: the second group is partial; the set's last launch is shorter still"""
    planes, ref, kinds = place_boards
    rows = np.nonzero(kinds == which)[0]
    compare(ref, launches_of(planes[rows], 17), rows, "%s, launches of 17 (%d boards)" % (which, len(rows)))


@pytest.mark.parametrize("which", SETS)
def test_set_in_launches_of_one(place_boards, which):
    """one board, one wavefront at work"""
    planes, ref, kinds = place_boards
    rows = np.nonzero(kinds == which)[0]
    compare(ref, launches_of(planes[rows], 1), rows, "%s, launches of 1 (%d boards)" % (which, len(rows)))
