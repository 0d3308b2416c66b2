"""K1's frame -- what every board pays for whatever is on it: phase 0 (clears, line words, the score block's start values), the loop head and
phase 5 (the write-out, whose stores take one scalar base per board and immediate offsets) -- against the oracle's from-scratch evaluator
(oracle/go_scratch.c) on positions built by hand to sit where that code has its edges.  Integer outputs: exact.

A position is a move list (black first, colours alternate), so black has as many stones as white or one more; `position` interleaves the
two colours' cells and says so if they cannot be interleaved."""
import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

NAMES = ("scores", "density", "totals", "status")
WORDS = (900, 900, 11, 1)
SENTINEL = 0x5A5A5A5A
STRIDE = 232                       # a move list's row: 225 moves and padding
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


def check(oracle, positions, what):
    moves, lens = pack(positions)
    ref = oracle.scratch_batch(moves, lens)
    compare(ref, G.eval_batch_host(G.moves_to_planes(moves, lens)), what)
    return ref


def status_fields(word):
    """(over, flagged, winner, to_move) of a status word"""
    s8 = lambda v: v - 256 if v > 127 else v
    return bool(word & 1), bool(word & 2), s8((int(word) >> 8) & 0xFF), s8((int(word) >> 16) & 0xFF)


# ---- item: the score block's start values, written per quarter row / per cell pass ----

def quarter_row_positions():
    """Sixty positions, one per quarter row (cells 0-3, 4-7, 8-11, 12-14 of a row): every cell of it holds a stone, colours alternating."""
    out = []
    for y in range(15):
        for part in range(4):
            cells = [cell(x, y) for x in range(4 * part, min(4 * part + 4, 15))]
            out.append(position(cells[0::2], cells[1::2]))
    return out


def row_end_positions():
    """The first and the last cell of a row, for every row on its own, in both colour orders, and for all rows at once (colours alternating
    down the two columns: no five)."""
    out = []
    for y in range(15):
        out.append(position([cell(0, y)], [cell(14, y)]))
        out.append(position([cell(14, y)], [cell(0, y)]))
        out.append(position([cell(0, y)], []))
        out.append(position([cell(14, y), cell(7, (y + 7) % 15)], [cell(0, y)]) if y != 7 else position([cell(14, y), cell(7, 0)], [cell(0, y)]))
    black = [cell(0, y) for y in range(0, 15, 2)] + [cell(14, y) for y in range(1, 15, 2)]
    white = [cell(0, y) for y in range(1, 15, 2)] + [cell(14, y) for y in range(0, 15, 2)]
    out.append(position(black, white))
    return out


def test_quarter_rows_and_row_ends(oracle):
    check(oracle, quarter_row_positions(), "quarter rows")
    check(oracle, row_end_positions(), "row ends")


# ---- item: the status word on the scalar unit ----

def full_board():
    """All 225 cells, no five anywhere: colour by (x + 2 y) mod 4 < 2 -- runs of two along rows and both diagonals, of one along columns --
    with single cells flipped until black has 113 stones (a flip is kept only if it lengthens no run to five: checked here, not assumed)."""
    black = {(x, y) for x in range(15) for y in range(15) if (x + 2 * y) % 4 < 2}

    def longest_run(stones):
        best = 0
        for (x, y) in stones:
            for dx, dy in DIRS:
                n = 1
                while (x + n * dx, y + n * dy) in stones:
                    n += 1
                best = max(best, n)
        return best

    every = {(x, y) for x in range(15) for y in range(15)}
    for (x, y) in sorted(every):
        if len(black) == 113:
            break
        trial = black ^ {(x, y)}
        if abs(len(trial) - 113) < abs(len(black) - 113) and longest_run(trial) < 5 and longest_run(every - trial) < 5:
            black = trial
    assert len(black) == 113 and longest_run(black) < 5 and longest_run(every - black) < 5
    return position([cell(x, y) for (x, y) in sorted(black)], [cell(x, y) for (x, y) in sorted(every - black)])


def test_empty_and_full_board(oracle):
    ref = check(oracle, [position([], []), full_board(), position([cell(7, 7)], []), position([cell(7, 7)], [cell(8, 8)])], "empty / full / one / two stones")
    assert status_fields(ref[3][0]) == (False, False, 0, 1), "the empty board: black to move"
    assert status_fields(ref[3][1]) == (True, False, 0, 0), "the full board without a five: over, a draw, nobody to move"
    assert status_fields(ref[3][2]) == (False, False, 0, -1) and status_fields(ref[3][3]) == (False, False, 0, 1)


def five_positions():
    """A five for each colour in each direction (the other colour's stones scattered on the far rows, never two in line next to each other)."""
    out, expect = [], []
    for d, (dx, dy) in enumerate(DIRS):
        x0, y0 = (9 if dx < 0 else 3), 4
        five = [cell(x0 + i * dx, y0 + i * dy) for i in range(5)]
        far = [cell(2 * i, 12 + (i & 1) * 2) for i in range(5)]
        out.append(position(five, far[:4]))         # black's fifth stone ends the game
        expect.append(1)
        out.append(position(far, five))             # white's
        expect.append(-1)
    return out, expect


def test_a_five_for_each_colour(oracle):
    positions, expect = five_positions()
    ref = check(oracle, positions, "fives")
    for i, want in enumerate(expect):
        assert status_fields(ref[3][i]) == (True, False, want, 0), "position %d: winner %d expected, the oracle says %s" % (i, want, status_fields(ref[3][i]))


# ---- item: the component entry of phase 3b -> phase 4 ----

def compound_positions():
    """Two open twos of one colour that cross in an empty cell q: a compound of two components (a double two), the kind whose components are
    queued for the counter-move rescans.  q x every pair of directions x both colours, at the board's centre, and with one component on the
    longest diagonal / anti-diagonal (15 cells) and on the shortest ones that can hold an open two."""
    out = []

    def cross(q, d1, d2, colour, s1=1, s2=1):
        (qx, qy), own = q, []
        for (dx, dy), s in ((DIRS[d1], s1), (DIRS[d2], s2)):
            own += [cell(qx + s * k * dx, qy + s * k * dy) for k in (1, 2)]
        used = set(own) | {cell(qx, qy)}
        # the other colour's stones: far from q, never adjacent to each other
        spare = [c for c in (cell(x, y) for y in (0, 14) for x in range(0, 15, 2)) if c not in used and all(abs(c % 15 - u % 15) > 3 or abs(c // 15 - u // 15) > 3 for u in used)]
        other = spare[:4]
        assert len(other) == 4, "no room for the other colour's stones"
        return position(own, other) if colour > 0 else position(other + [spare[4]], own)

    for colour in (1, -1):
        for d1 in range(4):
            for d2 in range(d1 + 1, 4):
                out.append(cross((7, 7), d1, d2, colour))
        # the longest diagonal (x = y) and anti-diagonal (x + y = 14), each crossed with a row and a column
        out.append(cross((6, 6), 2, 0, colour))
        out.append(cross((6, 6), 2, 1, colour))
        out.append(cross((6, 8), 3, 0, colour))
        out.append(cross((8, 6), 3, 1, colour, s1=-1))
        # short diagonals: x - y = +-8 (seven cells) and x + y = 6, 22 (seven cells), the component two cells into the line
        out.append(cross((10, 2), 2, 1, colour))
        out.append(cross((2, 10), 2, 0, colour))
        out.append(cross((4, 2), 3, 1, colour))
        out.append(cross((12, 10), 3, 0, colour, s2=-1))
    return out


def test_compound_components_on_every_direction(oracle):
    positions = compound_positions()
    ref = check(oracle, positions, "compounds")
    compounds = (ref[2][:, 8:11] != 0).any(axis=1)
    print("positions with a compound, by the oracle: %d of %d" % (int(compounds.sum()), len(positions)))
    assert compounds.all(), "positions %s hold no compound by the oracle: the construction is wrong" % np.nonzero(~compounds)[0].tolist()


def test_shortest_lines_hold_patterns(oracle):
    """Every line of five cells and more (the four shortest diagonals and anti-diagonals among them) with an open three of either colour on its
    first cells that can hold one, and the lines of four cells (no pattern fits: their cells only take part in other lines)."""
    out = []
    for colour in (1, -1):
        for (x0, y0, dx, dy, n) in [(10, 0, 1, 1, 5), (0, 10, 1, 1, 5), (4, 0, -1, 1, 5), (14, 10, -1, 1, 5), (9, 0, 1, 1, 6), (5, 0, -1, 1, 6),
                                    (11, 0, 1, 1, 4), (3, 0, -1, 1, 4), (0, 0, 1, 1, 15), (14, 0, -1, 1, 15)]:
            own = [cell(x0 + k * dx, y0 + k * dy) for k in range(1, min(n - 1, 4))]
            spare = [c for c in (cell(x, 7) for x in (0, 3, 6, 9, 12)) if c not in own]
            out.append(position(own, spare[:len(own) - 1]) if colour > 0 else position(spare[:len(own)], own))
    check(oracle, out, "short lines")


# ---- item: the write-out's immediates ----

@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
def test_every_output_stays_inside_its_boards(oracle, n):
    """Sixteen boards of a sentinel behind every output buffer, and one board of it in front: intact after the launch; the boards themselves
    equal to the oracle's.  The hand-made positions above are spread through the batch (its last board among them)."""
    import torch
    G.init(0)
    dev = torch.device("cuda", 0)
    moves, lens, _ = G.synth_boards(n, n & 1, first_board=110000 + 13 * n, stride=STRIDE)
    special = quarter_row_positions() + row_end_positions() + [position([], []), full_board()] + five_positions()[0] + compound_positions()
    step = max(1, n // len(special))
    for i, p in enumerate(special):
        at = n - 1 - i * step
        if at < 0:
            break
        moves[at] = 0
        moves[at, :len(p)] = p
        lens[at] = len(p)
    planes = G.moves_to_planes(moves, lens)
    ref = oracle.scratch_batch(moves, lens)
    front, extra = 1, 16
    d_planes = torch.from_numpy(planes.view(np.int16).reshape(n, 32)).to(dev)
    sentinel = np.int32(SENTINEL)
    bufs = [torch.full(((front + n + extra) * words,), int(sentinel), dtype=torch.int32, device=dev) for words in WORDS]
    ptrs = [b.data_ptr() + 4 * front * words for b, words in zip(bufs, WORDS)]
    G.eval_batch(d_planes.data_ptr(), n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for name, h, words in zip(NAMES, host, WORDS):
        outside = np.concatenate([h[:front * words], h[(front + n) * words:]])
        touched = int((outside != sentinel).sum())
        print("n=%d %s: %d of %d sentinel words overwritten" % (n, name, touched, outside.size))
        assert touched == 0, "%s: %d words outside boards 0 .. %d were written" % (name, touched, n - 1)
    body = [h[front * words:(front + n) * words] for h, words in zip(host, WORDS)]
    got = (body[0].reshape(n, 4, 225), body[1].reshape(n, 2, 2, 225), body[2].view(np.uint32).reshape(n, 11), body[3])
    compare(ref, got, "n=%d (device buffers)" % n)
