"""Why K1's phase 3b no longer evaluates the reference's density gate (Pattern.cpp:182: a colour's compound at an empty cell q is looked
at only if the colour's density COUNT at q is two or more).  A (cell, colour) pair reaches phase 3b because a LiveThree, DeadThree or
LiveTwo match of that colour has a '_' piece on q; the match's stones are on the board, on one line through q.  Two facts, both checked
here on the CPU, make the count at least two for every such pair, so the gate never decides anything:

  1. in every pattern of those three types, every '_' has two or more of the pattern's own stones within three cells of it on the line;
  2. the density count at an empty cell counts the colour's stones under the non-zero cells of the 7x7 BlockWeights mask, and those cover
     all eight line directions out to three cells.

The GPU parity tests (tests/test_eval_compound_quads_gpu.py among them) hold the kernel to the oracle, which does evaluate the gate."""
import numpy as np

from gomokuai_amd import lib as G

FEEDING = (3, 4, 5)                # LiveTwo, DeadThree, LiveThree: the types whose '_' pieces count towards compounds
DIRS = ((1, 0), (0, 1), (1, 1), (-1, 1))


def test_every_blank_of_a_compound_feeding_pattern_has_two_own_stones_within_three_cells():
    seen = {t: 0 for t in FEEDING}
    fewest = 99
    for i in range(G.tables_info().n_patterns):
        text, favour, typ, _ = G.tables_pattern(i)
        if typ not in FEEDING:
            continue
        stone = "x" if favour == 1 else "o"
        for k, piece in enumerate(text):
            if piece != "_":
                continue
            near = sum(1 for m, other in enumerate(text) if other == stone and 1 <= abs(m - k) <= 3)
            assert near >= 2, "pattern %r (favour %d, type %d): the '_' at %d has %d own stones within three cells" % (text, favour, typ, k, near)
            fewest = min(fewest, near)
            seen[typ] += 1
    print("'_' pieces per type %s, fewest own stones within three cells: %d" % (seen, fewest))
    assert all(v > 0 for v in seen.values()) and fewest == 2


def test_the_density_count_covers_the_eight_line_directions_to_three_cells(oracle):
    """one black stone in the middle of the board, and in a corner with its mask cut by the edges: black's count plane is 1 on every
    cell of the board within three cells of the stone on a line through it (and the stone's own cell holds ~count)"""
    for sx, sy in ((7, 7), (0, 0), (14, 3)):
        moves = np.zeros((1, 64), dtype=np.uint8)
        moves[0, 0] = 15 * sy + sx
        density = oracle.scratch_batch(moves, np.array([1], dtype=np.int32))[1][0]
        planes = [density[colour, 0].reshape(15, 15) for colour in (0, 1)]
        black = [p for p in planes if (p > 0).any()]             # (the stone's own cell holds ~count in both colours' planes)
        assert len(black) == 1, "one colour has a stone"
        count = black[0]
        checked = 0
        for dx, dy in DIRS:
            for k in (-3, -2, -1, 1, 2, 3):
                x, y = sx + k * dx, sy + k * dy
                if 0 <= x < 15 and 0 <= y < 15:
                    assert count[y, x] == 1, "stone (%d, %d): the count at (%d, %d) is %d" % (sx, sy, x, y, count[y, x])
                    checked += 1
        assert checked >= 9 and count[sy, sx] < 0
