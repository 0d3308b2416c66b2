"""The positions on which the pattern heuristic's float32 restatements and kernels are held to tests/heuristic_f64_reference.py.

TEST INFRASTRUCTURE ONLY.  Built from fixed seeds with the CPU oracle alone (no HIP library), so tests/test_heuristic_f64.py runs
in the CPU suite and tests/test_heuristic_f64_gpu.py draws from the same set.  Every position is live (the game is not over)."""
import functools

import numpy as np

N = 225
c = lambda y, x: y * 15 + x

# the hand-made fours and threes of tests/test_oracle_trad.py ...
OWN_FOUR = [c(7, 7), c(0, 0), c(7, 8), c(0, 2), c(7, 9), c(0, 4), c(7, 10), c(0, 6)]
RIVAL_FOUR = [c(0, 0), c(7, 7), c(0, 2), c(7, 8), c(0, 4), c(7, 9), c(14, 14), c(7, 10)]
OWN_THREE = [c(7, 7), c(0, 0), c(7, 8), c(0, 2), c(7, 9), c(0, 5)]
SEARCHED = [c(7, 7), c(7, 8), c(8, 8), c(6, 6), c(8, 7), c(8, 6)]
# ... a four whose two completing cells are the only non-zero probabilities and lie in cells 192 .. 224 (row 13), one with them in
# cells 0 .. 63 (row 1): the last of a lane's four strided values on its own, and the first
HIGH_CELLS = [c(13, 4), c(0, 0), c(13, 5), c(0, 3), c(13, 6), c(0, 6), c(13, 7), c(0, 9)]
LOW_CELLS = [c(1, 4), c(14, 0), c(1, 5), c(14, 3), c(1, 6), c(14, 6), c(1, 7), c(14, 9)]


def _compounds():
    """Compound positions: two lines of the side to move through one empty cell (7, 7), the rival's stones scattered on the far edge
    rows where they make nothing.  Two open twos make a double three there, an open two and a three with one end shut a four-three,
    two shut threes a double four; each with either side to move and with the colours exchanged (a lone black stone first), so that
    the owner and the answering side both see it in both colours."""
    far = [c(0, 0), c(0, 3), c(0, 6), c(0, 9), c(0, 12), c(14, 1), c(14, 4), c(14, 7), c(14, 10), c(14, 13)]
    open_two_h, open_two_v = [c(7, 8), c(7, 9)], [c(8, 7), c(9, 7)]
    three_h = [c(7, 8), c(7, 9), c(7, 10)]                      # shut at (7, 11) by a rival stone
    three_v = [c(8, 7), c(9, 7), c(10, 7)]                      # shut at (11, 7)
    shapes = {"double_three": (open_two_h + open_two_v, []),
              "four_three": (three_h + open_two_v, [c(7, 11)]),
              "double_four": (three_h + three_v, [c(7, 11), c(11, 7)])}
    out = {}
    for name, (own, shut) in shapes.items():
        rival = shut + [f for f in far if f not in shut][:len(own) - len(shut)]
        for dy, dx in ((0, 0), (-3, -2), (2, 1), (1, -4)):
            sh = lambda cells: [q + dy * 15 + dx if 15 <= q < 210 else q for q in cells]      # the far rows stay where they are
            o, r = sh(own), sh(rival)
            seq = [m for pair in zip(o, r) for m in pair]
            out["%s_%+d%+d_own" % (name, dy, dx)] = seq                                      # black's shape, black to move
            out["%s_%+d%+d_rival" % (name, dy, dx)] = seq + [c(13, 13)]                      # ... white to move: it has to answer
            out["%s_%+d%+d_white_own" % (name, dy, dx)] = [c(13, 13)] + seq                  # white's shape, white to move
            out["%s_%+d%+d_white_rival" % (name, dy, dx)] = [c(13, 13)] + seq[:-1]           # ... black to move
    return out


def tie_order(rng):
    """A game that fills the board without a five: the class construction of
    tests/test_evalstate_gpu.py::test_dense_games_to_the_full_board_and_back, black on one class and white on the other."""
    cls = lambda q: ((q % 15) // 2 + q // 15) % 2
    b = list(rng.permutation([q for q in range(N) if cls(q) == 0]))
    w = list(rng.permutation([q for q in range(N) if cls(q) == 1]))
    seq = []
    while b or w:
        if b:
            seq.append(int(b.pop()))
        if w:
            seq.append(int(w.pop()))
    return seq


def replay(O, moves):
    ev = O.Evaluator()
    for m in moves:
        assert not ev.check_end()
        r, err = ev.apply(int(m))
        assert not err
    return ev


def _live(O, moves):
    """the longest prefix of `moves` that is a live position"""
    ev = O.Evaluator()
    k = 0
    for m in moves:
        ev.apply(int(m))
        if ev.check_end():
            break
        k += 1
    return [int(m) for m in moves[:k]]


@functools.lru_cache(maxsize=None)
def positions():
    """-> list of (group, name, moves), at least 3 000 of them"""
    from oracle import oracle as O
    out = []
    rng = np.random.RandomState(20240611)
    for i in range(1000):                                        # random-permutation prefixes of 1 .. 120 stones
        out.append(("random", "random%d" % i, _live(O, rng.permutation(N)[:1 + i % 120])))
    for i in range(1000):                                        # clustered random games of 1 .. 70 stones
        cy, cx = rng.randint(4, 11, 2)                          # a 9 x 9 window that lies on the board: 81 cells
        window = [c(cy + dy, cx + dx) for dy in range(-4, 5) for dx in range(-4, 5)]
        out.append(("clustered", "clustered%d" % i, _live(O, rng.permutation(window)[:1 + i % 70])))
    for i in range(45):                                          # greedy games with the oracle's own heuristic from 0 .. 8 random stones
        moves = _live(O, rng.permutation(N)[:i % 9])
        ev = replay(O, moves)
        while not ev.check_end():
            out.append(("greedy", "greedy%d_%d" % (i, len(moves)), list(moves)))
            probs, _ = O.trad_heuristic(moves)
            best = int(np.argmax(probs))
            if best in moves:                                    # an all-zero vector: the loop would stall
                break
            ev.apply(best)
            moves.append(best)
    hand = {"own_four": OWN_FOUR, "rival_four": RIVAL_FOUR, "own_three": OWN_THREE, "searched": SEARCHED, "high_cells": HIGH_CELLS,
            "low_cells": LOW_CELLS, "empty": [], "corner": [0], "corner_far": [N - 1]}
    hand.update(_compounds())
    for name, moves in hand.items():
        assert _live(O, moves) == list(moves), name
        out.append(("hand", name, list(moves)))
    for i in range(40):                                          # full-board tie prefixes of 150 .. 224 stones
        seq = tie_order(rng)[:224 if i < 2 else int(rng.randint(150, 225))]
        assert _live(O, seq) == seq
        out.append(("tie", "tie%d" % i, seq))
    assert len(out) >= 3000
    return out
