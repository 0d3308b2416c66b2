"""Board sets for K1's phase 3b as it runs since round 15 -- four lanes per (candidate cell, colour) pair, sixteen pairs per round -- shared by
tests/test_eval_compound_quads.py (CPU: the sets hold what they claim, by the oracle's load counts) and tests/test_eval_compound_quads_gpu.py.
A position is a move list, black first; everything is built from a fixed seed, the same boards on every run.

Gadgets around an empty cell q (directions as the kernel numbers them: 0 row, 1 column, 2 diagonal, 3 anti-diagonal):
  cross   two lines of one colour's stones that start next to q, two or three stones each: a compound at q
  dual    white's two-stone lines along directions 0 and 1 and black's along 2 and 3, around the SAME q: a candidate of both colours
Stones that only make up the colours' balance ("fillers") stand five or more cells from each other and more than three from every
gadget cell where a set promises that one colour alone has candidates: two stones that far apart are part of no pattern."""
import random

import numpy as np

STRIDE = 232
DIRS = ((1, 0), (0, 1), (1, 1), (-1, 1))


def cell(x, y):
    return 15 * y + x


def on_board(x, y):
    return 0 <= x < 15 and 0 <= y < 15


def cross(q, arms):
    """arms: (direction, sign, stones) -> the cells of the lines that start next to q, or None where one leaves the board"""
    out = []
    for d, s, n in arms:
        for k in range(1, n + 1):
            x, y = q[0] + s * k * DIRS[d][0], q[1] + s * k * DIRS[d][1]
            if not on_board(x, y):
                return None
            out.append(cell(x, y))
    return out if len(set(out)) == len(out) else None


def fillers(used, count, apart, clear):
    """`count` cells `apart` or more from each other (Chebyshev) and more than `clear` from every used cell, spread over the board; None if there is no room"""
    if count == 0:
        return []
    free = [(x, y) for y in range(15) for x in range(15) if all(max(abs(x - u % 15), abs(y - u // 15)) > clear for u in used)]
    out = []
    for p in free:
        if all(max(abs(p[0] - o[0]), abs(p[1] - o[1])) >= apart for o in out):
            out.append(p)
    if len(out) < count:
        return None
    step = max(1, len(out) // count)
    return [cell(*p) for p in out[::step][:count]]


def position(black, white, empty, pure):
    """the move list of black's and white's stones with the balance made up by fillers (pure: fillers that are part of no pattern), or None"""
    used = set(black) | set(white) | set(empty)
    if len(used) != len(black) + len(white) + len(set(empty)):
        return None
    short = len(black) - len(white)
    extra = fillers(used, short - 1 if short > 0 else -short, 5 if pure else 3, 3 if pure else 1)
    if extra is None:
        return None
    black, white = (list(black), list(white) + extra) if short > 0 else (list(black) + extra, list(white))
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


def random_board(rng, mode, gadgets):
    """mode 'white' / 'black': that colour's crosses and the other's fillers; 'mixed': crosses of either colour and duals"""
    black, white, empty = [], [], []
    for _ in range(gadgets):
        for _attempt in range(20):
            q = (rng.randrange(15), rng.randrange(15))
            d1, d2 = rng.sample(range(4), 2)
            kind = rng.choice(("two-two", "two-two", "three-two", "dual")) if mode == "mixed" else rng.choice(("two-two", "two-two", "three-two"))
            s1, s2 = rng.choice((1, -1)), rng.choice((1, -1))
            if kind == "dual":
                a, b = cross(q, [(0, s1, 2), (1, s2, 2)]), cross(q, [(2, s1, 2), (3, s2, 2)])
                parts = None if a is None or b is None else (b, a)
            else:
                own = cross(q, [(d1, s1, 3 if kind == "three-two" else 2), (d2, s2, 2)])
                colour = {"white": -1, "black": 1}.get(mode) or rng.choice((1, -1))
                parts = None if own is None else ((own, []) if colour > 0 else ([], own))
            if parts is None:
                continue
            cells = set(parts[0]) | set(parts[1]) | {cell(*q)}
            taken = set(black) | set(white) | set(empty)
            # a gadget keeps one cell's distance from the ones before it (their stones would lengthen its lines)
            if any(max(abs(c % 15 - t % 15), abs(c // 15 - t // 15)) <= 1 for c in cells for t in taken):
                continue
            black += parts[0]; white += parts[1]; empty.append(cell(*q))
            break
    return position(black, white, empty, mode != "mixed")


def candidate_sweep(oracle, counts=range(1, 21), tries=1500, seed=20150):
    """-> {mode: {n: move list}}: for every mode the first board of a seeded random series with exactly n candidate cells and no five"""
    F = oracle.LOAD_FIELDS
    found = {}
    for mode, most, share in (("white", 3, 8), ("black", 3, 8), ("mixed", 14, 1)):
        rng = random.Random(seed + len(mode))
        boards = [b for b in (random_board(rng, mode, 1 + i % most) for i in range(tries // share)) if b is not None]
        load = oracle.scratch_load(*pack(boards))
        found[mode] = {}
        for b, row in zip(boards, load):
            n = int(row[F.index("candidates")])
            if n in counts and row[F.index("fives")] == 0 and n not in found[mode]:
                found[mode][n] = b
    return found


def edge_row_boards():
    """crosses whose q lies in rows 0..2 and 12..14 (phase 3b's rows around q fall on the zero padding), every pair of directions that fits,
    both colours; and a dual in each of the rows"""
    out = []
    for qy in (0, 1, 2, 12, 13, 14):
        sy = 1 if qy < 7 else -1                                  # the lines run into the board
        for qx in (3, 11):
            sx = 1 if qx < 7 else -1
            for d1 in range(4):
                for d2 in range(d1 + 1, 4):
                    sign = lambda d: sx if d == 0 else sy if d == 1 else sy if d == 2 else sy      # directions 1..3 move in y by their sign
                    own = cross((qx, qy), [(d1, sign(d1), 2), (d2, sign(d2), 2)])
                    if own is None:
                        continue
                    for colour in (1, -1):
                        p = position(own if colour > 0 else [], [] if colour > 0 else own, [cell(qx, qy)], True)
                        if p is not None:
                            out.append(p)
            a, b = cross((qx, qy), [(0, sx, 2), (1, sy, 2)]), cross((qx, qy), [(2, sy, 2), (3, sy, 2)])
            if a is not None and b is not None:
                p = position(b, a, [cell(qx, qy)], True)
                if p is not None:
                    out.append(p)
    return out


def direction_order_boards():
    """compounds of exactly two components along directions (0, 3) and (1, 2), at four cells, both colours, the lines on either side of q: the quad's
    lane 0 queues the lower direction's rescan, lane 1 the higher one's"""
    out = []
    for q in ((7, 7), (4, 9), (10, 5), (3, 3)):
        for d1, d2 in ((0, 3), (1, 2)):
            for s1, s2 in ((1, 1), (-1, 1), (1, -1)):
                own = cross(q, [(d1, s1, 2), (d2, s2, 2)])
                if own is None:
                    continue
                for colour in (1, -1):
                    p = position(own if colour > 0 else [], [] if colour > 0 else own, [cell(*q)], True)
                    if p is not None:
                        out.append(p)
    return out
