"""K1's lane table restated in Python (eval_kernel.hip, "Lane -> lines" and lane_tables): the 72 lines of five or more cells sorted as the host
sorts them, the pairing of the eight leftovers with a line of their own direction, the plain statement of where step s of a lane's stream lies,
and the kernel's arithmetic on the lane record's two packed words.  Shared by tests/test_eval_place_entries.py and its GPU counterpart."""
import numpy as np

STRIDES = (1, 15, 16, 14)                                                   # rows, columns, diagonals, anti-diagonals
PADS = 2
STEPS = 17
PREFIX = 4
FIRST_PAIRED = 56
SEAM_STEP_LONG, SEAM_STEP_SHORT = 10, 9                                     # the second line's first cell: lanes 56..59 (8 cells first), 60..63 (7 cells)
MAIN_DIAGONAL_LANE = 30                                                     # rows 0..14, columns 15..29, then the 15-cell diagonal and anti-diagonal


def lines():
    """-> [(direction, [cells])], the longest first, the order of the host's stable sort"""
    out = [(0, [15 * y + x for x in range(15)]) for y in range(15)] + [(1, [15 * y + x for y in range(15)]) for x in range(15)]
    for d in range(-10, 11):
        x0, y0 = (d, 0) if d > 0 else (0, -d)
        out.append((2, [15 * (y0 + i) + x0 + i for i in range(15 - abs(d))]))
    for k in range(4, 25):
        x0 = min(k, 14)
        y0 = k - x0
        out.append((3, [15 * (y0 + i) + x0 - i for i in range(min(k, 28 - k) + 1)]))
    out.sort(key=lambda l: -len(l[1]))
    assert len(out) == 72 and [len(l[1]) for l in out[56:]] == [8] * 4 + [7] * 4 + [6] * 4 + [5] * 4
    return out


def second_line(lane):
    """the index of the line that rides behind lane's first one, or None: 5 cells behind 8 (lanes 56..59), 6 behind 7 (lanes 60..63)"""
    if lane < FIRST_PAIRED:
        return None
    return lane + 12 if lane < FIRST_PAIRED + 4 else lane + 4


def pairs():
    """-> [(lane, first line, second line)] of the eight lanes that walk two lines, lines as (direction, cells)"""
    ls = lines()
    return [(lane, ls[lane], ls[second_line(lane)]) for lane in range(FIRST_PAIRED, 64)]


def plain_place(ls, lane, step):
    """where step `step` of lane's stream lies, stated plainly: which segment, the place on its line, first cell + place * stride -> (cell, direction, stride)"""
    d, cells = ls[lane]
    seg_a = len(cells) + PADS
    other = second_line(lane)
    if other is not None and step >= seg_a:
        d, cells = ls[other]
        step -= seg_a
    return cells[0] + step * STRIDES[d], d, STRIDES[d]


def entry_bits(cell, direction, stride):
    """the low 17 bits of a queue entry: cell | direction << 9 | (minus the stride, six bits) << 11"""
    return cell | direction << 9 | ((-stride) & 63) << 11


def packed_places(records):
    """the kernel's arithmetic on the lane records ([64, 8] uint32): -> [64, 17] int64, the low 17 bits of the running place at steps 4..16 (0 in front)"""
    out = np.zeros((64, STEPS), dtype=np.int64)
    for lane in range(64):
        lines_word, place_word = int(records[lane, 0]), int(records[lane, 1])
        jump = (place_word >> 17) & 1023
        jump -= 1024 if jump & 512 else 0                                   # a signed 10-bit field
        place = place_word
        for step in range(PREFIX, STEPS):
            if step > PREFIX:
                place = (place + (lines_word >> 24)) & 0xFFFFFFFF           # + byte 3, the stride
            if (step == SEAM_STEP_SHORT and lane >= FIRST_PAIRED + 4) or (step == SEAM_STEP_LONG and FIRST_PAIRED <= lane < FIRST_PAIRED + 4):
                place = (place + jump) & 0xFFFFFFFF
            out[lane, step] = place & 0x1FFFF
    return out


def reports_on_last_pad(trans, cells_tail):
    """Walks `blank ... blank cells_tail ? ?`, the main diagonal's 17 symbols, from S as the scan does -> True iff the transition on the second
    trailing pad, step 16, reports a match.  Symbols: 0 black, 1 white, 2 '?', 3 blank.  trans: the host's table (lib.tables_copy)."""
    nxt = (trans & 0x3FF).astype(np.int64).reshape(-1, 4)
    lst = ((trans >> 10) & 0x3FF).astype(np.int64).reshape(-1, 4)
    state = int(nxt[0, 2])                                                  # S: the root on '?'
    stream = [3] * (15 - len(cells_tail)) + list(cells_tail) + [2, 2]
    report = 0
    for sym in stream:
        report = int(lst[state, sym])
        state = int(nxt[state, sym])
    return report != 0
