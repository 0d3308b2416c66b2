"""K1's scan queues, with every emitting transition, the PLACE of the symbol it consumed -- cell, direction, minus the stride -- and the deposits
use the entry as it is (eval_kernel.hip, phases 1 and 2).  The place is a running value: the lane record's place word at step 4, plus the stride
(byte 3 of the record's lines word) per step, plus a signed jump where a two-line lane steps from its first line's second pad onto its second
line's first cell.  For that, a lane's two lines have to lie in the same direction.

On the CPU, with the host's own lane records (lib.eval_lane_records, the words gmk_eval_batch stages) and transition table (lib.tables_copy):
  * the records' fields against the lane table restated in tests/eval_place_reference.py;
  * the packed place of every lane at every step 4..16 against the plain statement: segment, place on the line, first cell + place * stride;
  * the eight pairs: one direction each, seventeen symbols each, the seam steps the kernel's text fixes;
  * the one place that needs a ninth cell bit: the main diagonal's second trailing pad, step 16, is "cell" 256, and some filling of the main
    diagonal does report a match on that step."""
import itertools

import numpy as np

import eval_place_reference as R
from gomokuai_amd import lib as G

COL_BASE, DIAG_BASE, ANTI_BASE = 20, 36, 65                                 # line word indices (eval_kernel.hip, kLineWords)


def _line_word(direction, cells):
    x0, y0 = cells[0] % 15, cells[0] // 15
    return (y0, COL_BASE + x0, DIAG_BASE + x0 - y0 + 14, ANTI_BASE + x0 + y0)[direction]


def test_record_fields_are_the_restated_lane_table():
    rec = G.eval_lane_records()
    ls = R.lines()
    for lane in range(64):
        d, cells = ls[lane]
        other = R.second_line(lane)
        lines_word, place_word = int(rec[lane, 0]), int(rec[lane, 1])
        assert lines_word & 31 == len(cells) + R.PADS, "lane %d" % lane
        assert (lines_word >> 10) & 127 == _line_word(d, cells), "lane %d" % lane
        assert lines_word >> 24 == R.STRIDES[d], "lane %d" % lane
        if other is None:
            assert (lines_word >> 5) & 31 == R.PADS and (lines_word >> 17) & 127 == 15 and place_word >> 17 == 0, "lane %d" % lane
        else:
            assert (lines_word >> 5) & 31 == len(ls[other][1]) + R.PADS and (lines_word >> 17) & 127 == _line_word(*ls[other]), "lane %d" % lane
        assert place_word & 0x1FFFF == R.entry_bits(cells[0] + R.PREFIX * R.STRIDES[d], d, R.STRIDES[d]), "lane %d" % lane
        assert place_word >> 27 == 0, "lane %d" % lane


def test_packed_place_is_the_plain_statement_at_every_step():
    rec = G.eval_lane_records()
    ls = R.lines()
    got = R.packed_places(rec)
    top = 0
    for lane in range(64):
        for step in range(R.PREFIX, R.STEPS):
            cell, d, stride = R.plain_place(ls, lane, step)
            assert 0 <= cell < 512
            top = max(top, cell)
            assert got[lane, step] == R.entry_bits(cell, d, stride), "lane %d step %d: packed %#x, plain (%d, %d, %d)" % (lane, step, got[lane, step], cell, d, stride)
            # ... and what phase 2 reads out of the entry
            e = int(got[lane, step])
            back = (e >> 11) & 63
            assert (e & 511, (e >> 9) & 3, back - 64 if back & 32 else back) == (cell, d, -stride)
    print("largest place: %d" % top)


def test_pairs_are_one_direction_and_seventeen_symbols():
    pairs = R.pairs()
    assert [lane for lane, _, _ in pairs] == list(range(56, 64))
    seen = set()
    for lane, (da, a), (db, b) in pairs:
        assert da == db and da in (2, 3), "lane %d pairs directions %d and %d" % (lane, da, db)
        assert len(a) + R.PADS + len(b) + R.PADS == R.STEPS and len(a) >= R.PREFIX
        assert len(a) + R.PADS == (R.SEAM_STEP_LONG if lane < 60 else R.SEAM_STEP_SHORT)
        assert (len(a), len(b)) == ((8, 5) if lane < 60 else (7, 6))
        assert not set(a) & set(b)
        seen |= {tuple(a), tuple(b)}
    ls = R.lines()
    assert seen == {tuple(c) for _, c in ls[56:]}                            # the sixteen shortest lines, each once
    assert sorted(len(c) for _, c in ls[56:64]) == [7] * 4 + [8] * 4
    # per direction: one 8 + 5 and one 7 + 6 ... twice
    assert sorted((da, len(a)) for _, (da, a), _ in pairs) == [(2, 7), (2, 7), (2, 8), (2, 8), (3, 7), (3, 7), (3, 8), (3, 8)]


def test_main_diagonal_reports_on_step_16_at_cell_256():
    ls = R.lines()
    d, cells = ls[R.MAIN_DIAGONAL_LANE]
    assert d == 2 and cells == [16 * i for i in range(15)]
    assert R.plain_place(ls, R.MAIN_DIAGONAL_LANE, 16) == (256, 2, 16)
    assert R.packed_places(G.eval_lane_records())[R.MAIN_DIAGONAL_LANE, 16] == R.entry_bits(256, 2, 16)
    # every other symbol of every line stays below 256 (the 14-cell diagonal from cell 15 ends its stream on 255): the ninth bit is for this one symbol
    trans, _, _ = G.tables_copy()
    hits = [t for t in itertools.product((0, 1, 3), repeat=6) if R.reports_on_last_pad(trans, t)]
    print("of the 729 fillings of the main diagonal's last six cells, %d report on step 16, e.g. %s" % (len(hits), hits[:3]))
    assert len(hits) > 0
    top = max(R.plain_place(ls, lane, step)[0] for lane in range(64) for step in range(R.PREFIX, R.STEPS)
              if step < sum(len(ls[i][1]) + R.PADS for i in (lane, R.second_line(lane)) if i is not None) and (lane, step) != (R.MAIN_DIAGONAL_LANE, 16))
    print("largest place of a symbol of a line besides it: %d" % top)
    assert top == 255
