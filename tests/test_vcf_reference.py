"""The restatement of the forced-win solver's contract (tests/vcf_reference.py), held to positions checked by hand.  CPU only."""
import random

import vcf_reference as R


def cell(x, y):
    return y * 15 + x


def interleave(black, white):
    """A move list, black first, from the two colours' cells (black has as many stones as white, or one more)."""
    assert len(black) - len(white) in (0, 1)
    moves = []
    for i, b in enumerate(black):
        moves.append(b)
        if i < len(white):
            moves.append(white[i])
    return moves


FAR = [cell(0, 14), cell(4, 13), cell(9, 14), cell(14, 12), cell(14, 9), cell(0, 10), cell(12, 7), cell(2, 8)]      # no two of them on a line within four steps
ROW0 = interleave([5, 6, 7], FAR[:3])                          # black 5, 6, 7 on row 0, black to move


def test_open_three_on_row_0():
    r = R.solve(ROW0, max_depth=8)
    assert (r["status"], r["pv"], r["length"], r["nodes"], r["move"]) == (R.WIN, [4, 3, 8], 2, 4, 4)
    R.check_pv(ROW0, r)
    r = R.solve(ROW0, max_depth=1)
    assert (r["status"], r["nodes"], r["move"], r["length"], r["pv"]) == (R.DEPTH, 0, -1, 0, [])
    assert R.solve(ROW0, max_depth=8, opponent=True)["status"] == R.NONE


def test_rows_do_not_wrap():
    """Black at (13,3), (14,3), (0,4), (1,4) are four consecutive cell ids and no line."""
    black = [cell(13, 3), cell(14, 3), cell(0, 4), cell(1, 4)]
    assert [b - black[0] for b in black] == [0, 1, 2, 3]
    moves = interleave(black, FAR[:4])
    r = R.solve(moves, max_depth=8)
    assert (r["status"], r["nodes"]) == (R.NONE, 0)
    assert R.completing(R.board_of(moves), 1) == []


def test_empty_list_and_full_board():
    r = R.solve([], max_depth=8)
    assert (r["status"], r["nodes"]) == (R.NONE, 0)
    r = R.solve(full_board(), max_depth=8)
    assert (r["status"], r["nodes"]) == (R.NONE, 0)


def full_board():
    """225 moves without a five: black where (x + 2 y) mod 4 < 2.  Rows and both diagonals then run B B W W, columns alternate, and black has
    8 cells on each of the 8 even rows and 7 on each of the 7 odd ones: 113 to white's 112."""
    black = [cell(x, y) for y in range(15) for x in range(15) if (x + 2 * y) % 4 < 2]
    white = [c for c in range(225) if c not in black]
    moves = interleave(black, white)
    board = R.board_of(moves)
    assert board is not None and len(moves) == 225 and not R.has_five(board, 1) and not R.has_five(board, 2)
    return moves


def test_a_six_is_over():
    moves = interleave([cell(x, 7) for x in (2, 3, 4, 6, 7, 5)], FAR[:5])
    r = R.solve(moves, max_depth=8)
    assert (r["status"], r["nodes"], r["move"], r["length"]) == (R.OVER, 0, -1, 0)
    assert R.solve(moves, max_depth=8, opponent=True)["status"] == R.OVER


def test_defender_four_answered_by_a_non_four():
    """White has four in a row with one end blocked: black must take the other end, which makes no four of its own -> no candidate."""
    white = [cell(x, 10) for x in (1, 2, 3, 4)]
    black = [cell(0, 10), 5, 6, 7]                              # black also has the open three of ROW0, which it has no time for
    moves = interleave(black, white)
    board = R.board_of(moves)
    assert R.completing(board, 2) == [cell(5, 10)] and R.completing(board, 1) == []
    r = R.solve(moves, max_depth=8)
    assert (r["status"], r["nodes"]) == (R.NONE, 0)


def test_each_status():
    assert R.solve(ROW0, 8)["status"] == R.WIN
    assert R.solve(ROW0, 8, opponent=True)["status"] == R.NONE
    assert R.solve(ROW0, 1)["status"] == R.DEPTH
    r = R.solve(ROW0, 8, budget=2)
    assert (r["status"], r["nodes"], r["move"], r["length"], r["pv"]) == (R.BUDGET, 2, -1, 0, [])
    assert R.solve(interleave([cell(x, 7) for x in range(2, 7)], FAR[:4]), 8)["status"] == R.OVER
    for bad in ([3, 3], [225], list(range(225)) + [0], [7, 300]):
        r = R.solve(bad, 8)
        assert (r["status"], r["nodes"], r["move"], r["length"]) == (R.BAD, 0, -1, 0)


def test_budget_edge():
    k = R.solve(ROW0, 8)["nodes"]
    assert k == 4
    assert R.solve(ROW0, 8, budget=k)["status"] == R.WIN
    r = R.solve(ROW0, 8, budget=k - 1)
    assert (r["status"], r["nodes"]) == (R.BUDGET, k - 1)
    r = R.solve(ROW0, 8, budget=0)
    assert (r["status"], r["nodes"]) == (R.BUDGET, 0)


def test_iterative_finds_the_shorter_win():
    """The plain walk takes the first winning line in cell order, however long; the iterative one the shortest."""
    rng = random.Random(1)
    found = 0
    for _ in range(40):
        moves = R.random_position(rng, 24, 3)
        if moves is None:
            continue
        plain, iterative = R.solve(moves, 12, 5000), R.solve(moves, 12, 5000, iterative=True)
        if plain["status"] == R.WIN:
            assert iterative["status"] == R.WIN and iterative["length"] <= plain["length"]
            R.check_pv(moves, plain)
            R.check_pv(moves, iterative)
            found += iterative["length"] < plain["length"]
    assert found >= 3


def test_iterative_on_row_0():
    r = R.solve(ROW0, 8, iterative=True)                       # limit 1: cut at the root; limit 2: cell 3 (its child is cut), then cell 4
    assert (r["status"], r["pv"], r["nodes"]) == (R.WIN, [4, 3, 8], 2)
    r = R.solve(ROW0, 8, opponent=True, iterative=True)        # limit 1 is cut, limit 2 fails without a cut and ends the run
    assert (r["status"], r["nodes"]) == (R.NONE, 0)


def test_every_win_replays():
    rng = random.Random(7)
    wins = 0
    for plies, spread in ((16, 3), (30, 4), (60, 5)):
        done = 0
        while done < 12:
            moves = R.random_position(rng, plies, spread)
            if moves is None:
                continue
            done += 1
            for opponent in (False, True):
                r = R.solve(moves, 10, 2000, opponent=opponent)
                if r["status"] == R.WIN:
                    R.check_pv(moves, r, opponent)
                    wins += 1
                else:
                    assert (r["move"], r["length"], r["pv"]) == (-1, 0, [])
    assert wins >= 20


def test_the_shortcut_is_the_full_count():
    """fours_after looks only along the lines through the new stone; on boards without a completing cell that is all of completing()."""
    rng = random.Random(11)
    checked = 0
    while checked < 300:
        moves = R.random_position(rng, *rng.choice(((10, 3), (24, 3), (40, 4), (60, 5))))
        if moves is None:
            continue
        board = R.board_of(moves)
        for colour in (1, 2):
            for c in rng.sample([e for e in range(225) if board[e] == 0], 6):
                near = R.fours_after(board, c, colour)
                board[c] = colour
                assert near == R.completing(board, colour)
                board[c] = 0
                checked += 1
