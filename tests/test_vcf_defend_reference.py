"""The restatement of the defence's contract (tests/vcf_defend_reference.py, "K15" in include/gomoku_hip.h), held to positions checked by hand
and, for soundness, to a full solve of every cell.  CPU only."""
import random

import vcf_defend_reference as DR
import vcf_reference as R


def cell(x, y):
    return y * 15 + x


def interleave(black, white):
    assert len(black) - len(white) in (0, 1)
    moves = []
    for i, b in enumerate(black):
        moves.append(b)
        if i < len(white):
            moves.append(white[i])
    return moves


OPEN_THREE = [cell(5, 7), cell(0, 0), cell(6, 7), cell(14, 0), cell(7, 7)]      # black 110, 111, 112 on row 7; white to move
FAR = [cell(0, 14), cell(14, 12), cell(14, 9), cell(0, 10), cell(12, 0)]        # no two of them on a line within four steps, and off the lines used


def empties(moves):
    return [c for c in range(225) if c not in moves]


def test_the_open_three():
    d = DR.defend(OPEN_THREE, 8, 1000)
    t = d["threat"]
    assert (t["status"], t["pv"], t["length"], t["nodes"]) == (R.WIN, [109, 108, 113], 2, 4)
    assert DR.cells_with(d, DR.CELL_HOLDS) == [109, 113]
    loses = DR.cells_with(d, DR.CELL_LOSES)
    assert len(loses) == 218 and loses == [c for c in empties(OPEN_THREE) if c not in (109, 113)]
    assert all(d["length"][c] == 2 for c in loses) and 108 in loses          # the far end of the three loses: 109 then makes a four with two ends
    assert d["searched"] == [108, 109, 113] and [d["nodes"][c] for c in d["searched"]] == [2, 2, 2]
    assert sum(d["nodes"]) == 6 and all(d["length"][c] == 0 for c in (109, 113))
    assert DR.cells_with(d, DR.CELL_NONE) == sorted(OPEN_THREE)
    assert not DR.cells_with(d, DR.CELL_UNKNOWN) and not DR.cells_with(d, DR.CELL_FIVE)
    assert DR.defend(OPEN_THREE, 8, 1000, iterative=True)["verdict"] == d["verdict"]


def test_the_defender_has_four_in_a_row():
    moves = [cell(*xy) for xy in [(5, 7), (1, 0), (6, 7), (2, 0), (7, 7), (3, 0), (10, 12), (4, 0), (12, 3)]]
    d = DR.defend(moves, 8, 1000)
    assert d["threat"]["status"] == R.NONE                                   # two completing cells of the defender: the attacker's walk fails at once
    assert DR.cells_with(d, DR.CELL_FIVE) == [0, 5]
    assert DR.cells_with(d, DR.CELL_HOLDS) == [c for c in empties(moves) if c not in (0, 5)]
    assert d["searched"] == [] and not any(d["nodes"]) and not any(d["length"])


def test_a_threat_that_is_already_a_four():
    """Black 110 .. 113 with white on 109: the only block is 114.  Every other cell loses in 1."""
    moves = interleave([110, 111, 112, 113, FAR[0]], [109, FAR[1], FAR[2], FAR[3]])
    d = DR.defend(moves, 8, 1000)
    assert (d["threat"]["status"], d["threat"]["pv"], d["threat"]["length"]) == (R.WIN, [114], 1)
    assert DR.cells_with(d, DR.CELL_HOLDS) == [114] and d["searched"] == [114]
    loses = DR.cells_with(d, DR.CELL_LOSES)
    assert loses == [c for c in empties(moves) if c != 114] and all(d["length"][c] == 1 for c in loses)
    # an open four has no block
    moves = interleave([110, 111, 112, 113, FAR[0]], [FAR[4], FAR[1], FAR[2], FAR[3]])
    d = DR.defend(moves, 8, 1000)
    assert d["threat"]["pv"] == [109] and not DR.cells_with(d, DR.CELL_HOLDS)
    assert d["searched"] == [] and DR.cells_with(d, DR.CELL_LOSES) == empties(moves)       # with 109 taken 114 still completes: follow's first test
    assert all(d["length"][c] == 1 for c in empties(moves))


def test_a_counter_four_that_holds():
    """Black's open three on row 7; white has 33, 34, 35 on row 2 with black on 32.  White 36 or 37 makes a four whose block is no black four,
    so besides the two ends of the three those two cells hold."""
    moves = interleave([110, 111, 112, 32, FAR[0]], [33, 34, 35, FAR[1]])
    d = DR.defend(moves, 8, 1000)
    assert (d["threat"]["status"], d["threat"]["pv"]) == (R.WIN, [109, 108, 113])
    assert DR.cells_with(d, DR.CELL_HOLDS) == [36, 37, 109, 113]
    assert set(d["searched"]) >= {36, 37} and d["nodes"][36] == 0 and d["nodes"][37] == 0
    assert not DR.cells_with(d, DR.CELL_FIVE) and not DR.cells_with(d, DR.CELL_UNKNOWN)


def test_over_and_bad_lists():
    over = interleave([cell(x, 7) for x in range(2, 7)], FAR[:4])
    for moves, status in ((over, R.OVER), ([3, 3], R.BAD), ([225], R.BAD), (list(range(225)) + [0], R.BAD)):
        d = DR.defend(moves, 8, 1000)
        assert d["threat"]["status"] == status
        assert d["verdict"] == [DR.CELL_NONE] * 225 and not any(d["length"]) and not any(d["nodes"]) and d["searched"] == []


def test_a_budget_too_small_for_a_cell():
    """random_position(Random(5), 20, 3)'s first position whose threat is found within 6 nodes while some replies need more."""
    moves = [142, 141, 64, 160, 155, 109, 68, 99, 110, 145, 126, 100, 83, 157, 139, 140, 67, 96, 130, 158]
    d = DR.defend(moves, 8, 6)
    assert (d["threat"]["status"], d["threat"]["nodes"], d["threat"]["length"]) == (R.WIN, 5, 5)
    unknown = DR.cells_with(d, DR.CELL_UNKNOWN)
    assert unknown == [38, 53, 80, 113, 128, 156, 159, 161] and all(d["nodes"][c] == 6 and d["length"][c] == 0 for c in unknown)
    assert DR.cells_with(d, DR.CELL_HOLDS) == [65, 66, 78, 94]
    # a threat that itself runs out of budget or depth: nothing is searched, every empty cell is UNKNOWN
    for limits, status in (((8, 4), R.BUDGET), ((1, 1000), R.DEPTH)):
        d = DR.defend(moves, *limits)
        assert d["threat"]["status"] == status and d["searched"] == [] and not any(d["nodes"])
        assert DR.cells_with(d, DR.CELL_UNKNOWN) == empties(moves)
    roomy = DR.defend(moves, 8, 1000)
    assert not DR.cells_with(roomy, DR.CELL_UNKNOWN)
    assert all(roomy["verdict"][c] == v for c, v in enumerate(DR.defend(moves, 8, 6)["verdict"]) if v != DR.CELL_UNKNOWN)      # more budget changes no verdict but UNKNOWN


def test_follow_and_the_none_rule_are_sound():
    """On 6 threatened and 3 quiet random positions every verdict that is not UNKNOWN equals that of a full solve of P + [c] at an unbounded
    budget, with no follow and no rule for NONE: the shortcuts change the cost, not the answer."""
    rng = random.Random(9)
    threatened = quiet = 0
    while threatened < 6 or quiet < 3:
        moves = R.random_position(rng, *rng.choice(((16, 3), (24, 3), (30, 4), (40, 4))))
        if moves is None:
            continue
        d = DR.defend(moves, 6, 3000)
        status = d["threat"]["status"]
        if status == R.WIN and threatened < 6:
            threatened += 1
        elif status == R.NONE and quiet < 3:
            quiet += 1
        else:
            continue
        board = R.board_of(moves)
        fives = R.completing(board, 1 + (len(moves) & 1))
        for c in range(225):
            verdict = d["verdict"][c]
            if board[c]:
                assert verdict == DR.CELL_NONE
            elif c in fives:
                assert verdict == DR.CELL_FIVE
            elif verdict != DR.CELL_UNKNOWN:
                s = R.solve(moves + [c], 6, 10 ** 9)
                want = {R.WIN: DR.CELL_LOSES, R.NONE: DR.CELL_HOLDS, R.DEPTH: DR.CELL_UNKNOWN}[s["status"]]
                assert verdict == want, (moves, c, verdict, s)
                if verdict == DR.CELL_LOSES and c not in d["searched"]:
                    assert s["length"] <= 6 and d["length"][c] >= 1
