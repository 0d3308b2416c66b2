"""The restatement of the two K17 contracts (tests/vct_reference.py; include/gomoku_hip.h, "K17"), held to positions checked by hand, to the
soundness of every line it reports, and to the results committed in tests/golden/vct_cases.json, which the GPU tests compare the kernels
with.  CPU only.  The restatement is slow, so every search here is made once."""
import functools
import json
import os

import vcf_defend_reference as DR
import vcf_reference as R
import vct_reference as V

HERE = os.path.dirname(os.path.abspath(__file__))


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


CORNERS = [cell(0, 0), cell(14, 0), cell(0, 14), cell(14, 14)]
FAR = [cell(0, 14), cell(14, 12), cell(14, 9), cell(0, 10), cell(12, 0)]        # no two of them on a line within four steps, and off the lines used
DOUBLE_THREE = interleave([cell(6, 7), cell(7, 7), cell(8, 5), cell(8, 6)], CORNERS)                  # black to move; (8, 7) makes two open threes
OPEN_TWO = [cell(6, 7), cell(0, 0), cell(7, 7), cell(14, 0)]
# black to move: (7, 7) makes a four on row 7, closed by white on (3, 7), and an open three on column 7
FOUR_THREE = interleave([cell(4, 7), cell(5, 7), cell(6, 7), cell(7, 5), cell(7, 6)], [cell(3, 7)] + FAR[:4])
# black to move against white's four on (1, 0) .. (4, 0), closed by black on (5, 0): only (0, 0) does not ignore it
WHITE_FOUR = interleave([cell(5, 0), FAR[0], FAR[1], FAR[2]], [cell(1, 0), cell(2, 0), cell(3, 0), cell(4, 0)])


@functools.lru_cache(maxsize=None)
def cases():
    """tests/golden/vct_cases.json, the threat cells unpacked into lists of 225 (make_vct_cases.packed)"""
    def unpacked(p):
        if isinstance(p, str):
            return [int(v) for v in p]
        out = [0] * 225
        for c, v in zip(p[0::2], p[1::2]):
            out[c] = v
        return out
    with open(os.path.join(HERE, "golden", "vct_cases.json")) as f:
        data = json.load(f)
    for rows in list(data["threats"].values()) + [data["borders"]["threats"]]:
        for t in rows:
            t.update({k: unpacked(t[k]) for k in ("verdict", "length", "nodes")})
    return data


@functools.lru_cache(maxsize=None)
def search(name, max_threats, max_positions=1 << 20):
    return V.vct_solve({"double_three": DOUBLE_THREE, "open_two": OPEN_TWO}[name], max_threats=max_threats, max_positions=max_positions)


def test_double_three():
    """K14 sees nothing; every stone that makes an open three threatens, and the one that makes two of them wins: no reply holds."""
    t = V.threats(DOUBLE_THREE)
    assert t["own"]["status"] == R.NONE
    wins = V.cells_with(t, V.THREAT_WINS)
    assert len(wins) == 18 and cell(8, 7) in wins and not V.cells_with(t, V.THREAT_FOUR) and not V.cells_with(t, V.THREAT_UNKNOWN)
    assert all(2 <= t["length"][c] <= 4 and t["nodes"][c] > 0 for c in wins)           # the three becomes an open four, on the walk's first line
    assert (t["length"][113], t["nodes"][113]) == (3, 15)                              # (8, 3) first, a four with one end, then the other three
    assert V.cells_with(t, V.THREAT_NONE) == sorted(DOUBLE_THREE) and len(V.cells_with(t, V.THREAT_QUIET)) == 225 - 8 - 18
    for max_threats in (1, 2):
        r = search("double_three", max_threats)
        assert (r["status"], r["move"], r["threats"], r["positions"], r["pv"]) == (R.WIN, 113, 1, 47, [113]), (max_threats, r)
        assert r["levels"] == [1, 46]
        assert V.check_line(DOUBLE_THREE, r)


def test_open_two():
    """It has no win: every threat is answered.  Level T is cut, so the answer is DEPTH."""
    for max_threats, levels in ((1, [1, 10]), (2, [1, 10, 28])):
        r = search("open_two", max_threats)
        assert r["levels"] == levels and r["positions"] == sum(levels)
        assert (r["status"], r["move"], r["threats"], r["pv"]) == (R.DEPTH, -1, 0, [])


def test_max_positions():
    """Level 1 of the open two has 10 positions: a cap of 9 ends the root, of 10 does not; the discarded level is not counted."""
    r = V.vct_solve(OPEN_TWO, max_threats=1, max_positions=9)
    assert (r["status"], r["move"], r["threats"], r["positions"], r["pv"]) == (V.VCT_BUDGET, -1, 0, 1, [])
    assert search("open_two", 1, 10)["status"] == R.DEPTH and search("open_two", 1, 10)["positions"] == 11


def test_four_three():
    """A four-three is K14's own: the root is won at depth 0 and the line is K14's.  Whoever wins by fours still does after a stone elsewhere,
    so every other empty cell WINS; the two cells of the four are FOUR with one completing cell."""
    own = R.solve(FOUR_THREE)
    assert (own["status"], own["move"], own["length"]) == (R.WIN, cell(7, 7), 3)
    r = V.vct_solve(FOUR_THREE, max_threats=2)
    assert (r["status"], r["move"], r["threats"], r["positions"], r["pv"]) == (R.WIN, own["move"], 0, 1, own["pv"])
    assert V.check_line(FOUR_THREE, r)
    t = V.threats(FOUR_THREE)
    assert t["own"] == own
    assert V.cells_with(t, V.THREAT_FOUR) == [cell(7, 7), cell(8, 7)] and [t["length"][c] for c in (112, 113)] == [1, 1] and [t["nodes"][c] for c in (112, 113)] == [0, 0]
    assert len(V.cells_with(t, V.THREAT_WINS)) == 225 - len(FOUR_THREE) - 2 and not V.cells_with(t, V.THREAT_QUIET)


def test_a_four_of_the_defender_is_ignored():
    t = V.threats(WHITE_FOUR)
    assert (t["own"]["status"], t["own"]["nodes"]) == (R.NONE, 0)
    assert V.cells_with(t, V.THREAT_IGNORES) == [c for c in range(1, 225) if c not in WHITE_FOUR]
    assert t["verdict"][0] == V.THREAT_QUIET and not any(t["length"]) and not any(t["nodes"])
    r = V.vct_solve(WHITE_FOUR, max_threats=2)
    assert (r["status"], r["positions"]) == (R.NONE, 1)                                 # no candidate, nothing cut


def test_fives_fours_and_the_order_of_the_table():
    """Black 110 .. 113 with white on 109: 114 is FIVE.  White to move after black's far stone: white's own open three gives FOUR cells, but
    only where the stone also takes 114; everywhere else black makes five next: IGNORES."""
    black_to_move = interleave([110, 111, 112, 113], [109, FAR[1], FAR[2], FAR[3]])
    t = V.threats(black_to_move)
    assert (t["own"]["status"], t["own"]["move"]) == (R.WIN, 114)
    assert V.cells_with(t, V.THREAT_FIVE) == [114] and t["length"][114] == 0
    assert V.cells_with(t, V.THREAT_FOUR) == [c for c in range(225) if c not in black_to_move and c != 114]       # the four stays a four
    assert all(t["length"][c] == 1 for c in V.cells_with(t, V.THREAT_FOUR))
    white_to_move = black_to_move + [FAR[0]]
    t = V.threats(white_to_move)
    assert t["own"]["status"] == R.NONE
    assert V.cells_with(t, V.THREAT_IGNORES) == [c for c in range(225) if c not in white_to_move and c != 114]
    assert t["verdict"][114] == V.THREAT_QUIET
    # two completing cells: an open four
    t = V.threats(interleave([110, 111, 112, FAR[0]], [FAR[4], FAR[1], FAR[2], FAR[3]]))
    assert [t["length"][c] for c in (109, 113)] == [2, 2] and [t["verdict"][c] for c in (109, 113)] == [V.THREAT_FOUR] * 2
    assert [t["length"][c] for c in (108, 114)] == [1, 1]


def test_over_and_bad_lists():
    over = interleave([cell(x, 7) for x in range(2, 7)], FAR[:4])
    for moves, status in ((over, R.OVER), ([3, 3], R.BAD), ([225], R.BAD), (list(range(225)) + [0], R.BAD)):
        t = V.threats(moves, 8, 1000)
        assert t["own"]["status"] == status and t["verdict"] == [V.THREAT_NONE] * 225 and not any(t["length"]) and not any(t["nodes"])
        r = V.vct_solve(moves, 8, 1000, max_threats=2)
        assert (r["status"], r["move"], r["threats"], r["positions"], r["pv"]) == (status, -1, 0, 1, [])


def test_a_counter_four_costs_a_threat_move():
    """The double three with a white three on row 12, closed on one side: white answers (8, 7) with a four on (5, 12) or (6, 12), which holds,
    since the block is no four of black's.  Black blocks -- a second threat move, for the double three still stands -- and then nothing holds.
    The searches are committed (tests/golden/make_vct_cases.py: level 1 has dozens of positions); here the line is replayed."""
    from golden.make_vct_cases import COUNTER_FOUR
    assert len(COUNTER_FOUR) % 2 == 0 and R.solve(COUNTER_FOUR)["status"] == R.NONE
    one, two = cases()["hand"]["counter_four_1"], cases()["hand"]["counter_four_2"]
    assert (one[0], one[1], one[2], one[4]) == (R.DEPTH, -1, 0, [])
    assert (two[0], two[1], two[2], two[4]) == (R.WIN, 113, 2, [113, cell(5, 12), cell(6, 12)])
    assert one[5] == two[5][:2] and two[3] == sum(two[5]) and one[3] == sum(one[5])
    assert V.check_line(COUNTER_FOUR, {"status": two[0], "move": two[1], "threats": two[2], "pv": two[4]})


# ---------------- the committed cases ----------------
def limits(run):
    max_depth, budget, iterative = cases()["runs"][run]
    return max_depth, budget, bool(iterative)


def test_the_committed_cases_cover_the_contract():
    """Every verdict but FIVE and IGNORES occurs in the random set (its positions have no completing cell; the hand positions above have both),
    UNKNOWN and searched cells among them; the searches end in WIN, DEPTH, NONE and VCT_BUDGET, with wins at depth 0 and 1 in the random set
    and at depth 2 in the hand search; the border searches are there for all ten positions at T = 1 and 2."""
    data = cases()
    verdicts, statuses, depths = set(), set(), set()
    for rows in data["threats"].values():
        for t in rows:
            verdicts |= set(t["verdict"])
    assert verdicts == {V.THREAT_NONE, V.THREAT_QUIET, V.THREAT_WINS, V.THREAT_UNKNOWN, V.THREAT_FOUR}, verdicts
    for s in data["searches"]:
        for status, move, threats, positions, pv in s["results"]:
            statuses.add(status)
            if status == R.WIN:
                depths.add(threats)
    assert statuses == {R.NONE, R.WIN, R.DEPTH, V.VCT_BUDGET}, statuses
    assert depths == {0, 1} and data["hand"]["counter_four_2"][:3] == [R.WIN, 113, 2], depths
    assert [(s["max_threats"], len(s["results"])) for s in data["borders"]["searches"]] == [(1, 10), (2, 10)]


def test_every_committed_win_replays():
    """Soundness: each attacker move of a line but a closing lone one leaves a K14 win if the defender passes, each defender move HOLDS, and
    the rest is the leaf's own line."""
    data = cases()
    wins = 0
    for s in data["searches"]:
        for q, (status, move, threats, positions, pv) in zip(data["positions"], s["results"]):
            if status == R.WIN:
                wins += 1
                assert V.check_line(q, {"status": status, "move": move, "threats": threats, "pv": pv}, *limits(s["run"])), (s, q)
    assert wins >= 5


def test_a_sample_of_the_committed_cases_is_recomputed():
    data = cases()
    for k, (run, rows) in enumerate(data["threats"].items()):
        for i in range(5 * k, len(rows), 17):
            t, want = V.threats(data["positions"][i], *limits(run)), rows[i]
            own = t["own"]
            assert [own["status"], own["move"], own["length"], own["nodes"], own["pv"]] == want["own"], (run, i)
            assert (t["verdict"], t["length"], t["nodes"]) == (want["verdict"], want["length"], want["nodes"]), (run, i)
    i = 7                                                      # and one border position
    t, want = V.threats(data["borders"]["positions"][i], *data["borders"]["limits"][:2]), data["borders"]["threats"][i]
    assert (t["own"]["status"], t["verdict"], t["length"], t["nodes"]) == (want["own"][0], want["verdict"], want["length"], want["nodes"])
    for k, s in enumerate(data["searches"]):
        if s["max_threats"] != 1:
            continue
        for i in (2 * k,):                                         # one root of each search at T = 1: a search is several seconds
            r = V.vct_solve(data["positions"][i], *limits(s["run"]), max_threats=1, max_positions=s["max_positions"])
            assert [r["status"], r["move"], r["threats"], r["positions"], r["pv"]] == s["results"][i], (s["run"], i)
