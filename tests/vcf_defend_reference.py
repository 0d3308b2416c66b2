"""A plain-Python restatement of the contract of the defence against a forced win by continuous fours (include/gomoku_hip.h, "K15"), on top
of the restatement of the solver's (tests/vcf_reference.py: solve and completing).  `follow` is written out cell by cell.  It imports nothing
from the package and nothing from the oracle."""
import vcf_reference as R

CELLS = R.CELLS
CELL_NONE, CELL_HOLDS, CELL_LOSES, CELL_UNKNOWN, CELL_FIVE = 0, 1, 2, 3, 4
CELL_NAMES = ["NONE", "HOLDS", "LOSES", "UNKNOWN", "FIVE"]
FAIL = None


def follow(board, attacker, pv):
    """The walk of attack with exactly one candidate per level, pv's attacker move of that level, on `board` (P with the defender's stone on c
    already placed; changed and restored) -> the losing length, or FAIL."""
    defender = 3 - attacker
    played = []
    i = 0
    try:
        while True:
            if R.completing(board, attacker):
                return i + 1
            threats = R.completing(board, defender)
            if len(threats) >= 2:
                return FAIL
            if 2 * i >= len(pv):
                return FAIL
            a = pv[2 * i]
            if board[a] or (threats and a not in threats):
                return FAIL
            board[a] = attacker
            played.append(a)
            fours = R.completing(board, attacker)
            if not fours:
                return FAIL
            if len(fours) >= 2:
                return i + 2
            board[fours[0]] = defender
            played.append(fours[0])
            i += 1
    finally:
        for e in played:
            board[e] = 0


def defend(moves, max_depth=16, budget=100000, iterative=False):
    """-> {"threat": solve(moves, opponent=True), "verdict": [225], "length": [225], "nodes": [225], "searched": the cells that were solved}"""
    moves = list(moves)
    threat = R.solve(moves, max_depth, budget, opponent=True, iterative=iterative)
    out = {"threat": threat, "verdict": [CELL_NONE] * CELLS, "length": [0] * CELLS, "nodes": [0] * CELLS, "searched": []}
    if threat["status"] in (R.OVER, R.BAD):
        return out
    board = R.board_of(moves)
    defender = 1 + (len(moves) & 1)
    attacker = 3 - defender
    fives = R.completing(board, defender)
    for c in range(CELLS):
        if board[c]:
            continue
        if c in fives:
            out["verdict"][c] = CELL_FIVE
        elif threat["status"] == R.NONE:
            out["verdict"][c] = CELL_HOLDS
        elif threat["status"] in (R.DEPTH, R.BUDGET):
            out["verdict"][c] = CELL_UNKNOWN
        else:
            board[c] = defender
            length = follow(board, attacker, threat["pv"])
            board[c] = 0
            if length is not FAIL:
                out["verdict"][c], out["length"][c] = CELL_LOSES, length
                continue
            s = R.solve(moves + [c], max_depth, budget, iterative=iterative)
            out["searched"].append(c)
            out["nodes"][c] = s["nodes"]
            if s["status"] == R.WIN:
                out["verdict"][c], out["length"][c] = CELL_LOSES, s["length"]
            elif s["status"] == R.NONE:
                out["verdict"][c] = CELL_HOLDS
            else:
                assert s["status"] in (R.DEPTH, R.BUDGET)
                out["verdict"][c] = CELL_UNKNOWN
    return out


def cells_with(result, verdict):
    return [c for c in range(CELLS) if result["verdict"][c] == verdict]
