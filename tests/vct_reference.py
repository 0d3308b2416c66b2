"""A plain-Python restatement of the two contracts of include/gomoku_hip.h, "K17": what a stone of the side to move threatens on every cell
(threats), and the forced win by continuous threats, fours and threes (vct_solve).  Both stand on the restatements below them
(tests/vcf_reference.py: solve and completing; tests/vcf_defend_reference.py: defend) and are written level by level, list by list, as the
contract words them.  It imports nothing from the package and nothing from the oracle.  It is slow: a threats call is most of a second, a
search of some forty positions several seconds."""
import vcf_defend_reference as DR
import vcf_reference as R

CELLS = R.CELLS
THREAT_NONE, THREAT_QUIET, THREAT_WINS, THREAT_UNKNOWN, THREAT_FIVE, THREAT_FOUR, THREAT_IGNORES = 0, 1, 2, 3, 4, 5, 6
THREAT_NAMES = ["NONE", "QUIET", "WINS", "UNKNOWN", "FIVE", "FOUR", "IGNORES"]
VCT_BUDGET = 6                                                  # the statuses are R's, and this one: a level above max_positions
STATUS_NAMES = R.STATUS_NAMES + ["VCT_BUDGET"]
MAX_THREATS, PV = 8, 80


def threats(moves, max_depth=16, budget=100000, iterative=False):
    """-> {"own": solve(moves), "verdict": [225], "length": [225], "nodes": [225]}"""
    moves = list(moves)
    own = R.solve(moves, max_depth, budget, iterative=iterative)
    out = {"own": own, "verdict": [THREAT_NONE] * CELLS, "length": [0] * CELLS, "nodes": [0] * CELLS}
    if own["status"] in (R.OVER, R.BAD):
        return out
    board = R.board_of(moves)
    attacker = 1 + (len(moves) & 1)
    fives = R.completing(board, attacker)
    for c in range(CELLS):
        if board[c]:
            continue
        if c in fives:
            out["verdict"][c] = THREAT_FIVE
            continue
        board[c] = attacker
        answer, fours = R.completing(board, 3 - attacker), R.completing(board, attacker)
        board[c] = 0
        if answer:
            out["verdict"][c] = THREAT_IGNORES
        elif fours:
            out["verdict"][c], out["length"][c] = THREAT_FOUR, 1 if len(fours) == 1 else 2
        else:
            s = R.solve(moves + [c], max_depth, budget, opponent=True, iterative=iterative)
            out["nodes"][c] = s["nodes"]
            if s["status"] == R.WIN:
                out["verdict"][c], out["length"][c] = THREAT_WINS, s["length"]
            elif s["status"] == R.NONE:
                out["verdict"][c] = THREAT_QUIET
            else:
                assert s["status"] in (R.DEPTH, R.BUDGET)
                out["verdict"][c] = THREAT_UNKNOWN
    return out


def cells_with(result, verdict):
    return [c for c in range(CELLS) if result["verdict"][c] == verdict]


def vct_solve(moves, max_depth=16, budget=100000, iterative=False, max_threats=1, max_positions=1 << 20):
    """-> {"status", "move", "threats", "positions", "pv", "levels": the sizes of the levels that were solved}"""
    assert 1 <= max_threats <= MAX_THREATS and max_positions >= 1
    result = {"status": R.NONE, "move": -1, "threats": 0, "positions": 1, "pv": [], "levels": [1]}
    # a position of the tree: its list, its own solve, its candidates [(c, [children])] and, once it is proven, its depth
    root = {"moves": list(moves), "own": None, "candidates": [], "depth": None}
    levels = [[root]]
    cut = False
    for t in range(max_threats + 1):
        level = levels[t]
        for q in level:
            q["own"] = R.solve(q["moves"], max_depth, budget, iterative=iterative)
            if q["own"]["status"] == R.WIN:
                q["depth"] = 0
            elif q["own"]["status"] in (R.DEPTH, R.BUDGET):
                cut = True
        if root["own"]["status"] in (R.OVER, R.BAD):
            result["status"] = root["own"]["status"]
            return result
        for above in reversed(levels[:t]):                         # bottom-up: a candidate is proven once every child has a depth
            for q in above:
                if q["own"]["status"] == R.WIN:
                    continue
                proven = [1 + max([k["depth"] for k in kids], default=0) for _, kids in q["candidates"] if all(k["depth"] is not None for k in kids)]
                q["depth"] = min(proven) if proven else None
        if root["depth"] is not None:
            result.update(status=R.WIN, move=_move(root), threats=root["depth"], pv=_line(root))
            return result
        if t == max_threats:
            cut = cut or any(q["depth"] is None for q in level)   # level T is never expanded
            break
        following = []
        for q in level:
            if q["depth"] == 0:
                continue
            th = threats(q["moves"], max_depth, budget, iterative)
            for c in range(CELLS):
                if th["verdict"][c] == THREAT_UNKNOWN:
                    cut = True
                if th["verdict"][c] not in (THREAT_WINS, THREAT_FOUR):
                    continue
                d = DR.defend(q["moves"] + [c], max_depth, budget, iterative)
                if DR.CELL_UNKNOWN in d["verdict"]:
                    cut = True
                    continue
                if DR.CELL_FIVE in d["verdict"]:
                    continue
                kids = [{"moves": q["moves"] + [c, r], "own": None, "candidates": [], "depth": None} for r in DR.cells_with(d, DR.CELL_HOLDS)]
                q["candidates"].append((c, kids))
                following += kids
        if len(following) > max_positions:
            result["status"] = VCT_BUDGET
            return result
        levels.append(following)
        result["levels"].append(len(following))
        result["positions"] += len(following)
    result["status"] = R.DEPTH if cut else R.NONE
    return result


def _best(q):
    """the lowest candidate of minimal depth and its children"""
    for c, kids in q["candidates"]:
        if all(k["depth"] is not None for k in kids) and 1 + max([k["depth"] for k in kids], default=0) == q["depth"]:
            return c, kids
    raise AssertionError("a proven position has a proven candidate")


def _move(q):
    return q["own"]["move"] if q["depth"] == 0 else _best(q)[0]


def _line(q):
    if q["depth"] == 0:
        return list(q["own"]["pv"])
    c, kids = _best(q)
    if not kids:
        return [c]
    deepest = max(k["depth"] for k in kids)
    k = next(k for k in kids if k["depth"] == deepest)            # children are in ascending order of the reply
    return [c, k["moves"][-1]] + _line(k)


def check_line(moves, result, max_depth=16, budget=100000, iterative=False):
    """Replays a WIN's pv: every attacker move of the threat part but a closing lone one leaves a win by fours for the attacker if the defender
    passes, every defender move of that part HOLDS, and the rest is the own line of the leaf."""
    assert result["status"] == R.WIN and result["move"] == result["pv"][0]
    q, pv = list(moves), list(result["pv"])
    for _ in range(result["threats"]):
        c = pv.pop(0)
        assert R.solve(q + [c], max_depth, budget, opponent=True, iterative=iterative)["status"] == R.WIN
        d = DR.defend(q + [c], max_depth, budget, iterative)
        if not pv:
            assert not DR.cells_with(d, DR.CELL_HOLDS) and DR.CELL_UNKNOWN not in d["verdict"]
            return True
        r = pv.pop(0)
        assert d["verdict"][r] == DR.CELL_HOLDS
        q += [c, r]
    own = R.solve(q, max_depth, budget, iterative=iterative)
    assert own["status"] == R.WIN and own["pv"] == pv
    return True
