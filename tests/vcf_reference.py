"""A plain-Python restatement of the forced-win solver's contract (include/gomoku_hip.h, "K14"): victory by continuous fours.

Independent of the kernel's method on purpose: the board is a list of 225 cells, runs are counted cell by cell, candidates are tried one empty
cell after the other.  It imports nothing from the package and nothing from the oracle."""

SIZE = 15
CELLS = SIZE * SIZE
NONE, WIN, DEPTH, BUDGET, OVER, BAD = 0, 1, 2, 3, 4, 5
STATUS_NAMES = ["NONE", "WIN", "DEPTH", "BUDGET", "OVER", "BAD"]
PV = 64
DIRECTIONS = ((1, 0), (0, 1), (1, 1), (1, -1))


def _ray(cell, dx, dy):
    x, y = cell % SIZE + dx, cell // SIZE + dy
    out = []
    while 0 <= x < SIZE and 0 <= y < SIZE and len(out) < 4:      # four stones on one side already make five with the cell
        out.append(y * SIZE + x)
        x, y = x + dx, y + dy
    return tuple(out)


# RAYS[cell] = for each direction the (up to four) cells ahead and the cells behind, nearest first; rays stop at the board's edge
RAYS = [tuple((_ray(c, dx, dy), _ray(c, -dx, -dy)) for dx, dy in DIRECTIONS) for c in range(CELLS)]


def run_along(board, cell, colour, ahead, behind):
    """The run of `colour` through `cell` along one line, counting the cell itself as `colour` (capped at nine)."""
    length = 1
    for ray in (ahead, behind):
        for e in ray:
            if board[e] != colour:
                break
            length += 1
    return length


def run_through(board, cell, colour):
    """The longest such run over the four directions."""
    return max(run_along(board, cell, colour, ahead, behind) for ahead, behind in RAYS[cell])


def completing(board, colour):
    """Ascending list of the empty cells where a stone of `colour` makes five or more."""
    out = []
    for c in range(CELLS):
        if board[c]:
            continue
        for ahead, behind in RAYS[c]:                             # run_through(board, c, colour) >= 5, written out: this is the hot loop
            stones = 0
            for e in ahead:
                if board[e] != colour:
                    break
                stones += 1
            for e in behind:
                if board[e] != colour:
                    break
                stones += 1
            if stones >= 4:
                out.append(c)
                break
    return out


def fours_after(board, c, colour):
    """completing(colour) with c played, for a board on which completing(colour) is empty: every such cell is new, so it lies on a line
    through c, at most four steps away, and its five runs along that line.  (Only a shortcut for speed: the cells are judged by counting.)"""
    board[c] = colour
    found = set()
    for d, (ahead, behind) in enumerate(RAYS[c]):
        if sum(board[e] == colour for e in ahead) + sum(board[e] == colour for e in behind) < 3:
            continue
        for e in ahead + behind:
            if board[e] == 0 and run_along(board, e, colour, *RAYS[e][d]) >= 5:
                found.add(e)
    board[c] = 0
    return sorted(found)


def has_five(board, colour):
    return any(board[c] == colour and run_through(board, c, colour) >= 5 for c in range(CELLS))


def board_of(moves):
    """moves -> (board with 1 = black, 2 = white, 0 = empty) or None when the list is no position."""
    if len(moves) > CELLS:
        return None
    board = [0] * CELLS
    for i, c in enumerate(moves):
        if not 0 <= c < CELLS or board[c]:
            return None
        board[c] = 1 + (i & 1)
    return board


class _Stop(Exception):
    pass


def solve(moves, max_depth=16, budget=100000, opponent=False, iterative=False):
    """-> {"status", "move", "length", "nodes", "pv"}; pv is the list of cells (no padding)."""
    assert 1 <= max_depth <= 32
    result = {"status": BAD, "move": -1, "length": 0, "nodes": 0, "pv": []}
    board = board_of(list(moves))
    if board is None:
        return result
    if has_five(board, 1) or has_five(board, 2):
        result["status"] = OVER
        return result
    attacker = 1 + (len(moves) & 1)
    if opponent:
        attacker = 3 - attacker
    defender = 3 - attacker
    state = {"nodes": 0, "cut": False}

    def attack(depth, limit):
        won = completing(board, attacker)
        if won:
            return [won[0]]
        threats = completing(board, defender)
        if len(threats) >= 2:
            return None
        if depth + 2 > limit:
            state["cut"] = True
            return None
        for c in (threats if threats else [e for e in range(CELLS) if board[e] == 0]):
            fours = fours_after(board, c, attacker)       # completing(attacker) is empty here, or the walk had returned above
            if not fours:
                continue
            if state["nodes"] == budget:
                raise _Stop
            state["nodes"] += 1
            if len(fours) >= 2:
                return [c, fours[0], fours[1]]
            r = fours[0]
            board[c] = attacker
            board[r] = defender
            rest = attack(depth + 1, limit)
            board[c] = board[r] = 0
            if rest is not None:
                return [c, r] + rest
        return None

    pv = None
    try:
        for limit in (range(1, max_depth + 1) if iterative else [max_depth]):
            state["cut"] = False
            pv = attack(0, limit)
            if pv is not None or not state["cut"]:
                break
    except _Stop:
        result.update(status=BUDGET, nodes=state["nodes"])
        return result
    result["nodes"] = state["nodes"]
    if pv is not None:
        result.update(status=WIN, move=pv[0], length=(len(pv) + 1) // 2, pv=pv)
    else:
        result["status"] = DEPTH if state["cut"] else NONE
    return result


def check_pv(moves, result, opponent=False):
    """Replays a WIN's pv: every attacker move but the last leaves completing(attacker) non-empty, every defender move lies in that set, the
    last move makes five."""
    assert result["status"] == WIN
    pv = result["pv"]
    assert len(pv) == 2 * result["length"] - 1 and result["move"] == pv[0]
    board = board_of(list(moves))
    attacker = 1 + (len(moves) & 1)
    if opponent:
        attacker = 3 - attacker
    for i, c in enumerate(pv):
        assert board[c] == 0
        if i == len(pv) - 1:
            assert i % 2 == 0 and run_through(board, c, attacker) >= 5
        elif i % 2 == 0:
            board[c] = attacker
            assert completing(board, attacker)
        else:
            assert c in completing(board, attacker)
            board[c] = 3 - attacker
    return True


def random_position(rng, plies, spread):
    """`plies` distinct cells drawn uniformly from the square of half-width `spread` around the centre; None unless neither colour has a five
    and neither has a completing cell."""
    square = [y * SIZE + x for y in range(7 - spread, 8 + spread) for x in range(7 - spread, 8 + spread)]
    moves = rng.sample(square, plies)
    board = board_of(moves)
    if has_five(board, 1) or has_five(board, 2) or completing(board, 1) or completing(board, 2):
        return None
    return moves
