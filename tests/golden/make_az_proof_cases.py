"""Writes tests/golden/az_proof_cases.json: nearly full boards (at most 6 empty cells, no five on them, fives possible) for the soundness test
of tests/test_az_proof_reference.py, which searches them with tests/az_proof_reference.ProofSearch and holds every proof bit against a full
minimax.  Run on the CPU, once:  python tests/golden/make_az_proof_cases.py

A board starts from a colouring without a run of three in any direction, black where ((x + 2 y) // 2) is even.  A random segment of six or
seven cells on a line gets 4 .. 6 empties and one colour on the rest, further cells are flipped (never completing a five) until the stone
counts are those of a game with black to move first, and the position is kept when its searches show what the test must see: a node proven
LOSES by exhaustion, a proof chain of three levels, a root whose choice differs from the most visited child."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import az_leaves_reference as R      # noqa: E402
import az_proof_reference as P       # noqa: E402

N = 225
PLAYOUTS, C_PUCT = 240, 5.0          # the test's settings
SETTINGS = [(1, 0), (4, 0), (1, 8), (4, 8)]      # (leaves, vcf_depth)


def any_five(colour):
    return any(colour[c] and R._five_through(colour, c) for c in range(N))


def make_position(rng):
    board = np.array([1 if ((c % 15 + 2 * (c // 15)) // 2) % 2 == 0 else 2 for c in range(N)])      # 1 black, 2 white
    dx, dy = ((1, 0), (0, 1), (1, 1), (1, -1))[rng.integers(4)]
    length = int(rng.integers(6, 8))
    x0, y0 = int(rng.integers(0, 15)), int(rng.integers(0, 15))
    cells = [(x0 + i * dx, y0 + i * dy) for i in range(length)]
    if not all(0 <= x < 15 and 0 <= y < 15 for x, y in cells):
        return None
    cells = [y * 15 + x for x, y in cells]
    n_empty = int(rng.integers(4, 7))
    empties = list(rng.choice(cells, size=min(n_empty, len(cells) - 1), replace=False))
    colour = int(rng.integers(1, 3))
    for c in cells:
        board[c] = 0 if c in empties else colour
    for c in rng.choice(N, size=int(rng.integers(0, 3)), replace=False):      # a few more empties elsewhere
        if len(empties) < 6 and board[c] != 0:
            board[c] = 0
            empties.append(int(c))
    stones = N - len(empties)
    want_black = (stones + 1) // 2
    for _ in range(400):
        diff = int((board == 1).sum()) - want_black
        if diff == 0:
            break
        c = int(rng.integers(N))
        if board[c] == (1 if diff > 0 else 2):
            board[c] = 3 - board[c]
            if R._five_through(board == board[c], c):
                board[c] = 3 - board[c]
    if int((board == 1).sum()) != want_black or any_five(board == 1) or any_five(board == 2):
        return None
    black, white = [c for c in range(N) if board[c] == 1], [c for c in range(N) if board[c] == 2]
    moves = []
    for i in range(stones):
        moves.append(black[i // 2] if i % 2 == 0 else white[i // 2])
    return [int(c) for c in moves]


def facts(moves):
    """what the searches of this position show, over the test's settings"""
    out = {"exhaustion": False, "chain": False, "choice": False, "bits": 0}
    for leaves, depth in SETTINGS:
        s = P.ProofSearch(moves, R.uniform, depth, 64, proof=True, c_puct=C_PUCT, leaves=leaves)
        s.search(PLAYOUTS)
        for i in range(s.n_nodes):
            if s.proof[i] == P.NONE:
                continue
            out["bits"] += 1
            if s.proof[i] == P.LOSES and s.nkids[i]:
                out["exhaustion"] = True
            p = s.parent[i]
            if p != P.NO_NODE and s.proof[p] != P.NONE and s.parent[p] != P.NO_NODE and s.proof[s.parent[p]] != P.NONE:
                out["chain"] = True
        if s.choice() != s.plain_choice():
            out["choice"] = True
    return out


def main():
    rng = np.random.default_rng(20260118)
    cases, seen = [], {"exhaustion": 0, "chain": 0, "choice": 0}
    tries = 0
    while (min(seen.values()) < 2 or len(cases) < 6) and tries < 4000 and len(cases) < 10:
        tries += 1
        moves = make_position(rng)
        if moves is None:
            continue
        f = facts(moves)
        if f["bits"] == 0:
            continue
        new = [k for k in seen if f[k] and seen[k] < 2]
        if not new and len(cases) >= 4:
            continue
        for k in seen:
            seen[k] += bool(f[k])
        cases.append({"moves": moves, "empty": N - len(moves), "minimax": P.minimax(moves), **{k: bool(f[k]) for k in ("exhaustion", "chain", "choice")}})
        print(tries, cases[-1]["empty"], cases[-1]["minimax"], f, flush=True)
    with open(os.path.join(HERE, "az_proof_cases.json"), "w") as fh:
        json.dump({"playouts": PLAYOUTS, "c_puct": C_PUCT, "settings": SETTINGS, "cases": cases}, fh)
    print(len(cases), "cases,", seen)


if __name__ == "__main__":
    main()
