"""Writes tests/golden/vct_cases.json: the results of the plain-Python restatement (tests/vct_reference.py) on a fixed random set, which the
GPU tests compare the kernels with and tests/test_vct_reference.py recomputes a sample of.  The restatement is slow (a quarter of an hour on eight
processes, most of it the counter-four search over two levels), so its results are made once and committed as data.

    python tests/golden/make_vct_cases.py
"""
import json
import multiprocessing
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vcf_reference as R            # noqa: E402
import vct_reference as V            # noqa: E402

# (max_depth, budget, iterative)
RUNS = {"deep": (8, 2000, False), "shallow": (3, 8, False), "deep_iterative": (8, 2000, True)}
# (run, max_threats, max_positions)
SEARCHES = [("deep", 1, 64), ("shallow", 1, 64), ("deep", 2, 24), ("shallow", 2, 24), ("deep_iterative", 1, 40)]
THREAT_POSITIONS, ROOTS = 40, 24


def cell(x, y):
    return y * 15 + x


# Hand positions that are too slow to search anew in a test, at K14's defaults (16, 100000): (moves, max_threats).
# counter_four: black's double three on (8, 7) with a white three on row 12, closed by black on (1, 12).  White answers the double three with
# a four on (5, 12) or (6, 12), which holds; black spends a second threat move on the block, and then nothing holds.
COUNTER_FOUR = [cell(6, 7), cell(2, 12), cell(7, 7), cell(3, 12), cell(8, 5), cell(4, 12), cell(8, 6), cell(14, 0), cell(1, 12), cell(14, 14)]
HAND = {"counter_four_1": (COUNTER_FOUR, 1), "counter_four_2": (COUNTER_FOUR, 2)}


# Both colours along all four borders and into the corners: the side to move has two stones on a line there (the third makes the three), black
# on the even lines and white on the odd ones; the other colour's stones are scattered in the middle.  Searched at (4, 100).
BORDER_LINES = [[cell(x, 0) for x in (5, 6)], [cell(x, 14) for x in (9, 10)], [cell(0, y) for y in (5, 6)], [cell(14, y) for y in (1, 2)],
                [cell(x, 0) for x in (1, 2)], [cell(x, 14) for x in (11, 12)], [cell(i, i) for i in (1, 2)], [cell(i, i) for i in (11, 12)],
                [cell(14 - i, i) for i in (1, 2)], [cell(i, 14 - i) for i in (1, 2)]]
MIDDLE = [cell(7, 7), cell(3, 8), cell(11, 6)]
BORDER_LIMITS = (4, 100, False)
BORDER_CAP = 64                 # max_positions of the border searches, T = 1 and 2
# the threat cells that are committed: every position at the shallow limits (UNKNOWN cells, every own status), the first eight at the deep ones
THREAT_RUNS = {"shallow": THREAT_POSITIONS, "deep": 8}


def border_positions():
    return [[line[0], MIDDLE[0], line[1], MIDDLE[1]] if i % 2 == 0 else [MIDDLE[0], line[0], MIDDLE[1], line[1], MIDDLE[2]] for i, line in enumerate(BORDER_LINES)]


def positions():
    """vcf_reference.random_position with 8 .. 22 plies and spread 3, the plies in turn"""
    rng = random.Random(1717)
    out = []
    while len(out) < THREAT_POSITIONS:
        q = R.random_position(rng, 8 + len(out) % 15, 3)
        if q is not None:
            out.append(q)
    return out


def packed(values):
    """225 small numbers, mostly zero -> a string of digits, or [cell, value, cell, value ..] for the cells that are not zero, whichever is shorter"""
    pairs = [x for c, v in enumerate(values) if v for x in (c, v)]
    return "".join(str(v) for v in values) if max(values) <= 9 and len(json.dumps(pairs, separators=(",", ":"))) > 227 else pairs


def threats_task(task):
    limits, q = task
    t = V.threats(q, *limits)
    own = t["own"]
    return {"own": [own["status"], own["move"], own["length"], own["nodes"], own["pv"]], "verdict": packed(t["verdict"]), "length": packed(t["length"]),
            "nodes": packed(t["nodes"])}


def search_task(task):
    (run, max_threats, max_positions), q = task
    r = V.vct_solve(q, *RUNS[run], max_threats=max_threats, max_positions=max_positions)
    return [r["status"], r["move"], r["threats"], r["positions"], r["pv"]]


def border_search_task(task):
    max_threats, q = task
    r = V.vct_solve(q, *BORDER_LIMITS, max_threats=max_threats, max_positions=BORDER_CAP)
    return [r["status"], r["move"], r["threats"], r["positions"], r["pv"]]


def hand_task(name):
    q, max_threats = HAND[name]
    r = V.vct_solve(q, max_threats=max_threats)
    return [r["status"], r["move"], r["threats"], r["positions"], r["pv"], r["levels"]]


def main():
    pool = multiprocessing.Pool()
    qs = positions()
    hand = pool.map_async(hand_task, list(HAND), chunksize=1)
    searches = [pool.map_async(search_task, [(s, q) for q in qs[:ROOTS]], chunksize=1) for s in SEARCHES]
    out = {"runs": {k: list(v) for k, v in RUNS.items()}, "positions": qs, "roots": ROOTS}
    out["threats"] = {run: pool.map(threats_task, [(RUNS[run], q) for q in qs[:count]], chunksize=1) for run, count in THREAT_RUNS.items()}
    out["searches"] = [{"run": s[0], "max_threats": s[1], "max_positions": s[2], "results": result.get()} for s, result in zip(SEARCHES, searches)]
    out["hand"] = dict(zip(HAND, hand.get()))
    out["borders"] = {"limits": list(BORDER_LIMITS), "positions": border_positions(),
                      "threats": pool.map(threats_task, [(BORDER_LIMITS, q) for q in border_positions()], chunksize=1),
                      "searches": [{"max_threats": t, "max_positions": BORDER_CAP, "results": pool.map(border_search_task, [(t, q) for q in border_positions()], chunksize=1)}
                                   for t in (1, 2)]}
    with open(os.path.join(HERE, "vct_cases.json"), "w") as f:             # one key per line
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main()
