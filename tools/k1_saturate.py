#!/usr/bin/env python3
"""Search for legal positions that load K1's fixed-size on-chip structures as heavily as possible, and write the best of
them as a test fixture (tests/golden/k1_saturated.npz).

K1 (gomokuai_amd/csrc/eval_kernel.hip) queues a board's emitting transitions, compound candidates and counter-move rescans
in fixed-size LDS queues and keeps its '_' counters in 4-bit fields.  oracle.scratch_load reports how much of each a position
asks for; this tool runs one simulated-annealing search per load (several restarts each) over legal positions -- every cell
used once, black - white in {0, 1}, no five -- then adds, for the best four positions of each search, the position that the side
to move finishes with exactly one five, and makes a targeted attempt at the reference's compound-type error
(Pattern.cpp:484-485): a direction whose LiveThree counter is 1 while its DeadThree or LiveTwo counter is 2 or more.

CPU only, deterministic for a given --seed / --steps / --restarts (numpy.random.RandomState per task; the number of worker
processes, at most 16, does not change the result).

    python tools/k1_saturate.py --seed 20261017 --steps 300000 --restarts 6 --out tests/golden/k1_saturated.npz

(the committed fixture: 36 runs, about five minutes on eight cores)
"""
import argparse
import itertools
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 225
# one search per load; the secondary terms only break ties on the plateaus of a small integer load
OBJECTIVES = ("transitions", "matches", "candidates", "compounds", "queued", "max_counter")
KEEP_PER_RUN = 6
ROW_WIDTH = 13


def _oracle():
    from oracle import oracle as O
    return O


def objective(load, name, fields):
    v = load[:, fields.index(name)].astype(np.float64)
    if name == "max_counter":
        v = 40.0 * v + 0.05 * load[:, fields.index("matches")]
    return v


def random_position(rng, O, stones):
    while True:
        cells = np.zeros(N, np.int8)
        at = rng.permutation(N)[:stones]
        cells[at[0::2]] = 1
        cells[at[1::2]] = -1
        if O.scratch_load_cells(cells)[0, O.LOAD_FIELDS.index("fives")] == 0:
            return cells


def propose(rng, cells):
    """One legal-count mutation of the position (the five check is the caller's): returns a new array or None."""
    c = cells.copy()
    black, white, empty = np.nonzero(c == 1)[0], np.nonzero(c == -1)[0], np.nonzero(c == 0)[0]
    kind = rng.randint(0, 10)
    if kind < 5 and len(empty):                                   # a stone moves, mostly to a cell next to a stone
        src = (black if rng.randint(0, 2) else white)
        if not len(src):
            return None
        s = src[rng.randint(0, len(src))]
        if rng.randint(0, 4):
            o = (black if rng.randint(0, 2) else white)
            a = int(o[rng.randint(0, len(o))]) if len(o) else 112
            x, y = a % 15 + rng.randint(-2, 3), a // 15 + rng.randint(-2, 3)
            if not (0 <= x < 15 and 0 <= y < 15) or c[y * 15 + x] != 0:
                return None
            d = y * 15 + x
        else:
            d = empty[rng.randint(0, len(empty))]
        c[d] = c[s]
        c[s] = 0
    elif kind < 7 and len(black) and len(white):                  # a black and a white stone change places
        b, w = black[rng.randint(0, len(black))], white[rng.randint(0, len(white))]
        c[b], c[w] = -1, 1
    elif kind == 7 and len(empty) >= 2:                           # one stone of each colour more
        e = empty[rng.permutation(len(empty))[:2]]
        c[e[0]], c[e[1]] = 1, -1
    elif kind == 8 and len(black) and len(white):                 # ... or less
        c[black[rng.randint(0, len(black))]] = 0
        c[white[rng.randint(0, len(white))]] = 0
    else:                                                         # the side to move plays, or the last stone comes off
        if len(black) == len(white):
            if rng.randint(0, 2) and len(empty):
                c[empty[rng.randint(0, len(empty))]] = 1
            elif len(white):
                c[white[rng.randint(0, len(white))]] = 0               # (white's last stone comes off: black == white + 1)
        else:
            if rng.randint(0, 2) and len(empty):
                c[empty[rng.randint(0, len(empty))]] = -1
            else:
                c[black[rng.randint(0, len(black))]] = 0
    return c


def anneal(task):
    name, restart, seed, steps = task
    O = _oracle()
    F = O.LOAD_FIELDS
    rng = np.random.RandomState((seed + 1000003 * OBJECTIVES.index(name) + 7919 * restart) % (2 ** 32))
    cells = random_position(rng, O, 60 + 20 * (restart % 4))
    cur = objective(O.scratch_load_cells(cells), name, F)[0]
    t0 = 4.0 if name in ("transitions", "matches") else 2.0
    t1 = 0.15
    best = []                                                      # (value, cells) of the run's successive records
    best_v = -1.0
    for step in range(steps):
        cand = propose(rng, cells)
        if cand is None:
            continue
        load = O.scratch_load_cells(cand)
        if load[0, F.index("fives")] or load[0, F.index("type_error")]:
            continue
        v = objective(load, name, F)[0]
        temp = t0 * (t1 / t0) ** (step / float(steps))
        if v >= cur or rng.random_sample() < np.exp((v - cur) / temp):
            cells, cur = cand, v
            if v > best_v:
                best_v = v
                best.append((v, cand.copy()))
                best = best[-KEEP_PER_RUN:]
    return name, restart, [b[1] for b in best]


def error_row_task(task):
    """All fillings of thirteen cells of the middle row (the rest of the board empty), from column `first` on, that trip the
    compound-type error.  A pattern that covers a cell lies within six cells of it, so first = 1 (cells 1 .. 13, the window of cell 7)
    decides every cell of a line that is six or more cells from both of its ends, and first = 0 (cells 0 .. 12) every cell less than
    six from one end of a line of thirteen or more.  Not covered: lines shorter than thirteen, stones off the line."""
    first, lo, hi = task
    O = _oracle()
    F = O.LOAD_FIELDS
    found = []
    width = ROW_WIDTH
    for base in range(lo, hi, 4096):
        idx = np.arange(base, min(base + 4096, hi))
        cells = np.zeros((len(idx), N), np.int8)
        rest = idx.copy()
        for k in range(width):
            cells[:, 7 * 15 + first + k] = (rest % 3).astype(np.int8) - 1
            rest //= 3
        load = O.scratch_load_cells(cells)
        for i in np.nonzero((load[:, F.index("type_error")] != 0) & (load[:, F.index("fives")] == 0))[0]:
            found.append(cells[i].copy())
    return found


def balance(cells, O):
    """Adds stones far from the row pattern (two rows at the board's edges, never three in a line) until black - white is 0 or 1;
    returns the legal position if the error is still there, else None."""
    F = O.LOAD_FIELDS
    c = cells.copy()
    spots = [y * 15 + x for y in (0, 14, 1, 13) for x in (0, 4, 8, 12, 2, 6, 10, 14)]
    diff = int((c == 1).sum()) - int((c == -1).sum())
    for s in spots:
        if diff in (0, 1):
            break
        c[s] = -1 if diff > 1 else 1
        diff += 1 if c[s] == 1 else -1
    if diff not in (0, 1):
        return None
    load = O.scratch_load_cells(c)[0]
    return c if load[F.index("type_error")] and not load[F.index("fives")] else None


def finished_variant(cells, name, O):
    """The position after the side to move has made exactly one five, the one with the highest load; None if it cannot."""
    F = O.LOAD_FIELDS
    mover = 1 if (cells == 1).sum() == (cells == -1).sum() else -1
    empty = np.nonzero(cells == 0)[0]
    cand = np.repeat(cells[None], len(empty), axis=0)
    cand[np.arange(len(empty)), empty] = mover
    load = O.scratch_load_cells(cand)
    ok = np.nonzero((load[:, F.index("fives")] == 1) & (load[:, F.index("type_error")] == 0))[0]
    if not len(ok):
        return None
    i = ok[np.argmax(objective(load[ok], name, F))]
    return cand[i], int(empty[i])


def to_moves(cells, last=None):
    """A move list of the position: black on the even plies, the stone `last` (if given) as the final ply."""
    black = [int(c) for c in np.nonzero(cells == 1)[0] if c != last]
    white = [int(c) for c in np.nonzero(cells == -1)[0] if c != last]
    if last is not None:
        (black if cells[last] == 1 else white).append(int(last))
    assert len(black) - len(white) in (0, 1)
    seq = [m for pair in itertools.zip_longest(black, white) for m in pair if m is not None]
    assert last is None or seq[-1] == last
    return seq


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--steps", type=int, default=300000, help="annealing steps per run")
    ap.add_argument("--restarts", type=int, default=6, help="runs per load")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "k1_saturated.npz"))
    args = ap.parse_args()
    O = _oracle()
    O.lib()
    F = O.LOAD_FIELDS
    workers = max(1, min(16, args.workers))
    t_start = time.time()
    tasks = [(name, r, args.seed, args.steps) for name in OBJECTIVES for r in range(args.restarts)]
    total = 3 ** ROW_WIDTH
    chunks = [(first, lo, min(lo + 65536, total)) for first in (1, 0) for lo in range(0, total, 65536)]
    with multiprocessing.Pool(workers) as pool:
        runs = pool.map(anneal, tasks, chunksize=1)
        rows = [c for part in pool.map(error_row_task, chunks, chunksize=1) for c in part]
    seconds = time.time() - t_start

    positions, lasts, origin = [], [], []                          # cells, final ply or -1, objective index (6 = error attempt)
    seen = set()

    def add(cells, last, o):
        key = cells.tobytes()
        if key not in seen and len(positions) < 256:
            seen.add(key)
            positions.append(cells)
            lasts.append(-1 if last is None else last)
            origin.append(o)

    for o, name in enumerate(OBJECTIVES):
        mine = [c for n_, _, cs in runs if n_ == name for c in cs]
        vals = objective(O.scratch_load_cells(np.array(mine)), name, F)
        order = np.argsort(-vals, kind="stable")[:30]
        for i in order:
            add(mine[i], None, o)
        for i in order[:4]:
            fin = finished_variant(mine[i], name, O)
            if fin is not None:
                add(fin[0], fin[1], o)
    n_error = 0
    for c in rows:
        legal = balance(c, O)
        if legal is not None and n_error < 16:
            add(legal, None, len(OBJECTIVES))
            n_error += 1

    n = len(positions)
    moves = np.zeros((n, 232), np.uint8)
    lens = np.zeros(n, np.int32)
    for i, (c, last) in enumerate(zip(positions, lasts)):
        seq = to_moves(c, None if last < 0 else last)
        moves[i, :len(seq)] = seq
        lens[i] = len(seq)
    load = O.scratch_load(moves, lens)
    assert (load == O.scratch_load_cells(np.array(positions))).all()
    np.savez_compressed(args.out, moves=moves, lens=lens, load=load, fields=np.array(F), origin=np.array(origin, np.int8),
                        objectives=np.array(OBJECTIVES + ("type_error",)), seed=np.int64(args.seed), steps=np.int64(args.steps),
                        restarts=np.int64(args.restarts), error_rows_found=np.int64(len(rows)), error_positions=np.int64(n_error))
    print("search: %.0f s on %d workers, seed %d, %d runs of %d steps, %d row fillings enumerated" % (seconds, workers, args.seed, len(tasks), args.steps, 2 * total))
    print("positions: %d (%d finished by a five, %d with the compound-type error; %d erroneous row fillings before balancing)" %
          (n, sum(l >= 0 for l in lasts), n_error, len(rows)))
    in_play = load[:, F.index("fives")] == 0
    for k, f in enumerate(F):
        print("  max %-12s %4d  (in play %4d)" % (f, load[:, k].max(), load[in_play, k].max()))


if __name__ == "__main__":
    main()
