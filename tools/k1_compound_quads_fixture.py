#!/usr/bin/env python3
"""Writes tests/golden/k1_compound_quads.npz: for each of 1 .. 20 candidate cells a board of crossing two- and three-stone lines with exactly
that many (tests/eval_compound_quads_boards.py, candidate_sweep: the first such board of a seeded random series per mode -- white's candidates
only, black's only, both colours mixed).  The tests check the fixture against the oracle's load counts again; this only spares them the search.
usage: k1_compound_quads_fixture.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import oracle as O
import eval_compound_quads_boards as B

found = B.candidate_sweep(O, tries=3000)
modes, counts, boards = [], [], []
for mode in ("white", "black", "mixed"):
    for n in sorted(found[mode]):
        modes.append(mode); counts.append(n); boards.append(found[mode][n])
moves, lens = B.pack(boards)
out = os.path.join(ROOT, "tests", "golden", "k1_compound_quads.npz")
np.savez_compressed(out, moves=moves, lens=lens, mode=np.array(modes), candidates=np.array(counts, dtype=np.int32))
print("%d boards -> %s (%d bytes); candidate counts per mode: %s" % (len(boards), out, os.path.getsize(out), {m: sorted(found[m]) for m in found}))
