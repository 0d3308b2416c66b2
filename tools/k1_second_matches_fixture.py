#!/usr/bin/env python3
"""Chooses tests/golden/k1_second_matches.npz (a recipe, CPU only): boards on which transitions report two matches, picked with
oracle.scratch_load from the synthetic kinds and from tests/golden/k1_saturated.npz.  What tells the boards apart is how their matches M lie
against their emitting transitions T in K1's deposit rounds of 64 lanes (one lane per transition; a second match is deposited by its transition's lane, or, in the form round 10 measured and dropped, by a lane of its own):
  more      M > T                                   (at least 100 boards)
  new_round ceil(M / 64) > ceil(T / 64)             the second matches would open a round of their own
  lane0     T % 64 == 0 and M > T                   the rounds are full: a second match of its own would be lane 0 of a new round
  crowded   M - T > ceil(T / 64)                    two or more second matches come from one round (pigeonhole)
  none      M == T
  heaviest  the boards of k1_saturated.npz with the most matches
usage: k1_second_matches_fixture.py [out.npz]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gomokuai_amd import lib as G
from oracle import oracle as O

STRIDE = 232
CASES = ("more", "new_round", "lane0", "crowded", "none", "heaviest")


def case_masks(load):
    """The cases a board belongs to, from its scratch_load row: bool[n] per case ("heaviest" is a choice, not a property: not here)."""
    t, m = load[:, O.LOAD_FIELDS.index("transitions")].astype(np.int64), load[:, O.LOAD_FIELDS.index("matches")].astype(np.int64)
    rounds = lambda v: (v + 63) // 64
    return {"more": m > t, "new_round": rounds(m) > rounds(t), "lane0": (t % 64 == 0) & (t > 0) & (m > t), "crowded": m - t > rounds(t), "none": (m == t) & (t > 0)}


def main(out):
    pool_moves, pool_lens = [], []
    for kind in (0, 1):
        moves, lens, _ = G.synth_boards(12000, kind, first_board=300000, stride=STRIDE)
        pool_moves.append(moves); pool_lens.append(lens)
    with np.load(os.path.join(ROOT, "tests", "golden", "k1_saturated.npz")) as f:
        sat_moves, sat_lens = f["moves"], f["lens"]
    pool_moves.append(sat_moves); pool_lens.append(sat_lens)
    moves, lens = np.concatenate(pool_moves), np.concatenate(pool_lens)
    load = O.scratch_load(moves, lens)
    masks = case_masks(load)
    want = {"more": 110, "new_round": 24, "lane0": 12, "crowded": 40, "none": 16}
    chosen = []
    for name in ("lane0", "new_round", "crowded", "none", "more"):
        have = int(masks[name][chosen].sum()) if chosen else 0
        for i in np.nonzero(masks[name])[0]:
            if have >= want[name]:
                break
            if i not in chosen:
                chosen.append(int(i)); have += 1
        print("%-10s %d in the pool, %d chosen so far hold it" % (name, int(masks[name].sum()), int(masks[name][chosen].sum())))
    sat_first = len(lens) - len(sat_lens)
    heavy = sat_first + np.argsort(-load[sat_first:, O.LOAD_FIELDS.index("matches")], kind="stable")[:12]
    chosen += [int(i) for i in heavy if i not in chosen]
    chosen = np.array(chosen)
    heaviest = np.isin(chosen, heavy)
    np.savez_compressed(out, moves=moves[chosen], lens=lens[chosen], load=load[chosen], fields=np.array(O.LOAD_FIELDS), heaviest=heaviest)
    print("%d boards, max matches %d, %d bytes" % (len(chosen), load[chosen][:, O.LOAD_FIELDS.index("matches")].max(), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "k1_second_matches.npz"))
