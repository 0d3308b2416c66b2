"""The two CPU restatements of the pattern heuristic's float32 path (oracle.trad_heuristic = oracle/go_trad.c, and
tests/trad_rave_reference.py with the filter on and off) against the independent float64 statement of Heuristic.hpp in
tests/heuristic_f64_reference.py: the support exactly, every probability and the value within the DERIVED rounding bound, the norm, the
best move.  The inputs are tests/heuristic_f64_inputs.py's; tests/test_heuristic_f64_gpu.py holds the kernels (K10, K6) to the same
statement on a draw of them.  The bound is checked here, on the CPU, before a GPU sees it.

test_mutants_are_caught is the evidence that these assertions bite: eight wrong heuristics, each a one-line change to a copy of the
float32 restatement kept in this file, each of which has to break an assertion on at least one input.

Measured on these inputs (printed by test_restatements_meet_the_float64_statement, quoted in DESIGN.md, "Pattern-guided search (K6,
K10): what holds the float part"): the largest err / bound is 0.166 for the probabilities and 0.093 for the value."""
import functools
import math

import numpy as np
import pytest

import heuristic_f64_inputs as inputs
import heuristic_f64_reference as H

F32 = np.float32
N = 225


# ---------------- a copy of the float32 restatement (tests/trad_rave_reference.py), with one switch per mutant ----------------
MUTANTS = ("value_score_group", "no_max", "literals_swapped", "literal_1_2", "density_formula", "zero_vector_division", "no_own_dead_three",
           "table_entry")


class Float32Heuristic:
    """trad_rave_reference's heuristic functions again, line for line; `mutant` names the one thing done wrongly (None: nothing)."""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.m = mutant
        table = [list(row) for row in H.AUTOMATA_TABLE]
        if mutant == "table_entry":
            table[0][H.SL3] = (H.STO43, 0)                        # {To44, 0} -> {To43, 0}: the own double four is never looked at
        self.table = table

    @staticmethod
    def sum225(x):
        p = x[0:64] + x[64:128]
        p = p + x[128:192]
        p[:N - 192] = p[:N - 192] + x[192:N]
        p = p.reshape(4, 16)
        for s in (8, 4, 2, 1):
            p[:, :s] = p[:, :s] + p[:, s:2 * s]
        return (p[0, 0] + p[1, 0]) + (p[2, 0] + p[3, 0])

    def normalize225(self, x):
        z = self.sum225(x * x)
        if self.m == "zero_vector_division":
            with np.errstate(all="ignore"):
                return x / np.sqrt(z)
        if z > F32(0):
            x = x / np.sqrt(z)
        return x

    def density_weight(self, density, player):
        g = H.group1(player)
        keep = (lambda a: a) if self.m == "no_max" else (lambda a: np.maximum(a, 0))
        n, w = keep(density[g, 0]).astype(F32), keep(density[g, 1]).astype(F32)
        if self.m == "density_formula":
            return self.normalize225((F32(3) * w) / (F32(1) + n))
        return self.normalize225((F32(3) * w) / (F32(1) + F32(2) * n))

    def evaluation_probs(self, scores, density, nrec, player):
        if nrec != 0:
            self_worthy = scores[H.group2(player, player)].astype(F32) * self.density_weight(density, player)
            rival_anti = scores[H.group2(-player, player)].astype(F32) * self.density_weight(density, -player)
            a, b = (F32(0.4), F32(0.6)) if self.m == "literals_swapped" else (F32(0.6), F32(0.4))
            return self.normalize225(a * self_worthy + b * rival_anti)
        probs = np.zeros(N, F32)
        probs[7 * 15 + 7] = 1
        return probs

    def evaluation_value(self, scores, density, player):
        rival_group = H.group2(-player, player) if self.m == "value_score_group" else H.group2(-player, -player)
        self_worthy = self.sum225(scores[H.group2(player, player)].astype(F32) * self.density_weight(density, player))
        rival_worthy = self.sum225(scores[rival_group].astype(F32) * self.density_weight(density, -player))
        k = 1.0 if self.m == "literal_1_2" else 1.2
        return F32(math.tanh((k * float(self_worthy) - float(rival_worthy)) / 500.0))

    def decisive_filter(self, pdist, cdist, cur, probs):
        state, anti = H.S4, 0
        while state != H.SEND:
            player = -cur if anti else cur
            if state == H.S4:
                cand = [(H.LIVE_FOUR, player), (H.DEAD_FOUR, player)]
            elif state == H.SL3:
                cand = [(H.LIVE_THREE, player)]
            else:
                cand = [(H.PATTERN_SIZE + (H.STO33 - state), player)]
            head = 0
            while head < len(cand):
                pattern, pl = cand[head]
                field = int(pdist[N, pattern] if pattern < H.PATTERN_SIZE else cdist[N, pattern - H.PATTERN_SIZE])
                if (field >> (16 * H.group1(pl))) & 0xFFFF:
                    if anti and state != H.S4 and self.m != "no_own_dead_three":
                        cand.append((H.DEAD_THREE, -pl))
                    break
                head += 1
            if head < len(cand):
                keep = np.zeros(N, bool)
                for pattern, pl in cand[head:]:
                    field = pdist[:N, pattern] if pattern < H.PATTERN_SIZE else cdist[:N, pattern % H.PATTERN_SIZE]
                    keep |= ((field >> np.uint32(8 * H.group2(pl, cur))) & np.uint32(0xFF)) != 0
                probs = np.where(keep, probs, F32(0)).astype(F32)
                probs = self.normalize225(probs)
                state = H.SEND
            else:
                state, anti = self.table[anti][state]
        return probs

    def both(self, st):
        """-> (unfiltered probs, filtered probs, value) on an evaluator state of _states()"""
        p = self.evaluation_probs(st["scores"], st["density"], st["nrec"], st["cur"])
        with np.errstate(all="ignore"):
            f = self.decisive_filter(st["pdist"], st["cdist"], st["cur"], p)
        return p, f, self.evaluation_value(st["scores"], st["density"], st["cur"])


# ---------------- the inputs, evaluated once ----------------
@functools.lru_cache(maxsize=None)
def _states():
    """per position: the integer evaluator state, the float64 statement with its bounds, and oracle.trad_heuristic's answer"""
    from oracle import oracle as O
    out = []
    for group, name, moves in inputs.positions():
        ev = inputs.replay(O, moves)
        assert not ev.check_end(), name
        b = ev.board
        st = {"group": group, "name": name, "moves": moves, "cur": int(b.cur_player), "nrec": int(b.nrec), "scores": ev.scores(),
              "density": ev.density(), "pdist": ev.pattern_dist(), "cdist": ev.compound_dist()}
        assert st["nrec"] == len(moves) and st["cur"] == (H.BLACK if len(moves) % 2 == 0 else H.WHITE)
        st["f64"] = H.Position(ev)
        st["c"] = O.trad_heuristic(moves)
        out.append(st)
    return out


def _passes(h, st):
    """whether the float32 heuristic `h` meets every assertion at this position"""
    try:
        p, f, v = h.both(st)
        H.check(st["f64"], 0, p, v)
        H.check(st["f64"], 1, f, v)
    except AssertionError:
        return False
    return True


# ---------------- the tests ----------------
def test_inputs_reach_every_group_and_every_exit():
    states = _states()
    assert len(states) >= 3000
    groups = {st["group"] for st in states}
    assert groups == {"random", "clustered", "greedy", "hand", "tie"}
    exits = np.bincount([st["f64"].exit for st in states], minlength=6)
    print("automaton exits", dict(zip(H.EXIT_NAMES, exits.tolist())))
    assert (exits >= 8).all(), exits                              # the five exits and the path that runs out
    lens = [len(st["moves"]) for st in states if st["group"] == "tie"]
    assert min(lens) >= 150 and max(lens) == 224
    names = {st["name"]: st for st in states}
    hi, lo = names["high_cells"]["f64"].filtered, names["low_cells"]["f64"].filtered
    assert hi[192:].any() and not hi[:192].any() and lo[:64].any() and not lo[64:].any()
    # the filter matters, the density words do go negative, and zero vectors occur
    assert sum((st["f64"].filtered != st["f64"].probs).any() for st in states) >= 500
    assert sum((st["density"] < 0).any() for st in states) >= 1000
    assert sum(not H.density_weight(st["density"], p).any() for st in states for p in (H.BLACK, H.WHITE)) >= 8


def test_the_copy_is_the_restatement():
    """the unmutated copy above equals tests/trad_rave_reference.py bit for bit: the mutants are mutants of THAT code"""
    import trad_rave_reference as R
    h = Float32Heuristic()
    for st in _states()[::7]:
        p, f, v = h.both(st)
        rp = R.evaluation_probs(st["scores"], st["density"], st["nrec"], st["cur"])
        rf = R.decisive_filter(st["pdist"], st["cdist"], st["cur"], rp)
        rv = R.evaluation_value(st["scores"], st["density"], st["cur"])
        assert p.tobytes() == np.asarray(rp, F32).tobytes() and f.tobytes() == np.asarray(rf, F32).tobytes() and F32(v).tobytes() == F32(rv).tobytes()


def test_restatements_meet_the_float64_statement():
    import trad_rave_reference as R
    margin_p = margin_v = 0.0
    for st in _states():
        f64 = st["f64"]
        cp, cv = st["c"]                                          # go_trad.c: filtered probabilities and the value
        rp = R.evaluation_probs(st["scores"], st["density"], st["nrec"], st["cur"])
        rf = R.decisive_filter(st["pdist"], st["cdist"], st["cur"], rp)
        rv = R.evaluation_value(st["scores"], st["density"], st["cur"])
        for filt, p, v, who in ((1, cp, cv, "go_trad.c"), (0, rp, rv, "restatement, unfiltered"), (1, rf, rv, "restatement, filtered")):
            mp, mv = H.check(f64, filt, p, v, "%s at %s" % (who, st["name"]))
            margin_p, margin_v = max(margin_p, mp), max(margin_v, mv)
    print("largest err / bound over %d positions: probabilities %.3f, value %.3f" % (len(_states()), margin_p, margin_v))
    # by the derivation both are below 1 (asserted cell by cell above); far below 0.01 the bound would be too loose to mean much
    assert 0.01 < margin_p < 1.0 and 0.01 < margin_v < 1.0


def test_search_root_carries_the_heuristic(oracle):
    """The sign convention tests/test_heuristic_f64_gpu.py relies on for K6: the root is the player's who has just moved, the first
    playout expands it with the filtered probabilities as priors and backs the value of the player to move up negated."""
    t = oracle.TraditionalMCTS(5.0)
    for st in _states()[::97]:
        t.search(st["moves"], 1)
        visits, _, priors, _ = t.root_children()
        probs, value = st["c"]
        assert priors.tobytes() == probs.tobytes() and not visits.any() and t.root_visits == 1
        assert F32(t.root_value) == -F32(value)
        assert abs(float(t.root_value) + st["f64"].value) <= st["f64"].value_bound


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_are_caught(mutant):
    states = _states()
    good = Float32Heuristic()
    assert all(_passes(good, st) for st in states[::11])         # the copy itself passes (all of it does, through the test above)
    h = Float32Heuristic(mutant)
    caught = sum(not _passes(h, st) for st in states)
    print("mutant %s: caught on %d of %d positions" % (mutant, caught, len(states)))
    assert caught >= 1
