"""A plain Python restatement of K7 with the defence solver at its leaves (include/gomoku_hip.h, "K7 + K15"), for the tests:
az_proof_reference.ProofSearch plus, with the solver (D > 0), proofs and the defend option all on, for every pending leaf P whose own verdict is
neither WIN nor OVER
    d = vcf_defend_reference.defend(P's moves, D, B)             (plain mode)
    d.threat WIN, once P's children exist (not dropped):
        every child whose cell is CELL_LOSES gets WINS with its own word (not through prove), proved += 1 and marked += 1 each;
        P has a child for every free cell and all of them are WINS: prove(P, LOSES), and +1.0 is backed up from P in place of -value.
    any other threat status marks nothing.
Counters per tree: threatened (pending leaves under a WIN threat), marked, searched (cells solved in full) and def_nodes (the nodes of those
solves); a leaf whose playout is dropped for a full arena marks nothing and counts nowhere.  With any of the three options
off it is ProofSearch, field for field.  It imports nothing from the package."""
import numpy as np

import az_leaves_reference as R
import az_proof_reference as P
import vcf_defend_reference as D
import vcf_reference as V

N = 225
NONE, WINS, LOSES = P.NONE, P.WINS, P.LOSES
NO_NODE = R.NO_NODE
_c = lambda y, x: y * 15 + x


def _position(black, white):
    """black and white cells -> a move list, black first; white is one stone short when white is to move"""
    assert len(black) in (len(white), len(white) + 1)
    moves = []
    for i in range(len(black)):
        moves.append(black[i])
        if i < len(white):
            moves.append(white[i])
    return moves


# the four positions of DESIGN.md K19, white to move in each
OPEN_FOUR = _position([_c(7, 3), _c(7, 4), _c(7, 5), _c(7, 6)], [_c(0, 0), _c(0, 2), _c(0, 4)])
OPEN_THREE = _position([_c(7, 4), _c(7, 5), _c(7, 6)], [_c(0, 0), _c(0, 2)])
_FIVE_WHITE = [_c(0, 0), _c(2, 3), _c(4, 14), _c(11, 1), _c(13, 9)]
TWO_THREES = _position([_c(7, 5), _c(7, 6), _c(7, 7), _c(10, 2), _c(10, 3), _c(10, 4)], _FIVE_WHITE)
THREE_AND_THREE = _position([_c(7, 5), _c(7, 6), _c(7, 7), _c(5, 8), _c(6, 8), _c(8, 8)], _FIVE_WHITE)
TABLE = [OPEN_FOUR, OPEN_THREE, TWO_THREES, THREE_AND_THREE]
# Black to move with two twos that cross at (7, 7) and no four to make (solve: NONE at (8, 64)).  After black's (7, 7) white faces two open
# threes through that stone and no cell holds: that child is proven LOSES when it is expanded, and the root WINS through it.
ONE_PLY_UP = _position([_c(7, 5), _c(7, 6), _c(5, 7), _c(6, 7)], _FIVE_WHITE[:4])
ONE_PLY_UP_MOVE = _c(7, 7)

_memo = {}


def defend(moves, depth, budget):
    """vcf_defend_reference.defend in plain mode, remembered: the tests ask for the same positions many times"""
    key = (tuple(moves), depth, budget)
    if key not in _memo:
        _memo[key] = D.defend(list(moves), depth, budget, iterative=False)
    return _memo[key]


class DefendSearch(P.ProofSearch):
    """ProofSearch with the defence solver at the leaves.  defend = False, proof = False or vcf_depth = 0: ProofSearch itself."""

    def __init__(self, moves, evaluator, vcf_depth=0, vcf_budget=64, proof=False, defend=False, **kw):
        self.defend_on = bool(defend)
        super().__init__(moves, evaluator, vcf_depth, vcf_budget, proof, **kw)

    @property
    def defend_active(self):
        return self.defend_on and self.proof_on and self.vcf_depth > 0

    def reset_counters(self):
        super().reset_counters()
        self.threatened, self.marked, self.searched, self.def_nodes = 0, 0, 0, 0
        self.defend_leaves, self.defend_losses = 0, 0             # leaves with a marked child, leaves proven LOSES by defence
        self.defences = []                                       # of the last step, one per pending leaf (None: not asked)

    def answers(self, states):
        out = super().answers(states)
        self.defences = []
        if self.defend_active:
            for (node, moves), r in zip(self.pending, self.verdicts):
                self.defences.append(None if r["status"] in (V.WIN, V.OVER) else defend(moves, self.vcf_depth, self.vcf_budget))
        return out

    def expand_step(self, values, probs):
        if not self.defend_active:
            return super().expand_step(values, probs)
        solved = len(self.verdicts) == len(self.pending)
        for k, (leaf, moves) in enumerate(self.pending):
            d = self.defences[k] if solved and len(self.defences) == len(self.pending) else None
            threat = d is not None and d["threat"]["status"] == V.WIN
            occupied = set(moves)
            pr = np.asarray(probs[k], dtype=np.float32)
            take = [c for c in range(N) if pr[c] != 0.0 and c not in occupied]
            dropped, lost = False, False
            if take:
                if self.n_nodes + len(take) > self.cap:
                    self.status |= R.STATUS_ARENA_FULL
                    dropped = True
                else:
                    self.first[leaf], self.nkids[leaf] = self.n_nodes, len(take)
                    self.proof[leaf] = NONE                      # the child word is rewritten
                    for c in take:
                        self.visits.append(0); self.value.append(np.float32(0.0)); self.prior.append(np.float32(pr[c]))
                        self.parent.append(leaf); self.first.append(0); self.nkids.append(0); self.cell.append(c); self.inflight.append(0)
                        self.proof.append(NONE)
                    if solved and self.verdicts[k]["status"] == V.WIN:
                        self.prove(leaf, WINS)
                    elif threat:
                        a, n = self.first[leaf], self.nkids[leaf]
                        marked = 0
                        for i in range(a, a + n):
                            if d["verdict"][self.cell[i]] == D.CELL_LOSES:
                                self.proof[i] = WINS
                                marked += 1
                        self.proved += marked
                        self.marked += marked
                        self.defend_leaves += marked > 0
                        if n == N - len(moves) and marked == n:
                            self.prove(leaf, LOSES)
                            self.defend_losses += 1
                            lost = True
            if threat and not dropped:
                self.threatened += 1
                self.searched += len(d["searched"])
                self.def_nodes += sum(d["nodes"])
            if not dropped:
                self._backup(leaf, np.float32(1.0) if lost else -np.float32(values[k]))
            up = leaf
            while up != NO_NODE:
                self.inflight[up] -= 1
                up = self.parent[up]
        self.pending = []

    def defend_stats(self):
        return {"threatened": self.threatened, "marked": self.marked, "searched": self.searched, "nodes": self.def_nodes}

    def defend_verdicts(self):
        """What gmk_az_defend_verdicts_host reads for the pending leaves of the last select step, after answers(): per leaf the threat's
        status and length and per cell the verdict and the nodes; a leaf that was not asked reads NONE and zeros."""
        out = []
        for d in self.defences:
            if d is None:
                out.append({"threat_status": V.NONE, "threat_length": 0, "verdict": [0] * N, "nodes": [0] * N})
            else:
                out.append({"threat_status": d["threat"]["status"], "threat_length": d["threat"]["length"], "verdict": list(d["verdict"]),
                            "nodes": list(d["nodes"])})
        return out
