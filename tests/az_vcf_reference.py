"""A plain Python restatement of K7 with forced wins by fours solved at its leaves (include/gomoku_hip.h, "K7 + K14"), for the tests: the search
of tests/az_leaves_reference.py with its evaluator wrapped,
    E'(position) = (1.0, one-hot(r.move)) if r.status == WIN else E(position),    r = vcf_reference.solve(the leaf's moves, D, B)
(plain mode, the side to move attacks).  Nothing else changes: the legality check, the arena-full rule, virtual loss, quota and the order of the
pending leaves are LeavesSearch's.  It imports nothing from the package."""
import numpy as np

import az_leaves_reference as R
import vcf_reference as V

N = 225
_c = lambda y, x: y * 15 + x
# stones far from everything, no two of them on a line within four steps (tests/test_vcf_reference.py's FAR)
FAR = [_c(14, 0), _c(13, 4), _c(14, 9), _c(12, 14), _c(9, 14), _c(10, 0), _c(7, 12), _c(8, 2)]
# black 5, 6, 7 on row 0, black to move: WIN in two moves, pv [4, 3, 8], four nodes (tests/test_vcf_reference.py's ROW0)
BLACK_THREE = [5, FAR[0], 6, FAR[1], 7, FAR[2]]
# the same three in white, white to move
WHITE_THREE = [FAR[0], 5, FAR[1], 6, FAR[2], 7, FAR[3]]
# white's three with black to move, who has nothing: the win is white's, one ply below the root wherever black does not block
WHITE_THREE_BLACK_TO_MOVE = [FAR[0], 5, FAR[1], 6, FAR[2], 7]
QUIET = R.OPENINGS[1]
# 22 stones, black to move: a forced win in three moves that the plain walk at depth 8 finds after 94 nodes
HARD = [127, 141, 125, 68, 69, 97, 126, 157, 67, 99, 140, 124, 98, 112, 110, 65, 158, 130, 156, 143, 144, 95]
# the five games of the GPU parity test
PARITY_OPENINGS = [QUIET, BLACK_THREE, WHITE_THREE, R.OPEN_FOUR, HARD]
PARITY_SETTINGS = [(8, 64), (3, 2)]                              # (D, B)


class VcfLeavesSearch(R.LeavesSearch):
    """LeavesSearch with the solver in front of the evaluator.  vcf_depth = 0: LeavesSearch itself."""

    def __init__(self, moves, evaluator, vcf_depth=0, vcf_budget=64, **kw):
        super().__init__(moves, evaluator, **kw)
        self.vcf_depth, self.vcf_budget = int(vcf_depth), int(vcf_budget)
        self.reset_counters()

    def reset_counters(self):
        self.solved, self.wins, self.cut, self.nodes = 0, 0, 0, 0
        self.wins_below_root, self.budget_leaves = 0, 0
        self.verdicts = []                                       # of the last step, one per pending leaf

    def answers(self, states):
        """The evaluator's answers for the pending leaves of the select step that returned `states`, after the solver."""
        out, self.verdicts = [], []
        for (node, moves), planes in zip(self.pending, states):
            value, probs = self.evaluator(planes)
            if self.vcf_depth > 0:
                r = V.solve(moves, self.vcf_depth, self.vcf_budget)
                self.verdicts.append(r)
                self.solved += 1
                self.nodes += r["nodes"]
                self.cut += r["status"] in (V.BUDGET, V.DEPTH)
                self.budget_leaves += r["status"] == V.BUDGET
                if r["status"] == V.WIN:
                    self.wins += 1
                    self.wins_below_root += node != 0
                    value, probs = np.float32(1.0), np.zeros(N, dtype=np.float32)
                    probs[r["move"]] = np.float32(1.0)
            out.append((value, probs))
        return out

    def step(self):
        out = self.answers(self.select_step())
        self.expand_step([v for v, _ in out], [p for _, p in out])
