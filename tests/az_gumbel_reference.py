"""K7's search at one leaf per step with the Gumbel root step of K21, restated for the tests: the tree, the PUCB descent below the root, the
expansion and the backup are tests/az_leaves_reference.py's (with tests/az_vcf_reference.py's solver in front of the evaluator when vcf_depth > 0);
the root step, the move and the improved-policy row are tests/gumbel_reference.py's.  It imports nothing from the package.

What K21 adds to the search (include/gomoku_gumbel.h, include/gomoku_hip.h "K21"):
  - a root without children is the leaf of its playout, as before; the first root step that finds children makes the root's set-up (`ready`);
  - a root step takes the set-up's pick, and the descent goes on below that child by PUCB;
  - whatever moves or replaces the root voids the set-up, and so does asking for the choice: choice() makes the set-up if the root has children and
    none yet, answers (move, row), and voids it."""
import numpy as np

import az_vcf_reference as V
import gumbel_reference as GR

N = 225


class GumbelSearch(V.VcfLeavesSearch):
    def __init__(self, moves, evaluator, m, n_sims, game_id, seed, c_visit=50.0, c_scale=1.0, **kw):
        kw.setdefault("leaves", 1)
        assert kw["leaves"] == 1
        self.m, self.n_sims, self.game_id, self.seed, self.c_visit, self.c_scale = int(m), int(n_sims), int(game_id), int(seed), float(c_visit), float(c_scale)
        self.ready = None
        self.setups = 0
        super().__init__(moves, evaluator, **kw)

    def _new_root(self):
        super()._new_root()
        self.ready = None

    def by_cell(self):
        prior, visits, value = np.zeros(N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.float32)
        for i in range(self.first[0], self.first[0] + self.nkids[0]):
            prior[self.cell[i]], visits[self.cell[i]], value[self.cell[i]] = self.prior[i], self.visits[i], self.value[i]
        return prior, visits, value

    def _child_of(self, cell):
        for i in range(self.first[0], self.first[0] + self.nkids[0]):
            if self.cell[i] == cell:
                return i
        raise AssertionError("no child of cell %d" % cell)

    def _set_up(self, prior, visits):
        if self.ready is None:
            self.ready = GR.Root(prior, visits, self.m, self.game_id, len(self.moves), self.seed, self.c_visit, self.c_scale)
            self.setups += 1

    def _descend(self):
        if not self.nkids[0]:
            return 0, []
        prior, visits, value = self.by_cell()
        self._set_up(prior, visits)
        cell = self.ready.pick(visits, value, self.value[0], self.n_sims)
        node, path = self._child_of(cell), [cell]
        while self.nkids[node]:                                  # Default::Select below the root, az_leaves_reference's formula at v = 0
            a, b = self.first[node], self.first[node] + self.nkids[node]
            n = np.array(self.visits[a:b], dtype=np.float64)
            q = np.array(self.value[a:b], dtype=np.float32).astype(np.float64)
            p = np.array(self.prior[a:b], dtype=np.float32).astype(np.float64)
            score = q + self.c_puct * p * np.sqrt(np.float64(self.visits[node])) / (n + 1.0)
            best = int(np.argmax(score))
            if not score[best] > -1.0:
                best = 0
            node = a + best
            path.append(self.cell[node])
        return node, path

    def choice(self):
        """(the move or -1, the improved-policy row uint16[225]) of the Gumbel root-choice and advance kernels; voids the set-up"""
        if not self.nkids[0]:
            self.ready = None
            return -1, np.zeros(N, np.uint16)
        prior, visits, value = self.by_cell()
        self._set_up(prior, visits)
        move = self.ready.move(visits, value, self.value[0])
        row = GR.row(prior, visits, value, self.value[0], self.c_visit, self.c_scale)
        self.ready = None
        return move, row

    def reroot(self, move=None):
        out = super().reroot(move)
        self.ready = None
        return out
