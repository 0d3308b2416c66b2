"""A plain Python restatement of K7 with proven wins and losses carried up the tree (include/gomoku_hip.h, "K7 + proofs"), for the tests:
az_vcf_reference.VcfLeavesSearch plus
    prove(X, s)     X has a proof: stop.  proof(X) = s, proved += 1.  No parent P: stop.  s == LOSES: prove(P, WINS).  s == WINS: prove(P, LOSES)
                    only when P has a child for every free cell of its position and every child of P is WINS.
    starts          (a) a descent that ends at a node with a five: prove(node, LOSES); (b) a pending leaf the solver answers WIN, once its child
                    exists: prove(leaf, WINS)
    descent         a node below the root that has a proof ends the descent: +1 is backed up from it for LOSES, -1 for WINS, stops += 1, quota - 1,
                    no mark, no row, no collision test.  Among children: the first LOSES child if there is one; otherwise children marked WINS are
                    left out of the maximum unless all are marked.  Nothing beats -1.0: the first child, marked or not.
    root choice     the first LOSES child; otherwise the most visited child among those not WINS with a visit; otherwise the old rule
With proof off the bits are neither read nor written (they stay and travel through reroot).  It imports nothing from the package."""
import numpy as np

import az_leaves_reference as R
import az_vcf_reference as A
import vcf_reference as V

N = 225
NONE, WINS, LOSES = 0, 1, 2
NO_NODE = R.NO_NODE


class ProofSearch(A.VcfLeavesSearch):
    """VcfLeavesSearch with proofs.  proof = False: VcfLeavesSearch itself, field for field."""

    def __init__(self, moves, evaluator, vcf_depth=0, vcf_budget=64, proof=False, **kw):
        self.proof_on = bool(proof)
        super().__init__(moves, evaluator, vcf_depth, vcf_budget, **kw)

    def reset_counters(self):
        super().reset_counters()
        self.proved, self.stops = 0, 0
        self.floor_picks = 0                                     # descents' levels at which nothing beat -1.0 (not a counter of the handle)

    def _new_root(self):
        super()._new_root()
        self.proof = [NONE]

    def depth_of(self, node):
        d = 0
        while self.parent[node] != NO_NODE:
            node, d = self.parent[node], d + 1
        return d

    def prove(self, x, s):
        while self.proof[x] == NONE:
            self.proof[x] = s
            self.proved += 1
            p = self.parent[x]
            if p == NO_NODE:
                return
            if s == WINS:
                a, n = self.first[p], self.nkids[p]
                if n != N - (len(self.moves) + self.depth_of(p)):
                    return                                       # Default::Expand dropped a free cell: an untried reply
                if any(self.proof[i] != WINS for i in range(a, a + n)):
                    return
            x, s = p, (LOSES if s == WINS else WINS)

    def _descend(self):
        """-> (node, path, the proof the descent stopped at or NONE)"""
        node, path = 0, []
        while True:
            if self.proof_on and node != 0 and self.proof[node] != NONE:
                return node, path, self.proof[node]
            if not self.nkids[node]:
                return node, path, NONE
            a, b = self.first[node], self.first[node] + self.nkids[node]
            n = np.array(self.visits[a:b], dtype=np.float64)
            v = np.array(self.inflight[a:b], dtype=np.float64)
            q = np.array(self.value[a:b], dtype=np.float32).astype(np.float64)
            p = np.array(self.prior[a:b], dtype=np.float32).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                q_eff = np.where(v == 0, q, (q * n - v) / (n + v))
            sqrt_n = np.sqrt(np.float64(self.visits[node] + self.inflight[node]))
            score = q_eff + self.c_puct * p * sqrt_n / (n + v + 1.0)
            lose = []
            if self.proof_on:
                pr = np.array(self.proof[a:b])
                lose = np.nonzero(pr == LOSES)[0]
                if (pr != WINS).any():
                    score = np.where(pr == WINS, -np.inf, score)
            best = int(np.argmax(score))                         # the first maximum
            if not score[best] > -1.0:
                best = 0
                self.floor_picks += 1
            if len(lose):
                best = int(lose[0])
            node = a + best
            path.append(self.cell[node])

    def select_step(self):
        self.pending = []
        rows = []
        for _ in range(min(self.leaves, self.quota)):
            node, path, stopped = self._descend()
            moves = self.moves + path
            self.max_depth = max(self.max_depth, len(path))
            if stopped != NONE:
                self._backup(node, np.float32(1.0 if stopped == LOSES else -1.0))
                self.quota -= 1
                self.stops += 1
                continue
            ended, winner = self._ended(moves)
            if ended:
                node_player = 1 if len(moves) % 2 == 1 else -1
                self._backup(node, np.float32(node_player * winner))
                if self.proof_on and winner != 0:
                    self.prove(node, LOSES)
                self.quota -= 1
                self.terminal_playouts += 1
                continue
            if self.inflight[node] > 0:
                self.collisions += 1
                break
            up = node
            while up != NO_NODE:
                self.inflight[up] += 1
                up = self.parent[up]
            self.pending.append((node, moves))
            rows.append(R._planes(moves))
            self.quota -= 1
        self.steps += 1
        self.leaves_per_step.append(len(self.pending))
        return np.stack(rows) if rows else np.zeros((0, 6, 15, 15), dtype=np.uint8)

    def expand_step(self, values, probs):
        """After answers(): self.verdicts holds the pending leaves' verdicts when the solver is on."""
        solved = self.vcf_depth > 0 and len(self.verdicts) == len(self.pending)
        for k, (leaf, moves) in enumerate(self.pending):
            occupied = set(moves)
            pr = np.asarray(probs[k], dtype=np.float32)
            take = [c for c in range(N) if pr[c] != 0.0 and c not in occupied]
            dropped = False
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
                    if self.proof_on and solved and self.verdicts[k]["status"] == V.WIN:
                        self.prove(leaf, WINS)
            if not dropped:
                self._backup(leaf, -np.float32(values[k]))
            up = leaf
            while up != NO_NODE:
                self.inflight[up] -= 1
                up = self.parent[up]
        self.pending = []

    # ---- the root ----
    def plain_choice(self):
        """the most visited root child with a visit, first maximum in cell order: its node, or NO_NODE"""
        a, n = self.first[0], self.nkids[0]
        vis = self.visits[a:a + n]
        return a + int(np.argmax(vis)) if n and max(vis) > 0 else NO_NODE

    def choice(self):
        """the root child gmk_az_root_choice / gmk_az_advance would play: its node, or NO_NODE"""
        a, n = self.first[0], self.nkids[0]
        if self.proof_on:
            for i in range(a, a + n):
                if self.proof[i] == LOSES:
                    return i
            best, best_v = NO_NODE, 0
            for i in range(a, a + n):
                if self.proof[i] != WINS and self.visits[i] > best_v:
                    best, best_v = i, self.visits[i]
            if best != NO_NODE:
                return best
        return self.plain_choice()

    def choice_cell(self):
        c = self.choice()
        return -1 if c == NO_NODE else self.cell[c]

    def reroot(self, move=None):
        a, n = self.first[0], self.nkids[0]
        child = NO_NODE
        if move is None:
            if n:
                child = self.choice()
                if child == NO_NODE:
                    child = a                                    # gmk_az_step(NULL) on unvisited children: the first
                move = self.cell[child]
        else:
            move = int(move)
            for i in range(a, a + n):
                if self.cell[i] == move:
                    child = i
        if move is None:
            return None
        if not (0 <= move < N) or move in self.moves:
            self.status |= R.STATUS_ILLEGAL_STEP
            return None
        self.moves.append(move)
        if child == NO_NODE:
            self._new_root()
            return move
        old = (self.visits, self.value, self.prior, self.first, self.nkids, self.cell, self.proof)
        self.visits, self.value, self.prior, self.proof = [old[0][child]], [old[1][child]], [old[2][child]], [old[6][child]]
        self.parent, self.first, self.nkids, self.cell, self.inflight = [NO_NODE], [0], [old[4][child]], [old[5][child]], [0]
        source = [child]
        i = 0
        while i < len(source):                                  # level by level, children consecutive
            s = source[i]
            if old[4][s]:
                self.first[i] = len(source)
                for c in range(old[3][s], old[3][s] + old[4][s]):
                    source.append(c)
                    self.visits.append(old[0][c]); self.value.append(old[1][c]); self.prior.append(old[2][c]); self.proof.append(old[6][c])
                    self.parent.append(i); self.first.append(0); self.nkids.append(old[4][c]); self.cell.append(old[5][c]); self.inflight.append(0)
            i += 1
        return move

    def root_proofs(self):
        out = {"root": self.proof[0], "children": np.zeros(N, np.int8)}
        for i in range(self.first[0], self.first[0] + self.nkids[0]):
            out["children"][self.cell[i]] = self.proof[i]
        return out

    def path_to(self, node):
        """the cells from the root to `node`"""
        path = []
        while self.parent[node] != NO_NODE:
            path.append(self.cell[node])
            node = self.parent[node]
        return path[::-1]


# ---- full minimax of a nearly full board, for the soundness test ----
def minimax(moves):
    """+1 the side to move wins, -1 it loses, 0 a draw, with best play, from the position after `moves` (black first): exhaustive."""
    black = np.zeros(N, dtype=bool)
    white = np.zeros(N, dtype=bool)
    black[moves[0::2]] = True
    white[moves[1::2]] = True
    memo = {}

    def solve(stones, last):
        own = white if (stones - 1) % 2 == 1 else black          # the side that made the last move
        if last is not None and R._five_through(own, last):
            return -1
        if stones == N:
            return 0
        key = (black.tobytes(), white.tobytes())                 # a five needs its last stone: transpositions agree on everything else
        mine = white if stones % 2 == 1 else black
        best = -1
        for c in range(N):
            if black[c] or white[c]:
                continue
            mine[c] = True
            k2 = (c, key)
            r = memo.get(k2)
            if r is None:
                r = -solve(stones + 1, c)
                memo[k2] = r
            mine[c] = False
            best = max(best, r)
            if best == 1:
                break
        return best

    return solve(len(moves), moves[-1] if moves else None)
