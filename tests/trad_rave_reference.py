"""Restatement of TraditionalPolicy(c_puct, use_rave) (core/lib/include/policies/Traditional.h:17-69 with the backup switched to
RAVE::BackPropogate<true>, MonteCarlo.hpp:113-184; agents/mcts.py:44-47) in Python over the CPU oracle's EXPORTED evaluator.

TEST INFRASTRUCTURE ONLY.  oracle/go_trad.c restates TraditionalPolicy with BackPropogate<false> and has no RAVE switch; this module
repeats its playout step for step -- Heuristic's probabilities, DecisiveFilter and value in go_trad.c's float order (sum225, sqrtf
normalisation, the 0.6f / 0.4f literals, tanh in double), Heuristic::CachedApplyMove / CachedRevertMove on ONE persistent evaluator
(whose board history the next playout inherits), the kept tree of MCTS::run / stepForward and Default::AddNoise from the
counter-based sampler -- and adds the all-moves-as-first backup against the leaf position.  With use_rave=False it must equal
go_trad bit for bit (tests/test_trad_rave_reference.py); with use_rave=True it is what the device's gmk_trad_run_rave is held to.
Each backup level is one vectorised numpy step: the first maximum of the scores is np.argmax's."""
import ctypes as C
import math

import numpy as np

from oracle import oracle as O

N = O.N
BLACK, WHITE = O.BLACK, O.WHITE
F32 = np.float32
S4, SL3, STO44, STO43, STO33, SEND = range(6)
# Heuristic::DecisiveFilter's AutomataTable[anti][state] = (next state, next anti) (Heuristic.hpp:103-107)
_TABLE = (((S4, 1), (STO44, 0), (SL3, 1), (STO43, 1), (STO33, 1), (SEND, 0)),
          ((SL3, 0), (STO44, 1), (STO43, 0), (STO33, 0), (SEND, 0), (SEND, 1)))
LIVE4, DEAD4, LIVE3, DEAD3, PT_SIZE = 7, 6, 5, 4, 9


def _group1(player):
    return 1 if player == BLACK else 0


def _group2(favour, perspective):
    return ((favour == BLACK) << 1) | (perspective == BLACK)


def sum225(x):
    """go_trad.c's sum225: 64 strided partial sums, a binary tree inside each group of 16, then (g0 + g1) + (g2 + g3); float32."""
    p = x[0:64] + x[64:128]
    p = p + x[128:192]
    p[:N - 192] = p[:N - 192] + x[192:N]
    p = p.reshape(4, 16)
    for s in (8, 4, 2, 1):
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
    return (p[0, 0] + p[1, 0]) + (p[2, 0] + p[3, 0])


def normalize225(x):
    z = sum225(x * x)
    if z > F32(0):
        x = x / np.sqrt(z)
    return x


def density_weight(density, player):
    g = _group1(player)
    n = np.maximum(density[g, 0], 0).astype(F32)
    w = np.maximum(density[g, 1], 0).astype(F32)
    return normalize225((F32(3) * w) / (F32(1) + F32(2) * n))


def evaluation_probs(scores, density, nrec, player):
    if nrec != 0:
        self_worthy = scores[_group2(player, player)].astype(F32) * density_weight(density, player)
        rival_anti = scores[_group2(-player, player)].astype(F32) * density_weight(density, -player)
        return normalize225(F32(0.6) * self_worthy + F32(0.4) * rival_anti)
    probs = np.zeros(N, F32)
    probs[7 * 15 + 7] = 1
    return probs


def evaluation_value(scores, density, player):
    self_worthy = sum225(scores[_group2(player, player)].astype(F32) * density_weight(density, player))
    rival_worthy = sum225(scores[_group2(-player, -player)].astype(F32) * density_weight(density, -player))
    return F32(math.tanh((1.2 * float(self_worthy) - float(rival_worthy)) / 500.0))


def decisive_filter(pdist, cdist, cur, probs):
    state, anti = S4, 0
    while state != SEND:
        player = -cur if anti else cur
        if state == S4:
            cand = [(LIVE4, player), (DEAD4, player)]
        elif state == SL3:
            cand = [(LIVE3, player)]
        else:
            cand = [(PT_SIZE + (STO33 - state), player)]
        head = 0
        while head < len(cand):
            pattern, pl = cand[head]
            field = int(pdist[N, pattern] if pattern < PT_SIZE else cdist[N, pattern - PT_SIZE])
            if (field >> (16 * _group1(pl))) & 0xFFFF:
                if anti and state != S4:
                    cand.append((DEAD3, -pl))
                break
            head += 1
        if head < len(cand):
            keep = np.zeros(N, bool)
            for pattern, pl in cand[head:]:
                field = pdist[:N, pattern] if pattern < PT_SIZE else cdist[:N, pattern % PT_SIZE]
                keep |= ((field >> np.uint32(8 * _group2(pl, cur))) & np.uint32(0xFF)) != 0
            probs = np.where(keep, probs, F32(0)).astype(F32)
            probs = normalize225(probs)
            state = SEND
        else:
            state, anti = _TABLE[anti][state]
    return probs


class TradRAVEReference:
    """go_trad's search object (one persistent evaluator, a tree of nodes with a current child order) plus the AMAF statistics."""

    def __init__(self, c_puct=5.0, use_rave=False, c_bias=0.0):
        self.L = O.lib()
        self.c_puct, self.use_rave, self.c_bias = float(c_puct), bool(use_rave), float(c_bias)
        self.ev = C.c_void_p(self.L.go_eval_new())
        self.bptr = self.L.go_eval_board(self.ev)
        self.board = self.bptr.contents
        self.states = np.ctypeslib.as_array(self.board.states)          # [player + 1][cell], a view of the evaluator's board
        self.record = np.ctypeslib.as_array(self.board.record)
        self.scores = np.zeros((4, N), np.int32)
        self.density = np.zeros((2, 2, N), np.int32)
        self.pdist = np.zeros((N + 1, 8), np.uint32)
        self.cdist = np.zeros((N + 1, 3), np.uint32)
        self.evaluator_updates = 0
        self.cached = self.init = 0
        self.have_tree = False
        self.noise = None
        self._alloc(1 << 12)
        self.n_nodes = self.n_kids = 0
        self.root = -1

    def __del__(self):
        if getattr(self, "ev", None) is not None:
            self.L.go_eval_free(self.ev)
            self.ev = None

    # ---- tree storage ----
    def _alloc(self, cap):
        old = getattr(self, "parent", None)
        fields = {"parent": np.int32, "pos": np.int16, "player": np.int8, "value": F32, "prior": F32, "visits": np.int64,
                  "first": np.int32, "n": np.int32, "amaf_visits": np.int64, "amaf_value": F32}
        for k, dt in fields.items():
            a = np.zeros(cap, dt)
            if old is not None:
                a[:len(getattr(self, k))] = getattr(self, k)
            setattr(self, k, a)
        kids = np.zeros(cap, np.int32)
        if old is not None:
            kids[:len(self.kids)] = self.kids
        self.kids = kids

    def _new_nodes(self, parent, cells, player, priors):
        k = len(cells)
        while self.n_nodes + k > len(self.parent) or self.n_kids + k > len(self.kids):
            self._alloc(2 * len(self.parent))
        ids = np.arange(self.n_nodes, self.n_nodes + k)
        self.parent[ids] = parent
        self.pos[ids] = cells
        self.player[ids] = player
        self.value[ids] = 0
        self.prior[ids] = priors
        self.visits[ids] = 0
        self.amaf_visits[ids] = 0
        self.amaf_value[ids] = 0
        self.first[ids] = 0
        self.n[ids] = 0
        self.n_nodes += k
        return ids

    def _new_node(self, parent, pos, player, prior):
        return int(self._new_nodes(parent, np.array([pos]), player, np.array([prior], F32))[0])

    def _expand(self, node, probs):
        cells = np.nonzero(probs != 0)[0]
        ids = self._new_nodes(node, cells, -int(self.player[node]), probs[cells])
        self.first[node] = self.n_kids
        self.kids[self.n_kids:self.n_kids + len(ids)] = ids
        self.n_kids += len(ids)
        self.n[node] = len(ids)

    def children(self, node):
        return self.kids[self.first[node]:self.first[node] + self.n[node]]

    # ---- the evaluator ----
    def _apply(self, move):
        self.L.go_eval_apply(self.ev, int(move), None)

    def _cached_apply(self, move):
        """Heuristic::CachedApplyMove (Heuristic.hpp:165-189), as go_trad.c's cached_apply_move"""
        nrec = self.board.nrec
        if self.cached == nrec or self.record[self.cached] != move:
            if (nrec - self.cached) % (1 << 64) > self.cached:
                rec = self.record[:self.cached].copy()
                self.L.go_eval_reset(self.ev)
                for m in rec:
                    self._apply(m)
                    self.evaluator_updates += 1
            else:
                self.evaluator_updates += nrec - self.cached
                self.L.go_eval_revert(self.ev, nrec - self.cached)
            self._apply(move)
            self.evaluator_updates += 1
            if self.cached < self.board.nrec:
                self.cached += 1
        else:
            self.cached += 1

    def _cached_revert(self):
        """Heuristic::CachedRevertMove (Heuristic.hpp:192-200): only the inner board goes back"""
        self.L.go_board_revert(self.bptr, self.board.nrec - self.cached)
        self.cached = self.init

    def _eval_sync(self, moves):
        """Evaluator::syncWithBoard (Pattern.cpp:356-368)"""
        i = 0
        while i < len(moves):
            if i < self.board.nrec:
                if self.record[i] == moves[i]:
                    i += 1
                    continue
                self.evaluator_updates += self.board.nrec - i
                self.L.go_eval_revert(self.ev, self.board.nrec - i)
            self._apply(moves[i])
            self.evaluator_updates += 1
            i += 1
        self.evaluator_updates += self.board.nrec - i
        self.L.go_eval_revert(self.ev, self.board.nrec - i)

    # ---- the playout ----
    def _back_propagate(self, node, value):
        """RAVE::BackPropogate<use_rave> (MonteCarlo.hpp:154-184); the board is the evaluator's, i.e. the leaf position"""
        value = F32(value)
        while node >= 0:
            k = int(self.n[node])
            if k:
                f = int(self.first[node])
                ids = self.kids[f:f + k]
                score = (self.c_puct * self.prior[ids].astype(np.float64)) * math.sqrt(float(self.visits[node])) / (self.visits[ids] + 1).astype(np.float64)
                if self.use_rave:
                    hit = ids[self.states[self.player[ids].astype(np.int64) + 1, self.pos[ids].astype(np.int64)] != 0]
                    self.amaf_visits[hit] += 1
                    aq = self.amaf_value[hit]
                    self.amaf_value[hit] = aq + ((-value) - aq) / self.amaf_visits[hit].astype(F32)
                    w = np.sqrt(800.0 / (3 * self.visits[ids].astype(np.float64) + 800.0))
                    score = score + ((1 - w) * self.value[ids].astype(np.float64) + w * self.amaf_value[ids].astype(np.float64))
                else:
                    score = score + self.value[ids].astype(np.float64)
                m = int(np.argmax(score))
                self.kids[f], self.kids[f + m] = self.kids[f + m], self.kids[f]
            self.visits[node] += 1
            self.value[node] = self.value[node] + (value - self.value[node]) / F32(self.visits[node])
            node = int(self.parent[node])
            value = -value

    def _playout(self):
        node = self.root
        while self.n[node]:
            node = int(self.kids[self.first[node]])
            self._cached_apply(int(self.pos[node]))
        if not self.L.go_eval_check_end(self.ev):
            cur = int(self.board.cur_player)
            L, ev = self.L, self.ev
            L.go_eval_get_scores(ev, self.scores.ctypes.data)
            L.go_eval_get_density(ev, self.density.ctypes.data)
            L.go_eval_get_pattern_dist(ev, self.pdist.ctypes.data)
            L.go_eval_get_compound_dist(ev, self.cdist.ctypes.data)
            probs = evaluation_probs(self.scores, self.density, self.board.nrec, cur)
            probs = decisive_filter(self.pdist, self.cdist, cur, probs)
            value = evaluation_value(self.scores, self.density, cur)
            self._expand(node, probs)
            node_value = -value
        else:
            node_value = F32(int(self.player[node]) * int(self.board.winner))
        self._back_propagate(node, node_value)
        self._cached_revert()

    # ---- the searches ----
    def search(self, moves, playouts):
        """go_trad_search: a fresh root at the position `moves`, the evaluator synchronised from wherever it was"""
        moves = [int(m) for m in moves]
        self.n_nodes = self.n_kids = 0
        self.root = self._new_node(-1, moves[-1] if moves else -1, BLACK if len(moves) & 1 else WHITE, 1.0)
        self.init = len(moves)
        self._eval_sync(moves)
        self.cached = self.init
        for _ in range(playouts):
            self._playout()

    def set_noise(self, alpha, epsilon, seed, game_id=0):
        """Default::AddNoise before every kept-tree run, from the counter-based sampler (gomoku_noise.h)"""
        self.noise = (float(alpha), float(epsilon), int(seed), int(game_id))

    def _add_noise(self, stones):
        if self.noise is None or not self.noise[0] > 0 or self.n[self.root] == 0:
            return
        alpha, eps, seed, game_id = self.noise
        ids = self.children(self.root)
        prior = np.zeros(N, F32)
        prior[self.pos[ids]] = self.prior[ids]
        self.L.go_noise_mix225(prior.ctypes.data, alpha, eps, game_id, stones, seed)
        self.prior[ids] = prior[self.pos[ids]]

    def _step_forward_move(self, move):
        ids = self.children(self.root)
        hit = ids[self.pos[ids] == move]
        nxt = int(hit[0]) if len(hit) else self._new_node(-1, move, -int(self.player[self.root]), 1.0)
        self.parent[nxt] = -1
        self.root = nxt

    def run(self, moves, playouts):
        """go_trad_run: MCTS::runPlayouts on the kept tree (syncWithBoard, AddNoise, Policy::prepare, the playouts)"""
        moves = [int(m) for m in moves]
        if not self.have_tree:
            self.n_nodes = self.n_kids = 0
            self.root = self._new_node(-1, -1, WHITE, 1.0)
            self.have_tree = True
        i = 0
        while i < len(moves) and moves[i] != self.pos[self.root]:
            i += 1
        i = 0 if i == len(moves) else i + 1
        for m in moves[i:]:
            self._step_forward_move(m)
        self._add_noise(len(moves))
        self.init = len(moves)
        self._eval_sync(moves)
        self.cached = self.init
        for _ in range(playouts):
            self._playout()

    def step_forward(self):
        """MCTS::stepForward(): the most visited child, first maximum in the current order; returns the root's move"""
        ids = self.children(self.root)
        if len(ids):
            best = int(ids[int(np.argmax(self.visits[ids]))])
            self.parent[best] = -1
            self.root = best
        return int(self.pos[self.root])

    # ---- what the device reports ----
    def root_children(self):
        """(visits, values, priors, amaf_visits, amaf_values by cell, the move stepForward() would play or -1)"""
        ids = self.children(self.root)
        out = [np.zeros(N, np.uint32), np.zeros(N, F32), np.zeros(N, F32), np.zeros(N, np.uint32), np.zeros(N, F32)]
        cells = self.pos[ids].astype(np.int64)
        for a, src in zip(out, (self.visits, self.value, self.prior, self.amaf_visits, self.amaf_value)):
            a[cells] = src[ids]
        best = int(self.pos[ids[int(np.argmax(self.visits[ids]))]]) if len(ids) else -1
        return (*out, best)

    @property
    def root_visits(self):
        return int(self.visits[self.root])

    @property
    def root_value(self):
        return F32(self.value[self.root])

    def subtree_size(self):
        """nodes reachable from the root: the device compacts a kept subtree, go_trad never frees"""
        count, frontier = 0, [self.root]
        while frontier:
            count += len(frontier)
            frontier = [int(c) for nd in frontier for c in self.children(nd)]
        return count
