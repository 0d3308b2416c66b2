"""A plain Python / numpy restatement of K7's search with several leaves per step and virtual loss ("Several leaves per
step"), for the tests.  It shares no code with the kernels and does not go through oracle/: the tree is a set of lists, np.float32
running means follow backup's form q + (value - q) / float32(visits), np.float64 does the PUCB, and the five-in-a-row test is its own.

The rules (one tree; the kernels run one wavefront per game):
  select step   min(leaves, quota) descents, one after the other.  A descent is Default::Select with, per child i of a node with
                real statistics (N, Q) and in-flight count v,
                    q_eff = Q if v == 0 else (Q * N - v) / (N + v)        n_i = N + v + 1        sqrt_n = sqrt(N_parent + v_parent)
                    score = q_eff + c_puct * p_i * sqrt_n / n_i           (float64, left to right; first maximum, strict '>' from -1.0)
                terminal leaf: the real value is backed up at once, quota -= 1, next descent;
                childless leaf with v > 0 (it waits for the network already): a collision, the step's descents end, nothing is counted;
                otherwise v += 1 from the root to the leaf, the leaf is the k-th pending leaf, quota -= 1.
  expand step   for k in order: children (probability not 0, cell free, ascending cells) appended at n_nodes -- or status |= 2 and the
                playout is dropped when they do not fit --, -value backed up unless dropped, v -= 1 from the leaf up.
With leaves = 1 this is the reference's MCTS with an external evaluator, bit for bit."""
import numpy as np

N = 225
NO_NODE = -1
STATUS_ARENA_FULL, STATUS_ILLEGAL_STEP = 2, 4


# six roots of 0 .. 12 stones (the first moves of six synthetic games), black first
OPENINGS = [[], [168, 196, 2], [132, 130, 103, 161, 102, 131], [29, 58, 41, 13, 125, 27, 95, 28, 54],
            [20, 52, 3, 19, 189, 64, 218, 223, 5, 4, 159, 127], [107, 137]]
_c = lambda y, x: y * 15 + x
# black has five through (7, 11): the root is terminal
WON = [_c(7, 7), _c(0, 0), _c(7, 8), _c(0, 2), _c(7, 9), _c(0, 4), _c(7, 10), _c(0, 6), _c(7, 11)]
# eight stones, black to move with an open four: a five one ply below the root on either side of it, and white's replies in between
OPEN_FOUR = [_c(7, 6), _c(0, 0), _c(7, 7), _c(0, 2), _c(7, 8), _c(0, 4), _c(7, 9), _c(0, 6)]


def surrogate(states):
    """tests/test_az_gpu.surrogate, copied: states uint8/float [6, 15, 15] -> (value, probs): deterministic, exactly reproducible, with zero
    probabilities on some empty cells and non-zero ones on some occupied cells."""
    s = np.asarray(states).reshape(6, 225).astype(np.int64)
    code = s[0] * 3 + s[1] * 5 + s[3] * 7 + s[4] * 11 + s[5]
    idx = np.arange(225, dtype=np.int64)
    h = (int((code * (idx + 1)).sum()) * 2654435761 + idx * 40503 * (int(code.sum()) + 1)) % 65536
    probs = ((h % 1021) + 1).astype(np.float32) / np.float32(1024.0)
    probs[h % 7 == 0] = 0.0
    value = np.float32((int(h.sum()) % 2001) - 1000) / np.float32(1000.0)
    return value, probs


def sharpened(states):
    """The surrogate with its probabilities squared five times in float32 (the 32nd power): a peaked prior, under which descents of one step
    meet again below the root (the plain surrogate is so flat that every playout opens a new root child)."""
    value, probs = surrogate(states)
    for _ in range(5):
        probs = (probs * probs).astype(np.float32)
    return value, probs


def uniform(states):
    return np.float32(0.0), np.full(N, np.float32(1.0) / np.float32(225.0), dtype=np.float32)


def _five_through(colour_cells, cell):
    """five or more stones of one colour in a line through `cell` (colour_cells: bool[225] of that colour, `cell` included)"""
    x0, y0 = cell % 15, cell // 15
    for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1)):
        run = 1
        for sign in (1, -1):
            x, y = x0 + sign * dx, y0 + sign * dy
            while 0 <= x < 15 and 0 <= y < 15 and colour_cells[y * 15 + x]:
                run += 1
                x, y = x + sign * dx, y + sign * dy
        if run >= 5:
            return True
    return False


def _planes(moves):
    """Board.encoded_states of the position after `moves` (black first): own stones, the opponent's, empties, the last move, the one
    before, all ones iff black is to move"""
    out = np.zeros((6, N), dtype=np.uint8)
    white_to_move = len(moves) % 2 == 1
    for i, c in enumerate(moves):
        out[0 if (i % 2 == 1) == white_to_move else 1, c] = 1
    out[2] = 1 - out[0] - out[1]
    if len(moves) >= 1:
        out[3, moves[-1]] = 1
    if len(moves) >= 2:
        out[4, moves[-2]] = 1
    out[5] = 0 if white_to_move else 1
    return out.reshape(6, 15, 15)


class LeavesSearch:
    """One game's tree.  moves: the cells played so far, black first (the root position)."""

    def __init__(self, moves, evaluator, c_puct=5.0, leaves=1, node_capacity=1 << 16):
        self.moves = [int(c) for c in moves]
        self.evaluator, self.c_puct, self.leaves, self.cap = evaluator, float(c_puct), int(leaves), int(node_capacity)
        self.status, self.quota = 0, 0
        self.steps, self.leaves_per_step, self.terminal_playouts, self.collisions, self.max_depth = 0, [], 0, 0, 0
        self._new_root()

    # ---- the tree: parallel lists, node 0 is the root ----
    def _new_root(self):
        self.visits, self.value, self.prior = [0], [np.float32(0.0)], [np.float32(1.0)]
        self.parent, self.first, self.nkids, self.cell, self.inflight = [NO_NODE], [0], [0], [self.moves[-1] if self.moves else 255], [0]

    @property
    def n_nodes(self):
        return len(self.visits)

    def _backup(self, node, value):
        value = np.float32(value)
        while node != NO_NODE:
            self.visits[node] += 1
            q = self.value[node]
            self.value[node] = np.float32(q + np.float32(value - q) / np.float32(self.visits[node]))
            node, value = self.parent[node], np.float32(-value)

    def _descend(self):
        node, path = 0, []
        while self.nkids[node]:
            a, b = self.first[node], self.first[node] + self.nkids[node]
            n = np.array(self.visits[a:b], dtype=np.float64)
            v = np.array(self.inflight[a:b], dtype=np.float64)
            q = np.array(self.value[a:b], dtype=np.float32).astype(np.float64)
            p = np.array(self.prior[a:b], dtype=np.float32).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                q_eff = np.where(v == 0, q, (q * n - v) / (n + v))
            sqrt_n = np.sqrt(np.float64(self.visits[node] + self.inflight[node]))
            score = q_eff + self.c_puct * p * sqrt_n / (n + v + 1.0)
            best = int(np.argmax(score))                         # the first maximum
            if not score[best] > -1.0:
                best = 0
            node = a + best
            path.append(self.cell[node])
        return node, path

    def _ended(self, moves):
        """(is the game over, winner +1 black / -1 white / 0)"""
        if moves:
            mover_white = (len(moves) - 1) % 2 == 1
            own = np.zeros(N, dtype=bool)
            own[[c for i, c in enumerate(moves) if (i % 2 == 1) == mover_white]] = True
            if _five_through(own, moves[-1]):
                return True, (-1 if mover_white else 1)
        return len(moves) == N, 0

    def select_step(self):
        """-> the pending leaves' feature planes, uint8[n_pending, 6, 15, 15]"""
        self.pending = []
        rows = []
        for _ in range(min(self.leaves, self.quota)):
            node, path = self._descend()
            moves = self.moves + path
            self.max_depth = max(self.max_depth, len(path))
            ended, winner = self._ended(moves)
            if ended:
                node_player = 1 if len(moves) % 2 == 1 else -1   # the one who made the last move
                self._backup(node, np.float32(node_player * winner))
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
            rows.append(_planes(moves))
            self.quota -= 1
        self.steps += 1
        self.leaves_per_step.append(len(self.pending))
        return np.stack(rows) if rows else np.zeros((0, 6, 15, 15), dtype=np.uint8)

    def expand_step(self, values, probs):
        for k, (leaf, moves) in enumerate(self.pending):
            occupied = set(moves)
            pr = np.asarray(probs[k], dtype=np.float32)
            take = [c for c in range(N) if pr[c] != 0.0 and c not in occupied]
            dropped = False
            if take:
                if self.n_nodes + len(take) > self.cap:
                    self.status |= STATUS_ARENA_FULL
                    dropped = True
                else:
                    self.first[leaf], self.nkids[leaf] = self.n_nodes, len(take)
                    for c in take:
                        self.visits.append(0); self.value.append(np.float32(0.0)); self.prior.append(np.float32(pr[c]))
                        self.parent.append(leaf); self.first.append(0); self.nkids.append(0); self.cell.append(c); self.inflight.append(0)
            if not dropped:
                self._backup(leaf, -np.float32(values[k]))
            up = leaf
            while up != NO_NODE:
                self.inflight[up] -= 1
                up = self.parent[up]
        self.pending = []

    def step(self):
        states = self.select_step()
        out = [self.evaluator(s) for s in states]
        self.expand_step([v for v, _ in out], [p for _, p in out])

    def search(self, playouts):
        self.quota += int(playouts)
        while self.quota > 0:
            self.step()

    # ---- MCTS::stepForward() / stepForward(move): the subtree of the chosen child becomes the tree ----
    def reroot(self, move=None):
        a, n = self.first[0], self.nkids[0]
        child = NO_NODE
        if move is None:
            if n:
                child = a + int(np.argmax(np.array(self.visits[a:a + n])))       # first maximum in child (= cell) order
                move = self.cell[child]
        else:
            move = int(move)
            for i in range(a, a + n):
                if self.cell[i] == move:
                    child = i
        if move is None:
            return None                                          # a childless root: nothing to play
        if not (0 <= move < N) or move in self.moves:
            self.status |= STATUS_ILLEGAL_STEP
            return None
        self.moves.append(move)
        if child == NO_NODE:
            self._new_root()
            return move
        old = (self.visits, self.value, self.prior, self.first, self.nkids, self.cell)
        self.visits, self.value, self.prior = [old[0][child]], [old[1][child]], [old[2][child]]
        self.parent, self.first, self.nkids, self.cell, self.inflight = [NO_NODE], [0], [old[4][child]], [old[5][child]], [0]
        source = [child]
        i = 0
        while i < len(source):                                  # level by level, children consecutive
            s = source[i]
            if old[4][s]:
                self.first[i] = len(source)
                for c in range(old[3][s], old[3][s] + old[4][s]):
                    source.append(c)
                    self.visits.append(old[0][c]); self.value.append(old[1][c]); self.prior.append(old[2][c])
                    self.parent.append(i); self.first.append(0); self.nkids.append(old[4][c]); self.cell.append(old[5][c]); self.inflight.append(0)
            i += 1
        return move

    def root_stats(self):
        out = {"visits": np.zeros(N, np.uint32), "values": np.zeros(N, np.float32), "priors": np.zeros(N, np.float32)}
        for i in range(self.first[0], self.first[0] + self.nkids[0]):
            out["visits"][self.cell[i]], out["values"][self.cell[i]], out["priors"][self.cell[i]] = self.visits[i], self.value[i], self.prior[i]
        out.update(root_visits=self.visits[0], root_value=np.float32(self.value[0]), n_nodes=self.n_nodes, status=self.status)
        return out

    def depth(self):
        """plies below the root of the deepest node"""
        d = [0] * self.n_nodes
        for i in range(1, self.n_nodes):                         # parents come before their children
            d[i] = d[self.parent[i]] + 1
        return max(d)
