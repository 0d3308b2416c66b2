"""K13: one position searched with the whole chip -- root-parallel tree ensembles.

`replicas` copies of the same root are searched as consecutive games of ONE batched handle (K3 BatchedMCTS, K6 TraditionalMCTS, K6 + RAVE
TraditionalRAVEMCTS, K8 PoolRAVEMCTS), each with its own arena and its own random streams, and a device kernel merges the replicas' root
tables into one (gmk_mcts_ensemble_merge / gmk_trad_ensemble_merge, include/gomoku_hip.h: integer sums, so the same bits in any order).
No search kernel is involved in the merge and none changes; `replicas=1` is the handle as it is used without this module.

The network search (K7) is out of scope here: one position there is served by AlphaZeroMCTS(leaves=), several leaves per step of one tree.
"""
import numpy as np

from . import lib as G

POLICIES = ("random", "traditional", "traditional-rave", "poolrave")
_DETERMINISTIC = ("traditional", "traditional-rave")          # no random numbers in the search: replicas differ through root noise only


class EnsembleSearch:
    """EnsembleSearch(policy, replicas, ...): several positions ("ensembles"), each searched by `replicas` trees.

    policy        "random" (K3), "traditional" (K6), "traditional-rave" (K6 + RAVE), "poolrave" (K8)
    c_puct        default 5.0, PoolRAVE 2.0 (the reference's); c_rollouts: K3's rollouts per leaf
    seed          key of every random stream; first_game_id: replica r of ensemble id k searches as game first_game_id + k * replicas + r,
                  so an ensemble's result does not depend on which other ensembles share the handle
    root_noise    None or (alpha, epsilon): Default::AddNoise on every replica's root, drawn by the counter-based sampler
                  (GMK_NOISE_SAMPLER_COUNTER, set here), keyed by the replica's game id.  AddNoise does nothing on a root without children, so
                  the first search of a root runs one playout (which expands it), mixes the noise in ONCE, and runs the rest; later
                  searches of the same root continue without drawing again.
    playouts_capacity / node_capacity    arena size per replica, as the lib classes have them (node_capacity = playouts_capacity * 225 + 1)

    K6 and K6 + RAVE searches are deterministic: their replicas would be copies of one tree, so replicas > 1 without root_noise is refused.
    K3 and K8 replicas differ by their rollout streams and need no noise."""

    def __init__(self, policy, replicas, c_puct=None, c_rollouts=5, seed=G.DEFAULT_SEED, first_game_id=0, root_noise=None,
                 playouts_capacity=1000, node_capacity=None):
        if policy not in POLICIES:
            raise ValueError("EnsembleSearch: unknown policy '%s' (one of %s)" % (policy, ", ".join(POLICIES)))
        replicas = int(replicas)
        if not 1 <= replicas <= G.ENSEMBLE_MAX_GROUP:
            raise ValueError("EnsembleSearch: 1 <= replicas <= %d" % G.ENSEMBLE_MAX_GROUP)
        if root_noise is not None and not (len(root_noise) == 2 and root_noise[0] > 0):
            raise ValueError("EnsembleSearch: root_noise is None or (alpha > 0, epsilon)")
        if policy in _DETERMINISTIC and replicas > 1 and root_noise is None:
            raise ValueError("EnsembleSearch: the '%s' search is deterministic -- its replicas differ only through root noise: give root_noise=(alpha, epsilon)" % policy)
        self.policy, self.replicas = policy, replicas
        self.c_puct = float(c_puct) if c_puct is not None else (2.0 if policy == "poolrave" else 5.0)
        self.c_rollouts, self.seed, self.first_game_id = int(c_rollouts), int(seed), int(first_game_id)
        self.root_noise = None if root_noise is None else (float(root_noise[0]), float(root_noise[1]))
        self.node_capacity = int(node_capacity) if node_capacity is not None else int(playouts_capacity) * 225 + 1
        self.tree = None
        self.n_ensembles = 0

    def close(self):
        if self.tree is not None:
            self.tree.close()
            self.tree = None

    # ---- the handle ----
    def _make_tree(self, n):
        if self.policy == "random":
            t = G.BatchedMCTS(n, c_puct=self.c_puct, c_rollouts=self.c_rollouts, seed=self.seed, node_capacity=self.node_capacity)
        elif self.policy == "traditional":
            t = G.TraditionalMCTS(n, node_capacity=max(256, self.node_capacity), c_puct=self.c_puct)
        elif self.policy == "traditional-rave":
            t = G.TraditionalRAVEMCTS(n, node_capacity=max(256, self.node_capacity), c_puct=self.c_puct)
        else:
            t = G.PoolRAVEMCTS(n, node_capacity=max(256, self.node_capacity), c_puct=self.c_puct, seed=self.seed, first_game_id=self.first_game_id)
        if self.root_noise is not None:
            t.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
        return t

    def set_positions(self, move_lists, ensemble_ids=None):
        """One move list (cells, black first) per ensemble; ensemble_ids (default 0, 1, ...) number them for the random streams.  Creates the
        handle of len(move_lists) * replicas games, or reuses the one there is when the size is the same; every tree starts anew."""
        import torch
        n_ens = len(move_lists)
        ids = list(range(n_ens)) if ensemble_ids is None else [int(i) for i in ensemble_ids]
        if n_ens < 1 or len(ids) != n_ens:
            raise ValueError("EnsembleSearch.set_positions: one id per move list, at least one list")
        n, R = n_ens * self.replicas, self.replicas
        if self.tree is None or self.tree.n != n:
            self.close()
            self.tree = self._make_tree(n)
        self.n_ensembles = n_ens
        moves = np.zeros((n, 225), np.uint8)
        lens = np.zeros(n, np.int32)
        for k, ml in enumerate(move_lists):
            moves[k * R:(k + 1) * R, :len(ml)] = np.asarray(ml, dtype=np.uint8)
            lens[k * R:(k + 1) * R] = len(ml)
        relative = np.repeat(np.asarray(ids, dtype=np.int64) * R, R) + np.tile(np.arange(R, dtype=np.int64), n_ens)
        if self.policy == "random":
            last = np.array([ml[-1] if len(ml) else -1 for ml in move_lists for _ in range(R)], dtype=np.int16)
            self.tree.set_roots(G.moves_to_planes(moves, lens), last, self.first_game_id)
            self.tree.set_game_ids((relative + self.first_game_id).astype(np.uint32))
        else:
            self.tree.set_game_ids(relative.astype(np.uint32))
            self.tree.set_positions(moves, lens)
        self.stones = [len(ml) for ml in move_lists]
        self._noise_due = self.root_noise is not None
        dev = torch.device("cuda")
        self._cells_per_game = torch.empty(n, dtype=torch.int16, device=dev)
        if self.policy == "random":                  # the record outputs gmk_mcts_step asks for
            self._rec = (torch.zeros((n, 225), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                         torch.zeros(n, dtype=torch.int8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        else:
            self._verdict = torch.zeros(n, dtype=torch.int32, device=dev)          # MATCH_MOVED for every replica

    def _stream(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def _run(self, playouts):
        if playouts > 0:
            self.tree.run(playouts, stream=self._stream())

    def _add_noise(self):
        import torch
        alpha, eps = self.root_noise
        torch.cuda.current_stream().synchronize()    # (the K6 / K8 noise launch goes on the default stream)
        if self.policy == "random":
            self.tree.add_root_noise(alpha, eps, stream=self._stream())
        else:
            self.tree.add_root_noise(alpha, eps, seed=self.seed, first_game_id=self.first_game_id, stream=self._stream())

    def search(self, playouts):
        """`playouts` more playouts for every replica, on the current stream (no wait).  With root_noise, the first search of a root draws it."""
        playouts = int(playouts)
        if self._noise_due and playouts > 0:
            self._run(1)
            self._add_noise()
            self._noise_due = False
            playouts -= 1
        self._run(playouts)

    def _merge(self, **outputs):
        self.tree.ensemble_merge(self.replicas, stream=self._stream(), **outputs)

    def merged(self):
        """The merged root tables: {"visits" u32[E,225], "values" f32[E,225], "cell" i16[E], "root_visits" u32[E], "root_value" f32[E],
        "status" i32[E]} (host arrays; waits for the stream)."""
        import torch
        E, dev = self.n_ensembles, torch.device("cuda")
        visits = torch.empty((E, 225), dtype=torch.int32, device=dev)
        values = torch.empty((E, 225), dtype=torch.float32, device=dev)
        cells = torch.empty(E, dtype=torch.int16, device=dev)
        root_visits = torch.empty(E, dtype=torch.int32, device=dev)
        root_value = torch.empty(E, dtype=torch.float32, device=dev)
        status = torch.empty(E, dtype=torch.int32, device=dev)
        self._merge(visits=visits, values=values, cells=cells, cells_per_game=self._cells_per_game, root_visits=root_visits, root_value=root_value, status=status)
        return {"visits": visits.cpu().numpy().view(np.uint32), "values": values.cpu().numpy(), "cell": cells.cpu().numpy(),
                "root_visits": root_visits.cpu().numpy().view(np.uint32), "root_value": root_value.cpu().numpy(), "status": status.cpu().numpy()}

    def eval_state(self):
        """Per ensemble (root value, pi float32[225]): MCTS::evalState on the merged table (pi from the merged visits, gmk_visits_to_pi)."""
        m = self.merged()
        return [(float(m["root_value"][k]), G.visits_to_pi(m["visits"][k], self.stones[k])) for k in range(self.n_ensembles)]

    def step(self, cells=None):
        """MCTS::stepForward for every replica, subtrees kept: to its ensemble's merged cell (None), or to cells[k] for ensemble k.  The merged
        cells go from the merge kernel to the step kernel in device memory."""
        import torch
        if cells is None:
            self._merge(cells_per_game=self._cells_per_game)
        else:
            given = torch.as_tensor(np.asarray(cells, dtype=np.int16).reshape(self.n_ensembles), device=torch.device("cuda"))
            self._cells_per_game.copy_(torch.repeat_interleave(given, self.replicas))
        if self.policy == "random":
            moves, lens, winner, unfinished = self._rec
            self.tree.step(self._cells_per_game.data_ptr(), moves.data_ptr(), None, lens.data_ptr(), winner.data_ptr(), unfinished.data_ptr(),
                           reuse_subtree=True, stream=self._stream())
        else:
            self.tree.step_device(self._cells_per_game, self._verdict, fresh_root=False, stream=self._stream())
        self.stones = [s + 1 for s in self.stones]
        self._noise_due = self.root_noise is not None
