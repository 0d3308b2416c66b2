"""The reference's front ends (core/interface/src/Interface.h:9-129, Agent.h:19-170) on top of CorePyExt: a Botzone bot
(one JSON request per process, or the keep-alive protocol), and the console match between two agents that ends with the
game as Botzone-readable JSON.  The searches behind the agents run on the GPU (K3 / K6 / K8 through core.MCTS); this module
is host-side interop only.

    python -m gomokuai_amd.interface botzone   --agent traditional:5 --ms 960        < request.json
    python -m gomokuai_amd.interface keepalive --agent random:5:5    --iterations 2000
    python -m gomokuai_amd.interface console   --agent traditional:5 --agent2 traditional:7 --ms 1000
    python -m gomokuai_amd.interface botzone   --agent random-mcts:5:5 --replicas 1024 --ms 960     < request.json
    python -m gomokuai_amd.interface botzone   --agent traditional:5 --vcf 16 --ms 960              < request.json
    python -m gomokuai_amd.interface botzone   --agent traditional:5 --vcf 16 --vcf-defend --ms 960 < request.json
    python -m gomokuai_amd.interface botzone   --agent traditional:5 --vcf 16 --vct 2 --ms 960        < request.json
    python -m gomokuai_amd.interface botzone   --agent network:run.pt --leaves 8 --symmetry all --ms 960 < request.json
    python -m gomokuai_amd.interface botzone   --agent pattern-az:5 --leaves 8 --ms 960               < request.json
"""
import datetime
import json
import random
import sys

import numpy as np


def _core():
    from . import core
    return core


def _pos_json(p):
    return {"x": int(p.x), "y": int(p.y)}                          # to_json(Position) (Agent.h:15)


def _pos_from(core, j):
    return core.Position(int(j["x"]), int(j["y"]))                 # from_json (Agent.h:16)


# ---------------- agents (Agent.h:19-170) ----------------
class Agent:
    def name(self):
        raise NotImplementedError

    def get_action(self, board):
        raise NotImplementedError

    def debug_message(self):
        return None

    def sync_with_board(self, board):
        pass

    def reset(self):
        pass


class HumanAgent(Agent):
    """Agent.h:34-51: two hexadecimal coordinates from the input stream; -1 -1 asks the console to take two moves back."""

    def __init__(self, instream=None, outstream=None):
        self.instream, self.outstream = instream or sys.stdin, outstream or sys.stdout

    def name(self):
        return "HumanAgent"

    def get_action(self, board):
        core = _core()
        self.outstream.write("\nInput your move({-1 -1} to revert): ")
        self.outstream.flush()
        tokens = []
        while len(tokens) < 2:
            line = self.instream.readline()
            if not line:
                raise EOFError("HumanAgent: input stream ended")
            tokens += line.split()
        x, y = (int(t, 16) if not t.startswith("-") else -int(t[1:], 16) for t in tokens[:2])
        return core.Position(x, y)


class RandomAgent(Agent):
    """Agent.h:53-62: Board::getRandomMove."""

    def name(self):
        return "RandomAgent"

    def get_action(self, board):
        return board.random_move()


class MCTSAgent(Agent):
    """Agent.h:64-106: MCTS(duration, policy); the move is the argmax of evalState's probabilities (not stepForward's choice),
    the state value goes to stdout like the reference's `cout << state_value`."""

    def __init__(self, policy, milliseconds=None, iterations=None, quiet=False):
        self.policy, self.ms, self.iterations, self.quiet, self.mcts = policy, milliseconds, iterations, quiet, None

    def name(self):
        return "MCTSAgent:%s" % ("%dms" % self.ms if self.iterations is None else "%dit" % self.iterations)

    def sync_with_board(self, board):
        core = _core()
        if self.mcts is None:
            last = board.move_record[-1] if board.move_record else core.Position(-1)
            last_player = -board.status["cur_player"] if board.status["cur_player"] != core.Player.none else core.Player.white
            if self.iterations is not None:
                self.mcts = core.MCTS(c_iterations=int(self.iterations), last_move=last, last_player=last_player, policy=self.policy)
            else:
                self.mcts = core.MCTS(c_duration=datetime.timedelta(milliseconds=self.ms), last_move=last, last_player=last_player, policy=self.policy)
        else:
            self.mcts.sync_with_board(board)

    def get_action(self, board):
        value, probs = self.mcts.eval_state(board)
        if not self.quiet:
            print(value)
        return _core().Position(int(np.argmax(probs)))             # maxCoeff: the first maximum

    def debug_message(self):
        return {"iterations": int(self.mcts.iterations), "duration": "%dms" % int(self.mcts.duration.total_seconds() * 1000)}

    def reset(self):
        if self.mcts is not None:
            self.mcts.reset()


class EnsembleAgent(Agent):
    """An MCTS agent whose search is an ensemble of `replicas` trees of the same root on one GPU (gomokuai_amd/ensemble.py, K13), merged on the
    device; the move is the argmax of evalState's probabilities from the merged visits, as MCTSAgent plays it.  iterations = playouts per
    REPLICA and move; milliseconds = launches of `chunk` playouts per replica until the time has passed (at least one, at most max_playouts
    per move: the arenas are sized for that).  The trees are kept across moves (step) while the board advances by played moves; anything else
    -- a revert, a new game -- starts them anew from the board."""

    def __init__(self, policy, replicas, milliseconds=None, iterations=None, quiet=False, chunk=64, max_playouts=1024, **search_args):
        from .ensemble import EnsembleSearch
        self.ms, self.iterations, self.quiet, self.chunk = milliseconds, iterations, quiet, int(chunk)
        self.max_playouts = int(iterations) if iterations is not None else int(max_playouts)
        search_args.setdefault("playouts_capacity", 3 * self.max_playouts)      # a kept subtree and the new search
        self.search = EnsembleSearch(policy, replicas, **search_args)
        self.moves, self.playouts, self.seconds = None, 0, 0.0

    def name(self):
        return "EnsembleAgent:%s:%dx%s" % (self.search.policy, self.search.replicas, "%dms" % self.ms if self.iterations is None else "%dit" % self.iterations)

    def sync_with_board(self, board):
        moves = [int(p.id) for p in board.move_record]
        known = self.moves
        if known is not None and len(known) < len(moves) <= len(known) + 2 and moves[:len(known)] == known:
            for cell in moves[len(known):]:                        # our own move and the opponent's reply: follow them, subtrees kept
                self.search.step([cell])
        elif known is None or moves != known:
            self.search.set_positions([moves])
        self.moves = moves

    def get_action(self, board):
        import time
        import torch
        t0 = time.perf_counter()
        self.playouts = 0
        if self.iterations is not None:
            self.search.search(self.iterations)
            self.playouts = int(self.iterations)
        else:
            while True:                                            # at least one chunk
                self.search.search(self.chunk)
                torch.cuda.current_stream().synchronize()
                self.playouts += self.chunk
                if (time.perf_counter() - t0) * 1000.0 >= self.ms or self.playouts + self.chunk > self.max_playouts:
                    break
        value, probs = self.search.eval_state()[0]
        self.seconds = time.perf_counter() - t0
        if not self.quiet:
            print(value)
        return _core().Position(int(np.argmax(probs)))             # maxCoeff: the first maximum

    def debug_message(self):
        return {"replicas": self.search.replicas, "playouts_per_replica": self.playouts, "total_playouts": self.playouts * self.search.replicas,
                "duration": "%dms" % int(self.seconds * 1000)}

    def reset(self):
        self.moves = None


class NetworkAgent(Agent):
    """The trained network at play: K7 (lib.AlphaZeroMCTS, one game, `leaves` leaves per step) with `network` at the leaves, the reference's
    PyConvNetAgent (agents/alphazero.py:5-9) on the device.  network: a network.FusedPolicyValueNetwork; symmetry "all" (default) or "random"
    evaluates the leaves through network.symmetric(symmetry) (K22) -- one game's batch is `leaves` rows, so all eight orientations still sit on
    the flat part of the network's cost --, None or "none" leaves the network as it is.  Every get_action takes a fresh root from the board's
    move list, searches `iterations` playouts -- or, with `milliseconds`, chunks of `chunk` playouts until the time has passed (at least one
    chunk, at most max_playouts: the arena is sized for that), as EnsembleAgent does -- and plays the most visited root child, the first
    maximum in cell order (gmk_az_root_choice)."""

    def __init__(self, network, milliseconds=None, iterations=None, leaves=8, symmetry="all", c_puct=5.0, quiet=False, chunk=64, max_playouts=2048):
        if milliseconds is None and iterations is None:
            raise ValueError("NetworkAgent: give milliseconds or iterations")
        if symmetry in (None, "none"):
            self.network, self.symmetry = network, None
        elif symmetry in ("all", "random"):
            if not hasattr(network, "symmetric"):
                raise ValueError("NetworkAgent: symmetry needs a network with symmetric(mode) (network.FusedPolicyValueNetwork)")
            self.network, self.symmetry = network.symmetric(symmetry), symmetry
        else:
            raise ValueError("NetworkAgent: symmetry is \"all\", \"random\" or None, not %r" % (symmetry,))
        self.ms, self.iterations, self.leaves, self.c_puct, self.quiet, self.chunk = milliseconds, iterations, int(leaves), float(c_puct), quiet, int(chunk)
        self.max_playouts = int(iterations) if iterations is not None else int(max_playouts)
        self.tree, self.cells, self.moves, self.playouts, self.seconds, self.value = None, None, [], 0, 0.0, 0.0

    def name(self):
        return "NetworkAgent:%s:L%d:%s" % ("%dms" % self.ms if self.iterations is None else "%dit" % self.iterations, self.leaves, self.symmetry or "none")

    def sync_with_board(self, board):
        self.moves = [int(p.id) for p in board.move_record]

    def get_action(self, board):
        import time
        import torch
        from . import lib as G
        from .selfplay import _arena_nodes, _last_two
        t0 = time.perf_counter()
        self.moves = [int(p.id) for p in board.move_record]
        if self.tree is None:
            self.tree = G.AlphaZeroMCTS(1, node_capacity=_arena_nodes("network", self.max_playouts), c_puct=self.c_puct, leaves=self.leaves)
            self.cells = torch.full((1,), -1, dtype=torch.int16, device="cuda")
        moves, lens = np.zeros((1, G.N), np.uint8), np.array([len(self.moves)], np.int32)
        moves[0, :len(self.moves)] = self.moves
        self.tree.set_roots(G.moves_to_planes(moves, lens), _last_two(moves, lens))
        self.playouts = 0
        with torch.no_grad():
            if self.iterations is not None:
                self.tree.search(self.network, int(self.iterations))
                self.playouts = int(self.iterations)
            else:
                while True:                                        # at least one chunk
                    k = min(self.chunk, self.max_playouts - self.playouts)
                    self.tree.search(self.network, k)
                    torch.cuda.current_stream().synchronize()
                    self.playouts += k
                    if (time.perf_counter() - t0) * 1000.0 >= self.ms or self.playouts >= self.max_playouts:
                        break
        self.tree.root_choice(self.cells)
        cell = int(self.cells.cpu()[0])
        self.value = float(self.tree.root_stats()["root_value"][0])
        self.seconds = time.perf_counter() - t0
        if cell < 0:
            raise RuntimeError("NetworkAgent: the root has no child to play (the game is over)")
        if not self.quiet:
            print(self.value)
        return _core().Position(cell)

    def debug_message(self):
        return {"playouts": self.playouts, "leaves": self.leaves, "symmetry": self.symmetry or "none", "root_value": self.value,
                "duration": "%dms" % int(self.seconds * 1000)}

    def reset(self):
        self.moves = []

    def close(self):
        if self.tree is not None:
            self.tree.close()
            self.tree = None


class PatternEvalAgent(Agent):
    """Agent.h:108-161: no search, the move with the largest Heuristic::EvaluationProbs after DecisiveFilter on the agent's own
    incremental evaluator (Heuristic.hpp:16-28, 94-161); the centre on an empty board.  On the GPU that is the policy head of K6:
    the root priors after one playout of a one-game handle, whose evaluator persists and is synchronised like the reference's.
    The debug message gives the pattern and compound counts before and after the move (K1 on the two positions)."""

    def __init__(self):
        self.tree, self.moves, self.this_move = None, [], None

    def name(self):
        return "PatternEvalAgent"

    def sync_with_board(self, board):
        self.moves = [int(p.id) for p in board.move_record]

    def get_action(self, board):
        from . import lib as G
        core = _core()
        if not self.moves:
            self.this_move = core.Position(7, 7)
        else:
            if self.tree is None:
                self.tree = G.TraditionalMCTS(1, node_capacity=1024)
            self.tree.set_positions([self.moves])
            self.tree.run(1)
            self.this_move = core.Position(int(np.argmax(self.tree.root_stats()["priors"][0])))      # maxCoeff: the first maximum
        return self.this_move

    def debug_message(self):
        from . import lib as G
        after = self.moves + [int(self.this_move.id)]
        moves = np.zeros((2, 64 if len(after) <= 64 else 225), np.uint8)
        moves[0, :len(self.moves)] = self.moves
        moves[1, :len(after)] = after
        planes = G.moves_to_planes(moves, np.array([len(self.moves), len(after)], np.int32))
        totals = G.eval_batch_host(planes)[2]
        def message(t):                                            # Record: white in the low, black in the high 16 bits (Pattern.cpp:390-393)
            return {name: [[int((t[i] >> sh) & 0xFFFF) for i in range(8)], [int((t[8 + i] >> sh) & 0xFFFF) for i in range(3)]]
                    for name, sh in (("black", 16), ("white", 0))}
        return {"before": message(totals[0]), "current": message(totals[1])}

    def reset(self):
        if self.tree is not None:
            self.tree.reset_evaluators()


class VCFAgent(Agent):
    """Any agent with the exact solver for forced wins by continuous fours in front of it (K14, lib.vcf_solve): when the side to move has such
    a win within `depth` own moves and `budget` candidates, its first move is played and the inner agent is not asked; otherwise the inner agent
    decides.  The debug message adds both verdicts, the own one and the opponent's ("what threatens me?", reported only).
    defend=True acts on the opponent's verdict as well (K15, lib.vcf_defend): when the side to move has no forced win and the opponent has one,
    the inner agent is still asked, so that its tree stays in step, but its move stands only if it lies in the best class of cells there is:
    those that HOLD, else those UNKNOWN, else those that LOSE in the greatest number of moves.  Otherwise the cell of that class with the highest
    lib.pattern_policy(filter=False) probability is played, the lowest cell on a tie.  The debug message then adds `vcf_defence`.
    threats=T > 0 adds the forced win by continuous threats (K17, lib.vct_solve: at most T moves that threaten a win by fours, every reply
    that holds answered, then a win by fours).  It is tried last, after the own win by fours and after the defence: only when the inner
    agent's move stands, a WIN's first move is played in its place.  The debug message then adds `vct`, the verdict and `positions`.
    That search comes after the inner agent has spent its time and is bounded by its own limits only, not by a clock: `threats`, `depth`,
    `budget` and `max_positions`, the cap per level (default 512, the setting tools/vct_time.py measured: tens of milliseconds at T <= 3 with
    depth 8 and budget 1000; a root that runs into the cap ends VCT_BUDGET and the inner move is played)."""

    def __init__(self, inner, depth=16, budget=100000, defend=False, threats=0, max_positions=512):
        from . import lib as G
        if not 0 <= int(threats) <= G.VCT_MAX_THREATS:
            raise ValueError("threats must be in 0 .. %d" % G.VCT_MAX_THREATS)
        self.inner, self.depth, self.budget, self.defend = inner, int(depth), int(budget), bool(defend)
        self.threats, self.max_positions = int(threats), int(max_positions)
        self.moves, self.own, self.threat, self.defence, self.vct = [], None, None, None, None

    def name(self):
        return "VCF(" + self.inner.name() + ")"

    def sync_with_board(self, board):
        self.moves = [int(p.id) for p in board.move_record]
        self.inner.sync_with_board(board)

    def reset(self):
        self.inner.reset()

    def _lists(self):
        moves = np.zeros((1, max(1, len(self.moves))), np.uint8)
        moves[0, :len(self.moves)] = self.moves
        return moves, np.array([len(self.moves)], np.int32)

    @staticmethod
    def _verdict(status, move, length, nodes, pv):
        from . import lib as G
        return {"status": G.VCF_STATUS_NAMES[int(status)], "move": int(move), "length": int(length), "nodes": int(nodes),
                "pv": [int(c) for c in pv[:max(0, 2 * int(length) - 1)]]}

    def _solve(self, opponent):
        from . import lib as G
        out = G.vcf_solve(*self._lists(), self.depth, self.budget, opponent=opponent)
        return self._verdict(out["status"][0], out["move"][0], out["length"][0], out["nodes"][0], out["pv"][0])

    def _defend(self, inner_move):
        """The threat and, where it is a WIN, (the cell to play, the report for the debug message); else (None, None)."""
        from . import lib as G
        moves, lens = self._lists()
        out = G.vcf_defend(moves, lens, self.depth, self.budget)
        length = int(out["threat_length"][0])
        self.threat = self._verdict(out["threat_status"][0], out["threat_pv"][0][0] if length else -1, length, out["threat_nodes"][0], out["threat_pv"][0])
        if self.threat["status"] != "WIN":
            return None, None
        verdict, lengths, nodes = out["verdict"][0], out["length"][0].astype(np.int64), out["nodes"][0]
        holds, unknown, loses = (np.flatnonzero(verdict == v) for v in (G.VCF_CELL_HOLDS, G.VCF_CELL_UNKNOWN, G.VCF_CELL_LOSES))
        # a cell was searched unless the threat's own line settled it: such a cell LOSES without a node, and a search that finds a win has one
        report = {"holds": [int(c) for c in holds], "unknown": len(unknown), "loses": len(loses),
                  "searched": len(holds) + len(unknown) + int(np.count_nonzero(nodes[loses])), "overruled": False}
        # no cell is FIVE here: the side to move has no forced win, so it has no completing cell
        longest = loses[lengths[loses] == lengths[loses].max()] if len(loses) else loses
        best = next((cells for cells in (holds, unknown, longest) if len(cells)), None)
        if best is None or inner_move in best:
            return inner_move, report
        probs = G.pattern_policy(moves, lens, filter=False)["probs"][0]
        report["overruled"] = True
        return int(best[int(np.argmax(probs[best]))]), report      # argmax takes the first of equals: the lowest cell

    def _threats(self):
        """The verdict of lib.vct_solve for the side to move, as the debug message carries it."""
        from . import lib as G
        out = G.vct_solve(*self._lists(), self.depth, self.budget, max_threats=self.threats, max_positions=self.max_positions)
        cells = [int(c) for c in out["pv"][0]]
        return {"status": G.VCT_STATUS_NAMES[int(out["status"][0])], "move": int(out["move"][0]), "threats": int(out["threats"][0]),
                "positions": int(out["positions"][0]), "pv": cells[:cells.index(255)] if 255 in cells else cells}

    def get_action(self, board):
        self.moves = [int(p.id) for p in board.move_record]
        self.own, self.threat, self.defence, self.vct = self._solve(False), None, None, None
        if self.own["status"] == "WIN":
            return _core().Position(self.own["move"])
        action = self.inner.get_action(board)
        if self.defend:
            cell, self.defence = self._defend(int(action.id))
            if self.defence is not None and self.defence["overruled"]:
                return _core().Position(cell)
        if self.threats > 0:
            self.vct = self._threats()
            if self.vct["status"] == "WIN":
                return _core().Position(self.vct["move"])
        return action

    def debug_message(self):
        if self.own is None:
            return self.inner.debug_message()
        if self.threat is None:
            self.threat = self._solve(True)
        inner = None if self.own["status"] == "WIN" else self.inner.debug_message()      # a forced win was played: the inner agent was not asked
        message = dict(inner) if isinstance(inner, dict) else {"inner": inner}
        message["vcf"], message["vcf_opponent"] = self.own, self.threat
        if self.defence is not None:
            message["vcf_defence"] = self.defence
        if self.vct is not None:
            message["vct"] = self.vct
        return message


def make_agent(spec, milliseconds=960, iterations=None, quiet=False, replicas=1, seed=None, vcf=0, vcf_defend=False, vct=0, leaves=8, symmetry="all"):
    """'random', 'human', 'pattern', 'random-mcts[:c_puct[:c_rollouts]]', 'traditional[:c_puct]', 'poolrave[:c_puct[:c_bias]]',
    'network:PATH[:c_puct]' (NetworkAgent on the weights network.load_weights reads from PATH, with `leaves` leaves per step and the
    leaves evaluated under `symmetry`: "all", "random" or "none"; `replicas` does not apply to it),
    'pattern-az[:c_puct]' (the same search with no network: NetworkAgent over network.PatternEvaluator(), the pattern heuristic as K7's prior
    and value (K23), with `leaves` leaves per step; `symmetry` and `replicas` do not apply to it).
    replicas > 1 turns the three MCTS kinds into an EnsembleAgent of that many trees per position ('traditional' with the reference's root
    noise, alpha 0.05 / epsilon 0.25: its search has no other source of difference); replicas = 1 builds the agents as ever.
    vcf = D > 0 puts the forced-win solver in front of the agent (VCFAgent, depth D); 'human' and 'random' stay as they are.
    vcf_defend=True (with vcf > 0 only) lets that agent also refuse moves that lose to the opponent's forced win (VCFAgent(defend=True)).
    vct = T in 1 .. lib.VCT_MAX_THREATS (with vcf > 0 only) lets it also play a forced win by at most T threat moves (VCFAgent(threats=T)); that
    search runs after the agent's own and is not bounded by `milliseconds`.  0 builds today's agents."""
    if vcf_defend and vcf <= 0:
        raise ValueError("vcf_defend needs vcf > 0")
    if vct and vcf <= 0:
        raise ValueError("vct needs vcf > 0")
    from . import lib as G
    if not 0 <= vct <= G.VCT_MAX_THREATS:
        raise ValueError("vct must be in 0 .. %d" % G.VCT_MAX_THREATS)
    if vcf > 0 and spec.split(":")[0] not in ("human", "random"):
        return VCFAgent(make_agent(spec, milliseconds, iterations, quiet, replicas, seed, leaves=leaves, symmetry=symmetry), depth=vcf, defend=vcf_defend, threats=vct)
    core = _core()
    kind, *args = spec.split(":")
    if kind == "network":
        if symmetry not in (None, "none", "all", "random"):
            raise ValueError("symmetry must be \"all\", \"random\" or \"none\"")
        if not 1 <= int(leaves) <= G.AZ_MAX_LEAVES:
            raise ValueError("leaves must be in 1 .. %d" % G.AZ_MAX_LEAVES)
        if not args or not args[0] or len(args) > 2:
            raise ValueError("the network agent is 'network:PATH[:c_puct]'")
        from .network import FusedPolicyValueNetwork, load_weights
        module = load_weights(args[0]).cuda().eval()
        return NetworkAgent(FusedPolicyValueNetwork(module), milliseconds=None if iterations is not None else milliseconds, iterations=iterations,
                            leaves=leaves, symmetry=symmetry, c_puct=float(args[1]) if len(args) > 1 else 5.0, quiet=quiet)
    if kind == "pattern-az":
        if not 1 <= int(leaves) <= G.AZ_MAX_LEAVES:
            raise ValueError("leaves must be in 1 .. %d" % G.AZ_MAX_LEAVES)
        if len(args) > 1:
            raise ValueError("the pattern search agent is 'pattern-az[:c_puct]'")
        from .network import PatternEvaluator
        return NetworkAgent(PatternEvaluator(), milliseconds=None if iterations is not None else milliseconds, iterations=iterations,
                            leaves=leaves, symmetry=None, c_puct=float(args[0]) if args and args[0] else 5.0, quiet=quiet)
    num = [float(a) for a in args]
    if kind == "random":
        return RandomAgent()
    if kind == "human":
        return HumanAgent()
    if kind == "pattern":
        return PatternEvalAgent()
    if replicas > 1 and kind in ("random-mcts", "traditional", "poolrave"):
        extra = {} if seed is None else {"seed": int(seed)}
        if kind == "random-mcts":
            return EnsembleAgent("random", replicas, milliseconds, iterations, quiet, c_puct=num[0] if num else 5.0, c_rollouts=int(num[1]) if len(num) > 1 else 5, **extra)
        if kind == "traditional":
            return EnsembleAgent("traditional", replicas, milliseconds, iterations, quiet, c_puct=num[0] if num else 5.0, root_noise=(0.05, 0.25), **extra)
        return EnsembleAgent("poolrave", replicas, milliseconds, iterations, quiet, c_puct=num[0] if num else 2.0, **extra)
    if kind == "random-mcts":
        policy = core.RandomPolicy(num[0] if num else 5.0, int(num[1]) if len(num) > 1 else 5)
    elif kind == "traditional":
        policy = core.TraditionalPolicy(num[0] if num else 5.0)
    elif kind == "poolrave":
        policy = core.PoolRAVEPolicy(num[0] if num else 2.0, num[1] if len(num) > 1 else 0.0)
    else:
        raise ValueError("unknown agent '%s'" % spec)
    return MCTSAgent(policy, milliseconds=milliseconds, iterations=iterations, quiet=quiet)


# ---------------- front ends (Interface.h:9-129) ----------------
def _restore(core, board, request):
    """requests has one entry more than responses; {"x": -1, "y": -1} (we play black) is rejected by applyMove: a no-op."""
    responses = request.get("responses", [])
    for i in range(len(responses)):
        board.apply_move(_pos_from(core, request["requests"][i]), False)
        board.apply_move(_pos_from(core, responses[i]), False)
    board.apply_move(_pos_from(core, request["requests"][len(responses)]), False)


def botzone_interface(agent, instream=None, outstream=None):
    """Interface.h:9-31: one request, one response."""
    core = _core()
    instream, outstream = instream or sys.stdin, outstream or sys.stdout
    board = core.Board()
    _restore(core, board, json.loads(instream.read()))
    agent.sync_with_board(board)
    out = {"response": _pos_json(agent.get_action(board)), "debug": agent.debug_message()}
    outstream.write(json.dumps(out) + "\n")
    outstream.flush()
    return 0


def keep_alive_botzone_interface(agent, instream=None, outstream=None, max_turns=None):
    """Interface.h:33-62: the first line restores the position, every later line is the opponent's move; each answer is
    followed by the keep-running marker.  Ends when the input ends (the reference loops until it is killed)."""
    core = _core()
    instream, outstream = instream or sys.stdin, outstream or sys.stdout
    board = core.Board()
    turn = 0
    while max_turns is None or turn < max_turns:
        line = instream.readline()
        if not line:
            break
        if not line.strip():
            continue
        request = json.loads(line)
        if turn == 0:
            _restore(core, board, request if "requests" in request else {"requests": [request], "responses": []})
        else:
            board.apply_move(_pos_from(core, request), False)
        agent.sync_with_board(board)
        board.apply_move(agent.get_action(board))
        out = {"response": _pos_json(board.move_record[-1]), "debug": agent.debug_message()}
        outstream.write(json.dumps(out) + "\n>>>BOTZONE_REQUEST_KEEP_RUNNING<<<\n")
        outstream.flush()
        turn += 1
    return 0


def board_text(board):
    states = board.move_states
    core = _core()
    black, white = states[core.Player.black], states[core.Player.white]
    rows = ["  " + " ".join("%X" % x for x in range(15))]
    for y in range(15):
        rows.append("%X " % y + " ".join("x" if black[y][x] else "o" if white[y][x] else "." for x in range(15)))
    return "\n".join(rows) + "\n"


def console_interface(agent0, agent1, outstream=None, black_player=None):
    """Interface.h:64-127: a match on the console; returns 1 for a tie, else 0, and prints the record from the winner's point of view
    as Botzone JSON ({-1,-1} first in requests when the winner played black)."""
    core = _core()
    out = outstream or sys.stdout
    board = core.Board()
    if black_player is None:
        black_player = random.randrange(2)
    agents = [agent0, agent1]
    index = {core.Player.white: 1 - black_player, core.Player.black: black_player}
    out.write("black: %d.%s\nwhite: %d.%s\n\n%s\n-------------------------\n" % (
        index[core.Player.black], agents[index[core.Player.black]].name(), index[core.Player.white], agents[index[core.Player.white]].name(), board_text(board)))
    cur = core.Player.black
    while True:
        i = index[cur]
        agent = agents[i]
        agent.sync_with_board(board)
        move = agent.get_action(board)
        if move.x == -1 and move.y == -1:
            board.revert_move(2)
            out.write(board_text(board))
            continue
        result = board.apply_move(move)
        if result == cur:
            out.write("Invalid move: %s\n" % str(move))
            continue
        out.write("\n%d.%s's move: %s:\n\n%s\nDebug Messages:%s\n-------------------------\n" % (i, agent.name(), str(move), board_text(board), json.dumps(agent.debug_message())))
        if result == core.Player.none:
            break
        cur = result
    winner = board.status["winner"]
    if winner != core.Player.none:
        out.write("\nGame end. Winner: %d.%s\nRecord JSON:\n" % (index[winner], agents[index[winner]].name()))
    else:
        out.write("\nTie.\n")
    records = {"requests": [], "responses": []}
    for i, p in enumerate(board.move_record):
        if i == 0 and winner == core.Player.black:
            records["requests"].append({"x": -1, "y": -1})
        if (i % 2 == 0) == (winner == core.Player.black):
            records["responses"].append(_pos_json(p))
        else:
            records["requests"].append(_pos_json(p))
    out.write(json.dumps(records) + "\n")
    out.flush()
    return int(winner == core.Player.none)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["botzone", "keepalive", "console"])
    ap.add_argument("--agent", default="traditional:5",
                    help="random, human, pattern, random-mcts[:c_puct[:c_rollouts]], traditional[:c_puct], poolrave[:c_puct[:c_bias]], "
                         "network:PATH[:c_puct], pattern-az[:c_puct] (the network agent's search over the pattern heuristic; honours --leaves)")
    ap.add_argument("--agent2", default="traditional:7", help="console mode: the second agent")
    ap.add_argument("--ms", type=int, default=960, help="search time per move (the reference's default constraint)")
    ap.add_argument("--iterations", type=int, default=None, help="playouts per move instead of a time budget")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--replicas", type=int, default=1, help="trees per position for the MCTS agents (root-parallel ensemble, merged on the GPU); --iterations then counts playouts per replica")
    ap.add_argument("--vcf", type=int, default=0, metavar="DEPTH", help="put the exact forced-win solver (continuous fours, up to DEPTH own moves) in front of the agents; 0: off")
    ap.add_argument("--vcf-defend", action="store_true", help="with --vcf: also refuse moves that lose to the opponent's forced win by fours, as far as any cell holds")
    ap.add_argument("--vct", type=int, default=0, metavar="T", help="with --vcf: also play a forced win by at most T moves that threaten a win by fours (fours and threes); 0: off.  This search runs after the agent's own and is not bounded by --ms")
    ap.add_argument("--leaves", type=int, default=8, metavar="L", help="the network and pattern-az agents: leaves per search step (1 .. 8)")
    ap.add_argument("--symmetry", choices=["all", "random", "none"], default="all", help="the network agent: evaluate every leaf averaged over the board's eight orientations, in one orientation picked per position, or as it stands")
    args = ap.parse_args(argv)
    if args.vcf_defend and args.vcf <= 0:
        ap.error("--vcf-defend needs --vcf DEPTH")
    if args.vct and args.vcf <= 0:
        ap.error("--vct needs --vcf DEPTH")
    from . import lib as G
    if not 0 <= args.vct <= G.VCT_MAX_THREATS:
        ap.error("--vct takes 0 .. %d" % G.VCT_MAX_THREATS)
    if not 1 <= args.leaves <= G.AZ_MAX_LEAVES:
        ap.error("--leaves takes 1 .. %d" % G.AZ_MAX_LEAVES)
    if args.seed is not None:
        _core().set_seed(args.seed)
        random.seed(args.seed)
    quiet = args.mode != "console"                                  # a bot's stdout carries the protocol only
    agent = make_agent(args.agent, args.ms, args.iterations, quiet, replicas=args.replicas, seed=args.seed, vcf=args.vcf, vcf_defend=args.vcf_defend, vct=args.vct, leaves=args.leaves, symmetry=args.symmetry)
    if args.mode == "botzone":
        return botzone_interface(agent)
    if args.mode == "keepalive":
        return keep_alive_botzone_interface(agent)
    return console_interface(agent, make_agent(args.agent2, args.ms, args.iterations, quiet, replicas=args.replicas, seed=args.seed, vcf=args.vcf, vcf_defend=args.vcf_defend, vct=args.vct, leaves=args.leaves, symmetry=args.symmetry))


if __name__ == "__main__":
    sys.exit(main())
