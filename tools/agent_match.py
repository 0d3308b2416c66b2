#!/usr/bin/env python3
"""Playing strength of one agent against another, measured: matches of selfplay.play_agent_match in batches of paired games, until the
sequential test of gomokuai_amd.rating decides or the games run out.

  python tools/agent_match.py --first network,playouts=64,gumbel=16 --second network,playouts=64 [--games 64] [--max-games 512]
                              [--elo0 0] [--elo1 30] [--alpha 0.05] [--beta 0.05] [--opening-plies 4] [--max-moves 225] [--seed 7] [--out FILE]
  python tools/agent_match.py --suite [--games 64] [--max-games 256] [--out profiles/agent_match.json]
  python tools/agent_match.py --suite-pattern [--games 64] [--max-games 128] [--out profiles/agent_match_pattern.json]

A side is `kind[:first][,key=value ...]`:
  network[:PATH]     K7.  PATH: weights for network.load_weights; without it the weights of --weights, and without those
                     PolicyValueNetwork(seed=S) with the side's seed=S (default 0).  Keys: playouts, c_puct, leaves, vcf=DEPTH/BUDGET, proof,
                     vcf_defend, symmetry=all|random, gumbel=M[/C_VISIT/C_SCALE], sample_plies, sample_power, node_capacity, precision=f32|bf16.
  pattern            K7 over network.PatternEvaluator (K23): the pattern heuristic as prior and value, no weights.  Keys: a network side's but
                     weights, seed, precision and symmetry (the heuristic is not averaged over orientations), and filter=0|1, norm=sum|l2.
  traditional:P      K6 at P playouts (traditional_rave:P with RAVE), rave:P K8, random:P K3.  Keys: c_puct, c_rollouts.
Batch b plays the games first_game_id + b * games onwards, so no opening and no random stream is used twice; per batch and in total the tool
reports rating.summary (paired), the Elo interval, the LLR of H0: elo0 against H1: elo1, and the seconds per ply and group.

--suite records the comparisons the README's rows point to, each against plain K7 at the same playouts: K16 + K18, K19 on top, leaves=8,
symmetry "all", Gumbel at 32 and 64 playouts, bf16 against f32, and K7 against traditional_mcts at 400.
--suite-pattern records the first strength figures of K7 with the pattern evaluator (paired openings, no noise): at 64 and at 400 playouts
against traditional_mcts at 400, K16 + K18 on top of it, leaves=8 against leaves=1, and Gumbel at 32 playouts against plain.
A run without trained weights (seed networks) speaks for the exact tactical options, the symmetry average and the search shape; it does not
speak for what a trained prior would change.  No figure here is a bar: they are measurements."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_KINDS = {"traditional": ("traditional_mcts", {}), "traditional_rave": ("traditional_mcts", {"use_rave": True}), "rave": ("rave_mcts", {}), "random": ("random_mcts", {})}
_FLAGS = ("proof", "vcf_defend")
_INTS = ("playouts", "leaves", "sample_plies", "sample_power", "node_capacity", "seed")


def parse_side(text):
    """'kind[:first][,key=value ...]' -> {"kind", "kwargs" (what the agent spec takes, without the network), "weights", "seed", "precision"}.  Needs no GPU."""
    head, *items = [t.strip() for t in text.split(",")]
    kind, _, first = head.partition(":")
    side = {"text": text, "weights": None, "seed": 0, "precision": "f32"}
    if kind in _KINDS:
        name, kw = _KINDS[kind]
        kw = dict(kw, c_puct=2.0 if kind == "rave" else 5.0)
        if first:
            kw["c_iterations"] = int(first)
        for item in items:
            key, _, value = item.partition("=")
            if key not in ("c_puct", "c_rollouts", "c_iterations"):
                raise ValueError("agent_match: %s takes c_puct, c_rollouts and c_iterations, not '%s'" % (kind, key))
            kw[key] = float(value) if key == "c_puct" else int(value)
        return dict(side, kind=name, kwargs=kw)
    if kind not in ("network", "pattern"):
        raise ValueError("agent_match: a side is network, pattern, %s -- not '%s'" % (", ".join(_KINDS), kind))
    kw = {}
    side["weights"] = first or None
    if kind == "pattern":
        if first:
            raise ValueError("agent_match: the pattern side has no weights to name ('%s')" % first)
        side["pattern"] = {"filter": True, "norm": "sum"}
    for item in items:
        key, _, value = item.partition("=")
        if kind == "pattern" and key in ("seed", "precision", "symmetry"):
            raise ValueError("agent_match: a pattern side does not take '%s'" % key)
        if kind == "pattern" and key in ("filter", "norm"):
            side["pattern"][key] = (value in ("", "1", "true", "True")) if key == "filter" else value
        elif key in _FLAGS:
            kw[key] = value in ("", "1", "true", "True")
        elif key == "seed":
            side["seed"] = int(value)
        elif key == "precision":
            side["precision"] = value
        elif key in _INTS:
            kw[key] = int(value)
        elif key == "c_puct":
            kw[key] = float(value)
        elif key == "symmetry":
            kw[key] = value
        elif key == "vcf":
            depth, _, budget = value.partition("/")
            kw[key] = (int(depth), int(budget or 64))
        elif key == "gumbel":
            parts = value.split("/")
            kw[key] = (int(parts[0]), float(parts[1]) if len(parts) > 1 else 50.0, float(parts[2]) if len(parts) > 2 else 1.0)
        else:
            raise ValueError("agent_match: a network side does not take '%s'" % key)
    return dict(side, kind="network", kwargs=kw)                     # (a pattern side is K7 too: its evaluator stands where the network does)


SUITE = [
    ("K16 + K18: fours solved at the leaves, proofs carried up", "network,playouts=64,vcf=10/64,proof", "network,playouts=64"),
    ("K16 + K18 + K19: lost replies proven as well", "network,playouts=64,vcf=10/64,proof,vcf_defend", "network,playouts=64"),
    ("leaves=8: eight leaves per step with virtual loss", "network,playouts=64,leaves=8", "network,playouts=64"),
    ("K22: the average over the eight symmetries", "network,playouts=64,symmetry=all", "network,playouts=64"),
    ("K21: Gumbel root search, 32 playouts", "network,playouts=32,gumbel=16", "network,playouts=32"),
    ("K21: Gumbel root search, 64 playouts", "network,playouts=64,gumbel=16", "network,playouts=64"),
    ("bf16 trunk against f32", "network,playouts=64,precision=bf16", "network,playouts=64"),
    ("K7 against traditional_mcts at 400", "network,playouts=64", "traditional:400"),
]

SUITE_PATTERN = [
    ("K7(pattern) at 64 against traditional_mcts at 400", "pattern,playouts=64", "traditional:400"),
    ("K7(pattern) at 400 against traditional_mcts at 400", "pattern,playouts=400", "traditional:400"),
    ("K7(pattern) + K16 + K18 against K7(pattern), 64 playouts", "pattern,playouts=64,vcf=10/64,proof", "pattern,playouts=64"),
    ("K7(pattern) leaves=8 against leaves=1, 64 playouts", "pattern,playouts=64,leaves=8", "pattern,playouts=64"),
    ("K7(pattern) Gumbel at 32 playouts against plain", "pattern,playouts=32,gumbel=16", "pattern,playouts=32"),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--first")
    ap.add_argument("--second")
    ap.add_argument("--suite", action="store_true")
    ap.add_argument("--suite-pattern", action="store_true", help="the comparisons of K7 with the pattern evaluator (K23)")
    ap.add_argument("--weights", default=None, help="weights (network.load_weights) of every network side that names none")
    ap.add_argument("--games", type=int, default=64, help="games per batch (even: the games are paired)")
    ap.add_argument("--max-games", type=int, default=512)
    ap.add_argument("--elo0", type=float, default=0.0)
    ap.add_argument("--elo1", type=float, default=30.0)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--beta", type=float, default=0.05)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--max-moves", type=int, default=225)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--first-game-id", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    suite = SUITE_PATTERN if a.suite_pattern else SUITE if a.suite else None
    if (a.suite and a.suite_pattern) or (suite is not None) == bool(a.first or a.second) or (suite is None and not (a.first and a.second)):
        ap.error("give --first and --second, or --suite, or --suite-pattern")
    if a.games < 2 or a.games % 2 or a.max_games < a.games:
        ap.error("--games is even and at most --max-games")
    comparisons = suite if suite is not None else [("%s against %s" % (a.first, a.second), a.first, a.second)]
    parsed = [(title, parse_side(f), parse_side(s)) for title, f, s in comparisons]      # every refusal before the device is touched

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd import network, rating, selfplay
    G.init(0)
    networks = {}

    def agent(side):
        """The agent spec of a parsed side; networks are shared between the sides and comparisons that name the same one"""
        if side["kind"] != "network":
            return side["kind"], side["kwargs"]
        if "pattern" in side:
            key = ("pattern", side["pattern"]["filter"], side["pattern"]["norm"])
            if key not in networks:
                networks[key] = network.PatternEvaluator(filter=key[1], norm=key[2])
            return "network", dict(side["kwargs"], network=networks[key])
        weights = side["weights"] or a.weights
        key = (weights, None if weights else side["seed"], side["precision"])
        if key not in networks:
            module = network.load_weights(weights) if weights else network.PolicyValueNetwork(seed=side["seed"])
            networks[key] = network.FusedPolicyValueNetwork(module.cuda().eval(), precision=side["precision"])
        return "network", dict(side["kwargs"], network=networks[key])

    def figures(scores):
        s = rating.summary(scores, paired=True)
        lo, mid, hi = rating.elo_interval(s["score"], s["stderr"])
        test = rating.sprt(scores, a.elo0, a.elo1, a.alpha, a.beta, paired=True)
        finite = lambda v: v if math.isfinite(v) else ("inf" if v > 0 else "-inf")
        return dict(s, elo=finite(mid), elo_interval=[finite(lo), finite(hi)], llr=test["llr"], decision=test["decision"])

    rows = []
    for title, f, s in parsed:
        first, second = agent(f), agent(s)
        scores, batches, seconds, plies = np.zeros(0), [], 0.0, 0
        while len(scores) < a.max_games:
            n = min(a.games, a.max_games - len(scores))
            n -= n % 2
            if n == 0:
                break
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec, _, got = selfplay.play_agent_match(n, first, second, seed=a.seed, first_game_id=a.first_game_id + len(scores), opening_plies=a.opening_plies,
                                                    paired=True, max_moves=a.max_moves)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            lens = rec.lens.cpu().numpy()
            group_plies = sum(int(lens[g["games"]].max()) - a.opening_plies for g in rec.groups if len(g["games"]))
            seconds, plies = seconds + dt, plies + group_plies
            scores = np.concatenate([scores, got])
            batches.append(dict(figures(got), first_game_id=a.first_game_id + len(scores) - n, seconds_per_group_ply=dt / max(group_plies, 1),
                                mean_length=float(lens.mean()), unfinished=int(sum(g["unfinished"] for g in rec.groups)), overflow=bool(rec.overflow)))
            total = figures(scores)
            print("%-58s %4d games  score %.3f +- %.3f  elo %s [%s, %s]  llr %+.2f  %s" % (title[:58], len(scores), total["score"], total["stderr"], *[
                v if isinstance(v, str) else "%+.0f" % v for v in (total["elo"], *total["elo_interval"])], total["llr"], total["decision"] or ""), flush=True)
            if total["decision"] is not None:
                break
        rows.append({"comparison": title, "first": f["text"], "second": s["text"], "total": dict(figures(scores), seconds_per_group_ply=seconds / max(plies, 1)), "batches": batches})
    uses_pattern = any("pattern" in side for _, f, s in parsed for side in (f, s))
    uses_network = any(side["kind"] == "network" and "pattern" not in side for _, f, s in parsed for side in (f, s))
    res = {"device": G.device_info()["name"], "runs": "one run of this tool",
           "weights": (a.weights or "none: PolicyValueNetwork(seed=...), untrained") if uses_network else "none: no side uses a network",
           "pattern_evaluator": "network.PatternEvaluator (K23): canonical move order, include/gomoku_pattern_states.h" if uses_pattern else None,
           "reading": "K7 over the pattern heuristic: a real prior and value, no weights" if uses_pattern and not uses_network else "untrained (seed) networks: the rows speak for the exact tactical options (K16 / K18 / K19), the symmetry average and the search shape, "
                      "not for what a trained prior would change" if not a.weights else "trained weights",
           "games_per_batch": a.games, "max_games": a.max_games, "paired": True, "opening_plies": a.opening_plies, "max_moves": a.max_moves, "seed": a.seed,
           "root_noise": None, "reuse_subtree": True, "sprt": {"elo0": a.elo0, "elo1": a.elo1, "alpha": a.alpha, "beta": a.beta},
           "score": "the first side's: 1 win, 0.5 tie, 0 loss; stderr from the pair means (pentanomial); elo_interval = elo(score -+ 1.96 stderr)", "rows": rows}
    for net in networks.values():
        if hasattr(net, "close"):
            net.close()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
