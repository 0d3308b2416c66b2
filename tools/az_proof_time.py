#!/usr/bin/env python3
"""What carrying proven wins and losses up K7's tree (lib.AlphaZeroMCTS(proof=True), GMK_OPT_AZ_PROOF) costs and saves.

  python tools/az_proof_time.py [--shapes 4096:1:64,1:8:400,64:8:400] [--vcf 16:64] [--stones 4] [--stones-on 24] [--rounds 5]
                                [--off-only] [--match] [--out profiles/az_proof_time.json]

A shape is games:leaves:playouts.  The network is network.FusedPolicyValueNetwork (K9); times are HIP events, after a warm-up search of the
same shape, over `rounds` rounds.
OFF leg: one AlphaZeroMCTS.search per round on a handle that never names the option, from positions of `stones` stones: ms per search (mean,
min, max and the spread (max - min) / mean over the rounds).  With --off-only nothing else runs and nothing of the option is touched, so the
same file runs on the commit before; the two OFF legs, on one machine, in alternating processes, are the comparison the off path is held to.
ON leg: from positions of `stones-on` stones (the first plies of synthetic games: enough stones for threes and fours to exist), with the solver
at the leaves (--vcf D:B), proof off and on alternating within a round: ms per search, steps (network calls) and batch rows per search, the
pending leaves and those the network answered (pending - WIN: the rows that were worth computing), and `proved` / `stops` per search.
--match: one evaluation match in K12's shape (64 games, 64 network playouts, traditional_mcts at 200, seed 3, two opening plies, whole games)
with the solver on and proofs off and on: games won and mean length.  Recorded, no claim."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096:1:64,1:8:400,64:8:400")
    ap.add_argument("--vcf", default="16:64")
    ap.add_argument("--stones", type=int, default=4)
    ap.add_argument("--stones-on", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--match", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",") if s]
    vcf = tuple(int(v) for v in a.vcf.split(":"))

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=1).cuda().eval())
    calls = {"steps": 0, "rows": 0}

    def counted(states):
        calls["steps"] += 1
        calls["rows"] += int(states.shape[0])
        return net(states)

    def summary(v):
        return {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v)), "spread": float((np.max(v) - np.min(v)) / np.mean(v))}

    def roots(n, stones):
        moves, lens, _ = G.synth_boards(n, 0)
        lens = np.minimum(lens, stones).astype(np.int32)
        last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
        return G.moves_to_planes(moves, lens), last

    def timed_search(tree, playouts):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        with torch.no_grad():
            tree.search(counted, playouts)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end)

    res = {"device": G.device_info()["name"], "rounds": a.rounds, "stones_off": a.stones, "stones_on": a.stones_on, "vcf": list(vcf), "off": [], "on": [], "match": []}
    for n, L, playouts in shapes:
        kw = {"leaves": L} if L != 1 else {}
        # ---- OFF: the handle never hears of the option ----
        planes, last = roots(n, a.stones)
        tree = G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1, **kw)
        ms = []
        for r in range(a.rounds + 1):                             # round 0 warms up
            tree.set_roots(planes, last)
            t = timed_search(tree, playouts)
            if r:
                ms.append(t)
        tree.close()
        row = {"games": n, "leaves": L, "playouts": playouts, "ms_per_search": summary(ms)}
        res["off"].append(row)
        print(json.dumps(row), flush=True)
        if a.off_only:
            continue
        # ---- ON: the solver at the leaves, proofs off and on alternating within a round ----
        planes, last = roots(n, a.stones_on)
        trees = {p: G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1, vcf_depth=vcf[0], vcf_budget=vcf[1], proof=p, **kw) for p in (False, True)}
        runs = {p: [] for p in trees}
        for r in range(a.rounds + 1):
            for p, tree in trees.items():
                tree.set_roots(planes, last)
                calls.update(steps=0, rows=0)
                t = timed_search(tree, playouts)
                if r:
                    runs[p].append((t, calls["steps"], calls["rows"]))
        for p, tree in trees.items():
            st, ps = tree.vcf_stats(), tree.proof_stats()         # of the last round's search
            pending, wins = int(st["leaves"].sum()), int(st["wins"].sum())
            row = {"games": n, "leaves": L, "playouts": playouts, "proof": p, "ms_per_search": summary([t for t, _, _ in runs[p]]), "steps": runs[p][-1][1],
                   "batch_rows": runs[p][-1][2], "pending_leaves": pending, "win_leaves": wins, "network_rows": pending - wins,
                   "proved": int(ps["proved"].sum()), "stops": int(ps["stops"].sum()), "root_visits": int(tree.root_stats()["root_visits"].sum())}
            res["on"].append(row)
            print(json.dumps(row), flush=True)
            tree.close()
    if a.match and not a.off_only:
        from gomokuai_amd import selfplay
        for p in (False, True):
            rec, black, scores = selfplay.play_evaluation_games(64, net, ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 200}), playouts=64, seed=3, first_game_id=0,
                                                                opening_plies=2, vcf=vcf, proof=p)
            row = {"proof": p, "games": 64, "won": float((scores == 1.0).sum()), "score": float(scores.sum()), "mean_length": float(rec.cpu().lens.float().mean())}
            res["match"].append(row)
            print(json.dumps(row), flush=True)
    net.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
