#!/usr/bin/env python3
"""What solving forced wins by fours at the leaves of K7 (lib.AlphaZeroMCTS(vcf_depth=, vcf_budget=), GMK_OPT_AZ_VCF_DEPTH) costs.

  python tools/az_vcf_time.py [--shapes 4096:1:64,1:8:400,64:8:400] [--settings 8:32,16:64,16:256] [--stones 4] [--stones-on 24] [--rounds 5]
                              [--off-only] [--out profiles/az_vcf_time.json]

A shape is games:leaves:playouts.  The network is network.FusedPolicyValueNetwork (K9); times are HIP events, after a warm-up search of the
same shape, over `rounds` rounds in which the settings of one shape alternate.
OFF leg: one AlphaZeroMCTS.search per round on a handle that never names the option, from positions of `stones` stones: ms per search and per
step (mean, min, max and the spread (max - min) / mean over the rounds).  With --off-only nothing else runs and nothing of the option is
touched, so the same file runs on the commit before; the two OFF legs, on one machine, are the comparison the D = 0 path is held to.
ON leg: per (D, B), from positions of `stones-on` stones (the first plies of synthetic games: enough stones for threes and fours to exist), the
same search stepped by hand with events between select (the select kernel and, when on, the solver kernel behind it), the network and expand:
ms per step, the three parts, and the solver's share = (select part ON - select part OFF on the same positions) / step ON; then leaves solved,
answered WIN and cut per search (gmk_az_vcf_stats), and the nodes per leaf, mean and largest (the largest from the verdicts of every step of
one more, untimed search)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096:1:64,1:8:400,64:8:400")
    ap.add_argument("--settings", default="8:32,16:64,16:256")
    ap.add_argument("--stones", type=int, default=4)
    ap.add_argument("--stones-on", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",") if s]
    settings = [] if a.off_only else [tuple(int(v) for v in s.split(":")) for s in a.settings.split(",") if s]

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=1).cuda().eval())

    def summary(v):
        return {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v)), "spread": float((np.max(v) - np.min(v)) / np.mean(v))}

    def roots(n, stones):
        moves, lens, _ = G.synth_boards(n, 0)
        lens = np.minimum(lens, stones).astype(np.int32)
        last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
        return G.moves_to_planes(moves, lens), last

    def make(n, L, playouts, setting):
        kw = {"leaves": L} if L != 1 else {}
        if setting is not None:
            kw.update(vcf_depth=setting[0], vcf_budget=setting[1])
        return G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1, **kw)

    def event():
        return torch.cuda.Event(enable_timing=True)

    def timed_search(tree, playouts):
        start, end = event(), event()
        torch.cuda.synchronize()
        start.record()
        with torch.no_grad():
            tree.search(net, playouts)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end)

    def stepped_search(tree, playouts, L, verdicts=None):
        """-> (steps, ms in select [+ solver], ms in the network, ms in expand); verdicts: a list that takes every step's node counts (untimed use)"""
        marks, steps = [], 0
        if L > 1:
            tree.add_playouts(playouts)
        with torch.no_grad():
            while (steps < playouts) if L == 1 else (steps < -(-playouts // L) or tree.playouts_owed() > 0):
                e = [event() for _ in range(4)]
                e[0].record()
                states = tree.select()
                e[1].record()
                if verdicts is not None:
                    verdicts.append(tree.vcf_verdicts()["nodes"])
                values, probs = net(states)
                e[2].record()
                tree.expand(values.contiguous(), probs.contiguous())
                e[3].record()
                marks.append(e)
                steps += 1
        torch.cuda.synchronize()
        parts = [sum(e[i].elapsed_time(e[i + 1]) for e in marks) for i in range(3)]
        return steps, parts[0], parts[1], parts[2]

    res = {"device": G.device_info()["name"], "rounds": a.rounds, "stones_off": a.stones, "stones_on": a.stones_on, "off": [], "on": []}
    for n, L, playouts in shapes:
        # ---- OFF: the handle never hears of the option ----
        planes, last = roots(n, a.stones)
        tree = make(n, L, playouts, None)
        ms = []
        for r in range(a.rounds + 1):                             # round 0 warms up
            tree.set_roots(planes, last)
            t = timed_search(tree, playouts)
            if r:
                ms.append(t)
        tree.set_roots(planes, last)
        steps = stepped_search(tree, playouts, L)[0]
        tree.close()
        row = {"games": n, "leaves": L, "playouts": playouts, "steps": steps, "ms_per_search": summary(ms), "us_per_step": summary([1e3 * t / steps for t in ms])}
        res["off"].append(row)
        print(json.dumps(row), flush=True)
        if not settings:
            continue
        # ---- ON: the settings and OFF alternate within a round, on positions with enough stones ----
        planes, last = roots(n, a.stones_on)
        trees = {s: make(n, L, playouts, s) for s in [None] + settings}
        runs = {s: [] for s in trees}
        for r in range(a.rounds + 1):
            for s, tree in trees.items():
                tree.set_roots(planes, last)
                out = stepped_search(tree, playouts, L)
                if r:
                    runs[s].append(out)
        off_select = float(np.mean([sel / st for st, sel, _, _ in runs[None]]))
        for s in [None] + settings:
            st = [o[0] for o in runs[s]]
            step_us = [1e3 * (sel + nn + ex) / k for k, sel, nn, ex in runs[s]]
            row = {"games": n, "leaves": L, "playouts": playouts, "depth": 0 if s is None else s[0], "budget": None if s is None else s[1], "steps": st[-1],
                   "us_per_step": summary(step_us), "select_us_per_step": summary([1e3 * sel / k for k, sel, _, _ in runs[s]]),
                   "network_us_per_step": summary([1e3 * nn / k for k, _, nn, _ in runs[s]]), "expand_us_per_step": summary([1e3 * ex / k for k, _, _, ex in runs[s]])}
            if s is not None:
                stats = trees[s].vcf_stats()                      # of the last round's search
                solver_us = 1e3 * (float(np.mean([sel / k for k, sel, _, _ in runs[s]])) - off_select)
                seen = []
                trees[s].set_roots(planes, last)
                stepped_search(trees[s], playouts, L, verdicts=seen)
                leaves = int(stats["leaves"].sum())
                row.update(solver_us_per_step=solver_us, solver_share_of_step=solver_us / row["us_per_step"]["mean"], leaves_solved=leaves,
                           wins=int(stats["wins"].sum()), cut=int(stats["cut"].sum()), nodes_per_leaf_mean=float(stats["nodes"].sum()) / max(leaves, 1),
                           nodes_per_leaf_max=int(max(int(v.max()) for v in seen)))
            res["on"].append(row)
            print(json.dumps(row), flush=True)
        for tree in trees.values():
            tree.close()
    net.close()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
