#!/usr/bin/env python3
"""What proving lost replies at K7's leaves with the defence solver (lib.AlphaZeroMCTS(vcf_defend=True), GMK_OPT_AZ_VCF_DEFEND) costs and saves.

  python tools/az_defend_time.py [--shapes 4096:1:64,1:8:400,64:8:400] [--vcf 16:64] [--stones 4] [--stones-on 24] [--rounds 5]
                                 [--off-only] [--out profiles/az_defend_time.json]

A shape is games:leaves:playouts.  The network is network.FusedPolicyValueNetwork (K9); times are HIP events, after a warm-up search of the
same shape, over `rounds` rounds.
OFF leg: one AlphaZeroMCTS.search per round on a handle that never names the option, from positions of `stones` stones: ms per search (mean,
min, max and the spread (max - min) / mean over the rounds).  With --off-only nothing else runs and nothing of the option is touched, so the
same file runs on the commit before; the two OFF legs, on one machine, in alternating processes, are the comparison the off path is held to.
ON leg: from positions of `stones-on` stones (the first plies of synthetic games: enough stones for threes and fours to exist), with the solver
at the leaves (--vcf D:B) and proofs on, the defence off and on alternating within a round: ms per search and per step, the time the defence
adds per step, steps (network calls) and batch rows per search, the leaves expanded under a WIN threat, the children marked, the cells solved
in full and their nodes, the pending leaves the network answered, and `proved` / `stops` per search.  Recorded, no claim: the step pays for its
heaviest searched cell."""
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

    res = {"device": G.device_info()["name"], "rounds": a.rounds, "stones_off": a.stones, "stones_on": a.stones_on, "vcf": list(vcf), "off": [], "on": []}
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
        # ---- ON: the solver at the leaves and proofs, the defence off and on alternating within a round ----
        planes, last = roots(n, a.stones_on)
        trees = {d: G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1, vcf_depth=vcf[0], vcf_budget=vcf[1], proof=True, vcf_defend=d, **kw) for d in (False, True)}
        runs = {d: [] for d in trees}
        for r in range(a.rounds + 1):
            for d, tree in trees.items():
                tree.set_roots(planes, last)
                calls.update(steps=0, rows=0)
                t = timed_search(tree, playouts)
                if r:
                    runs[d].append((t, calls["steps"], calls["rows"]))
        per_step = {d: float(np.mean([t / s for t, s, _ in runs[d]])) for d in trees}
        for d, tree in trees.items():
            st, ps, ds = tree.vcf_stats(), tree.proof_stats(), tree.defend_stats()      # of the last round's search
            pending, wins = int(st["leaves"].sum()), int(st["wins"].sum())
            row = {"games": n, "leaves": L, "playouts": playouts, "defend": d, "ms_per_search": summary([t for t, _, _ in runs[d]]), "ms_per_step": per_step[d],
                   "added_ms_per_step": per_step[d] - per_step[False], "steps": runs[d][-1][1], "batch_rows": runs[d][-1][2], "pending_leaves": pending,
                   "win_leaves": wins, "network_rows": pending - wins, "threatened": int(ds["threatened"].sum()), "marked": int(ds["marked"].sum()),
                   "searched": int(ds["searched"].sum()), "nodes": int(ds["nodes"].sum()), "proved": int(ps["proved"].sum()), "stops": int(ps["stops"].sum()),
                   "root_visits": int(tree.root_stats()["root_visits"].sum()), "arena_full": int((tree.root_stats()["status"] & 2 != 0).sum())}
            res["on"].append(row)
            print(json.dumps(row), flush=True)
            tree.close()
    net.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
