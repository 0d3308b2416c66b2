#!/usr/bin/env python3
"""What several leaves per game per step (lib.AlphaZeroMCTS(leaves=), GMK_OPT_AZ_LEAVES) buy, by the number of games.

  python tools/az_leaves_time.py [--games 1,11,64,4096] [--leaves 1,2,4,8] [--playouts 400] [--playouts-large 64] [--rounds 3]
                                 [--match-leaves 1,8] [--no-match] [--graph] [--out profiles/az_leaves_time.json]

Search leg: for every number of games n and leaves L, one search of `playouts` playouts (`playouts-large` from 1 024 games on) with
network.FusedPolicyValueNetwork (K9) from positions of four stones, timed by HIP events around AlphaZeroMCTS.search after a warm-up search of
the same shape; the L of one n alternate within a round.  Per cell: the time (mean, min, max over the rounds), the steps taken (network
calls) and the mean leaves per game per step (playouts / steps: collisions cut steps short).  The yardstick is the leaves = 1 column of the
same run -- the one-leaf kernels, untouched; `--leaves 1` runs on a tree without the option as well (it never names it), which is how the
column is compared with the commit before.
Match leg: one selfplay.play_evaluation_games match in the shape of profiles/eval_match_time.json (64 games, 64 network playouts,
traditional_mcts at 200, 60 moves at most) per leaves setting, device loop, wall clock around a call that ends synchronised, per group ply.
The matches of different leaves settings are different games (the searches differ), so their plies are counted per match."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="1,11,64,4096")
    ap.add_argument("--leaves", default="1,2,4,8")
    ap.add_argument("--playouts", type=int, default=400)
    ap.add_argument("--playouts-large", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--match-leaves", default="1,8")
    ap.add_argument("--no-match", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    games = [int(x) for x in a.games.split(",") if x]
    leaves = [int(x) for x in a.leaves.split(",") if x]
    match_leaves = [] if a.no_match else [int(x) for x in a.match_leaves.split(",") if x]

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd import selfplay
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=1).cuda().eval())
    calls = [0]

    def network(states):
        calls[0] += 1
        return net(states)

    def summary(v):
        return {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    res = {"device": G.device_info()["name"], "rounds": a.rounds, "graph": bool(a.graph), "search": [], "match": []}
    for n in games:
        playouts = a.playouts_large if n >= 1024 else a.playouts
        moves, lens, _ = G.synth_boards(n, 0)
        lens = np.minimum(lens, 4).astype(np.int32)
        planes = G.moves_to_planes(moves, lens)
        last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
        trees = {L: G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1, **({"leaves": L} if L != 1 else {})) for L in leaves}
        ms, steps = {L: [] for L in leaves}, {}
        for r in range(a.rounds + 1):                             # round 0 warms up
            for L in leaves:
                tree = trees[L]
                tree.set_roots(planes, last)
                calls[0] = 0
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                with torch.no_grad():
                    tree.search(network, playouts, graph=a.graph)
                end.record()
                torch.cuda.synchronize()
                if r:
                    ms[L].append(start.elapsed_time(end))
                    if not a.graph:
                        steps[L] = calls[0]
        st = {L: trees[L].root_stats() for L in leaves}
        for L in leaves:
            assert (st[L]["root_visits"] == playouts).all() and (st[L]["status"] == 0).all(), (n, L)
            row = {"games": n, "leaves": L, "playouts": playouts, "ms": summary(ms[L])}
            if L in steps:
                row.update(steps=steps[L], mean_leaves_per_step=playouts / steps[L], batch_rows=n * L)
            if 1 in leaves:
                row["speedup_over_one_leaf"] = float(np.mean(ms[1]) / np.mean(ms[L]))
            res["search"].append(row)
            print(json.dumps(row), flush=True)
            trees[L].close()
    opponent = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 200, "use_rave": False})
    for r in range(a.rounds + 1 if match_leaves else 0):
        for L in match_leaves:
            kw = dict(playouts=64, seed=3, first_game_id=0, opening_plies=2, max_moves=60, device_loop=True, **({"leaves": L} if L != 1 else {}))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec, black, scores = selfplay.play_evaluation_games(64, net, opponent, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rl = rec.lens.cpu().numpy()
            plies = sum(int(rl[g["games"]].max()) - 2 for g in rec.groups if len(g["games"]))
            if r:
                row = next((m for m in res["match"] if m["leaves"] == L), None)
                if row is None:
                    row = {"leaves": L, "games": 64, "network_playouts": 64, "opponent": "traditional_mcts", "opponent_playouts": 200, "max_moves": 60,
                           "group_plies": plies, "win_rate": float(scores.mean()), "ms_per_ply_runs": []}
                    res["match"].append(row)
                row["ms_per_ply_runs"].append(1e3 * dt / plies)
    for row in res["match"]:
        row["ms_per_ply"] = summary(row.pop("ms_per_ply_runs"))
        print(json.dumps(row), flush=True)
    by = {m["leaves"]: m["ms_per_ply"]["mean"] for m in res["match"]}
    if 1 in by:
        res["match_speedup_over_one_leaf"] = {str(L): by[1] / v for L, v in by.items() if L != 1}
    net.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
