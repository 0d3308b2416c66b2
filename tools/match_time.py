#!/usr/bin/env python3
"""Timing of one evaluation match (selfplay.play_evaluation_games): the device loop (K12: root choice, referee and both steps as kernels)
against the same match through the host (root_stats down, numpy boards, moves up).

  python tools/match_time.py [--games 64] [--playouts 64] [--opponent traditional_mcts] [--opponent-playouts 200] [--max-moves 60]
                             [--rounds 3] [--out profiles/eval_match_time.json]

The two loops play the same games (the records are compared) and are timed alternately in one process after one warm-up round, wall clock
around a call that ends synchronised; the figure is per ply of a group: a match of two groups that each play p plies counts 2 p.  The
searches are inside both figures (they are the same launches); the difference is what the host loop does between them."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--opponent", default="traditional_mcts", choices=["traditional_mcts", "traditional_rave", "rave_mcts"])
    ap.add_argument("--opponent-playouts", type=int, default=200)
    ap.add_argument("--max-moves", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd import selfplay
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    G.init(0)
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=1).cuda().eval())
    kwargs = {"c_puct": 5.0, "c_iterations": a.opponent_playouts}
    opponent = ("rave_mcts", kwargs) if a.opponent == "rave_mcts" else ("traditional_mcts", dict(kwargs, use_rave=a.opponent == "traditional_rave"))
    kw = dict(playouts=a.playouts, seed=3, first_game_id=0, opening_plies=2, max_moves=a.max_moves)

    def play(device_loop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec, black, scores = selfplay.play_evaluation_games(a.games, net, opponent, device_loop=device_loop, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lens = rec.lens.cpu().numpy()
        plies = sum(int(lens[g["games"]].max()) - 2 for g in rec.groups if len(g["games"]))
        return dt, plies, rec.cpu(), float(scores.mean())

    per = {"device": [], "host": []}
    same = True
    for r in range(a.rounds + 1):                                 # round 0 warms up; the loops alternate within a round
        dt_d, plies_d, rec_d, rate_d = play(True)
        dt_h, plies_h, rec_h, rate_h = play(False)
        # (the dense layers' sums may follow the batch size, and the device loop hands the network live games only: equality is expected,
        # the tests hold it behind a fixed batch size)
        same &= bool((rec_d.lens == rec_h.lens).all() and (rec_d.moves == rec_h.moves).all())
        if r:
            per["device"].append(dt_d / plies_d)
            per["host"].append(dt_h / plies_h)
    res = {"device": G.device_info()["name"], "games": a.games, "network_playouts": a.playouts, "opponent": a.opponent, "opponent_playouts": a.opponent_playouts,
           "max_moves": a.max_moves, "rounds": a.rounds, "group_plies": plies_d, "win_rate": rate_d, "same_games": same,
           "ms_per_ply": {k: {"mean": 1e3 * float(np.mean(v)), "min": 1e3 * float(np.min(v)), "max": 1e3 * float(np.max(v))} for k, v in per.items()}}
    res["host_over_device"] = res["ms_per_ply"]["host"]["mean"] / res["ms_per_ply"]["device"]["mean"]
    net.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
