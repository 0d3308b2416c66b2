#!/usr/bin/env python3
"""Timing of K10, the pattern policy on the device (pattern_kernel.hip).

  python tools/pattern_time.py [--positions 65536] [--games 16384] [--compare 2048] [--reps 10] [--out profiles/pattern_time.json]

  policy   gmk_pattern_policy on --positions random-opening positions (synth_boards kind 0, whole lists: 8 .. 60 moves), inputs and outputs
           resident on the device: positions/s and evaluator updates/s (a position costs one update per move of its list, then the heuristic)
  play     gmk_pattern_play on --games games from 4-ply openings of the same generator, filter on: games/s and plies/s
  compare  --compare positions through gmk_pattern_policy (host form: buffers in, run, four arrays out) against the route that existed
           before it: TraditionalMCTS(n).set_positions(...), run(1), root_stats()["priors"] -- with a fresh handle per call as the expression
           stands (what interface.PatternEvalAgent does per move), and for the record with a kept handle whose evaluators are reset, and with a
           kept handle whose evaluators already stand at the positions (it then replays nothing: not a position evaluation from a list).
           Alternating, same process; all routes must agree on the bits of the probabilities.
Every figure is the mean of --reps runs after one warm-up run, device events around work that ends in a synchronise."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 225


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=65536)
    ap.add_argument("--games", type=int, default=16384)
    ap.add_argument("--compare", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    G.init(0)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"device": G.device_info()["name"], "reps": a.reps}

    def device_timed(fn, prepare=None):
        times = []
        for r in range(a.reps + 1):                              # run 0 warms up
            if prepare:
                prepare()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.mean(times)), float(np.min(times)), float(np.max(times))

    # ---- policy ----
    n = a.positions
    moves, lens, _ = G.synth_boards(n, 0, first_board=0)
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    probs = torch.empty((n, N), dtype=torch.float32, device="cuda")
    value = torch.empty(n, dtype=torch.float32, device="cuda")
    best = torch.empty(n, dtype=torch.int32, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    for filt in (1, 0):
        mean, lo, hi = device_timed(lambda: G.pattern_policy_device(d_moves.data_ptr(), moves.shape[1], d_lens.data_ptr(), n, filt, probs.data_ptr(),
                                                                    value.data_ptr(), best.data_ptr(), status.data_ptr(), stream))
        st = status.cpu().numpy()
        assert not (st & ~1).any()
        res["policy_filter%d" % filt] = {"positions": n, "mean_list_length": float(lens.mean()), "seconds": mean, "seconds_min": lo, "seconds_max": hi,
                                         "positions_per_s": n / mean, "evaluator_updates_per_s": float(lens.sum()) / mean, "finished_positions": int((st & 1).sum())}

    # ---- whole games ----
    n = a.games
    m, l, _ = G.synth_boards(n, 0, first_board=0)
    open_moves = np.zeros((n, N), np.uint8)
    open_moves[:, :4] = m[:, :4]
    open_lens = np.minimum(l, 4).astype(np.int32)
    h_moves, h_lens = torch.from_numpy(open_moves).cuda(), torch.from_numpy(open_lens).cuda()
    g_moves, g_lens = torch.empty_like(h_moves), torch.empty_like(h_lens)
    winner = torch.empty(n, dtype=torch.int8, device="cuda")
    values = torch.empty((n, N), dtype=torch.float32, device="cuda")
    gstatus = torch.empty(n, dtype=torch.int32, device="cuda")

    def fresh():
        g_moves.copy_(h_moves)
        g_lens.copy_(h_lens)

    mean, lo, hi = device_timed(lambda: G.pattern_play(g_moves.data_ptr(), g_lens.data_ptr(), n, 1, 0, winner.data_ptr(), values.data_ptr(), gstatus.data_ptr(), stream), fresh)
    gl, gs, gw = g_lens.cpu().numpy(), gstatus.cpu().numpy(), winner.cpu().numpy()
    plies = int((gl - open_lens).sum())
    res["play"] = {"games": n, "opening_plies": 4, "seconds": mean, "seconds_min": lo, "seconds_max": hi, "games_per_s": n / mean, "plies_per_s": plies / mean,
                   "mean_length": float(gl.mean()), "max_length": int(gl.max()), "stalled": int(((gs & 8) != 0).sum()), "errors": int(((gs & 6) != 0).sum()),
                   "black_wins": int((gw == 1).sum()), "white_wins": int((gw == -1).sum()), "ties": int(((gw == 0) & ((gs & 1) != 0)).sum())}

    # ---- the comparison that decides whether the kernel is worth having ----
    n = a.compare
    cm, cl, _ = G.synth_boards(n, 0, first_board=0)
    cm225 = np.zeros((n, N), np.uint8)
    cm225[:, :cm.shape[1]] = cm

    def fresh_handle_route():                                    # the expression as it stands, and what interface.PatternEvalAgent does per move
        t = G.TraditionalMCTS(n, node_capacity=1024)
        t.set_positions(cm225, cl)
        t.run(1)
        p = t.root_stats()["priors"]
        t.close()
        return p

    tree = G.TraditionalMCTS(n, node_capacity=1024)

    def kept_handle_cold_route():                                # a kept handle whose evaluators start from the empty board
        tree.reset_evaluators()
        tree.set_positions(cm225, cl)
        tree.run(1)
        return tree.root_stats()["priors"]

    def kept_handle_warm_route():                                # ... whose evaluators already stand at these positions: nothing is replayed
        tree.set_positions(cm225, cl)
        tree.run(1)
        return tree.root_stats()["priors"]

    def new_route():
        return G.pattern_policy(cm225, cl, filter=True)["probs"]

    routes = [("trad_mcts_fresh_handle", fresh_handle_route), ("trad_mcts_kept_handle_reset", kept_handle_cold_route),
              ("trad_mcts_kept_handle_in_place", kept_handle_warm_route), ("pattern_policy_host", new_route)]
    times = {name: [] for name, _ in routes}
    outs = {}
    for r in range(a.reps + 1):                                  # alternating; run 0 warms up
        for name, fn in routes:
            t0 = time.perf_counter()
            outs[name] = fn()
            if r:
                times[name].append(time.perf_counter() - t0)
    tree.close()
    same = all(bool((outs[name].view(np.uint32) == outs["pattern_policy_host"].view(np.uint32)).all()) for name, _ in routes)
    res["compare"] = {"positions": n, "probabilities_bit_equal": same}
    for name, _ in routes:
        res["compare"][name + "_s"] = float(np.mean(times[name]))
        res["compare"][name + "_min_s"] = float(np.min(times[name]))
    res["compare"]["speedup_over_fresh_handle"] = res["compare"]["trad_mcts_fresh_handle_s"] / res["compare"]["pattern_policy_host_s"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    assert same, "the two routes disagree"


if __name__ == "__main__":
    main()
