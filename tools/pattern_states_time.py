#!/usr/bin/env python3
"""What the pattern heuristic costs as K7's leaf evaluator (K23, gmk_pattern_evaluate_states).

  python tools/pattern_states_time.py [--rows 64,512,4096] [--stones 24] [--rounds 9] [--games 4096] [--playouts 32] [--out profiles/pattern_states_time.json]

Per batch size, ONE call each of four contenders on the same positions (the first `stones` plies of synthetic games, as tools/az_vcf_time.py's
ON leg), timed with HIP events in interleaved rounds after a warm-up round; medians, and the spread (max - min) / median of each:
  states    gmk_pattern_evaluate_states on the rows of planes (filter 1, norm SUM)
  states_l2 the same with norm L2: states - states_l2 is what the binary64 normalisation costs
  lists     gmk_pattern_policy on the canonical lists of the same rows: the existing kernel doing the same evaluator work
  pvnet_f32 / pvnet_bf16    gmk_pvnet_evaluate on the same rows
ratio_to_lists = states / lists; read_us_derived = the rows' bytes (5 400 per row) at `--hbm-tbs` TB/s, the only work the new front adds
besides scalar mask walks; --stones 0 and a second stone count split states - lists into a part per row and a part per ply.
Then a K7 search (games x playouts, one leaf per step; --games 0: none) with the pattern evaluator and with the f32 network, from the same
roots: us per step, interleaved the same way."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,512,4096")
    ap.add_argument("--stones", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=32)
    ap.add_argument("--hbm-tbs", type=float, default=4.0, help="the HBM rate the derived read time assumes, TB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd.network import FusedPolicyValueNetwork, PatternEvaluator, PolicyValueNetwork
    G.init(0)
    module = PolicyValueNetwork(seed=1).cuda().eval()
    nets = {"pvnet_f32": FusedPolicyValueNetwork(module), "pvnet_bf16": FusedPolicyValueNetwork(module, precision="bf16")}

    def positions(n):
        moves, lens, _ = G.synth_boards(n, 0)
        lens = np.minimum(lens, a.stones).astype(np.int32)
        return moves, lens

    def planes_of(moves, lens):
        """Board.encoded_states of every position: own, opp, empty, last move, the move before, colour"""
        n = len(lens)
        rows = np.zeros((n, 6, 225), np.float32)
        for g in range(n):
            ml = moves[g, :lens[g]].astype(np.int64)
            btm = len(ml) % 2 == 0
            rows[g, 0 if btm else 1, ml[0::2]] = 1.0
            rows[g, 1 if btm else 0, ml[1::2]] = 1.0
            if len(ml) >= 1:
                rows[g, 3, ml[-1]] = 1.0
            if len(ml) >= 2:
                rows[g, 4, ml[-2]] = 1.0
            rows[g, 5] = 1.0 if btm else 0.0
        rows[:, 2] = 1.0 - rows[:, 0] - rows[:, 1]
        return rows.reshape(n, 6, 15, 15)

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        return 1e3 * start.elapsed_time(end)                     # us

    def summary(v):
        med = float(np.median(v))
        return {"median_us": med, "min_us": float(np.min(v)), "max_us": float(np.max(v)), "spread": float((np.max(v) - np.min(v)) / med)}

    res = {"device": G.device_info()["name"], "runs": "one run of this tool", "rounds": a.rounds, "stones": a.stones, "filter": 1, "norm": "sum",
           "hbm_tbs_assumed": a.hbm_tbs, "calls": [], "k7": []}
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for n in [int(v) for v in a.rows.split(",") if v]:
        moves, lens = positions(n)
        rows = planes_of(moves, lens)
        c_moves, c_lens, c_status = G.pattern_states_list_host(rows)
        assert not c_status.any()
        d_rows = torch.from_numpy(rows).cuda()
        d_moves, d_lens = torch.from_numpy(c_moves).cuda(), torch.from_numpy(c_lens).cuda()
        value, probs = torch.zeros(n, device="cuda"), torch.zeros((n, 225), device="cuda")
        status, best = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        contenders = {
            "states": lambda: G.pattern_evaluate_states(d_rows, True, "sum", value=value, probs=probs, status=status),
            "states_l2": lambda: G.pattern_evaluate_states(d_rows, True, "l2", value=value, probs=probs, status=status),
            "lists": lambda: G.pattern_policy_device(d_moves.data_ptr(), 225, d_lens.data_ptr(), n, True, probs.data_ptr(), value.data_ptr(), best.data_ptr(),
                                                     status.data_ptr(), stream()),
        }
        for name, net in nets.items():
            contenders[name] = (lambda net: lambda: net(d_rows))(net)
        runs = {k: [] for k in contenders}
        with torch.no_grad():
            for r in range(a.rounds + 1):                         # round 0 warms up
                for k, fn in contenders.items():
                    t = timed(fn)
                    if r:
                        runs[k].append(t)
        row = {"rows": n, "read_bytes": n * 5400, "read_us_derived": n * 5400 / (a.hbm_tbs * 1e6)}
        row.update({k: summary(v) for k, v in runs.items()})
        row["ratio_to_lists"] = row["states"]["median_us"] / row["lists"]["median_us"]
        row["positions_per_s_states"] = n / (row["states"]["median_us"] * 1e-6)
        res["calls"].append(row)
        print(json.dumps(row), flush=True)

    # ---- a K7 search with either evaluator ----
    n, playouts = a.games, a.playouts
    if n <= 0:
        evaluators = {}
    else:
        moves, lens = positions(n)
        last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
        planes = G.moves_to_planes(moves, lens)
        evaluators = {"pattern": PatternEvaluator(), "pvnet_f32": nets["pvnet_f32"]}
    trees = {k: G.AlphaZeroMCTS(n, node_capacity=playouts * 225 + 1) for k in evaluators}
    runs = {k: [] for k in evaluators}
    rounds = max(3, a.rounds // 2)
    with torch.no_grad():
        for r in range(rounds + 1):
            for k, ev in evaluators.items():
                trees[k].set_roots(planes, last)
                t = timed(lambda: trees[k].search(ev, playouts))
                if r:
                    runs[k].append(t / playouts)
    for k in evaluators:
        row = {"evaluator": k, "games": n, "playouts": playouts, "leaves": 1, "rounds": rounds, "us_per_step": summary(runs[k])}
        res["k7"].append(row)
        print(json.dumps(row), flush=True)
        trees[k].close()
    for net in nets.values():
        net.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
