#!/usr/bin/env python3
"""K9 in bf16, measured: the trunk in float32 against bf16 in ONE process, rounds interleaved, HIP events around windows of >= ~50 ms after a
warm-up; then a K7 step and a 64-playout search at 4 096 games with either network, and how far the two precisions' outputs and searches
differ for a glorot net on real feature planes (recorded, not asserted).  Writes one JSON (default profiles/pvnet_bf16_time.json).

    python tools/pvnet_bf16_time.py [--out FILE] [--rounds 7] [--games 4096] [--playouts 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gomokuai_amd import lib as G
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork

FLOP_PER_POSITION = 2 * 225 * (54 * 32 + 288 * 64 + 576 * 128 + 128 * 6)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(fns, reps, rounds):
    """{name: [ms per call, one per round]}: every round times each variant once, in turn"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, reps))
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def roots(n):
    moves, lens, _ = G.synth_boards(n, 0)
    lens = np.minimum(lens, 12).astype(np.int32)
    planes = G.moves_to_planes(moves, lens)
    last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], 1).astype(np.int16)
    return planes, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pvnet_bf16_time.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=64)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    G.init(0)
    net = PolicyValueNetwork(seed=1).cuda().eval()
    nets = {"f32": FusedPolicyValueNetwork(net), "bf16": FusedPolicyValueNetwork(net, precision="bf16")}
    result = {"device": torch.cuda.get_device_name(0), "cu_count": G.device_info()["cu_count"], "rounds": args.rounds, "trunk": {}, "evaluate": {}}

    # settle the chip: half a second of the float32 trunk before anything is timed
    warm = (torch.rand((4096, 6, 15, 15), device="cuda") > 0.7).float()
    t0 = time.time()
    while time.time() - t0 < 0.5:
        nets["f32"].trunk(warm)
        torch.cuda.synchronize()

    for n in (64, 256, 4096, 16384):
        states = (torch.rand((n, 6, 15, 15), device="cuda", generator=torch.Generator("cuda").manual_seed(n)) > 0.7).float()
        reps = max(10, min(400, int(50.0 / (0.0004 * n + 0.05))))
        ms = interleaved({k: (lambda f=f: f.trunk(states)) for k, f in nets.items()}, reps, args.rounds)
        row = {k: dict(summary(v), tflops=round(n * FLOP_PER_POSITION / statistics.median(v) / 1e9, 1)) for k, v in ms.items()}
        row["reps_per_window"] = reps
        row["f32_over_bf16"] = round(statistics.median(ms["f32"]) / statistics.median(ms["bf16"]), 3)
        # "faster by more than the runs' spread": the slowest bf16 round against the fastest float32 round
        row["bf16_max_below_f32_min"] = max(ms["bf16"]) < min(ms["f32"])
        result["trunk"][str(n)] = row
        ms = interleaved({k: (lambda f=f: f(states)) for k, f in nets.items()}, reps, args.rounds)
        result["evaluate"][str(n)] = {k: summary(v) for k, v in ms.items()}
        print("n = %5d: trunk f32 %.4f ms, bf16 %.4f ms (x %.2f); with the dense kernel f32 %.4f ms, bf16 %.4f ms" % (
            n, row["f32"]["median_ms"], row["bf16"]["median_ms"], row["f32_over_bf16"],
            result["evaluate"][str(n)]["f32"]["median_ms"], result["evaluate"][str(n)]["bf16"]["median_ms"]), flush=True)

    # ---- K7: a search of `playouts` lock-step playouts at `games` games, either network; a step = search / playouts ----
    planes, last = roots(args.games)
    searches, stats = {k: [] for k in nets}, {}
    for rnd in range(3 + 1):                                                      # the first round warms up
        for k, f in nets.items():
            tree = G.AlphaZeroMCTS(args.games, node_capacity=args.playouts * 225 + 1)
            tree.set_roots(planes, last)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                tree.search(f, args.playouts)
            torch.cuda.synchronize()
            if rnd:
                searches[k].append((time.perf_counter() - t0) * 1e3)
            stats[k] = tree.root_stats()
            tree.close()
    result["search"] = {"games": args.games, "playouts": args.playouts,
                        **{k: {"search_ms": summary(v), "step_ms": round(statistics.median(v) / args.playouts, 4),
                               "playouts_per_s": round(args.games * args.playouts / statistics.median(v) * 1e3)} for k, v in searches.items()}}
    a, b = stats["f32"], stats["bf16"]
    result["search"]["most_visited_root_move_agrees"] = round(float((a["visits"].argmax(1) == b["visits"].argmax(1)).mean()), 4)
    print("search %d x %d: f32 %.1f ms, bf16 %.1f ms; most-visited root move agrees in %.1f %% of games" % (
        args.games, args.playouts, statistics.median(searches["f32"]), statistics.median(searches["bf16"]), 100 * result["search"]["most_visited_root_move_agrees"]), flush=True)

    # ---- the two precisions' outputs on the roots' feature planes (a glorot net) ----
    tree = G.AlphaZeroMCTS(args.games, node_capacity=args.playouts * 225 + 1)
    tree.set_roots(planes, last)
    states = tree.select().clone()
    with torch.no_grad():
        (v32, p32), (v16, p16) = nets["f32"](states), nets["bf16"](states)
        tree.expand(v32, p32)
    torch.cuda.synchronize()
    tree.close()
    result["outputs_f32_against_bf16"] = {"positions": int(states.shape[0]), "max_abs_dvalue": float((v32 - v16).abs().max()), "max_abs_dprob": float((p32 - p16).abs().max()),
                                          "max_prob": float(p32.max()), "policy_argmax_agrees": round(float((p32.argmax(1) == p16.argmax(1)).float().mean()), 4)}
    result["playing_strength"] = "not measured"
    print(json.dumps(result["outputs_f32_against_bf16"]))
    for f in nets.values():
        f.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
