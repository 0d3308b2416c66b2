#!/usr/bin/env python3
"""K20, self-play moves drawn from the root's visit counts: what a sampled gmk_az_advance costs and what it buys -> profiles/az_sample_time.json.

  advance     ms per advance() of 4 096 games behind a 32-playout search, greedy against sampled (every ply drawn, power 1), in one process
              with the rounds interleaved; every round starts from the same roots.
  distinct    the number of distinct move sequences among 256 self-play games (32 playouts, empty openings, default root noise) with the
              first S = 0, 8 and 30 plies drawn, for two seeds.  The figure the feature exists for.  Whole games rarely coincide even
              without sampling (the root noise sees to that), so the distinct openings of 4, 8 and 16 plies are counted as well, and the
              whole games once more with the root noise off, where sampling is the only source of variety.
  selfplay64  seconds for 4 096 whole greedy self-play games at 64 playouts through 2 048 slots (gmk_az_set_slots + gmk_az_advance): the path
              that existed before.  --selfplay64-only measures nothing else and takes --package-root, the checkout whose package is imported,
              so that the same measurement runs against the commit before; --merge-selfplay64 LABEL=FILE adds such a result to the profile.
  --sections takes a subset of the three; the sections left out keep what the profile already holds.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--selfplay64-only", action="store_true")
ap.add_argument("--merge-selfplay64", action="append", default=[], metavar="LABEL=FILE")
ap.add_argument("--out", default=None)
ap.add_argument("--games", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--sections", default="advance,distinct,selfplay64")
args = ap.parse_args()
sys.path.insert(0, args.package_root)

import numpy as np
import torch
from gomokuai_amd import lib as G, selfplay
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork

torch.cuda.set_device(0)
G.init(0)
net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=1).cuda().eval())
N = 225


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": list(xs)}


def selfplay64(reps=3):
    times, moves = [], 0
    for rep in range(reps + 1):                                  # (the first run warms the allocator's pool up and is dropped)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        rec = selfplay.play_network_games(args.games, net, 64, first_game_id=0, opening_plies=2, slots=args.games // 2, reuse_subtree=True, root_noise=(0.05, 0.25))
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        moves = int(rec.lens.sum()) - 2 * args.games
        if rep:
            times.append(dt)
    return {"games": args.games, "slots": args.games // 2, "playouts": 64, "moves": moves, "seconds": spread(times)}


def advance_ms():
    n = args.games
    games = selfplay._HostGames.opened(n, G.DEFAULT_SEED, 0, 2)
    planes, last = G.moves_to_planes(games.moves, games.lens), games.last_two()
    tree = G.AlphaZeroMCTS(n, node_capacity=32 * N + 1, c_puct=5.0)
    tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    ms = {"greedy": [], "sampled": []}
    chosen = {}
    with torch.no_grad():
        for rnd in range(args.rounds + 1):                       # (round 0 makes the second arena and is dropped)
            for kind in ("greedy", "sampled"):
                tree.set_roots(planes, last)
                d_moves, d_lens = torch.from_numpy(games.moves).cuda(), torch.from_numpy(games.lens).cuda()
                d_winner, d_visits = torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros((n, N, N), dtype=torch.int16, device="cuda")
                tree.search(net, 32)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                tree.advance(d_moves, d_visits, d_lens, d_winner, True, sample=(N, 1, G.DEFAULT_SEED, 0) if kind == "sampled" else None)
                dt = time.perf_counter() - t0
                if rnd:
                    ms[kind].append(dt * 1e3)
                chosen[kind] = d_moves.cpu().numpy()[np.arange(n), games.lens]
    tree.close()
    return {"games": n, "playouts": 32, "rounds": args.rounds, "greedy_ms": spread(ms["greedy"]), "sampled_ms": spread(ms["sampled"]),
            "moves_that_differ": int((chosen["greedy"] != chosen["sampled"]).sum())}


def distinct():
    out, openings = {}, {}
    for seed in (G.DEFAULT_SEED, 1):
        for plies in (0, 8, 30):
            rec = selfplay.play_network_games(256, net, 32, seed=seed, sample_plies=plies, sample_power=1).cpu()
            seqs = {tuple(rec.moves[g, :int(rec.lens[g])].tolist()) for g in range(256)}
            out.setdefault("S=%d" % plies, []).append(len(seqs))
            for k in (4, 8, 16):
                openings.setdefault("S=%d" % plies, {}).setdefault("first %d plies" % k, []).append(len({tuple(rec.moves[g, :min(k, int(rec.lens[g]))].tolist()) for g in range(256)}))
    quiet = {}
    for seed in (G.DEFAULT_SEED, 1):
        for plies in (0, 8, 30):
            rec = selfplay.play_network_games(256, net, 32, seed=seed, root_noise=None, sample_plies=plies, sample_power=1).cpu()
            quiet.setdefault("S=%d" % plies, []).append(len({tuple(rec.moves[g, :int(rec.lens[g])].tolist()) for g in range(256)}))
    return {"games": 256, "playouts": 32, "seeds": [G.DEFAULT_SEED, 1], "distinct_sequences": out, "distinct_openings": openings, "distinct_sequences_without_root_noise": quiet}


if args.selfplay64_only:
    result = selfplay64()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    sys.exit(0)

out = args.out or os.path.join(args.package_root, "profiles", "az_sample_time.json")
report = json.load(open(out)) if os.path.exists(out) else {}
report["device"] = G.device_info()["name"]
sections = args.sections.split(",")
if "advance" in sections:
    report["advance"] = advance_ms()
if "distinct" in sections:
    report["distinct"] = distinct()
if "selfplay64" in sections:
    report.setdefault("selfplay64", {})["this"] = selfplay64()
for item in args.merge_selfplay64:
    label, path = item.split("=", 1)
    report.setdefault("selfplay64", {})[label] = json.load(open(path))
with open(out, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(report, indent=1, sort_keys=True))
