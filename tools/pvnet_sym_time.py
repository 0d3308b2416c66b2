#!/usr/bin/env python3
"""K22, the network evaluated over the board's eight symmetries: what gmk_pvnet_evaluate_sym costs -> profiles/pvnet_sym_time.json.
One process, the rounds of every comparison interleaved.

  all      ms per call of GMK_PVNET_SYM_ALL on n = 1, 8, 64, 512 positions against gmk_pvnet_evaluate on the same 8n rows expanded beforehand
           (the difference is the two new kernels) and against gmk_pvnet_evaluate on the n rows themselves (what the eight orientations cost).
  random   ms per call of GMK_PVNET_SYM_RANDOM against gmk_pvnet_evaluate at n = 4 096.
  game     one game, 400 playouts, leaves = 8, from an opening of 6 plies: ms per search, the plain network against symmetric("all").
  match    the 64-game match of tools/match_time.py (64 playouts a move with leaves = 8 against traditional_mcts at 200, 2 opening plies, at most
           60 moves, device loop): seconds, the plain network against symmetry="all".
  --sections takes a subset; the sections left out keep what the profile already holds.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--calls", type=int, default=20, help="calls per timed burst")
ap.add_argument("--precision", default="f32", choices=["f32", "bf16"])
ap.add_argument("--sections", default="all,random,game,match")
args = ap.parse_args()
sys.path.insert(0, args.package_root)

import numpy as np
import torch
from gomokuai_amd import lib as G, selfplay
from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork

torch.cuda.set_device(0)
G.init(0)
net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=1).cuda().eval(), precision=args.precision)
N = 225


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": list(xs)}


def boards(n, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    stones = torch.rand((n, 1, 15, 15), generator=g, device="cuda")
    planes = torch.cat([(stones < 0.1).float(), ((stones >= 0.1) & (stones < 0.2)).float(), (stones >= 0.2).float(), torch.zeros((n, 2, 15, 15), device="cuda"),
                        torch.ones((n, 1, 15, 15), device="cuda")], dim=1)
    return planes.contiguous()


def burst_ms(fn):
    """ms per call of a burst of args.calls calls, by events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / args.calls


def compare(fns):
    """{name: spread of ms per call}, the rounds interleaved; round 0 (allocations) is dropped"""
    ms = {k: [] for k in fns}
    for rnd in range(args.rounds + 1):
        for k, fn in fns.items():
            t = burst_ms(fn)
            if rnd:
                ms[k].append(t)
    return {k: spread(v) for k, v in ms.items()}


def section_all():
    out = {}
    sym = net.symmetric("all")
    for n in (1, 8, 64, 512):
        x = boards(n)
        x8 = x.repeat_interleave(8, dim=0).contiguous()          # (the same number of rows; the trunk's time does not depend on their content)
        out["n=%d" % n] = compare({"all": lambda: sym(x), "evaluate_8n_rows": lambda: net(x8), "evaluate_n_rows": lambda: net(x)})
    return out


def section_random():
    x = boards(4096)
    sym = net.symmetric("random")
    return {"n=4096": compare({"random": lambda: sym(x), "evaluate": lambda: net(x)})}


def section_game():
    moves = np.zeros((1, N), np.uint8)
    opening = [112, 113, 128, 96, 129, 127]
    moves[0, :6] = opening
    lens = np.array([6], np.int32)
    planes, last = G.moves_to_planes(moves, lens), selfplay._last_two(moves, lens)
    tree = G.AlphaZeroMCTS(1, node_capacity=400 * N + 1, c_puct=5.0, leaves=8)
    networks = {"plain": net, "all": net.symmetric("all")}
    ms = {k: [] for k in networks}
    with torch.no_grad():
        for rnd in range(args.rounds + 1):
            for k, network in networks.items():
                tree.set_roots(planes, last)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                tree.search(network, 400)
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
                if rnd:
                    ms[k].append(dt * 1e3)
    tree.close()
    return {"playouts": 400, "leaves": 8, "search_ms": {k: spread(v) for k, v in ms.items()}}


def section_match():
    opponent = ("traditional_mcts", {"c_puct": 5.0, "c_iterations": 200})
    kw = dict(playouts=64, seed=3, first_game_id=0, opening_plies=2, max_moves=60, leaves=8, device_loop=True)
    seconds, plies = {"plain": [], "all": []}, {}
    for rnd in range(4):                                         # (round 0 warms the allocator's pool up and is dropped)
        for k, symmetry in (("plain", None), ("all", "all")):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            rec, _, _ = selfplay.play_evaluation_games(64, net, opponent, symmetry=symmetry, **kw)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            plies[k] = int(rec.lens.sum()) - 2 * 64
            if rnd:
                seconds[k].append(dt)
    return {"games": 64, "network_playouts": 64, "leaves": 8, "opponent": "traditional_mcts", "opponent_playouts": 200, "max_moves": 60, "plies": plies,
            "seconds": {k: spread(v) for k, v in seconds.items()}}


out = args.out or os.path.join(args.package_root, "profiles", "pvnet_sym_time.json")
report = json.load(open(out)) if os.path.exists(out) else {}
report["device"], report["precision"], report["calls_per_burst"] = G.device_info()["name"], args.precision, args.calls
sections = args.sections.split(",")
for name, fn in (("all", section_all), ("random", section_random), ("game", section_game), ("match", section_match)):
    if name in sections:
        report[name] = fn()
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(report, indent=1, sort_keys=True))
net.close()
