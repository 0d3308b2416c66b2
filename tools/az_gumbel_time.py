#!/usr/bin/env python3
"""K21, the Gumbel root search of K7: what the option costs -> profiles/az_gumbel_time.json.

  off   a search with the option off -- 4 096 games x 64 playouts and one game x 400 playouts, behind the fused network -- on this checkout
        against the commit before (--parent-root: a checkout of it with its library built).  One child process per measurement, this checkout
        and the parent's in turn for --rounds rounds; medians; the ratio stands beside the parent's own round-to-round spread from the same
        run, which is what it is judged against.  No bar is fixed in advance.
  on    the same two shapes on this checkout with the option on at m = 16 (n_sims = the playouts), in one process with the rounds interleaved
        off / on: the added time per step, and the one-off set-up -- the first step on roots that have children, against the steps after it.
  --measure-off prints one child's measurement and nothing else (what the rounds run).
Playing strength and training benefit are not measured here.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=HERE)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--measure-off", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
SHAPES = ((4096, 64), (1, 400))
N = 225


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": list(xs)}


def measure(gumbel_rounds=0):
    """ms per search of each shape with the option off; with gumbel_rounds > 0 (this checkout only) also on, interleaved, and the set-up"""
    sys.path.insert(0, args.package_root)
    import torch
    from gomokuai_amd import lib as G, selfplay
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    torch.cuda.set_device(0)
    G.init(0)
    net = FusedPolicyValueNetwork(PolicyValueNetwork(seed=1).cuda().eval())
    out = {}
    with torch.no_grad():
        for n, playouts in SHAPES:
            games = selfplay._HostGames.opened(n, G.DEFAULT_SEED, 0, 2)
            planes, last = G.moves_to_planes(games.moves, games.lens), games.last_two()
            tree = G.AlphaZeroMCTS(n, node_capacity=playouts * N + 1, c_puct=5.0)

            def search(on):
                if gumbel_rounds:
                    tree.set_gumbel(16 if on else 0, playouts, 50.0, 1.0, G.DEFAULT_SEED, 0)
                tree.set_roots(planes, last)
                tree.search(net, 1)                              # the playout that gives the roots their children
                torch.cuda.synchronize(); t0 = time.perf_counter()
                tree.search(net, 1)                              # under the option: the set-up and the first scheduled playout
                torch.cuda.synchronize(); t1 = time.perf_counter()
                tree.search(net, playouts - 2)
                torch.cuda.synchronize(); t2 = time.perf_counter()
                return (t1 - t0) * 1e3, (t2 - t1) * 1e3 / (playouts - 2)
            search(False)                                        # (warms the allocator and the network's first call of this batch size)
            kinds = (False, True) if gumbel_rounds else (False,)
            first, step = {k: [] for k in kinds}, {k: [] for k in kinds}
            for _ in range(max(gumbel_rounds, 3)):
                for on in kinds:
                    a, b = search(on)
                    first[on].append(a); step[on].append(b)
            key = "%d games x %d playouts" % (n, playouts)
            out[key] = {"off_ms_per_step": spread(step[False]), "off_first_step_ms": spread(first[False])}
            if gumbel_rounds:
                out[key].update(on_ms_per_step=spread(step[True]), on_first_step_ms=spread(first[True]),
                                added_ms_per_step=statistics.median(step[True]) - statistics.median(step[False]),
                                setup_ms=(statistics.median(first[True]) - statistics.median(step[True])) - (statistics.median(first[False]) - statistics.median(step[False])))
            tree.close()
    net.close()
    return out, G.device_info()["name"]


if args.measure_off:
    print(json.dumps(measure()[0]))
    sys.exit(0)

report = {"m": 16, "c_visit": 50.0, "c_scale": 1.0, "note": "playing strength and training benefit are not measured"}
on, report["device"] = measure(gumbel_rounds=args.rounds)
report["on"] = on
if args.parent_root:
    runs = {"this": [], "parent": []}
    for _ in range(args.rounds):
        for label, root in (("this", args.package_root), ("parent", args.parent_root)):
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure-off", "--package-root", root], check=True, capture_output=True, text=True, timeout=300)
            runs[label].append(json.loads(child.stdout.strip().splitlines()[-1]))
    off = {}
    for key in runs["this"][0]:
        this = [r[key]["off_ms_per_step"]["median"] for r in runs["this"]]
        parent = [r[key]["off_ms_per_step"]["median"] for r in runs["parent"]]
        off[key] = {"this_ms_per_step": spread(this), "parent_ms_per_step": spread(parent), "ratio_this_over_parent": statistics.median(this) / statistics.median(parent),
                    "parent_spread_max_over_min": max(parent) / min(parent)}
    report["off"] = off
out = args.out or os.path.join(HERE, "profiles", "az_gumbel_time.json")
with open(out, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(report, indent=1, sort_keys=True))
