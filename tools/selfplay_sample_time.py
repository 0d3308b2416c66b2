#!/usr/bin/env python3
"""K20 in the K3 and K6 self-play loops: what the sampled instantiations cost and what they buy -> profiles/selfplay_sample_time.json.

  off       seconds, playouts/s and games/s of the persistent loops with sampling OFF, through the entries that existed before:
              K3  --k3-games whole games through --k3-slots slots at 800 playouts per move, a new root every move (README's K3 pipeline row, the
                  quads form of mcts_playouts_kernel, at half its games);
              K6  --k6-games whole games through --k6-slots slots at 1 000 playouts per move, kept subtree + root noise from the counter
                  sampler (README's K6 "reference semantics" row at half its games).
            --off-only measures nothing else, takes --package-root (the checkout whose package is imported) and prints / writes ONE run, so
            that the same measurement runs against the commit before, alternating; --merge LABEL=FILE adds such runs to the profile (a
            label may come several times: its runs are kept in order).  The bar: the median of "this" may not be slower than the median of
            "parent" by more than the parent's own spread (max - min of its runs).
  on        the same two runs with the first S = 8 and S = 30 plies drawn (power 1).  The games differ in length, so playouts/s and
            games/s stand beside the off rows; there is no bar.
  distinct  the number of distinct games among 256 K6 games without root noise (200 playouts, a new root every move, empty openings) at
            S = 0, 8 and 30: the figure the feature exists for.
Playing strength and training benefit are not measured here.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--merge", action="append", default=[], metavar="LABEL=FILE")
ap.add_argument("--out", default=None)
ap.add_argument("--k3-games", type=int, default=16384)
ap.add_argument("--k3-slots", type=int, default=8192)
ap.add_argument("--k6-games", type=int, default=8192)
ap.add_argument("--k6-slots", type=int, default=2048)
ap.add_argument("--sections", default="on,distinct")
args = ap.parse_args()
sys.path.insert(0, args.package_root)

import torch
from gomokuai_amd import lib as G, selfplay

torch.cuda.set_device(0)
G.init(0)


def timed(play, playouts, opening_plies):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    rec = play()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    games, moves = len(rec), int(rec.lens.sum()) - opening_plies * len(rec)
    return {"seconds": dt, "games": games, "moves": moves, "playouts_per_s": moves * playouts / dt, "games_per_s": games / dt, "overflow": bool(rec.overflow)}


def k3(games, sample=None):
    kw = dict(opening_plies=2, slots=args.k3_slots, **({} if sample is None else dict(sample_plies=sample, sample_power=1)))
    selfplay.play_games(games, 800, prepare_only=True, **kw)    # the arenas go to the library's pool: not timed
    return timed(lambda: selfplay.play_games(games, 800, **kw), 800, 2)


def k6(games, sample=None):
    kw = dict(opening_plies=2, slots=args.k6_slots, reuse_subtree=True, root_noise=(0.05, 0.25), device_loop="persistent",
              **({} if sample is None else dict(sample_plies=sample, sample_power=1)))
    selfplay.play_supervisor_games(games, 1000, prepare_only=True, **kw)
    return timed(lambda: selfplay.play_supervisor_games(games, 1000, **kw), 1000, 2)


def warm_up():
    """the first launches of a process (code objects, pool) are not the measurement's"""
    k3(args.k3_slots // 8)
    k6(args.k6_slots // 8)


def distinct():
    out = {}
    for plies in (0, 8, 30):
        rec = selfplay.play_supervisor_games(256, 200, reuse_subtree=False, root_noise=None, **({} if plies == 0 else dict(sample_plies=plies, sample_power=1))).cpu()
        out["S=%d" % plies] = len({tuple(rec.moves[g, :int(rec.lens[g])].tolist()) for g in range(256)})
    return {"games": 256, "playouts": 200, "distinct_games": out}


warm_up()
if args.off_only:
    result = {"k3": k3(args.k3_games), "k6": k6(args.k6_games)}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    sys.exit(0)

out = args.out or os.path.join(args.package_root, "profiles", "selfplay_sample_time.json")
report = json.load(open(out)) if os.path.exists(out) else {}
report["device"] = G.device_info()["name"]
report["shapes"] = {"k3": {"games": args.k3_games, "slots": args.k3_slots, "playouts": 800, "form": "a new root every move, no noise"},
                    "k6": {"games": args.k6_games, "slots": args.k6_slots, "playouts": 1000, "form": "kept subtree + root noise (counter sampler)"}}
sections = args.sections.split(",")
if "on" in sections:
    report["on"] = {"S=%d" % s: {"k3": k3(args.k3_games, s), "k6": k6(args.k6_games, s)} for s in (8, 30)}
if "distinct" in sections:
    report["distinct"] = distinct()
if args.merge:
    report["off"] = {}
    for item in args.merge:
        label, path = item.split("=", 1)
        report["off"].setdefault(label, []).append(json.load(open(path)))
    if "parent" in report["off"] and "this" in report["off"]:
        report["off_verdict"] = {}
        for k in ("k3", "k6"):
            parent, this = ([run[k]["seconds"] for run in report["off"][label]] for label in ("parent", "this"))
            spread, slower = max(parent) - min(parent), statistics.median(this) - statistics.median(parent)
            report["off_verdict"][k] = {"parent_median_s": statistics.median(parent), "this_median_s": statistics.median(this), "parent_spread_s": spread,
                                        "this_minus_parent_s": slower, "within_parent_spread": slower <= spread}
with open(out, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(report, indent=1, sort_keys=True))
