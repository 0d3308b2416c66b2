#!/usr/bin/env python3
"""Timing of the replay buffer's checkpoint: ReplayBuffer.state_dict() and load_state_dict() of a full buffer.

  python tools/replay_image_time.py [--capacity 200000] [--games 4096] [--playouts 100] [--rounds 5] [--out profiles/replay_image_time.json]

One real self-play batch (play_games, RandomPolicy) fills a buffer of --capacity plies (the oldest games leave if the batch is larger).
state_dict() -- state words to the host, descriptor kernel, ring copies, image to the host -- and load_state_dict() into a second buffer
of the same size -- host check, image to the device, check kernel, ring copies, commit kernel -- are timed alternately, device events
around each call plus the wall clock (the host copy and the host check are not device work); one warm-up round, then the median of
--rounds.  Also reported: the image's size and whether the restored buffer's snapshot is the image again."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=200000)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd import selfplay
    G.init(0)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0

    rec = selfplay.play_games(a.games, a.playouts, seed=7)
    torch.cuda.synchronize()
    src = selfplay.ReplayBuffer(a.capacity, max_games=a.games, seed=1)
    dst = selfplay.ReplayBuffer(a.capacity, max_games=a.games, seed=1)
    src.extend(rec)
    assert src.status()[0] == 0
    stats = src.stats()
    res = {"device": G.device_info()["name"], "capacity_plies": a.capacity, "games_played": a.games, "playouts": a.playouts,
           "games_held": stats["games"], "plies_held": stats["plies"], "population": stats["population"], "rounds": a.rounds}
    per = {"state_dict": [], "load_state_dict": []}
    state = None
    for r in range(a.rounds + 1):                                 # round 0 warms up
        state, dev_s, wall_s = timed(src.state_dict)
        if r:
            per["state_dict"].append((dev_s, wall_s))
        _, dev_s, wall_s = timed(lambda: dst.load_state_dict(state))
        if r:
            per["load_state_dict"].append((dev_s, wall_s))
    res["image_bytes"] = int(state["image"].numel())
    res["restored_snapshot_is_the_image"] = bool(torch.equal(dst.state_dict()["image"], state["image"])) and dst.stats() == stats
    for k, v in per.items():
        v = np.array(v)
        res[k] = {"device_event_seconds_median": float(np.median(v[:, 0])), "wall_seconds_median": float(np.median(v[:, 1])),
                  "wall_seconds_min": float(v[:, 1].min()), "wall_seconds_max": float(v[:, 1].max()),
                  "GB_per_s_wall": res["image_bytes"] / float(np.median(v[:, 1])) * 1e-9}
    src.close()
    dst.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
