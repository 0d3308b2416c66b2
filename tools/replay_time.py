#!/usr/bin/env python3
"""Timing of the replay buffer's draw (replay_kernel.hip) against the route that existed before it.

  python tools/replay_time.py [--games 4096] [--playouts 100] [--batches 512,4096] [--reps 300] [--out profiles/replay_time.json]

One real self-play batch (play_games, RandomPolicy) fills both routes:
  replay        ReplayBuffer.extend(records) once, then ReplayBuffer.sample(B) per batch: float32 states, augmented, built at draw time
  materialised  GameRecords.to_samples(augment=True) once, then per batch torch.randperm(S)[:B] and a gather of the three tensors, the
                states cast to float32 (what the network takes): the only route to a minibatch before the buffer existed
The two are timed alternately in one process, device events around --reps draws that end in a synchronise, after one warm-up round; the
figures are per draw.  Also reported: the bytes each route keeps resident, the one-off costs (extend, to_samples), and whether the two
routes can produce the same tuple bits (row 8 s + a of the materialised set for every pick of one replay batch)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 225


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=100)
    ap.add_argument("--batches", default="512,4096")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd import selfplay
    G.init(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    def timed(fn, reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    rec = selfplay.play_games(a.games, a.playouts, seed=7)
    torch.cuda.synchronize()
    lens = rec.lens.cpu().numpy()
    plies = int(lens.sum())
    res = {"device": G.device_info()["name"], "games": a.games, "playouts": a.playouts, "plies": plies, "mean_length": float(lens.mean()),
           "reps": a.reps, "rounds": a.rounds}

    # ---- fill both routes (one-off costs, one measurement each after a warm-up of the same call) ----
    cap = max(plies, N)
    buf = selfplay.ReplayBuffer(cap, max_games=a.games, seed=1)
    buf.extend(rec)
    buf.reset()
    res["extend_seconds"] = timed(lambda: buf.extend(rec), 1)
    assert buf.status()[0] == 0 and buf.stats()["population"] == plies
    mat = rec.to_samples(augment=True)
    del mat
    holder = {}
    res["to_samples_seconds"] = timed(lambda: holder.update(mat=rec.to_samples(augment=True)), 1)
    states, values, pi = holder.pop("mat")
    S = int(values.shape[0])
    assert S == 8 * plies
    res["resident_bytes"] = {
        "replay": cap * 451 + a.games * 32,
        "materialised": states.numel() + 4 * values.numel() + 4 * pi.numel(),
        "records_fixed_stride": rec.moves.numel() + 4 * rec.lens.numel() + rec.winner.numel() + 2 * rec.visits.numel(),
    }
    res["resident_bytes"]["materialised_over_replay"] = res["resident_bytes"]["materialised"] / res["resident_bytes"]["replay"]

    # ---- the same bits: every pick of one replay batch is a row of the materialised set ----
    cum = np.concatenate([[0], np.cumsum(lens)])
    st_u8, v_r, pi_r, picked = buf.sample(4096 if S >= 4096 else S, step=0, dtype=torch.uint8, return_picked=True)
    p = picked.cpu().numpy()
    rows = torch.from_numpy(8 * (cum[p[:, 0]] + p[:, 1]) + p[:, 2]).to(dev)
    res["same_bits_as_materialised"] = bool(torch.equal(st_u8, states[rows]) and torch.equal(v_r.view(torch.int32), values[rows].view(torch.int32))
                                            and torch.equal(pi_r.view(torch.int32), pi[rows].view(torch.int32)))

    def gather(B):
        idx = torch.randperm(S, device=dev)[:B]
        return states[idx].to(torch.float32), values[idx], pi[idx]

    def gather_only(idx):
        return states[idx].to(torch.float32), values[idx], pi[idx]

    res["draws"] = {}
    for B in [int(b) for b in a.batches.split(",")]:
        if B > S:
            continue
        fixed = torch.randperm(S, device=dev)[:B]
        routes = {"replay": lambda: buf.sample(B), "materialised": lambda: gather(B), "materialised_gather_only": lambda: gather_only(fixed)}
        per = {k: [] for k in routes}
        for r in range(a.rounds + 1):                             # round 0 warms up; the routes alternate within a round
            for k, fn in routes.items():
                t = timed(fn, a.reps)
                if r:
                    per[k].append(t)
        res["draws"][str(B)] = {k: {"us_per_draw": 1e6 * float(np.mean(v)), "us_min": 1e6 * float(np.min(v)), "us_max": 1e6 * float(np.max(v)),
                                    "samples_per_s": B / float(np.mean(v))} for k, v in per.items()}
    assert buf.status()[1] == 0
    buf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
