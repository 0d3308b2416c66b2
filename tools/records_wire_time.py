#!/usr/bin/env python3
"""Timing of the wire form of game records on the device (records_wire.hip) against the torch code in selfplay.py, configs[3]'s 32 768 games.

  python tools/records_wire_time.py [--games 32768] [--reps 10] [--out FILE.json]
      game lengths from a short real self-play run (512 games x 100 playouts, RandomPolicy, seed 1), tiled to --games in a seeded random
      order; moves a random permutation of the cells per game, visits random uint16 (their values do not change the bytes moved).
      Times each path end to end (device events around the Python call, synchronisations included) and checks it against the torch one.
  python tools/records_wire_time.py --stats STATS.csv|RESULTS.db --sizes FILE.json
      kernel time of each wire kernel from a `rocprofv3 --kernel-trace --stats` run of the first form, and its algorithmic bytes over that
      time as a share of the 8 TB/s HBM peak.
Algorithmic bytes: pack reads 5n + 451 T and writes as much; unpack reads the 5n + 451 T of the wire form and writes n (225 + 4 + 1 + 101 250)."""
import argparse
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
N = 225


def sizes(n, T):
    wire = 5 * n + 451 * T
    return {"games": n, "moves_T": T, "wire_bytes": wire, "visit_section_odd": (5 * n + T) % 2,
            "pack_bytes": 2 * wire, "unpack_bytes": wire + n * (225 + 4 + 1 + 101250)}


def from_stats(stats_csv, sizes_json):
    sz = json.load(open(sizes_json))["sizes"]
    rows = {}
    if stats_csv.endswith(".db"):                          # rocprofv3's default SQLite output
        import sqlite3
        for name, calls, total in sqlite3.connect(stats_csv).execute("select name, count(*), sum(end - start) from kernels group by name"):
            rows[name] = (int(calls), float(total))
    else:
        for r in csv.DictReader(open(stats_csv)):
            rows[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    out = []
    for kernel, key in (("records_pack_kernel", "pack_bytes"), ("records_unpack_kernel", "unpack_bytes")):
        hits = [(name, v) for name, v in rows.items() if kernel in name]
        if not hits:
            out.append({"kernel": kernel, "missing": True})
            continue
        calls, total = hits[0][1]
        per = total / calls * 1e-9
        out.append({"kernel": kernel, "calls": calls, "mean_ms": per * 1e3, "alg_bytes": sz[key], "GB_per_s": sz[key] / per / 1e9,
                    "share_of_8TBps": sz[key] / per / HBM_PEAK})
    for name, (calls, total) in sorted(rows.items()):
        if "records_scan" in name or "samples_from" in name:
            out.append({"kernel": re.search(r"(records_scan_\w+|samples_from_\w+)", name).group(1), "calls": calls, "mean_ms": total / calls * 1e-6})
    for o in out:
        print(json.dumps(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--sizes", default=None)
    a = ap.parse_args()
    if a.stats:
        return from_stats(a.stats, a.sizes)

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd import selfplay
    G.init(0)
    dev = "cuda"
    play = selfplay.play_games(512, 100, seed=1, record_visits=False)
    played = play.lens.cpu().numpy()
    rng = np.random.default_rng(1234)
    lens_np = played[rng.integers(0, len(played), a.games)].astype(np.int32)
    n = a.games
    g = torch.Generator(device=dev).manual_seed(1234)
    lens = torch.from_numpy(lens_np).to(dev)
    moves = torch.argsort(torch.rand((n, N), generator=g, device=dev), dim=1).to(torch.uint8)
    winner = torch.randint(-1, 2, (n,), generator=g, device=dev, dtype=torch.int8)
    visits = torch.randint(-32768, 32768, (n, N, N), generator=g, device=dev, dtype=torch.int16)
    rec = selfplay.GameRecords(moves, lens, winner, visits)
    T = int(lens_np.sum())
    sz = sizes(n, T)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e-3, r

    res = {"sizes": sz, "lengths": {"source": "selfplay.play_games(512, 100, seed=1) lengths, tiled with numpy default_rng(1234)",
                                    "mean": float(lens_np.mean()), "min": int(lens_np.min()), "max": int(lens_np.max())}, "reps": a.reps}
    t_pt, buf_pt = timed(lambda: selfplay.pack_records(rec))
    t_pd, buf_pd = timed(lambda: selfplay.pack_records_device(rec))
    assert torch.equal(buf_pt, buf_pd), "device pack differs from pack_records"
    res["pack"] = {"torch_s": t_pt, "device_s": t_pd, "torch_GBps": sz["pack_bytes"] / t_pt / 1e9, "device_GBps": sz["pack_bytes"] / t_pd / 1e9}
    del buf_pt
    t_ut, up_t = timed(lambda: selfplay.unpack_records(buf_pd, n, True))
    del up_t
    t_ud, up_d = timed(lambda: selfplay.unpack_records_device(buf_pd, n, True))
    ref = selfplay.unpack_records(buf_pd, n, True)
    assert torch.equal(up_d.visits, ref.visits) and torch.equal(up_d.moves, ref.moves) and torch.equal(up_d.lens, ref.lens), "device unpack differs"
    del up_d
    res["unpack"] = {"torch_s": t_ut, "device_s": t_ud, "torch_GBps": sz["unpack_bytes"] / t_ut / 1e9, "device_GBps": sz["unpack_bytes"] / t_ud / 1e9}
    S = T
    out_bytes = S * (6 * N + 4 + 4 * N)
    t_st, s_t = timed(lambda: selfplay.unpack_records(buf_pd, n, True).to_samples())
    del ref
    t_sd, s_d = timed(lambda: selfplay.samples_from_packed(buf_pd, n))
    assert all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(s_t, s_d)), "tuples differ"
    res["samples"] = {"torch_s": t_st, "device_s": t_sd, "samples": S, "output_bytes": out_bytes,
                      "torch_output_GBps": out_bytes / t_st / 1e9, "device_output_GBps": out_bytes / t_sd / 1e9}
    res["device"] = G.device_info()["name"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
