#!/usr/bin/env python3
"""Timing of K17 on the device: the threat cells (vcf_threats_kernel.hip) and the forced-win search by continuous threats (vct_kernel.hip).

  python tools/vct_time.py [--roots 64] [--depth 8] [--budget 1000] [--max-positions 512] [--reps 3] [--out profiles/vct_time.json]

The lists are tools/vcf_time.py's -- random-opening move lists (synth_boards kind 0, whole lists: 8 .. 60 moves) -- the first --roots of them,
inputs and outputs resident on the device.  First one call of gmk_vcf_threats over them: milliseconds per call and the verdict histogram.
Then gmk_vct_solve at max_threats T = 1, 2, 3: milliseconds per call (host clock: the call synchronises between its levels), the statuses, the
positions searched, and the size of level T over the batch -- the positions of T less those of T - 1, since a root that ended below T has
the same count at both.  --max-positions is the cap per root and level; the batch is chosen so that a level fits.
Every time is the mean of --reps runs after one warm-up run.  Nothing sets a bar for these figures; they are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--budget", type=int, default=1000)
    ap.add_argument("--max-positions", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    G.init(0)
    stream = torch.cuda.current_stream().cuda_stream
    n = a.roots
    res = {"device": G.device_info()["name"], "reps": a.reps, "roots": n, "max_depth": a.depth, "budget": a.budget, "max_positions": a.max_positions}

    def timed(fn):
        times = []
        for r in range(a.reps + 1):                              # run 0 warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
        return float(np.mean(times)), float(np.min(times)), float(np.max(times))

    moves, lens, _ = G.synth_boards(n, 0, first_board=0)
    stride = moves.shape[1]
    res["mean_list_length"] = float(lens.mean())
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    own = torch.empty(n, dtype=torch.int32, device="cuda")
    verdict = torch.empty((n, 225), dtype=torch.uint8, device="cuda")
    nodes = torch.empty((n, 225), dtype=torch.int32, device="cuda")
    mean, lo, hi = timed(lambda: G.vcf_threats_device(d_moves.data_ptr(), stride, d_lens.data_ptr(), n, a.depth, a.budget, d_own_status=own.data_ptr(),
                                                      d_verdict=verdict.data_ptr(), d_cell_nodes=nodes.data_ptr(), stream=stream))
    v, nd = verdict.cpu().numpy(), nodes.cpu().numpy().view(np.uint32).astype(np.int64)
    res["threats"] = {"ms_per_call": mean * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3, "positions_per_s": n / mean,
                      "own_status": {name: int((own.cpu().numpy() == i).sum()) for i, name in enumerate(G.VCF_STATUS_NAMES)},
                      "verdict": {name: int((v == i).sum()) for i, name in enumerate(G.VCF_THREAT_NAMES)},
                      "cell_nodes_total": int(nd.sum()), "cell_nodes_max": int(nd.max())}
    print(json.dumps(res["threats"]), flush=True)

    status = torch.empty(n, dtype=torch.int32, device="cuda")
    threats = torch.empty(n, dtype=torch.int32, device="cuda")
    positions = torch.empty(n, dtype=torch.int32, device="cuda")
    before = n
    for t in (1, 2, 3):
        mean, lo, hi = timed(lambda: G.vct_solve_device(d_moves.data_ptr(), stride, d_lens.data_ptr(), n, a.depth, a.budget, max_threats=t,
                                                        max_positions=a.max_positions, d_status=status.data_ptr(), d_threats=threats.data_ptr(),
                                                        d_positions=positions.data_ptr(), stream=stream))
        st, th, total = status.cpu().numpy(), threats.cpu().numpy(), int(positions.cpu().numpy().astype(np.int64).sum())
        res["max_threats_%d" % t] = {"ms_per_call": mean * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3, "positions": total, "level_positions": total - before,
                                     "positions_per_s": total / mean, "status": {name: int((st == i).sum()) for i, name in enumerate(G.VCT_STATUS_NAMES)},
                                     "wins_by_threats": {str(d): int(((st == G.VCF_WIN) & (th == d)).sum()) for d in range(t + 1)}}
        before = total
        print(json.dumps(res["max_threats_%d" % t]), flush=True)
    text = "{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res.items()) + "\n}"      # one key per line
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
