#!/usr/bin/env python3
"""Timing of K14, the forced-win solver by continuous fours on the device (vcf_kernel.hip).

  python tools/vcf_time.py [--positions 65536] [--budget 10000] [--reps 10] [--out profiles/vcf_time.json]

One launch of gmk_vcf_solve over --positions random-opening move lists (synth_boards kind 0, whole lists: 8 .. 60 moves, the generator
tools/pattern_time.py uses), inputs and outputs resident on the device, at max_depth 8 and 16, plain and iterative: milliseconds per launch,
positions/s, nodes/s (four-making candidates tried), the status histogram and the largest node count of a position.  Beside each, the same
launch for ONE position (n = 1): the batch's first position and its heaviest one -- what a front end pays per move.
Every figure is the mean of --reps runs after one warm-up run, device events around work that ends in a synchronise."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=65536)
    ap.add_argument("--budget", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    G.init(0)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"device": G.device_info()["name"], "reps": a.reps, "positions": a.positions, "budget": a.budget}

    def device_timed(fn):
        times = []
        for r in range(a.reps + 1):                              # run 0 warms up
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.mean(times)), float(np.min(times)), float(np.max(times))

    n = a.positions
    moves, lens, _ = G.synth_boards(n, 0, first_board=0)
    stride = moves.shape[1]
    d_moves, d_lens = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    move = torch.empty(n, dtype=torch.int32, device="cuda")
    length = torch.empty(n, dtype=torch.int32, device="cuda")
    nodes = torch.empty(n, dtype=torch.int32, device="cuda")
    pv = torch.empty((n, G.VCF_PV), dtype=torch.uint8, device="cuda")

    def launch(first, count, max_depth, iterative):
        G.vcf_solve_device(d_moves.data_ptr() + first * stride, stride, d_lens.data_ptr() + 4 * first, count, max_depth, a.budget, iterative=iterative,
                           d_status=status.data_ptr(), d_move=move.data_ptr(), d_length=length.data_ptr(), d_nodes=nodes.data_ptr(), d_pv=pv.data_ptr(),
                           stream=stream)

    for max_depth in (8, 16):
        for iterative in (False, True):
            mean, lo, hi = device_timed(lambda: launch(0, n, max_depth, iterative))
            st = status.cpu().numpy()
            nd = nodes.cpu().numpy().view(np.uint32).astype(np.int64)
            ln = length.cpu().numpy()
            heaviest = int(nd.argmax())
            entry = {"max_depth": max_depth, "iterative": iterative, "mean_list_length": float(lens.mean()),
                     "ms_per_launch": mean * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3, "positions_per_s": n / mean, "nodes_per_s": float(nd.sum()) / mean,
                     "nodes_total": int(nd.sum()), "nodes_max": int(nd.max()), "longest_win": int(ln.max()),
                     "status": {name: int((st == i).sum()) for i, name in enumerate(G.VCF_STATUS_NAMES)}}
            for label, first in (("first", 0), ("heaviest", heaviest)):
                mean1, lo1, hi1 = device_timed(lambda: launch(first, 1, max_depth, iterative))
                entry["one_position_" + label] = {"index": first, "ms_per_launch": mean1 * 1e3, "ms_min": lo1 * 1e3, "ms_max": hi1 * 1e3,
                                                  "nodes": int(nodes[0].item()), "status": G.VCF_STATUS_NAMES[int(status[0].item())]}
            res["depth%d_%s" % (max_depth, "iterative" if iterative else "plain")] = entry
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
