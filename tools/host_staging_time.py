"""Wall time per call of the root read-outs and the batch host forms: the median over 200 calls of each, one line per entry.

    python tools/host_staging_time.py [--root CHECKOUT] [--calls 200] [--json FILE]

root_stats() on 1 024-game K3, K6 and K7 handles after one short search; vcf_solve and pattern_policy at n = 64; eval_batch_host at
n = 2 048.  These calls allocate, copy, launch, synchronise and free on the host's clock, so the figure is wall time around the call.  Run
it on two checkouts in turn (--root: the checkout whose built package is measured; this one by default) to compare them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def median_us(call, calls):
    for _ in range(10):
        call()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from gomokuai_amd import lib as G
    G.init()
    print("package: %s" % os.path.relpath(os.path.dirname(G.__file__)))
    n = 1024
    moves, lens, planes = G.synth_boards(n, 0, stride=225)
    lens = np.minimum(lens, 6).astype(np.int32)
    planes = G.moves_to_planes(moves, lens)
    last = np.stack([moves[np.arange(n), lens - 1], moves[np.arange(n), lens - 2]], axis=1).astype(np.int16)

    k3 = G.BatchedMCTS(n, playouts_capacity=8)
    k3.set_roots(planes, last[:, 0])
    k3.run(8)
    k6 = G.TraditionalMCTS(n, node_capacity=4096)
    k6.set_positions(moves, lens)
    k6.run(8)
    k7 = G.AlphaZeroMCTS(n, node_capacity=4096)
    k7.set_roots(planes, last)
    rows = k7.select().shape[0]
    k7.expand(torch.zeros(rows, dtype=torch.float32, device="cuda"), torch.full((rows, 225), 1.0 / 225, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    big_planes = G.synth_boards(2048, 0)[2]

    lines = {
        "k3_root_stats_n1024": k3.root_stats,
        "k6_root_stats_n1024": k6.root_stats,
        "k7_root_stats_n1024": k7.root_stats,
        "vcf_solve_n64": lambda: G.vcf_solve(moves[:64], lens[:64], 4, 64),
        "pattern_policy_n64": lambda: G.pattern_policy(moves[:64], lens[:64]),
        "eval_batch_host_n2048": lambda: G.eval_batch_host(big_planes),
    }
    result = {name: round(median_us(call, args.calls), 1) for name, call in lines.items()}
    for name, us in result.items():
        print("%-24s %10.1f us" % (name, us))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
