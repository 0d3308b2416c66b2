#!/usr/bin/env python3
"""Timing of K15, the defence against a forced win by continuous fours on the device (vcf_defend_kernel.hip), beside K14's own figures.

  python tools/vcf_defend_time.py [--positions 65536] [--budget 10000] [--reps 10] [--parent-tree DIR] [--out profiles/vcf_defend_time.json]

One call of gmk_vcf_defend (two launches: the threat, then the cells) over tools/vcf_time.py's lists -- --positions random-opening move lists
(synth_boards kind 0, whole lists: 8 .. 60 moves) -- inputs and outputs resident on the device, at max_depth 8 and 16: milliseconds per call,
positions/s, the share of positions under a threat (threat WIN), the cells searched per threatened position (cells that hold or are unknown,
and losing cells with nodes: what the threat's own line did not settle), the verdict histogram and the nodes.  Beside each, the same call for
ONE position: the first quiet one (threat NONE) and the first threatened one -- what a front end pays per move.
Then tools/vcf_time.py's four rows of K14 alone, rerun by that tool in a process of its own on this tree and, with --parent-tree DIR (a built
checkout of the parent commit), on the parent: K14 shares its device functions with K15 and must not have become slower.
Every figure is the mean of --reps runs after one warm-up run, device events around work that ends in a synchronise."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K14_ROWS = ("depth8_plain", "depth8_iterative", "depth16_plain", "depth16_iterative")


def k14_rows(tree, a):
    """tools/vcf_time.py of `tree`, in a process of its own with that tree's package -> its record"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "vcf_time.json")
        subprocess.run([sys.executable, os.path.join(tree, "tools", "vcf_time.py"), "--positions", str(a.positions), "--budget", str(a.budget),
                        "--reps", str(a.reps), "--out", out], check=True, cwd=tree, stdout=subprocess.DEVNULL)
        with open(out) as f:
            return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=65536)
    ap.add_argument("--budget", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its tools/vcf_time.py is run for comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    # K14 alone first, each in a fresh process, before this one touches the device
    k14 = {"this": k14_rows(ROOT, a)}
    if a.parent_tree:
        k14["parent"] = k14_rows(os.path.abspath(a.parent_tree), a)
        k14["this_over_parent_ms"] = {row: k14["this"][row]["ms_per_launch"] / k14["parent"][row]["ms_per_launch"] for row in K14_ROWS}

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
    length = torch.empty(n, dtype=torch.int32, device="cuda")
    threat_nodes = torch.empty(n, dtype=torch.int32, device="cuda")
    pv = torch.empty((n, G.VCF_PV), dtype=torch.uint8, device="cuda")
    verdict = torch.empty((n, 225), dtype=torch.uint8, device="cuda")
    cell_length = torch.empty((n, 225), dtype=torch.uint8, device="cuda")
    cell_nodes = torch.empty((n, 225), dtype=torch.int32, device="cuda")

    def call(first, count, max_depth):
        G.vcf_defend_device(d_moves.data_ptr() + first * stride, stride, d_lens.data_ptr() + 4 * first, count, max_depth, a.budget,
                            d_threat_status=status.data_ptr(), d_threat_length=length.data_ptr(), d_threat_pv=pv.data_ptr(),
                            d_threat_nodes=threat_nodes.data_ptr(), d_verdict=verdict.data_ptr(), d_cell_length=cell_length.data_ptr(),
                            d_cell_nodes=cell_nodes.data_ptr(), stream=stream)

    def searched_cells(v, nd):
        return int(((v == G.VCF_CELL_HOLDS) | (v == G.VCF_CELL_UNKNOWN) | ((v == G.VCF_CELL_LOSES) & (nd > 0))).sum())

    for max_depth in (8, 16):
        mean, lo, hi = device_timed(lambda: call(0, n, max_depth))
        st = status.cpu().numpy()
        v = verdict.cpu().numpy()
        nd = cell_nodes.cpu().numpy().view(np.uint32).astype(np.int64)
        threatened = st == G.VCF_WIN
        searched = searched_cells(v[threatened], nd[threatened])
        entry = {"max_depth": max_depth, "mean_list_length": float(lens.mean()), "ms_per_call": mean * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3,
                 "positions_per_s": n / mean, "threatened_share": float(threatened.mean()), "threatened": int(threatened.sum()),
                 "searched_cells": searched, "searched_cells_per_threatened_position": searched / max(1, int(threatened.sum())),
                 "cell_nodes_total": int(nd.sum()), "cell_nodes_max": int(nd.max()), "cell_nodes_per_s": float(nd.sum()) / mean,
                 "threat_status": {name: int((st == i).sum()) for i, name in enumerate(G.VCF_STATUS_NAMES)},
                 "verdict": {name: int((v == i).sum()) for i, name in enumerate(G.VCF_CELL_NAMES)}}
        for label, first in (("quiet", int(np.flatnonzero(st == G.VCF_NONE)[0])), ("threatened", int(np.flatnonzero(threatened)[0]))):
            mean1, lo1, hi1 = device_timed(lambda: call(first, 1, max_depth))
            v1, nd1 = verdict[0].cpu().numpy(), cell_nodes[0].cpu().numpy().view(np.uint32).astype(np.int64)
            entry["one_position_" + label] = {"index": first, "ms_per_call": mean1 * 1e3, "ms_min": lo1 * 1e3, "ms_max": hi1 * 1e3,
                                              "threat": G.VCF_STATUS_NAMES[int(status[0].item())], "searched_cells": searched_cells(v1, nd1) if label == "threatened" else 0,
                                              "cell_nodes": int(nd1.sum()), "holds": int((v1 == G.VCF_CELL_HOLDS).sum())}
        res["depth%d" % max_depth] = entry
    res["k14_alone"] = k14
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
