#!/usr/bin/env python3
"""What a root-parallel ensemble (gomokuai_amd/ensemble.py, K13) costs and buys on ONE position, by the number of replicas.

  python tools/ensemble_time.py [--k3 1,64,1024,4096] [--k6 1,64,2048] [--playouts 1000] [--rounds 5] [--limit 240]
                                [--match] [--out profiles/ensemble_time.json]

Search leg: the 4-ply opening of tools/mcts_one_game.py, searched by EnsembleSearch with `playouts` playouts per replica -- K3 ("random")
and K6 ("traditional", root noise 0.05 / 0.25 from the counter sampler) -- for every replica count R.  Per row, after one warm-up search of
the same shape: the search and the merge (all seven outputs) timed separately by HIP events, median of `rounds`; total playouts per second;
the merge's share of the search; the ratio of playouts per second to the R = 1 row of the same run.  The R = 1 row is the handle as it is
used without ensembles (one game, one wavefront): the yardstick, and the figure tools/mcts_one_game.py gives on the commit before.
Match leg (--match): 16 games, sides alternating, K3 with 256 replicas against K3 with one at 200 playouts per replica and move, from the
empty board; the score of the ensemble side (win 1, draw 0.5).  Sixteen games show a direction, not a strength.
Every row runs in a process of its own under a time limit (`--limit` seconds); the first row that fails or runs out of time ends the run,
and what was measured until then is written with the failure named."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _opening():
    import numpy as np
    from gomokuai_amd import lib as G
    moves, lens, _ = G.synth_boards(1, 0)
    return [int(c) for c in moves[0, :min(int(lens[0]), 4)]]


def search_row(policy, replicas, playouts, rounds):
    import numpy as np
    import torch
    from gomokuai_amd import lib as G
    from gomokuai_amd.ensemble import EnsembleSearch
    G.init(0)
    opening = _opening()
    noise = (0.05, 0.25) if policy == "traditional" else None
    es = EnsembleSearch(policy, replicas, root_noise=noise, playouts_capacity=playouts)
    dev = torch.device("cuda")
    out = dict(visits=torch.empty((1, 225), dtype=torch.int32, device=dev), values=torch.empty((1, 225), dtype=torch.float32, device=dev),
               cells=torch.empty(1, dtype=torch.int16, device=dev), cells_per_game=torch.empty(replicas, dtype=torch.int16, device=dev),
               root_visits=torch.empty(1, dtype=torch.int32, device=dev), root_value=torch.empty(1, dtype=torch.float32, device=dev),
               status=torch.empty(1, dtype=torch.int32, device=dev))
    search_ms, merge_ms = [], []
    for r in range(rounds + 1):                                   # round 0 warms up
        es.set_positions([opening])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        es.search(playouts)
        ev[1].record()
        es._merge(**out)
        ev[2].record()
        torch.cuda.synchronize()
        if r:
            search_ms.append(ev[0].elapsed_time(ev[1]))
            merge_ms.append(ev[1].elapsed_time(ev[2]))
    assert int(out["status"][0]) == 0 and int(out["root_visits"][0]) == replicas * playouts, (int(out["status"][0]), int(out["root_visits"][0]))
    s, m = float(np.median(search_ms)), float(np.median(merge_ms))
    es.close()
    return {"policy": policy, "replicas": replicas, "playouts_per_replica": playouts, "search_ms": s, "merge_ms": m, "search_ms_all": search_ms,
            "merge_ms_all": merge_ms, "merge_share_of_search": m / s, "playouts_per_s": replicas * playouts / ((s + m) * 1e-3),
            "merged_cell": int(out["cells"][0]), "device": G.device_info()["name"]}


def match_row(games, replicas, playouts):
    import numpy as np
    import torch
    from gomokuai_amd import core
    from gomokuai_amd import lib as G
    from gomokuai_amd.ensemble import EnsembleSearch
    G.init(0)
    sides = [EnsembleSearch("random", replicas, first_game_id=0, playouts_capacity=playouts),
             EnsembleSearch("random", 1, first_game_id=1 << 20, playouts_capacity=playouts)]
    score, results, plies = 0.0, [], 0
    for g in range(games):
        board = core.Board()
        black = g % 2                                            # the side that plays black: alternating
        side = black
        while board.status["cur_player"] != core.Player.none:
            es = sides[side]
            es.set_positions([[int(p.id) for p in board.move_record]], ensemble_ids=[g])
            es.search(playouts)
            board.apply_move(core.Position(int(np.argmax(es.eval_state()[0][1]))))
            side ^= 1
            plies += 1
        winner = board.status["winner"]
        result = 0.5 if winner == core.Player.none else float((winner == core.Player.black) == (black == 0))
        score += result
        results.append(result)
    for es in sides:
        es.close()
    return {"games": games, "policy": "random", "replicas": [replicas, 1], "playouts_per_replica_per_move": playouts, "ensemble_score": score,
            "results": results, "plies": plies}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k3", default="1,64,1024,4096")
    ap.add_argument("--k6", default="1,64,2048")
    ap.add_argument("--playouts", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a row may take")
    ap.add_argument("--match", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--row", default=None, help="(internal) run one row in this process: policy,replicas or match")
    a = ap.parse_args()
    if a.row:
        row = match_row(16, 256, 200) if a.row == "match" else search_row(a.row.split(",")[0], int(a.row.split(",")[1]), a.playouts, a.rounds)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = [("random", int(x)) for x in a.k3.split(",") if x] + [("traditional", int(x)) for x in a.k6.split(",") if x]
    res = {"playouts": a.playouts, "rounds": a.rounds, "search": [], "match": "not measured", "failure": None}
    jobs = ["%s,%d" % r for r in rows] + (["match"] if a.match else [])
    for job in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", job, "--playouts", str(a.playouts), "--rounds", str(a.rounds)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit * (3 if job == "match" else 1))
        except subprocess.TimeoutExpired:
            res["failure"] = "%s: no result within its time limit" % job
            break
        line = next((l for l in done.stdout.splitlines() if l.startswith("ROW ")), None)
        if done.returncode != 0 or line is None:
            res["failure"] = "%s: exit status %d: %s" % (job, done.returncode, done.stderr.strip().splitlines()[-1:] or "")
            break
        row = json.loads(line[4:])
        if job == "match":
            res["match"] = row
        else:
            base = next((b for b in res["search"] if b["policy"] == row["policy"] and b["replicas"] == 1), None)
            row["playouts_per_s_over_one_replica"] = row["playouts_per_s"] / base["playouts_per_s"] if base else None
            res["search"].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 1 if res["failure"] else 0


if __name__ == "__main__":
    sys.exit(main())
