#!/usr/bin/env python3
"""K6 timing aid: n games x playouts of the pattern-guided search, whole-launch time; and the oracle on one core.
--rave: the same searches with TraditionalPolicy(use_rave=True) (gmk_trad_run_rave) next to plain K6, their ratio, and the persistent
self-play loop with the reference agent's semantics (kept subtrees + counter-sampler noise) for both policies: --sup-games games through
n slots (tools/trad_time.py --rave [n playouts cap] [--sup-games 16384])."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gomokuai_amd import lib as G
torch.cuda.set_device(0); G.init(0)
rave = "--rave" in sys.argv
sup_games = int(sys.argv[sys.argv.index("--sup-games") + 1]) if "--sup-games" in sys.argv else 16384
sys.argv = [a for i, a in enumerate(sys.argv) if a != "--rave" and a != "--sup-games" and (i == 0 or sys.argv[i - 1] != "--sup-games")]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
playouts = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 18
moves, lens, _ = G.synth_boards(n, 1)
pos = [[int(m) for m in moves[g, :min(int(lens[g]), 12)]] for g in range(n)]
t = G.TraditionalMCTS(n, node_capacity=cap)
t.set_positions(pos); t.run(10); torch.cuda.synchronize()
t.set_positions(pos)
t0 = time.perf_counter(); t.run(playouts); torch.cuda.synchronize(); dt = time.perf_counter() - t0
s = t.root_stats()
print("gpu: %d games x %d playouts in %.3f s = %.2f M playouts/s; nodes/game mean %.0f max %d; status!=0: %d; updates/playout %.2f" %
      (n, playouts, dt, n * playouts / dt / 1e6, s["n_nodes"].mean(), s["n_nodes"].max(), int((s["status"] != 0).sum()), s["evaluator_updates"].mean() / playouts))
if rave:
    t.close()
    r = G.TraditionalRAVEMCTS(n, node_capacity=cap)
    r.set_positions(pos); r.run(10); torch.cuda.synchronize()
    r.set_positions(pos)
    t0 = time.perf_counter(); r.run(playouts); torch.cuda.synchronize(); dr = time.perf_counter() - t0
    s = r.root_stats()
    r.close()
    print("gpu rave: %d games x %d playouts in %.3f s = %.2f M playouts/s (%.3f x plain K6); nodes/game mean %.0f max %d; status!=0: %d" %
          (n, playouts, dr, n * playouts / dr / 1e6, dt / dr, s["n_nodes"].mean(), s["n_nodes"].max(), int((s["status"] != 0).sum())))
    from gomokuai_amd import selfplay
    for policy in ("traditional", "traditional_rave"):
        kw = dict(n_games=sup_games, playouts=playouts, slots=n, opening_plies=2, reuse_subtree=True, root_noise=(0.05, 0.25), policy=policy,
                  device_loop="persistent", node_capacity=min(3 * cap, (1 << 24) - 1))
        selfplay.play_supervisor_games(prepare_only=True, **kw)
        t0 = time.perf_counter(); rec = selfplay.play_supervisor_games(**kw); torch.cuda.synchronize(); ds = time.perf_counter() - t0
        moves = int(rec.lens.sum().item()) - 2 * sup_games
        print("persistent self-play, %s, reference semantics: %d games through %d slots, %d searched moves in %.2f s = %.0f games/s, %.2f M playouts/s; overflow %s" %
              (policy, sup_games, n, moves, ds, sup_games / ds, moves * playouts / ds / 1e6, rec.overflow))
    sys.exit(0)
from oracle import oracle as O
t0 = time.perf_counter(); k = 0
while time.perf_counter() - t0 < 5 and k < n:
    o = O.TraditionalMCTS(5.0); o.search(pos[k], playouts); k += 1
dt = time.perf_counter() - t0
print("cpu oracle, 1 core: %d searches in %.2f s = %.1f k playouts/s" % (k, dt, k * playouts / dt / 1e3))
