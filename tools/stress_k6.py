"""K6 (and through it K2's device functions) against the oracle on randomly drawn positions: clustered and random synthetic games cut at random
lengths, 100 .. 700 playouts, several c_puct, 1 .. 40 games per search (workgroups partly filled), a second search on the same handle from a
continued position (the evaluator is synchronised, not rebuilt).  Compared exactly: visit counts, the bits of values and priors, the move to
play, tree size, the number of evaluator updates, and the evaluator state left behind (scores, density, pattern and compound flag words).
tools/stress_k6.py [seconds]; run(budget, seed) is what tests/test_stress_gpu.py calls for a bounded slice.
tools/stress_k6.py --rave [seconds]: TraditionalPolicy(use_rave=True) (gmk_trad_run_rave) against the Python restatement of
tests/trad_rave_reference.py (30 .. 150 playouts, the restatement on a pool of worker processes that do not touch the GPU), the AMAF
statistics compared too (the evaluator state is not: the restatement's evaluator is the oracle's, which K6's plain leg checks)."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gomokuai_amd import lib as G
from oracle import oracle as O

L = None


def same(stats, dev, g, orc):
    v, q, p, best = orc.root_children()
    ok = stats["status"][g] == 0 and (stats["visits"][g] == v).all() and (stats["priors"][g].view(np.uint32) == p.view(np.uint32)).all() and \
         (stats["values"][g].view(np.uint32) == q.view(np.uint32)).all() and stats["best"][g] == best and stats["root_visits"][g] == orc.root_visits and \
         np.float32(stats["root_value"][g]).view(np.uint32) == np.float32(orc.root_value).view(np.uint32) and stats["n_nodes"][g] == orc.n_nodes and \
         stats["evaluator_updates"][g] == orc.evaluator_updates
    ev = L.go_trad_evaluator(orc.h)
    scores = np.zeros((4, 225), np.int32); density = np.zeros((2, 2, 225), np.int32)
    pd = np.zeros((226, 8), np.uint32); cd = np.zeros((226, 3), np.uint32)
    L.go_eval_get_scores(C.c_void_p(ev), scores.ctypes.data); L.go_eval_get_density(C.c_void_p(ev), density.ctypes.data)
    L.go_eval_get_pattern_dist(C.c_void_p(ev), pd.ctypes.data); L.go_eval_get_compound_dist(C.c_void_p(ev), cd.ctypes.data)
    return bool(ok) and (dev["scores"][g] == scores).all() and (dev["density"][g] == density).all() and (dev["pattern_dist"][g] == pd).all() and (dev["compound_dist"][g] == cd).all()


def run(budget=240.0, seed=4101, verbose=True):
    """Random configurations from the stream of RandomState(seed) until `budget` seconds have passed (the stream is the same every time: a failure
    names its configuration).  Returns (searches, game searches compared, mismatches as strings)."""
    global L
    rng = np.random.RandomState(seed)
    G.init(0)
    L = O.lib()
    t0 = time.time(); searches = games = 0; bad = []
    while time.time() - t0 < budget:
        n = int(rng.randint(1, 41)); P = int(rng.randint(100, 700)); c_puct = float(rng.choice([2.0, 5.0])); kind = int(rng.randint(0, 2))
        moves, lens, _ = G.synth_boards(n, kind, first_board=int(rng.randint(0, 2**24)))
        cut = [int(min(lens[g], rng.randint(0, 61))) for g in range(n)]
        pos = [[int(m) for m in moves[g, :cut[g]]] for g in range(n)]
        t = G.TraditionalMCTS(n, node_capacity=1 << 17, c_puct=c_puct)
        t.set_positions(pos)
        t.run(P)
        stats, dev = t.root_stats(), t.read_evaluators()
        orcs = []
        for g in range(n):
            orc = O.TraditionalMCTS(c_puct)
            orc.search(pos[g], P)
            orcs.append(orc)
            if not same(stats, dev, g, orc):
                bad.append("search %d (first): n %d P %d kind %d game %d stones %d" % (searches, n, P, kind, g, cut[g]))
                if verbose:
                    print("MISMATCH " + bad[-1], flush=True)
            games += 1
        # the game goes on by two moves of its own record (where there are any): a second search on the same handle and evaluator
        more = [pos[g] + [int(m) for m in moves[g, cut[g]:min(int(lens[g]), cut[g] + 2)]] for g in range(n)]
        t.set_positions(more)
        t.run(P // 2)
        stats, dev = t.root_stats(), t.read_evaluators()
        for g in range(n):
            orcs[g].search(more[g], P // 2)
            if not same(stats, dev, g, orcs[g]):
                bad.append("search %d (second): n %d P %d kind %d game %d stones %d" % (searches + 1, n, P, kind, g, len(more[g])))
                if verbose:
                    print("MISMATCH " + bad[-1], flush=True)
            games += 1
        t.close()
        searches += 2
        if verbose and searches % 20 == 0:
            print("%d searches, %d game searches compared, %d mismatches, %.0f s" % (searches, games, len(bad), time.time() - t0), flush=True)
    return searches, games, bad


def _rave_reference(job):
    """both searches of one game on one restatement object (its evaluator persists like the device's): root statistics of each"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from trad_rave_reference import TradRAVEReference
    c_puct, P, first, second = job
    ref, out = TradRAVEReference(c_puct, use_rave=True), []
    for pos, playouts in ((first, P), (second, P // 2)):
        ref.search(pos, playouts)
        out.append((ref.root_children(), ref.root_visits, ref.root_value, ref.n_nodes, ref.evaluator_updates))
    return out


def same_rave(st, g, got):
    (v, q, p, av, aq, best), rv, rq, n_nodes, updates = got
    return bool(st["status"][g] == 0 and (st["visits"][g] == v).all() and (st["values"][g].view(np.uint32) == q.view(np.uint32)).all() and
                (st["priors"][g].view(np.uint32) == p.view(np.uint32)).all() and (st["amaf_visits"][g] == av).all() and
                (st["amaf_values"][g].view(np.uint32) == aq.view(np.uint32)).all() and st["best"][g] == best and st["root_visits"][g] == rv and
                np.float32(st["root_value"][g]).view(np.uint32) == np.float32(rq).view(np.uint32) and st["n_nodes"][g] == n_nodes and
                st["evaluator_updates"][g] == updates)


def run_rave(budget=240.0, seed=4201, verbose=True, workers=12):
    """run() for TraditionalRAVEMCTS against tests/trad_rave_reference.py; returns (searches, game searches compared, mismatches)"""
    import multiprocessing as mp
    rng = np.random.RandomState(seed)
    G.init(0)
    pool = mp.get_context("spawn").Pool(workers)
    t0 = time.time(); searches = games = 0; bad = []
    try:
        while time.time() - t0 < budget:
            n = int(rng.randint(1, 41)); P = int(rng.randint(30, 151)); c_puct = float(rng.choice([2.0, 5.0])); kind = int(rng.randint(0, 2))
            moves, lens, _ = G.synth_boards(n, kind, first_board=int(rng.randint(0, 2**24)))
            cut = [int(min(lens[g], rng.randint(0, 61))) for g in range(n)]
            pos = [[int(m) for m in moves[g, :cut[g]]] for g in range(n)]
            more = [pos[g] + [int(m) for m in moves[g, cut[g]:min(int(lens[g]), cut[g] + 2)]] for g in range(n)]
            refs = pool.map_async(_rave_reference, [(c_puct, P, pos[g], more[g]) for g in range(n)])
            t = G.TraditionalRAVEMCTS(n, node_capacity=1 << 16, c_puct=c_puct)
            t.set_positions(pos)
            t.run(P)
            stats = [t.root_stats()]
            t.set_positions(more)
            t.run(P // 2)
            stats.append(t.root_stats())
            t.close()
            refs = refs.get()
            for g in range(n):
                for k in (0, 1):
                    if not same_rave(stats[k], g, refs[g][k]):
                        bad.append("search %d: n %d P %d c_puct %g kind %d game %d stones %d" % (searches + k, n, P, c_puct, kind, g, len((pos, more)[k][g])))
                        if verbose:
                            print("MISMATCH " + bad[-1], flush=True)
                    games += 1
            searches += 2
            if verbose and searches % 20 == 0:
                print("%d searches, %d game searches compared, %d mismatches, %.0f s" % (searches, games, len(bad), time.time() - t0), flush=True)
    finally:
        pool.close()
        pool.join()
    return searches, games, bad


if __name__ == "__main__":
    if "--rave" in sys.argv:
        args = [a for a in sys.argv[1:] if a != "--rave"]
        searches, games, bad = run_rave(float(args[0]) if args else 240.0)
        print("K6 + RAVE stress parity: %d searches, %d game searches compared with the restatement (visits, value, prior and AMAF bits, AMAF visits, best move, tree size, evaluator updates): %d mismatches" % (searches, games, len(bad)))
        sys.exit(1 if bad else 0)
    searches, games, bad = run(float(sys.argv[1]) if len(sys.argv) > 1 else 240.0)
    print("K6 stress parity: %d searches, %d game searches compared with the oracle (visits, value and prior bits, best move, tree size, evaluator updates, evaluator state with its flag words): %d mismatches" % (searches, games, len(bad)))
    sys.exit(1 if bad else 0)
