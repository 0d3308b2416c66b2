"""TraditionalPolicy(use_rave=True) on the device (gmk_trad_run_rave: K6's playout with RAVE::BackPropogate<true> against the leaf
position) against the Python restatement over the oracle's evaluator (tests/trad_rave_reference.py, itself held to oracle/go_trad.c
with use_rave=False).  PUCB and the HandSelect weighting are double, the running means float on both sides, so everything is
compared exactly: visit counts, the BITS of values, priors and AMAF values, AMAF visit counts, the chosen move, the tree size and
the evaluator updates; then the self-play and match loops that serve the policy."""
import ctypes as C

import numpy as np
import pytest

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay
from trad_rave_reference import TradRAVEReference

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678EF01


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def _positions(n, lo, hi, first):
    moves, lens, _ = G.synth_boards(n, 0, first_board=first)
    out = []
    for g in range(n):
        k = int(min(lens[g], lo + (g * 7) % (hi - lo + 1)))
        out.append([int(m) for m in moves[g, :k]])
    return out


def _compare(st, g, ref, where, n_nodes=None):
    v, q, p, av, aq, best = ref.root_children()
    assert st["status"][g] == 0, where
    np.testing.assert_array_equal(st["visits"][g], v, where)
    np.testing.assert_array_equal(st["values"][g].view(np.uint32), q.view(np.uint32), where)
    np.testing.assert_array_equal(st["priors"][g].view(np.uint32), p.view(np.uint32), where)
    np.testing.assert_array_equal(st["amaf_visits"][g], av, where)
    np.testing.assert_array_equal(st["amaf_values"][g].view(np.uint32), aq.view(np.uint32), where)
    assert st["best"][g] == best and st["root_visits"][g] == ref.root_visits, where
    assert np.float32(st["root_value"][g]).view(np.uint32) == ref.root_value.view(np.uint32), where
    assert st["n_nodes"][g] == (ref.n_nodes if n_nodes is None else n_nodes), where
    assert st["evaluator_updates"][g] == ref.evaluator_updates, where


@pytest.mark.parametrize("c_puct", [5.0, 2.5])
def test_search_matches_the_restatement(gmk, c_puct):
    """fresh roots from 0 to ~60 stones, twice on the same handle (the evaluators persist and are synchronised)"""
    n, playouts = 8, 200
    t = G.TraditionalRAVEMCTS(n, node_capacity=1 << 16, c_puct=c_puct)
    refs = [TradRAVEReference(c_puct, use_rave=True) for _ in range(n)]
    for rnd, first in enumerate((300, 700)):
        pos = _positions(n, 0, 60, first)
        t.set_positions(pos)
        t.run(playouts)
        st = t.root_stats()
        for g in range(n):
            refs[g].search(pos[g], playouts)
            _compare(st, g, refs[g], "round %d game %d" % (rnd, g))
    assert (st["amaf_visits"] > st["visits"]).any()                # siblings played later on the path count as if played first
    t.close()


def test_split_runs_equal_one_run_and_rave_reaches_the_kernel(gmk):
    n = 8
    pos = _positions(n, 6, 40, 40)
    a, b = G.TraditionalRAVEMCTS(n, 1 << 16), G.TraditionalRAVEMCTS(n, 1 << 16)
    plain = G.TraditionalMCTS(n, 1 << 16)
    for t in (a, b, plain):
        t.set_positions(pos)
    a.run(250)
    b.run(100)
    b.run(150)
    plain.run(250)
    sa, sb, sp = a.root_stats(), b.root_stats(), plain.root_stats()
    for k in ("visits", "values", "amaf_visits", "amaf_values", "best", "n_nodes"):
        np.testing.assert_array_equal(sa[k], sb[k], k)
    assert (sa["visits"] != sp["visits"]).any()           # the flag reaches the kernel: some search goes elsewhere than plain K6's
    for t in (a, b, plain):
        t.close()


def test_kept_subtree_and_counter_noise(gmk):
    """gmk_trad_step + gmk_trad_add_root_noise (counter-based sampler) over four moves == the restatement's kept-tree run"""
    n, playouts = 4, 150
    pos = _positions(n, 2, 20, 900)
    t = G.TraditionalRAVEMCTS(n, node_capacity=1 << 17, c_puct=5.0)
    t.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    refs = [TradRAVEReference(5.0, use_rave=True) for _ in range(n)]
    for g, r in enumerate(refs):
        r.set_noise(0.05, 0.25, SEED, 50 + g)
    t.set_positions(pos)
    lists = [list(p) for p in pos]
    for ply in range(4):
        t.add_root_noise(0.05, 0.25, seed=SEED, first_game_id=50)
        t.run(playouts)
        st = t.root_stats()
        for g in range(n):
            refs[g].run(lists[g], playouts)
            _compare(st, g, refs[g], "ply %d game %d" % (ply, g), n_nodes=refs[g].subtree_size())
            lists[g].append(refs[g].step_forward())
        t.step()
    assert st["root_visits"].min() > playouts              # the kept subtrees carried visits over
    t.close()


def test_node_capacity_is_reported(gmk):
    t = G.TraditionalRAVEMCTS(2, node_capacity=300)
    t.set_positions([[112], [112, 113]])
    t.run(400)
    assert (t.root_stats()["status"] & G.TraditionalMCTS.STATUS_ARENA_FULL).all()
    t.close()


def _dense_positions(n, lo, hi, seed):
    """prefixes (lo .. hi stones) of shuffled games between two colour classes that never line up five (as tests/test_trad_gpu.py)"""
    rng = np.random.RandomState(seed)
    cls = lambda c: ((c % 15) // 2 + c // 15) % 2
    blacks, whites = [c for c in range(225) if cls(c) == 0], [c for c in range(225) if cls(c) == 1]
    out = []
    for g in range(n):
        b, w = list(rng.permutation(blacks)), list(rng.permutation(whites))
        seq = []
        while b or w:
            if b:
                seq.append(int(b.pop()))
            if w:
                seq.append(int(w.pop()))
        out.append(seq[:int(rng.randint(lo, hi + 1))])
    return out


def test_nearly_full_boards(gmk):
    """roots with 1 .. 12 empty cells: the searches run into full boards and exhaust their trees"""
    pos = _dense_positions(6, 213, 224, 5)
    t = G.TraditionalRAVEMCTS(len(pos), node_capacity=1 << 16)
    t.set_positions(pos)
    t.run(300)
    st = t.root_stats()
    for g in range(len(pos)):
        ref = TradRAVEReference(5.0, use_rave=True)
        ref.search(pos[g], 300)
        _compare(st, g, ref, "game %d" % g)
    t.close()


def test_policies_do_not_mix_on_a_handle(gmk):
    L = G.load()
    t = G.TraditionalRAVEMCTS(2, 1 << 12)
    t.set_positions([[112], []])
    t.run(10)
    assert L.gmk_trad_run(t.h, 10, 5.0, None) == -4                           # GMK_ERR_STATE
    assert L.gmk_trad_run_poolrave(t.h, 10, 2.0, 0, 0, None) == -4
    t.close()
    for other in (G.TraditionalMCTS(2, 1 << 12), G.PoolRAVEMCTS(2, 1 << 12)):
        other.set_positions([[112], []])
        other.run(10)
        assert L.gmk_trad_run_rave(other.h, 10, 5.0, None) == -4
        other.close()


def _restated_game(game_id, playouts, seed, opening, noise, c_puct=5.0):
    """one TraditionalPolicy(use_rave=True) object for the whole game: run on the kept tree, then stepForward()'s move"""
    from oracle import oracle as O
    L = O.lib()
    b = O.new_board()
    for mv in opening:
        L.go_board_apply(C.byref(b), int(mv), 1)
    r = TradRAVEReference(c_puct, use_rave=True)
    if noise:
        r.set_noise(noise[0], noise[1], seed, game_id)
    moves, visits = [int(x) for x in opening], []
    while b.cur_player != 0:
        r.run(moves, playouts)
        visits.append(r.root_children()[0].copy())
        mv = r.step_forward()
        moves.append(mv)
        L.go_board_apply(C.byref(b), mv, 1)
    return moves, visits, int(b.winner)


@pytest.mark.parametrize("reuse,noise", [(False, None), (True, (0.05, 0.25))])
def test_self_play_loops_play_the_same_games(reuse, noise):
    """play_supervisor_games(policy="traditional_rave"): the persistent loop through 5 and 23 slots, the all-at-once lock-step loop and the
    host loop give the same records; with the reference agent's semantics three games equal the restatement's game loop"""
    n, playouts, seed, first = 12, 20, 7, 61
    kw = dict(c_puct=5.0, policy="traditional_rave", opening_plies=2, first_game_id=first, seed=seed, reuse_subtree=reuse, root_noise=noise)
    host = selfplay.play_supervisor_games(n, playouts, device_loop=False, **kw).cpu()
    runs = [selfplay.play_supervisor_games(n, playouts, device_loop="lockstep", **kw)]
    runs += [selfplay.play_supervisor_games(n, playouts, slots=s, device_loop="persistent", **kw) for s in (5, 23)]
    for i, a in enumerate(runs):
        assert not a.overflow
        a = a.cpu()
        assert (a.lens == host.lens).all() and (a.winner == host.winner).all(), i
        assert (a.moves == host.moves).all() and (a.visits == host.visits).all(), i
    if reuse:
        m, l, _ = G.synth_boards(n, 0, seed=seed, first_board=first)
        for g in range(3):
            opening = [int(x) for x in m[g, :min(int(l[g]), 2)]]
            moves, visits, winner = _restated_game(first + g, playouts, seed, opening, noise)
            assert [int(x) for x in host.moves[g, :int(host.lens[g])]] == moves, "game %d" % g
            assert int(host.winner[g]) == winner
            for t, v in enumerate(visits):
                assert (host.visits[g, len(opening) + t].numpy().astype(np.uint32) == np.minimum(v, 65535)).all(), "game %d move %d" % (g, t)


def test_match_games_serve_use_rave():
    """("traditional_mcts", {"use_rave": True}) builds a TraditionalRAVEMCTS: the supervisor's first searched ply equals a direct search"""
    n, playouts, first = 6, 40, 11
    sup = ("traditional_mcts", {"use_rave": True, "c_bias": 0.0, "c_puct": 5.0})
    rec, sup_black = selfplay.play_match_games(n, sup, ("traditional_mcts", {"c_puct": 5.0}), playouts=playouts, first_game_id=first,
                                               opening_plies=4, max_moves=6)
    rec = rec.cpu()
    m, l, _ = G.synth_boards(n, 0, seed=G.DEFAULT_SEED, first_board=first)
    opening = [[int(x) for x in m[g, :min(int(l[g]), 4)]] for g in range(n)]
    direct = G.TraditionalRAVEMCTS(n, node_capacity=playouts * 226 + 256, c_puct=5.0)
    direct.set_positions(opening)
    direct.run(playouts)
    v = direct.root_stats()["visits"]
    direct.close()
    checked = 0
    for g in range(n):
        k = len(opening[g])
        if (k % 2 == 0) == bool(sup_black[g]):               # the supervisor moves first after the opening
            assert (rec.visits[g, k].numpy().astype(np.uint32) == v[g]).all(), "game %d" % g
            checked += 1
    assert checked > 0
