"""TraditionalPolicy(use_rave) restated in Python (tests/trad_rave_reference.py) earns its trust against the oracle's go_trad with
use_rave=False -- fresh roots on one persistent evaluator, then a kept tree with stepForward and counter-sampler noise -- before the
device's gmk_trad_run_rave is held to it with use_rave=True.  The C entry point itself is checked without a device."""
import ctypes as C

import numpy as np

from trad_rave_reference import TradRAVEReference

SEED = 0x1234ABCD5678EF01


def _positions(n, seed=5):
    rng = np.random.RandomState(seed)
    out = []
    for g in range(n):
        k = (g * 7) % 41
        cells = rng.permutation(225)[:k] if g % 3 else 96 + rng.permutation(33)[:min(k, 20)]     # some crowded around the centre
        out.append([int(c) for c in cells])
    return out


def _same(orc, ref, where):
    v, q, p, best = orc.root_children()
    rv, rq, rp, _, _, rbest = ref.root_children()
    np.testing.assert_array_equal(v, rv, where)
    np.testing.assert_array_equal(q.view(np.uint32), rq.view(np.uint32), where)
    np.testing.assert_array_equal(p.view(np.uint32), rp.view(np.uint32), where)
    assert best == rbest, where
    assert orc.root_visits == ref.root_visits, where
    assert np.float32(orc.root_value).view(np.uint32) == ref.root_value.view(np.uint32), where
    assert orc.evaluator_updates == ref.evaluator_updates, where


def test_fresh_roots_equal_go_trad(oracle):
    orc, ref = oracle.TraditionalMCTS(5.0), TradRAVEReference(5.0, use_rave=False)
    for i, pos in enumerate(_positions(12)):           # one evaluator for all of them, as the policy object keeps it
        orc.search(pos, 200)
        ref.search(pos, 200)
        _same(orc, ref, "position %d" % i)
        assert orc.n_nodes == ref.n_nodes


def test_kept_tree_with_noise_equals_go_trad(oracle):
    for g, pos in enumerate(_positions(4, seed=9)):
        orc, ref = oracle.TraditionalMCTS(2.5), TradRAVEReference(2.5, use_rave=False)
        orc.set_noise(0.05, 0.25, SEED, game_id=g, sampler=1)
        ref.set_noise(0.05, 0.25, SEED, game_id=g)
        moves = list(pos)
        for ply in range(4):
            orc.run(moves, 150)
            ref.run(moves, 150)
            _same(orc, ref, "game %d ply %d" % (g, ply))
            assert orc.n_nodes == ref.n_nodes
            mv = orc.step_forward()
            assert ref.step_forward() == mv
            moves.append(mv)


def test_rave_invariants():
    ref = TradRAVEReference(5.0, use_rave=True)
    plain = TradRAVEReference(5.0, use_rave=False)
    differs = False
    for pos in _positions(6, seed=11):
        ref.search(pos, 200)
        plain.search(pos, 200)
        v, q, _, av, aq, best = ref.root_children()
        assert (av >= v).all()                         # a visited child's own cell is on every leaf board below it
        assert (np.abs(aq) <= 1).all() and ref.root_visits == 200
        differs |= (v != plain.root_children()[0]).any()
    assert differs                                     # the weighting reaches the choice of children


def test_run_rave_is_exported_and_checks_its_handle():
    from gomokuai_amd import lib as G
    L = G.load()
    assert "gmk_trad_run_rave" in G.EXPORTS
    assert L.gmk_trad_run_rave(None, 10, 5.0, None) == -3          # GMK_ERR_ARG, no device needed
    assert L.gmk_trad_selfplay_run(None, 2, 1, 0, 10, 5.0, 0, 0, 0.0, 0.0, None, 0, None, None, None, None, None, 0, 0, None, None, None) == -3
    assert L.gmk_trad_selfplay_run(None, 3, 1, 0, 10, 5.0, 0, 0, 0.0, 0.0, None, 0, None, C.c_void_p(1), None, C.c_void_p(1), C.c_void_p(1), 0, 0, None, None, None) == -3         # policy 3 does not exist
