""""K22" at the C-ABI, without a device: the two entries exist and are declared, their argument errors come back before anything touches a GPU,
and the pick of GMK_PVNET_SYM_RANDOM (gmk_pvnet_sym_pick_host, include/gomoku_symmetry.h) is the one tests/pvnet_sym_reference.py restates:
a function of a row's content and the seed only, and a fair eight-way draw."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pvnet_sym_reference as S
from gomokuai_amd import lib as G

_NEW = ("gmk_pvnet_evaluate_sym", "gmk_pvnet_sym_pick_host")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = os.path.join(_ROOT, "include", "gomoku_hip.h")
ERR_ARG = -3
SEED, OTHER_SEED = 0x9E3779B97F4A7C15, 20260117


@pytest.fixture(scope="module")
def boards():
    return S.positions(4096, 22)


def test_exports_exist_and_are_declared():
    lib = G.load()
    text = open(_HEADER).read()
    for name in _NEW:
        assert name in G.EXPORTS
        assert getattr(lib, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    for name, value in (("NONE", 0), ("ALL", 1), ("RANDOM", 2)):
        assert re.search(r"GMK_PVNET_SYM_%s\s*=\s*%d\b" % (name, value), text)
    assert G.PVNET_SYMMETRIES == {"none": 0, "all": 1, "random": 2}
    assert "K22" in text
    rule = open(os.path.join(_ROOT, "include", "gomoku_symmetry.h")).read()
    assert re.search(r"GMK_SYM_TAG\s+0x%xu" % S.SYM_TAG, rule)


def test_argument_errors_without_a_device():
    lib = G.load()
    x, v, p = np.zeros((2, 6, 225), np.float32), np.full(2, 7.0, np.float32), np.full((2, 225), 7.0, np.float32)
    fake = C.c_void_p(8)                                         # never dereferenced: every call below is refused on its arguments
    for mode in (0, 1, 2):
        assert lib.gmk_pvnet_evaluate_sym(None, x.ctypes.data, 2, mode, SEED, v.ctypes.data, p.ctypes.data, None) == ERR_ARG
        assert b"gmk_pvnet_evaluate_sym" in lib.gmk_last_error()
        assert lib.gmk_pvnet_evaluate_sym(fake, None, 2, mode, SEED, v.ctypes.data, p.ctypes.data, None) == ERR_ARG
        assert lib.gmk_pvnet_evaluate_sym(fake, x.ctypes.data, 2, mode, SEED, None, p.ctypes.data, None) == ERR_ARG
        assert lib.gmk_pvnet_evaluate_sym(fake, x.ctypes.data, 2, mode, SEED, v.ctypes.data, None, None) == ERR_ARG
        assert lib.gmk_pvnet_evaluate_sym(fake, x.ctypes.data, -1, mode, SEED, v.ctypes.data, p.ctypes.data, None) == ERR_ARG
    for mode in (-1, 3, 8):
        assert lib.gmk_pvnet_evaluate_sym(fake, x.ctypes.data, 2, mode, SEED, v.ctypes.data, p.ctypes.data, None) == ERR_ARG
    assert (v == 7.0).all() and (p == 7.0).all() and not x.any()
    sym = np.full(2, -5, np.int32)
    assert lib.gmk_pvnet_sym_pick_host(None, 2, SEED, sym.ctypes.data) == ERR_ARG
    assert b"gmk_pvnet_sym_pick_host" in lib.gmk_last_error()
    assert lib.gmk_pvnet_sym_pick_host(x.ctypes.data, 2, SEED, None) == ERR_ARG
    assert lib.gmk_pvnet_sym_pick_host(x.ctypes.data, -1, SEED, sym.ctypes.data) == ERR_ARG
    assert (sym == -5).all()
    assert lib.gmk_pvnet_sym_pick_host(None, 0, SEED, None) == 0
    assert G.pvnet_sym_pick_host(np.zeros((0, 6, 15, 15), np.float32), SEED).shape == (0,)


def test_symmetric_rejects_an_unknown_mode_before_the_device():
    """symmetric(mode) is checked before gmk_init: a typo is a ValueError on any machine, and so is symmetry= of the loops"""
    from gomokuai_amd import selfplay
    from gomokuai_amd.network import FusedPolicyValueNetwork, SymmetricNetwork
    from gomokuai_amd.training import EvaluationSchedule
    fused = FusedPolicyValueNetwork.__new__(FusedPolicyValueNetwork)      # no handle: nothing here may need one
    fused.h = None
    for mode in ("mean", "ALL", 1, None):
        with pytest.raises(ValueError):
            fused.symmetric(mode)
    net = fused.symmetric("random", seed=5)
    assert isinstance(net, SymmetricNetwork) and net.mode == "random" and net.seed == 5 and net.fused is fused
    assert fused.symmetric("all").seed == G.DEFAULT_SEED
    with pytest.raises(ValueError):
        selfplay.play_network_games(2, fused, 4, symmetry="mean")
    with pytest.raises(ValueError):
        selfplay.play_network_games(2, lambda states: None, 4, symmetry="all")          # a network without symmetric()
    with pytest.raises(ValueError):
        selfplay.play_evaluation_games(2, lambda states: None, ("traditional_mcts", {}), symmetry="random")
    with pytest.raises(ValueError):
        EvaluationSchedule(symmetry="mean")
    assert EvaluationSchedule(symmetry="all").symmetry == "all" and EvaluationSchedule().symmetry is None


def test_the_schedule_forwards_symmetry(monkeypatch):
    from gomokuai_amd import selfplay
    from gomokuai_amd.training import EvaluationSchedule, TrainingLoop
    seen = {}

    def fake(n_games, network, opponent, playouts=400, **options):
        seen.update(options)
        return None, np.ones(n_games, bool), np.ones(n_games)
    monkeypatch.setattr(selfplay, "play_evaluation_games", fake)
    loop = TrainingLoop.__new__(TrainingLoop)
    loop.schedule, loop.eval_options, loop.eval_playouts, loop.total_steps = EvaluationSchedule(eval_rounds=2, symmetry="all"), {}, 8, 0
    loop.on_best = loop.on_checkpoint = None
    loop.history = []
    loop.evaluate(None)
    assert seen == {"symmetry": "all"}
    loop.eval_options = {"symmetry": "random"}                   # eval_options may name its own
    loop.evaluate(None)
    assert seen == {"symmetry": "random"}


def test_the_reference_transforms_are_the_augmentation():
    """transform / back against tests/helpers.py's statement of the reference's augmentation order, and against each other"""
    from helpers import symmetries
    board = S.positions(1, 7)
    pi = np.arange(225, dtype=np.float32)
    for a, (planes, row) in enumerate(symmetries(board[0], pi)):
        np.testing.assert_array_equal(S.transform(board, a)[0], planes)
        np.testing.assert_array_equal(S.transform(pi.reshape(1, 15, 15), a).reshape(-1), row)
        np.testing.assert_array_equal(S.back(row[None], a)[0], pi)
    assert len({S.transform(board, a).tobytes() for a in range(8)}) == 8          # an asymmetric position: eight different inputs


@pytest.mark.parametrize("seed", [SEED, OTHER_SEED, 0])
def test_pick_equals_the_restatement(boards, seed):
    got = G.pvnet_sym_pick_host(boards, seed)
    assert got.dtype == np.int32 and got.tolist() == S.pick(boards, seed).tolist()


def test_pick_depends_on_content_and_seed_only(boards):
    want = G.pvnet_sym_pick_host(boards, SEED)
    order = np.random.RandomState(3).permutation(len(boards))
    assert G.pvnet_sym_pick_host(boards[order], SEED).tolist() == want[order].tolist()
    for g in (0, 1, 77, 4095):
        assert G.pvnet_sym_pick_host(boards[g:g + 1], SEED).tolist() == [want[g]]
    other = G.pvnet_sym_pick_host(boards, OTHER_SEED)
    assert 0.8 < (other != want).mean() < 0.95                   # two independent eight-way draws differ in 7 of 8 rows
    # the digest reads the stones and the colour: the last-move planes change nothing, one more stone or the other colour does
    b = boards[:64].copy()
    b[:, 3:5] = 0
    assert G.pvnet_sym_pick_host(b, SEED).tolist() == want[:64].tolist()
    flat = boards[:64].copy().reshape(64, 6, 225)
    empty = flat[:, 2].argmax(axis=1)
    flat[np.arange(64), 0, empty] = 1
    stone = G.pvnet_sym_pick_host(flat, SEED)
    colour = boards[:64].copy()
    colour[:, 5] = 1 - colour[:, 5]
    assert (stone != want[:64]).sum() > 40 and (G.pvnet_sym_pick_host(colour, SEED) != want[:64]).sum() > 40
    assert S.digest(boards).dtype == np.uint64 and len(set(S.digest(boards).tolist())) == len(boards)


@pytest.mark.parametrize("seed", [SEED, OTHER_SEED])
def test_pick_is_a_fair_eight_way_draw(boards, seed):
    """4 096 draws: every symmetry 512 times give or take 5 sigma = 5 sqrt(4096 * 1/8 * 7/8) = 106"""
    counts = np.bincount(G.pvnet_sym_pick_host(boards, seed), minlength=8)
    assert len(counts) == 8 and (abs(counts - 512) <= 106).all(), counts.tolist()
