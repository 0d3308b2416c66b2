"""K23 without a GPU: gmk_pattern_states_list_host and gmk_pattern_states_finish_host (the host forms of include/gomoku_pattern_states.h)
against the numpy restatement of the rule (tests/pattern_states_reference.py), bit for bit; the four entries at the C boundary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pattern_states_reference as R
from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_pattern_evaluate_states", "gmk_pattern_evaluate_states_host", "gmk_pattern_states_list_host", "gmk_pattern_states_finish_host")
N, F32 = 225, np.float32
SEAMS = (0, 63, 64, 191, 192, 224)                                 # the first and last cells of the four 64-cell ballots


def _check_lists(rows):
    rows = np.asarray(rows, F32).reshape(-1, 6, N)
    moves, lens, status = G.pattern_states_list_host(rows)
    rm, rl, rs = R.lists(rows)
    assert (status == rs).all(), np.flatnonzero(status != rs)
    assert (lens == rl).all(), np.flatnonzero(lens != rl)
    assert moves.tobytes() == rm.tobytes()
    return moves, lens, status


def _random_list(rng, length):
    return [int(c) for c in rng.permutation(N)[:length]]


# ---------------- the decode and the canonical list ----------------
def test_valid_rows_both_sides_every_last_move_form():
    rng = np.random.RandomState(23)
    rows, want = [], []
    for length in (0, 1, 2, 3, 4, 7, 8, 30, 31, 224, 225):
        for _ in range(3):
            ml = _random_list(rng, length)
            for last, last2 in ((True, True), (True, False), (False, False)):
                rows.append(R.planes(ml, last, last2))
                want.append((ml, last, last2))
    moves, lens, status = _check_lists(rows)
    assert not status.any()
    for i, (ml, last, last2) in enumerate(want):
        got = [int(c) for c in moves[i, :lens[i]]]
        assert lens[i] == len(ml)
        # round trip: the same stone sets, the same two last moves, the same side to move
        assert set(got[0::2]) == set(ml[0::2]) and set(got[1::2]) == set(ml[1::2])
        if last and ml:
            assert got[-1] == ml[-1]
        if last2 and len(ml) >= 2:
            assert got[-2] == ml[-2]
        assert not moves[i, lens[i]:].any()
        back = R.planes(got, last, last2)
        assert back.tobytes() == rows[i].tobytes()
        # the rest ascends per colour
        for colour in (0, 1):
            rest = [c for p, c in enumerate(got) if p % 2 == colour and not (last and p == len(got) - 1) and not (last2 and p == len(got) - 2)]
            assert rest == sorted(rest)


def test_seam_cells():
    rows = []
    for a in SEAMS:
        rows.append(R.planes([a]))                                                   # one black stone, white to move
        rows.append(R.planes([a], last=False))
        for b in SEAMS:
            if a != b:
                rows.append(R.planes([a, b]))                                        # one each, black to move
                rows.append(R.planes([a, b], last2=False))
                rows.append(R.planes([112, a, b, 111]))                              # a seam cell that is neither last move
    rows.append(R.planes(list(SEAMS)))
    rows.append(R.planes(list(SEAMS)[::-1], last=False, last2=False))
    moves, lens, status = _check_lists(rows)
    assert not status.any() and lens.max() == 6


def test_values_that_are_set_and_values_that_are_not():
    base = R.planes([112, 113, 0, 224])
    odd = base.copy()
    odd[0, 112], odd[1, 113], odd[3, 224], odd[4, 0] = np.nan, -3.5, 1e-40, np.inf     # all set: NaN, negative, subnormal, infinity
    odd[5, 0] = np.nan                                                                # black to move
    odd[5, 1:] = 0.0                                                                  # the rest of plane 5 is not read
    odd[2] = np.nan                                                                   # plane 2 is not read
    zero = base.copy()
    zero[1, 7] = -0.0                                                                 # -0.0 is not set: still the same position
    moves, lens, status = _check_lists([base, odd, zero])
    assert not status.any() and (moves[0] == moves[1]).all() and (moves[0] == moves[2]).all()


def test_every_invalidity_one_at_a_time():
    ok = R.planes([112, 113, 114, 115])                            # black to move: own = {112, 114}, opp = {113, 115}, last 115, last2 114
    okw = R.planes([112, 113, 114])                                # white to move: own = {113}, opp = {112, 114}
    bad = []

    def variant(base, edit):
        row = base.copy()
        edit(row)
        bad.append(row)

    variant(ok, lambda r: r[0].__setitem__(113, 1.0))              # own and opp share a cell
    variant(ok, lambda r: r[0].__setitem__(113, np.nan))           # ... through a NaN
    variant(ok, lambda r: r[0].__setitem__(7, 1.0))                # black to move, nb == nw + 1
    variant(ok, lambda r: r[1].__setitem__(7, 1.0))                # black to move, nw == nb + 1
    variant(okw, lambda r: r[0].__setitem__(7, 1.0))               # white to move, nb == nw
    variant(okw, lambda r: r[1].__setitem__(7, 1.0))               # white to move, nb == nw + 2
    variant(ok, lambda r: r[3].__setitem__(113, 1.0))              # two cells in plane 3
    variant(ok, lambda r: (r[3].__setitem__(115, 0.0), r[3].__setitem__(114, 1.0)))    # plane 3's cell in own
    variant(ok, lambda r: (r[3].__setitem__(115, 0.0), r[3].__setitem__(7, 1.0)))      # plane 3's cell empty
    variant(ok, lambda r: r[4].__setitem__(112, 1.0))              # two cells in plane 4
    variant(ok, lambda r: (r[4].__setitem__(114, 0.0), r[4].__setitem__(113, 1.0)))    # plane 4's cell in opp
    variant(ok, lambda r: (r[4].__setitem__(114, 0.0), r[4].__setitem__(7, 1.0)))      # plane 4's cell empty
    variant(ok, lambda r: r[3].__setitem__(115, 0.0))              # plane 4 without plane 3
    variant(ok, lambda r: r[3].__setitem__(224, np.nan))           # a NaN makes a second cell of plane 3
    variant(ok, lambda r: r[5].__setitem__(0, 0.0))                # the other side to move with these stones
    variant(ok, lambda r: r[5].__setitem__(0, -0.0))               # ... -0.0 is not set
    bad.append(np.zeros((6, N), F32))                              # the row of a finished K7 leaf: white to move, no stones
    bad.append(np.full((6, N), np.nan, F32))
    moves, lens, status = _check_lists([ok, okw] + bad)
    assert list(status[:2]) == [0, 0] and (status[2:] == G.PATTERN_ILLEGAL).all()
    assert not lens[2:].any() and not moves[2:].any()


def test_random_rows_of_noise_and_near_positions():
    rng = np.random.RandomState(5)
    rows = []
    for i in range(300):
        ml = _random_list(rng, int(rng.randint(0, 226)))
        last = bool(rng.randint(2))
        row = R.planes(ml, last, last and bool(rng.randint(2)))
        if i % 3 == 1:                                             # one entry of a plane that is read flipped
            p, c = (0, 1, 3, 4, 5)[rng.randint(5)], (0 if rng.randint(2) else int(rng.randint(N)))
            row[p, c] = 0.0 if R.is_set(row[p, c]) else (np.nan if rng.randint(2) else 1.0)
        if i % 3 == 2:
            row = (rng.rand(6, N) < 0.02).astype(F32)
        rows.append(row)
    _, _, status = _check_lists(rows)
    assert (status == 0).sum() >= 100 and (status != 0).sum() >= 100


# ---------------- the finish ----------------
def _check_finish(vec, rows):
    vec, rows = np.asarray(vec, F32), np.asarray(rows, F32).reshape(-1, 6, N)
    for name, norm in (("l2", R.NORM_L2), ("sum", R.NORM_SUM)):
        got = G.pattern_states_finish_host(vec, rows, name)
        want = np.stack([R.finish(v, row, norm) for v, row in zip(vec, rows)])
        assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), name
    return G.pattern_states_finish_host(vec, rows, "sum")


def test_finish_random_vectors():
    rng = np.random.RandomState(11)
    rows = [R.planes(_random_list(rng, int(rng.randint(0, 200)))) for _ in range(64)]
    vec = rng.rand(64, N).astype(F32) * (rng.rand(64, N) < 0.3)
    vec[1] *= F32(1e-30)                                           # tiny and huge entries: the quotient is taken in binary64
    vec[2] *= F32(1e30)
    vec[3, :] = 0.0
    vec[3, 224] = 1.0
    got = _check_finish(vec, rows)
    sums = got.astype(np.float64).sum(axis=1)
    assert (np.abs(sums - 1.0) <= 225 * 2.0 ** -24).all()
    assert ((got == 0) == (vec == 0)).all()
    assert G.pattern_states_finish_host(vec, rows, "l2").tobytes() == vec.tobytes()


def test_finish_zero_vector_uniform_fallback_and_full_board():
    rng = np.random.RandomState(12)
    lists_ = [[], [112], _random_list(rng, 100), _random_list(rng, 224), _random_list(rng, 225)]
    rows = [R.planes(ml) for ml in lists_]
    got = _check_finish(np.zeros((5, N), F32), rows)
    for ml, p in zip(lists_, got):
        empty = np.ones(N, bool)
        empty[ml] = False
        assert not p[~empty].any()
        if empty.any():
            assert (p[empty] == F32(1.0 / float(empty.sum()))).all()
    assert not got[4].any()                                        # a full board has no cell to offer
    assert got[3].sum() == 1.0                                     # one empty cell


def test_finish_rows_that_are_no_position_get_zeros():
    vec = np.ones((2, N), F32)
    rows = [np.zeros((6, N), F32), np.full((6, N), np.nan, F32)]
    assert not _check_finish(vec, rows).any()


# ---------------- the C boundary ----------------
def test_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K23" in text and "GMK_PATTERN_NORM_SUM" in text
    assert os.path.exists(os.path.join(ROOT, "include", "gomoku_pattern_states.h"))
    assert (G.PATTERN_NORM_L2, G.PATTERN_NORM_SUM) == (0, 1)
    from gomokuai_amd import network
    assert callable(G.pattern_evaluate_states) and callable(G.pattern_evaluate_states_host) and callable(network.PatternEvaluator)


def test_bad_arguments_are_refused_before_any_device_is_asked_for():
    L = G.load()
    ERR_ARG = -3
    s, v, p = np.zeros((1, 6, N), F32), np.zeros(1, F32), np.zeros((1, N), F32)
    st, mv, ln = np.zeros(1, np.int32), np.zeros((1, N), np.uint8), np.zeros(1, np.int32)
    sp, vp, pp = s.ctypes.data, v.ctypes.data, p.ctypes.data
    for args in ((None, 1, 1, 1, vp, pp, None), (sp, 1, 1, 1, None, pp, None), (sp, 1, 1, 1, vp, None, None), (sp, -1, 1, 1, vp, pp, None),
                 (sp, 1, 1, 2, vp, pp, None), (sp, 1, 1, -1, vp, pp, None), (sp, 1, 2, 1, vp, pp, None), (sp, 1, -1, 0, vp, pp, None)):
        assert L.gmk_pattern_evaluate_states(*args, None) == ERR_ARG, args
        assert b"gmk_pattern_evaluate_states" in L.gmk_last_error()
        assert L.gmk_pattern_evaluate_states_host(*args) == ERR_ARG, args
    assert L.gmk_pattern_states_list_host(None, 1, mv.ctypes.data, ln.ctypes.data, st.ctypes.data) == ERR_ARG
    assert L.gmk_pattern_states_list_host(sp, 1, None, ln.ctypes.data, st.ctypes.data) == ERR_ARG
    assert L.gmk_pattern_states_list_host(sp, 1, mv.ctypes.data, None, st.ctypes.data) == ERR_ARG
    assert L.gmk_pattern_states_list_host(sp, 1, mv.ctypes.data, ln.ctypes.data, None) == ERR_ARG
    assert L.gmk_pattern_states_list_host(sp, -1, mv.ctypes.data, ln.ctypes.data, st.ctypes.data) == ERR_ARG
    assert L.gmk_pattern_states_list_host(None, 0, None, None, None) == 0
    assert L.gmk_pattern_states_finish_host(None, sp, 1, 1, pp) == ERR_ARG
    assert L.gmk_pattern_states_finish_host(pp, None, 1, 1, pp) == ERR_ARG
    assert L.gmk_pattern_states_finish_host(pp, sp, 1, 1, None) == ERR_ARG
    assert L.gmk_pattern_states_finish_host(pp, sp, 1, 2, pp) == ERR_ARG
    assert L.gmk_pattern_states_finish_host(pp, sp, -1, 1, pp) == ERR_ARG
    assert L.gmk_pattern_states_finish_host(None, None, 0, 1, None) == 0
    with pytest.raises(ValueError):
        G.pattern_states_finish_host(p, s, "softmax")
    from gomokuai_amd.network import PatternEvaluator
    with pytest.raises(ValueError):
        PatternEvaluator(norm="softmax")
    for mode in ("all", "random", "ALL", 1):
        with pytest.raises(ValueError, match="not a learned function"):
            PatternEvaluator().symmetric(mode)
    ev = PatternEvaluator()
    assert ev.symmetric(None) is ev and ev.symmetric("none") is ev


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    s, v, p = np.zeros((4, 6, N), F32), np.zeros(4, F32), np.zeros((4, N), F32)
    assert L.gmk_pattern_evaluate_states(s.ctypes.data, 4, 1, 1, v.ctypes.data, p.ctypes.data, None, None) == -4          # GMK_ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_pattern_evaluate_states_host(s.ctypes.data, 4, 1, 1, v.ctypes.data, p.ctypes.data, None) == -4
    assert b"no CPU fallback" in L.gmk_last_error()
    with pytest.raises(G.GmkError):
        G.pattern_evaluate_states_host(s)
    # ... while the two forms that need no GPU work here
    assert (G.pattern_states_list_host(s)[2] == G.PATTERN_ILLEGAL).all()
