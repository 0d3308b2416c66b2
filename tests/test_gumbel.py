"""K21 on the CPU: the header's statements behind the C-ABI (gmk_gumbel_*_host, which need no GPU) against tests/gumbel_reference.py, an
independent restatement in Python floats, bit for bit; the draws against libm; the schedule's and the row's invariants; and Gumbel-max as the
distribution it claims to be.  The GPU side of the same header is held to the same restatement by tests/test_az_gumbel_gpu.py."""
import math

import numpy as np
import pytest

import gumbel_reference as R
from gomokuai_amd import lib as G

N = 225
SEED = 0x0123456789ABCDEF
U = 2.0 ** -53                                                   # the unit roundoff of binary64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _setup(prior, visits, stones, game_id, m, seed=SEED):
    return G.gumbel_setup_host(prior[None], visits[None], [stones], [game_id], m, seed)


# ---------------- the draws ----------------
GAME_IDS, STONES = (0, 1, 77777, 0xFFFFFFFF), (0, 9, 224)


def test_draws_match_the_restatement_bit_for_bit():
    prior = np.zeros((len(GAME_IDS) * len(STONES), N), np.float32)
    ids = [g for g in GAME_IDS for _ in STONES]
    stones = [s for _ in GAME_IDS for s in STONES]
    got = G.gumbel_setup_host(prior, np.zeros_like(prior, dtype=np.uint32), stones, ids, 1, SEED)["draws"]
    for row, (g, s) in enumerate(zip(ids, stones)):
        want = np.array([R.draw(g, s, c, SEED) for c in range(N)])
        np.testing.assert_array_equal(_bits(got[row]), _bits(want), "game %d, %d stones" % (g, s))


def test_draws_follow_libm():
    """g = -log(-log u) through gmk_noise_log twice, against libm.  The bound, from the header's statement of its logarithm: for x = m 2^e it
    returns e ln2 + 2 s p with p the odd atanh series up to s^23 (truncation < 2e-19 relative, far below one rounding).  The roundings: m + 1,
    the division, s2, about two units in the Horner chain, s p, and the final sum, i.e. at most 6 units of |2 s p| <= 0.35, plus two units of
    |e| ln 2 (the product and the constant) and one of the result: an absolute error of at most 6 U max(1, |log x|).
    a = -log u: where a is small (u near 1) e is 0 and the error is relative, 6 U; elsewhere |log u| >= 0.34 and it is at most 6 U / 0.34 = 18 U
    relative.  So log(a) is shifted by at most 18 U, and the outer logarithm adds 6 U max(1, |g|).  libm's own two logarithms are within one
    unit each: U more on the shift and U |g| on the result.  Together |g - g_libm| <= (19 + 7 max(1, |g|)) U, taken as (25 + 8 max(1, |g|)) U."""
    worst = 0.0
    for g in GAME_IDS:
        for s in STONES:
            draws = _setup(np.zeros(N, np.float32), np.zeros(N, np.uint32), s, g, 1)["draws"][0]
            for c in range(N):
                libm = -math.log(-math.log(R.uniform_of(g, s, c, SEED)))
                err = abs(draws[c] - libm) / ((25.0 + 8.0 * max(1.0, abs(libm))) * U)
                worst = max(worst, err)
    print("largest error / bound: %.3f" % worst)
    assert worst <= 1.0


# ---------------- the schedule ----------------
SCHEDULES = [(1, 5), (2, 7), (3, 16), (16, 32), (16, 200), (225, 16), (5, 1), (225, 4096)]


@pytest.mark.parametrize("m_eff,n", SCHEDULES)
def test_schedule(m_eff, n):
    seq = G.gumbel_sequence_host(m_eff, n).tolist()              # (the entry also checks the kernels' walk against the sequence it built)
    assert seq == R.sequence(m_eff, n)
    assert len(seq) == n and seq[0] == 0 and all(0 <= b - a <= 1 for a, b in zip(seq, seq[1:]))      # n long, non-decreasing, no count left out
    if m_eff == 1:
        assert seq == list(range(n))
        return
    runs = [seq.count(c) for c in range(seq[-1] + 1)]
    assert runs[0] == min(m_eff, n)                              # every considered child once, first
    for c, (a, b) in enumerate(zip(runs, runs[1:])):
        assert b <= a, c                                         # halving: later counts go to fewer children
    assert all(r >= 2 for r in runs[:-1])                        # whole runs except the last, which n cuts


def test_schedule_refuses_bad_arguments():
    L = G.load()
    out = np.zeros(8, np.uint32)
    for m_eff, n in ((0, 4), (226, 4), (4, 0), (4, 4097)):
        assert L.gmk_gumbel_sequence_host(m_eff, n, out.ctypes.data) == -3
    assert L.gmk_gumbel_sequence_host(4, 4, None) == -3


# ---------------- set-up, pick, move and row on hand-built roots ----------------
def _root(rng, n_children, kept):
    """A root by cell: n_children random cells with float32 priors; kept: statistics of a kept subtree (visits and values) or none"""
    prior, visits, value = np.zeros(N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.float32)
    cells = np.sort(rng.choice(N, n_children, replace=False))
    prior[cells] = (rng.randint(1, 1022, n_children).astype(np.float32) / np.float32(1024.0)) ** (3 if kept else 1)
    if kept:
        visits[cells] = rng.randint(0, 40, n_children)
        value[cells] = np.where(visits[cells] > 0, rng.uniform(-1, 1, n_children), 0.0).astype(np.float32)
    return prior, visits, value


def _same_setup(got, ref, prior):
    children = [c for c in range(N) if prior[c] != 0]
    score = np.zeros(N)
    score[children] = [ref.score[c] for c in children]
    np.testing.assert_array_equal(_bits(got["score"][0]), _bits(score))
    base = np.zeros(N, np.uint32)
    base[children] = [ref.base[c] for c in children]
    np.testing.assert_array_equal(got["base"][0][children], base[children])
    considered = np.zeros(N, np.uint8)
    considered[ref.considered] = 1
    np.testing.assert_array_equal(got["considered"][0], considered)
    assert got["m_eff"][0] == ref.m_eff


def _ask(prior, visits, value, root_value, setup, ref, n, c_visit, c_scale):
    """pick, move and row of the host forms against the restatement; returns the pick"""
    rv = np.array([root_value], np.float32)
    pick = int(G.gumbel_pick_host(prior[None], visits[None], value[None], rv, setup, n, c_visit, c_scale)[0])
    assert pick == ref.pick(visits, value, root_value, n)
    assert int(G.gumbel_move_host(prior[None], visits[None], value[None], rv, setup, c_visit, c_scale)[0]) == ref.move(visits, value, root_value)
    got = G.gumbel_row_host(prior[None], visits[None], value[None], rv, c_visit, c_scale)[0]
    np.testing.assert_array_equal(got, R.row(prior, visits, value, root_value, c_visit, c_scale))
    _row_invariants(got, prior)
    return pick


def _row_invariants(row, prior):
    children = prior != 0
    assert not row[~children].any()                              # no entry where there is no child
    if children.any():
        assert abs(int(row.astype(np.int64).sum()) - 65535) <= 225 and int(row.max()) >= 291        # 225 roundings; the largest e_c is 1 and Z <= 225


@pytest.mark.parametrize("n_children,m,n,kept", [(1, 4, 6, False), (5, 16, 8, False), (40, 4, 16, True), (225, 16, 32, False), (225, 225, 8, True), (60, 3, 50, True)])
def test_rule_on_random_roots(n_children, m, n, kept):
    """Set-up on a fresh or kept root, then n + 6 playouts whose root steps follow the pick (so t runs past n), each with pick, move and row"""
    rng = np.random.RandomState(1000 * n_children + m)
    prior, visits, value = _root(rng, n_children, kept)
    c_visit, c_scale, game_id, stones = 50.0, 1.0, 4242 + n, 7
    setup = _setup(prior, visits, stones, game_id, m)
    ref = R.Root(prior, visits, m, game_id, stones, SEED, c_visit, c_scale)
    _same_setup(setup, ref, prior)
    root_value = np.float32(0.125)
    for _ in range(n + 6):
        pick = _ask(prior, visits, value, root_value, setup, ref, n, c_visit, c_scale)
        assert setup["considered"][0][pick] == 1
        visits[pick] += 1
        value[pick] = np.float32(rng.uniform(-1, 1))
        root_value = np.float32(rng.uniform(-1, 1))


def test_all_visits_zero_and_other_constants():
    rng = np.random.RandomState(5)
    prior, visits, value = _root(rng, 30, False)
    for c_visit, c_scale in ((50.0, 1.0), (0.0, 0.0), (5.0, 0.1)):
        setup = _setup(prior, visits, 0, 3, 8)
        ref = R.Root(prior, visits, 8, 3, 0, SEED, c_visit, c_scale)
        _ask(prior, visits, value, np.float32(-0.5), setup, ref, 16, c_visit, c_scale)


def test_ties_go_to_the_lower_cell():
    """Equal base scores cannot be drawn to order, so they are written into the set-up by hand: equal keys in pick and move"""
    prior, visits, value = np.zeros(N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.float32)
    cells = [200, 17, 90, 18]
    prior[cells] = 0.25
    setup = _setup(prior, visits, 0, 1, 4)
    ref = R.Root(prior, visits, 4, 1, 0, SEED)
    for c in cells:
        setup["score"][0][c] = 0.5
        ref.score[c] = 0.5
    assert _ask(prior, visits, value, np.float32(0.0), setup, ref, 8, 50.0, 1.0) == 17
    visits[17] = 1                                               # value 0 = the stand-in of the others: the keys stay equal
    assert _ask(prior, visits, value, np.float32(0.0), setup, ref, 8, 50.0, 1.0) == 18


def test_a_count_without_a_match_and_visits_outside_the_considered_set():
    rng = np.random.RandomState(11)
    prior, visits, value = _root(rng, 20, True)
    setup = _setup(prior, visits, 12, 9, 4)
    ref = R.Root(prior, visits, 4, 9, 12, SEED)
    considered = np.flatnonzero(setup["considered"][0])
    others = [c for c in np.flatnonzero(prior) if c not in considered]
    visits[considered] += np.array([3, 5, 3, 4], np.uint32)      # t = 15 of 16: seq[15] = 5 is held by one child; then t = 16
    assert _ask(prior, visits, value, np.float32(0.3), setup, ref, 16, 50.0, 1.0) == considered[1]
    visits[others[0]] += 2                                       # t = 17 >= n: the smallest count
    pick = _ask(prior, visits, value, np.float32(0.3), setup, ref, 16, 50.0, 1.0)
    assert pick in (considered[0], considered[2])
    visits[others[0]] -= 2
    visits[considered] = setup["base"][0][considered] + np.array([3, 3, 3, 3], np.uint32)      # t = 12, seq[12] = 4 for m_eff = 4, n = 16: nobody has it
    assert G.gumbel_sequence_host(4, 16)[12] == 4
    pick = _ask(prior, visits, value, np.float32(0.3), setup, ref, 16, 50.0, 1.0)
    assert pick in considered


def test_a_root_without_children():
    z = np.zeros(N, np.float32)
    setup = _setup(z, np.zeros(N, np.uint32), 3, 1, 4)
    assert setup["m_eff"][0] == 0 and not setup["considered"].any()
    rv = np.zeros(1, np.float32)
    assert G.gumbel_pick_host(z[None], np.zeros((1, N), np.uint32), z[None], rv, setup, 8)[0] == -1
    assert G.gumbel_move_host(z[None], np.zeros((1, N), np.uint32), z[None], rv, setup)[0] == -1
    assert not G.gumbel_row_host(z[None], np.zeros((1, N), np.uint32), z[None], rv).any()


def test_saturated_rows():
    """One child far ahead: the row is one-hot 65535; equal children: uniform"""
    prior, visits, value = np.zeros(N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.float32)
    prior[:] = 1.0 / 225.0
    row = G.gumbel_row_host(prior[None], visits[None], value[None], np.zeros(1, np.float32))[0]
    assert (row == 291).all()
    visits[7], value[7] = 30, 1.0
    value[8], visits[8] = -1.0, 30
    row = G.gumbel_row_host(prior[None], visits[None], value[None], np.zeros(1, np.float32))[0]
    assert row[7] == 65535 and row.sum() == 65535
    np.testing.assert_array_equal(row, R.row(prior, visits, value, np.float32(0.0)))


# ---------------- Gumbel-max is a sample from the prior ----------------
def test_gumbel_max_samples_the_prior():
    """m = 1 and equal values: the move is argmax(g_c + log p_c), which is distributed as p.  20 000 game ids on a five-child prior, chi-square with 4
    degrees of freedom; the threshold 23.51 is its 1 - 1e-4 quantile, so a correct sampler fails with probability 1e-4 -- once, since the draws
    are a fixed function of the seed."""
    games = 20000
    p = np.array([0.1, 0.15, 0.2, 0.25, 0.3], np.float32)
    cells = [3, 50, 112, 113, 224]
    prior = np.zeros((games, N), np.float32)
    prior[:, cells] = p
    zeros = np.zeros((games, N), np.uint32)
    setup = G.gumbel_setup_host(prior, zeros, np.full(games, 5, np.int32), np.arange(games, dtype=np.uint32) + 1000, 1, SEED)
    assert (setup["m_eff"] == 1).all() and (setup["considered"].sum(axis=1) == 1).all()
    moves = G.gumbel_move_host(prior, zeros, np.zeros((games, N), np.float32), np.zeros(games, np.float32), setup)
    counts = np.array([(moves == c).sum() for c in cells], np.float64)
    assert counts.sum() == games
    expected = games * p.astype(np.float64) / float(p.astype(np.float64).sum())
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print("chi-square = %.2f" % chi2)
    assert chi2 < 23.51
