"""The device form of Default::AddNoise with the counter-based sampler (noise_device.h: mix_root_priors, gamma_draw, tree_sum) against its serial
statement (include/gomoku_noise.h: gmk_noise_mix225 and gmk_noise_gamma, through gcc: the oracle's go_noise_mix225 / go_noise_gamma, which
tests/test_noise.py pins), through the diagnostic entry gmk_noise_mix_rows: rows of priors by cell that the test supplies, one wavefront per row.

Every comparison is on the uint32 views of the floats; there is no tolerance anywhere.  The rows are chosen for the lane layout (lane l owns the cells
l, l + 64, l + 128, l + 192; the norm is a tree inside rows of 16 lanes, then the four row leaders), the parameters for the sampler's branches
(alpha >= 1: no boost; small alpha: most draws flushed to 0; a zero vector of draws: normalized() leaves it), the keys for the 32-bit edges of
the game id and of the two seed halves."""
import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

N = 225
ONE = np.float32(1)
ALPHAS = [0.01, 0.03, 0.05, 0.3, float(np.nextafter(ONE, np.float32(0))), 1.0, 2.5, 50.0]
EPSILONS = [0.0, 0.25, 0.75, 1.0]
GAME_IDS = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
STONES = [0, 1, 224]
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345, 2 ** 64 - 1]
TINY_SUBNORMAL, TINY_NORMAL = np.float32(2.0 ** -149), np.float32(2.0 ** -126)


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the rows ----------------------------------------------------------------
def _row(cells, priors):
    r = np.zeros(N, np.float32)
    r[np.asarray(cells, dtype=np.int64)] = priors
    return r


def _random_set(rng, size):
    """`size` children with random priors, normalised in float32; about one in eight (none below five children) set to exact 0 afterwards"""
    cells = np.sort(rng.choice(N, size, replace=False))
    p = rng.uniform(0.01, 1.0, size).astype(np.float32)
    p = p / p.sum(dtype=np.float32)
    if size >= 5:
        p[rng.choice(size, max(1, size // 8), replace=False)] = 0.0
    return _row(cells, p)


def full_rows():
    rng = np.random.RandomState(7)
    return [("uniform 225", np.full(N, ONE / np.float32(N), np.float32)), ("random 225", rng.uniform(1e-4, 1.0, N).astype(np.float32))]


def random_rows():
    rng = np.random.RandomState(8)
    return [("random set of %d" % k, _random_set(rng, k)) for k in (2, 3, 5, 17, 64, 65, 140, 224)]


def layout_rows():
    """child sets that sit on the seams of the lane layout"""
    out = [("one child at %d" % c, _row([c], ONE)) for c in (0, 15, 16, 47, 48, 63, 64, 127, 128, 191, 192, 224)]
    out += [("children %d and %d" % ab, _row(ab, np.float32(0.5))) for ab in ((63, 64), (127, 128), (191, 192), (15, 16))]
    out.append(("cells 16..31: one DPP row of register 0", _row(range(16, 32), ONE / np.float32(16))))
    out.append(("cells 192..224: register 3 alone", _row(range(192, 225), ONE / np.float32(33))))
    out.append(("the cells of lane 63", _row([63, 127, 191], ONE / np.float32(3))))
    return out


def tiny_rows():
    """the smallest subnormal and the smallest normal float as priors, beside ordinary ones and on their own"""
    mixed = _row([3, 64, 100, 130, 200, 224], [0.25, TINY_SUBNORMAL, 0.5, TINY_NORMAL, 0.25, TINY_SUBNORMAL])
    return [("tiny priors beside ordinary ones", mixed), ("the smallest subnormal alone", _row([77], TINY_SUBNORMAL)), ("the smallest normal alone", _row([191], TINY_NORMAL)),
            ("both tiny priors", _row([63, 192], [TINY_SUBNORMAL, TINY_NORMAL]))]


def every_family():
    return full_rows() + random_rows() + layout_rows() + tiny_rows()


def stack(named):
    return [name for name, _ in named], np.stack([r for _, r in named]).astype(np.float32)


# ---------------------------------------------------------------- the two sides ----------------------------------------------------------------
def serial(O, rows, ids, stones, alpha, epsilon, seed):
    """(mixed, draws) by the serial statement: go_noise_mix225 on a copy of every row, go_noise_gamma on the entries whose scaled prior is not 0"""
    L = O.lib()
    mixed = np.ascontiguousarray(rows, dtype=np.float32).copy()
    draws = np.zeros_like(mixed)
    scale = ONE - np.float32(epsilon)                            # the header's `1 - epsilon`: a float32 subtraction
    for i in range(len(mixed)):
        row = mixed[i]
        takes = np.nonzero(row * scale != 0)[0]
        L.go_noise_mix225(row.ctypes.data, alpha, epsilon, int(ids[i]), int(stones[i]), int(seed))
        for c in takes:
            draws[i, c] = L.go_noise_gamma(alpha, int(ids[i]), int(stones[i]), int(c), int(seed))
    return mixed, draws


def u32(values):
    import torch
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def device(rows, ids, stones, alpha, epsilon, seed, want_draws=True):
    import torch
    p = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32).copy()).cuda()
    d = torch.full(p.shape, 123.0, dtype=torch.float32, device="cuda") if want_draws else None      # (every entry of d_draws is written)
    G.noise_mix_rows(p, u32(ids), u32(stones), alpha, epsilon, seed, draws=d)
    torch.cuda.synchronize()
    return p.cpu().numpy(), (d.cpu().numpy() if want_draws else None)


def hold(O, names, rows, ids, stones, alpha, epsilon, seed):
    """the device's mixed priors and draws == the serial statement's, bit for bit; -> the serial statement's, for the caller's own checks"""
    ref_mixed, ref_draws = serial(O, rows, ids, stones, alpha, epsilon, seed)
    got_mixed, got_draws = device(rows, ids, stones, alpha, epsilon, seed)
    for i, name in enumerate(names):
        where = "%s (row %d): alpha %r epsilon %r game %d stones %d seed %#x" % (name, i, alpha, epsilon, ids[i], stones[i], seed)
        np.testing.assert_array_equal(bits(got_draws[i]), bits(ref_draws[i]), "draws of " + where)
        np.testing.assert_array_equal(bits(got_mixed[i]), bits(ref_mixed[i]), "mixed priors of " + where)
    return ref_mixed, ref_draws


# ---------------------------------------------------------------- alphas x every family ----------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
def test_every_alpha_on_every_family(gmk, oracle, alpha):
    names, rows = stack(every_family())
    n = len(names)
    ids = np.array([GAME_IDS[i % len(GAME_IDS)] + (i // len(GAME_IDS)) * 1000003 for i in range(n)], dtype=np.uint64) % (1 << 32)
    stones = np.array([(37 * i + 5) % 225 for i in range(n)], dtype=np.uint32)
    mixed, draws = hold(oracle, names, rows, ids, stones, alpha, 0.25, 0x0123456789ABCDEF)
    took = rows * np.float32(0.75) != 0
    assert took.sum() >= 900 and (mixed != rows)[took].any()                 # (priors changed: the test is not about a no-op)
    assert (mixed[rows == 0] == 0).all()
    if alpha == 0.01:
        assert (draws[took] == 0).sum() > took.sum() // 2, "alpha 0.01: most draws are flushed to zero"
    if alpha >= 1.0:
        assert (draws[took] != 0).all(), "alpha >= 1: no draw is anywhere near the flush"
    else:
        assert (draws[took] != 0).any()


@pytest.mark.parametrize("epsilon", [0.25, 0.75])
def test_tiny_priors(gmk, oracle, epsilon):
    """2^-149 * 0.75 rounds to 2^-149: the entry keeps its draw.  2^-149 * 0.25 rounds to 0: it takes none, and ends at 0.  The smallest normal float
    is scaled to a subnormal either way and keeps its draw."""
    names, rows = stack(tiny_rows())
    ids, stones = np.arange(len(names)) + 11, np.full(len(names), 40)
    mixed, draws = hold(oracle, names, rows, ids, stones, 2.5, epsilon, 99)
    sub, nrm = rows == TINY_SUBNORMAL, rows == TINY_NORMAL
    assert sub.sum() == 4 and nrm.sum() == 3
    assert (draws[nrm] > 0).all()
    if epsilon == 0.25:
        assert (draws[sub] > 0).all() and (mixed[sub] > 0).all()
    else:
        assert (draws[sub] == 0).all() and (bits(mixed[sub]) == 0).all()
        assert not bits(mixed[1]).any()                                      # the row of the lone subnormal: nothing drew, the zero vector stays


# ---------------------------------------------------------------- epsilons, ids, stones, seeds on the full and random families ----------------------------------------------------------------
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("seed", SEEDS)
def test_keys_and_epsilons(gmk, oracle, epsilon, seed):
    """every game id with the stones cycling, every stone count with the ids cycling, under every seed and epsilon"""
    family = full_rows() + random_rows()
    names, rows, ids, stones = [], [], [], []
    for k, (name, row) in enumerate(family):
        keys = [(gid, STONES[(k + j) % 3]) for j, gid in enumerate(GAME_IDS)] + [(GAME_IDS[(k + j) % 5], st) for j, st in enumerate(STONES)]
        for gid, st in keys:
            names.append(name); rows.append(row); ids.append(gid); stones.append(st)
    rows = np.stack(rows)
    mixed, draws = hold(oracle, names, rows, ids, stones, 0.05, epsilon, seed)
    if epsilon == 0.0:
        np.testing.assert_array_equal(bits(mixed), bits(rows))               # P * 1 + 0 * noise
        assert (draws != 0).any()                                            # (the draws are made all the same)
    elif epsilon == 1.0:
        assert not bits(mixed).any() and not bits(draws).any()               # every entry is masked: P * 0 == 0 takes no draw
    else:
        assert (mixed != rows).any() and (draws != 0).any() and (draws[rows != 0] == 0).any()
    # the keys matter: the same row under two ids, and under two stone counts, drew differently
    if 0.0 < epsilon < 1.0:
        assert (draws[0] != draws[1]).any() and (draws[5] != draws[6]).any()


def test_seed_halves_and_id_bits_are_told_apart(gmk):
    """Device against device: a swapped pair of seed halves, a seed whose halves are equal to another's in one half only, and ids that differ only in
    bit 31 all give different draws (the comparisons with the serial statement above say which are right)."""
    row = np.full((1, N), ONE / np.float32(N), np.float32)
    base = device(row, [5], [9], 0.3, 0.25, 0x0000000100000002)[1]
    for ids, seed in (([5], 0x0000000200000001), ([5], 0x0000000100000000), ([5], 0x0000000000000002), ([5 + 2 ** 31], 0x0000000100000002)):
        assert (device(row, ids, [9], 0.3, 0.25, seed)[1] != base).any()


# ---------------------------------------------------------------- the zero-vector branch ----------------------------------------------------------------
def test_zero_vector_rows(gmk, oracle):
    """One root child at alpha 0.05: the only draw is flushed to 0 in about one root of eight, the vector of draws is then the zero vector, and
    normalized() leaves it: the prior ends at 0.75 p, not at NaN.  2 000 roots: cell 0, games 0 .. 1999, 220 stones, seed 5."""
    n = 2000
    rows = np.zeros((n, N), np.float32)
    rows[:, 0] = ONE
    ids, stones = np.arange(n), np.full(n, 220)
    names = ["single child, game %d" % g for g in range(n)]
    mixed, draws = hold(oracle, names, rows, ids, stones, 0.05, 0.25, 5)
    zero = draws[:, 0] == 0
    assert zero.sum() >= 50, "the inputs do not take the zero-vector branch often enough: %d of %d" % (zero.sum(), n)
    assert not zero.all()
    got = device(rows, ids, stones, 0.05, 0.25, 5)[0]
    expect = rows * np.float32(0.75)
    np.testing.assert_array_equal(bits(got[zero]), bits(expect[zero]))       # 0.75 p, to the bit, and finite
    assert (np.abs(got[~zero, 0] - 1) < 1e-6).all()                          # (one non-zero draw normalises to 1, give or take sqrt's rounding: the bits are held above)


# ---------------------------------------------------------------- rows are isolated; calls compose ----------------------------------------------------------------
def test_rows_are_isolated(gmk, oracle):
    """A row's result is the same bits alone, at another index of a larger call, and next to a row of NaN priors."""
    named = [full_rows()[1], random_rows()[3], random_rows()[6], layout_rows()[13]]
    names, rows = stack(named)
    ids, stones = np.array([2 ** 31, 3, 2 ** 32 - 1, 8]), np.array([0, 17, 224, 100])
    ref, ref_draws = hold(oracle, names, rows, ids, stones, 0.3, 0.25, 2 ** 63 + 12345)
    nan = np.full(N, np.nan, np.float32)
    for i in range(len(names)):
        alone, alone_draws = device(rows[i:i + 1], ids[i:i + 1], stones[i:i + 1], 0.3, 0.25, 2 ** 63 + 12345)
        np.testing.assert_array_equal(bits(alone[0]), bits(ref[i]))
        np.testing.assert_array_equal(bits(alone_draws[0]), bits(ref_draws[i]))
        crowd = np.stack([nan, rows[(i + 1) % 4], nan, rows[i], nan, rows[(i + 2) % 4], nan])
        cids, cst = [7, ids[(i + 1) % 4], ids[i], ids[i], ids[i], ids[(i + 2) % 4], 9], [1, stones[(i + 1) % 4], stones[i], stones[i], stones[i], stones[(i + 2) % 4], 2]
        got, got_draws = device(crowd, cids, cst, 0.3, 0.25, 2 ** 63 + 12345)
        np.testing.assert_array_equal(bits(got[3]), bits(ref[i]))
        np.testing.assert_array_equal(bits(got_draws[3]), bits(ref_draws[i]))
        np.testing.assert_array_equal(bits(got[1]), bits(ref[(i + 1) % 4]))
        np.testing.assert_array_equal(bits(got[5]), bits(ref[(i + 2) % 4]))
        assert np.isnan(got[[0, 2, 4, 6]]).all()                             # (a NaN prior is "a child": it draws, and stays NaN)


def test_a_second_call_mixes_again(gmk, oracle):
    import torch
    names, rows = stack(full_rows() + random_rows() + layout_rows())
    n = len(names)
    ids, stones = np.arange(n) * 977 + 2 ** 31 - 3, (np.arange(n) * 29) % 225
    once, _ = serial(oracle, rows, ids, stones, 0.05, 0.25, 2 ** 32)
    twice, draws2 = serial(oracle, once, ids, stones, 0.05, 0.25, 2 ** 32)
    p, d = torch.from_numpy(rows.copy()).cuda(), torch.zeros((n, N), device="cuda")
    G.noise_mix_rows(p, u32(ids), u32(stones), 0.05, 0.25, 2 ** 32)
    G.noise_mix_rows(p, u32(ids), u32(stones), 0.05, 0.25, 2 ** 32, draws=d)  # (the same stream: the second call follows the first)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(p.cpu().numpy()), bits(twice))
    np.testing.assert_array_equal(bits(d.cpu().numpy()), bits(draws2))
    assert (twice != once).any()


def test_no_rows_and_no_draws(gmk, oracle):
    import torch
    empty = torch.zeros((0, N), device="cuda")
    G.noise_mix_rows(empty, u32([]), u32([]), 0.05, 0.25, 1)                  # n = 0: nothing happens
    G.noise_mix_rows(empty, u32([]), u32([]), 0.05, 0.25, 1, draws=torch.zeros((0, N), device="cuda"))
    assert G.load().gmk_noise_mix_rows(None, None, None, None, 0, 0.05, 0.25, 1, None) == 0
    names, rows = stack(every_family())
    ids, stones = np.arange(len(names)), np.full(len(names), 12)
    with_draws, _ = device(rows, ids, stones, 0.3, 0.25, 1)
    without, none = device(rows, ids, stones, 0.3, 0.25, 1, want_draws=False)
    assert none is None
    np.testing.assert_array_equal(bits(without), bits(with_draws))
    np.testing.assert_array_equal(bits(without), bits(serial(oracle, rows, ids, stones, 0.3, 0.25, 1)[0]))


# ---------------------------------------------------------------- refused arguments ----------------------------------------------------------------
def test_refused_arguments_leave_the_rows_alone(gmk):
    import torch
    names, rows = stack(random_rows())
    n = len(names)
    p, d = torch.from_numpy(rows.copy()).cuda(), torch.full((n, N), 7.0, device="cuda")
    ids, stones = u32(np.arange(n)), u32(np.full(n, 3))
    bad = [(a, 0.25, "alpha") for a in (-1.0, float("nan"), float("inf"), 0.0)] + [(0.05, e, "epsilon") for e in (-0.5, 2.0, float("nan"))]
    for alpha, epsilon, which in bad:
        with pytest.raises(G.GmkError, match="gmk_noise_mix_rows: %s" % which):
            G.noise_mix_rows(p, ids, stones, alpha, epsilon, 1, draws=d)
    L = G.load()
    assert L.gmk_noise_mix_rows(p.data_ptr(), d.data_ptr(), ids.data_ptr(), stones.data_ptr(), -1, 0.05, 0.25, 1, None) == -3           # n < 0
    assert L.gmk_noise_mix_rows(p.data_ptr() + 2, d.data_ptr(), ids.data_ptr(), stones.data_ptr(), n - 1, 0.05, 0.25, 1, None) == -3     # misaligned
    assert L.gmk_noise_mix_rows(p.data_ptr(), d.data_ptr() + 1, ids.data_ptr(), stones.data_ptr(), n - 1, 0.05, 0.25, 1, None) == -3
    assert L.gmk_noise_mix_rows(p.data_ptr(), None, None, stones.data_ptr(), n, 0.05, 0.25, 1, None) == -3                              # a null input
    assert L.gmk_noise_mix_rows(None, None, ids.data_ptr(), stones.data_ptr(), n, 0.05, 0.25, 1, None) == -3
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(p.cpu().numpy()), bits(rows))          # nothing was launched
    assert (d == 7.0).all()


# ---------------------------------------------------------------- the entry keeps to its stream ----------------------------------------------------------------
def test_behind_a_delayed_producer(gmk, oracle):
    """tests/stream_harness.py: d_priors holds a decoy, the real rows arrive by a delayed copy on a side stream, and the entry is enqueued behind it.
    A launch on another stream would mix the decoy."""
    import torch
    from stream_harness import Harness
    from test_stream_contract_gpu import stateless
    H = Harness()
    names, rows = stack(every_family())
    n = len(names)
    rng = np.random.RandomState(21)
    real, decoy = torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(rng.uniform(0.1, 1.0, (n, N)).astype(np.float32)).cuda()
    ids_h, stones_h = (np.arange(n) * 131071 + 2 ** 32 - 9) % (1 << 32), (np.arange(n) * 13) % 225
    buf, draws, ids, stones = real.clone(), torch.zeros((n, N), device="cuda"), u32(ids_h), u32(stones_h)
    entry = lambda s: G.noise_mix_rows(buf, ids, stones, 0.3, 0.25, 2 ** 63 + 12345, draws=draws, stream=s)
    out = H.check("gmk_noise_mix_rows", stateless([(buf, decoy, real)], [draws], entry))
    ref_mixed, ref_draws = serial(oracle, rows, ids_h, stones_h, 0.3, 0.25, 2 ** 63 + 12345)
    np.testing.assert_array_equal(out["out0"].view(np.uint32), bits(ref_draws).reshape(-1))
    np.testing.assert_array_equal(out["out1"].view(np.uint32), bits(ref_mixed).reshape(-1))
