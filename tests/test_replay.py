"""The replay buffer's draw rule on the host (gmk_replay_draw_host) against a numpy restatement written from the text of
include/gomoku_hip.h ("replay buffer", "Draw rule"), exact bijectivity, and what the entries and ReplayBuffer refuse without a GPU."""
import ctypes as C

import numpy as np
import pytest

from gomokuai_amd import lib as G

POPULATIONS = [1, 2, 3, 8, 225, 1800, 10007, 8 * 1300000]
KEYS = [(0, 0), (G.DEFAULT_SEED, 0), (G.DEFAULT_SEED, 1), (12345, 7), (0xFFFFFFFFFFFFFFFF, (1 << 40) + 3), (1, 0xFFFFFFFF)]

U32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10_word0(c0, c1, c2, c3, k0, k1):
    """First output word of Philox4x32 with ten rounds (Salmon et al., SC'11); every argument a uint64 array holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64).copy() for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & U32, p0 & U32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return c0


def _half_bits(M):
    k = 0
    while 4 ** k < M:
        k += 1
    return k


def _feistel(x, k, seed, step):
    mask = np.uint64((1 << k) - 1)
    kk = np.uint64(k)
    L, R = (x >> kk) & mask, x & mask
    for r in range(4):
        F = _philox4x32_10_word0(R, np.uint64(r), np.uint64(step & 0xFFFFFFFF), np.uint64((step >> 32) & 0xFFFFFFFF),
                                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF) & mask
        L, R = R, L ^ F
    return (L << kk) | R


def draw_numpy(seed, step, M, batch):
    """perm(0 .. batch-1): the Feistel network applied once, and again while the result is >= M."""
    k = _half_bits(M)
    x = _feistel(np.arange(batch, dtype=np.uint64), k, seed, step)
    while True:
        out = x >= np.uint64(M)
        if not out.any():
            return x.astype(np.int64)
        x[out] = _feistel(x[out], k, seed, step)


@pytest.mark.parametrize("M", POPULATIONS)
def test_draw_host_equals_numpy_restatement(M):
    for seed, step in KEYS:
        batch = min(M, 4096)
        got = G.replay_draw_host(seed, step, M, batch)
        assert got.dtype == np.int64 and got.shape == (batch,)
        assert np.array_equal(got, draw_numpy(seed, step, M, batch)), (M, seed, step)
    if M <= 10007:                                     # the whole permutation, index for index
        assert np.array_equal(G.replay_draw_host(99, 3, M, M), draw_numpy(99, 3, M, M))


@pytest.mark.parametrize("M", POPULATIONS)
def test_full_draw_is_a_permutation(M):
    for seed, step in KEYS[:3]:
        got = G.replay_draw_host(seed, step, M, M)
        assert got.min() == 0 and got.max() == M - 1
        assert np.array_equal(np.bincount(got, minlength=M), np.ones(M, dtype=np.int64))      # every index exactly once


def test_steps_differ_and_repeat():
    M, B = 8 * 1300000, 512
    a = G.replay_draw_host(G.DEFAULT_SEED, 10, M, B)
    assert np.array_equal(a, G.replay_draw_host(G.DEFAULT_SEED, 10, M, B))
    assert not np.array_equal(a, G.replay_draw_host(G.DEFAULT_SEED, 11, M, B))
    assert not np.array_equal(a, G.replay_draw_host(G.DEFAULT_SEED + 1, 10, M, B))
    assert len(set(a.tolist())) == B
    # a prefix of a larger batch of the same (seed, step) is the smaller batch
    assert np.array_equal(a[:100], G.replay_draw_host(G.DEFAULT_SEED, 10, M, 100))


def test_draw_host_refuses():
    L = G.load()
    out = np.zeros(8, dtype=np.int64)
    assert L.gmk_replay_draw_host(1, 0, 5, 6, out.ctypes.data) == -3           # batch > population: GMK_ERR_ARG
    assert L.gmk_replay_draw_host(1, 0, 5, -1, out.ctypes.data) == -3
    assert L.gmk_replay_draw_host(1, 0, -5, 0, out.ctypes.data) == -3
    assert L.gmk_replay_draw_host(1, 0, 5, 5, None) == -3
    assert L.gmk_replay_draw_host(1, 0, 0, 0, None) == 0                       # batch = 0 is a no-op
    assert (out == 0).all()
    with pytest.raises(G.GmkError):
        G.replay_draw_host(1, 0, 5, 6)


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_init(0) == -1                                                  # GMK_ERR_NO_DEVICE
    h = C.c_void_p()
    assert L.gmk_replay_create(1000, 10, 0, C.byref(h)) == -4                   # GMK_ERR_STATE
    assert not h.value
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_replay_reset(None, None) == -4
    assert L.gmk_replay_append(None, None, None, None, None, 4, 0, None, None) == -4
    assert L.gmk_replay_append_packed(None, None, 4, None, 0, None, None) == -4
    assert L.gmk_replay_size(None, None, None, None, None, None) == -4
    assert L.gmk_replay_sample(None, 4, 0, 1, 1, None, None, None, None, None, None) == -4
    assert L.gmk_replay_destroy(None) == 0
    with pytest.raises(G.GmkError):
        G.ReplayHandle(1000, 10)
    from gomokuai_amd import selfplay
    with pytest.raises(G.GmkError):
        selfplay.ReplayBuffer(1000, device="cuda:0")


def test_replay_buffer_argument_checks():
    from gomokuai_amd import selfplay
    with pytest.raises(ValueError):
        selfplay.ReplayBuffer(224)                                              # less than one full game
    with pytest.raises(ValueError):
        selfplay.ReplayBuffer(1000, max_games=0)
    with pytest.raises(ValueError):
        selfplay.ReplayBuffer(1000, max_games=1001)
    assert G.REPLAY_BAD_LENGTH == 1 and G.REPLAY_TOO_FEW == 2
    for name in ("extend", "extend_packed", "sample", "batches", "stats", "status", "reset", "close", "__len__"):
        assert callable(getattr(selfplay.ReplayBuffer, name))
