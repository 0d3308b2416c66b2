"""An independent restatement of include/gomoku_symmetry.h ("K22") in numpy, with none of the library's code in between: the transform of a
position and the way back for a policy row through np.rot90 / np.fliplr (not through an index table), the ordered float32 average of
GMK_PVNET_SYM_ALL, and the pick of GMK_PVNET_SYM_RANDOM in numpy and Python integers.

Symmetry a in 0..7: k = a >> 1 quarter turns (np.rot90), then a left-right mirror (np.fliplr) when a & 1 -- the family and the order of the
training augmentation (tests/helpers.py: symmetries)."""
import numpy as np

N = 225
SYM_TAG = 0x73796D6D                                             # 'symm'
MASK64 = (1 << 64) - 1


def transform(states, a):
    """states [n, 6, 15, 15] (or [n, 15, 15]) -> every plane turned a >> 1 times and mirrored if a & 1"""
    x = np.asarray(states)
    out = np.rot90(x, a >> 1, axes=(x.ndim - 2, x.ndim - 1))
    if a & 1:
        out = out[..., ::-1]                                     # np.fliplr of every plane
    return np.ascontiguousarray(out)


def back(probs, a):
    """probs [n, 225] over the a-transformed board -> over the board itself: the mirror undone, then the turns"""
    g = np.asarray(probs).reshape(-1, 15, 15)
    if a & 1:
        g = g[..., ::-1]
    g = np.rot90(g, -(a >> 1), axes=(1, 2))
    return np.ascontiguousarray(g).reshape(-1, N)


def combine_all(values, probs):
    """values: eight float32 [n]; probs: eight float32 [n, 225], already back-transformed -> ((v_0 + v_1) + .. + v_7) * 0.125f, likewise per cell"""
    v, p = np.asarray(values[0], np.float32).copy(), np.asarray(probs[0], np.float32).copy()
    for a in range(1, 8):
        v = (v + np.asarray(values[a], np.float32)).astype(np.float32)
        p = (p + np.asarray(probs[a], np.float32)).astype(np.float32)
    return (v * np.float32(0.125)).astype(np.float32), (p * np.float32(0.125)).astype(np.float32)


def splitmix64(x):
    """x: numpy uint64 array -> SplitMix64's output function of x + the golden-ratio increment, modulo 2^64"""
    with np.errstate(over="ignore"):
        z = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def digest(states):
    """states [n, 6, 15, 15] -> uint64 [n]: the sum of splitmix64(4 c + code) over the occupied cells, plus splitmix64(900 + colour)"""
    s = np.asarray(states).reshape(-1, 6, N)
    code = (s[:, 0] != 0).astype(np.uint64) + np.uint64(2) * (s[:, 1] != 0).astype(np.uint64)
    terms = np.where(code != 0, splitmix64(np.uint64(4) * np.arange(N, dtype=np.uint64)[None, :] + code), np.uint64(0))
    with np.errstate(over="ignore"):
        d = terms.sum(axis=1, dtype=np.uint64) + splitmix64(np.uint64(900) + (s[:, 5, 0] != 0).astype(np.uint64))
    return d


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., SC11) in Python integers"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def pick(states, seed):
    """-> int32 [n]: word 0 & 7 of philox(digest low, digest high, 'symm', 0; key = seed low, seed high)"""
    seed &= MASK64
    out = []
    for d in digest(states).tolist():
        out.append(philox4x32((d & 0xFFFFFFFF, d >> 32, SYM_TAG, 0), (seed & 0xFFFFFFFF, seed >> 32))[0] & 7)
    return np.array(out, dtype=np.int32)


def positions(n, seed, max_stones=60):
    """n distinct, asymmetric random positions as Board.encoded_states() lays them out, float32 [n, 6, 15, 15]: 5 .. max_stones stones split
    between the mover and the opponent as a game would have them, the empty plane, the last two moves, the colour plane."""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, 6, N), np.float32)
    for g in range(n):
        stones = int(rng.randint(5, max_stones + 1))
        cells = rng.permutation(N)[:stones]
        mine, theirs = cells[stones % 2::2], cells[1 - stones % 2::2]       # the opponent made the last move
        out[g, 0, mine] = 1
        out[g, 1, theirs] = 1
        out[g, 2] = 1 - out[g, 0] - out[g, 1]
        out[g, 3, cells[-1]] = 1
        out[g, 4, cells[-2]] = 1
        out[g, 5] = 1 if stones % 2 == 0 else 0
    return out.reshape(n, 6, 15, 15)
