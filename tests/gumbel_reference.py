"""The Gumbel root rule of K21 (include/gomoku_gumbel.h) restated in Python floats, for the tests.  It shares nothing with the header: its own
Philox4x32-10, its own log and exp (IEEE binary64, the same operations in the same order as the header's gmk_noise_log / gmk_noise_exp, as
tests/test_noise.py restates them), and the rule written from its statement -- the schedule is built as a list, the considered set comes from
a sort, the row's sum is added along the association the header names.  A root is given by cell: prior (0 = no child), visits, value."""
import math
import struct

import numpy as np

N = 225
M32 = 0xFFFFFFFF
TAG = 0x676D626C                                                 # 'gmbl'


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def py_log(x):
    b = _bits(x)
    e = (b >> 52) - 1023
    m = _from_bits((b & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000)
    if m > 1.4142135623730951:
        m, e = m * 0.5, e + 1
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = 1.0 / 23.0
    for d in (21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
        p = p * s2 + 1.0 / d
    p = p * s2 + 1.0
    return float(e) * 0.6931471805599453 + 2.0 * (s * p)


def py_exp(x):
    if x < -700.0:
        return 0.0
    k = int(x * 1.4426950408889634 - 0.5)
    r = (x - float(k) * 0.693147180369123816490) - float(k) * 1.90821492927058770002e-10
    p = 1.0 / 6227020800.0
    for d in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / d
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    return p * _from_bits((k + 1023) << 52)


def uniform_of(game_id, stones, cell, seed):
    w = philox4x32_10((game_id & M32, stones, TAG, cell), (seed & M32, (seed >> 32) & M32))
    return (float(w[0]) + 0.5) * 2.3283064365386962890625e-10


def draw(game_id, stones, cell, seed):
    """g_c"""
    return -py_log(-py_log(uniform_of(game_id, stones, cell, seed)))


def logit(prior):
    return py_log(float(np.float32(prior)))


def sequence(m_eff, n):
    """seq[0 .. n), built as the rule states it"""
    if m_eff == 1:
        return list(range(n))
    levels = int(math.ceil(math.log2(m_eff)))
    seq, k, c = [], m_eff, 0
    while len(seq) < n:
        extra = max(1, n // (levels * k))
        for _ in range(extra):
            seq.extend([c] * k)
            c += 1
        k = max(2, k // 2)
    return seq[:n]


def sum225(v):
    """the association of gmk_noise_sum225, in Python floats"""
    p = [0.0] * 64
    for l in range(64):
        p[l] = v[l]
        for j in (1, 2, 3):
            if l + 64 * j < N:
                p[l] = p[l] + v[l + 64 * j]
    for off in (8, 4, 2, 1):
        p = [p[l] + (p[l + off] if (l & 15) + off < 16 else 0.0) for l in range(64)]
    return (p[0] + p[16]) + (p[32] + p[48])


class Root:
    """One root's set-up (fixed when it is made) and the three questions asked of it."""

    def __init__(self, prior, visits, m, game_id, stones, seed, c_visit=50.0, c_scale=1.0):
        self.c_visit, self.c_scale = float(c_visit), float(c_scale)
        self.children = [c for c in range(N) if prior[c] != 0]
        self.score = {c: draw(game_id, stones, c, seed) + logit(prior[c]) for c in self.children}
        ranked = sorted(self.children, key=lambda c: (-self.score[c], c))        # the largest first, ties to the lower cell
        self.m_eff = min(int(m), len(self.children))
        self.considered = sorted(ranked[:self.m_eff])
        self.base = {c: int(visits[c]) for c in self.children}

    def _sigma(self, c, visits, value, root_value):
        most = max(int(visits[b]) for b in self.children)
        if visits[c] > 0:
            qhat = (float(np.float32(value[c])) + 1.0) / 2.0
        else:
            qhat = (-float(np.float32(root_value)) + 1.0) / 2.0
        return ((self.c_visit + float(most)) * self.c_scale) * qhat

    def _best(self, cells, visits, value, root_value):
        best, best_key = -1, None
        for c in cells:                                          # ascending cells, strict '>': ties to the lower cell
            key = self.score[c] + self._sigma(c, visits, value, root_value)
            if best < 0 or key > best_key:
                best, best_key = c, key
        return best

    def r(self, c, visits):
        return int(visits[c]) - self.base[c]

    def pick(self, visits, value, root_value, n):
        if not self.children:
            return -1
        t = sum(self.r(c, visits) for c in self.children)
        if t < n:
            want = sequence(self.m_eff, n)[t]
            cells = [c for c in self.considered if self.r(c, visits) == want]
            if cells:
                return self._best(cells, visits, value, root_value)
        least = min(self.r(c, visits) for c in self.considered)
        return self._best([c for c in self.considered if self.r(c, visits) == least], visits, value, root_value)

    def move(self, visits, value, root_value):
        if not self.children:
            return -1
        most = max(self.r(c, visits) for c in self.considered)
        return self._best([c for c in self.considered if self.r(c, visits) == most], visits, value, root_value)


def row(prior, visits, value, root_value, c_visit=50.0, c_scale=1.0):
    """the improved-policy row, uint16[225]"""
    children = [c for c in range(N) if prior[c] != 0]
    out = np.zeros(N, dtype=np.uint16)
    if not children:
        return out
    most = max(int(visits[b]) for b in children)
    x = {}
    for c in children:
        qhat = (float(np.float32(value[c])) + 1.0) / 2.0 if visits[c] > 0 else (-float(np.float32(root_value)) + 1.0) / 2.0
        x[c] = logit(prior[c]) + ((float(c_visit) + float(most)) * float(c_scale)) * qhat
    top = max(x.values())
    e = [0.0] * N
    for c in children:
        e[c] = py_exp(x[c] - top)
    z = sum225(e)
    for c in children:
        out[c] = int(math.floor(e[c] / z * 65535.0 + 0.5))
    return out
