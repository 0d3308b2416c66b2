"""The move-sampling rule of self-play on the host (gmk_move_sample_host, include/gomoku_sample.h) against tests/move_sample_reference.py, a
restatement in Python integers with its own Philox: known-answer blocks, exact agreement on random and edge rows, the frequencies of a
five-cell root over 32 768 games, and the arguments the entry refuses.  No GPU is needed."""
import numpy as np
import pytest

import move_sample_reference as M
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

N = 225
SEED = 0x9E3779B97F4A7C15
ERR_ARG = -3
KNOWN = {                                                        # (game id, stones) -> the block of counter (game id, stones, 'samp', 0) under SEED
    (0, 0): (0x5DBC6595, 0xB229535A, 0xFC22710A, 0x53A00566),
    (7, 3): (0xEA06A2B5, 0x9DBD3202, 0x00AA1693, 0x531E2CCA),
}


def _host(visits, stones, ids, plies, power, seed=SEED, proofs=None):
    return G.move_sample_host(np.asarray(visits, np.uint32), stones, ids, plies, power, seed, proofs).tolist()


def _row(pairs):
    row = np.zeros(N, np.uint32)
    for cell, v in pairs:
        row[cell] = v
    return row


# ---------------- 1. known answers ----------------
def test_the_tag_and_the_known_blocks():
    assert M.SAMPLE_TAG == 0x73616D70
    for (game, stones), block in KNOWN.items():
        assert M.philox4x32_10((game, stones, M.SAMPLE_TAG, 0), (SEED & M.M32, SEED >> 32)) == block
        assert M.draw(SEED, game, stones) == block[0] | block[1] << 32


@pytest.mark.parametrize("key", sorted(KNOWN))
def test_the_host_form_draws_the_known_blocks(key):
    """Two children of a and b visits: the first is played exactly when floor(r (a^k + b^k) / 2^64) < a^k, r written out from the known block.
    For each b the values of a are the integers around the one at which a^k / (a^k + b^k) crosses r / 2^64, so the answers change sides
    within the rows and a host form with another block, tag or word order disagrees on some of them."""
    game, stones = key
    r = KNOWN[key][0] | KNOWN[key][1] << 32
    frac = r / 2.0 ** 64
    rows, want, powers = [], [], []
    for power in (1, 2, 3):
        for b in (1000, 4001, 65535):
            # a^k / (a^k + b^k) close to frac from either side: a = b (frac / (1 - frac))^(1/k), then the integers around it
            centre = int(round(b * (frac / (1.0 - frac)) ** (1.0 / power)))
            for a in range(max(1, centre - 3), min(65535, centre + 3) + 1):
                wa, wb = a ** power, b ** power
                rows.append(_row([(17, a), (200, b)]))
                want.append(17 if (r * (wa + wb)) >> 64 < wa else 200)
                powers.append(power)
    assert len(set(want)) == 2                                   # both sides of the draw are met
    for power in (1, 2, 3):
        idx = [i for i, p in enumerate(powers) if p == power]
        got = _host(np.stack([rows[i] for i in idx]), [stones] * len(idx), [game] * len(idx), stones + 1, power)
        assert got == [want[i] for i in idx]


# ---------------- 2. exact agreement ----------------
def _random_rows(rng, n, with_proofs):
    visits = np.zeros((n, N), np.uint32)
    proofs = np.zeros((n, N), np.int8) if with_proofs else None
    for g in range(n):
        kids = rng.choice(N, size=rng.integers(1, N + 1), replace=False)
        scale = [4, 40, 3000, 70000, 200000][g % 5]
        visits[g, kids] = rng.integers(0, scale, size=len(kids))
        if with_proofs:
            proofs[g, kids] = rng.choice([0, 0, 0, M.PROOF_WINS, M.PROOF_LOSES] if g % 3 == 0 else [0, 0, M.PROOF_WINS], size=len(kids))
    return visits, proofs


@pytest.mark.parametrize("with_proofs", [False, True])
def test_random_rows_equal_the_restatement(with_proofs):
    rng = np.random.default_rng(20 + with_proofs)
    n = 2000
    visits, proofs = _random_rows(rng, n, with_proofs)
    stones = rng.integers(0, 40, size=n).astype(np.int32)
    ids = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    seen = set()
    for plies, power, seed in ((30, 1, SEED), (30, 2, 12345), (225, 3, 2 ** 64 - 1), (0, 1, SEED)):
        got = _host(visits, stones, ids, plies, power, seed, proofs)
        want = [M.choose(visits[g], int(stones[g]), int(ids[g]), plies, power, seed, None if proofs is None else proofs[g]) for g in range(n)]
        assert got == want
        seen.add(tuple(got))
    assert len(seen) == 4                                        # plies, power and seed all matter
    greedy = selfplay._root_choice(visits, proofs).tolist()
    assert _host(visits, stones, ids, 0, 1, SEED, proofs) == greedy       # off is today's choice, as the host loops make it


def test_edge_rows():
    zero = np.zeros(N, np.uint32)
    assert _host([zero], [0], [0], 225, 1) == [-1] and M.choose(zero, 0, 0, 225, 1, SEED) == -1
    one = _row([(112, 3)])
    assert _host([one] * 3, [0, 1, 2], [5, 6, 7], 225, 2) == [112] * 3
    # 225 children of 65 535 visits at k = 3: T = 225 * 65535^3 < 2^56, every child weighs the same: the cell is floor(225 r / 2^64)
    full = np.full(N, 65535, np.uint32)
    ids = list(range(300))
    want = [(225 * M.draw(SEED, g, 4)) >> 64 for g in ids]
    assert _host([full] * 300, [4] * 300, ids, 225, 3) == want == [M.choose(full, 4, g, 225, 3, SEED) for g in ids]
    assert len(set(want)) > 150
    # visits above 65 535 are saturated first: the weights are those of the record's row
    big = _row([(3, 65535), (90, 70000), (91, 4000000000), (224, 65536)])
    sat = np.minimum(big, 65535)
    for power in (1, 2, 3):
        got = _host([big] * 200, [0] * 200, ids[:200], 1, power)
        assert got == _host([sat] * 200, [0] * 200, ids[:200], 1, power) == [M.choose(big, 0, g, 1, power, SEED) for g in ids[:200]]
        assert sorted(set(got)) == [3, 90, 91, 224]
    assert _host([big], [1], [0], 1, 1) == [91]                  # the greedy choice reads the raw counts
    # stones = S - 1 is drawn, stones = S is not
    row = _row([(10, 50), (20, 49), (30, 48), (40, 47)])
    for s in (1, 6, 225):
        drawn = _host([row] * 200, [s - 1] * 200, ids[:200], s, 1)
        assert drawn == [M.choose(row, s - 1, g, s, 1, SEED) for g in ids[:200]] and len(set(drawn)) == 4
        if s < 225:
            assert _host([row] * 200, [s] * 200, ids[:200], s, 1) == [10] * 200


def test_proof_rows():
    ids = list(range(200))
    row = _row([(10, 50), (20, 49), (30, 0), (40, 47)])
    # a LOSES child is played, the first one, with or without a visit, and nothing is drawn
    proofs = np.zeros(N, np.int8)
    proofs[[30, 40]] = M.PROOF_LOSES
    assert _host([row] * 200, [0] * 200, ids, 6, 1, proofs=[proofs] * 200) == [30] * 200
    # WINS children weigh nothing
    proofs = np.zeros(N, np.int8)
    proofs[10] = M.PROOF_WINS
    got = _host([row] * 200, [0] * 200, ids, 6, 1, proofs=[proofs] * 200)
    assert got == [M.choose(row, 0, g, 6, 1, SEED, proofs) for g in ids] and sorted(set(got)) == [20, 40]
    # every visited child is WINS: today's choice, the most visited child
    proofs = np.zeros(N, np.int8)
    proofs[[10, 20, 40]] = M.PROOF_WINS
    want = int(selfplay._root_choice(row[None], proofs[None])[0])
    assert want == 10 and _host([row] * 200, [0] * 200, ids, 6, 3, proofs=[proofs] * 200) == [10] * 200
    assert M.choose(row, 0, 9, 6, 3, SEED, proofs) == 10
    # and with no visit anywhere there is nothing to play
    assert _host([np.zeros(N, np.uint32)], [0], [0], 6, 1, proofs=[proofs]) == [-1]


# ---------------- 3. frequencies ----------------
CELLS, VISITS = (7, 60, 112, 113, 224), (1, 2, 4, 8, 17)
GAMES = 32768


@pytest.mark.parametrize("stones", [0, 5])
@pytest.mark.parametrize("power", [1, 2, 3])
def test_frequencies(power, stones):
    row = _row(zip(CELLS, VISITS))
    got = _host(np.broadcast_to(row, (GAMES, N)), [stones] * GAMES, np.arange(GAMES), 225, power)
    counts = [got.count(c) for c in CELLS]
    assert sum(counts) == GAMES
    ref = [0] * 5
    for g in range(GAMES):
        ref[CELLS.index(M.choose(row, stones, g, 225, power, SEED))] += 1
    assert counts == ref
    total = sum(v ** power for v in VISITS)
    for count, v in zip(counts, VISITS):
        p = v ** power / total
        assert abs(count - GAMES * p) <= 4.0 * (GAMES * p * (1.0 - p)) ** 0.5, (power, stones, counts)
    if (power, stones) == (1, 0):
        assert counts == [976, 2026, 4123, 8018, 17625]


# ---------------- 4. arguments ----------------
def test_bad_arguments_are_refused():
    L = G.load()
    v, s, i, c = np.zeros((2, N), np.uint32), np.zeros(2, np.int32), np.zeros(2, np.uint32), np.full(2, 77, np.int16)
    args = lambda plies, power, n=2: L.gmk_move_sample_host(v.ctypes.data, None, s.ctypes.data, i.ctypes.data, n, plies, power, SEED, c.ctypes.data)
    assert args(-1, 1) == ERR_ARG and args(226, 1) == ERR_ARG and args(6, 0) == ERR_ARG and args(6, 4) == ERR_ARG and args(6, 1, -1) == ERR_ARG
    assert b"gmk_move_sample_host" in L.gmk_last_error()
    assert L.gmk_move_sample_host(None, None, s.ctypes.data, i.ctypes.data, 2, 6, 1, SEED, c.ctypes.data) == ERR_ARG
    assert L.gmk_move_sample_host(v.ctypes.data, None, None, i.ctypes.data, 2, 6, 1, SEED, c.ctypes.data) == ERR_ARG
    assert L.gmk_move_sample_host(v.ctypes.data, None, s.ctypes.data, None, 2, 6, 1, SEED, c.ctypes.data) == ERR_ARG
    assert L.gmk_move_sample_host(v.ctypes.data, None, s.ctypes.data, i.ctypes.data, 2, 6, 1, SEED, None) == ERR_ARG
    s[1] = 226
    assert args(6, 1) == ERR_ARG
    s[1] = -1
    assert args(6, 1) == ERR_ARG
    s[1] = 225
    assert c.tolist() == [77, 77]                                # a refused call writes nothing
    assert args(225, 3) == 0 and c.tolist() == [-1, -1] and args(0, 1) == 0 and args(6, 1, 0) == 0
    with pytest.raises(G.GmkError):
        G.move_sample_host(v, s, i, 6, 5, SEED)
    with pytest.raises(ValueError):
        selfplay.play_network_games(2, None, 4, sample_plies=226)
    with pytest.raises(ValueError):
        selfplay.play_network_games(2, None, 4, sample_plies=6, sample_power=4)
