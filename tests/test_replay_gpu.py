"""The replay buffer on the device (replay_kernel.hip, selfplay.ReplayBuffer): every drawn tuple bit for bit against
GameRecords.to_samples of the records it came from, the picks against gmk_replay_draw_host and the documented population order,
eviction against a host mirror, both append forms, first_move, errors that change nothing, side streams and poisoned pool blocks."""
import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

pytestmark = pytest.mark.gpu

N = 225
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _synth(n, seed, lens=None):
    """Fixed-stride records with garbage past every length; all of the lengths 0, 1, 224, 225 present unless lens are given."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if lens is None:
        lens = torch.randint(0, N + 1, (n,), generator=g, device=DEV, dtype=torch.int32)
        edge = torch.tensor([0, 1, 224, 225], dtype=torch.int32, device=DEV)
        lens[: min(n, 4)] = edge[: min(n, 4)]
        if n > 8:
            lens[n // 2: n // 2 + 4] = edge.flip(0)
    else:
        lens = torch.as_tensor(lens, dtype=torch.int32, device=DEV)
    moves = torch.argsort(torch.rand((n, N), generator=g, device=DEV), dim=1).to(torch.uint8)
    winner = torch.randint(-1, 2, (n,), generator=g, device=DEV, dtype=torch.int8)
    vis = torch.randint(-32768, 32768, (n, N, N), generator=g, device=DEV, dtype=torch.int16)
    return selfplay.GameRecords(moves, lens, winner, vis)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Source:
    """One appended batch of records and the tuples to_samples makes of it."""

    def __init__(self, rec, first_move):
        self.rec, self.first = rec, first_move
        self.lens = rec.lens.cpu().numpy().astype(np.int64)
        self.cum = np.concatenate([[0], np.cumsum(np.maximum(self.lens - first_move, 0))])
        self._ref = {}

    def ref(self, augment):
        if augment not in self._ref:
            self._ref[augment] = self.rec.to_samples(augment=augment, first_move=self.first)
        return self._ref[augment]

    def row(self, game, ply, sym, augment):
        s = int(self.cum[game] + ply - self.first)
        return 8 * s + sym if augment else s


class Mirror:
    """The buffer's bookkeeping on the host, from the text of include/gomoku_hip.h: serials, eviction, population order."""

    def __init__(self, capacity_plies, max_games):
        self.cap, self.max_games, self.tail, self.held, self.sources = capacity_plies, max_games, 0, [], []

    def append(self, rec, first_move):
        src = Source(rec, first_move)
        self.sources.append(src)
        for g, l in enumerate(src.lens.tolist()):
            self.held.append({"serial": self.tail, "src": src, "game": g, "len": l, "first": first_move})
            self.tail += 1
        while sum(h["len"] for h in self.held) > self.cap or len(self.held) > self.max_games:
            self.held.pop(0)

    def stats(self):
        return {"games": len(self.held), "plies": sum(h["len"] for h in self.held),
                "population": sum(max(h["len"] - h["first"], 0) for h in self.held),
                "evicted_games": self.held[0]["serial"] if self.held else self.tail}

    def population(self):
        """[(held game, ply)] oldest first"""
        return [(h, t) for h in self.held for t in range(h["first"], h["len"])]


def _stats(buf):
    s = buf.stats()
    return {k: s[k] for k in ("games", "plies", "population", "evicted_games")}


def _check_draw(buf, mirror, batch, step, augment, float_too=True):
    """One draw against the mirror: picks, then states / value / pi bit for bit.  Returns the picks."""
    states, values, pi, picked = buf.sample(batch, step=step, augment=augment, dtype=torch.uint8, return_picked=True)
    assert buf.status()[1] == 0
    pop = mirror.population()
    M = len(pop) * (8 if augment else 1)
    idx = G.replay_draw_host(buf.seed, step, M, batch)
    exp_picked, rows = [], {}
    for i, p in enumerate(idx.tolist()):
        h, t = pop[p // 8] if augment else pop[p]
        a = p % 8 if augment else 0
        exp_picked.append((h["serial"], t, a))
        rows.setdefault(id(h["src"]), (h["src"], [], []))
        rows[id(h["src"])][1].append(i)
        rows[id(h["src"])][2].append(h["src"].row(h["game"], t, a, augment))
    assert picked.cpu().tolist() == [list(e) for e in exp_picked]
    for src, at, ref_rows in rows.values():
        r_states, r_values, r_pi = src.ref(augment)
        at = torch.tensor(at, device=DEV)
        ref_rows = torch.tensor(ref_rows, device=DEV)
        assert _bits_equal(states[at], r_states[ref_rows])
        assert _bits_equal(values[at], r_values[ref_rows])
        assert _bits_equal(pi[at], r_pi[ref_rows])
    if float_too:
        f_states, f_values, f_pi = buf.sample(batch, step=step, augment=augment, dtype=torch.float32)
        assert f_states.dtype == torch.float32 and _bits_equal(f_states, states.to(torch.float32))
        assert _bits_equal(f_values, values) and _bits_equal(f_pi, pi)
    return picked


def test_bits_real_games():
    rec = selfplay.play_games(6, 30, seed=5, first_game_id=0)
    buf = selfplay.ReplayBuffer(4096, max_games=64, seed=11)
    mirror = Mirror(4096, 64)
    buf.extend(rec)
    mirror.append(rec, 0)
    assert buf.status()[0] == 0 and _stats(buf) == mirror.stats()
    assert len(buf) == 8 * mirror.stats()["population"]
    for step in (0, 1, 2):
        _check_draw(buf, mirror, 64, step, True)
        _check_draw(buf, mirror, 32, step, False)
    a = buf.sample(16, step=5)
    b = buf.sample(16, step=5)
    c = buf.sample(16, step=6)
    assert all(_bits_equal(x, y) for x, y in zip(a, b)) and not _bits_equal(a[2], c[2])
    buf.close()


def test_bits_synthetic_and_first_move():
    cap = 3 * 12 * N
    buf = selfplay.ReplayBuffer(cap, max_games=40, seed=3)
    mirror = Mirror(cap, 40)
    for seed, fm in ((21, 0), (22, 3), (23, 225)):
        rec = _synth(12, seed)
        buf.extend(rec, first_move=fm)
        mirror.append(rec, fm)
    assert buf.status()[0] == 0 and _stats(buf) == mirror.stats()
    for augment in (True, False):
        picked = _check_draw(buf, mirror, 200, 7, augment).cpu().numpy()
        second = (picked[:, 0] >= 12) & (picked[:, 0] < 24)
        assert second.any() and (picked[second, 1] >= 3).all()           # plies below first_move are never drawn
        assert (picked[:, 0] < 24).all()                                 # first_move = 225: nothing of the third append is in the population
    # positions at later plies still contain the opening stones: ply t shows t stones
    states, _, _, picked = buf.sample(200, step=9, dtype=torch.uint8, return_picked=True)
    stones = states[:, 0].sum((1, 2)).to(torch.int64) + states[:, 1].sum((1, 2)).to(torch.int64)
    assert torch.equal(stones, picked[:, 1])
    buf.close()


def test_full_sweep_returns_every_sample_once():
    rec = _synth(9, 31)
    buf = selfplay.ReplayBuffer(9 * N, max_games=9, seed=4)
    mirror = Mirror(9 * N, 9)
    buf.extend(rec, first_move=2)
    mirror.append(rec, 2)
    for augment in (True, False):
        M = mirror.stats()["population"] * (8 if augment else 1)
        states, values, pi, picked = buf.sample(M, step=1, augment=augment, dtype=torch.uint8, return_picked=True)
        assert buf.status()[1] == 0
        src = mirror.sources[0]
        p = picked.cpu().numpy()
        rows = np.array([src.row(int(g), int(t), int(a), augment) for g, t, a in p])
        assert np.array_equal(np.sort(rows), np.arange(M))                # every sample exactly once
        order = torch.from_numpy(np.argsort(rows)).to(DEV)
        r_states, r_values, r_pi = src.ref(augment)
        assert _bits_equal(states[order], r_states) and _bits_equal(values[order], r_values) and _bits_equal(pi[order], r_pi)
    buf.close()


def test_append_forms_agree():
    recs = [selfplay.play_games(6, 30, seed=5, first_game_id=0), _synth(10, 41)]
    a = selfplay.ReplayBuffer(4000, max_games=12, seed=8)
    b = selfplay.ReplayBuffer(4000, max_games=12, seed=8)
    mirror = Mirror(4000, 12)
    for rec, fm in zip(recs, (1, 0)):
        a.extend(rec, first_move=fm)
        wire = selfplay.pack_records_device(rec)
        assert torch.equal(wire, selfplay.pack_records(rec))
        b.extend_packed(wire, len(rec), first_move=fm)
        mirror.append(rec, fm)
    assert a.status()[0] == 0 and b.status()[0] == 0
    assert _stats(a) == _stats(b) == mirror.stats()
    for augment in (True, False):
        _check_draw(b, mirror, 128, 3, augment)
        x = a.sample(128, step=3, augment=augment, return_picked=True)
        y = b.sample(128, step=3, augment=augment, return_picked=True)
        assert all(_bits_equal(p, q) for p, q in zip(x, y))
    a.close()
    b.close()


def test_eviction_third_append_evicts_the_first():
    first, second, third = _synth(3, 51, lens=[50, 60, 70]), _synth(2, 52, lens=[40, 30]), _synth(2, 53, lens=[100, 80])
    cap = 40 + 30 + 100 + 80                                              # the second and third appends fill it exactly
    buf = selfplay.ReplayBuffer(cap, max_games=10, seed=6)
    mirror = Mirror(cap, 10)
    for rec in (first, second):
        buf.extend(rec)
        mirror.append(rec, 0)
    assert _stats(buf) == mirror.stats() == {"games": 5, "plies": 250, "population": 250, "evicted_games": 0}
    buf.extend(third)
    mirror.append(third, 0)
    assert _stats(buf) == mirror.stats() == {"games": 4, "plies": 250, "population": 250, "evicted_games": 3}
    picked = _check_draw(buf, mirror, 8 * 250, 2, True, float_too=False).cpu().numpy()
    assert picked[:, 0].min() == 3 and picked[:, 0].max() == 6           # no draw returns an evicted game
    _check_draw(buf, mirror, 250, 2, False)
    buf.close()


def test_append_larger_than_the_buffer_keeps_the_newest():
    buf = selfplay.ReplayBuffer(300, max_games=10, seed=6)
    mirror = Mirror(300, 10)
    for rec in (_synth(2, 61, lens=[20, 30]), _synth(4, 62, lens=[200, 150, 100, 90])):
        buf.extend(rec)
        mirror.append(rec, 0)
    assert _stats(buf) == mirror.stats() == {"games": 2, "plies": 190, "population": 190, "evicted_games": 4}
    picked = _check_draw(buf, mirror, 190, 0, False).cpu().numpy()
    assert set(picked[:, 0].tolist()) == {4, 5}
    tail = _synth(1, 63, lens=[120])                                      # and the ring goes on from there
    buf.extend(tail)
    mirror.append(tail, 0)
    assert _stats(buf) == mirror.stats() == {"games": 2, "plies": 210, "population": 210, "evicted_games": 5}
    _check_draw(buf, mirror, 8 * 210, 1, True, float_too=False)
    buf.close()


def test_max_games_binds_before_the_ply_limit():
    buf = selfplay.ReplayBuffer(2000, max_games=3, seed=6)
    mirror = Mirror(2000, 3)
    for rec in (_synth(5, 71, lens=[10, 11, 12, 13, 14]), _synth(2, 72, lens=[9, 0])):
        buf.extend(rec, first_move=1)
        mirror.append(rec, 1)
    assert _stats(buf) == mirror.stats() == {"games": 3, "plies": 23, "population": 21, "evicted_games": 4}
    picked = _check_draw(buf, mirror, 8 * 21, 4, True).cpu().numpy()
    assert set(picked[:, 0].tolist()) == {4, 5}                           # the empty game 6 is held and never drawn
    buf.reset()
    assert _stats(buf) == {"games": 0, "plies": 0, "population": 0, "evicted_games": 0}
    buf.close()


def test_errors_change_nothing():
    rec = _synth(6, 81, lens=[30, 31, 32, 33, 34, 35])
    buf = selfplay.ReplayBuffer(1000, max_games=20, seed=9)
    mirror = Mirror(1000, 20)
    buf.extend(rec)
    mirror.append(rec, 0)
    before = buf.sample(100, step=1, return_picked=True)
    for bad_len in (226, -1):
        bad = _synth(4, 82, lens=[5, 6, bad_len, 7])
        buf.extend(bad)
        assert buf.status()[0] == G.REPLAY_BAD_LENGTH
        assert _stats(buf) == mirror.stats()
        wire = torch.cat([bad.lens.view(torch.uint8).reshape(-1), torch.zeros(4 + 18 * 451, dtype=torch.uint8, device=DEV)])
        buf.extend_packed(wire, 4)
        assert buf.status()[0] == G.REPLAY_BAD_LENGTH
        assert _stats(buf) == mirror.stats()
    after = buf.sample(100, step=1, return_picked=True)
    assert all(_bits_equal(x, y) for x, y in zip(before, after))
    good = _synth(1, 83, lens=[12])
    buf.extend(good)                                                      # a good append clears the word
    mirror.append(good, 0)
    assert buf.status()[0] == 0 and _stats(buf) == mirror.stats()

    # a draw of more than the population writes no output byte
    P = mirror.stats()["population"]
    for augment, batch in ((True, 8 * P + 1), (False, P + 1)):
        states = torch.full((batch, 6, 15, 15), 0x5A, dtype=torch.uint8, device=DEV)
        values = torch.full((batch,), 7.0, device=DEV)
        pi = torch.full((batch, N), 7.0, device=DEV)
        picked = torch.full((batch, 3), -7, dtype=torch.int64, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        buf._h.sample(batch, 0, augment, False, states.data_ptr(), values.data_ptr(), pi.data_ptr(), picked.data_ptr(), status.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
        assert int(status.item()) == G.REPLAY_TOO_FEW
        assert (states == 0x5A).all() and (values == 7.0).all() and (pi == 7.0).all() and (picked == -7).all()
        buf.sample(batch, step=0, augment=augment)
        assert buf.status()[1] == G.REPLAY_TOO_FEW
    assert _stats(buf) == mirror.stats()
    _check_draw(buf, mirror, 8 * P, 0, True, float_too=False)             # exactly the population is fine
    L = G.load()
    assert L.gmk_replay_sample(buf._h.h, -1, 0, 1, 1, None, None, None, None, None, None) == -3
    assert L.gmk_replay_sample(buf._h.h, 0, 0, 1, 1, None, None, None, None, None, None) == 0
    assert L.gmk_replay_append(buf._h.h, None, None, None, None, 0, 0, None, None) == 0
    assert L.gmk_replay_append(buf._h.h, None, None, None, None, 3, 0, None, None) == -3
    assert L.gmk_replay_append(buf._h.h, rec.moves.data_ptr(), rec.lens.data_ptr() + 2, rec.winner.data_ptr(), rec.visits.data_ptr(), 3, 0,
                               buf._status.data_ptr(), None) == -3       # misaligned lens
    buf.close()


def test_batches_generator():
    rec = _synth(2, 91, lens=[20, 12])
    buf = selfplay.ReplayBuffer(500, seed=2)
    assert list(buf.batches(16)) == []
    buf.extend(rec)
    assert len(buf) == 8 * 32
    gen = buf.batches(8 * 32)                                             # yields only while len > batch_size (data_helper.py:137)
    assert list(gen) == []
    gen = buf.batches(64)
    first, second = next(gen), next(gen)
    assert first[0].shape == (64, 6, 15, 15) and first[0].dtype == torch.float32 and first[2].shape == (64, N)
    assert not _bits_equal(first[2], second[2])                           # the internal step counter moves on
    buf.close()


def test_side_stream_and_poisoned_pool():
    rec = selfplay.play_games(6, 30, seed=5, first_game_id=0)
    cap = 40000                                                           # 18 MB of visit rows: a block of the library's pool
    ref = selfplay.ReplayBuffer(cap, max_games=64, seed=13)
    ref.extend(rec, first_move=1)
    want = ref.sample(256, step=4, return_picked=True)
    torch.cuda.synchronize()
    ref.close()
    G.pool_poison(True)
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            buf = selfplay.ReplayBuffer(cap, max_games=64, seed=13)      # the block ref gave back, filled with 0xA5
            mirror = Mirror(cap, 64)
            buf.extend(rec, first_move=1)
            mirror.append(rec, 1)
            got = buf.sample(256, step=4, return_picked=True)
            _check_draw(buf, mirror, 256, 5, True)
        side.synchronize()
        assert all(_bits_equal(x, y) for x, y in zip(want, got))
        buf.close()
    finally:
        G.pool_poison(False)
