"""Each searcher's own kernel around the device mixing of Default::AddNoise (counter-based sampler), beyond (alpha, epsilon) = (0.05, 0.25).

K7 (az_root_noise_kernel), K6, K6 + RAVE and K8 (trad_root_noise_kernel) read their root priors out by cell, so the kernel's gather, key and scatter
are held directly: the priors after add_root_noise == the serial statement (include/gomoku_noise.h through gcc: the oracle's go_noise_mix225) of the
priors before it, bit for bit, keyed by (first_game_id + id) mod 2^32, the stones on the root and the seed.  tests/test_noise_rows_gpu.py holds
the mixing itself at every alpha, child set and key edge; here the roots, ids and seeds are chosen for what each kernel adds.

K3 has no prior read-out, and a persistent launch (K3's root_noise_one, K6's trad_root_noise inside trad_playouts_kernel) shows nothing between
its searches: they are held through the game records, as tests/test_selfplay_gpu.py and tests/test_selfplay_sample_gpu.py hold them at
(0.05, 0.25) -- persistent == lock step == host loop == the oracle's kept-tree game loop with the same sampler -- at three more pairs.

The argument rule of include/gomoku_hip.h ("Root noise parameters") is held on every entry: a refused call changes nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

pytestmark = pytest.mark.gpu

N = 225
COUNTER = G.NOISE_SAMPLERS["counter"]
PAIRS = [(0.05, 0.25), (1.0, 0.25), (2.5, 0.5), (0.01, 0.25)]
NEW_PAIRS = PAIRS[1:]
FIRST = 5
SEED_A, SEED_B = 2 ** 32, 2 ** 63 + 12345
BAD = [(-1.0, 0.25, "alpha"), (float("nan"), 0.25, "alpha"), (float("inf"), 0.25, "alpha"),
       (0.05, -0.5, "epsilon"), (0.05, 2.0, "epsilon"), (0.05, float("nan"), "epsilon")]
DENSE = (4, 5, 6, 7)                                              # roots()' nearly full boards: 12, 3, 2 and 1 empty cells
cell = lambda y, x: 15 * y + x
WON = [cell(7, 7), cell(0, 0), cell(7, 8), cell(0, 2), cell(7, 9), cell(0, 4), cell(7, 10), cell(0, 6), cell(7, 11)]      # black has five: the game is over


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dense(stones, seed):
    from test_rave_gpu import _dense_positions
    return _dense_positions(1, stones, stones, seed)[0]


@functools.lru_cache(maxsize=None)
def roots():
    """move lists: the empty board, early synthetic positions, tie-game prefixes with 12, 3, 2 and 1 empty cells, and a game that is over"""
    G.init()
    moves, lens, _ = G.synth_boards(3, 0, first_board=40)
    early = [[int(m) for m in moves[g, :min(int(lens[g]), k)]] for g, k in enumerate((3, 7, 12))]
    return [[]] + early + [_dense(213, 1), _dense(222, 2), _dense(223, 3), _dense(224, 4)] + [list(WON)]


def game_ids(n):
    """ids for set_game_ids: 2^31 and 2^32 - 1 among them; with first_game_id = 5 the second wraps to 4, and 2^31 - 5 lands on bit 31"""
    edge = [0, 2 ** 31, 2 ** 32 - 1, 2 ** 31 - FIRST, 7, 2 ** 32 - FIRST, 2 ** 31 - FIRST - 1, 123456789]
    return np.array([edge[g % len(edge)] for g in range(n)], dtype=np.uint32)


def serial_mix(O, priors, ids, stones, alpha, epsilon, seed):
    """go_noise_mix225 on a copy of every row that has a child; a row without one is left alone (the kernels return before the mixing)"""
    out = np.ascontiguousarray(priors, dtype=np.float32).copy()
    for g in range(len(out)):
        if out[g].any():
            O.lib().go_noise_mix225(out[g].ctypes.data, alpha, epsilon, (FIRST + int(ids[g])) % (1 << 32), int(stones[g]), int(seed))
    return out


# ---------------------------------------------------------------- K6, K6 + RAVE, K8 ----------------------------------------------------------------
TRAD = {"K6": lambda n: G.TraditionalMCTS(n, node_capacity=1 << 12), "K6+RAVE": lambda n: G.TraditionalRAVEMCTS(n, node_capacity=1 << 12),
        "K8": lambda n: G.PoolRAVEMCTS(n, node_capacity=1 << 12, c_puct=2.0, seed=77, first_game_id=FIRST)}


def _trad_handle(kind):
    pos = roots()
    t = TRAD[kind](len(pos))
    t.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
    t.set_positions(pos)
    t.set_game_ids(game_ids(len(pos)))
    return t


@functools.lru_cache(maxsize=None)
def _trad_plain_priors(kind):
    """the root children's priors after the first playout, on a handle no noise entry was ever called on"""
    t = _trad_handle(kind)
    t.run(1)
    priors = t.root_stats()["priors"]
    t.close()
    return priors


@pytest.mark.parametrize("alpha,epsilon", PAIRS)
@pytest.mark.parametrize("kind", sorted(TRAD))
def test_trad_root_noise_is_the_serial_statement(oracle, kind, alpha, epsilon):
    pos = roots()
    n, ids, stones = len(pos), game_ids(len(pos)), [len(p) for p in pos]
    t = _trad_handle(kind)
    t.add_root_noise(alpha, epsilon, seed=SEED_A, first_game_id=FIRST)       # fresh roots, no root node yet: a no-op that returns GMK_OK
    t.run(1)                                                                 # the first playout gives every live root its children
    before = t.root_stats()["priors"]
    np.testing.assert_array_equal(bits(before), bits(_trad_plain_priors(kind)))      # ... and the no-op left nothing behind
    live = before.any(1)
    assert live.tolist() == [True] * (n - 1) + [False]                       # the game that is over has no child
    assert all(0 < (before[g] != 0).sum() <= k for g, k in zip(DENSE, (12, 3, 2, 1)))      # (a policy may give a child the prior 0: it then takes no draw)
    assert (before[DENSE[-1]] != 0).sum() == 1                               # one root child: the root where a zero vector of draws is most likely
    t.add_root_noise(alpha, epsilon, seed=SEED_A, first_game_id=FIRST)
    once = t.root_stats()["priors"]
    want = serial_mix(oracle, before, ids, stones, alpha, epsilon, SEED_A)
    for g in range(n):
        np.testing.assert_array_equal(bits(once[g]), bits(want[g]), "%s root %d (%d stones, id %d)" % (kind, g, stones[g], ids[g]))
    several = (before != 0).sum(1) >= 2                                      # (an only child with the prior 1 and a draw that is not 0 ends at 0.75 + 0.25 * 1)
    assert several.sum() >= 5 and (once[several] != before[several]).any(1).all()      # every root with a choice was mixed
    assert not bits(once[~live]).any()                                       # the root that is over keeps its (empty) priors
    t.add_root_noise(alpha, epsilon, seed=SEED_B, first_game_id=FIRST)       # two calls compose
    twice = t.root_stats()["priors"]
    np.testing.assert_array_equal(bits(twice), bits(serial_mix(oracle, once, ids, stones, alpha, epsilon, SEED_B)))
    assert (twice != once).any()
    t.close()


@pytest.mark.parametrize("kind", sorted(TRAD))
def test_trad_refuses_bad_parameters_and_changes_nothing(kind):
    t = _trad_handle(kind)
    t.run(3)
    before = t.root_stats()
    for alpha, epsilon, which in BAD:
        with pytest.raises(G.GmkError, match="gmk_trad_add_root_noise: %s" % which):
            t.add_root_noise(alpha, epsilon, seed=SEED_A, first_game_id=FIRST)
    import torch
    rec = selfplay._record_tensors(4, torch.device("cuda"))
    for alpha, epsilon, which in BAD:
        for sample in (None, (4, 1)):
            entry = "gmk_trad_selfplay_run" if sample is None else "gmk_trad_selfplay_run_sampled"
            with pytest.raises(G.GmkError, match="%s: %s" % (entry, which)):
                t.selfplay_run(4, FIRST, 5, rec[0].data_ptr(), rec[3].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), reuse_subtree=True, root_noise=(alpha, epsilon),
                               persistent=kind != "K8", sample=sample)
    after = t.root_stats()
    assert sorted(after) == sorted(before)
    for k in before:
        np.testing.assert_array_equal(np.ascontiguousarray(after[k]).view(np.uint8), np.ascontiguousarray(before[k]).view(np.uint8), k)
    t.add_root_noise(0.05, 0.0, seed=SEED_A, first_game_id=FIRST)            # the ends of epsilon's range are inside it
    np.testing.assert_array_equal(bits(t.root_stats()["priors"]), bits(before["priors"]))
    t.add_root_noise(0.05, 1.0, seed=SEED_A, first_game_id=FIRST)
    assert not bits(t.root_stats()["priors"]).any()                          # every prior is masked: P * 0 takes no draw
    t.close()


# ---------------------------------------------------------------- K7 ----------------------------------------------------------------
def _az_roots():
    """K6's roots, and two more for the evaluator's special rows: another empty board and another early position"""
    pos = roots()
    pos = pos + [[], list(pos[2])]
    moves, lens = np.zeros((len(pos), N), np.uint8), np.array([len(p) for p in pos], np.int32)
    for g, p in enumerate(pos):
        moves[g, :len(p)] = p
    return pos, moves, lens


def _az_probs(pos):
    """The evaluator's answer for every root: random probabilities with exact zeros on a fifth of the cells (no child there); children only in the
    cells 192 .. 224 for the second empty board; the smallest normal float on one child of the last root."""
    rng = np.random.RandomState(31)
    n = len(pos)
    probs = rng.uniform(0.001, 1.0, (n, N)).astype(np.float32)
    probs /= probs.sum(1, keepdims=True, dtype=np.float32)
    probs[(np.arange(N)[None, :] * 7 + np.arange(n)[:, None]) % 5 == 0] = 0.0
    for g in DENSE:                                              # the nearly full boards keep a child in every empty cell, but for two of the root with twelve
        free = [c for c in range(N) if c not in pos[g]]
        probs[g, free] = rng.uniform(0.001, 1.0, len(free)).astype(np.float32)
    probs[DENSE[0], [c for c in range(N) if c not in pos[DENSE[0]]][3:5]] = 0.0
    probs[n - 2, :192] = 0.0
    probs[n - 2, 192:] = np.float32(1) / np.float32(33)
    tiny = next(c for c in range(100, N) if c not in pos[n - 1])
    probs[n - 1, tiny] = np.float32(2.0 ** -126)
    return probs, tiny


def _az_handle(probs, moves, lens):
    import torch
    n = len(lens)
    t = G.AlphaZeroMCTS(n, node_capacity=1 << 10, c_puct=5.0)
    t.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
    t.set_roots(G.moves_to_planes(moves, lens), selfplay._last_two(moves, lens))
    t.set_game_ids(game_ids(n))
    d_probs = torch.from_numpy(probs).cuda()
    return t, lambda states: (torch.zeros(n, device="cuda"), d_probs)


@pytest.mark.parametrize("alpha,epsilon", PAIRS)
def test_az_root_noise_is_the_serial_statement(oracle, alpha, epsilon):
    pos, moves, lens = _az_roots()
    n, ids = len(pos), game_ids(len(pos))
    probs, tiny = _az_probs(pos)
    t, evaluator = _az_handle(probs, moves, lens)
    t.add_root_noise(alpha, epsilon, seed=SEED_A, first_game_id=FIRST)       # before the first playout no root has children: a no-op that returns GMK_OK
    t.search(evaluator, 1)
    st = t.root_stats()
    before = st["priors"]
    over = np.arange(n) == 8                                                 # the finished game: its root is terminal, the playout ends there and expands nothing
    assert (st["status"] == 0).all() and st["n_nodes"][8] == 1 and (st["n_nodes"][~over] > 1).all()
    empty = np.ones((n, N), bool)
    for g, p in enumerate(pos):
        empty[g, p] = False
    want_before = np.where(empty & ~over[:, None], probs, np.float32(0))     # Default::Expand: the evaluator's probability, verbatim, on every empty cell where it is not 0
    np.testing.assert_array_equal(bits(before), bits(want_before))
    assert (before[n - 2] != 0).nonzero()[0].tolist() == list(range(192, 225)) and before[n - 1, tiny] == np.float32(2.0 ** -126)
    assert [int((before[g] != 0).sum()) for g in DENSE] == [10, 3, 2, 1]
    roomy = [g for g in range(n) if g not in DENSE and not over[g]]
    assert ((before == 0) & empty)[roomy].any(1).all()                       # every other live root has empty cells without a child
    t.add_root_noise(alpha, epsilon, seed=SEED_A, first_game_id=FIRST)
    once = t.root_stats()["priors"]
    want = serial_mix(oracle, before, ids, lens, alpha, epsilon, SEED_A)
    for g in range(n):
        np.testing.assert_array_equal(bits(once[g]), bits(want[g]), "K7 root %d (%d stones, id %d)" % (g, lens[g], ids[g]))
    assert (once[~over] != before[~over]).any(1).all() and not bits(once[over]).any()
    assert once[n - 1, tiny] > 0
    t.add_root_noise(alpha, epsilon, seed=SEED_B, first_game_id=FIRST)       # two calls compose
    twice = t.root_stats()["priors"]
    np.testing.assert_array_equal(bits(twice), bits(serial_mix(oracle, once, ids, lens, alpha, epsilon, SEED_B)))
    assert (twice != once).any()
    t.close()


def test_az_refuses_bad_parameters_and_changes_nothing():
    pos, moves, lens = _az_roots()
    t, evaluator = _az_handle(_az_probs(pos)[0], moves, lens)
    t.search(evaluator, 3)
    before = t.root_stats()
    for alpha, epsilon, which in BAD:
        with pytest.raises(G.GmkError, match="gmk_az_add_root_noise: %s" % which):
            t.add_root_noise(alpha, epsilon, seed=SEED_A, first_game_id=FIRST)
    after = t.root_stats()
    for k in before:
        np.testing.assert_array_equal(np.ascontiguousarray(after[k]).view(np.uint8), np.ascontiguousarray(before[k]).view(np.uint8), k)
    t.close()


# ---------------------------------------------------------------- K3 ----------------------------------------------------------------
def _k3(n=4):
    moves, lens = selfplay._opening(n, 9, 300, 4)
    t = G.BatchedMCTS(n, playouts_capacity=64, seed=9)
    t.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
    t.set_roots(G.moves_to_planes(moves, lens), selfplay._last_two(moves, lens)[:, 0], 300)
    return t


def test_k3_refuses_bad_parameters_and_changes_nothing():
    import torch
    t, twin = _k3(), _k3()
    t.run(20); twin.run(20)
    before = t.root_stats()
    for alpha, epsilon, which in BAD:
        with pytest.raises(G.GmkError, match="gmk_mcts_add_root_noise: %s" % which):
            t.add_root_noise(alpha, epsilon)
    rec = selfplay._record_tensors(4, torch.device("cuda"))
    for alpha, epsilon, which in BAD:
        for sample in (None, (4, 1)):
            entry = "gmk_selfplay_run" if sample is None else "gmk_selfplay_run_sampled"
            with pytest.raises(G.GmkError, match="%s: %s" % (entry, which)):
                t.selfplay_run(4, 300, 5, rec[0].data_ptr(), rec[3].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), reuse_subtree=True, root_noise=(alpha, epsilon), sample=sample)
    for a, b in zip(t.root_stats(), before):
        np.testing.assert_array_equal(a, b)
    t.run(20); twin.run(20)                                                  # no refused call left a noise flag or a prior behind: the searches go on alike
    for a, b in zip(t.root_stats(), twin.root_stats()):
        np.testing.assert_array_equal(a, b)
    assert not any(bool(x.any()) for x in rec)                               # and no record buffer was touched
    t.close(); twin.close()


def test_alpha_zero_still_means_no_noise():
    """noise_alpha == 0: no noise, epsilon ignored (even a NaN): the games of root_noise=None"""
    kw = dict(seed=5, first_game_id=40, opening_plies=3, reuse_subtree=True, slots=2)
    plain = selfplay.play_games(3, 10, root_noise=None, **kw).cpu()
    zero = selfplay.play_games(3, 10, root_noise=(0.0, float("nan")), **kw).cpu()
    assert (plain.moves == zero.moves).all() and (plain.lens == zero.lens).all() and (plain.visits == zero.visits).all()


@pytest.mark.parametrize("noise", NEW_PAIRS)
def test_k3_reference_semantics_in_one_launch(oracle, noise):
    """tests/test_selfplay_gpu.py::test_reference_semantics_in_one_launch at the other pairs: the persistent launch (root_noise_one) == the lock-step
    loop (mcts_root_noise_kernel) == the oracle's kept-tree game loop with sampler 1, through the game records."""
    from test_selfplay_gpu import _oracle_game_reuse
    n, playouts, seed, first, plies = 6, 30, 4242, 700, 3
    kw = dict(seed=seed, first_game_id=first, opening_plies=plies, reuse_subtree=True, root_noise=noise, slots=4)
    one = selfplay.play_games(n, playouts, **kw).cpu()
    step = selfplay.play_games(n, playouts, lockstep=True, **kw).cpu()
    assert not one.overflow and not step.overflow
    assert (one.lens == step.lens).all() and (one.winner == step.winner).all() and (one.moves == step.moves).all() and (one.visits == step.visits).all()
    m, l, _ = G.synth_boards(n, 0, seed=seed, first_board=first)
    for g in range(n):
        opening = [int(x) for x in m[g, :min(int(l[g]), plies)]]
        moves, visits, winner = _oracle_game_reuse(oracle, first + g, playouts, seed, noise=noise, sampler=1, opening=opening)
        assert [int(x) for x in one.moves[g, :int(one.lens[g])]] == moves, "game %d" % g
        assert int(one.winner[g]) == winner
        for ply, v in enumerate(visits):
            assert (one.visits[g, len(opening) + ply].numpy().astype(np.uint32) == np.minimum(v, 65535)).all(), "game %d move %d" % (g, ply)
    plain = selfplay.play_games(n, playouts, **dict(kw, root_noise=None)).cpu()
    assert not (plain.moves == one.moves).all()                              # the noise does change the games


# ---------------------------------------------------------------- K6, K6 + RAVE and K8 self-play loops ----------------------------------------------------------------
def _same(a, b):
    return (a.lens == b.lens).all() and (a.winner == b.winner).all() and (a.moves == b.moves).all() and (a.visits == b.visits).all()


@pytest.mark.parametrize("noise", NEW_PAIRS)
@pytest.mark.parametrize("policy", ["traditional", "traditional_rave"])
def test_k6_one_set_of_games_on_every_loop(oracle, policy, noise):
    """persistent (trad_root_noise inside trad_playouts_kernel) == lock step (trad_root_noise_kernel) == the host-driven loop; for K6 also two
    games of the oracle's kept-tree loop with the same sampler."""
    from test_selfplay_gpu import _oracle_supervisor_game
    n, playouts, seed, first = 6, 60, 7, 61
    kw = dict(c_puct=5.0, policy=policy, opening_plies=2, first_game_id=first, seed=seed, reuse_subtree=True, root_noise=noise)
    one = selfplay.play_supervisor_games(n, playouts, slots=4, device_loop="persistent", **kw).cpu()
    assert not one.overflow and int(one.lens.min()) >= 9
    for other in (dict(device_loop="lockstep"), dict(device_loop=False)):
        rec = selfplay.play_supervisor_games(n, playouts, **other, **kw).cpu()
        assert not rec.overflow and _same(one, rec), other
    assert not _same(one, selfplay.play_supervisor_games(n, playouts, slots=4, device_loop="persistent", **dict(kw, root_noise=None)).cpu())
    if policy == "traditional":
        m, l, _ = G.synth_boards(n, 0, seed=seed, first_board=first)
        for g in (0, 5):
            opening = [int(x) for x in m[g, :min(int(l[g]), 2)]]
            moves, visits, winner = _oracle_supervisor_game(oracle, first + g, playouts, seed, opening, noise)
            assert [int(x) for x in one.moves[g, :int(one.lens[g])]] == moves and int(one.winner[g]) == winner, "game %d" % g
            for ply, v in enumerate(visits):
                assert (one.visits[g, len(opening) + ply].numpy().astype(np.uint32) == np.minimum(v, 65535)).all(), "game %d move %d" % (g, ply)


@pytest.mark.parametrize("noise", NEW_PAIRS)
def test_k8_device_loop_plays_the_host_loops_games(noise):
    """K8 has no persistent loop, and selfplay.play_supervisor_games draws its noise on the host: here the handle is told to draw on the device, and
    gmk_trad_selfplay_run's lock-step loop (trad_root_noise_kernel behind the refill kernel's ids) == the host-driven loop (set_game_ids + add_root_noise)."""
    import torch
    n, playouts, seed, first, plies = 6, 40, 9, 21, 2
    dev, stream = selfplay._device(None)

    def tree():
        t = G.PoolRAVEMCTS(n, node_capacity=selfplay._arena_nodes("supervisor", playouts, True), c_puct=2.0, seed=seed, first_game_id=first)
        t.set_option(G.OPT_NOISE_SAMPLER, COUNTER)
        return t
    t = tree()
    rec = selfplay._record_tensors(n, dev)
    open_moves, open_lens = selfplay._opening(n, seed, first, plies)
    torch.cuda.synchronize()
    _, overflow = t.selfplay_run(n, first, playouts, rec[0].data_ptr(), rec[3].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), open_moves, open_lens,
                                 reuse_subtree=True, root_noise=noise, seed=seed, stream=stream)
    torch.cuda.synchronize()
    t.close()
    t = tree()
    games = selfplay._HostGames.opened(n, seed, first, plies)
    visits, host_overflow = selfplay._supervisor_host_loop(t, games, n, N, playouts, True, noise, seed, first, stream)
    t.close()
    assert not overflow and not host_overflow and int(games.lens.min()) >= 9
    np.testing.assert_array_equal(rec[1].cpu().numpy(), games.lens)
    np.testing.assert_array_equal(rec[0].cpu().numpy(), games.moves)
    np.testing.assert_array_equal(rec[2].cpu().numpy(), games.winner)
    np.testing.assert_array_equal(rec[3].cpu().numpy().view(np.uint16), visits)

