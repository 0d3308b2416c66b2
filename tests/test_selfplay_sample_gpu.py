"""K20 in the self-play loops of K3, K6, K6 + RAVE and K8 (gmk_mcts_advance_sampled, gmk_selfplay_run_sampled, gmk_trad_selfplay_run_sampled,
gmk_trad_root_choice_sampled: the sampled instantiations of mcts_advance_kernel, mcts_playouts_kernel, trad_advance_kernel,
trad_playouts_kernel and trad_root_choice_kernel) against tests/move_sample_reference.py, the restatement tests/test_move_sample.py holds the
host form to, and against each other: one set of games on every loop.  Everything is compared exactly.
Greedy plies keep each search's own choice: K3 the first maximum in cell order, K6 / K8 (one step kernel, trad_advance_kernel, and one
choice, most_visited_child of trad_tree.h) the most visited child that is first in the CURRENT child order -- of a row, that is a maximum.
The 65 535 saturation of the weights is not reachable at test size; tests/test_move_sample.py covers it in the shared header."""
import ctypes as C
import functools

import numpy as np
import pytest

import move_sample_reference as M
from gomokuai_amd import lib as G
from gomokuai_amd import selfplay

pytestmark = pytest.mark.gpu

N = 225
ERR_ARG = -3
POLICIES = {"K6": dict(policy="traditional", c_puct=5.0), "K6+RAVE": dict(policy="traditional_rave", c_puct=5.0), "K8": dict(policy="poolrave", c_puct=2.0)}
TREES = {"K6": lambda n: G.TraditionalMCTS(n, node_capacity=1 << 15), "K6+RAVE": lambda n: G.TraditionalRAVEMCTS(n, node_capacity=1 << 15)}


def _openings(n=12, first_board=300):
    """n openings of 0 .. 8 plies (game g: g % 9), so that one batch lies on both sides of a cut at five stones"""
    moves, lens, _ = G.synth_boards(n, 0, first_board=first_board)
    lens = np.array([min(int(lens[g]), g % 9) for g in range(n)], dtype=np.int32)
    out = np.zeros((n, N), dtype=np.uint8)
    for g in range(n):
        out[g, :lens[g]] = moves[g, :lens[g]]
    return out, lens


def _want(row, stones, game_id, S, power, seed):
    """the cell a sampled ply must play from its row by cell, None where the search's own greedy choice is played"""
    row = np.asarray(row).astype(np.uint32)
    return M.choose(row, int(stones), int(game_id), S, power, seed) if stones < S and row.any() else None


def _same(a, b):
    return (a.lens == b.lens).all() and (a.winner == b.winner).all() and (a.moves == b.moves).all() and (a.visits == b.visits).all()


# ---------------- 1. the choice equals the independent restatement ----------------
@pytest.mark.parametrize("seed", [5, 0x9E3779B97F4A7C15])
def test_k3_advance_plays_the_restatements_cell(seed):
    import torch
    moves, lens = _openings()
    n, first, playouts = len(lens), 4000, 40
    last = selfplay._last_two(moves, lens)[:, 0]
    for S in (5, 225):
        for power in (1, 2, 3):
            tree = G.BatchedMCTS(n, playouts_capacity=playouts, seed=seed)
            tree.set_roots(G.moves_to_planes(moves, lens), last, first)
            tree.run(playouts)
            visits = tree.root_stats()[0]
            assert visits.any(1).all()
            rec = [torch.from_numpy(moves).cuda(), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"), torch.from_numpy(lens).cuda(),
                   torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]
            tree.advance(*[t.data_ptr() for t in rec], False, None, sample=(S, power))
            torch.cuda.synchronize()
            tree.close()
            assert rec[2].cpu().tolist() == (lens + 1).tolist() and int(rec[4]) == n
            drawn = 0
            for g in range(n):
                row = rec[1][g, lens[g]].cpu().numpy().view(np.uint16)
                assert (row == np.minimum(visits[g], 65535)).all()
                want = _want(row, lens[g], first + g, S, power, seed)
                drawn += want is not None and want != int(row.argmax())
                assert int(rec[0][g, lens[g]]) == (int(row.argmax()) if want is None else want), (S, power, g)
            assert drawn > 0 and (S == 225 or (lens >= S).sum() >= 4)


@pytest.mark.parametrize("kind", sorted(TREES))
def test_k6_root_choice_plays_the_restatements_cell(kind):
    import torch
    moves, lens = _openings()
    n, first, playouts = len(lens), 4000, 60
    tree = TREES[kind](n)
    tree.set_positions(moves, lens)
    tree.run(playouts)
    st = tree.root_stats()
    assert (st["root_visits"] >= playouts).all() and (st["status"] == 0).all()
    cells, rows = torch.full((n,), -7, dtype=torch.int16, device="cuda"), torch.full((n, N), -7, dtype=torch.int16, device="cuda")
    drawn = 0
    for seed in (5, 0x9E3779B97F4A7C15):
        for S in (5, 225):
            for power in (1, 2, 3):
                for with_rows in (True, False):                  # the row in the caller's memory, or in the kernel's LDS
                    cells.fill_(-7)
                    rows.fill_(-7)
                    tree.root_choice(cells, rows if with_rows else None, sample=(S, power, seed, first))
                    got = cells.cpu().numpy()
                    if with_rows:
                        np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint16), np.minimum(st["visits"], 65535))
                    for g in range(n):
                        want = _want(st["visits"][g], lens[g], first + g, S, power, seed)
                        drawn += want is not None and want != int(st["best"][g])
                        assert int(got[g]) == (int(st["best"][g]) if want is None else want), (seed, S, power, with_rows, g)
    assert drawn > 0
    # the ids of gmk_trad_set_game_ids name the games
    other = (np.arange(n)[::-1] * 3).astype(np.uint32)
    tree.set_game_ids(other)
    tree.root_choice(cells, sample=(225, 1, 5, 17))
    assert cells.cpu().tolist() == [_want(st["visits"][g], lens[g], 17 + int(other[g]), 225, 1, 5) for g in range(n)]
    tree.close()


# ---------------- 2. every move follows from its row ----------------
def _follows(rec, first, S, power, seed, argmax_on_greedy_plies, opening_plies=2):
    moves, visits, lens = rec.moves.numpy(), rec.visits.numpy().view(np.uint16), rec.lens.numpy()
    assert not rec.overflow and int(lens.min()) >= 9
    drawn = 0
    for g in range(len(lens)):
        for t in range(opening_plies, int(lens[g])):
            row = visits[g, t].astype(np.uint32)
            want = _want(row, t, first + g, S, power, seed)
            if want is not None:
                drawn += want != int(row.argmax())
                assert int(moves[g, t]) == want, (g, t)
            elif argmax_on_greedy_plies:
                assert int(moves[g, t]) == int(row.argmax()), (g, t)      # the first maximum
            else:
                assert row[int(moves[g, t])] == row.max(), (g, t)        # a maximum: the first in the current child order, not in cell order
    assert drawn > 0


@pytest.mark.parametrize("power", [1, 2])
def test_k3_every_move_follows_from_its_visit_row(power):
    kw = dict(opening_plies=2, first_game_id=900, seed=77)
    rec = selfplay.play_games(23, 40, sample_plies=8, sample_power=power, **kw).cpu()
    _follows(rec, 900, 8, power, 77, True)
    assert not _same(rec, selfplay.play_games(23, 40, sample_plies=0, **kw).cpu())


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("kind", sorted(POLICIES))
def test_supervisor_every_move_follows_from_its_visit_row(kind, power):
    kw = dict(opening_plies=2, first_game_id=61, seed=7, **POLICIES[kind])
    playouts = 40 if kind == "K8" else 60
    rec = selfplay.play_supervisor_games(11, playouts, sample_plies=8, sample_power=power, **kw).cpu()
    _follows(rec, 61, 8, power, 7, False)
    assert not _same(rec, selfplay.play_supervisor_games(11, playouts, sample_plies=0, **kw).cpu())


# ---------------- 3. one set of games on every loop ----------------
def test_k3_one_set_of_games_on_every_loop():
    kw = dict(opening_plies=2, first_game_id=900, seed=77, reuse_subtree=True, root_noise=(0.05, 0.25), sample_plies=8, sample_power=1)
    one = selfplay.play_games(23, 40, slots=5, **kw).cpu()
    assert not one.overflow and int(one.lens.min()) >= 9
    for other in (dict(slots=23), dict(lockstep=True), dict(slots=None, handles=2)):
        rec = selfplay.play_games(23, 40, **other, **kw).cpu()
        assert not rec.overflow and _same(one, rec), other
    std = selfplay.play_games(23, 40, slots=23, noise_sampler="std", **kw).cpu()       # host-drawn noise (a lock-step loop): other games, the same rule
    _follows(std, 900, 8, 1, 77, True)
    capped = selfplay.play_games(23, 40, max_moves=6, **kw).cpu()                                          # the max_moves lock-step loop
    assert (capped.lens == 8).all() and (capped.moves[:, :8] == one.moves[:, :8]).all() and (capped.visits[:, :8] == one.visits[:, :8]).all()


def test_k6_one_set_of_games_on_every_loop():
    kw = dict(opening_plies=2, first_game_id=61, seed=7, reuse_subtree=True, root_noise=(0.05, 0.25), sample_plies=8, sample_power=1, **POLICIES["K6"])
    one = selfplay.play_supervisor_games(11, 60, slots=4, device_loop="persistent", **kw).cpu()
    assert not one.overflow and int(one.lens.min()) >= 9
    for other in (dict(slots=11, device_loop="persistent"), dict(device_loop="lockstep"), dict(device_loop=False)):
        rec = selfplay.play_supervisor_games(11, 60, **other, **kw).cpu()
        assert not rec.overflow and _same(one, rec), other
    std = selfplay.play_supervisor_games(11, 60, device_loop="lockstep", noise_sampler="std", **kw).cpu()  # host-drawn noise: other games, the same rule
    _follows(std, 61, 8, 1, 7, False)


@pytest.mark.parametrize("kind", ["K6+RAVE", "K8"])
def test_rave_device_loop_plays_the_host_loops_games(kind):
    kw = dict(opening_plies=2, first_game_id=61, seed=7, sample_plies=8, sample_power=2, **POLICIES[kind])
    if kind == "K8":
        dev = selfplay.play_supervisor_games(11, 40, **kw).cpu()
        host = selfplay.play_supervisor_games(11, 40, device_loop=False, **kw).cpu()
    else:
        dev = selfplay.play_supervisor_games(11, 60, slots=4, device_loop="persistent", reuse_subtree=True, root_noise=(0.05, 0.25), **kw).cpu()
        host = selfplay.play_supervisor_games(11, 60, device_loop=False, reuse_subtree=True, root_noise=(0.05, 0.25), **kw).cpu()
    assert not dev.overflow and not host.overflow and int(dev.lens.min()) >= 9 and _same(dev, host)


@functools.lru_cache(maxsize=None)
def _k6_fresh_games():
    kw = dict(opening_plies=2, first_game_id=61, seed=7, reuse_subtree=False, sample_plies=8, sample_power=1, **POLICIES["K6"])
    one = selfplay.play_supervisor_games(11, 60, slots=4, device_loop="persistent", **kw).cpu()
    for other in (dict(device_loop="lockstep"), dict(device_loop=False)):
        assert _same(one, selfplay.play_supervisor_games(11, 60, **other, **kw).cpu()), other
    return one


def test_k6_fresh_roots_on_every_loop():
    one = _k6_fresh_games()
    assert not one.overflow and int(one.lens.min()) >= 9
    _follows(one, 61, 8, 1, 7, False)


# ---------------- the sampled games' searches are the pinned searches ----------------
def test_sampled_games_show_the_oracles_rows(oracle):
    """A strided sample of plies of the fresh-root, noise-free sampled games: each shows the row the oracle's search of that position has"""
    k6 = _k6_fresh_games()
    k3 = selfplay.play_games(23, 40, opening_plies=2, first_game_id=900, seed=77, sample_plies=8, sample_power=1).cpu()
    checked = 0
    for g in range(0, 11, 3):
        for t in range(2, int(k6.lens[g]), 5):
            o = oracle.TraditionalMCTS(5.0)
            o.search([int(m) for m in k6.moves[g, :t]], 60)
            assert (np.minimum(o.root_children()[0], 65535) == k6.visits[g, t].numpy().view(np.uint16)).all(), (g, t)
            checked += 1
    for g in range(0, 23, 6):
        for t in range(2, int(k3.lens[g]), 7):
            b = oracle.new_board()
            for mv in k3.moves[g, :t]:
                oracle.lib().go_board_apply(C.byref(b), int(mv), 1)
            _, _, v = oracle.MCTS(40, 5.0, 5, 77, 900 + g).eval_state(b)
            assert (np.minimum(v, 65535) == k3.visits[g, t].numpy().view(np.uint16)).all(), (g, t)
            checked += 1
    assert checked >= 12


# ---------------- 4. off is off ----------------
def _k3_run(sample, n=23, slots=5, playouts=40):
    import torch
    dev, stream = selfplay._device(None)
    open_moves, open_lens = selfplay._opening(n, 77, 900, 2)
    rec = selfplay._record_tensors(n, dev)
    tree = G.BatchedMCTS(slots, seed=77, node_capacity=3 * playouts * N + 1)
    tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    tree.selfplay_run(n, 900, playouts, rec[0].data_ptr(), rec[3].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), open_moves, open_lens, True, (0.05, 0.25), stream, sample)
    torch.cuda.synchronize()
    tree.close()
    return [t.cpu() for t in rec]


def _k6_run(sample, n=11, slots=4, playouts=60):
    import torch
    dev, stream = selfplay._device(None)
    open_moves, open_lens = selfplay._opening(n, 7, 61, 2)
    rec = selfplay._record_tensors(n, dev)
    tree = G.TraditionalMCTS(slots, node_capacity=3 * playouts * 226 + 1)
    tree.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    torch.cuda.synchronize()
    tree.selfplay_run(n, 61, playouts, rec[0].data_ptr(), rec[3].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), open_moves, open_lens, True, (0.05, 0.25), 7, stream, 0, True, sample)
    torch.cuda.synchronize()
    tree.close()
    return [t.cpu() for t in rec]


@pytest.mark.parametrize("run", [_k3_run, _k6_run], ids=["K3", "K6"])
def test_zero_plies_is_the_unsampled_entry(run):
    old, new, on = run(None), run((0, 3)), run((8, 1))
    assert int(old[1].min()) >= 9
    for a, b in zip(old, new):
        assert (a == b).all()
    assert any((a != b).any() for a, b in zip(old, on))


def test_zero_plies_is_the_unsampled_step_and_choice():
    import torch
    moves, lens = _openings()
    n = len(lens)
    recs = []
    for sample in (None, (0, 2)):
        tree = G.BatchedMCTS(n, playouts_capacity=40, seed=5)
        tree.set_roots(G.moves_to_planes(moves, lens), selfplay._last_two(moves, lens)[:, 0], 4000)
        tree.run(40)
        rec = [torch.from_numpy(moves).cuda(), torch.zeros((n, N, N), dtype=torch.int16, device="cuda"), torch.from_numpy(lens).cuda(),
               torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]
        tree.advance(*[t.data_ptr() for t in rec], False, None, sample=sample)
        torch.cuda.synchronize()
        tree.close()
        recs.append([t.cpu() for t in rec])
    for a, b in zip(*recs):
        assert (a == b).all()
    tree = TREES["K6"](n)
    tree.set_positions(moves, lens)
    tree.run(60)
    out = []
    for sample in (None, (0, 3, 5, 4000)):
        cells, rows = torch.full((n,), -7, dtype=torch.int16, device="cuda"), torch.full((n, N), -7, dtype=torch.int16, device="cuda")
        tree.root_choice(cells, rows, sample=sample)
        out.append((cells.cpu(), rows.cpu()))
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all() and out[0][0].tolist() == tree.root_stats()["best"].tolist()
    tree.close()


# ---------------- 5. misuse ----------------
def test_misuse_is_refused_and_the_handles_go_on():
    import torch
    L = G.load()
    G.init()
    moves, lens = _openings(4)
    k3, k6 = G.BatchedMCTS(4, playouts_capacity=3 * 20, seed=5), G.TraditionalMCTS(4, node_capacity=1 << 14)
    k3.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    k6.set_option(G.OPT_NOISE_SAMPLER, G.NOISE_SAMPLERS["counter"])
    k3.set_roots(G.moves_to_planes(moves, lens), selfplay._last_two(moves, lens)[:, 0], 0)
    k6.set_positions(moves, lens)
    rec = [torch.full((4, N), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((4, N, N), 0x5A5A, dtype=torch.int16, device="cuda"),
           torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), torch.full((4,), 0x5A, dtype=torch.int8, device="cuda"), torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")]
    cells = torch.full((4,), 0x5A5A, dtype=torch.int16, device="cuda")
    before = [t.clone() for t in rec + [cells]]
    stream = torch.cuda.current_stream().cuda_stream
    m, v, l, w, u = [t.data_ptr() for t in rec]
    steps, overflow = C.c_int32(), C.c_int32()
    entries = {
        "gmk_mcts_advance_sampled": lambda S, k, h=k3.h: L.gmk_mcts_advance_sampled(h, m, v, l, w, u, 0, S, k, stream),
        "gmk_selfplay_run_sampled": lambda S, k, h=k3.h: L.gmk_selfplay_run_sampled(h, 4, 0, 20, 1, 0.05, 0.25, S, k, None, 0, None, m, v, l, w, C.byref(steps), stream),
        "gmk_trad_selfplay_run_sampled": lambda S, k, h=k6.h: L.gmk_trad_selfplay_run_sampled(h, 0, 4, 0, 20, 5.0, 7, 1, 0.05, 0.25, S, k, None, 0, None, m, v, l, w, 1, 0,
                                                                                            C.byref(overflow), C.byref(steps), stream),
        "gmk_trad_root_choice_sampled": lambda S, k, h=k6.h: L.gmk_trad_root_choice_sampled(h, cells.data_ptr(), v, S, k, 7, 0, stream),
    }
    for name, entry in entries.items():
        for S, k in ((-1, 1), (226, 1), (6, 0), (6, 4)):
            assert entry(S, k) == ERR_ARG, (name, S, k)
            assert name.encode() in L.gmk_last_error(), (name, L.gmk_last_error())
        assert entry(6, 1, None) == ERR_ARG and name.encode() in L.gmk_last_error(), name      # a NULL handle
    torch.cuda.synchronize()
    for a, b in zip(before, rec + [cells]):
        assert (a == b).all()                                    # no record byte changed
    # the handles play on
    k3.run(20)
    rec[0].copy_(torch.from_numpy(moves)); rec[2].copy_(torch.from_numpy(lens))
    k3.advance(m, v, l, w, u, False, None, sample=(225, 1))
    assert rec[2].cpu().tolist() == (lens + 1).tolist()
    assert k3.selfplay_run(4, 0, 20, m, v, l, w, None, None, True, (0.05, 0.25), stream, (6, 1)) == 1 and int(rec[2].min()) >= 9
    k6.run(30)
    k6.root_choice(cells, sample=(225, 1, 7, 0))
    assert (cells.cpu() >= 0).all()
    assert k6.selfplay_run(4, 0, 20, m, v, l, w, None, None, True, (0.05, 0.25), 7, stream, 0, True, (6, 1)) == (1, False) and int(rec[2].min()) >= 9
    k3.close()
    k6.close()
    for who in (selfplay.play_games, selfplay.play_supervisor_games):
        for bad in (dict(sample_plies=-1), dict(sample_plies=226), dict(sample_plies=6, sample_power=0), dict(sample_plies=6, sample_power=4)):
            with pytest.raises(ValueError):
                who(2, 4, **bad)
