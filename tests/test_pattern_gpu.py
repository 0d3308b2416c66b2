"""K10 parity: the pattern policy on the device (gmk_pattern_policy, gmk_pattern_play; Heuristic.hpp:16-45, 61-83, 94-161) against the CPU
oracle.  filter=1 is held to oracle.trad_heuristic (go_trad.c: TraditionalPolicy::hybridSimulate), filter=0 and the whole-game loop to the
Python restatement of the same float order (tests/trad_rave_reference.py) fed from oracle.Evaluator.  Both sides add in one fixed order and
K6 already meets the oracle bit for bit with this code, so everything is compared on BITS: no tolerances.
The kernels against an independent float64 statement of the formula, within a derived bound: tests/test_heuristic_f64_gpu.py."""
import functools

import numpy as np
import pytest

from gomokuai_amd import lib as G

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 225
OVER, EVAL_ERROR, ILLEGAL, STALLED = 1, 2, 4, 8


@pytest.fixture(scope="module")
def gmk():
    G.init()
    return G


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------- the CPU side ----------------
def _reference(ev, filt):
    """(probs, value) for the player to move on a live oracle evaluator, in go_trad.c's float order"""
    import trad_rave_reference as R
    b = ev.board
    cur, nrec = int(b.cur_player), int(b.nrec)
    scores, density = ev.scores(), ev.density()
    probs = R.evaluation_probs(scores, density, nrec, cur)
    if filt:
        probs = R.decisive_filter(ev.pattern_dist(), ev.compound_dist(), cur, probs)
    return np.asarray(probs, F32), F32(R.evaluation_value(scores, density, cur))


def _replay(O, moves):
    """an oracle evaluator after `moves`; (evaluator, any evaluator error)"""
    ev = O.Evaluator()
    bad = 0
    for m in moves:
        bad |= ev.apply(int(m))[1]
    return ev, bad


@functools.lru_cache(maxsize=None)
def _policy_inputs():
    """2 048 boards each of the two synthetic kinds, every one cut at a random prefix: lengths 0 .. 60"""
    rng = np.random.RandomState(2024)
    moves = np.zeros((4096, N), np.uint8)
    lens = np.zeros(4096, np.int32)
    for kind in (0, 1):
        m, l, _ = G.synth_boards(2048, kind, first_board=7000 + 100000 * kind)
        cut = np.minimum(l, rng.randint(0, 61, size=2048)).astype(np.int32)
        cut[::5] = l[::5]                                       # every fifth board whole: the ones that end on a five are among them
        sl = slice(2048 * kind, 2048 * (kind + 1))
        moves[sl, :m.shape[1]] = m
        lens[sl] = cut
    assert lens.min() == 0 and lens.max() == 60
    return moves, lens


@functools.lru_cache(maxsize=None)
def _policy_reference(filt):
    from oracle import oracle as O
    moves, lens = _policy_inputs()
    n = len(lens)
    probs, value, over = np.zeros((n, N), F32), np.zeros(n, F32), np.zeros(n, bool)
    for g in range(n):
        ml = moves[g, :lens[g]]
        ev, bad = _replay(O, ml)
        assert not bad
        over[g] = ev.check_end()
        if filt:
            p, v = O.trad_heuristic(ml)                         # the C oracle for the filtered form
            probs[g], value[g] = p, v
            if g % 16 == 0 and not over[g]:                     # ... and the Python restatement agrees with it
                p2, v2 = _reference(ev, True)
                assert (_bits(p2) == _bits(p)).all() and _bits(v2) == _bits(F32(v))
        elif not over[g]:
            probs[g], value[g] = _reference(ev, False)
    assert over.sum() >= 8 and (~over).sum() >= 3000
    return probs, value, over


def _check_policy(out, filt, rows=slice(None)):
    probs, value, over = _policy_reference(filt)
    probs, value, over = probs[rows], value[rows], over[rows]
    assert (out["status"] == np.where(over, OVER, 0)).all()
    bad = np.nonzero((_bits(out["probs"]) != _bits(probs)).any(axis=1))[0]
    assert len(bad) == 0, "probs differ on %d positions, first %d" % (len(bad), bad[0])
    assert (_bits(out["value"]) == _bits(value)).all()
    assert (out["best"] == np.where(over, -1, np.argmax(probs, axis=1))).all()
    assert not out["probs"][over].any() and (_bits(out["value"][over]) == 0).all()


def _cpu_game(O, opening, filt, max_moves=0):
    """the greedy loop: reference probs, np.argmax, apply, until check_end -> (moves, values f32[225], winner, finished, stalled)"""
    ev, bad = _replay(O, opening)
    assert not bad
    moves, values = [int(m) for m in opening], np.zeros(N, F32)
    finished = stalled = False
    added = 0
    while True:
        if ev.check_end():
            finished = True
            break
        if max_moves and added >= max_moves:
            break
        probs, value = _reference(ev, filt)
        best = int(np.argmax(probs))
        if best in moves:
            stalled = True
            break
        values[len(moves)] = value
        assert not ev.apply(best)[1]
        moves.append(best)
        added += 1
    return moves, values, (int(ev.board.winner) if finished else 0), finished, stalled


def _openings(n, seed):
    rng = np.random.RandomState(seed)
    return [[int(c) for c in rng.permutation(N)[:g % 9]] for g in range(n)]         # 0 .. 8 distinct cells


@functools.lru_cache(maxsize=None)
def _games_reference(filt, n=256):
    from oracle import oracle as O
    opens = _openings(n, 99 + filt)
    games = [_cpu_game(O, op, filt) for op in opens]
    assert not any(g[4] for g in games), "the reference loop stalls on these openings: choose another seed"
    assert all(g[3] for g in games)
    return opens, games


# ---------------- the device side ----------------
def _policy_device(moves, lens, filt):
    """gmk_pattern_policy on device buffers; every output starts from a sentinel, so a row the kernel skipped shows"""
    import torch
    moves, lens = np.ascontiguousarray(moves, np.uint8), np.ascontiguousarray(lens, np.int32)
    n = len(lens)
    dm, dl = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    probs = torch.full((n, N), -7.0, dtype=torch.float32, device="cuda")
    value = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    best = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    G.pattern_policy_device(dm.data_ptr(), moves.shape[1], dl.data_ptr(), n, filt, probs.data_ptr(), value.data_ptr(), best.data_ptr(),
                            status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {"probs": probs.cpu().numpy(), "value": value.cpu().numpy(), "best": best.cpu().numpy(), "status": status.cpu().numpy()}


def _play_device(opens, filt, max_moves=0):
    import torch
    n = len(opens)
    moves, lens = np.zeros((n, N), np.uint8), np.zeros(n, np.int32)
    for g, op in enumerate(opens):
        moves[g, :len(op)] = op
        lens[g] = len(op)
    dm, dl = torch.from_numpy(moves).cuda(), torch.from_numpy(lens).cuda()
    winner = torch.full((n,), -7, dtype=torch.int8, device="cuda")
    values = torch.full((n, N), -7.0, dtype=torch.float32, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    G.pattern_play(dm.data_ptr(), dl.data_ptr(), n, filt, max_moves, winner.data_ptr(), values.data_ptr(), status.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {"moves": dm.cpu().numpy(), "lens": dl.cpu().numpy(), "winner": winner.cpu().numpy(), "values": values.cpu().numpy(),
            "status": status.cpu().numpy()}


def _check_games(got, games):
    n = len(games)
    moves, values = np.zeros((n, N), np.uint8), np.zeros((n, N), F32)
    for g, (ml, vals, _, _, _) in enumerate(games):
        moves[g, :len(ml)] = ml
        values[g] = vals
    assert not (got["status"] & STALLED).any()
    assert (got["status"] == [OVER if g[3] else 0 for g in games]).all()
    assert (got["lens"] == [len(g[0]) for g in games]).all()
    assert got["moves"].tobytes() == moves.tobytes()
    assert (got["winner"] == [g[2] for g in games]).all()
    assert got["values"].tobytes() == values.tobytes()


# ---------------- 1. policy parity ----------------
@pytest.mark.parametrize("filt", [1, 0])
def test_policy_matches_oracle(gmk, oracle, filt):
    moves, lens = _policy_inputs()
    _check_policy(G.pattern_policy(moves, lens, filter=filt), filt)


def test_policy_device_form_writes_every_row(gmk, oracle):
    moves, lens = _policy_inputs()
    _check_policy(_policy_device(moves[:1000, :64], lens[:1000], 1), 1, slice(0, 1000))


# ---------------- 2. edges ----------------
def _lists(cases, stride=N):
    moves, lens = np.zeros((len(cases), stride), np.uint8), np.zeros(len(cases), np.int32)
    for i, c in enumerate(cases):
        moves[i, :len(c)] = c
        lens[i] = len(c)
    return moves, lens


def _tie_order():
    order = []
    for j in range(15):
        y = 2 * j if j <= 7 else 2 * (j - 7) - 1
        order += [y * 15 + i for i in range(15)]
    return order


def test_edge_positions(gmk, oracle):
    pos = lambda x, y: y * 15 + x
    black_five = [pos(3, 3), pos(3, 4), pos(4, 4), pos(3, 5), pos(5, 5), pos(3, 6), pos(6, 6), pos(3, 7), pos(7, 7)]
    white_five = [pos(3, 3), pos(3, 4), pos(4, 4), pos(3, 5), pos(5, 5), pos(3, 6), pos(6, 6), pos(3, 7), pos(8, 8), pos(3, 8)]
    order = _tie_order()
    cases = [[], black_five, white_five, order, order[:224], black_five[:8]]
    moves, lens = _lists(cases)
    for filt in (1, 0):
        out = G.pattern_policy(moves, lens, filter=filt)
        centre = np.zeros(N, F32)
        centre[112] = 1.0
        assert (_bits(out["probs"][0]) == _bits(centre)).all() and out["best"][0] == 112 and _bits(out["value"][0]) == 0 and out["status"][0] == 0
        for g in (1, 2, 3):
            assert out["status"][g] == OVER and not out["probs"][g].any() and _bits(out["value"][g]) == 0 and out["best"][g] == -1
        for g in (4, 5):                                        # one empty cell left; one move before the five
            ev, bad = _replay(oracle, cases[g])
            assert not bad and not ev.check_end()
            p, v = _reference(ev, filt)
            assert out["status"][g] == 0 and (_bits(out["probs"][g]) == _bits(p)).all() and _bits(out["value"][g]) == _bits(v)
            assert out["best"][g] == int(np.argmax(p))


def test_illegal_lists(gmk):
    pos = lambda x, y: y * 15 + x
    black_five = [pos(3, 3), pos(3, 4), pos(4, 4), pos(3, 5), pos(5, 5), pos(3, 6), pos(6, 6), pos(3, 7), pos(7, 7)]
    cases = [[112, 113, 112], black_five + [0], [112, 240], [112, 113], list(range(0, 225))]
    moves, lens = _lists(cases)
    lens[4] = 226                                               # longer than a board (and than the row: nothing beyond it may be read)
    extra = np.array([-1], np.int32)
    moves = np.concatenate([moves, np.zeros((1, N), np.uint8)])
    lens = np.concatenate([lens, extra])
    for filt in (1, 0):
        out = G.pattern_policy(moves, lens, filter=filt)
        for g in (0, 1, 2, 4, 5):
            assert out["status"][g] & ILLEGAL and not out["status"][g] & OVER, g
            assert not out["probs"][g].any() and _bits(out["value"][g]) == 0 and out["best"][g] == -1
        assert out["status"][3] == 0 and out["best"][3] >= 0
    got = _play_device([cases[0], cases[3]], 1, max_moves=1)      # an illegal opening is left as it was given
    assert got["status"][0] == ILLEGAL and got["lens"][0] == 3 and got["winner"][0] == 0 and not got["values"][0].any()
    assert list(got["moves"][0, :3]) == cases[0] and got["status"][1] == 0 and got["lens"][1] == 3


def test_batch_shapes_and_null_outputs(gmk, oracle):
    import ctypes as C
    moves, lens = _policy_inputs()
    empty = G.pattern_policy(np.zeros((0, N), np.uint8), np.zeros(0, np.int32))
    assert empty["probs"].shape == (0, N) and empty["status"].shape == (0,)
    L = G.load()
    assert L.gmk_pattern_policy(None, N, None, 0, 1, None, None, None, None, None) == 0
    assert L.gmk_pattern_play(None, None, 0, 1, 0, None, None, None, None) == 0
    assert L.gmk_pattern_policy(None, N, None, -1, 1, None, None, None, None, None) == -3       # GMK_ERR_ARG
    assert L.gmk_pattern_policy(None, N, None, 3, 1, None, None, None, None, None) == -3
    for n in (1, 13, 100):                                      # 13 and 100: not a multiple of a workgroup's wavefronts
        _check_policy(G.pattern_policy(moves[:n], lens[:n]), 1, slice(0, n))
    # permuting the batch permutes the outputs
    perm = np.random.RandomState(3).permutation(600)
    a, b = G.pattern_policy(moves[:600], lens[:600]), G.pattern_policy(moves[perm], lens[perm])
    for k in ("probs", "value", "best", "status"):
        assert a[k][perm].tobytes() == b[k].tobytes(), k
    # any output may be left out
    m, l = np.ascontiguousarray(moves[:50]), np.ascontiguousarray(lens[:50])
    best = np.full(50, -7, np.int32)
    assert L.gmk_pattern_policy_host(m.ctypes.data, N, l.ctypes.data, 50, 1, None, None, best.ctypes.data, None) == 0
    assert (best == a["best"][:50]).all()
    probs = np.full((50, N), -7, F32)
    assert L.gmk_pattern_policy_host(m.ctypes.data, N, l.ctypes.data, 50, 1, probs.ctypes.data, None, None, None) == 0
    assert probs.tobytes() == a["probs"][:50].tobytes()
    assert L.gmk_pattern_policy_host(m.ctypes.data, N, l.ctypes.data, 50, 1, None, None, None, None) == 0
    import torch
    dm, dl = torch.zeros((9, N), dtype=torch.uint8, device="cuda"), torch.zeros(9, dtype=torch.int32, device="cuda")
    G.pattern_play(dm.data_ptr(), dl.data_ptr(), 9, 1, 3)       # no winner, values or status asked for
    torch.cuda.synchronize()
    assert (dl.cpu().numpy() == 3).all()


# ---------------- 3. whole games ----------------
@pytest.mark.parametrize("filt", [1, 0])
def test_whole_games_match_the_cpu_loop(gmk, oracle, filt):
    opens, games = _games_reference(filt)
    _check_games(_play_device(opens, filt), games)
    lens = np.array([len(g[0]) for g in games])
    assert lens.min() >= 9 and lens.max() <= N


@pytest.mark.parametrize("filt", [1, 0])
def test_move_limit(gmk, oracle, filt):
    opens, games = _games_reference(filt)
    opens, games = opens[:64], games[:64]
    assert all(len(g[0]) - len(op) > 5 for op, g in zip(opens, games))      # nobody's game is over within five plies
    got = _play_device(opens, filt, max_moves=5)
    assert not got["status"].any() and not got["winner"].any()
    for g, (op, ref) in enumerate(zip(opens, games)):
        k = len(op) + 5
        assert got["lens"][g] == k and list(got["moves"][g, :k]) == ref[0][:k] and not got["moves"][g, k:].any()
        assert _bits(got["values"][g, :k]).tobytes() == _bits(ref[1][:k]).tobytes() and not got["values"][g, k:].any()


# ---------------- 4. consistency of the two entries ----------------
@pytest.mark.parametrize("filt", [1, 0])
def test_policy_on_every_prefix_of_played_games(gmk, filt):
    got = _play_device(_openings(32, 17), filt)
    assert not (got["status"] & ~OVER).any()
    rows, cuts, game = [], [], []
    for g in range(32):
        for k in range(g % 9, int(got["lens"][g]) + 1):
            rows.append(got["moves"][g])
            cuts.append(k)
            game.append(g)
    out = _policy_device(np.stack(rows), np.array(cuts, np.int32), filt)
    for i, (g, k) in enumerate(zip(game, cuts)):
        if k == got["lens"][g]:
            assert out["status"][i] == (got["status"][g] & OVER) == OVER and out["best"][i] == -1
        else:
            assert out["status"][i] == 0 and out["best"][i] == got["moves"][g, k], (g, k)
            assert _bits(out["value"][i]) == _bits(got["values"][g, k]), (g, k)


# ---------------- 5. play_pattern_games ----------------
def test_play_pattern_games_by_global_id(gmk, oracle):
    import torch
    from gomokuai_amd import selfplay
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a, va = selfplay.play_pattern_games(64, first_game_id=0)
        b, vb = selfplay.play_pattern_games(16, first_game_id=32)
        c, vc = selfplay.play_pattern_games(8, first_game_id=32, filter=False, max_moves=6)
    side.synchronize()
    assert a.visits is None and a.first_game_id == 0 and b.first_game_id == 32 and len(a) == 64
    sa, sb = a.status.cpu().numpy(), b.status.cpu().numpy()
    a, b, c = a.cpu(), b.cpu(), c.cpu()
    assert not (sa & (EVAL_ERROR | ILLEGAL)).any()
    for x, y in ((a.moves[32:48], b.moves), (a.lens[32:48], b.lens), (a.winner[32:48], b.winner), (va.cpu()[32:48], vb.cpu()), (sa[32:48], sb)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert (c.lens.numpy() == 4 + 6).all() and not c.winner.numpy().any()
    # one of them against the CPU loop, from its opening
    g = 40
    ref = _cpu_game(oracle, [int(m) for m in a.moves[g, :4]], 1)
    if not ref[4]:
        assert [int(m) for m in a.moves[g, :int(a.lens[g])]] == ref[0] and int(a.winner[g]) == ref[2] and sa[g] == OVER
        assert _bits(va.cpu().numpy()[g]).tobytes() == _bits(ref[1]).tobytes()
    else:
        assert sa[g] & STALLED


# ---------------- 6. pool poison ----------------
def test_on_poisoned_pool_blocks(gmk, oracle):
    """The host form's device block goes through the library's pool once it is large enough (>= 16 MB): five copies of the parity batch make
    it so; the first call leaves the block to the pool, the second gets it back filled with 0xA5 and must read nothing it has not written."""
    moves, lens = _policy_inputs()
    big_m, big_l = np.tile(moves, (5, 1)), np.tile(lens, 5)
    G.release_pool()
    G.pool_poison(True)
    try:
        for _ in range(2):
            out = G.pattern_policy(big_m, big_l, filter=1)
        for r in range(5):
            _check_policy({k: v[4096 * r:4096 * (r + 1)] for k, v in out.items()}, 1)
        opens, games = _games_reference(1)
        _check_games(_play_device(opens, 1), games)
    finally:
        G.pool_poison(False)
        G.release_pool()
